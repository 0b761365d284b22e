"""Host side of GPT text generation (no GPU): the drop-in top_k_logits against a literal torch statement (ties at the
k-th value included), plan_generation's split into cached and sliding steps, the attention-mask refusals, the fp64
sampler helper (tests/gpt_decode_ref.py) against torch.softmax + cumsum, the plain loop of token_idx_sample on a model
without `generate`, and the Python mirror of the decode descriptor against the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gpt_decode_ref as ref
from common_utils import language_model_utils as lmu
from vcg_hip.gpt_decode import _Desc, _Layer, check_prefix_mask, plan_generation


def _literal_top_k(logits, k):
    v, _ = torch.topk(logits, k)
    out = logits.clone()
    out[out < v[:, [-1]]] = -float("Inf")
    return out


def test_top_k_logits_matches_literal_statement_with_ties():
    g = torch.Generator().manual_seed(0)
    z = torch.randn(5, 37, generator=g)
    z[1, [3, 9, 20]] = z[1].topk(3).values[-1]  # three entries tie at the 3rd-largest value
    for k in (1, 3, 10, 37):
        out = lmu.top_k_logits(z, k)
        assert torch.equal(out, _literal_top_k(z, k))
    assert int(torch.isfinite(lmu.top_k_logits(z, 3)[1]).sum()) > 3  # the ties all stay
    assert torch.equal(z, z.clone())  # (the input is not modified)


def test_plan_generation():
    # prompt 7, 50 steps, block 50: tokens 0..43 see contexts of 7..50 tokens (cached), the last 6 slide
    assert plan_generation([7], 50, 50) == (44, 6)
    # a prompt already at block size: its own forward serves token 0, every later one slides
    assert plan_generation([50], 10, 50) == (1, 9)
    assert plan_generation([51], 10, 50) == (0, 10)
    # unequal lengths: the longest sequence decides
    assert plan_generation([5, 1, 12], 20, 512) == (20, 0)
    assert plan_generation([5, 1, 12], 20, 16) == (5, 15)
    assert plan_generation([3], 4, 512) == (4, 0)
    for bad in ([], [0], [3, 0]):
        with pytest.raises(ValueError):
            plan_generation(bad, 4, 16)


def test_mask_refusals():
    ok = np.array([[1, 1, 1, 0], [1, 0, 0, 0], [1, 1, 1, 1]])
    assert check_prefix_mask(ok).tolist() == [3, 1, 4]
    for bad in ([[0, 1, 1, 1]],            # left padding
                [[1, 0, 1, 0]],            # a hole
                [[1, 1, 0, 0], [0, 0, 0, 0]]):  # an empty row
        with pytest.raises(ValueError):
            check_prefix_mask(np.array(bad))


@pytest.mark.parametrize("top_k", [0, 1, 3, 10])
@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_sampler_helper_against_torch(top_k, temperature):
    g = torch.Generator().manual_seed(top_k * 10 + int(temperature * 10))
    z = torch.randn(4, 29, generator=g, dtype=torch.float64) * 2
    z[2, [4, 11]] = z[2].topk(max(top_k, 1)).values[-1]  # ties at the k-th value
    for b in range(4):
        zt = z[b:b + 1] / temperature
        p = torch.softmax(_literal_top_k(zt, top_k) if top_k else zt, dim=-1)[0]
        cdf = torch.cumsum(p, 0).numpy()
        idx, c = ref.cdf_ref(z[b].numpy(), temperature, top_k)
        assert idx.tolist() == torch.nonzero(p > 0)[:, 0].tolist()
        np.testing.assert_allclose(c, cdf[idx], rtol=0, atol=1e-12)
        us, toks = ref.midpoints(z[b].numpy(), temperature, top_k)
        for u, tok in zip(us, toks):
            assert ref.sample_ref(z[b].numpy(), temperature, top_k, u)[0] == tok == int(np.argmax(cdf > u))
        assert ref.sample_ref(z[b].numpy(), temperature, top_k, 0.0)[0] == idx[0]
        assert ref.greedy_ref(z[b].numpy()) == int(z[b].argmax())
    assert ref.greedy_ref([1.0, 3.0, 3.0, 2.0]) == 1


def test_attention_helper_against_torch():
    g = np.random.default_rng(0)
    q, K, V = g.standard_normal(64), g.standard_normal((9, 64)), g.standard_normal((9, 64))
    w = torch.softmax(torch.from_numpy(K @ q) * 0.125, 0)
    np.testing.assert_allclose(ref.attn_one_query(q, K, V, 0.125), (w[None] @ torch.from_numpy(V))[0].numpy(),
                               rtol=0, atol=1e-13)


class _Bigram(torch.nn.Module):
    """logits of position t depend on token t only: next = (3 token + 1) mod V is the argmax"""

    def __init__(self, V=11):
        super().__init__()
        self.V = V

    def forward(self, x):
        return torch.nn.functional.one_hot((3 * x + 1) % self.V, self.V).float() * 5.0, None


def test_token_idx_sample_plain_loop():
    m = _Bigram().train()
    x = torch.tensor([[2, 5]])
    out, ids = lmu.token_idx_sample(m, x, steps=4)
    want, cur = [], 5
    for _ in range(4):
        cur = (3 * cur + 1) % 11
        want.append(cur)
    assert ids == want and out.tolist() == [[2, 5] + want] and not m.training
    a = lmu.token_idx_sample(m, x, 6, temperature=0.7, sample=True, top_k=3, generator=torch.Generator().manual_seed(1))
    b = lmu.token_idx_sample(m, x, 6, temperature=0.7, sample=True, top_k=3, generator=torch.Generator().manual_seed(1))
    assert a[1] == b[1] and len(a[1]) == 6 and a[0].shape == (1, 8)


def test_descriptor_mirror_matches_header():
    """Every field of vcg_gpt_decode_layer / vcg_gpt_decode_desc, in the header's order."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(here, "include", "vcg_gpt_decode.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)

    def fields(name):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", src, flags=re.S).group(1)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            names = decl.split(",")
            names[0] = names[0].split()[-1]
            out += [re.sub(r"[\*\s]|\[.*\]", "", n) for n in names]
        return out

    assert fields("vcg_gpt_decode_layer") == [f[0] for f in _Layer._fields_]
    assert fields("vcg_gpt_decode_desc") == [f[0] for f in _Desc._fields_]
    assert int(re.search(r"#define VCG_GPT_MAX_LAYERS (\d+)", src).group(1)) == len(_Desc().layers)
    assert ctypes.sizeof(_Layer) == 14 * 8
