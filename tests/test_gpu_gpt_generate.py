"""GPTHugface.generate and the KV-cached decoder (vcg_hip/gpt_decode.py) against the fp64 oracle tests/gpt_ref.py.

Model: a 2-layer GPT (H = 768, 12 heads, V = 40478, synth.init_params), B = 3, right-padded prompts of 5, 1 and 12
tokens, 20 teacher-forced tokens each (the sequences grow across lengths 8 and 16). ONE pass of gpt_ref.gpt_lm over the
full forced sequences gives the exact logits of every position.

  * the cached path's logits (the prompt's last position, then step_logits of every step) against that oracle: fp32
    mode within 1e-3, bf16 mode within 5e-2 (tests/test_gpu_gpt_model.py's bounds); bf16 also: Frobenius error over all
    compared positions <= 1.5 x that of the native full forward's logits at the same positions (the recompute path);
  * fp32 greedy generation equals the oracle's greedy loop token for token; PROMPT_SEED was picked on the CPU so that the
    oracle's top-1 / top-2 logit margin is >= 1e-2 at every step, which the test asserts (fp32 logits are within 1e-3
    of exact, so no argmax can flip);
  * cached generation equals the recompute path (GPTHugface.use_kv_cache = False: the same window, never cropped) --
    greedy under that margin, and sampled (top_k = 10) on the same uniforms; with block_size = 12 the sequences the
    window does not crop still agree while they fit;
  * token_idx_sample with a prompt of 7, 50 steps (block 50: 44 cached + 6 sliding): 50 ids, x grows by 50 columns,
    identical for one generator seed;
  * generation after an optimizer step reads the new weights;
  * train_lang/test_gpt_hugface.py end to end on a checkpoint pretrain_gpt_lang_model.py wrote (1 layer, 2 epochs).
"""
import os

import numpy as np
import pytest
import torch

from gpt_ref import gpt_hidden, gpt_lm

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, NH = 40478, 12
LENS, STEPS = [5, 1, 12], 20
PROMPT_SEED = 25  # the first seed whose greedy margin (_oracle_greedy) is >= 1e-2: 1.5e-2


def _build(precision, device=None, n_layer=2):
    from vcg_hip.build import build_gpt_model
    from vcg_hip.nn import OpenAIGPTConfig
    return build_gpt_model(seed=123, device=device, precision=precision, dropout=0.0,
                           config=OpenAIGPTConfig(n_layer=n_layer)).eval()


def _prompts(seed=PROMPT_SEED):
    g = torch.Generator().manual_seed(seed)
    L = max(LENS)
    x = torch.zeros(len(LENS), L, dtype=torch.int64)
    mask = torch.zeros(len(LENS), L, dtype=torch.int64)
    for b, n in enumerate(LENS):
        x[b, :n], mask[b, :n] = torch.randint(0, V, (n,), generator=g), 1
    forced = torch.randint(0, V, (len(LENS), STEPS), generator=g)
    return x, mask, forced


def _padded(rows):
    L = max(len(r) for r in rows)
    x = torch.zeros(len(rows), L, dtype=torch.int64)
    mask = torch.zeros(len(rows), L, dtype=torch.int64)
    for b, r in enumerate(rows):
        x[b, :len(r)], mask[b, :len(r)] = torch.tensor(r), 1
    return x, mask


def _oracle_greedy(P, x, mask, steps):
    """The reference loop in fp64 on right-padded rows: (tokens [B, steps], the smallest top-1 / top-2 margin)."""
    rows = [x[b, :int(mask[b].sum())].tolist() for b in range(x.shape[0])]
    out, margin = [[] for _ in rows], float("inf")
    for _ in range(steps):
        xs, ms = _padded(rows)
        h = gpt_hidden(P, xs, ms, NH, prefix="base_model.")
        last = torch.stack([h[b, len(r) - 1] for b, r in enumerate(rows)])
        top = (last @ P["head.weight"].t()).topk(2, dim=-1)
        margin = min(margin, float((top.values[:, 0] - top.values[:, 1]).min()))
        for b, tok in enumerate(top.indices[:, 0].tolist()):
            rows[b].append(tok)
            out[b].append(tok)
    return torch.tensor(out), margin


@pytest.fixture(scope="module")
def oracle():
    """Computed once for the module and only read by the tests."""
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    cpu = _build("fp32")
    P = {n: p.detach().double() for n, p in cpu.named_parameters()}
    x, mask, forced = _prompts()
    full, fmask = _padded([x[b, :n].tolist() + forced[b].tolist() for b, n in enumerate(LENS)])
    with torch.no_grad():
        logits, _ = gpt_lm(P, full, fmask, torch.zeros_like(full), NH)
        greedy, margin = _oracle_greedy(P, x, mask, STEPS)
    # logits the generation draws token g from: position len0 + g - 1
    want = torch.stack([torch.stack([logits[b, n - 1 + g] for g in range(STEPS)]) for b, n in enumerate(LENS)])
    return dict(x=x, mask=mask, forced=forced, full=full, fmask=fmask, want=want, greedy=greedy, margin=margin)


@pytest.fixture(scope="module", autouse=True)
def _init():
    from vcg_hip import _lib
    _lib.call("vcg_init", 0)


def _cached_logits(m, o):
    """[B, STEPS, V]: prefill's logits, then step_logits of every step, teacher-forced"""
    from vcg_hip.gpt_decode import GptDecoder
    dec = GptDecoder(m, 64)
    out = [dec.prefill(o["x"].to(DEV), o["mask"].to(DEV), steps=STEPS, greedy=True, forced=o["forced"].to(DEV)).clone()]
    for t in range(STEPS - 1):
        out.append(dec.step_logits(t))
    torch.cuda.synchronize()
    seq = dec.seq.cpu()
    for b, n in enumerate(LENS):  # the forced tokens are what the token matrix holds
        assert seq[b, :n + STEPS].tolist() == o["full"][b, :n + STEPS].tolist()
    assert torch.equal(dec.chosen.cpu(), torch.stack(out, 1).argmax(-1).cpu())  # the sampler's own choice is returned
    return torch.stack(out, 1).double().cpu()


def test_cached_logits_fp32(oracle):
    got = _cached_logits(_build("fp32", DEV), oracle)
    err = (got - oracle["want"]).abs().amax(dim=(0, 2))
    print("fp32 cached logits, max err per generated token:", " ".join(f"{e:.1e}" for e in err.tolist()))
    assert err.max().item() <= 1e-3


def test_cached_logits_bf16(oracle):
    m = _build("bf16", DEV)
    got = _cached_logits(m, oracle)
    with torch.no_grad():
        full = m(oracle["full"].to(DEV), oracle["fmask"].to(DEV))[0].double().cpu()
    recompute = torch.stack([torch.stack([full[b, n - 1 + g] for g in range(STEPS)]) for b, n in enumerate(LENS)])
    err = (got - oracle["want"]).abs().amax(dim=(0, 2))
    e_c, e_r = (got - oracle["want"]).norm().item(), (recompute - oracle["want"]).norm().item()
    print("bf16 cached logits, max err per generated token:", " ".join(f"{e:.1e}" for e in err.tolist()))
    print(f"bf16 Frobenius error: cached {e_c:.4e}, native full forward {e_r:.4e}, ratio {e_c / e_r:.3f}")
    assert err.max().item() <= 5e-2
    assert e_c <= 1.5 * e_r


def test_greedy_generation_fp32_equals_oracle_and_recompute(oracle):
    from model.lang.gpt_hugface import GPTHugface
    print(f"oracle top-1 / top-2 margin over {STEPS} steps: {oracle['margin']:.4f}")
    assert oracle["margin"] >= 1e-2
    m = _build("fp32", DEV)
    x, mask = oracle["x"].to(DEV), oracle["mask"].to(DEV)
    seq, new = m.generate(x, mask, steps=STEPS)
    assert torch.equal(new.cpu(), oracle["greedy"])
    for b, n in enumerate(LENS):
        assert seq[b, :n].tolist() == oracle["x"][b, :n].tolist()
        assert seq[b, n:n + STEPS].tolist() == oracle["greedy"][b].tolist()
    GPTHugface.use_kv_cache = False
    try:
        seq_r, new_r = m.generate(x, mask, steps=STEPS)
    finally:
        GPTHugface.use_kv_cache = True
    assert torch.equal(new_r, new) and torch.equal(seq_r, seq)


def test_sampled_generation_cached_equals_recompute(oracle):
    from model.lang.gpt_hugface import GPTHugface
    m = _build("fp32", DEV)
    x, mask = oracle["x"].to(DEV), oracle["mask"].to(DEV)
    kw = dict(steps=STEPS, temperature=0.9, sample=True, top_k=10)
    seq, new = m.generate(x, mask, generator=torch.Generator().manual_seed(5), **kw)
    GPTHugface.use_kv_cache = False
    try:
        seq_r, new_r = m.generate(x, mask, generator=torch.Generator().manual_seed(5), **kw)
    finally:
        GPTHugface.use_kv_cache = True
    assert torch.equal(new_r, new) and torch.equal(seq_r, seq)
    assert not torch.equal(new, m.generate(x, mask, generator=torch.Generator().manual_seed(6), **kw)[1])
    # block 12: token 0 on the cache, the rest on the sliding window; a sequence agrees while its context fits
    _, new_s = m.generate(x, mask, block_size=12, generator=torch.Generator().manual_seed(5), **kw)
    for b, n in enumerate(LENS):
        fits = 12 - n + 1  # tokens drawn from an uncropped context
        assert new_s[b, :fits].tolist() == new[b, :fits].tolist()


def test_token_idx_sample_on_the_model():
    from common_utils import language_model_utils as lmu
    from vcg_hip.gpt_decode import plan_generation
    m = _build("bf16", DEV).train()
    x = torch.randint(0, V, (1, 7), generator=torch.Generator().manual_seed(2)).to(DEV)
    assert plan_generation([7], 50, 50) == (44, 6)
    runs = [lmu.token_idx_sample(m, x, 50, temperature=1.0, sample=True, top_k=10,
                                 generator=torch.Generator().manual_seed(11)) for _ in range(2)]
    out, ids = runs[0]
    assert not m.training
    assert len(ids) == 50 and all(isinstance(i, int) and 0 <= i < V for i in ids)
    assert out.shape == (1, 57) and out[0, :7].tolist() == x[0].tolist() and out[0, 7:].tolist() == ids
    assert runs[1][1] == ids and torch.equal(runs[1][0], out)


def test_generation_follows_an_optimizer_step(oracle):
    from train_lang.pretrain_gpt_lang_model import TrainerConfig
    from vcg_hip.gpt_decode import GptDecoder
    m = _build("bf16", DEV)
    x, mask, forced = (oracle[k].to(DEV) for k in ("x", "mask", "forced"))

    def two(dec):
        a = dec.prefill(x, mask, steps=3, greedy=True, forced=forced[:, :3]).clone()
        return a, dec.step_logits(0)

    dec = GptDecoder(m, 32)
    before = two(dec)
    m.train()
    opt = m.configure_optimizers(TrainerConfig(learning_rate=1e-3))
    m.zero_grad()
    y = torch.where(oracle["fmask"] > 0, oracle["full"], torch.full_like(oracle["full"], -1)).to(DEV)
    m.lm_loss(oracle["full"].to(DEV), oracle["fmask"].to(DEV), y)[0].backward()
    opt.clip_and_step(1.0)
    after = two(dec)
    fresh = two(GptDecoder(m, 32))
    torch.cuda.synchronize()
    for i in range(2):
        assert not torch.equal(after[i], before[i])
        assert torch.equal(after[i], fresh[i])


def test_generate_refusals():
    m = _build("bf16", DEV, n_layer=1)
    x = torch.zeros(2, 4, dtype=torch.int64, device=DEV)
    for bad in ([[0, 1, 1, 1], [1, 1, 1, 1]], [[1, 0, 1, 0], [1, 1, 1, 1]], [[1, 1, 0, 0], [0, 0, 0, 0]]):
        with pytest.raises(ValueError):
            m.generate(x, torch.tensor(bad, device=DEV), steps=2)
    with pytest.raises(ValueError):
        m.generate(x, None, steps=2, block_size=513)
    from vcg_hip.gpt_decode import GptDecoder
    with pytest.raises(ValueError, match="context"):
        GptDecoder(m, 8).prefill(x, None, steps=6)  # 4 + 6 - 1 > 8


def test_driver_reads_the_checkpoint_back(tmp_path, capsys):
    from train_lang import pretrain_gpt_lang_model as train
    from train_lang import test_gpt_hugface as drv
    ck = tmp_path / "ck"
    common = ["--batch_size", "4", "--videos", "8", "--max_text_len", "16", "--n_layer", "1", "--ckpt_path", str(ck)]
    train.main(["--epoch", "2"] + common)
    res = drv.main(common + ["--batches", "2", "--generate_num", "1"])
    text = capsys.readouterr().out
    assert os.path.basename(res["checkpoint"]).startswith("pretrain_") and res["count"] > 0
    assert 0 <= res["correct"] <= res["count"]
    assert len(res["generated"]) == 2 and all(len(g) == 16 and all(0 <= i < V for i in g) for g in res["generated"])
    assert text.count("Gen: ") == 2 and text.count("GT: ") == 2 and "Generate self-defined sentence" in text
    assert text.count(" * ") == 2
