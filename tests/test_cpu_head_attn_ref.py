"""The plain-torch reference of the attention fusion head (tests/head_attn_ref.py) checked without a GPU: it is the
reference module's function (tests/golden/head_attn.npz and oracle.model.chapter_head_attn), its dropout seeds drop
a sensible share of attention row 0, and the LDS arithmetic that places the GPU test's accepted and refused shapes
either side of the 64 KB limit is right."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_attn_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_reference_matches_oracle_and_golden():
    """p = 0: logits, input gradients and every parameter gradient of sum(logits * R) equal the reference module's
    (head_attn.npz) and the oracle's logits, at 1e-5 relative as test_oracle_attn_head_matches_reference asks. The
    two ReLU projections in front of the head run in plain torch; everything in fp64."""
    from oracle import model as om
    from test_cpu_oracle import _head_params
    g = np.load(os.path.join(GOLD, "head_attn.npz"), allow_pickle=False)
    p32 = _head_params(g)
    p = {n[len("fusion_head."):]: t.detach().double().requires_grad_() for n, t in p32.items()}
    lang = torch.from_numpy(g["head_lang"]).double().requires_grad_()
    vis = torch.from_numpy(g["head_vis"]).double().requires_grad_()
    B, T = vis.shape[:2]
    Lout = F.relu(F.linear(lang, p["lang_proj_head.weight"]))
    Vout = F.relu(F.linear(vis.reshape(B * T, -1), p["vision_proj_head.weight"]))
    out = R.head_attn_ref(Vout, Lout, p["head.query.weight"], p["head.query.bias"], p["head.key.weight"],
                          p["head.key.bias"], p["head.value.weight"], p["head.value.bias"], p["head.proj.weight"],
                          p["head.proj.bias"], n_head=4)
    lg = out["logits"]
    with torch.no_grad():
        lg_oracle = om.chapter_head_attn(p32, torch.from_numpy(g["head_lang"]), torch.from_numpy(g["head_vis"]))
    assert np.abs(lg.detach().numpy() - lg_oracle.numpy()).max() < 1e-5
    assert np.abs(lg.detach().numpy() - g["head_logits"]).max() < 1e-5
    assert torch.allclose(out["prob"].sum(1), torch.ones(B, dtype=torch.float64), atol=1e-12)
    (lg * torch.from_numpy(g["head_R"]).double()).sum().backward()
    assert np.abs(lang.grad.numpy() - g["head_dlang"]).max() < 1e-5
    assert np.abs(vis.grad.numpy() - g["head_dvis"]).max() < 1e-5
    keys = [k for k in g.files if k.startswith("head_grad::")]
    assert len(keys) == 10
    for k in keys:
        ref = g[k]
        assert np.abs(p[k.split("::", 1)[1]].grad.numpy() - ref).max() <= 1e-5 * (1 + np.abs(ref).max()), k


def test_reference_intermediates_are_row_zero():
    """The saved blocks the reference returns are those of query row 0: y0 = P V per head, q0 = X[:, 0] Wq^T + bq."""
    shape = (3, 7, 24, 4, 2)
    B, T, hid, nh, O = shape
    inp = R.make_inputs(shape, torch.float32)
    out, _ = R.head_attn_grads(inp, nh, 0.0, 0, False)
    hs = hid // nh
    y0 = torch.einsum("bhj,bjhe->bhe", out["P"], out["V"].view(B, T + 1, nh, hs)).reshape(B, hid)
    assert torch.allclose(y0, out["y0"], atol=1e-12)
    assert torch.allclose(out["P"].sum(-1), torch.ones(B, nh, dtype=torch.float64), atol=1e-12)
    assert torch.equal(out["X"][:, :T].reshape(B * T, hid), inp["Vout"].double())
    assert torch.equal(out["X"][:, T], inp["Lout"].double())


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_dropout_seeds_drop_a_sensible_share(shape):
    """At p = 0.3 each shape's seed drops 10 % to 50 % of the B * nh * T1 elements of attention row 0, and every
    head keeps at least one key in every window (no all-zero context)."""
    B, T, hid, nh, O = shape
    keep = R.row0_keep(B, nh, T + 1, R.P_DROP, R.SEEDS[shape])
    assert keep.shape == (B, nh, T + 1)
    dropped = 1.0 - keep.mean()
    assert 0.10 <= dropped <= 0.50, dropped
    assert keep.any(-1).all()


def test_dropout_reference_scales_kept_and_zeroes_dropped():
    """The reference's dropout acts on row 0 alone: y0 is the context of P * keep / (1 - p); P itself is returned
    before dropout; another seed gives another mask."""
    shape = (2, 8, 96, 3, 5)
    B, T, hid, nh, O = shape
    inp = R.make_inputs(shape, torch.float32)
    seed = R.SEEDS[shape]
    out0, _ = R.head_attn_grads(inp, nh, 0.0, 0, False)
    out, _ = R.head_attn_grads(inp, nh, R.P_DROP, seed, False)
    assert torch.equal(out["P"], out0["P"])
    keep = torch.from_numpy(R.row0_keep(B, nh, T + 1, R.P_DROP, seed)).double()
    y0 = torch.einsum("bhj,bjhe->bhe", out["P"] * keep / (1 - R.P_DROP),
                      out["V"].view(B, T + 1, nh, hid // nh)).reshape(B, hid)
    assert torch.allclose(y0, out["y0"], atol=1e-12)
    assert not torch.equal(out["y0"], out0["y0"])
    assert (R.row0_keep(B, nh, T + 1, R.P_DROP, seed) != R.row0_keep(B, nh, T + 1, R.P_DROP, seed + 1)).any()


def test_lds_arithmetic():
    """The forward's dynamic LDS in bytes, against figures worked out by hand: the accepted shapes sit inside 64 KB
    (two of them are the largest T of their hid), the refused ones are one token beyond, and the backward never
    asks for more than the forward."""
    table = {(1, 1, 8, 1, 1): 264, (3, 7, 24, 4, 2): 2624, (2, 8, 96, 3, 5): 11244, (5, 16, 128, 4, 2): 27408,
             (2, 16, 256, 16, 256): 55360, (2, 19, 256, 4, 2): 63808, (1, 40, 128, 4, 2): 64656}
    assert list(table) == R.SHAPES
    for (B, T, hid, nh, O), want in table.items():
        assert R.fwd_lds_bytes(T, hid, nh) == want <= R.LDS_LIMIT
    refused = {(1, 20, 256, 4, 2): 66896, (1, 41, 128, 4, 2): 66208, (1, 63, 256, 16, 2): 202752}
    assert list(refused) == R.REFUSED_LDS
    for (B, T, hid, nh, O), want in refused.items():
        assert R.fwd_lds_bytes(T, hid, nh) == want > R.LDS_LIMIT
    # one token fewer than the first two refusals is an accepted shape of the GPU test
    assert (2, 19, 256, 4, 2) in R.SHAPES and (1, 40, 128, 4, 2) in R.SHAPES
    assert R.LDS_LIMIT == 65536
    for T in range(1, 64):
        for hid, nh in ((8, 1), (24, 4), (96, 3), (128, 4), (256, 4), (256, 16), (16, 16)):
            assert R.bwd_lds_bytes(T, hid, nh) <= R.fwd_lds_bytes(T, hid, nh)
