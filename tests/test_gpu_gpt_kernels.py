"""The kernels of the generative (GPT) stage against fp64 references (reference: transformers OpenAIGPTModel via
model/lang/gpt_hugface.py:18):

  * causal fused attention (bert_attn.hip L <= 128, bert_attn_long.hip above; VCG_ATTN_CAUSAL) against
    tests/gpt_ref.causal_attention_ref (HF's `w * b + -1e4 (1 - b)` fill and finfo.min padding bias, the library's
    dropout mask) and against the unfused causal chain, by tests/test_gpu_bert_attn.py's criterion: relative Frobenius
    error of ctx / dQ / dK / dV <= 2e-2 and <= 1.25 x the unfused path's + 2e-3. Masks: right padding, a hole (behind a
    valid position 0), one fully masked sequence. L sits inside, on and next to the 16-wide MFMA tile edges (short
    kernels) and the 128-wide tile edges (tiled kernels: a one-row last tile, full length);
  * a LEFT-padded mask (uniform rows in front of normal ones, nothing skipped): fused against the unfused chain;
  * the packed (_varlen) form bit-identical to the padded one on the kept rows;
  * no leak from the future, bitwise: changing Q / K / V rows behind a cut t leaves ctx rows <= t bit-identical, and a
    dctx that is zero behind t gives exactly zero dK / dV there;
  * the tanh-GELU epilogues (wide engine, 128 x 128 engine, fp32 GEMM) by tests/test_gpu_wide.py's shapes and criteria
    with the tanh form in the fp64 reference, plus M = 1;
  * the GPT embedding forward / backward against fp64 with repeated ids, deterministic run to run.
"""
import numpy as np
import pytest
import torch

from bert_attn_ref import rel
from dropout_util import row_keep
from gpt_ref import causal_attention_ref, new_gelu, new_gelu_grad

pytestmark = pytest.mark.gpu
DEV = "cuda"
NH, H = 12, 768


@pytest.fixture(scope="module", autouse=True)
def _init():
    from vcg_hip import _lib
    _lib.call("vcg_init", 0)


def _masks(B, L):
    """right padding; a hole behind a valid position 0 (B = 3); one fully masked sequence"""
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[0, L - L // 3:] = 0
    mask[1, :] = 0
    if B > 2 and L > 4:
        mask[2, 1 + L // 4:1 + L // 2] = 0
    return mask


def _attn_case(B, L, p):
    Lp = (L + 7) // 8 * 8
    g = torch.Generator().manual_seed(B * 1000 + L)
    qkv = (torch.randn(B * L + 8, 3 * H, generator=g) * 1.5).to(torch.bfloat16)
    dctx = torch.randn(B * L, H, generator=g).to(torch.bfloat16)
    return qkv, dctx, _masks(B, L), Lp, 0x1234567890AB + L


def _run(qkv, dctx, mask, B, L, Lp, p, seed, fused, **kw):
    from vcg_hip.bert import attention_bwd, attention_fwd
    qkv, dctx, mask = qkv.to(DEV), dctx.to(DEV), mask.to(DEV)
    ctx, att = attention_fwd(qkv, mask, B, NH, L, Lp, 64, 0.125, p, seed, fused, causal=True, **kw)
    dqkv = attention_bwd(qkv, dctx, ctx, mask, att, B, NH, L, Lp, 64, 0.125, p, seed, causal=True, **kw)
    torch.cuda.synchronize()
    return ctx.cpu(), dqkv.cpu()


SHORT = [(2, 1), (2, 7), (3, 16), (2, 17), (3, 33), (2, 64), (3, 128)]
LONG = [(2, 129), (3, 200), (2, 256), (2, 257), (2, 512)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,L", SHORT + LONG)
def test_causal_attention_matches_fp64_and_unfused(B, L, p):
    qkv, dctx, mask, Lp, seed = _attn_case(B, L, p)
    ref_ctx, ref_dqkv = causal_attention_ref(qkv, mask, dctx, B, NH, L, Lp, p, seed)
    out = {fused: _run(qkv, dctx, mask, B, L, Lp, p, seed, fused) for fused in (True, False)}
    for fused in out:
        assert torch.isfinite(out[fused][0]).all() and torch.isfinite(out[fused][1]).all()
    for name, sl in (("ctx", None), ("dQ", slice(0, H)), ("dK", slice(H, 2 * H)), ("dV", slice(2 * H, 3 * H))):
        f = out[True][0] if sl is None else out[True][1][:, sl]
        u = out[False][0] if sl is None else out[False][1][:, sl]
        r = ref_ctx if sl is None else ref_dqkv[:, sl]
        if not r.any():  # (L = 1: a softmax over one key has no gradient -- dQ and dK are exactly zero)
            assert L == 1 and not f.any() and not u.any(), name
            continue
        ef, eu = rel(f, r), rel(u, r)
        print(f"causal B={B} L={L} p={p} {name}: fused {ef:.3e} unfused {eu:.3e}")
        assert ef <= 2e-2 and ef <= 1.25 * eu + 2e-3, (name, ef, eu)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("L", [40, 128, 300])
def test_left_padded_mask_fused_matches_unfused(L, p):
    """A LEFT-padded mask (leading positions masked, later ones valid): the queries before the first valid key have no
    visible key and attend uniformly to all L keys (the documented divergence from transformers); nothing may be
    skipped for such a sequence. No fp64 statement of HF applies here, so the fused kernels are held to the unfused
    chain, which implements the same convention by other code: both bf16, so by the criterion's 2e-2."""
    B = 3
    Lp = (L + 7) // 8 * 8
    g = torch.Generator().manual_seed(31 + L)
    qkv = (torch.randn(B * L + 8, 3 * H, generator=g) * 1.5).to(torch.bfloat16)
    dctx = torch.randn(B * L, H, generator=g).to(torch.bfloat16)
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[0, :5] = 0                 # uniform rows 0-4, normal rows behind
    mask[1, :L // 2 + 3] = 0        # the first valid key lies past a 16-tile / 128-tile edge
    mask[1, L - 2:] = 0
    mask[2, 0] = 0                  # one uniform row
    seed = 0xFEED + L
    (cf, df), (cu, du) = (_run(qkv, dctx, mask, B, L, Lp, p, seed, fused) for fused in (True, False))
    assert torch.isfinite(cf).all() and torch.isfinite(df).all()
    for name, f, u in (("ctx", cf, cu), ("dQ", df[:, :H], du[:, :H]), ("dK", df[:, H:2 * H], du[:, H:2 * H]),
                       ("dV", df[:, 2 * H:], du[:, 2 * H:])):
        e = rel(f, u)
        print(f"left padding L={L} p={p} {name}: fused vs unfused {e:.3e}")
        assert e <= 2e-2, (name, e)
    # a uniform row without dropout is the mean of all L values
    if p == 0.0:
        v = qkv[:L, 2 * H:2 * H + 64].double()
        assert (cf[0, :64].double() - v.mean(0)).abs().max().item() <= 2e-2 * v.abs().max().item()


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("L", [128, 300])
def test_causal_varlen_matches_padded(L, p):
    """tests/test_gpu_bert_attn.py::test_varlen_attention_matches_padded with the causal flag: prefix sequences packed
    (vcg_bert_attn_fwd/bwd_ex with seq) are bit-identical to the padded form on the kept rows, given the dropped rows'
    upstream gradient is zero."""
    from vcg_hip.bert import Packing
    B = 4
    lens = [L, L * 3 // 5, 1, 50]
    mask_np = np.zeros((B, L), np.int64)
    for b, n in enumerate(lens):
        mask_np[b, :n] = 1
    pk = Packing(mask_np.copy(), DEV)
    rows = pk.rows.cpu()
    assert pk.R == sum(lens)
    g = torch.Generator().manual_seed(5 + L)
    qkv = (torch.randn(B * L + 8, 3 * H, generator=g) * 1.5).to(torch.bfloat16)
    dctx = torch.randn(B * L, H, generator=g).to(torch.bfloat16)
    drop = torch.ones(B * L, dtype=torch.bool)
    drop[rows] = False
    dctx[drop] = 0
    seed = 0xABCDEF + int(p * 10)
    Lp = (L + 7) // 8 * 8
    ctx_p, dqkv_p = _run(qkv, dctx, torch.from_numpy(mask_np), B, L, Lp, p, seed, True)
    qkv_k = torch.cat([qkv[rows], torch.zeros(8, 3 * H, dtype=qkv.dtype)])
    ctx_k, dqkv_k = _run(qkv_k, dctx[rows], pk.keys.cpu(), B, L, Lp, p, seed, True, seq=pk.seq, rows=pk.R)
    assert torch.equal(ctx_k, ctx_p[rows]) and torch.equal(dqkv_k, dqkv_p[rows])


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("L,cuts", [(64, (15, 16, 31, 32)), (300, (127, 128, 143, 255, 256))])
def test_no_leak_from_the_future(L, cuts, p):
    B = 2
    Lp = (L + 7) // 8 * 8
    g = torch.Generator().manual_seed(77 + L)
    qkv = (torch.randn(B * L + 8, 3 * H, generator=g) * 1.5).to(torch.bfloat16)
    other = (torch.randn(B * L + 8, 3 * H, generator=g) * 1.5).to(torch.bfloat16)
    dctx = torch.randn(B * L, H, generator=g).to(torch.bfloat16)
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[1, L - 5:] = 0
    seed = 0x5EED + L
    ctx0, _ = _run(qkv, dctx, mask, B, L, Lp, p, seed, True)
    pos = torch.arange(B * L) % L
    for t in cuts:
        after = torch.cat([pos > t, torch.zeros(8, dtype=torch.bool)])
        q2 = qkv.clone()
        q2[after] = other[after]
        d2 = dctx.clone()
        d2[pos > t] = 0
        ctx1, dqkv1 = _run(q2, d2, mask, B, L, Lp, p, seed, True)
        assert torch.equal(ctx1[pos <= t], ctx0[pos <= t]), t
        assert not dqkv1[pos > t][:, H:].any(), t  # dK, dV behind the cut
        assert dqkv1[pos <= t].any()


# ------------------------------------------------------------------------------------------------ tanh GELU
R, I = 8192, 3072
WIDE = 0x200


def _bf(shape, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(torch.bfloat16).to(DEV)


def _rel(a, ref):
    return ((a.double() - ref).norm() / ref.norm()).item()


def _census(fn, prefix):
    from vcg_hip import ops
    ops.gemm_census_enable(True)
    out = fn()
    torch.cuda.synchronize()
    keys = [k for k in ops.gemm_census() if k.startswith(prefix)]
    ops.gemm_census_enable(False)
    return out, keys


@pytest.mark.parametrize("M", [R, 128, 1])
def test_ffn1_gelu_tanh_aux(M):
    """tests/test_gpu_wide.py::test_ffn1_gelu_aux with the tanh form: wide engine (we5), 128 x 128 engine, fp32."""
    from vcg_hip import ops
    gen = torch.Generator().manual_seed(11 + M)
    A, W = _bf((M, H), gen), _bf((I, H), gen, 0.02)
    b = (torch.randn(I, generator=gen) * 0.1).to(DEV)
    pre = torch.empty((M, I), dtype=torch.bfloat16, device=DEV)
    out, keys = _census(lambda: ops.gemm(A, W, M, I, H, H, H, bias=b, act=ops.ACT_GELU_TANH | WIDE, aux=pre),
                        "gemm_wide")
    assert keys and "we5" in keys[0], keys
    ref_pre = A.double() @ W.double().t() + b.double()
    g = new_gelu(ref_pre)
    assert _rel(pre, ref_pre) < 4e-3
    assert _rel(out, g) < 4e-3
    pre_e = torch.empty_like(pre)
    eng = ops.gemm(A, W, M, I, H, H, H, bias=b, act=ops.ACT_GELU_TANH, aux=pre_e)
    err = (out.double() - eng.double()).abs()
    assert (err <= eng.double().abs() * 2.0 ** -7 + 1e-6).all(), err.max().item()
    assert _rel(eng, g) < 4e-3 and _rel(pre_e, ref_pre) < 4e-3
    out2 = ops.gemm(A, W, M, I, H, H, H, bias=b, act=ops.ACT_GELU_TANH | WIDE)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    # fp32 GEMM (tanhf): the fp32 product's error
    Mf = min(M, 128)
    A32, W32 = A[:Mf].float(), W.float()
    pre32 = torch.empty((Mf, I), dtype=torch.float32, device=DEV)
    o32 = ops.gemm(A32, W32, Mf, I, H, H, H, bias=b, act=ops.ACT_GELU_TANH, aux=pre32)
    torch.cuda.synchronize()
    assert _rel(o32, g[:Mf]) < 1e-5 and _rel(pre32, ref_pre[:Mf]) < 1e-5


@pytest.mark.parametrize("M", [R, 128, 1])
def test_ffn2_input_gradient_gelu_tanh_bwd(M):
    """tests/test_gpu_wide.py::test_ffn2_input_gradient_gelu_bwd with the tanh form: wide (we6), 128 x 128 (its own
    staged-epilogue kernel, r3), fp32."""
    from vcg_hip import ops
    gen = torch.Generator().manual_seed(23 + M)
    dY, Wt = _bf((M, H), gen, 0.05), _bf((I, H), gen, 0.02)
    pre = _bf((M, I), gen)
    out, keys = _census(lambda: ops.gemm(dY, Wt, M, I, H, H, H, act=ops.ACT_GELU_TANH_BWD | WIDE, residual=pre, ldr=I),
                        "gemm_wide")
    assert keys and "we6" in keys[0], keys
    eng, keys = _census(lambda: ops.gemm(dY, Wt, M, I, H, H, H, act=ops.ACT_GELU_TANH_BWD, residual=pre, ldr=I),
                        "igemm_fast")
    assert keys and " r3 " in keys[0], keys
    ref = (dY.double() @ Wt.double().t()) * new_gelu_grad(pre.double())
    e_w, e_e = _rel(out, ref), _rel(eng, ref)
    print(f"tanh gelu' M={M}: wide {e_w:.2e} engine {e_e:.2e}")
    assert e_w < 1.5 * e_e + 4e-3
    # the engine's own error: the product rounded to bf16 (2^-9 relative per element), then the stored product
    assert e_e < 6e-3
    Mf = min(M, 128)
    o32 = ops.gemm(dY[:Mf].float(), Wt.float(), Mf, I, H, H, H, act=ops.ACT_GELU_TANH_BWD,
                   residual=pre[:Mf].float().contiguous(), ldr=I)
    torch.cuda.synchronize()
    assert _rel(o32, ref[:Mf]) < 1e-5


# ------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("L", [1, 50])
def test_gpt_embedding(L, p, dtype):
    from vcg_hip import ops
    B, V, NP = 3, 97, 64
    g = torch.Generator().manual_seed(L)
    tok = torch.randn(V, H, generator=g)
    pos = torch.randn(NP, H, generator=g)
    ids = torch.randint(0, V, (B, L), generator=g)
    ids[1] = ids[0]  # repeated ids: the fixed-order accumulation
    if L > 3:
        ids[2, :3] = ids[0, 0]
    seed = 0xC0FFEE + L
    out = ops.gpt_embed_fwd(ids.to(DEV), tok.to(DEV), pos.to(DEV), B, L, H, dtype, p, seed)
    keep = torch.from_numpy(row_keep(seed, B * L, H, p)).double()
    ref = (tok.double()[ids.reshape(-1)] + pos.double()[:L].repeat(B, 1)) * keep / (1.0 - p)
    tol = 1e-6 if dtype == torch.float32 else 2.0 ** -8  # (one rounding of the stored value)
    assert ((out.double().cpu() - ref).abs() <= tol * ref.abs() + 1e-30).all()
    # backward: dout in the forward's dtype, and fp32 beside a bf16 forward (the residual-gradient stream)
    for ddt in {dtype, torch.float32}:
        dout = torch.randn(B * L, H, generator=g).to(ddt)
        d = dout.double() * keep / (1.0 - p)
        ref_tok = torch.zeros(V, H, dtype=torch.float64).index_add_(0, ids.reshape(-1), d)
        ref_pos = torch.zeros(NP, H, dtype=torch.float64)
        ref_pos[:L] = d.view(B, L, H).sum(0)
        res = []
        for _ in range(2):
            gt = torch.zeros(V, H, device=DEV)
            gp = torch.zeros(NP, H, device=DEV)
            ops.gpt_embed_bwd(dout.to(DEV), ids.to(DEV), gt, gp, B, L, H, p, seed, storage_dtype=dtype)
            torch.cuda.synchronize()
            res.append((gt.cpu(), gp.cpu()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        # fp32 sums of at most B L terms
        assert (res[0][0].double() - ref_tok).abs().max().item() <= 1e-5 * max(1.0, ref_tok.abs().max().item())
        assert (res[0][1].double() - ref_pos).abs().max().item() <= 1e-5 * max(1.0, ref_pos.abs().max().item())
        assert not res[0][1][L:].any()
