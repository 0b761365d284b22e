"""Kernel-level numerics of the BERT support kernels (csrc/bert.hip) against plain fp64 torch on the CPU:
embeddings + LayerNorm (forward, and the deterministic scatter of the backward), LayerNorm(dropout(x) + res) at
p > 0, the masked attention softmax with dropout, and the pooler's tanh backward.

Every reference is built from the same, already storage-rounded, inputs; backwards come from torch.autograd.grad.
The dropout mask is the library's counter hash restated in numpy (tests/dropout_util.py), so the reference drops
exactly the elements the kernels drop. Tolerances are those of tests/test_gpu_kernels.py: max abs error <=
2e-5 x max|ref| for fp32 storage, 2e-2 x max|ref| for bf16 storage; parameter gradients (fp32 accumulators of
already-rounded operands) are held to the fp32 figure whatever the activation storage. Exact statements (a dropped
element is 0, pad columns are 0, untouched rows, two runs agree) are asserted bit for bit.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dropout_util import row_keep, score_keep

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
EPS = 1e-12


def _tol(dtype):
    return 2e-5 if dtype == torch.float32 else 2e-2


def _close(out, ref, dtype, what=""):
    out = out.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    scale = ref.abs().max().item() + 1e-6
    err = (out - ref).abs().max().item()
    print(f"ERRSTAT {what} | {err / (_tol(dtype) * scale):.4f} of bound")
    assert err <= _tol(dtype) * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _name(dtype):
    return "fp32" if dtype == F32 else "bf16"


@pytest.fixture(scope="module")
def K():
    from vcg_hip import ops, _lib
    _lib.call("vcg_init", 0)
    return ops


# ============================================================================ embeddings + LayerNorm
EMB_SHAPES = [(3, 111, 768), (5, 130, 768), (2, 37, 200), (2, 70, 1024), (1, 1, 768)]
VOCAB = 48
PAD = 0
ID_WAVE, ID_CHUNK, ID_ENDS, ID_ONCE = 41, 42, 43, 44  # ids 45..47 never occur
EMB_SEED = 0x5EED00C0FFEE1234  # (high word set: the hash adds seed >> 32)


def _embed_ids(B, L):
    """Token ids that hit the scatter's boundaries on purpose: one id at rows 63 / 64 only (two waves of a chunk), one
    at rows 255 / 256 only (two chunks), one at row 0 and the last row, one id once, a run of pad rows, and every
    other row drawn from 40 ids, so that each of those repeats across waves and chunks."""
    rows = B * L
    ids = np.random.default_rng(1000 + rows).integers(1, 41, size=rows)
    if rows == 1:
        ids[0] = ID_ENDS
        return ids
    ids[rows // 2:min(rows // 2 + 9, rows - 1)] = PAD
    ids[rows // 3] = ID_ONCE
    if rows > 64:
        ids[63] = ids[64] = ID_WAVE
    if rows > 256:
        ids[255] = ids[256] = ID_CHUNK
    ids[0] = ids[-1] = ID_ENDS
    return ids


@functools.lru_cache(maxsize=None)
def _embed_inputs(B, L, H):
    g = torch.Generator().manual_seed(B * 100003 + L * 101 + H)
    ids = torch.from_numpy(_embed_ids(B, L)).long()
    word = torch.randn(VOCAB, H, generator=g) + 0.25
    pos = torch.randn(L, H, generator=g) * 0.5
    typ = torch.randn(2, H, generator=g) * 0.5
    gamma = torch.rand(H, generator=g) + 0.5
    beta = torch.randn(H, generator=g) * 0.1
    dout = torch.randn(B * L, H, generator=g)
    return ids, word, pos, typ, gamma, beta, dout


def _embed_ref(B, L, H, p, pad_idx, dout=None):
    """fp64: dropout(LayerNorm(word[ids] + pos[l] + type[0])) with the numpy mask, its row statistics, and (with
    dout) the five parameter gradients by autograd through F.embedding(padding_idx)."""
    ids, word, pos, typ, gamma, beta, _ = _embed_inputs(B, L, H)
    w, ps, ty, gm, bt = (t.double().requires_grad_() for t in (word, pos, typ, gamma, beta))
    e = F.embedding(ids, w, padding_idx=pad_idx if pad_idx >= 0 else None) + ps.repeat(B, 1) + ty[0]
    y = F.layer_norm(e, (H,), gm, bt, eps=EPS)
    keep = torch.from_numpy(row_keep(EMB_SEED, B * L, H, p))
    out = y * keep / (1.0 - p)
    mean = e.mean(1)
    rstd = (e.var(1, unbiased=False) + EPS).rsqrt()
    grads = torch.autograd.grad(out, (w, ps, ty, gm, bt), dout.double()) if dout is not None else None
    return out.detach(), mean.detach(), rstd.detach(), keep, grads


def _embed_dev(B, L, H):
    return tuple(t.to(DEV) for t in _embed_inputs(B, L, H)[:6])


@pytest.mark.parametrize("out_dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("shape", EMB_SHAPES, ids=str)
def test_embed_ln_fwd(K, shape, p, out_dtype):
    """out / mean / rstd against fp64; at p > 0 the zeros of out are exactly the numpy mask's dropped elements."""
    B, L, H = shape
    ids, word, pos, typ, gamma, beta = _embed_dev(B, L, H)
    ref, mean_ref, rstd_ref, keep, _ = _embed_ref(B, L, H, p, -1)
    out, mean, rstd = K.embed_ln_fwd(ids, word, pos, typ, gamma, beta, B, L, H, EPS, out_dtype, p, EMB_SEED)
    _close(out, ref, out_dtype, f"embed_ln_fwd out {_name(out_dtype)}")
    _close(mean, mean_ref, F32, "embed_ln_fwd mean")
    _close(rstd, rstd_ref, F32, "embed_ln_fwd rstd")
    assert torch.equal(out.cpu() != 0, keep), "kept / dropped positions differ from the numpy mask"
    out2, mean2, rstd2 = K.embed_ln_fwd(ids, word, pos, typ, gamma, beta, B, L, H, EPS, out_dtype, p, EMB_SEED)
    assert torch.equal(out, out2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)


PREFILL = (0.25, -0.5, 0.125, 1.0, 2.0)  # word, pos, type, gamma, beta gradient buffers before the call


def _embed_bwd(K, B, L, H, dout, stats, p, pad_idx, skip=None):
    ids, word, pos, typ, gamma, _ = _embed_dev(B, L, H)
    shapes = ((VOCAB, H), (L, H), (2, H), (H,), (H,))
    bufs = [None if i == skip else torch.full(s, c, device=DEV) for i, (s, c) in enumerate(zip(shapes, PREFILL))]
    K.embed_ln_bwd(dout, ids, word, pos, typ, gamma, stats[0], stats[1], *bufs, B, L, H, p, EMB_SEED, pad_idx)
    return bufs


@pytest.mark.parametrize("pad_idx", [PAD, -1])
@pytest.mark.parametrize("dout_dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("shape", EMB_SHAPES, ids=str)
def test_embed_ln_bwd(K, shape, p, dout_dtype, pad_idx):
    """word / pos / type / gamma / beta gradients against autograd in fp64 (fp32 bound: fp32 accumulators), accumulated
    into prefilled buffers; the pad row and the rows of absent ids keep their bits; a gradient passed as None leaves
    the others bit-identical; two runs agree bit for bit (the scatter is a fixed-order reduction)."""
    B, L, H = shape
    ids_cpu = _embed_inputs(B, L, H)[0]
    dout = _embed_inputs(B, L, H)[6].to(dout_dtype)
    *_, grads = _embed_ref(B, L, H, p, pad_idx, dout)
    ids, word, pos, typ, gamma, beta = _embed_dev(B, L, H)
    _, mean, rstd = K.embed_ln_fwd(ids, word, pos, typ, gamma, beta, B, L, H, EPS, F32, p, EMB_SEED)
    dout = dout.to(DEV)
    full = _embed_bwd(K, B, L, H, dout, (mean, rstd), p, pad_idx)
    names = ("word_grad", "pos_grad", "type_grad", "gamma_grad", "beta_grad")
    for name, buf, c, ref in zip(names, full, PREFILL, grads):
        if name == "type_grad":
            assert torch.equal(buf[1], torch.full_like(buf[1], c)), "token type 1 is never used"
        _close(buf.double() - c, ref, F32, f"embed_ln_bwd {name} (dout {_name(dout_dtype)})")
    untouched = sorted(set(range(VOCAB)) - set(ids_cpu.tolist()) | ({pad_idx} if pad_idx >= 0 else set()))
    assert len(untouched) >= 3
    wg = full[0].cpu()
    assert torch.equal(wg[untouched], torch.full((len(untouched), H), PREFILL[0])), "pad / absent rows were written"
    again = _embed_bwd(K, B, L, H, dout, (mean, rstd), p, pad_idx)
    for name, a, b in zip(names, full, again):
        assert torch.equal(a, b), f"{name} differs between two runs"
    for skip in range(3):
        part = _embed_bwd(K, B, L, H, dout, (mean, rstd), p, pad_idx, skip=skip)
        for i, name in enumerate(names):
            if i != skip:
                assert torch.equal(part[i], full[i]), f"{name} changed with {names[skip]} = None"


def _refused(K, B, L, H, match):
    from vcg_hip._lib import VcgError
    ids = torch.zeros(B * L, dtype=torch.int64, device=DEV)
    word, pos, typ = (torch.zeros(n, H, device=DEV) for n in (VOCAB, L, 2))
    gamma = torch.ones(H, device=DEV)
    mean, rstd = torch.zeros(B * L, device=DEV), torch.ones(B * L, device=DEV)
    dout = torch.ones(B * L, H, device=DEV)
    shapes = ((VOCAB, H), (L, H), (2, H), (H,), (H,))
    bufs = [torch.full(s, c, device=DEV) for s, c in zip(shapes, PREFILL)]
    with pytest.raises(VcgError, match=match):
        K.embed_ln_bwd(dout, ids, word, pos, typ, gamma, mean, rstd, *bufs, B, L, H, 0.0, 0, -1)
    torch.cuda.synchronize()
    for buf, c in zip(bufs, PREFILL):
        assert torch.equal(buf, torch.full_like(buf, c)), "a refused call launched something"


def test_embed_ln_bwd_refuses_wide_hidden(K):
    """H = 1280 > 4 x 256: the word-gradient reduction holds 4 elements per thread; VCG_ERR_INVALID, nothing runs."""
    _refused(K, 1, 2, 1280, r"\(-1\).*hidden size > 1024")


def test_embed_ln_bwd_refuses_long_single_sequence(K):
    """B = 1, L = 1025: 342 row blocks, so the [L][H] per-position sums would overrun the [342][2][H] partial region
    into the rows the position kernel is still reading; VCG_ERR_INVALID, nothing runs."""
    _refused(K, 1, 1025, 8, r"\(-1\).*L > 2 \* row blocks")


# ============================================================================ LayerNorm(dropout(x) + res)
# (rows, H). The backward is row-wise when H % 256 == 0, H <= 1024 and its [min(ceil(rows / 4), 256)][3][H] partials fit
# the block kernel's [row blocks][2][H] (or always, for the fp32 gradient stream): (1, 768) and (1030, 1024) take the
# block backward in the storage dtype, (1030, 1024) walks the wave stride loop in the fp32-stream test, and
# (1153, 256) walks it (1024 waves, 1153 rows) in the storage dtype.
LN_SHAPES = [(1, 768), (2, 768), (3, 256), (37, 768), (1030, 1024), (37, 200), (9, 1280), (1153, 256)]
LN_SEED = 0x0BADC0DE00001357


@functools.lru_cache(maxsize=None)
def _ln_inputs(rows, H, dtype, dout_dtype):
    g = torch.Generator().manual_seed(rows * 7919 + H)
    x = (torch.randn(rows, H, generator=g) + 0.3).to(dtype)
    r = (torch.randn(rows, H, generator=g) + 0.2).to(dtype)
    gamma = torch.rand(H, generator=g) + 0.5
    beta = torch.randn(H, generator=g) * 0.1
    dout = torch.randn(rows, H, generator=g).to(dout_dtype)
    return x, r, gamma, beta, dout


def _ln_ref(x, r, gamma, beta, dout, p, seed, with_res):
    """fp64 LayerNorm(x * keep / (1 - p) + res): out, mean, rstd, keep, (dx, dres, dgamma, dbeta). Without a residual
    dres is the gradient of the LayerNorm's input (what the kernel writes there)."""
    rows, H = x.shape
    keep = torch.from_numpy(row_keep(seed, rows, H, p))
    xd, gd, bd = (t.double().requires_grad_() for t in (x, gamma, beta))
    rd = (r.double() if with_res else torch.zeros(rows, H, dtype=torch.float64)).requires_grad_()
    pre = xd * keep / (1.0 - p) + rd
    y = F.layer_norm(pre, (H,), gd, bd, eps=EPS)
    mean = pre.mean(1)
    rstd = (pre.var(1, unbiased=False) + EPS).rsqrt()
    grads = torch.autograd.grad(y, (xd, rd, gd, bd), dout.double())
    return y.detach(), mean.detach(), rstd.detach(), keep, grads


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", LN_SHAPES, ids=str)
def test_layernorm_dropout_fwd_bwd(K, shape, dtype, p, with_res):
    """The p > 0 branches of the row-wise (H % 256 == 0, H <= 1024) and block kernels, with and without a residual;
    (1, 768) takes the block backward by the workspace rule. dx is exactly 0 where the mask drops; the fused bias
    gradient is the fp64 column sum of the returned dx; want_dx / want_dres = False leave the rest bit-identical."""
    rows, H = shape
    x, r, gamma, beta, dout = _ln_inputs(rows, H, dtype, dtype)
    y, mean_ref, rstd_ref, keep, (dx_ref, dr_ref, dg_ref, db_ref) = _ln_ref(x, r, gamma, beta, dout, p, LN_SEED,
                                                                            with_res)
    xg, gg_, bg_, dg = x.to(DEV), gamma.to(DEV), beta.to(DEV), dout.to(DEV)
    rg = r.to(DEV) if with_res else None
    tag = f"{_name(dtype)}"
    out, mean, rstd = K.ln_fwd(xg, rg, gg_, bg_, rows, H, EPS, p, LN_SEED)
    _close(out, y, dtype, f"ln_fwd out {tag}")
    _close(mean, mean_ref, F32, "ln_fwd mean")
    _close(rstd, rstd_ref, F32, "ln_fwd rstd")

    def run(want_dx=True, want_dres=True, bias=True):
        gg, gb = torch.full((H,), 1.0, device=DEV), torch.full((H,), 2.0, device=DEV)
        gbias = torch.full((H,), 0.5, device=DEV) if bias else None
        dx, dres = K.ln_bwd(dg, xg, rg, gg_, mean, rstd, gg, gb, rows, H, p, LN_SEED, want_dx=want_dx,
                            want_dres=want_dres, bias_grad=gbias)
        return dx, dres, gg, gb, gbias

    dx, dres, gg, gb, gbias = run()
    _close(dx, dx_ref, dtype, f"ln_bwd dx {tag}")
    assert torch.equal(dx.cpu() != 0, keep), "zeros of dx differ from the numpy mask"
    _close(dres, dr_ref, dtype, f"ln_bwd dres {tag}")
    _close(gg.double() - 1.0, dg_ref, F32, f"ln_bwd gamma_grad (x {tag})")
    _close(gb.double() - 2.0, db_ref, F32, f"ln_bwd beta_grad (x {tag})")
    _close(gbias.double() - 0.5, dx.double().sum(0), F32, f"ln_bwd bias_grad (x {tag})")
    _, dres1, gg1, gb1, _ = run(want_dx=False, bias=False)
    assert torch.equal(dres1, dres) and torch.equal(gg1, gg) and torch.equal(gb1, gb), "want_dx = False changed outputs"
    dx2, none2, gg2, gb2, gbias2 = run(want_dres=False)
    assert none2 is None and torch.equal(dx2, dx) and torch.equal(gg2, gg) and torch.equal(gb2, gb)
    assert torch.equal(gbias2, gbias), "want_dres = False changed outputs"


@pytest.mark.parametrize("shape", [s for s in LN_SHAPES if s[1] % 256 == 0 and s[1] <= 1024], ids=str)
def test_layernorm_dropout_fp32_gradient_stream(K, shape):
    """bf16 x / res with an fp32 incoming gradient (VCG_GRAD_F32) at p = 0.1: dres comes back fp32 within 1e-5
    relative Frobenius of fp64 (fp32 rounding only), dx bf16 within the bf16 bound and 0 where dropped."""
    rows, H = shape
    p = 0.1
    x, r, gamma, beta, dout = _ln_inputs(rows, H, BF16, F32)
    _, _, _, keep, (dx_ref, dr_ref, dg_ref, db_ref) = _ln_ref(x, r, gamma, beta, dout, p, LN_SEED, True)
    xg, rg, gmg = x.to(DEV), r.to(DEV), gamma.to(DEV)
    _, mean, rstd = K.ln_fwd(xg, rg, gmg, beta.to(DEV), rows, H, EPS, p, LN_SEED)
    gg, gb, gbias = (torch.zeros(H, device=DEV) for _ in range(3))
    dx, dres = K.ln_bwd(dout.to(DEV), xg, rg, gmg, mean, rstd, gg, gb, rows, H, p, LN_SEED, bias_grad=gbias)
    assert dx.dtype == BF16 and dres.dtype == F32
    e = ((dres.double().cpu() - dr_ref).norm() / dr_ref.norm()).item()
    print(f"ERRSTAT ln_bwd dres (fp32 stream, rel Frobenius) | {e / 1e-5:.4f} of bound")
    assert e < 1e-5, e
    _close(dx, dx_ref, BF16, "ln_bwd dx (fp32 stream)")
    assert torch.equal(dx.cpu() != 0, keep)
    _close(gg, dg_ref, F32, "ln_bwd gamma_grad (fp32 stream)")
    _close(gb, db_ref, F32, "ln_bwd beta_grad (fp32 stream)")
    _close(gbias, dx.double().sum(0), F32, "ln_bwd bias_grad (fp32 stream)")


@pytest.mark.parametrize("H", [768, 200])
def test_dropout_mask_shared_by_ln_and_embed(K, H):
    """The same (seed, p) drops the same element indices row * H + c in vcg_ln_fwd and vcg_embed_ln_fwd, and a
    different seed (low or high word) drops others. With x = 1, no residual, gamma = 1 and beta = 0 a LayerNorm output
    is positive exactly where its input was kept."""
    B, L, p = 1, 37, 0.1
    rows = B * L
    ids, word, pos, typ, gamma, beta = _embed_dev(B, L, H)
    ones, zeros = torch.ones(H, device=DEV), torch.zeros(H, device=DEV)
    x = torch.ones(rows, H, device=DEV)
    masks = []
    for seed in (LN_SEED, LN_SEED + 1, LN_SEED + (1 << 32)):
        out, _, _ = K.ln_fwd(x, None, ones, zeros, rows, H, EPS, p, seed)
        emb, _, _ = K.embed_ln_fwd(ids, word, pos, typ, gamma, beta, B, L, H, EPS, F32, p, seed)
        keep = torch.from_numpy(row_keep(seed, rows, H, p))
        assert torch.equal(out.cpu() > 0, keep), "vcg_ln_fwd's mask differs from the numpy mask"
        assert torch.equal(emb.cpu() != 0, keep), "vcg_embed_ln_fwd's mask differs from the numpy mask"
        masks.append(keep)
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[0], masks[2])


# ============================================================================ attention softmax
# (B, nh, L, Lp, seed): seeds chosen so that the numpy mask's drop rate over the L x L scores is within 0.02 of p = 0.1
# (tests/test_cpu_dropout_mask.py states that condition on the CPU)
SOFTMAX_CASES = [(2, 3, 7, 8, 0x51A0000000200007), (2, 2, 41, 42, 0x51A0000000000029),
                 (1, 2, 128, 128, 0x51A0000000000080), (1, 2, 130, 136, 0x51A0000000000082),
                 (1, 1, 512, 512, 0x51A0000000000200)]
SOFTMAX_P = 0.1
SCALE = 0.125


def softmax_drop_rate(case, p=SOFTMAX_P):
    B, nh, L, Lp, seed = case
    return 1.0 - score_keep(seed, B * nh, L, Lp, p)[..., :L].mean()


def _softmax_mask(B, L, rot):
    """Sequence b is of kind (b + rot) % 3: all keys valid, a valid prefix, every key masked."""
    mask = torch.ones(B, L, dtype=torch.int64)
    for b in range(B):
        kind = (b + rot) % 3
        if kind == 1:
            mask[b, max(1, (2 * L) // 3):] = 0
        elif kind == 2:
            mask[b, :] = 0
    return mask


def _softmax_check(K, case, dtype, p, mask):
    B, nh, L, Lp, seed = case
    Z = B * nh
    g = torch.Generator().manual_seed(L * 31 + Lp)
    S = (torch.randn(Z, L, Lp, generator=g) * 3.0).to(dtype)
    dPd = torch.randn(Z, L, Lp, generator=g).to(dtype)
    S[..., L:] = float("nan")
    dPd[..., L:] = float("nan")
    # fp64 reference: HF's additive finfo(f32).min bias (a fully masked row comes out uniform, 1 / L)
    Sd = S[..., :L].double().requires_grad_()
    bias = torch.zeros(B, L, dtype=torch.float64) if mask is None else \
        (1.0 - mask.double()) * torch.finfo(torch.float32).min
    bias = bias.repeat_interleave(nh, 0)[:, None, :]
    P_ref = torch.softmax(SCALE * Sd + bias, -1)
    keep = torch.from_numpy(score_keep(seed, Z, L, Lp, p)[..., :L])
    Pd_ref = P_ref * keep / (1.0 - p)
    (dS_ref,) = torch.autograd.grad(Pd_ref, Sd, dPd[..., :L].double())
    if mask is not None:
        for b in range(B):
            if not mask[b].any():
                assert torch.equal(P_ref[b * nh:(b + 1) * nh].detach(),
                                   torch.full((nh, L, L), 1.0 / L, dtype=torch.float64))

    Pm, Pd, dS = (torch.full((Z, L, Lp), float("nan"), dtype=dtype, device=DEV) for _ in range(3))
    K.attn_softmax_fwd(S.to(DEV), None if mask is None else mask.to(DEV), Pm, Pd, B, nh, L, Lp, SCALE, p, seed)
    K.attn_softmax_bwd(dPd.to(DEV), Pm, dS, Z, L, Lp, SCALE, p, seed)
    Pm, Pd, dS = Pm.cpu(), Pd.cpu(), dS.cpu()
    tag = _name(dtype)
    for name, t in (("P", Pm), ("Pd", Pd), ("dS", dS)):
        assert torch.isfinite(t).all(), f"{name} is not finite"
        assert torch.equal(t[..., L:], torch.zeros(Z, L, Lp - L, dtype=dtype)), f"{name}: pad columns are not 0"
    _close(Pm[..., :L], P_ref, dtype, f"attn_softmax_fwd P {tag}")
    _close(Pd[..., :L], Pd_ref, dtype, f"attn_softmax_fwd Pd {tag}")
    assert torch.equal(Pd[..., :L] != 0, keep & (Pm[..., :L] != 0)), "zeros of Pd differ from the numpy mask"
    _close(dS[..., :L], dS_ref, dtype, f"attn_softmax_bwd dS {tag}")


@pytest.mark.parametrize("rot", [0, 1, 2])
@pytest.mark.parametrize("p", [0.0, SOFTMAX_P])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=lambda c: str(c[:4]))
def test_attention_softmax(K, case, dtype, p, rot):
    """P, Pd = dropout(P) and dS against fp64 autograd through softmax(scale * S + bias) * keep / (1 - p), with a random
    upstream gradient; odd L (the pair load that straddles L), L > 128 (a second lane element), pad columns that hold
    NaN on the way in and exactly 0 on the way out, all three kinds of sequence in every shape (rot)."""
    if p > 0:
        assert abs(softmax_drop_rate(case, p) - p) < 0.02, "pick another seed: the mask's own drop rate is off"
    _softmax_check(K, case, dtype, p, _softmax_mask(case[0], case[2], rot))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_attention_softmax_no_mask(K, dtype):
    _softmax_check(K, SOFTMAX_CASES[1], dtype, SOFTMAX_P, None)


# ============================================================================ pooler tanh backward
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [1, 767, 8192 * 256 + 5])
def test_tanh_bwd(K, dtype, n):
    """dx = dy * (1 - t^2) from the stored t, with t at +-1 and 0; 8192 x 256 + 5 elements wrap the grid-stride loop."""
    g = torch.Generator().manual_seed(n)
    t = torch.tanh(torch.randn(n, generator=g) * 1.5).to(dtype)
    dy = torch.randn(n, generator=g).to(dtype)
    t[0] = 1.0
    if n > 3:
        t[1], t[2], t[-1] = -1.0, 0.0, -1.0
    dx = K.tanh_bwd(dy.to(DEV), t.to(DEV)).cpu()
    _close(dx, dy.double() * (1.0 - t.double() ** 2), dtype, f"tanh_bwd {_name(dtype)}")
    assert dx[0] == 0
    if n > 3:
        assert dx[1] == 0 and dx[-1] == 0 and dx[2] == dy[2]
