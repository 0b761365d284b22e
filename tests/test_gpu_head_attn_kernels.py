"""Kernel-level numerics of the attention fusion head (csrc/head_attn.hip: vcg_head_attn_fwd / _bwd, also the window
"self_attn" head with O = hid) against plain fp64 torch on the CPU (tests/head_attn_ref.py), through the C ABI.

Shapes (tests/head_attn_ref.py SHAPES) reach one, two, three and six passes of the kernels' 8-token loops, with
and without a tail; one head and sixteen; O = 1, 5 (> 4 waves) and 256; hid below one wave and at 256; and the two
largest windows the 64 KB LDS limit admits. Every block of `saved` (X, K, V, q0, y0, P) is compared on its own, so
a failure names its stage; gradients come from autograd through the reference, with the library's dropout mask on
attention row 0 at p = 0.3 (tests/dropout_util.py), and are accumulated into buffers prefilled with 0.5.

Bounds, those of tests/test_gpu_head_kernels.py: max abs error <= 2e-5 x max|ref| for everything held in fp32
(logits, prob, saved blocks, parameter gradients, fp32 dVout / dLout), 2e-2 x max|ref| for bf16 dVout / dLout.
dbk is analytically zero (the softmax is shift-invariant): it is bounded by 2e-5 x max_n sum_r |dK_ref[r][n]|, the
size of the terms that cancel. Each comparison also prints the error of the same reference run in torch fp32.
"""
import functools

import pytest
import torch

import head_attn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
PS = [0.0, R.P_DROP]
BLOCKS = ("X", "K", "V", "q0", "y0", "P")  # the order of `saved`, as vcg_head_attn_fwd lays it out
GRADS = ("dWq", "dbq", "dWk", "dbk", "dWv", "dbv", "dWp", "dbp")  # the order of vcg_head_attn_bwd's arguments
FILL = 0.5


def _tol(dtype):
    return 2e-5 if dtype == torch.float32 else 2e-2


def _close(out, ref, dtype, what="", ref32=None, scale=None):
    out = out.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    scale = (ref.abs().max().item() if scale is None else scale) + 1e-6
    err = (out - ref).abs().max().item()
    bound = _tol(dtype) * scale
    f32 = "" if ref32 is None else f" | torch-fp32 {(ref32.double() - ref).abs().max().item() / bound:.4f} of bound"
    print(f"ERRSTAT {what} | {err / bound:.4f} of bound{f32}")
    assert err <= bound, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _name(dtype):
    return "fp32" if dtype == F32 else "bf16"


@pytest.fixture(scope="module")
def K():
    from vcg_hip import ops, _lib
    _lib.call("vcg_init", 0)
    return ops


@functools.lru_cache(maxsize=None)
def _case(shape, dtype, p, relu_mask=False, bias_p=True):
    """Inputs, the fp64 reference (forward, gradients) and its torch-fp32 twin; computed once and shared."""
    inp = R.make_inputs(shape, dtype)
    seed = R.SEEDS[shape] if p > 0 else 0
    ref = R.head_attn_grads(inp, shape[3], p, seed, relu_mask, torch.float64, bias_p)
    r32 = R.head_attn_grads(inp, shape[3], p, seed, relu_mask, torch.float32, bias_p)
    return inp, seed, ref, r32


def _fwd(K, inp, shape, p, seed, prob=True, bias_p=True, logits=None, saved=None):
    """vcg_head_attn_fwd through the C ABI -> logits, prob (None when not asked for), saved."""
    from vcg_hip import _lib
    B, T, hid, nh, O = shape
    dev = {k: v.to(DEV) for k, v in inp.items()}
    n = _lib.query("vcg_head_attn_saved_floats", B, T, hid, nh)
    saved = torch.full((n,), float("nan"), device=DEV) if saved is None else saved
    logits = torch.full((B, O), float("nan"), device=DEV) if logits is None else logits
    pr = torch.full((B, O), float("nan"), device=DEV) if prob else None
    _lib.call("vcg_head_attn_fwd", K.dt_code(inp["Vout"].dtype), K.P(dev["Vout"]), K.P(dev["Lout"]), K.P(dev["Wq"]),
              K.P(dev["bq"]), K.P(dev["Wk"]), K.P(dev["bk"]), K.P(dev["Wv"]), K.P(dev["bv"]), K.P(dev["Wp"]),
              K.P(dev["bp"]) if bias_p else None, K.P(saved), saved.numel(), K.P(logits), K.P(pr), B, T, hid, nh, O,
              float(p), seed, K.stream())
    torch.cuda.synchronize()
    return logits, pr, saved


def _bwd(K, inp, shape, saved, p, seed, relu_mask, want=GRADS, dV=None, dL=None, bufs=None):
    """vcg_head_attn_bwd through the C ABI; the gradients named in `want` accumulate into buffers prefilled with
    FILL, the others are passed as NULL. -> dVout, dLout, {name: buffer}."""
    from vcg_hip import _lib
    B, T, hid, nh, O = shape
    dev = {k: v.to(DEV) for k, v in inp.items()}
    if bufs is None:
        bufs = {g: torch.full(inp[g[1:]].shape, FILL, device=DEV) for g in want}
    dV = torch.empty_like(dev["Vout"]) if dV is None else dV
    dL = torch.empty_like(dev["Lout"]) if dL is None else dL
    ws = torch.empty(_lib.query("vcg_head_attn_bwd_ws_floats", B, T, hid), device=DEV)
    _lib.call("vcg_head_attn_bwd", K.dt_code(inp["Vout"].dtype), K.P(saved), K.P(dev["Wq"]), K.P(dev["Wk"]),
              K.P(dev["Wv"]), K.P(dev["Wp"]), K.P(dev["dlogits"]), K.P(dV), K.P(dL),
              *(K.P(bufs.get(g)) for g in GRADS), K.P(ws), ws.numel(), B, T, hid, nh, O, float(p), seed,
              int(relu_mask), K.stream())
    torch.cuda.synchronize()
    return dV, dL, bufs


def _blocks(saved, shape):
    """`saved` cut into its blocks: X, K, V [B][T1][hid], q0, y0 [B][hid], P [B][nh][T1]."""
    B, T, hid, nh, O = shape
    T1 = T + 1
    sizes = {"X": (B, T1, hid), "K": (B, T1, hid), "V": (B, T1, hid), "q0": (B, hid), "y0": (B, hid),
             "P": (B, nh, T1)}
    out, o = {}, 0
    for name in BLOCKS:
        n = 1
        for d in sizes[name]:
            n *= d
        out[name] = saved[o:o + n].view(sizes[name])
        o += n
    assert o == saved.numel()
    return out


@pytest.mark.parametrize("p", PS, ids=["p0", "p0.3"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_head_attn_fwd(K, shape, dtype, p):
    """logits, prob and each block of `saved` against fp64; X is the input itself and must be exact."""
    inp, seed, (ref, _), (r32, _) = _case(shape, dtype, p)
    logits, prob, saved = _fwd(K, inp, shape, p, seed)
    tag = f"{shape} x {_name(dtype)} p={p}"
    got = _blocks(saved, shape)
    assert torch.equal(got["X"].cpu().double(), ref["X"]), "saved X is not the input"
    for name in BLOCKS:
        _close(got[name], ref[name], F32, f"head_attn_fwd saved {name} ({tag})", r32[name])
    _close(logits, ref["logits"], F32, f"head_attn_fwd logits ({tag})", r32["logits"])
    _close(prob, ref["prob"], F32, f"head_attn_fwd prob ({tag})", r32["prob"])


@pytest.mark.parametrize("relu_mask", [0, 1], ids=["norelu", "relu"])
@pytest.mark.parametrize("p", PS, ids=["p0", "p0.3"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_head_attn_bwd(K, shape, dtype, p, relu_mask):
    """dVout / dLout (exactly 0 where the ReLU mask closes) and the eight parameter gradients, accumulated into
    buffers prefilled with 0.5, against autograd through the fp64 reference."""
    inp, seed, (_, gref), (_, g32) = _case(shape, dtype, p, bool(relu_mask))
    _, _, saved = _fwd(K, inp, shape, p, seed)
    dV, dL, bufs = _bwd(K, inp, shape, saved, p, seed, relu_mask)
    tag = f"{shape} {_name(dtype)} p={p} relu={relu_mask}"
    _close(dV, gref["dVout"], dtype, f"head_attn_bwd dVout ({tag})", g32["dVout"])
    _close(dL, gref["dLout"], dtype, f"head_attn_bwd dLout ({tag})", g32["dLout"])
    for g in GRADS:
        # dbk: zero up to cancellation of the column sums of dK
        scale = gref["dK"].abs().sum((0, 1)).max().item() if g == "dbk" else None
        _close(bufs[g].double() - FILL, gref[g], F32, f"head_attn_bwd {g} (x {tag})", g32[g], scale)
    V, L = inp["Vout"].float(), inp["Lout"].float()
    if relu_mask:
        assert (dV.cpu()[V <= 0] == 0).all() and (dL.cpu()[L <= 0] == 0).all(), "gradient through a closed ReLU"
    else:
        assert (dV.cpu()[V <= 0] != 0).any(), "relu_mask = 0 must let the gradient through"


@pytest.mark.parametrize("shape", [(2, 8, 96, 3, 5), (5, 16, 128, 4, 2)], ids=str)
def test_head_attn_optional_pointers(K, shape):
    """prob = NULL and bp = NULL: the logits are those of the reference without the proj bias. Backward with only
    dWk and dbp: both correct, and dVout / dLout bit-identical to the call with every gradient pointer."""
    p = R.P_DROP
    inp, seed, (ref, gref), (r32, g32) = _case(shape, F32, p, True, False)
    logits, prob, saved = _fwd(K, inp, shape, p, seed, prob=False, bias_p=False)
    assert prob is None
    _close(logits, ref["logits"], F32, f"head_attn_fwd logits, bp = NULL ({shape})", r32["logits"])
    with_bias = _case(shape, F32, p, True)[2][0]["logits"]
    assert (with_bias - ref["logits"] - inp["bp"].double()).abs().max() < 1e-12
    full_logits, full_prob, full_saved = _fwd(K, inp, shape, p, seed)
    assert torch.equal(full_saved, saved), "prob = NULL / bp = NULL changed the saved state"
    assert not torch.equal(full_logits, logits), "bp = NULL must drop the bias"
    dV, dL, bufs = _bwd(K, inp, shape, saved, p, seed, 1)
    dV2, dL2, some = _bwd(K, inp, shape, saved, p, seed, 1, want=("dWk", "dbp"))
    assert set(some) == {"dWk", "dbp"}
    assert torch.equal(dV2, dV) and torch.equal(dL2, dL), "NULL gradient pointers changed dVout / dLout"
    assert torch.equal(some["dWk"], bufs["dWk"]) and torch.equal(some["dbp"], bufs["dbp"])
    _close(some["dWk"].double() - FILL, gref["dWk"], F32, f"head_attn_bwd dWk alone ({shape})", g32["dWk"])
    _close(some["dbp"].double() - FILL, inp["dlogits"].double().sum(0), F32, f"head_attn_bwd dbp alone ({shape})")


def test_head_attn_deterministic(K):
    """Forward + backward twice on the benchmarked shape with dropout: every output bit-identical (fixed-order
    reductions, no atomics)."""
    shape, p = (5, 16, 128, 4, 2), R.P_DROP
    inp = R.make_inputs(shape, BF16)
    seed = R.SEEDS[shape]
    runs = []
    for _ in range(2):
        logits, prob, saved = _fwd(K, inp, shape, p, seed)
        dV, dL, bufs = _bwd(K, inp, shape, saved, p, seed, 1)
        runs.append([logits, prob, saved, dV, dL] + [bufs[g] for g in GRADS])
    for a, b, what in zip(runs[0], runs[1], ["logits", "prob", "saved", "dVout", "dLout"] + list(GRADS)):
        assert not torch.isnan(a).any(), what
        assert torch.equal(a, b), f"{what} differs between two runs"


SENTINEL = -7.25
REFUSED = [(s, 0.0, "64 KB LDS limit") for s in R.REFUSED_LDS] + [
    ((2, 4, 30, 4, 2), 0.0, "divisible by n_head"),        # hid % nh != 0
    ((1, 64, 8, 1, 2), 0.0, r"T \+ 1 <= 64"),              # T + 1 > 64
    ((2, 4, 32, 4, 257), 0.0, "output_size <= 256"),       # O > 256
    ((2, 4, 32, 4, 2), 1.0, r"dropout p must be in \[0, 1\)"),
]


@pytest.mark.parametrize("shape,p,msg", REFUSED, ids=lambda v: str(v) if isinstance(v, tuple) else None)
def test_head_attn_refuses_beyond_lds(K, shape, p, msg):
    """Windows beyond the 64 KB of LDS (one token past the largest that fits at hid 256 and 128, and the maximum
    of the other limits), and the older refusals: both entry points return VCG_ERR_INVALID (-1) with their message
    before any launch, and no output buffer is touched."""
    from vcg_hip._lib import VcgError
    B, T, hid, nh, O = shape
    T1 = T + 1
    g = torch.Generator().manual_seed(5)
    inp = {"Vout": torch.randn(B * T, hid, generator=g), "Lout": torch.randn(B, hid, generator=g),
           "Wp": torch.randn(O, hid, generator=g), "bp": torch.zeros(O), "dlogits": torch.randn(B, O, generator=g)}
    for w in ("q", "k", "v"):
        inp["W" + w], inp["b" + w] = torch.randn(hid, hid, generator=g) * hid ** -0.5, torch.zeros(hid)
    n_saved = B * (3 * T1 * hid + 2 * hid + nh * T1)
    saved = torch.full((n_saved,), SENTINEL, device=DEV)
    logits = torch.full((B, O), SENTINEL, device=DEV)
    with pytest.raises(VcgError, match=rf"vcg_head_attn_fwd failed \(-1\).*{msg}"):
        _fwd(K, inp, shape, p, 1, saved=saved, logits=logits)
    torch.cuda.synchronize()
    assert (saved == SENTINEL).all() and (logits == SENTINEL).all(), "a refused forward wrote to its outputs"
    dV = torch.full((B * T, hid), SENTINEL, device=DEV)
    dL = torch.full((B, hid), SENTINEL, device=DEV)
    bufs = {gname: torch.full(inp[gname[1:]].shape, SENTINEL, device=DEV) for gname in GRADS}
    with pytest.raises(VcgError, match=rf"vcg_head_attn_bwd failed \(-1\).*{msg}"):
        _bwd(K, inp, shape, saved, p, 1, 1, dV=dV, dL=dL, bufs=bufs)
    torch.cuda.synchronize()
    assert (dV == SENTINEL).all() and (dL == SENTINEL).all(), "a refused backward wrote to dVout / dLout"
    for gname, b in bufs.items():
        assert (b == SENTINEL).all(), f"a refused backward wrote to {gname}"
