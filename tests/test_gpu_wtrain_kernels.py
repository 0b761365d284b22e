"""Kernel-level numerics of the window-model training kernels (csrc/wtrain.hip) against plain fp64 torch on the CPU,
fed the same fp32 inputs: ln_act_drop, act_drop, mul_bwd, mha_small, posenc, linear_small, softmax_rows, at the shapes
where each kernel takes another path (widths that are no multiple of the workgroup, several elements per thread, several
rows per workgroup with a partial last one, strided thread loops, odd head sizes, strided fused-QKV views, a key bias
longer than the window) and with dropout on and off.

Criterion (tests/test_gpu_kernels.py::_close, fp32): max abs error <= 2e-5 x max|reference|.

Dropout masks are never re-derived from the hash here: the keep decision depends on (seed, element index, p) only, so
the mask is read back from a forward on inputs that cannot be zero and reused, with the same seed, in the fp64
reference of the random-input forward and of the backward.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
ACTS = [ACT_NONE, ACT_RELU, ACT_GELU]
ACT_NAME = {ACT_NONE: "none", ACT_RELU: "relu", ACT_GELU: "gelu"}
PS = [0.0, 0.3]
SEED_A = 0x9E3779B97F4A7C15  # the upper 32 bits take part in the hash too
SEED_B = 12345


@pytest.fixture(scope="module")
def L():
    from vcg_hip import _lib
    _lib.call("vcg_init", 0)
    return _lib


def _ptr(t):
    from vcg_hip.ops import P
    return P(t)


def _stream():
    from vcg_hip.ops import stream
    return stream()


def _close(out, ref, what=""):
    out = out.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    scale = ref.abs().max().item() + 1e-6
    err = (out - ref).abs().max().item()
    assert err <= 2e-5 * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _rand(shape, seed, std=1.0, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * std + mean


def _act64(u, act):
    if act == ACT_RELU:
        return torch.relu(u)
    if act == ACT_GELU:
        return F.gelu(u)  # erf form, as nn.GELU()
    return u


def _leaf(t):
    return t.double().clone().requires_grad_()


def _kept_fraction_ok(mask, p):
    n = mask.numel()
    return abs(mask.double().mean().item() - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n)


# ================================================================================================ ln_act_drop
LN_SHAPES = [(3, 128), (5, 100), (4, 257), (2, 2048), (1100, 64)]


def _ln_fwd(L, x, g, b, act, p, seed, eps=1e-5):
    rows, D = x.shape
    out = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=DEV)
    rstd = torch.empty_like(mean)
    L.call("vcg_ln_act_drop_fwd", _ptr(x), _ptr(g), _ptr(b), _ptr(out), _ptr(mean), _ptr(rstd), rows, D, eps, act, p,
           seed, _stream())
    return out, mean, rstd


def _ln_bwd(L, dout, x, g, b, mean, rstd, gg, bg, act, p, seed):
    from vcg_hip import ops
    rows, D = x.shape
    dx = torch.empty_like(x)
    w = ops.ws(L.query("vcg_ln_act_drop_bwd_ws_bytes", rows, D), DEV)
    L.call("vcg_ln_act_drop_bwd", _ptr(dout), _ptr(x), _ptr(g), _ptr(b), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(gg),
           _ptr(bg), _ptr(w), w.numel() * 4, rows, D, act, p, seed, _stream())
    return dx


def _ln_mask(L, rows, D, p, seed):
    """LayerNorm output with beta = 10, gamma = 1 and no activation is never zero, so out != 0 is the keep mask."""
    x = _rand((rows, D), 99).to(DEV)
    out, _, _ = _ln_fwd(L, x, torch.ones(D, device=DEV), torch.full((D,), 10.0, device=DEV), ACT_NONE, p, seed)
    return (out != 0).cpu()


def _ln_ref(x, g, b, dout, act, mask, p, eps=1e-5):
    x, g, b = _leaf(x), _leaf(g), _leaf(b)
    mu = x.mean(1, keepdim=True)
    rstd = (x.var(1, unbiased=False, keepdim=True) + eps).rsqrt()
    out = _act64((x - mu) * rstd * g + b, act) * mask.double() / (1 - p)
    out.backward(dout.double())
    return out.detach(), mu.detach().flatten(), rstd.detach().flatten(), x.grad, g.grad, b.grad


def _ln_inputs(rows, D):
    x = _rand((rows, D), 1, 0.5, 3.0)
    g = 1 + 0.3 * _rand((D,), 2)
    b = 0.3 * _rand((D,), 3)
    dout = _rand((rows, D), 4)
    gg0, bg0 = _rand((D,), 5), _rand((D,), 6)
    return x, g, b, dout, gg0, bg0


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_ln_act_drop_fwd_bwd(L, rows, D, p):
    seed = SEED_A ^ (rows * 4099 + D)
    mask = _ln_mask(L, rows, D, p, seed)
    if p == 0.0:
        assert mask.all()
    x, g, b, dout, gg0, bg0 = _ln_inputs(rows, D)
    xd, gd, bd, doutd = (t.to(DEV) for t in (x, g, b, dout))
    for act in ACTS:
        tag = f"ln ({rows},{D}) p={p} {ACT_NAME[act]}"
        r_out, r_mean, r_rstd, r_dx, r_dg, r_db = _ln_ref(x, g, b, dout, act, mask, p)
        out, mean, rstd = _ln_fwd(L, xd, gd, bd, act, p, seed)
        _close(out, r_out, tag + " out")
        _close(mean, r_mean, tag + " mean")
        _close(rstd, r_rstd, tag + " rstd")
        gg, bg = gg0.to(DEV), bg0.to(DEV)
        dx = _ln_bwd(L, doutd, xd, gd, bd, mean, rstd, gg, bg, act, p, seed)
        _close(dx, r_dx, tag + " dx")
        _close(gg, gg0.double() + r_dg, tag + " gamma_grad (accumulated)")
        _close(bg, bg0.double() + r_db, tag + " beta_grad (accumulated)")


def test_ln_act_drop_width_limit(L):
    from vcg_hip._lib import VcgError
    rows, D = 2, 2049
    x = _rand((rows, D), 1).to(DEV)
    g, b = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    with pytest.raises(VcgError, match="LayerNorm width"):
        _ln_fwd(L, x, g, b, ACT_NONE, 0.0, 0)
    mean, rstd = torch.zeros(rows, device=DEV), torch.ones(rows, device=DEV)
    with pytest.raises(VcgError, match="LayerNorm width"):
        _ln_bwd(L, x, x, g, b, mean, rstd, None, None, ACT_NONE, 0.0, 0)


def test_dropout_mask_statistics(L):
    p, rows, D = 0.3, 1100, 64
    m_a = _ln_mask(L, rows, D, p, SEED_A)
    m_b = _ln_mask(L, rows, D, p, SEED_B)
    for m in (m_a, m_b):
        assert _kept_fraction_ok(m, p), m.double().mean().item()
    assert not torch.equal(m_a, m_b), "two seeds gave the same mask"
    assert not (m_a == m_a[0:1]).all(), "every row has the same mask"
    # seeds that differ only in the upper 32 bits
    assert not torch.equal(m_a, _ln_mask(L, rows, D, p, SEED_A ^ (1 << 40)))
    assert _ln_mask(L, rows, D, 0.0, SEED_A).all()
    n = 256 * 4096 + 5
    e_a, e_b = _act_drop_mask(L, n, p, SEED_A), _act_drop_mask(L, n, p, SEED_B)
    assert _kept_fraction_ok(e_a, p) and _kept_fraction_ok(e_b, p)
    assert not torch.equal(e_a, e_b)
    assert _act_drop_mask(L, n, 0.0, SEED_A).all()
    # LayerNorm and the elementwise kernel index the same flat element space
    assert torch.equal(m_a.flatten(), e_a[:rows * D])


@pytest.mark.parametrize("rows,D", [(4, 257), (1100, 64)])
def test_ln_act_drop_function_accumulates(L, rows, D):
    """LNActDropFn on a real nn.LayerNorm: dx is returned, the parameter gradients are added onto what .grad holds,
    and the backward uses the forward's mask (the seed the Function drew)."""
    from vcg_hip.nn import new_seed
    from vcg_hip.wtrain import LNActDropFn
    p, act = 0.3, ACT_GELU
    x, g, b, dout, gg0, bg0 = _ln_inputs(rows, D)
    ln = torch.nn.LayerNorm(D).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(g)
        ln.bias.copy_(b)
    ln.weight.grad, ln.bias.grad = gg0.to(DEV), bg0.to(DEV)
    torch.manual_seed(31)
    seed = new_seed()
    mask = _ln_mask(L, rows, D, p, seed)
    xd = x.to(DEV).requires_grad_()
    torch.manual_seed(31)
    out = LNActDropFn.apply(xd, ln, act, p)
    out.backward(dout.to(DEV))
    r_out, _, _, r_dx, r_dg, r_db = _ln_ref(x, g, b, dout, act, mask, p, eps=ln.eps)
    _close(out, r_out, "LNActDropFn out")
    _close(xd.grad, r_dx, "LNActDropFn dx")
    _close(ln.weight.grad, gg0.double() + r_dg, "LNActDropFn weight.grad")
    _close(ln.bias.grad, bg0.double() + r_db, "LNActDropFn bias.grad")


# ================================================================================================ act_drop, mul
def _act_drop_fwd(L, x, res, act, p, seed):
    out = torch.empty_like(x)
    L.call("vcg_act_drop_fwd", _ptr(x), _ptr(res), _ptr(out), x.numel(), act, p, seed, _stream())
    return out


def _act_drop_mask(L, n, p, seed):
    out = _act_drop_fwd(L, torch.ones(n, device=DEV), None, ACT_NONE, p, seed)
    return (out != 0).cpu()


def _act_drop_ref(x, res, dout, act, mask, p):
    x = _leaf(x)
    out = _act64(x, act) * mask.double() / (1 - p)
    if res is not None:
        out = out + res.double()
    out.backward(dout.double())
    return out.detach(), x.grad


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n", [7, 256 * 4096 + 5])
def test_act_drop_fwd_bwd(L, n, p):
    seed = SEED_B + n
    mask = _act_drop_mask(L, n, p, seed)
    if p == 0.0:
        assert mask.all()
    x, res, dout = _rand((n,), 1), _rand((n,), 2), _rand((n,), 3)
    xd, resd, doutd = x.to(DEV), res.to(DEV), dout.to(DEV)
    for act in ACTS:
        for r, rd in ((None, None), (res, resd)):
            tag = f"act_drop n={n} p={p} {ACT_NAME[act]} res={r is not None}"
            r_out, r_dx = _act_drop_ref(x, r, dout, act, mask, p)
            _close(_act_drop_fwd(L, xd, rd, act, p, seed), r_out, tag + " out")
            dx = torch.empty_like(xd)
            L.call("vcg_act_drop_bwd", _ptr(doutd), _ptr(xd), _ptr(dx), n, act, p, seed, _stream())
            _close(dx, r_dx, tag + " dx")


def test_act_drop_function(L):
    from vcg_hip.nn import new_seed
    from vcg_hip.wtrain import ActDropFn
    n, p = 1000, 0.3
    x, res, dout = _rand((n,), 1), _rand((n,), 2), _rand((n,), 3)
    torch.manual_seed(41)
    mask = _act_drop_mask(L, n, p, new_seed())
    xd, rd = x.to(DEV).requires_grad_(), res.to(DEV).requires_grad_()
    torch.manual_seed(41)
    out = ActDropFn.apply(xd, ACT_GELU, p, rd)
    out.backward(dout.to(DEV))
    r_out, r_dx = _act_drop_ref(x, res, dout, ACT_GELU, mask, p)
    _close(out, r_out, "ActDropFn out")
    _close(xd.grad, r_dx, "ActDropFn dx")
    _close(rd.grad, dout, "ActDropFn dres")


def test_mul_bwd(L):
    from vcg_hip.wtrain import MulFn
    n = 1000
    a, b, d = _rand((n,), 1), _rand((n,), 2), _rand((n,), 3)
    ad, bd, dd = a.to(DEV), b.to(DEV), d.to(DEV)
    r_da, r_db = d.double() * b.double(), d.double() * a.double()
    for want_a, want_b in ((True, True), (True, False), (False, True)):
        da = torch.full((n,), 7.0, device=DEV) if want_a else None
        db = torch.full((n,), 7.0, device=DEV) if want_b else None
        L.call("vcg_mul_bwd", _ptr(dd), _ptr(ad), _ptr(bd), _ptr(da), _ptr(db), n, _stream())
        if want_a:
            _close(da, r_da, "mul_bwd da")
        if want_b:
            _close(db, r_db, "mul_bwd db")
    ag, bg = ad.clone().requires_grad_(), bd.clone().requires_grad_()
    out = MulFn.apply(ag, bg)
    out.backward(dd)
    _close(out, a.double() * b.double(), "MulFn out")
    _close(ag.grad, r_da, "MulFn da")
    _close(bg.grad, r_db, "MulFn db")


# ================================================================================================ mha_small
def _scale(dh):
    return float(np.float32(1.0 / math.sqrt(dh)))


def _mha_fwd(L, q, ldq, k, ldk, v, ldv, bias, Pb, dims, p, seed):
    B, Sq, Sk, nh, dh = dims
    H = nh * dh
    ctx = torch.empty((B * Sq, H), dtype=torch.float32, device=DEV)
    probs = torch.empty(B * nh * Sq * Sk, dtype=torch.float32, device=DEV)
    L.call("vcg_mha_small_fwd", _ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv, _ptr(bias), Pb, _ptr(ctx), H, _ptr(probs), B,
           Sq, Sk, nh, dh, _scale(dh), p, seed, _stream())
    return ctx, probs.view(B, nh, Sq, Sk)


def _mha_dropped_probs(L, q, k, bias, Pb, dims, p, seed):
    """The dropped probabilities the kernel multiplies into V, read from ctx with one-hot value rows:
    v[b, j, h*dh + e] = (e == j - pass*dh) makes ctx[b, i, h*dh + e] the dropped probability of key pass*dh + e."""
    B, Sq, Sk, nh, dh = dims
    H = nh * dh
    Pd = torch.zeros(B, nh, Sq, Sk)
    for ps in range((Sk + dh - 1) // dh):
        lo, hi = ps * dh, min(Sk, ps * dh + dh)
        v1 = torch.zeros(B, Sk, nh, dh)
        for j in range(lo, hi):
            v1[:, j, :, j - lo] = 1.0
        ctx, _ = _mha_fwd(L, q, H, k, H, v1.view(B * Sk, H).to(DEV), H, bias, Pb, dims, p, seed)
        Pd[..., lo:hi] = ctx.cpu().view(B, Sq, nh, dh).permute(0, 2, 1, 3)[..., :hi - lo]
    return Pd


def _mha_ref(q, k, v, bias, dctx, dims, mask, p):
    B, Sq, Sk, nh, dh = dims
    q, k, v = _leaf(q), _leaf(k), _leaf(v)
    b = _leaf(bias) if bias is not None else None
    qh = q.view(B, Sq, nh, dh).permute(0, 2, 1, 3)
    kh = k.view(B, Sk, nh, dh).permute(0, 2, 1, 3)
    vh = v.view(B, Sk, nh, dh).permute(0, 2, 1, 3)
    s = qh @ kh.transpose(-1, -2) * _scale(dh)
    if b is not None:
        s = s + b[:, :Sk].view(1, nh, 1, Sk)
    probs = torch.softmax(s, -1)
    Pd = probs * mask.double() / (1 - p)
    ctx = (Pd @ vh).permute(0, 2, 1, 3).reshape(B * Sq, nh * dh)
    ctx.backward(dctx.double())
    return ctx.detach(), probs.detach(), Pd.detach(), q.grad, k.grad, v.grad, (b.grad if b is not None else None)


# (B, Sq, Sk, nh, dh), Pb (0 = no key bias), q / k / v as column slices of one [rows, 3H] buffer
MHA_CASES = [
    ((2, 3, 3, 16, 8), 3, False),     # the window model's own shape
    ((2, 3, 3, 16, 8), 3, True),      # ... on fused-QKV views (row stride 3H)
    ((3, 1, 16, 8, 16), 0, False),    # cross attention, one query
    ((2, 32, 12, 16, 8), 0, False),   # nh * Sq = 512 > 256 threads
    ((1, 5, 32, 4, 5), 0, False),     # odd head size, Sk at the limit
    ((5, 7, 7, 2, 16), 9, False),     # key bias longer than the window
]


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("dims,Pb,fused", MHA_CASES)
def test_mha_small_fwd_bwd(L, dims, Pb, fused, p):
    from vcg_hip import ops
    B, Sq, Sk, nh, dh = dims
    H = nh * dh
    seed = SEED_A + 17 * B + Sq
    bias = 0.5 * _rand((nh, Pb), 5) if Pb else None
    dctx = _rand((B * Sq, H), 6)
    db0 = _rand((nh, Pb), 7) if Pb else None
    if fused:
        assert Sq == Sk
        buf = _rand((B * Sq, 3 * H), 8).to(DEV)
        qd, kd, vd = buf[:, :H], buf[:, H:2 * H], buf[:, 2 * H:]
        ld = 3 * H
        q, k, v = (t.cpu().contiguous() for t in (qd, kd, vd))
        dbuf = torch.full((B * Sq, 3 * H), 7.0, device=DEV)
        dq, dk, dv = dbuf[:, :H], dbuf[:, H:2 * H], dbuf[:, 2 * H:]
    else:
        q, k, v = _rand((B * Sq, H), 1), _rand((B * Sk, H), 2), _rand((B * Sk, H), 3)
        qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
        ld = H
        dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    biasd = bias.to(DEV) if Pb else None
    tag = f"mha {dims} Pb={Pb} fused={fused} p={p}"

    Pd = _mha_dropped_probs(L, q.to(DEV), k.to(DEV), biasd, Pb, dims, p, seed)
    mask = Pd != 0
    if p == 0.0:
        assert mask.all()
    else:
        assert _kept_fraction_ok(mask, p), mask.double().mean().item()
    r_ctx, r_probs, r_Pd, r_dq, r_dk, r_dv, r_db = _mha_ref(q, k, v, bias, dctx, dims, mask, p)
    _close(Pd, r_Pd, tag + " dropped probs")

    ctx, probs = _mha_fwd(L, qd, ld, kd, ld, vd, ld, biasd, Pb, dims, p, seed)
    _close(probs, r_probs, tag + " probs (pre-dropout)")
    _close(ctx, r_ctx, tag + " ctx")

    dbias = db0.to(DEV) if Pb else None
    dctxd = dctx.to(DEV)
    w = ops.ws(L.query("vcg_mha_small_bwd_ws_bytes", B, nh, max(Pb, 1)), DEV)
    L.call("vcg_mha_small_bwd", _ptr(qd), ld, _ptr(kd), ld, _ptr(vd), ld, _ptr(probs), _ptr(dctxd), H, _ptr(dq),
           ld, _ptr(dk), ld, _ptr(dv), ld, _ptr(dbias), Pb, _ptr(w), w.numel() * 4, B, Sq, Sk, nh, dh, _scale(dh), p, seed,
           _stream())
    _close(dq, r_dq, tag + " dq")
    _close(dk, r_dk, tag + " dk")
    _close(dv, r_dv, tag + " dv")
    if Pb:
        _close(dbias[:, :Sk], db0[:, :Sk].double() + r_db[:, :Sk], tag + " dbias (accumulated)")
        assert torch.equal(dbias[:, Sk:].cpu(), db0[:, Sk:]), tag + ": bias columns beyond the window were written"


def test_mha_function_accumulates_dbias(L):
    from vcg_hip.nn import new_seed
    from vcg_hip.wtrain import MHAFn
    dims, Pb, p = (5, 7, 7, 2, 16), 9, 0.3
    B, Sq, Sk, nh, dh = dims
    H = nh * dh
    q, k, v = _rand((B * Sq, H), 1), _rand((B * Sk, H), 2), _rand((B * Sk, H), 3)
    bias, dctx, db0 = 0.5 * _rand((nh, Pb), 5), _rand((B * Sq, H), 6), _rand((nh, Pb), 7)
    bp = torch.nn.Parameter(bias.view(1, nh, 1, Pb).to(DEV))  # window_pos_bias layout
    bp.grad = db0.view(1, nh, 1, Pb).to(DEV)
    torch.manual_seed(51)
    seed = new_seed()
    mask = _mha_dropped_probs(L, q.to(DEV), k.to(DEV), bias.to(DEV), Pb, dims, p, seed) != 0
    qd, kd, vd = (t.to(DEV).requires_grad_() for t in (q, k, v))
    torch.manual_seed(51)
    ctx = MHAFn.apply(qd, kd, vd, bp, B, Sq, Sk, nh, p)
    ctx.backward(dctx.to(DEV))
    r_ctx, _, _, r_dq, r_dk, r_dv, r_db = _mha_ref(q, k, v, bias, dctx, dims, mask, p)
    _close(ctx, r_ctx, "MHAFn ctx")
    _close(qd.grad, r_dq, "MHAFn dq")
    _close(kd.grad, r_dk, "MHAFn dk")
    _close(vd.grad, r_dv, "MHAFn dv")
    got = bp.grad.view(nh, Pb)
    _close(got[:, :Sk], db0[:, :Sk].double() + r_db[:, :Sk], "MHAFn bias.grad")
    assert torch.equal(got[:, Sk:].cpu(), db0[:, Sk:])


def test_mha_small_refuses_windows_beyond_the_lds(L):
    """nh = 16, Sq = Sk = 32 needs 2 * 16 * 32 * 32 * 4 B = 128 KB of LDS score buffers in the backward, which
    refuses it; the forward refuses the same shapes, so a training step fails before it has run half way."""
    from vcg_hip import ops
    from vcg_hip._lib import VcgError
    dims = (1, 32, 32, 16, 8)
    B, Sq, Sk, nh, dh = dims
    H = nh * dh
    q, k, v = (_rand((B * 32, H), s).to(DEV) for s in (1, 2, 3))
    with pytest.raises(VcgError, match="too large for the LDS"):
        _mha_fwd(L, q, H, k, H, v, H, None, 0, dims, 0.0, 0)
    probs = torch.full((B * nh * Sq * Sk,), 1.0 / Sk, device=DEV)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    w = ops.ws(L.query("vcg_mha_small_bwd_ws_bytes", B, nh, 1), DEV)
    with pytest.raises(VcgError, match="too large for the LDS"):
        L.call("vcg_mha_small_bwd", _ptr(q), H, _ptr(k), H, _ptr(v), H, _ptr(probs), _ptr(q), H, _ptr(dq), H, _ptr(dk),
               H, _ptr(dv), H, None, 0, _ptr(w), w.numel() * 4, B, Sq, Sk, nh, dh, _scale(dh), 0.0, 0, _stream())
    # the largest window of 16 heads that fits (2 * 16 * 32 * 16 * 4 B = 64 KB) is accepted by both
    dims = (1, 32, 16, 16, 8)
    k2, v2 = k[:16].contiguous(), v[:16].contiguous()
    ctx, probs = _mha_fwd(L, q, H, k2, H, v2, H, None, 0, dims, 0.0, 0)
    dk2, dv2 = torch.empty_like(k2), torch.empty_like(v2)
    L.call("vcg_mha_small_bwd", _ptr(q), H, _ptr(k2), H, _ptr(v2), H, _ptr(probs), _ptr(q), H, _ptr(dq), H, _ptr(dk2),
           H, _ptr(dv2), H, None, 0, _ptr(w), w.numel() * 4, 1, 32, 16, nh, dh, _scale(dh), 0.0, 0, _stream())
    torch.cuda.synchronize()
    _close(probs.sum(-1), torch.ones(1, nh, 32), "probs rows")


# ================================================================================================ posenc
@pytest.mark.parametrize("rows,S,H", [(15, 5, 128), (700, 7, 36)])
def test_posenc_fwd_bwd(L, rows, S, H):
    from vcg_hip.wtrain import PosEncFn
    x, dout = _rand((rows, H), 1), _rand((rows, H), 2)
    pos = _rand((S,), 3)
    lin = torch.nn.Linear(1, H).to(DEV)
    w, b = _rand((H, 1), 4), _rand((H,), 5)
    dw0, db0 = _rand((H, 1), 6), _rand((H,), 7)
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(b)
    lin.weight.grad, lin.bias.grad = dw0.to(DEV), db0.to(DEV)
    # fp64: out[r] = x[r] + pos[r % S] * w + b
    x64, w64, b64 = _leaf(x), _leaf(w), _leaf(b)
    pr = pos.double()[torch.arange(rows) % S]
    ref = x64 + pr[:, None] * w64[:, 0][None, :] + b64
    ref.backward(dout.double())
    # forward through the C ABI
    out = torch.empty((rows, H), dtype=torch.float32, device=DEV)
    xd, posd = x.to(DEV).requires_grad_(), pos.to(DEV)
    L.call("vcg_posenc_fwd", _ptr(xd), _ptr(posd), _ptr(lin.weight), _ptr(lin.bias), _ptr(out), rows, S, H, _stream())
    _close(out, ref, f"posenc ({rows},{S},{H}) out")
    out2 = PosEncFn.apply(xd, lin, posd)
    out2.backward(dout.to(DEV))
    _close(out2, ref, "PosEncFn out")
    _close(xd.grad, x64.grad, "PosEncFn dx")
    _close(lin.weight.grad, dw0.double() + w64.grad, "PosEncFn weight.grad (accumulated)")
    _close(lin.bias.grad, db0.double() + b64.grad, "PosEncFn bias.grad (accumulated)")


# ================================================================================================ linear_small
LIN_SHAPES = [(5, 2, 130), (300, 3, 7), (1, 2, 4)]


def _lin_inputs(M, N, K):
    return (_rand((M, K), 1), _rand((N, K), 2, 1.0 / math.sqrt(K)), _rand((N,), 3), _rand((M, N), 4), _rand((M, N), 5),
            _rand((N, K), 6), _rand((N,), 7))


@pytest.mark.parametrize("M,N,K", LIN_SHAPES)
def test_linear_small_fwd_bwd(L, M, N, K):
    x, W, b, res, g, dW0, db0 = _lin_inputs(M, N, K)
    xd, Wd, bd, resd, gd = (t.to(DEV) for t in (x, W, b, res, g))
    lin64 = x.double() @ W.double().t() + b.double()
    for act in ACTS:
        for r, rd in ((None, None), (res, resd)):
            y = torch.empty((M, N), dtype=torch.float32, device=DEV)
            L.call("vcg_linear_small_fwd", _ptr(xd), _ptr(Wd), _ptr(bd), _ptr(rd), _ptr(y), M, N, K, act, _stream())
            ref = _act64(lin64 + (r.double() if r is not None else 0.0), act)
            _close(y, ref, f"linear_small ({M},{N},{K}) {ACT_NAME[act]} res={r is not None}")
    y = torch.empty((M, N), dtype=torch.float32, device=DEV)
    L.call("vcg_linear_small_fwd", _ptr(xd), _ptr(Wd), None, None, _ptr(y), M, N, K, ACT_NONE, _stream())
    _close(y, x.double() @ W.double().t(), "linear_small without bias")
    dx = torch.empty_like(xd)
    dW, db = dW0.to(DEV), db0.to(DEV)
    L.call("vcg_linear_small_bwd", _ptr(gd), _ptr(xd), _ptr(Wd), _ptr(dx), _ptr(dW), _ptr(db), M, N, K, _stream())
    _close(dx, g.double() @ W.double(), "linear_small dx")
    _close(dW, dW0.double() + g.double().t() @ x.double(), "linear_small dW (accumulated)")
    _close(db, db0.double() + g.double().sum(0), "linear_small db (accumulated)")
    # dx is optional; dW / db still accumulate, a second time
    L.call("vcg_linear_small_bwd", _ptr(gd), _ptr(xd), _ptr(Wd), None, _ptr(dW), _ptr(db), M, N, K, _stream())
    _close(dW, dW0.double() + 2 * (g.double().t() @ x.double()), "linear_small dW (second accumulation)")
    _close(db, db0.double() + 2 * g.double().sum(0), "linear_small db (second accumulation)")


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU])
@pytest.mark.parametrize("M,N,K", LIN_SHAPES)
def test_linear_function_small_path(L, M, N, K, act):
    from vcg_hip.wtrain import LinearFn
    x, W, b, res, g, dW0, db0 = _lin_inputs(M, N, K)
    lin = torch.nn.Linear(K, N).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(W)
        lin.bias.copy_(b)
    lin.weight.grad, lin.bias.grad = dW0.to(DEV), db0.to(DEV)
    xd, rd = x.to(DEV).requires_grad_(), res.to(DEV).requires_grad_()
    y = LinearFn.apply(xd, lin, act, rd)
    y.backward(g.to(DEV))
    x64, W64, b64, r64 = _leaf(x), _leaf(W), _leaf(b), _leaf(res)
    ref = _act64(x64 @ W64.t() + b64 + r64, act)
    ref.backward(g.double())
    tag = f"LinearFn ({M},{N},{K}) {ACT_NAME[act]}"
    _close(y, ref, tag + " y")
    _close(xd.grad, x64.grad, tag + " dx")
    _close(rd.grad, r64.grad, tag + " dres")
    _close(lin.weight.grad, dW0.double() + W64.grad, tag + " weight.grad (accumulated)")
    _close(lin.bias.grad, db0.double() + b64.grad, tag + " bias.grad (accumulated)")


# ================================================================================================ softmax_rows
@pytest.mark.parametrize("rows,C", [(300, 2), (3, 7)])
def test_softmax_rows(L, rows, C):
    from vcg_hip.wtrain import softmax_rows
    x = _rand((rows, C), 1, 3.0)
    x[0] = 80.0                      # a row of equal (large) values
    x[1, 0], x[1, 1:] = 80.0, -80.0  # the largest spread
    x[2, 0], x[2, 1:] = -80.0, 80.0
    out = softmax_rows(x.to(DEV))
    ref = torch.softmax(x.double(), 1)
    _close(out, ref, f"softmax_rows ({rows},{C})")
    assert torch.isfinite(out).all()
    assert (out.double().sum(1).cpu() - 1).abs().max().item() <= 1e-6
