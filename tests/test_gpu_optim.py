"""Fused clip + AdamW (csrc/optim.hip: vcg_sumsq, vcg_adamw; vcg_hip/optim.py: FusedAdamW) against fp64 AdamW.

Hyper-parameters at which every term of the update is far above fp32 rounding (lr 1e-2, weight decay 0.1, betas
(0.9, 0.95), |p| ~ 0.1), several steps (bias corrections for t > 1), the three codes of the per-256-element flag table
(0 = no decay, 1 = decay, 2 = frozen), the clip coefficient in its three regimes, grad_scale != 1, the bf16 shadow and
the grid-stride loop (more than 8192 blocks of 256 elements).

Criterion: the references are plain fp64 torch on the CPU, fed the same fp32 inputs. A quantity passes when its
largest error against fp64 is at most max(3 x the error of the same chain evaluated by torch in fp32 on the CPU,
2e-5 x max|fp64 reference|); both terms are computed inside the test.
"""
import copy
import math

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

DEV = "cuda"
BLK = 256  # elements per flag byte (flat.ALIGN)
LR, WD, BETAS, EPS = 1e-2, 0.1, (0.9, 0.95), 1e-8
STEPS = 5


@pytest.fixture(scope="module")
def K():
    from vcg_hip import _lib, ops
    _lib.call("vcg_init", 0)
    return ops


def _check(out, ref64, ref32, what):
    """error vs fp64 <= max(3 x torch-fp32's error vs fp64, 2e-5 x max|ref|)"""
    out, ref32 = out.double().cpu(), ref32.double()
    err = (out - ref64).abs().max().item()
    err32 = (ref32 - ref64).abs().max().item()
    tol = max(3 * err32, 2e-5 * ref64.abs().max().item())
    print(f"{what}: err {err:.3e}  torch-fp32 err {err32:.3e}  tol {tol:.3e}")
    assert err <= tol, f"{what}: err {err:.3e} > tol {tol:.3e} (torch-fp32 err {err32:.3e})"
    return tol


# ------------------------------------------------------------------------------------------------ (a) kernel level
def _flag_table(nblk):
    """Runs of 0 / 1 / 2, single-block runs among them, and a 2 as the very last block. With more than 8192 blocks the
    last three (the ones the grid-stride loop reaches on its second trip) are 0, 1, 2."""
    if nblk == 6:
        return torch.tensor([1, 1, 0, 2, 1, 2], dtype=torch.uint8)
    runs = [(1, 700), (0, 1), (2, 300), (1, 1), (0, 1500), (2, 1), (1, 3000), (0, 400), (2, 2), (0, 37), (1, 1)]
    fl = torch.cat([torch.full((n,), c, dtype=torch.uint8) for c, n in runs])
    assert fl.numel() < nblk - 3
    fl = torch.cat([fl, torch.full((nblk - 3 - fl.numel(),), 1, dtype=torch.uint8),
                    torch.tensor([0, 1, 2], dtype=torch.uint8)])
    assert fl.numel() == nblk and fl[-1] == 2
    return fl


# name -> (clip, grad_scale, max_norm as a multiple of sqrt(n) or an absolute value)
# gradients are N(0, 1), so ||g|| ~ sqrt(n): "inactive" puts max_norm between ||g|| * grad_scale and ||g||, so a clip
# taken against the unscaled norm (or a grad_scale applied twice) changes the result.
CASES = {
    "noclip": (False, 1.0, None),
    "clip_active": (True, 1.0, 1.0),
    "clip_inactive": (True, 0.5, ("sqrt_n", 0.75)),
    "clip_active_scaled": (True, 0.5, 1.0),
}


def _max_norm(spec, n):
    if spec is None:
        return 1.0
    if isinstance(spec, tuple):
        return spec[1] * math.sqrt(n)
    return spec


def _inputs(n, flags):
    gen = torch.Generator().manual_seed(1000 + n % 997)
    p0 = torch.randn(n, generator=gen) * 0.1
    grads = [torch.randn(n, generator=gen) for _ in range(STEPS)]
    code = flags.repeat_interleave(BLK)
    frozen = code == 2
    # moments start at zero (AdamW from scratch) except on frozen blocks, whose contents must survive untouched
    m0 = torch.where(frozen, torch.randn(n, generator=gen), torch.zeros(n))
    v0 = torch.where(frozen, torch.rand(n, generator=gen), torch.zeros(n))
    sentinel = ((torch.arange(n) % 251).float() - 100.0).to(torch.bfloat16)
    return p0, grads, code, m0, v0, sentinel


def _ref_adamw(p0, grads, code, case, dtype, wd=WD):
    """torch.optim.AdamW's formula (decoupled decay, lerp first moment, sqrt(v) / sqrt(bc2) + eps) after
    clip_grad_norm_ of grad_scale * g, in `dtype` on the CPU. Returns [(p, m, v)] after every step."""
    clip, gs, mn = CASES[case]
    max_norm = _max_norm(mn, p0.numel())
    b1, b2 = BETAS
    act, dec = code != 2, code == 1
    p = p0.to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for t, g32 in enumerate(grads, 1):
        g = g32.to(dtype) * gs
        if clip:
            c = torch.clamp(max_norm / (g.norm() + 1e-6), max=1.0)
            g = g * c
        pn = torch.where(dec, p * (1 - LR * wd), p)
        mn_ = m.lerp(g, 1 - b1)
        vn = (v * b2).addcmul(g, g, value=1 - b2)
        denom = (vn.sqrt() / math.sqrt(1 - b2 ** t)).add(EPS)
        pn = pn.addcdiv(mn_, denom, value=-(LR / (1 - b1 ** t)))
        p, m, v = torch.where(act, pn, p), torch.where(act, mn_, m), torch.where(act, vn, v)
        out.append((p.clone(), m.clone(), v.clone()))
    return out


def _run_kernel(K, inputs, flags, case, with_shadow, force_no_clip=False):
    """STEPS steps of ops.adamw; returns [(p, m, v, shadow)] (GPU clones) after every step."""
    p0, grads, code, m0, v0, sentinel = inputs
    clip, gs, mn = CASES[case]
    max_norm = _max_norm(mn, p0.numel())
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    shadow = sentinel.to(DEV) if with_shadow else None
    fl = flags.to(DEV)
    sumsq = torch.zeros(1, device=DEV)
    b1, b2 = BETAS
    out, wsp = [], None
    for t, g in enumerate(grads, 1):
        g = g.to(DEV)
        dev_sumsq = None
        if clip and not force_no_clip:
            wsp = K.sumsq(g, sumsq, wsp)
            dev_sumsq = sumsq
        K.adamw(p, g, m, v, fl, 8, LR, b1, b2, EPS, WD, t, dev_sumsq, max_norm, gs, shadow)
        out.append((p.clone(), m.clone(), v.clone(), shadow.clone() if with_shadow else None))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("nblk", [6, 8192 + 3])
def test_adamw_kernel_vs_fp64(K, nblk, case):
    n = nblk * BLK
    flags = _flag_table(nblk)
    inputs = _inputs(n, flags)
    p0, grads, code, m0, v0, sentinel = inputs
    ref64 = _ref_adamw(p0, grads, code, case, torch.float64)
    ref32 = _ref_adamw(p0, grads, code, case, torch.float32)
    nowd64 = _ref_adamw(p0, grads, code, case, torch.float64, wd=0.0)
    got = _run_kernel(K, inputs, flags, case, with_shadow=True)
    frozen = code == 2
    frozen_d = frozen.to(DEV)
    live_d = ~frozen_d
    p0d = p0.double()
    for t in range(STEPS):
        p, m, v, sh = got[t]
        for c in (0, 1):
            sel = code == c
            for name, o, k in (("m", m, 1), ("v", v, 2)):
                _check(o.cpu()[sel], ref64[t][k][sel], ref32[t][k][sel], f"{case} step {t + 1} code {c} {name}")
            tol = _check(p.cpu().double()[sel] - p0d[sel], ref64[t][0][sel] - p0d[sel],
                         ref32[t][0].double()[sel] - p0d[sel], f"{case} step {t + 1} code {c} p - p0")
            if c == 1:
                # the decay is visible: leaving it out would move the fp64 result by far more than the tolerance
                gap = (ref64[t][0][sel] - nowd64[t][0][sel]).abs().max().item()
                assert gap > 20 * tol, f"decay gap {gap:.3e} vs tol {tol:.3e}"
        # frozen blocks: bit-identical to the initial contents
        assert torch.equal(p[frozen_d].cpu(), p0[frozen]), f"{case} step {t + 1}: frozen p changed"
        assert torch.equal(m[frozen_d].cpu(), m0[frozen]), f"{case} step {t + 1}: frozen m changed"
        assert torch.equal(v[frozen_d].cpu(), v0[frozen]), f"{case} step {t + 1}: frozen v changed"
        # bf16 shadow: f2bf(p) on updated blocks, untouched (sentinel) on frozen ones
        want = p.to(torch.bfloat16).view(torch.int16)
        assert torch.equal(sh.view(torch.int16)[live_d], want[live_d]), f"{case} step {t + 1}: shadow != bf16(p)"
        assert torch.equal(sh.view(torch.int16)[frozen_d].cpu(), sentinel.view(torch.int16)[frozen]), \
            f"{case} step {t + 1}: shadow of a frozen block was written"
    if case == "clip_inactive":
        # c = 1 exactly: the same bits as the same steps without the clip (same grad_scale), shadow or not
        plain = _run_kernel(K, inputs, flags, case, with_shadow=False, force_no_clip=True)
        for t in range(STEPS):
            for name, a, b in zip("pmv", got[t][:3], plain[t][:3]):
                assert torch.equal(a, b), f"inactive clip changed {name} at step {t + 1}"


# ------------------------------------------------------------------------------------------------ (b) optimiser level
class _Leaf(nn.Module):
    def __init__(self, gen, **shapes):
        super().__init__()
        for k, s in shapes.items():
            self.register_parameter(k, nn.Parameter(torch.randn(s, generator=gen) * 0.1))


class _Toy(nn.Module):
    """Parameter names that hit both grouping rules (bias leaf; LayerNorm / bn / emb in the full name), sizes that are
    and are not multiples of 256, a 2-D weight and a frozen parameter."""

    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(7)
        self.fc = _Leaf(gen, weight=(300,), bias=(7,))
        self.LayerNorm = _Leaf(gen, weight=(256,), bias=(256,))
        self.bn1 = _Leaf(gen, weight=(513,))
        self.emb = _Leaf(gen, weight=(1000,))
        self.proj = _Leaf(gen, weight=(20, 30))
        self.frozen = _Leaf(gen, weight=(40,))
        self.frozen.weight.requires_grad_(False)
        self._flat = None

    def native_flat(self):
        from vcg_hip.flat import FlatParams
        if self._flat is None:
            self._flat = FlatParams(list(self.named_parameters()), DEV, shadow_dtype=torch.bfloat16)
        return self._flat


DECAY = {"fc.weight", "proj.weight", "frozen.weight"}
GRAD_STD = [0.05, 0.01, 0.05, 0.01]  # ||g|| ~ 2.6 (clip active) and ~ 0.5 (inactive), alternating


def _toy_grads(model):
    gen = torch.Generator().manual_seed(11)
    return [{n: torch.randn(p.shape, generator=gen) * s for n, p in model.named_parameters() if p.requires_grad}
            for s in GRAD_STD]


def _ref_optim_run(dtype, grads):
    """torch.optim.AdamW + clip_grad_norm_(1.0) on a CPU copy of the toy in `dtype`, grouped by param_groups.
    Returns per step {name: (p, exp_avg, exp_avg_sq)} and the pre-clip gradient norms."""
    from vcg_hip.optim import param_groups
    model = _Toy().to(dtype)
    groups = param_groups(model, WD)
    opt = torch.optim.AdamW(groups, lr=LR, betas=BETAS, eps=EPS)
    named = dict(model.named_parameters())
    out, norms = [], []
    for g in grads:
        for n, p in named.items():
            p.grad = g[n].to(dtype).clone() if n in g else None
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(named.values()), 1.0)))
        opt.step()
        out.append({n: (p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                    for n, p in named.items() if p.requires_grad})
    return out, norms


def _gpu_toy(K):
    from vcg_hip.optim import FusedAdamW, param_groups
    model = _Toy().to(DEV)
    f = model.native_flat()
    f.refresh_shadow()  # as a forward would
    opt = FusedAdamW(param_groups(model, WD), lr=LR, betas=BETAS, eps=EPS, model=model)
    return model, f, opt


def _set_grads(model, g):
    for n, p in model.named_parameters():
        if n in g:
            p.grad.copy_(g[n])


def test_param_groups_split_of_the_toy():
    from vcg_hip.optim import param_groups
    model = _Toy()
    names = {id(p): n for n, p in model.named_parameters()}
    decay, no_decay = param_groups(model, WD)
    assert {names[id(p)] for p in decay["params"]} == DECAY and decay["weight_decay"] == WD
    assert {names[id(p)] for p in no_decay["params"]} == set(names.values()) - DECAY
    assert no_decay["weight_decay"] == 0.0


def test_fused_adamw_vs_fp64_and_resume(K):
    grads = _toy_grads(_Toy())
    ref64, norms64 = _ref_optim_run(torch.float64, grads)
    ref32, _ = _ref_optim_run(torch.float32, grads)
    assert norms64[0] > 1.5 and norms64[1] < 0.8, norms64  # both clip regimes occur

    model, f, opt = _gpu_toy(K)
    named = dict(model.named_parameters())
    init = {n: p.detach().clone() for n, p in named.items()}
    fz = named["frozen.weight"]
    fo = None
    saved = None
    trace = []
    for t, g in enumerate(grads, 1):
        _set_grads(model, g)
        gn = opt.grad_norm().item()
        # test_sumsq's bound on the sum of squares is 1e-5 relative; the square root halves it (+ two fp32 roundings)
        assert abs(gn - norms64[t - 1]) <= (0.5e-5 + 2 ** -23) * norms64[t - 1], (gn, norms64[t - 1])
        opt.clip_and_step(1.0)
        torch.cuda.synchronize()
        if fo is None:
            fo = f.offset_of(fz)
        for n, p in named.items():
            st = opt.state[p]
            assert float(st["step"]) == t, (n, st["step"])
            if not p.requires_grad:
                continue
            r64, r32 = ref64[t - 1][n], ref32[t - 1][n]
            i0 = init[n].double().cpu()
            _check(p.detach().double().cpu() - i0, r64[0] - i0, r32[0].double() - i0, f"step {t} {n} p - p0")
            _check(p.detach(), r64[0], r32[0], f"step {t} {n} p")
            _check(st["exp_avg"], r64[1], r32[1], f"step {t} {n} exp_avg")
            _check(st["exp_avg_sq"], r64[2], r32[2], f"step {t} {n} exp_avg_sq")
        # the frozen parameter, its moments and its shadow never move
        assert torch.equal(fz.detach(), init["frozen.weight"])
        assert opt.state[fz]["exp_avg"].abs().max().item() == 0 and opt.state[fz]["exp_avg_sq"].abs().max().item() == 0
        assert torch.equal(f.shadow[fo:fo + fz.numel()].view(torch.int16),
                           init["frozen.weight"].to(torch.bfloat16).view(torch.int16))
        assert torch.equal(f.shadow.view(torch.int16), f.data.to(torch.bfloat16).view(torch.int16))
        trace.append({n: (p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                      for n, p in named.items()})
        if t == 2:
            saved = (copy.deepcopy(opt.state_dict()), {n: p.detach().clone() for n, p in named.items()})

    # resume after step 2 in a fresh module + optimiser: steps 3-4 reproduce the uninterrupted run bit for bit
    sd, params2 = saved
    model2, f2, opt2 = _gpu_toy(K)
    named2 = dict(model2.named_parameters())
    with torch.no_grad():
        for n, p in named2.items():
            p.copy_(params2[n])
    f2.refresh_shadow(force=True)
    opt2.load_state_dict(sd)
    for t in (3, 4):
        _set_grads(model2, grads[t - 1])
        opt2.clip_and_step(1.0)
        torch.cuda.synchronize()
        for n, p in named2.items():
            a = trace[t - 1][n]
            assert float(opt2.state[p]["step"]) == t
            assert torch.equal(p.detach(), a[0]), f"resumed step {t}: {n} differs"
            assert torch.equal(opt2.state[p]["exp_avg"], a[1]), f"resumed step {t}: {n} exp_avg differs"
            assert torch.equal(opt2.state[p]["exp_avg_sq"], a[2]), f"resumed step {t}: {n} exp_avg_sq differs"
    assert torch.equal(f2.shadow.view(torch.int16), f2.data.to(torch.bfloat16).view(torch.int16))
