"""Kernel-level tests of the listwise fine-tuning kernels (csrc/listnet.hip) through vcg_hip.ops, against float64 on the
CPU. The inputs are rounded to bf16 first and both storage types of P are run, so the float64 reference sees the same
numbers and what is measured is the kernels' own fp32 arithmetic (tests/test_gpu_contrast_kernels.py's convention).

Bound, for every output: max error against float64 <= max(5 E, 2e-5 scale), E the max error of the same formula
evaluated by torch in fp32 on the CPU and scale the float64 result's largest magnitude (5x is _check_grads' factor,
2e-5 is _close's). The loss and its two parts lie within 1e-4. dW / db are added into buffers prefilled with 0.5, dP is
written into a buffer prefilled with NaN (a row nobody wrote shows).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _formula(P, t, sel, cls, W, b, g, dtype):
    """Reference bert_hugface_listnet.py:148-176 on the CPU in `dtype`, and its gradients for the upstream scalar g."""
    P = P.to(dtype).requires_grad_()
    W = W.to(dtype).requires_grad_()
    b = b.to(dtype).requires_grad_()
    t = t.to(dtype)
    B, S = t.shape
    A = P.view(B, S, -1)
    z = torch.bmm(A[:, 0, :].unsqueeze(1), torch.transpose(A[:, 1:, :], 1, 2)).squeeze(1)
    p = F.softmax(z, dim=1)
    sur = torch.mean(-torch.sum(t[:, 1:] * torch.log(p + 1e-10), dim=1))
    y = F.linear(P[sel], W, b)
    q = F.softmax(y, dim=1)
    bce = F.cross_entropy(y, cls)
    loss = sur + bce
    loss.backward(torch.tensor(g, dtype=dtype))
    out = dict(loss=loss, surrogate=sur, binary=bce, logits=y, prob=q, p=p, dP=P.grad, dW=W.grad, db=b.grad)
    return {k: v.detach().double() for k, v in out.items()}


def _r(x):
    return x.to(torch.bfloat16).float()


def _inputs(name):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == "single":  # one contrast clip: p = 1 and the slate gradient is exactly 0
        B, S, H, up = 1, 2, 64, 1.0
        sel, cls = [1], [1]
    elif name == "reference":  # the reference's slate, hard targets [1, 1, 0, ...]
        B, S, H, up = 3, 12, 768, 1.0
        sel, cls = [1, 12 + 0, 24 + 7], [1, 1, 0]
    elif name == "soft":  # soft targets, one all-zero target row, duplicates in sel, a slate's row 0, g != 1
        B, S, H, up = 5, 33, 768, 0.37
        sel, cls = [0, 33, 33, 40, 70, 70, 70, 164, 100], [1, 1, 0, 0, 1, 1, 0, 0, 1]
    elif name == "max_slate":  # the stated upper limit of S
        B, S, H, up = 2, 64, 256, -1.5
        sel, cls = [63, 64], [0, 1]
    elif name == "saturated":  # z spans +-200: exp without the maximum subtracted overflows
        B, S, H, up = 2, 6, 768, 1.0
        sel, cls = [2, 6], [1, 0]
    else:
        raise KeyError(name)
    if name == "saturated":
        P = torch.zeros(B * S, H)
        sign = torch.tensor([1, 1, -1, 0, 1, -1, -1, -1, 1, 0, 1, -1], dtype=torch.float32)
        P[:, :200] = sign[:, None]
        P[4, 100:200] = 0   # z = 100
        P[5, 100:200] = 0   # z = -100
        P[10, 100:200] = 0
    else:
        P = torch.tanh(torch.randn(B * S, H, generator=g) * (0.3 if name == "reference" else 0.12))
    if name in ("soft", "saturated"):
        t = torch.rand(B, S, generator=g) * 0.7
        if name == "soft":
            t[2] = 0
    else:
        t = torch.zeros(B, S)
        t[:, :2] = 1
    W = torch.randn(2, H, generator=g) * (0.02 if name != "soft" else 0.2)
    b = torch.randn(2, generator=g) * 0.1
    return _r(P), _r(t), torch.tensor(sel), torch.tensor(cls), _r(W), _r(b), up


@functools.lru_cache(maxsize=None)
def _case(name):
    torch.set_num_threads(4)
    P, t, sel, cls, W, b, up = _inputs(name)
    r64 = _formula(P, t, sel, cls, W, b, up, torch.float64)
    r32 = _formula(P, t, sel, cls, W, b, up, torch.float32)
    e32 = {k: (r32[k] - r64[k]).abs().max().item() for k in r64}
    return dict(P=P, t=t, sel=sel, cls=cls, W=W, b=b, up=up, ref=r64, e32=e32)


def _run(c, dtype, sel=None, cls=None):
    """The kernels on case c -> dict of CPU results (dW / db with their 0.5 prefill taken off)."""
    from vcg_hip import ops
    P = c["P"].to(DEV, dtype)
    t, W, b = c["t"].to(DEV), c["W"].to(DEV), c["b"].to(DEV)
    sel = c["sel"] if sel is None else sel
    cls = c["cls"] if cls is None else cls
    loss3, logits, prob, p, idx = ops.listnet_fwd(P, t, sel, cls, W, b)
    dW = torch.full((2, P.shape[1]), 0.5, device=DEV)
    db = torch.full((2,), 0.5, device=DEV)
    dP = torch.full((P.shape[0], P.shape[1]), float("nan"), device=DEV)
    out = ops.listnet_bwd(P, t, idx, W, p, prob, torch.tensor([c["up"]], device=DEV), dW=dW, db=db, out=dP)
    assert out.data_ptr() == dP.data_ptr()
    torch.cuda.synchronize()
    return dict(loss=loss3[0].cpu(), surrogate=loss3[1].cpu(), binary=loss3[2].cpu(), logits=logits.cpu(),
                prob=prob.cpu(), p=p.cpu(), dP=dP.cpu(), dW=dW.cpu(), db=db.cpu())


CASES = ["single", "reference", "soft", "max_slate", "saturated"]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", CASES)
def test_listnet_against_float64(name, prec):
    c = _case(name)
    got = _run(c, DTYPES[prec])
    ref, e32 = c["ref"], c["e32"]
    for k in ("loss", "surrogate", "binary", "logits", "prob", "p", "dP", "dW", "db"):
        out = got[k].double()
        if k in ("dW", "db"):
            out = out - 0.5  # (added into the prefilled buffers)
        assert torch.isfinite(out).all(), f"{name} {k}: not finite (a dP row nobody wrote is NaN)"
        scale = ref[k].abs().max().item() + 1e-6
        err = (out - ref[k]).abs().max().item()
        bound = max(5 * e32[k], 2e-5 * scale)
        print(f"{name} {prec} {k}: err {err:.3e}  fp32-torch {e32[k]:.3e}  scale {scale:.3e}  "
              f"ratio to bound {err / bound:.3f}")
        assert err <= bound, f"{name} {prec} {k}: err {err:.3e} > {bound:.3e}"
        if k in ("loss", "surrogate", "binary"):
            assert err <= 1e-4
    assert got["dP"].dtype == torch.float32 and got["logits"].dtype == torch.float32


def test_single_contrast_clip_has_zero_slate_gradient():
    c = _case("single")
    for dt in DTYPES.values():
        got = _run(c, dt)
        assert got["p"].item() == 1.0
        assert got["surrogate"].item() == 0.0  # -1 * log(1 + 1e-10) in fp32
        assert (got["dP"][0] == 0).all()  # row 0 is not selected: only the slate term, exactly 0
        assert (c["ref"]["dP"][0] == 0).all()


def test_saturated_probabilities():
    c = _case("saturated")
    got = _run(c, torch.bfloat16)
    assert torch.isfinite(got["loss"]) and torch.isfinite(got["p"]).all()
    # slate 0: z = (200, -200, 0, 100, -100) -> p = (1, 0, e^-200, e^-100, 0)
    assert got["p"][0, 0].item() == pytest.approx(1.0, abs=1e-6) and got["p"][0, 1].item() == 0.0
    assert (got["p"].double() - c["ref"]["p"]).abs().max().item() <= 2e-5


def test_duplicates_add():
    """sel = [r, r] gives twice the head gradient of sel = [r] at half the 1 / M."""
    c = _case("reference")
    one = _run(c, torch.float32, sel=torch.tensor([5]), cls=torch.tensor([1]))
    two = _run(c, torch.float32, sel=torch.tensor([5, 5]), cls=torch.tensor([1, 1]))
    assert torch.allclose(two["dW"], one["dW"], rtol=1e-6, atol=1e-9)
    assert torch.allclose(two["dP"], one["dP"], rtol=1e-5, atol=1e-9)
    assert torch.equal(two["logits"][0], one["logits"][0]) and torch.equal(two["logits"][1], one["logits"][0])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_two_runs_equal_bits(prec):
    c = _case("soft")
    a, b = _run(c, DTYPES[prec]), _run(c, DTYPES[prec])
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_device_indices_are_checked_too():
    c = _case("reference")
    a = _run(c, torch.float32)
    b = _run(c, torch.float32, sel=c["sel"].to(DEV), cls=c["cls"].to(DEV))
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _refusal_args(B=2, S=4, H=64, sel=(1,), cls=(0,)):
    P = torch.zeros(B * S, H, device=DEV)
    t = torch.zeros(B, S, device=DEV)
    return P, t, torch.tensor(sel, dtype=torch.int64), torch.tensor(cls, dtype=torch.int64), \
        torch.zeros(2, H, device=DEV), torch.zeros(2, device=DEV)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kw,text", [
    (dict(S=1), "slate length 1"),
    (dict(S=65), "slate length 65"),
    (dict(H=60), "hidden size 60"),
    (dict(H=8200), "hidden size 8200"),
    (dict(B=0), "batch size 0"),
    (dict(sel=(), cls=()), "0 selected rows"),
    (dict(sel=(-1,)), "selected row -1"),
    (dict(sel=(3, 8), cls=(0, 1)), "selected row 8 outside [0, 8)"),
    (dict(cls=(2,)), "binary label 2"),
    (dict(cls=(-1,)), "binary label -1"),
])
def test_refusals_launch_nothing(kw, text, on_device, monkeypatch):
    from vcg_hip import ops
    ops.listnet_limits()  # (loads the library before the recorder goes in)
    P, t, sel, cls, W, b = _refusal_args(**kw)
    if on_device:
        sel, cls = sel.to(DEV), cls.to(DEV)
    launched = []
    monkeypatch.setattr(ops._lib, "call", lambda name, *a: launched.append(name))
    with pytest.raises(ValueError) as e:
        ops.listnet_fwd(P, t, sel, cls, W, b)
    assert text in str(e.value), str(e.value)
    assert launched == []


def test_limits_are_stated():
    from vcg_hip import ops
    max_s, max_h = ops.listnet_limits()
    assert max_s >= 64 and max_h >= 768
    ops.listnet_check_shape(1, max_s, 768, 1)
    ops.listnet_check_shape(1, 2, 64, 1)
    with pytest.raises(ValueError):
        ops.listnet_check_shape(1, max_s + 1, 768, 1)
