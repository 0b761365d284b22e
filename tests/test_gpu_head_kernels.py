"""Kernel-level numerics of the MLP fusion head and the cross-entropy (csrc/head.hip) against plain fp64 torch on the
CPU: logits = cat([Vout.view(B, -1), Lout], 1) W^T + b, its softmax, the backward with and without the ReLU mask of
the projections in front of it, and the mean cross-entropy with its gradient, including logits at +-80.

References are built from the same, already storage-rounded, inputs; backwards come from torch.autograd.grad.
Tolerances are those of tests/test_gpu_kernels.py: max abs error <= 2e-5 x max|ref| for fp32 storage (logits, prob,
dW, dbias, the loss: fp32 accumulators of already-rounded operands), 2e-2 x max|ref| for bf16 storage (dV, dL).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]


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


# ============================================================================ MLP head
# (B, T, hid, O); the last: B * D = 2100 * 512 > 4096 * 256, the dF kernel's grid-stride loop wraps
HEAD_SHAPES = [(1, 1, 8, 2), (3, 5, 100, 2), (300, 3, 128, 16), (2100, 3, 128, 2)]


@functools.lru_cache(maxsize=None)
def _head_inputs(B, T, hid, O, dtype):
    """Vout / Lout as the ReLU projections leave them, except that negatives stay in too (about a third each of exact
    zeros, negatives and positives), so that relu_mask = 1 and relu_mask = 0 give different gradients."""
    g = torch.Generator().manual_seed(B * 1009 + T * 101 + hid + O)
    D = (T + 1) * hid

    def act(n):
        a = torch.randn(n, hid, generator=g)
        a[torch.rand(n, hid, generator=g) < 0.3] = 0.0
        return a.to(dtype)
    V, L = act(B * T), act(B)
    W = torch.randn(O, D, generator=g) / D ** 0.5
    b = torch.randn(O, generator=g) * 0.5
    dlogits = torch.randn(B, O, generator=g)
    return V, L, W, b, dlogits


def _head_ref(V, L, W, b, dlogits, B, relu_mask):
    Fm = torch.cat([V.double().view(B, -1), L.double()], 1).requires_grad_()
    Wd = W.double().requires_grad_()
    bd = (b.double() if b is not None else torch.zeros(W.shape[0], dtype=torch.float64)).requires_grad_()
    logits = Fm @ Wd.T + bd
    dF, dW, db = torch.autograd.grad(logits, (Fm, Wd, bd), dlogits.double())
    if relu_mask:
        dF = dF * (Fm.detach() > 0)
    TH = V.numel() // B
    return logits.detach(), torch.softmax(logits.detach(), 1), dF[:, :TH].reshape(V.shape), dF[:, TH:], dW, db


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=str)
def test_head_mlp_fwd(K, shape, dtype):
    """logits and prob against fp64; bias = NULL drops the bias; prob = NULL writes the same logits."""
    from vcg_hip import _lib
    B, T, hid, O = shape
    V, L, W, b, dlogits = _head_inputs(B, T, hid, O, dtype)
    logits_ref, prob_ref, *_ = _head_ref(V, L, W, b, dlogits, B, True)
    Vg, Lg, Wg, bg = (t.to(DEV) for t in (V, L, W, b))
    logits, prob = K.head_mlp_fwd(Vg, Lg, Wg, bg, B, T, hid, O)
    _close(logits, logits_ref, F32, f"head_mlp_fwd logits (x {_name(dtype)})")
    _close(prob, prob_ref, F32, f"head_mlp_fwd prob (x {_name(dtype)})")
    logits_nb, prob_nb = K.head_mlp_fwd(Vg, Lg, Wg, None, B, T, hid, O)
    nb_ref = _head_ref(V, L, W, None, dlogits, B, True)
    _close(logits_nb, nb_ref[0], F32, "head_mlp_fwd logits (no bias)")
    _close(prob_nb, nb_ref[1], F32, "head_mlp_fwd prob (no bias)")
    only = torch.full((B, O), float("nan"), device=DEV)
    _lib.call("vcg_head_mlp_fwd", K.dt_code(dtype), K.P(Vg), K.P(Lg), K.P(Wg), K.P(bg), K.P(only), None, B, T, hid, O,
              K.stream())
    assert torch.equal(only, logits), "prob = NULL changed the logits"


@pytest.mark.parametrize("relu_mask", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=str)
def test_head_mlp_bwd(K, shape, dtype, relu_mask):
    """dV / dL (exactly 0 where the ReLU mask closes), dW and dbias accumulated into prefilled buffers; dbias = NULL
    and dW = NULL leave the other outputs bit-identical."""
    B, T, hid, O = shape
    D = (T + 1) * hid
    V, L, W, b, dlogits = _head_inputs(B, T, hid, O, dtype)
    _, _, dV_ref, dL_ref, dW_ref, db_ref = _head_ref(V, L, W, b, dlogits, B, relu_mask)
    Vg, Lg, Wg, dg = (t.to(DEV) for t in (V, L, W, dlogits))
    dW, db = torch.full((O, D), 0.5, device=DEV), torch.full((O,), -0.25, device=DEV)
    dV, dL = K.head_mlp_bwd(Vg, Lg, Wg, dg, dW, db, B, T, hid, O, relu_mask=relu_mask)
    tag = _name(dtype)
    _close(dV, dV_ref, dtype, f"head_mlp_bwd dV {tag}")
    _close(dL, dL_ref, dtype, f"head_mlp_bwd dL {tag}")
    _close(dW.double() - 0.5, dW_ref, F32, f"head_mlp_bwd dW (x {tag})")
    _close(db.double() + 0.25, db_ref, F32, f"head_mlp_bwd dbias (x {tag})")
    if relu_mask:
        assert (dV.cpu()[V <= 0] == 0).all() and (dL.cpu()[L <= 0] == 0).all(), "gradient through a closed ReLU"
    else:
        assert (dV.cpu()[V <= 0] != 0).any(), "relu_mask = 0 must let the gradient through"
    dW2 = torch.full((O, D), 0.5, device=DEV)
    dV2, dL2 = K.head_mlp_bwd(Vg, Lg, Wg, dg, dW2, None, B, T, hid, O, relu_mask=relu_mask)
    assert torch.equal(dW2, dW) and torch.equal(dV2, dV) and torch.equal(dL2, dL), "dbias = NULL changed outputs"
    dV3, dL3 = K.head_mlp_bwd(Vg, Lg, Wg, dg, None, None, B, T, hid, O, relu_mask=relu_mask)
    assert torch.equal(dV3, dV) and torch.equal(dL3, dL), "dW = NULL changed dV / dL"


def test_head_mlp_refuses_17_outputs(K):
    """The forward keeps its logits in 16 LDS slots: O = 17 is VCG_ERR_INVALID, and nothing runs."""
    from vcg_hip._lib import VcgError
    B, T, hid, O = 2, 1, 8, 17
    V, L = torch.ones(B * T, hid, device=DEV), torch.ones(B, hid, device=DEV)
    W, b = torch.ones(O, (T + 1) * hid, device=DEV), torch.zeros(O, device=DEV)
    with pytest.raises(VcgError, match=r"\(-1\).*too many outputs"):
        K.head_mlp_fwd(V, L, W, b, B, T, hid, O)


# ============================================================================ cross-entropy
CE_SHAPES = [(1, 2), (257, 2), (300, 5), (1000, 3)]


def _ce_inputs(B, C, kind):
    g = torch.Generator().manual_seed(B * 31 + C)
    labels = torch.randint(0, C, (B,), generator=g)
    if kind == "unit":
        logits = torch.randn(B, C, generator=g)
    else:  # every logit at +80 or -80, one row of equal logits
        logits = torch.where(torch.rand(B, C, generator=g) < 0.5, 80.0, -80.0)
        logits[B // 2] = 80.0
    return logits, labels


@pytest.mark.parametrize("kind", ["unit", "pm80"])
@pytest.mark.parametrize("shape", CE_SHAPES, ids=str)
def test_cross_entropy(K, shape, kind):
    """Mean cross-entropy and its gradient against F.cross_entropy in fp64 (B > 256: the forward's row loop wraps,
    the backward takes a second block), with dloss = NULL (1) and a device scalar; finite at logits of +-80."""
    B, C = shape
    logits, labels = _ce_inputs(B, C, kind)
    ld = logits.double().requires_grad_()
    loss_ref = F.cross_entropy(ld, labels)
    (dl_ref,) = torch.autograd.grad(loss_ref, ld)
    lg, yg = logits.to(DEV), labels.to(DEV)
    loss = K.cross_entropy_fwd(lg, yg)
    assert torch.isfinite(loss).all()
    _close(loss, loss_ref, F32, f"cross_entropy_fwd loss ({kind})")
    for dloss, c in ((None, 1.0), (torch.tensor(0.37, device=DEV), 0.37)):
        dlogits = K.cross_entropy_bwd(lg, yg, dloss)
        assert torch.isfinite(dlogits).all()
        _close(dlogits, dl_ref * float(torch.tensor(c, dtype=torch.float32)), F32, f"cross_entropy_bwd ({kind})")
