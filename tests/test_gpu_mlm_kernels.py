"""Kernel-level tests of the masked-LM vocabulary head (csrc/mlm_head.hip) through vcg_hip.ops / ctypes, against float64
on the CPU. The inputs are rounded to bf16 first, so the float64 reference sees the same numbers and what is measured is
the kernels' own fp32 accumulation.

Bounds: lse and the mean loss within 1e-4 (the project's loss bound; bf16 operands with fp32 accumulation over K = 768
give ~1e-5). n_correct is compared on the rows whose float64 top-1 / top-2 gap exceeds 1e-3 (at most 2 % of the rows may
fall under it). dX / dW as relative Frobenius error against float64: <= max(1.5 E, floor), E the error of torch's CPU
autocast(bf16) F.linear + F.cross_entropy on the same numbers, the floor 0.0 (test_gpu_bf16_train.py's floor for the
language model's gradients). Each dZ row sums to 0 within its bf16 rounding: every element carries at most 2^-9 of
itself and a row's absolute values sum to at most 2 dloss / R, plus 1e-4 dloss / R for the fp32 exponentials and lse.
"""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = 0.5  # the mean loss' incoming gradient
# (R, V, H, where the targets sit)
CASES = [(1, 1210, 256, "rand"), (37, 1210, 768, "first_last"), (300, 1210, 768, "last_tile"),
         (37, 30522, 768, "rand")]
IDS = [f"R{r}-V{v}-H{h}-{k}" for r, v, h, k in CASES]


def _close(out, ref, what=""):  # tests/test_gpu_kernels.py's fp32 criterion
    out = out.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = ref.abs().max().item() + 1e-6
    err = (out - ref).abs().max().item()
    assert err <= 2e-5 * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _rel(a, b):
    return (a.double().cpu() - b).norm().item() / max(b.norm().item(), 1e-300)


@functools.lru_cache(maxsize=None)
def _case(R, V, H, kind):
    """Inputs (bf16-rounded) and the float64 / CPU-autocast references of one case; computed once, never modified."""
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    g = torch.Generator().manual_seed(1000 + R + V + H)
    total = R + 13  # hidden has more rows than R
    X = torch.randn((total, H), generator=g).to(torch.bfloat16)
    W = (torch.randn((V, H), generator=g) * (0.5 / H ** 0.5)).to(torch.bfloat16)  # logit sigma ~ 0.5
    rows = torch.randperm(total, generator=g)[:R].contiguous()  # non-monotonic
    x64 = X.double()[rows]
    z = x64 @ W.double().t()
    top2 = z.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3
    if kind == "first_last":
        t = torch.where(torch.arange(R) % 2 == 0, 0, V - 1)
    elif kind == "last_tile":  # the last, partial 128-column tile
        t = torch.randint(V // 128 * 128, V, (R,), generator=g)
    else:
        t = torch.randint(0, V, (R,), generator=g)
        t[::2] = z.argmax(1)[::2]  # half of the rows are predicted correctly
    t = t.to(torch.int64)
    lse = torch.logsumexp(z, 1)
    row_loss = lse - z.gather(1, t[:, None])[:, 0]
    correct = z.argmax(1) == t
    dz = (torch.softmax(z, 1) - F.one_hot(t, V).double()) * (G / R)
    dX, dW = dz @ W.double(), dz.t() @ x64
    # the same computation by torch under CPU autocast(bf16): the yardstick E
    xa, wa = X.float()[rows].requires_grad_(), W.float().requires_grad_()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        la = F.cross_entropy(F.linear(xa, wa), t)
    (la * G).backward()
    return dict(X=X, W=W, rows=rows, t=t, lse=lse, row_loss=row_loss, loss=row_loss.mean().item(), clear=clear, correct=correct, dX=dX,
                dW=dW, e_dx=_rel(xa.grad, dX), e_dw=_rel(wa.grad, dW))


def _dev(c):
    return c["X"].to(DEV), c["W"].to(DEV), c["rows"].to(DEV), c["t"].to(DEV)


@pytest.mark.parametrize("R,V,H,kind", CASES, ids=IDS)
def test_mlm_loss_forward(R, V, H, kind):
    from vcg_hip import ops
    c = _case(R, V, H, kind)
    X, W, rows, t = _dev(c)
    lse, row_loss, loss, n_correct = ops.mlm_loss_fwd(X, rows, W, t)
    e_lse = (lse.double().cpu() - c["lse"]).abs().max().item()
    e_loss = abs(loss.item() - c["loss"])
    print(f"lse err {e_lse:.3e} loss err {e_loss:.3e} n_correct {n_correct.item()} ref {int(c['correct'].sum())}")
    assert e_lse <= 1e-4 and e_loss <= 1e-4
    assert (row_loss.double().cpu() - c["row_loss"]).abs().max().item() <= 1e-4  # (the target's logit was found)
    # two runs are bit-identical
    lse2, row_loss2, loss2, n2 = ops.mlm_loss_fwd(X, rows, W, t)
    assert torch.equal(lse, lse2) and torch.equal(row_loss, row_loss2) and torch.equal(loss, loss2)
    assert torch.equal(n_correct, n2)
    # the argmax count over the rows with a clear float64 top-1
    clear = c["clear"]
    assert (~clear).float().mean().item() <= 0.02
    if clear.any():
        keep = clear.to(DEV)
        _, _, _, nc = ops.mlm_loss_fwd(X, rows[keep].contiguous(), W, t[keep].contiguous())
        assert nc.item() == int(c["correct"][clear].sum())
        if kind == "rand":
            assert nc.item() >= int(clear[::2].sum())  # (the test has rows that are predicted correctly)


@pytest.mark.parametrize("R,V,H,kind", CASES, ids=IDS)
def test_mlm_loss_backward(R, V, H, kind):
    from vcg_hip import ops
    c = _case(R, V, H, kind)
    X, W, rows, t = _dev(c)
    lse, _, _, _ = ops.mlm_loss_fwd(X, rows, W, t)
    dloss = torch.full((), G, dtype=torch.float32, device=DEV)
    Vp = ops.mlm_vp(V)
    dZ = ops.mlm_loss_bwd(X, rows, W, t, lse, dloss)
    assert dZ.shape == (R, Vp) and dZ.dtype == torch.bfloat16
    assert (dZ[:, V:] == 0).all()  # pad columns are exactly 0
    rs = dZ.double().sum(1).abs().max().item()
    bound = (2 ** -9 * 2 + 1e-4) * G / R
    print(f"max |row sum of dZ| {rs:.3e} (bound {bound:.3e})")
    assert rs <= bound
    xg = X.index_select(0, rows)
    dX = torch.empty((R, H), dtype=torch.float32, device=DEV)
    ops.gemm_splitk(dZ, W, dX, R, H, V, Vp, H, transA=False, transB=True, accumulate=False)
    dW = torch.zeros((V, H), dtype=torch.float32, device=DEV)
    ops.gemm_splitk(dZ, xg, dW, V, H, R, Vp, H, transA=True, transB=True, accumulate=True)
    e_dx, e_dw = _rel(dX, c["dX"]), _rel(dW, c["dW"])
    print(f"dX rel err {e_dx:.3e} (autocast {c['e_dx']:.3e})  dW rel err {e_dw:.3e} (autocast {c['e_dw']:.3e})")
    floor = 0.0
    assert e_dx <= max(1.5 * c["e_dx"], floor)
    assert e_dw <= max(1.5 * c["e_dw"], floor)


@pytest.mark.parametrize("R,V,H,kind", CASES[:2], ids=IDS[:2])
def test_mlm_f32_reduce_matches(R, V, H, kind):
    """The fp32 parity path: logits in memory -> the same partial / finalize reduction, and dZ in place."""
    from vcg_hip import ops
    c = _case(R, V, H, kind)
    X, W, rows, t = _dev(c)
    Vp = ops.mlm_vp(V)
    z = torch.zeros((R, Vp), dtype=torch.float32, device=DEV)
    z[:, :V] = (c["X"].double()[c["rows"]] @ c["W"].double().t()).float().to(DEV)
    lse, row_loss, loss, n_correct = ops.mlm_reduce_f32(z, V, t)
    assert (lse.double().cpu() - c["lse"]).abs().max().item() <= 1e-4
    assert abs(loss.item() - c["loss"]) <= 1e-4
    dz = ops.mlm_dz_f32(z, V, lse, t, torch.full((), G, dtype=torch.float32, device=DEV))
    assert (dz[:, V:] == 0).all()
    ref = (c["dX"], c["dW"])
    assert _rel(dz[:, :V].double().cpu() @ c["W"].double(), ref[0]) <= 1e-5


def test_mlm_k_tail():
    """H = 72 is one 64-wide k stage plus one 8-wide chunk: the zero-filled k tail of the tile loop, which no H that is
    a multiple of 64 reaches. 70 rows are a partial second row block, 200 columns a partial second column tile. Only the
    tile kernels run (no GEMM). dZ elementwise against float64: 2^-8 of the value for the bf16 rounding plus the
    module's 1e-4 G / R for the fp32 exponentials and lse."""
    from vcg_hip import ops
    R, V, H = 70, 200, 72
    c = _case(R, V, H, "rand")
    X, W, rows, t = _dev(c)
    lse, row_loss, loss, n_correct = ops.mlm_loss_fwd(X, rows, W, t)
    e_lse = (lse.double().cpu() - c["lse"]).abs().max().item()
    e_row = (row_loss.double().cpu() - c["row_loss"]).abs().max().item()
    e_loss = abs(loss.item() - c["loss"])
    print(f"lse err {e_lse:.3e} row loss err {e_row:.3e} loss err {e_loss:.3e} n_correct {n_correct.item()}")
    assert e_lse <= 1e-4 and e_row <= 1e-4 and e_loss <= 1e-4
    clear = c["clear"]
    assert (~clear).float().mean().item() <= 0.02
    keep = clear.to(DEV)
    nc = ops.mlm_loss_fwd(X, rows[keep].contiguous(), W, t[keep].contiguous())[3]
    assert nc.item() == int(c["correct"][clear].sum())

    dZ = ops.mlm_loss_bwd(X, rows, W, t, lse, torch.full((), G, dtype=torch.float32, device=DEV))
    z64 = c["X"].double()[c["rows"]] @ c["W"].double().t()
    dz64 = (torch.softmax(z64, 1) - F.one_hot(c["t"], V).double()) * (G / R)
    err = (dZ[:, :V].double().cpu() - dz64).abs()
    bound = 2 ** -8 * dz64.abs() + 1e-4 * G / R
    print(f"dZ max err {err.max().item():.3e}, worst err / bound {(err / bound).max().item():.3f}")
    assert dZ.shape == (R, ops.mlm_vp(V)) and (err <= bound).all()

    zl = ops.mlm_logits(X, W)  # every hidden row, the identity gather
    assert zl.shape == (R + 13, ops.mlm_vp(V))
    e_z = (zl[:, :V].double().cpu() - c["X"].double() @ c["W"].double().t()).abs().max().item()
    print(f"logits err {e_z:.3e}")
    assert e_z <= 1e-4


@pytest.mark.parametrize("B,L,V,ld", [(3, 5, 1210, 1210), (3, 5, 1210, 1216), (2, 50, 30522, 30528)])
def test_seq_softmax(B, L, V, ld):
    from vcg_hip import ops
    g = torch.Generator().manual_seed(B * L + V)
    z = torch.zeros((B, L, ld), dtype=torch.float32)
    z[..., :V] = torch.randn((B, L, V), generator=g) * 2.0
    ref = torch.softmax(z[..., :V].double(), dim=1)
    prob = ops.seq_softmax_fwd(z.to(DEV), B, L, V, ldz=ld)
    assert prob.shape == (B, L, V)
    _close(prob, ref, "seq softmax")
    assert (prob.double().sum(1) - 1).abs().max().item() <= 1e-6


def test_seq_softmax_long():
    """L above the in-register limit (64) takes the two-read kernel."""
    from vcg_hip import ops
    B, L, V = 2, 70, 300
    z = torch.randn((B, L, V), generator=torch.Generator().manual_seed(5))
    prob = ops.seq_softmax_fwd(z.to(DEV), B, L, V)
    _close(prob, torch.softmax(z.double(), dim=1), "seq softmax L=70")
    assert (prob.double().sum(1) - 1).abs().max().item() <= 1e-6


def test_mlm_shape_limits():
    from vcg_hip import _lib, ops
    R, V = 4, 300
    t = torch.zeros(R, dtype=torch.int64, device=DEV)
    sentinel = torch.full((R,), -7.0, dtype=torch.float32, device=DEV)
    work = ops.ws(1 << 20, DEV)
    lib = _lib.lib()
    s = ops.stream()
    for H in (100, 4104):  # not a multiple of 8; above the limit
        X = torch.zeros((R, H), dtype=torch.bfloat16, device=DEV)
        W = torch.zeros((V, H), dtype=torch.bfloat16, device=DEV)
        rc = lib.vcg_mlm_loss_fwd(X.data_ptr(), R, None, W.data_ptr(), t.data_ptr(), R, V, H, work.data_ptr(),
                                  work.numel() * 4, sentinel.data_ptr(), None, None, None, s)
        assert rc == -2  # VCG_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert (sentinel == -7.0).all()  # nothing ran
    H = 64
    X = torch.zeros((R, H), dtype=torch.bfloat16, device=DEV)
    W = torch.zeros((V, H), dtype=torch.bfloat16, device=DEV)
    need = lib.vcg_mlm_loss_ws_bytes(R, V, H)
    assert need > 0
    rc = lib.vcg_mlm_loss_fwd(X.data_ptr(), R, None, W.data_ptr(), t.data_ptr(), R, V, H, work.data_ptr(), need - 4,
                              sentinel.data_ptr(), None, None, None, s)
    assert rc != 0 and "workspace" in _lib.last_error()
    torch.cuda.synchronize()
    assert (sentinel == -7.0).all()
