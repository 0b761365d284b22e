"""Kernel-level tests of the MoCo pre-training kernels (csrc/contrast.hip) through vcg_hip.ops, against float64 on the
CPU. The inputs are rounded to bf16 first, so the float64 reference sees the same numbers and what is measured is the
kernels' own fp32 arithmetic.

Bounds: the momentum update and the enqueue are bit-exact. The fp32 mode meets tests/test_gpu_kernels.py's fp32
criterion (max error <= 2e-5 of the reference's scale). lse, per-row loss and mean loss within 1e-4 (the project's
loss bound). n_correct / the selected candidates are compared where the float64 reference has a clear winner (top-1 /
top-2 gap above 1e-3 in logits, 1e-2 in cosine), which the cases are built to have. bf16 results as errors against
float64 <= max(1.5 E, floor), E the error of torch's CPU autocast(bf16) on the same numbers, the floor 0.0
(tests/test_gpu_mlm_kernels.py's convention).
"""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
T = 0.07
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _close(out, ref, what=""):  # tests/test_gpu_kernels.py's fp32 criterion
    out = out.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = ref.abs().max().item() + 1e-6
    err = (out - ref).abs().max().item()
    print(f"{what}: max err {err:.3e} vs scale {scale:.3e}")
    assert err <= 2e-5 * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _rel(a, b):
    return (a.double().cpu() - b).norm().item() / max(b.norm().item(), 1e-300)


def _maxerr(a, b):
    return (a.double().cpu() - b).abs().max().item()


def _threads():
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))


# ------------------------------------------------------------------------------------------------ momentum update
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", [1, 255, 256 + 3, 1000003])
def test_momentum_update(n, off):
    from vcg_hip import ops
    m = 0.999
    g = torch.Generator().manual_seed(n + off)
    pad = 8
    kb = torch.randn(n + off + pad, generator=g) * torch.rand(n + off + pad, generator=g).mul(4).exp()
    qb = torch.randn(n + off + pad, generator=g)
    want = kb[off:off + n] * m + qb[off:off + n] * (1. - m)  # the reference's expression, on the CPU
    kd, qd = kb.to(DEV), qb.to(DEV)
    sh = torch.full((n + off + pad,), -3.0, dtype=torch.bfloat16, device=DEV)
    ops.momentum_update(kd[off:off + n], qd[off:off + n], m, sh[off:off + n])
    assert torch.equal(kd[off:off + n].cpu(), want)  # bit for bit
    assert torch.equal(sh[off:off + n].cpu(), want.to(torch.bfloat16))
    assert torch.equal(qd.cpu(), qb)  # the query span is untouched
    assert torch.equal(kd[:off].cpu(), kb[:off]) and torch.equal(kd[off + n:].cpu(), kb[off + n:])  # nothing outside
    assert (sh[:off] == -3.0).all() and (sh[off + n:] == -3.0).all()
    # fp32 mode: no shadow
    kd2 = kb.to(DEV)
    ops.momentum_update(kd2[off:off + n], qd[off:off + n], m)
    assert torch.equal(kd2.cpu()[off:off + n], want)


# ------------------------------------------------------------------------------------------------ normalisation
def _norm_ref(x64, g64, eps=1e-12):
    d = x64.norm(dim=1, keepdim=True).clamp_min(eps)
    y = x64 / d
    return y, (g64 - y * (y * g64).sum(1, keepdim=True)) / d


@functools.lru_cache(maxsize=None)
def _norm_case(N, H, zero_row):
    _threads()
    g = torch.Generator().manual_seed(N * 1000 + H)
    x = (torch.randn((N, H), generator=g) * 0.7).to(torch.bfloat16)
    if zero_row:
        x[N // 2] = 0
    gy = torch.randn((N, H), generator=g).to(torch.bfloat16)
    y64, dx64 = _norm_ref(x.double(), gy.double())
    if not zero_row:  # the formula is F.normalize's derivative
        xa = x.double().requires_grad_()
        F.normalize(xa, dim=1).backward(gy.double())
        assert (xa.grad - dx64).abs().max().item() <= 1e-12 * dx64.abs().max().item()
    xb = x.clone().requires_grad_()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        yb = F.normalize(xb, dim=1)
    yb.backward(gy.to(yb.dtype))
    return dict(x=x, gy=gy, y=y64, dx=dx64, e_y=_maxerr(yb.detach(), y64), e_dx=_maxerr(xb.grad, dx64))


NORM_CASES = [(1, 256, False), (37, 768, False), (70, 768, False), (3, 768, True)]


@pytest.mark.parametrize("N,H,zero_row", NORM_CASES)
def test_l2norm_fp32(N, H, zero_row):
    from vcg_hip import ops
    c = _norm_case(N, H, zero_row)
    x = c["x"].float().to(DEV)
    y, denom = ops.l2norm_fwd(x)
    _close(y, c["y"], "normalize fwd")
    dx = ops.l2norm_bwd(c["gy"].float().to(DEV), x, denom)
    _close(dx, c["dx"], "normalize bwd")
    if zero_row:
        assert denom[N // 2].item() == pytest.approx(1e-12, rel=1e-6) and (y[N // 2] == 0).all()


@pytest.mark.parametrize("N,H,zero_row", NORM_CASES)
def test_l2norm_bf16(N, H, zero_row):
    from vcg_hip import ops
    c = _norm_case(N, H, zero_row)
    x = c["x"].to(DEV)
    y, denom = ops.l2norm_fwd(x)
    assert y.dtype == torch.bfloat16
    dx = ops.l2norm_bwd(c["gy"].float().to(DEV), x, denom)
    e_y, e_dx = _maxerr(y, c["y"]), _maxerr(dx, c["dx"])
    print(f"fwd err {e_y:.3e} (autocast {c['e_y']:.3e})  bwd err {e_dx:.3e} (autocast {c['e_dx']:.3e})")
    assert e_y <= 1.5 * c["e_y"] and e_dx <= 1.5 * c["e_dx"]


def test_l2norm_autograd():
    from vcg_hip.contrast import L2NormFn
    c = _norm_case(37, 768, False)
    x = c["x"].float().to(DEV).requires_grad_()
    L2NormFn.apply(x).backward(c["gy"].float().to(DEV))
    _close(x.grad, c["dx"], "L2NormFn")


# ------------------------------------------------------------------------------------------------ selection
@functools.lru_cache(maxsize=None)
def _select_case(B, C, H=768):
    """B rows of candidates normalize(a_c q + noise) with distinct a_c (the noise orthogonal to q, of unit length), each
    scaled by its own magnitude so the norms matter; then ONE extra row, row B, whose two best candidates are identical
    vectors. -> (q [B + 1, H], cand [B + 1, C, H], the expected indices [B + 1])."""
    _threads()
    R = B + 1
    g = torch.Generator().manual_seed(77 + B * 10 + C)
    q = F.normalize(torch.randn((R, H), generator=g), dim=1)
    a = torch.stack([0.3 * (1 + torch.randperm(C, generator=g)) for _ in range(R)]).float()  # [R, C], distinct per row
    noise = torch.randn((R, C, H), generator=g)
    noise = F.normalize(noise - (noise * q[:, None]).sum(-1, keepdim=True) * q[:, None], dim=-1)
    cand = F.normalize(a[..., None] * q[:, None] + noise, dim=-1) * (0.5 + 2.5 * torch.rand((R, C, 1), generator=g))
    q = (q * 1.7).to(torch.bfloat16)
    cand = cand.to(torch.bfloat16)
    best = int(a[B].argmax())
    other = (best + 1) % C  # the tie: the best vector copied over another candidate of the extra row
    cand[B, other] = cand[B, best]
    cos = F.cosine_similarity(cand.double(), q.double()[:, None], dim=-1)
    top2 = cos.topk(2, dim=1).values
    gap = top2[:, 0] - top2[:, 1]
    assert gap[B].item() == 0.0
    assert (gap[:B] > 1e-2).all()  # every planted float64 top-1 / top-2 cosine gap exceeds 1e-2
    want = cos.argmax(1)
    assert torch.equal(want[:B], a[:B].argmax(1))  # (the planted winner)
    want[B] = min(best, other)
    return q, cand, want


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,C", [(1, 2), (37, 6), (64, 6)])
def test_select(B, C, prec):
    from vcg_hip import ops
    q, cand, want = _select_case(B, C)
    dt = DTYPES[prec]
    k0 = ops.contrast_select(q.to(dt).to(DEV), cand.to(dt).to(DEV).contiguous())
    assert k0.dtype == torch.int64 and torch.equal(k0.cpu(), want)


# ------------------------------------------------------------------------------------------------ queue
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("N,K,ptr0,steps", [(5, 1210, 1200, 3), (64, 128, 64, 2)])
def test_enqueue_and_rebuild(N, K, ptr0, steps, prec):
    from vcg_hip import ops
    H, dt = 768, DTYPES[prec]
    g = torch.Generator().manual_seed(N + K)
    queue = F.normalize(torch.randn((H, K), generator=g), dim=0)
    qd = queue.to(DEV)
    km = ops.queue_rebuild(qd, dt)
    Kp = ops.queue_kp(K)
    assert km.shape == (Kp, H) and km.dtype == dt
    assert torch.equal(km[:K].cpu(), queue.t().to(dt)) and (km[K:] == 0).all()  # transpose + RNE cast, zero pad rows
    ptr = torch.tensor([ptr0], dtype=torch.int64, device=DEV)
    ref_q, ref_km, p = queue.clone(), queue.t().to(dt).clone(), ptr0
    for s in range(steps):
        keys = F.normalize(torch.randn((N, H), generator=g), dim=1)  # fp32 keys: queue_km receives the rounding
        ops.queue_enqueue(keys.to(DEV), qd, km, ptr)
        ref_q[:, p:p + N] = keys.t()
        ref_km[p:p + N] = keys.to(dt)
        p = (p + N) % K
        assert torch.equal(qd.cpu(), ref_q)  # the slice bit-exact, everything else unchanged
        assert torch.equal(km[:K].cpu(), ref_km) and (km[K:] == 0).all()
        assert ptr.item() == p
    assert p == (ptr0 + steps * N) % K and (N != 5 or p == 5)  # (N = 5: the pointer wrapped to 0, then moved to 5)
    if prec == "bf16":  # keys already in the compute dtype (the model's route)
        keys = F.normalize(torch.randn((N, H), generator=g), dim=1).to(dt)
        ops.queue_enqueue(keys.to(DEV), qd, km, ptr)
        assert torch.equal(qd[:, p:p + N].cpu(), keys.float().t()) and torch.equal(km[p:p + N].cpu(), keys)


def test_enqueue_rejects_bad_sizes():
    from vcg_hip import _lib, ops
    H, K = 256, 1210
    qd = torch.zeros((H, K), device=DEV)
    km = ops.queue_rebuild(qd, torch.bfloat16)
    ptr = torch.tensor([1200], dtype=torch.int64, device=DEV)
    for N in (7, 1211 * 2):  # K % N != 0; N > K
        keys = torch.ones((N, H), device=DEV)
        with pytest.raises(_lib.VcgError, match="multiple"):
            ops.queue_enqueue(keys, qd, km, ptr)
        torch.cuda.synchronize()
        assert (qd == 0).all() and (km == 0).all() and ptr.item() == 1200  # nothing written
    # a pointer that would run past the end writes nothing either
    ptr.fill_(1208)
    ops.queue_enqueue(torch.ones((5, H), device=DEV), qd, km, ptr)
    torch.cuda.synchronize()
    assert (qd == 0).all() and (km == 0).all() and ptr.item() == 1208


def test_outside_write_to_queue_is_seen():
    """After a direct write to model.queue (the version counter moves), the next loss uses the new values."""
    from vcg_hip import ops
    from vcg_hip.build import build_contrast_model
    from vcg_hip.nn import BertConfig
    cfg = BertConfig(vocab_size=1200, num_hidden_layers=1, max_position_embeddings=32)
    model = build_contrast_model(seed=5, device=DEV, precision="bf16", K=128, config=cfg)
    g = torch.Generator().manual_seed(9)
    q = F.normalize(torch.randn((4, 768), generator=g), dim=1).to(torch.bfloat16).to(DEV)
    k = F.normalize(torch.randn((4, 768), generator=g), dim=1).to(torch.bfloat16).to(DEV)

    def loss():
        return ops.infonce(q, k, model._operand_queue(), 128, 1 / T)[2].item()

    km = model._operand_queue()
    assert km is model._operand_queue()  # no rebuild while nothing changed
    l0 = loss()
    with torch.no_grad():
        model.queue[:, 7] = q[0].float() * 0.9  # a key close to query 0: its loss must rise
    l1 = loss()
    qz = model.queue.detach().t().to(torch.bfloat16).double().cpu()
    z = torch.cat([(q.double().cpu() * k.double().cpu()).sum(1, keepdim=True), q.double().cpu() @ qz.t()], 1) / T
    want = F.cross_entropy(z, torch.zeros(4, dtype=torch.int64)).item()
    assert l1 > l0 + 0.1 and abs(l1 - want) <= 1e-4
    model._dequeue_and_enqueue(k)  # the module's own write does not trigger a rebuild, and is in both copies
    assert model._operand_queue() is km and torch.equal(km[:4], k) and model.queue_ptr.item() == 4
    assert torch.equal(model.queue[:, :4].t().contiguous(), k.float())
    model.precision = "fp32"  # a precision change rebuilds the operand copy in the new dtype
    km32 = model._operand_queue()
    assert km32.dtype == torch.float32 and torch.equal(km32[:128], model.queue.t())


# ------------------------------------------------------------------------------------------------ InfoNCE
NCE_CASES = [(1, 256, 256), (37, 1184, 768), (70, 1190, 768), (64, 65536, 768)]
NCE_IDS = [f"N{n}-K{k}-H{h}" for n, k, h in NCE_CASES]
NCE_SEED = {(1, 256, 256): 1, (37, 1184, 768): 1, (70, 1190, 768): 1, (64, 65536, 768): 1, (70, 200, 72): 1}


@functools.lru_cache(maxsize=None)
def _nce_case(N, K, H):
    """Inputs (bf16-rounded unit vectors) and the float64 / CPU-autocast references; computed once, never modified."""
    _threads()
    g = torch.Generator().manual_seed(NCE_SEED[(N, K, H)] * 100003 + N + K + H)
    queue = F.normalize(torch.randn((K, H), generator=g), dim=1).to(torch.bfloat16)  # key-major
    q = F.normalize(torch.randn((N, H), generator=g), dim=1)
    k = F.normalize(torch.randn((N, H), generator=g), dim=1)
    near = F.normalize(q + 0.05 * torch.randn((N, H), generator=g), dim=1)
    k[::2] = near[::2]  # half of the rows: the positive wins
    q, k = q.to(torch.bfloat16), k.to(torch.bfloat16)
    q64, k64, w64 = q.double(), k.double(), queue.double()
    z = torch.cat([(q64 * k64).sum(1, keepdim=True), q64 @ w64.t()], dim=1) / T
    top2 = z.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3
    assert (~clear).float().mean().item() <= 0.02  # the float64 reference alone: at most 2 % unclear rows
    lse = torch.logsumexp(z, 1)
    row_loss = lse - z[:, 0]
    p = torch.softmax(z, 1)
    dq = ((p[:, :1] - 1) * k64 + p[:, 1:] @ w64) / (N * T)
    # the same computation by torch under CPU autocast(bf16), as the reference model writes it: the yardstick E
    qa = q.float().requires_grad_()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        l_pos = torch.einsum("nc,nc->n", [qa, k.float()]).unsqueeze(-1)
        l_neg = torch.einsum("nc,ck->nk", [qa, queue.float().t()])
        la = F.cross_entropy(torch.cat([l_pos, l_neg], dim=1) / T, torch.zeros(N, dtype=torch.int64))
    la.backward()
    return dict(q=q, k=k, queue=queue, z=z, lse=lse, row_loss=row_loss, loss=row_loss.mean().item(), clear=clear,
                correct=z.argmax(1) == 0, dq=dq, e_dq=_rel(qa.grad, dq))


def _nce_dev(c, dt):
    from vcg_hip import ops
    K, H = c["queue"].shape
    km = torch.zeros((ops.queue_kp(K), H), dtype=dt, device=DEV)
    km[:K] = c["queue"].to(dt).to(DEV)
    return c["q"].to(dt).to(DEV), c["k"].to(dt).to(DEV), km


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("N,K,H", NCE_CASES, ids=NCE_IDS)
def test_infonce_forward(N, K, H, prec):
    from vcg_hip import ops
    c = _nce_case(N, K, H)
    q, k, km = _nce_dev(c, DTYPES[prec])
    lse, row_loss, loss, n_correct, dq, logits = ops.infonce(q, k, km, K, 1 / T)
    assert dq is None and logits is None
    e_lse, e_row, e_loss = _maxerr(lse, c["lse"]), _maxerr(row_loss, c["row_loss"]), abs(loss.item() - c["loss"])
    print(f"lse err {e_lse:.3e} row loss err {e_row:.3e} loss err {e_loss:.3e} n_correct {n_correct.item()} "
          f"ref {int(c['correct'].sum())}")
    assert e_lse <= 1e-4 and e_row <= 1e-4 and e_loss <= 1e-4
    # two runs are bit-identical
    lse2, row2, loss2, n2, _, _ = ops.infonce(q, k, km, K, 1 / T)
    assert torch.equal(lse, lse2) and torch.equal(row_loss, row2) and torch.equal(loss, loss2)
    assert torch.equal(n_correct, n2)
    # the argmax count over the rows with a clear float64 top-1
    clear = c["clear"]
    if clear.any():
        keep = clear.to(DEV)
        nc = ops.infonce(q[keep].contiguous(), k[keep].contiguous(), km, K, 1 / T)[3]
        assert nc.item() == int(c["correct"][clear].sum())
        if N > 1:
            assert 0 < nc.item() < int(clear.sum())  # (the case has rows of both kinds)


@pytest.mark.parametrize("N,K,H", NCE_CASES, ids=NCE_IDS)
def test_infonce_gradient_bf16(N, K, H):
    from vcg_hip import ops
    c = _nce_case(N, K, H)
    q, k, km = _nce_dev(c, torch.bfloat16)
    dq = ops.infonce(q, k, km, K, 1 / T, want_dq=True)[4]
    assert dq.dtype == torch.float32 and dq.shape == (N, H)
    e = _rel(dq, c["dq"])
    print(f"dq rel err {e:.3e} (autocast {c['e_dq']:.3e})")
    floor = 0.0
    assert e <= max(1.5 * c["e_dq"], floor)
    assert torch.equal(dq, ops.infonce(q, k, km, K, 1 / T, want_dq=True)[4])  # bit-identical run to run


@pytest.mark.parametrize("N,K,H", NCE_CASES, ids=NCE_IDS)
def test_infonce_gradient_fp32(N, K, H):
    from vcg_hip import ops
    c = _nce_case(N, K, H)
    q, k, km = _nce_dev(c, torch.float32)
    dq = ops.infonce(q, k, km, K, 1 / T, want_dq=True)[4]
    _close(dq, c["dq"], "dq fp32")


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("N,K,H", NCE_CASES, ids=NCE_IDS)
def test_gradient_survives_the_enqueue(N, K, H, prec):
    """The trap: the keys are enqueued right after the loss, over queue rows the gradient needs. dq is fixed at forward
    time, so overwriting the rows at the pointer between forward and backward must not change it."""
    from vcg_hip import ops
    from vcg_hip.contrast import InfoNceLossFn
    c = _nce_case(N, K, H)
    q, k, km = _nce_dev(c, DTYPES[prec])
    want = ops.infonce(q, k, km, K, 1 / T, want_dq=True)[4]
    qa = q.clone().requires_grad_()
    loss, n_correct = InfoNceLossFn.apply(qa, k, km, K, 1 / T)
    km[:N] = 3.0  # what the enqueue at ptr = 0 does, with values that would wreck a recomputation
    (loss * 0.5).backward()
    assert torch.equal(qa.grad, (want * 0.5).to(qa.dtype))  # (autograd hands a bf16 leaf its gradient in bf16)
    assert abs(loss.item() - c["loss"]) <= 1e-4 and not n_correct.requires_grad
    with torch.no_grad():  # without gradient nothing is kept
        loss2, _ = InfoNceLossFn.apply(q, k, _nce_dev(c, DTYPES[prec])[2], K, 1 / T)
    assert abs(loss2.item() - c["loss"]) <= 1e-4


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("N,K,H", NCE_CASES, ids=NCE_IDS)
def test_infonce_logits(N, K, H, prec):
    from vcg_hip import ops
    from vcg_hip.contrast import InfoNceLogitsFn
    c = _nce_case(N, K, H)
    q, k, km = _nce_dev(c, DTYPES[prec])
    qa = q.clone().requires_grad_()
    logits = InfoNceLogitsFn.apply(qa, k, km, K, 1 / T)
    assert logits.shape == (N, 1 + K) and logits.dtype == torch.float32
    e = _maxerr(logits, c["z"])
    e0 = _maxerr(logits[:, 0], c["z"][:, 0])
    print(f"logits err {e:.3e} (column 0: {e0:.3e})")
    assert e <= 1e-3 and e0 <= 1e-3  # column 0 is the positive
    # the compatibility route's backward uses the queue as it was
    loss = F.cross_entropy(logits, torch.zeros(N, dtype=torch.int64, device=DEV))
    km[:N] = 3.0
    loss.backward()
    err = _rel(qa.grad.float(), c["dq"])
    print(f"logits-route dq rel err {err:.3e} (autocast {c['e_dq']:.3e})")
    assert err <= (1.5 * c["e_dq"] if prec == "bf16" else 1e-4)


def test_infonce_k_tail():
    """H = 72 is one 64-wide k stage plus one 8-wide chunk: the zero-filled k tail of the tile loop, which no H that is
    a multiple of 64 reaches. 70 rows are a partial second row block, 200 keys a partial second tile. Only the InfoNCE
    kernels run: the fp32 reduce gets its logits from the float64 reference instead of the GEMM. dZ elementwise against
    float64: 2^-8 of the value for the bf16 rounding plus 1e-4 / (N T) for the fp32 exponentials and lse."""
    from vcg_hip import _lib, ops
    N, K, H = 70, 200, 72
    c = _nce_case(N, K, H)
    q, k, km = _nce_dev(c, torch.bfloat16)
    s = ops.stream()

    def fused(keep):
        return ops.infonce(q[keep].contiguous(), k[keep].contiguous(), km, K, 1 / T)[:4]

    def reduce_f32(keep):
        z = c["z"][keep.cpu()].float().to(DEV)
        n = z.shape[0]
        buf, view = ops.infonce_logits_buffer(n, K, DEV)
        view.copy_(z)
        lse, row_loss, loss, n_correct = ops._nce_outputs(n, DEV)
        lpos, work = z[:, 0].contiguous(), ops.ws(6 * n * 4, DEV)
        _lib.call("vcg_infonce_reduce_f32", buf.data_ptr() + 16, buf.shape[1], lpos.data_ptr(), n, K, work.data_ptr(),
                  work.numel() * 4, lse.data_ptr(), row_loss.data_ptr(), None, loss.data_ptr(), n_correct.data_ptr(), s)
        return lse, row_loss, loss, n_correct

    clear = c["clear"]
    for name, run in (("bf16", fused), ("fp32", reduce_f32)):  # test_infonce_forward's assertions
        lse, row_loss, loss, n_correct = run(torch.ones(N, dtype=torch.bool, device=DEV))
        e_lse, e_row, e_loss = _maxerr(lse, c["lse"]), _maxerr(row_loss, c["row_loss"]), abs(loss.item() - c["loss"])
        print(f"{name}: lse err {e_lse:.3e} row loss err {e_row:.3e} loss err {e_loss:.3e} "
              f"n_correct {n_correct.item()} ref {int(c['correct'].sum())}")
        assert e_lse <= 1e-4 and e_row <= 1e-4 and e_loss <= 1e-4
        lse2, row2, loss2, n2 = run(torch.ones(N, dtype=torch.bool, device=DEV))
        assert torch.equal(lse, lse2) and torch.equal(row_loss, row2) and torch.equal(loss, loss2)
        assert torch.equal(n_correct, n2)
        nc = run(clear.to(DEV))[3]
        assert nc.item() == int(c["correct"][clear].sum())
        assert 0 < nc.item() < int(clear.sum())

    lse = fused(torch.ones(N, dtype=torch.bool, device=DEV))[0]
    Kp = ops.queue_kp(K)
    dZ = torch.empty((N, Kp), dtype=torch.bfloat16, device=DEV)
    _lib.call("vcg_infonce_dz", q.data_ptr(), km.data_ptr(), lse.data_ptr(), N, K, H, 1 / T, 1 / (N * T), dZ.data_ptr(),
              Kp, s)
    want = torch.softmax(c["z"], 1)[:, 1:] / (N * T)
    err = (dZ[:, :K].double().cpu() - want).abs()
    bound = 2 ** -8 * want + 1e-4 / (N * T)
    print(f"dZ max err {err.max().item():.3e}, worst err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()

    buf, view = ops.infonce_logits_buffer(N, K, DEV)
    _lib.call("vcg_infonce_logits", q.data_ptr(), km.data_ptr(), N, K, H, 1 / T, buf.data_ptr() + 16, buf.shape[1], s)
    e = _maxerr(view[:, 1:], c["z"][:, 1:])
    print(f"key logits err {e:.3e}")
    assert e <= 1e-3


def test_infonce_shape_limits():
    from vcg_hip import _lib, ops
    N, K = 4, 300
    work = ops.ws(1 << 20, DEV)
    sentinel = torch.full((N,), -7.0, dtype=torch.float32, device=DEV)
    lpos = torch.zeros(N, device=DEV)
    lib = _lib.lib()
    s = ops.stream()
    for H in (100, 4104):  # not a multiple of 8; above the limit
        q = torch.zeros((N, H), dtype=torch.bfloat16, device=DEV)
        km = torch.zeros((ops.queue_kp(K), H), dtype=torch.bfloat16, device=DEV)
        rc = lib.vcg_infonce_fwd(q.data_ptr(), km.data_ptr(), lpos.data_ptr(), N, K, H, 1.0, work.data_ptr(),
                                 work.numel() * 4, sentinel.data_ptr(), None, None, None, None, s)
        assert rc == -2  # VCG_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert (sentinel == -7.0).all()  # nothing ran
    H = 64
    q = torch.zeros((N, H), dtype=torch.bfloat16, device=DEV)
    km = torch.zeros((ops.queue_kp(K), H), dtype=torch.bfloat16, device=DEV)
    need = lib.vcg_infonce_ws_bytes(N, K, H)
    assert need > 0
    rc = lib.vcg_infonce_fwd(q.data_ptr(), km.data_ptr(), lpos.data_ptr(), N, K, H, 1.0, work.data_ptr(), need - 4,
                             sentinel.data_ptr(), None, None, None, None, s)
    assert rc != 0 and "workspace" in _lib.last_error()
    torch.cuda.synchronize()
    assert (sentinel == -7.0).all()
