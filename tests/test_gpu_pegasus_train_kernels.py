"""The kernels of the Pegasus training path (csrc/pegasus.hip, vcg_pegasus_embed_bwd in csrc/bert.hip) against fp64.

Cross-attention backward (B = 3 sequences with test_gpu_pegasus_kernels._mask: every key valid / two thirds valid with
a hole / no valid key; nh = 2, head dim 64; Lq on either side of the 16-query tile and of dkv's 64-query halves and
128-query tiles, Lk on either side of the per-wave 32-key strips and the 128-key tiles). q, kv and dO are column slices
of NaN-filled buffers with NaN rows behind them; the reference is the fp64 autograd of pegasus_ref.cross_attention_ref
(with dropout: pegasus_train_ref.cross_attention_train under dropout_util.score_keep(seed, B nh, Lq, Lk, p)).
  * fp32: max error <= 2e-5 x max|ref| for dQ and for dK | dV (the forward test's bound);
  * bf16: relative Frobenius error <= 2e-2, and <= 1.25 x the error of the unfused torch chain (bf16 bmm -> fp32 softmax
    with HF's finfo.min bias -> the same keep mask -> bf16 bmm, autograd) on the same inputs + 2e-3; at Lq = Lk in
    {16, 64, 128, 130, 257} also <= 1.25 x the fused self-attention backward's (bert_attn_bwd) + 2e-3 (130 and 257:
    the smallest lengths with a second and a third 128-tile, where the self-attention side is the tiled dkv kernel,
    the other caller of the dK | dV tile step the cross-attention kernel is built from);
  * the sequence without a valid key: finite, and the reference's uniform-P gradient within the same bounds;
  * two runs give equal bits; p = 0 through the training entry gives vcg_cross_attn_kv_fwd's bits.
With ONE key the softmax is constant, its Jacobian vanishes and the reference dQ (and dK) is exactly zero: dP = D. A
bound relative to the reference is 0 (fp32) or 0 / 0 (bf16) there, so where an output's reference is identically zero
its error is measured against the size of the terms that cancel, scale x max|dP| x max|K| per element (`_case`'s tq),
under the same factors.
LayerNorm backward of an fp32 input without a residual (vcg_ln_bwd_acc): dh += LN'(dout) and the gamma / beta gradients
against the fp64 autograd of F.layer_norm, for an fp32 and a bf16 dout, within 2e-5 x max|ref| (every operand is exact
in fp64, the sums are fp32 over at most 600 rows / 256 columns), added onto what is there, equal bits run to run.
Embedding: forward with dropout against row_keep; backward with repeated ids, pad ids, both dtype classes, added onto
existing gradients, the pad row untouched, equal bits run to run. Dropout-add and ReLU-dropout against numpy.
Refusals: bad shapes, misaligned bf16 pointers and dh != 64 are errors, nothing is written.
"""
import math

import numpy as np
import pytest
import torch

import pegasus_ref as ref
import pegasus_train_ref as tref
from bert_attn_ref import rel
from dropout_util import row_keep, score_keep
from test_gpu_pegasus_kernels import _mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, NH, H = 3, 2, 128
PAIRS = [(1, 300), (16, 128), (17, 31), (31, 129), (130, 1), (130, 300)]  # every Lq and every Lk of the issue
PADC, PADR = 8, 8  # NaN columns beside and NaN rows behind q, kv and dO
SEED = 0x1234567887654321


@pytest.fixture(scope="module", autouse=True)
def _init():
    from vcg_hip import _lib
    _lib.call("vcg_init", 0)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


_CASES = {}


def _case(Lq, Lk, dtype, p=0.0):
    """NaN-padded q, kv, dO in `dtype`, the mask, and the fp64 reference (ctx, dq, dkv); made once per key"""
    key = (Lq, Lk, dtype, p)
    if key not in _CASES:
        g = torch.Generator().manual_seed(7000 * Lq + Lk)
        qb = torch.full((B * Lq + PADR, H + PADC), float("nan"), dtype=dtype)
        kvb = torch.full((B * Lk + PADR, 2 * H + PADC), float("nan"), dtype=dtype)
        dob = torch.full((B * Lq + PADR, H + PADC), float("nan"), dtype=dtype)
        qb[:B * Lq, :H] = (torch.randn(B * Lq, H, generator=g) * 1.5).to(dtype)
        kvb[:B * Lk, :2 * H] = (torch.randn(B * Lk, 2 * H, generator=g) * 1.5).to(dtype)
        dob[:B * Lq, :H] = torch.randn(B * Lq, H, generator=g).to(dtype)
        mask = _mask(Lk)
        q64 = qb[:B * Lq, :H].double().requires_grad_()
        kv64 = kvb[:B * Lk, :2 * H].double().requires_grad_()
        keep = None
        if p > 0:
            keep = torch.from_numpy(score_keep(SEED, B * NH, Lq, Lk, p))
            ctx = tref.cross_attention_train(q64, kv64, mask, B, NH, Lq, Lk, keep, p)
        else:
            ctx = ref.cross_attention_ref(q64, kv64, mask, B, NH, Lq, Lk)[0]
            assert torch.allclose(ctx, tref.cross_attention_train(q64, kv64, mask, B, NH, Lq, Lk), rtol=0, atol=1e-12)
        ctx.backward(dob[:B * Lq, :H].double())
        with torch.no_grad():  # the size of dQ's terms: scale x max|dP| x max|K| (docstring)
            doh = dob[:B * Lq, :H].double().view(B, Lq, NH, 64).transpose(1, 2)
            vh = kv64[:, H:].reshape(B, Lk, NH, 64).transpose(1, 2)
            tq = 0.125 * (doh @ vh.transpose(-1, -2)).abs().max().item() * kv64[:, :H].abs().max().item()
        _CASES[key] = (qb, kvb, dob, mask, keep, ctx.detach(), q64.grad, kv64.grad, tq)
    return _CASES[key]


def _maxden(want, tq):
    m = want.abs().max().item()
    return m if m > 0 else tq


def _normden(want, tq):
    n = want.norm().item()
    return n if n > 0 else tq * math.sqrt(want.numel())


def _run(qb, kvb, dob, mask, Lq, Lk, p=0.0):
    """the training forward and the backward on the GPU -> (ctx, dq, dkv) on the CPU; dq and dkv are written into
    column slices of sentinel buffers whose other columns and pad rows must stay untouched"""
    from vcg_hip import ops
    qd, kvd, dod, md = qb.to(DEV), kvb.to(DEV), dob.to(DEV), mask.to(DEV)
    stats = torch.full((B * NH, Lq, 2), float("nan"), dtype=torch.float32, device=DEV)
    ctx = ops.cross_attn_kv_fwd(qd[:, :H], kvd[:, :2 * H], md, B, NH, Lq, Lk, 0.125, stats=stats, dropout_p=p, seed=SEED)
    dqb = torch.full((B * Lq + PADR, H + PADC), 7.0, dtype=qb.dtype, device=DEV)
    dkvb = torch.full((B * Lk + PADR, 2 * H + PADC), 7.0, dtype=qb.dtype, device=DEV)
    ops.cross_attn_kv_bwd(qd[:, :H], kvd[:, :2 * H], md, dod[:, :H], stats, B, NH, Lq, Lk, 0.125, p, SEED,
                          dq=dqb[:, :H], dkv=dkvb[:, :2 * H])
    torch.cuda.synchronize()
    dqb, dkvb = dqb.cpu(), dkvb.cpu()
    assert bool((dqb[:, H:] == 7.0).all()) and bool((dqb[B * Lq:] == 7.0).all())
    assert bool((dkvb[:, 2 * H:] == 7.0).all()) and bool((dkvb[B * Lk:] == 7.0).all())
    return ctx.cpu(), dqb[:B * Lq, :H], dkvb[:B * Lk, :2 * H]


def _chain(qb, kvb, dob, mask, keep, Lq, Lk, p):
    """the unfused chain on stock torch ops, bf16 on the GPU, P in HBM -> (dq, dkv)"""
    q = qb[:B * Lq, :H].to(DEV).requires_grad_()
    kv = kvb[:B * Lk, :2 * H].to(DEV).requires_grad_()
    qh = q.view(B, Lq, NH, 64).transpose(1, 2)
    kh = kv[:, :H].reshape(B, Lk, NH, 64).transpose(1, 2)
    vh = kv[:, H:].reshape(B, Lk, NH, 64).transpose(1, 2)
    s = (qh @ kh.transpose(-1, -2)).float() * 0.125
    s = s + ((mask == 0).to(DEV).float() * ref.FMIN)[:, None, None, :]
    w = torch.softmax(s, dim=-1)
    if keep is not None:
        w = w * keep.view(B, NH, Lq, Lk).to(DEV).float() / (1.0 - p)
    o = (w.to(q.dtype) @ vh).transpose(1, 2).reshape(B * Lq, H)
    o.backward(dob[:B * Lq, :H].to(DEV))
    return q.grad.cpu(), kv.grad.cpu()


def _nokey(t, L):
    return t[2 * L:3 * L]  # the rows of sequence 2: no valid key


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("Lq,Lk", PAIRS)
def test_cross_attention_bwd_fp32(Lq, Lk, p):
    qb, kvb, dob, mask, keep, wctx, wdq, wdkv, tq = _case(Lq, Lk, torch.float32, p)
    ctx, dq, dkv = _run(qb, kvb, dob, mask, Lq, Lk, p)
    for name, got, want, L in (("ctx", ctx, wctx, Lq), ("dq", dq, wdq, Lq), ("dkv", dkv, wdkv, Lk)):
        err, bound = (got.double() - want).abs().max().item(), 2e-5 * _maxden(want, tq)
        print(f"fp32 Lq={Lq} Lk={Lk} p={p} {name}: max err {err:.3e} (bound {bound:.3e})")
        assert torch.isfinite(got).all() and err <= bound
        nk = (_nokey(got, L).double() - _nokey(want, L)).abs().max().item()
        assert nk <= bound  # (the output's bound: with one key dP = D and the reference cancels to exactly 0)
    assert _nokey(wdq, Lq).abs().max() > 0 or Lk == 1  # the uniform-P gradient is not zero (one key: dP = D)
    ctx2, dq2, dkv2 = _run(qb, kvb, dob, mask, Lq, Lk, p)
    assert torch.equal(_bits(dq), _bits(dq2)) and torch.equal(_bits(dkv), _bits(dkv2))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("Lq,Lk", PAIRS)
def test_cross_attention_bwd_bf16(Lq, Lk, p):
    qb, kvb, dob, mask, keep, wctx, wdq, wdkv, tq = _case(Lq, Lk, torch.bfloat16, p)
    ctx, dq, dkv = _run(qb, kvb, dob, mask, Lq, Lk, p)
    cdq, cdkv = _chain(qb, kvb, dob, mask, keep, Lq, Lk, p)
    assert rel(ctx, wctx) <= 2e-2
    for name, got, chain, want, L in (("dq", dq, cdq, wdq, Lq), ("dkv", dkv, cdkv, wdkv, Lk)):
        den = _normden(want, tq)
        e, ec = (got.double() - want).norm().item() / den, (chain.double() - want).norm().item() / den
        # (the no-key rows relative to their own reference; only where that is identically zero -- one key -- against a
        # tenth of the whole output's denominator, the size of the terms that cancel)
        nkw = _nokey(want, L).norm().item()
        nk = (_nokey(got, L).double() - _nokey(want, L)).norm().item() / (nkw if nkw > 0 else 0.1 * den)
        print(f"bf16 Lq={Lq} Lk={Lk} p={p} {name}: rel err {e:.3e}, unfused chain {ec:.3e}, no-key sequence {nk:.3e}")
        assert torch.isfinite(got).all()
        assert e <= 2e-2 and e <= 1.25 * ec + 2e-3
        assert nk <= 2e-2
    ctx2, dq2, dkv2 = _run(qb, kvb, dob, mask, Lq, Lk, p)
    assert torch.equal(_bits(dq), _bits(dq2)) and torch.equal(_bits(dkv), _bits(dkv2))


@pytest.mark.parametrize("L", [16, 64, 128, 130, 257])
def test_cross_attention_bwd_bf16_against_fused_self_attention(L):
    """Lq = Lk, non-causal: the same Q | K | V (one fused [B L + 8, 3 H] buffer, read in place at row pitch 3 H) and dO
    through bert_attn_bwd"""
    from vcg_hip import ops
    from vcg_hip.bert import attention_bwd, attention_fwd
    g = torch.Generator().manual_seed(99 + L)
    qkv = torch.full((B * L + 8, 3 * H), float("nan"), dtype=torch.bfloat16)
    qkv[:B * L] = (torch.randn(B * L, 3 * H, generator=g) * 1.5).to(torch.bfloat16)
    dO = torch.randn(B * L, H, generator=g).to(torch.bfloat16)
    mask = _mask(L)
    q64 = qkv[:B * L, :H].double().requires_grad_()
    kv64 = qkv[:B * L, H:].double().requires_grad_()
    ref.cross_attention_ref(q64, kv64, mask, B, NH, L, L)[0].backward(dO.double())
    qd, md, dod = qkv.to(DEV), mask.to(DEV), dO.to(DEV)
    stats = torch.empty((B * NH, L, 2), dtype=torch.float32, device=DEV)
    ctx = ops.cross_attn_kv_fwd(qd[:, :H], qd[:, H:], md, B, NH, L, L, 0.125, stats=stats, dropout_p=0.0)
    dq, dkv = ops.cross_attn_kv_bwd(qd[:, :H], qd[:, H:], md, dod, stats, B, NH, L, L, 0.125)
    qz = qd.clone()
    qz[B * L:] = 0  # (the self-attention kernels may read their pad rows)
    Lp = (L + 7) // 8 * 8
    sctx, att = attention_fwd(qz, md, B, NH, L, Lp, 64, 0.125, 0.0, 1, True)
    dqkv = attention_bwd(qz, dod, sctx, md, att, B, NH, L, Lp, 64, 0.125, 0.0, 1)
    torch.cuda.synchronize()
    for name, got, yard, want in (("dq", dq, dqkv[:, :H], q64.grad), ("dkv", dkv, dqkv[:, H:], kv64.grad)):
        e, ey = rel(got.cpu(), want), rel(yard.cpu(), want)
        print(f"L={L} {name}: cross-attention backward {e:.3e}, fused self-attention backward {ey:.3e}")
        assert e <= 2e-2 and e <= 1.25 * ey + 2e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_training_forward_p0_gives_the_inference_bits(dtype):
    from vcg_hip import ops
    for Lq, Lk in ((17, 31), (31, 129)):
        qb, kvb, _, mask, *_ = _case(Lq, Lk, dtype)
        qd, kvd, md = qb.to(DEV), kvb.to(DEV), mask.to(DEV)
        out = []
        for p in (None, 0.0):
            stats = torch.full((B * NH, Lq, 2), float("nan"), dtype=torch.float32, device=DEV)
            ctx = ops.cross_attn_kv_fwd(qd[:, :H], kvd[:, :2 * H], md, B, NH, Lq, Lk, 0.125, stats=stats, dropout_p=p,
                                        seed=SEED)
            out.append((ctx.cpu(), stats.cpu()))
        assert torch.equal(_bits(out[0][0]), _bits(out[1][0])) and torch.equal(_bits(out[0][1]), _bits(out[1][1]))


def test_cross_attention_bwd_refusals():
    from vcg_hip import _lib, ops
    Lq, Lk = 17, 31
    qb, kvb, dob, mask, *_ = _case(Lq, Lk, torch.bfloat16)
    qd, kvd, dod, md = qb.to(DEV), kvb.to(DEV), dob.to(DEV), mask.to(DEV)
    stats = torch.empty((B * 4, Lq, 2), dtype=torch.float32, device=DEV)  # (room for the 4 heads of 32 asked for below)
    ops.cross_attn_kv_fwd(qd[:, :H], kvd[:, :2 * H], md, B, NH, Lq, Lk, 0.125, stats=stats, dropout_p=0.0)
    dq = torch.full((B * Lq, H), 3.0, dtype=torch.bfloat16, device=DEV)
    dkv = torch.full((B * Lk, 2 * H), 3.0, dtype=torch.bfloat16, device=DEV)

    def call(q=qd[:, :H], kv=kvd[:, :2 * H], do=dod[:, :H], nh=NH, lq=Lq, lk=Lk, dh=64, p=0.0):
        return ops.cross_attn_kv_bwd(q, kv, md, do, stats, B, nh, lq, lk, 0.125, p, SEED, dq=dq, dkv=dkv, dh=dh)

    with pytest.raises(_lib.VcgError, match=r"\(-1\).*head dim"):
        call(nh=4, dh=32)  # (H = 128 = 4 heads of 32)
    with pytest.raises(_lib.VcgError, match=r"\(-1\).*alignment"):
        call(q=qd[:, 1:H + 1])  # a bf16 pointer 2 bytes off
    with pytest.raises(_lib.VcgError, match=r"\(-1\).*alignment"):
        call(do=dod[:, 4:H + 4])
    with pytest.raises(_lib.VcgError, match=r"\(-1\).*dropout_p"):
        call(p=1.0)
    with pytest.raises(ValueError, match="too small"):
        call(lk=Lk + 13)  # more keys than kv has rows
    with pytest.raises(_lib.VcgError, match=r"\(-1\).*bad shape"):
        _lib.call("vcg_cross_attn_kv_bwd", 1, qd.data_ptr(), H + PADC, kvd.data_ptr(), 2 * H + PADC, None,
                  dod.data_ptr(), H + PADC, stats.data_ptr(), stats.data_ptr(), dq.data_ptr(), H,
                  dkv.data_ptr(), 2 * H, B, NH, 64, 0, Lk, 0.125, 0.0, 0, ops.stream())
    with pytest.raises(_lib.VcgError, match=r"\(-1\).*dropout_p"):
        ops.cross_attn_kv_fwd(qd[:, :H], kvd[:, :2 * H], md, B, NH, Lq, Lk, 0.125, dropout_p=-0.5)
    torch.cuda.synchronize()
    assert bool((dq == 3.0).all()) and bool((dkv == 3.0).all())


# ------------------------------------------------------------------------------------------------ embedding
V, NP, HE, BE, LE, PAD = 23, 40, 128, 3, 9, 0


def _embed_inputs():
    g = torch.Generator().manual_seed(11)
    tok, pos = torch.randn(V, HE, generator=g), torch.randn(NP, HE, generator=g)
    ids = torch.randint(1, 6, (BE, LE), generator=g)  # few distinct ids: every one repeats
    ids[:, 0] = PAD  # the decoder's start token is the pad token
    ids[1, 5:] = PAD
    return tok, pos, ids


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_pegasus_embed_dropout_fwd(dtype, p):
    from vcg_hip import ops
    tok, pos, ids = _embed_inputs()
    scale = math.sqrt(HE)
    s32 = float(np.float32(scale))
    out = ops.pegasus_embed_fwd(ids.to(DEV), tok.to(DEV), pos.to(DEV), BE, LE, HE, dtype, scale, 3, p=p, seed=SEED)
    base = (s32 * tok.double()[ids] + pos.double()[3:3 + LE][None]).float().view(BE * LE, HE)
    keep = torch.from_numpy(row_keep(SEED, BE * LE, HE, p))
    want = torch.where(keep, base / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32)),
                       torch.zeros(())).to(dtype)
    assert torch.equal(_bits(out.cpu()), _bits(want))
    if p == 0.0:
        plain = ops.pegasus_embed_fwd(ids.to(DEV), tok.to(DEV), pos.to(DEV), BE, LE, HE, dtype, scale, 3)
        assert torch.equal(_bits(out.cpu()), _bits(plain.cpu()))
    else:
        assert 0.02 < 1.0 - keep.float().mean().item() < 0.2


@pytest.mark.parametrize("cls", ["f32", "bf16", "bf16_grad_f32"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_pegasus_embed_bwd(cls, p):
    from vcg_hip import ops
    _, _, ids = _embed_inputs()
    g = torch.Generator().manual_seed(12)
    dout = torch.randn(BE * LE, HE, generator=g)
    dout = dout.to(torch.bfloat16) if cls == "bf16" else dout
    storage = torch.float32 if cls == "f32" else torch.bfloat16
    grad0 = torch.randn(V, HE, generator=g)  # existing gradients: the result is added onto them
    grad0[PAD] = -123.0  # the sentinel of the pad row
    scale = math.sqrt(HE)
    keep = torch.from_numpy(row_keep(SEED, BE * LE, HE, p))
    de = float(np.float32(scale)) * (dout.double() * keep / (1.0 - float(np.float32(p))))
    want = grad0.double().clone()
    flat = ids.view(-1)
    for r in range(BE * LE):
        if flat[r] != PAD:
            want[flat[r]] += de[r]
    got = []
    for _ in range(2):
        grad = grad0.clone().to(DEV)
        ops.pegasus_embed_bwd(dout.to(DEV), ids.to(DEV), grad, BE, LE, HE, scale, PAD, p, SEED, storage_dtype=storage)
        got.append(grad.cpu())
    assert torch.equal(got[0][PAD], grad0[PAD])  # untouched, bit for bit
    untouched = [v for v in range(V) if v not in set(flat.tolist())]
    assert torch.equal(got[0][untouched], grad0[untouched])
    err = (got[0].double() - want).abs().max().item()
    print(f"embed bwd {cls} p={p}: max err {err:.3e}")
    assert err <= 2e-5 * want.abs().max().item()  # fp32 sums of at most 27 fp32 terms
    assert torch.equal(_bits(got[0]), _bits(got[1]))


# ------------------------------------------------------------------------------------------------ elementwise
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_dropout_add_and_relu_dropout(dtype, rows, p):
    from vcg_hip import ops
    Hh = 128
    g = torch.Generator().manual_seed(100 * rows + int(10 * p))
    keep = row_keep(SEED, rows, Hh, p)
    inv = np.float32(1.0) - np.float32(p)
    h0 = torch.randn(rows, Hh, generator=g)
    br = torch.randn(rows, Hh, generator=g).to(dtype)
    dh = torch.randn(rows, Hh, generator=g)
    pre = torch.randn(rows, Hh, generator=g).to(dtype)
    dy = torch.randn(rows, Hh, generator=g).to(dtype)

    # h += dropout(branch): one fp32 division and one fp32 add
    h = ops.dropout_add_fwd(h0.clone().to(DEV), br.to(DEV), p, SEED).cpu()
    want = h0.numpy() + np.where(keep, br.float().numpy() / inv, np.float32(0))
    assert np.array_equal(h.numpy(), want.astype(np.float32))
    # dbranch = dropout'(dh), rounded to the compute dtype
    db = ops.dropout_add_bwd(dh.to(DEV), dtype, p, SEED).cpu()
    want = torch.from_numpy(np.where(keep, dh.numpy() / inv, np.float32(0)).astype(np.float32)).to(dtype)
    assert torch.equal(_bits(db), _bits(want))
    # f = dropout(relu(pre))
    f = ops.relu_dropout_fwd(pre.to(DEV), p, SEED).cpu()
    pn = pre.float().numpy()
    wf = torch.from_numpy(np.where(keep & (pn > 0), pn / inv, np.float32(0)).astype(np.float32)).to(dtype)
    assert torch.equal(_bits(f), _bits(wf))
    # dpre = dy * (f > 0 ? 1 / (1 - p) : 0) from the saved f
    dp = ops.relu_dropout_bwd(dy.to(DEV), f.to(DEV), p).cpu()
    wd = torch.from_numpy(np.where(wf.float().numpy() > 0, dy.float().numpy() / inv, np.float32(0)).astype(np.float32))
    assert torch.equal(_bits(dp), _bits(wd.to(dtype)))
    # ... which is the derivative of the forward wherever the pre-activation did not underflow
    assert np.array_equal(wf.float().numpy() > 0, keep & (pn > 0))
    # in place
    buf = pre.clone().to(DEV)
    assert ops.relu_dropout_fwd(buf, p, SEED, out=buf) is buf and torch.equal(_bits(buf.cpu()), _bits(wf))


def test_elementwise_refusals():
    from vcg_hip import _lib, ops
    h = torch.zeros(4, 128, device=DEV)
    with pytest.raises(_lib.VcgError, match=r"\(-1\).*dropout_p"):
        ops.dropout_add_fwd(h, torch.ones(4, 128, device=DEV), 1.0, 1)
    with pytest.raises(ValueError, match="at least"):
        ops.dropout_add_fwd(h, torch.ones(5, 128, device=DEV), 0.1, 1)
    with pytest.raises(TypeError):
        ops.relu_dropout_bwd(h, h.to(torch.bfloat16), 0.1)
    torch.cuda.synchronize()
    assert bool((h == 0).all())


def test_elementwise_unaligned_and_tail():
    """pointers off the 16-byte grid and a count that is no multiple of the 8-element groups: the element-by-element
    path and the partial last group give the bits of the aligned run on the same data"""
    from vcg_hip import ops
    n, p = 37 * 128 - 3, 0.1
    g = torch.Generator().manual_seed(8)
    for dtype in (torch.float32, torch.bfloat16):
        pre = torch.randn(n + 9, generator=g).to(dtype).to(DEV)
        h0 = torch.randn(n + 9, generator=g).to(DEV)
        want_f = ops.relu_dropout_fwd(pre[:n].clone(), p, SEED)
        want_h = ops.dropout_add_fwd(h0[:n].clone(), pre[:n].clone(), p, SEED)
        want_d = ops.dropout_add_bwd(h0[:n].clone(), dtype, p, SEED)
        for off in (1, 3):  # 2 / 6 bytes (bf16) and 4 / 12 bytes (fp32) off
            src, hs = torch.zeros_like(pre), torch.full_like(h0, 5.0)
            src[off:off + n] = pre[:n]
            hs[off:off + n] = h0[:n]
            f = ops.relu_dropout_fwd(src[off:off + n], p, SEED)
            assert torch.equal(_bits(f.cpu()), _bits(want_f.cpu()))
            d = ops.dropout_add_bwd(hs[off:off + n], dtype, p, SEED)
            assert torch.equal(_bits(d.cpu()), _bits(want_d.cpu()))
            ops.dropout_add_fwd(hs[off:off + n], src[off:off + n], p, SEED)
            assert torch.equal(_bits(hs[off:off + n].cpu()), _bits(want_h.cpu()))
            assert bool((hs[:off] == 5.0).all()) and bool((hs[off + n:] == 5.0).all())  # nothing outside is written
            dp = ops.relu_dropout_bwd(src[off:off + n], f, p)
            assert torch.equal(_bits(dp.cpu()), _bits(ops.relu_dropout_bwd(pre[:n].clone(), want_f, p).cpu()))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,Hh", [(1, 128), (37, 128), (600, 256)])  # (600 rows: more than one row per workgroup)
def test_ln_bwd_acc(rows, Hh, dt):
    import torch.nn.functional as F
    from vcg_hip import ops
    g = torch.Generator().manual_seed(rows + Hh)
    x = torch.randn(rows, Hh, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.2 * torch.randn(Hh, generator=g), 0.1 * torch.randn(Hh, generator=g)
    dout = torch.randn(rows, Hh, generator=g).to(dt)
    dh0, gg0, gb0 = (torch.randn(*s, generator=g) for s in ((rows, Hh), (Hh,), (Hh,)))
    x64, g64, b64 = (t.double().requires_grad_() for t in (x, gamma, beta))
    F.layer_norm(x64, (Hh,), g64, b64, 1e-5).backward(dout.double())
    want = (dh0.double() + x64.grad, gg0.double() + g64.grad, gb0.double() + b64.grad)
    xd = x.to(DEV)
    _, mean, rstd = ops.ln_fwd(xd, None, gamma.to(DEV), beta.to(DEV), rows, Hh, 1e-5)
    runs = []
    for _ in range(2):
        dh, gg, gb = dh0.clone().to(DEV), gg0.clone().to(DEV), gb0.clone().to(DEV)
        ops.ln_bwd_acc(dout.to(DEV), xd, gamma.to(DEV), mean, rstd, dh, gg, gb, rows, Hh)
        runs.append((dh.cpu(), gg.cpu(), gb.cpu()))
    for name, got, w in zip(("dh", "dgamma", "dbeta"), runs[0], want):
        err, bound = (got.double() - w).abs().max().item(), 2e-5 * w.abs().max().item()
        print(f"ln_bwd_acc rows={rows} H={Hh} {dt} {name}: max err {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs))
    # a frozen LayerNorm: no parameter gradient, the same dh
    dh = dh0.clone().to(DEV)
    ops.ln_bwd_acc(dout.to(DEV), xd, gamma.to(DEV), mean, rstd, dh, None, None, rows, Hh)
    assert torch.equal(_bits(dh.cpu()), _bits(runs[0][0]))
