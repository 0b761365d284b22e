"""The kernels of the Pegasus inference path (csrc/pegasus.hip) against the fp64 statements of tests/pegasus_ref.py.

Cross-attention (B = 3, nh = 3, head dim 64; Lq on either side of the 16-query tile, Lk on either side of the per-wave
32-key strips, the 128-key tiles and the 8 pad rows; per batch one sequence with every key valid, one with a shorter
valid prefix that has a hole, one fully masked; also key_mask = NULL). q and kv are column slices of wider buffers whose
other columns, and the 8 rows behind kv, hold NaN: nothing of them may reach ctx.
  * fp32: ctx and stats within 2e-5 x max|ref| of fp64, the project's fp32 kernel bound;
  * bf16: relative Frobenius error of ctx and stats against fp64 <= 2e-2, and at Lq = Lk in {16, 64, 128} ctx also
    <= 1.25 x the error of the fused self-attention kernel (bert_attn_fwd) on the same Q / K / V + 2e-3
    (tests/test_gpu_gpt_decode_kernels.py's measure);
  * a fully masked sequence is uniform over its Lk keys, stats (-inf, Lk);
  * a second run is bit-identical; head dim 32 is refused with ctx untouched.
Embedding: exactly the storage-dtype rounding of scale * tok[id] + pos[pos0 + t] computed in fp64; pos0 > 0; a window
past the table is refused.
"""
import math

import numpy as np
import pytest
import torch

import pegasus_ref as ref
from bert_attn_ref import rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, NH, H = 3, 3, 192
LQS = [1, 5, 16, 17, 31, 33]
LKS = [1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 257, 512, 513]
PADC = 8  # NaN columns beside q and kv


@pytest.fixture(scope="module", autouse=True)
def _init():
    from vcg_hip import _lib
    _lib.call("vcg_init", 0)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _mask(Lk):
    m = torch.zeros(B, Lk, dtype=torch.int64)
    m[0] = 1
    n = max(1, 2 * Lk // 3)
    m[1, :n] = 1
    if n >= 3:
        m[1, 1] = 0  # a hole
    return m  # (sequence 2: no valid key)


_CASES = {}


def _case(Lq, Lk, dtype):
    """q [B Lq, H] and kv [B Lk, 2 H] as column slices of NaN-filled buffers (kv with 8 NaN rows behind it), the mask,
    and the fp64 statements with the mask and without; made once per shape and dtype"""
    key = (Lq, Lk, dtype)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * Lq + Lk)
        qb = torch.full((B * Lq, H + PADC), float("nan"), dtype=dtype)
        kvb = torch.full((B * Lk + 8, 2 * H + PADC), float("nan"), dtype=dtype)
        qb[:, :H] = (torch.randn(B * Lq, H, generator=g) * 1.5).to(dtype)
        kvb[:B * Lk, :2 * H] = (torch.randn(B * Lk, 2 * H, generator=g) * 1.5).to(dtype)
        mask = _mask(Lk)
        want = {True: ref.cross_attention_ref(qb, kvb, mask, B, NH, Lq, Lk),
                False: ref.cross_attention_ref(qb, kvb, None, B, NH, Lq, Lk)}
        _CASES[key] = (qb, kvb, mask, want)
    return _CASES[key]


def _run(qb, kvb, mask, Lq, Lk, dh=64, ctx=None):
    from vcg_hip import ops
    qd, kvd = qb.to(DEV), kvb.to(DEV)
    stats = torch.full((B * NH, Lq, 2), float("nan"), dtype=torch.float32, device=DEV)
    ctx = ops.cross_attn_kv_fwd(qd[:, :H], kvd[:, :2 * H], None if mask is None else mask.to(DEV), B, NH, Lq, Lk, 0.125,
                                ctx=ctx, stats=stats, dh=dh)
    torch.cuda.synchronize()
    return ctx.cpu(), stats.cpu()


def _check_stats(stats, mx, sm, masked, Lk, bf16):
    got_mx, got_sm = stats[..., 0].double(), stats[..., 1].double()
    fin = torch.isfinite(mx)
    assert torch.equal(torch.isfinite(got_mx), fin)  # -inf exactly where no key is valid
    if masked:
        nk = ~fin
        assert nk.view(B, NH, -1)[2].all() and not nk.view(B, NH, -1)[:2].any()
        assert torch.equal(got_sm[nk], torch.full_like(got_sm[nk], float(Lk)))
    if bf16:
        assert rel(got_mx[fin], mx[fin]) <= 2e-2 and rel(got_sm, sm) <= 2e-2
    else:
        assert (got_mx[fin] - mx[fin]).abs().max().item() <= 2e-5 * mx[fin].abs().max().item()
        assert (got_sm - sm).abs().max().item() <= 2e-5 * sm.abs().max().item()


@pytest.mark.parametrize("Lk", LKS)
def test_cross_attention_fp32(Lk):
    for Lq in LQS:
        qb, kvb, mask, want = _case(Lq, Lk, torch.float32)
        for masked in (True, False):
            ctx, stats = _run(qb, kvb, mask if masked else None, Lq, Lk)
            wctx, mx, sm = want[masked]
            err, bound = (ctx.double() - wctx).abs().max().item(), 2e-5 * wctx.abs().max().item()
            print(f"fp32 Lq={Lq} Lk={Lk} mask={masked}: max err {err:.3e} (bound {bound:.3e})")
            assert torch.isfinite(ctx).all() and err <= bound
            _check_stats(stats, mx, sm, masked, Lk, bf16=False)
        ctx2, stats2 = _run(qb, kvb, None, Lq, Lk)
        assert torch.equal(_bits(ctx), _bits(ctx2)) and torch.equal(_bits(stats), _bits(stats2))


@pytest.mark.parametrize("Lk", LKS)
def test_cross_attention_bf16(Lk):
    for Lq in LQS:
        qb, kvb, mask, want = _case(Lq, Lk, torch.bfloat16)
        for masked in (True, False):
            ctx, stats = _run(qb, kvb, mask if masked else None, Lq, Lk)
            wctx, mx, sm = want[masked]
            e = rel(ctx, wctx)
            print(f"bf16 Lq={Lq} Lk={Lk} mask={masked}: rel err {e:.3e}")
            assert torch.isfinite(ctx).all() and e <= 2e-2
            _check_stats(stats, mx, sm, masked, Lk, bf16=True)
            if masked:  # the fully masked sequence: the mean of its Lk value rows
                v = kvb[2 * Lk:3 * Lk, H:2 * H].double().mean(0)
                assert rel(ctx[2 * Lq:3 * Lq], v[None].expand(Lq, H)) <= 2e-2
        ctx2, stats2 = _run(qb, kvb, mask, Lq, Lk)
        ctx3, stats3 = _run(qb, kvb, mask, Lq, Lk)
        assert torch.equal(_bits(ctx2), _bits(ctx3)) and torch.equal(_bits(stats2), _bits(stats3))


@pytest.mark.parametrize("L", [16, 64, 128])
def test_cross_attention_bf16_against_fused_self_attention(L):
    """Lq = Lk: the same Q / K / V through bert_attn_fwd (one fused [B L + 8, 3 H] buffer; the cross-attention kernel
    reads its column slices in place, row pitch 3 H)"""
    from vcg_hip import ops
    from vcg_hip.bert import attention_fwd
    g = torch.Generator().manual_seed(77 + L)
    qkv = torch.full((B * L + 8, 3 * H), float("nan"), dtype=torch.bfloat16)
    qkv[:B * L] = (torch.randn(B * L, 3 * H, generator=g) * 1.5).to(torch.bfloat16)
    mask = _mask(L)
    wctx, _, _ = ref.cross_attention_ref(qkv[:, :H], qkv[:, H:], mask, B, NH, L, L)
    qd, md = qkv.to(DEV), mask.to(DEV)
    ctx = ops.cross_attn_kv_fwd(qd[:, :H], qd[:, H:], md, B, NH, L, L, 0.125)
    qz = qd.clone()
    qz[B * L:] = 0  # (the self-attention kernels may read their pad rows)
    fused, _ = attention_fwd(qz, md, B, NH, L, (L + 7) // 8 * 8, 64, 0.125, 0.0, 1, True)
    torch.cuda.synchronize()
    e, e_fused = rel(ctx, wctx), rel(fused, wctx)
    print(f"L={L}: cross-attention kernel {e:.3e}, fused self-attention kernel {e_fused:.3e}")
    assert e <= 2e-2 and e <= 1.25 * e_fused + 2e-3


def test_cross_attention_refusals():
    from vcg_hip import _lib
    qb, kvb, mask, _ = _case(5, 9, torch.bfloat16)
    sentinel = torch.full((B * 5, H), 3.0, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.VcgError, match=r"\(-1\).*head dim"):
        _run(qb, kvb, mask, 5, 9, dh=32, ctx=sentinel)  # (H = 192 = 6 heads of 32)
    torch.cuda.synchronize()
    assert bool((sentinel == 3.0).all())
    from vcg_hip import ops
    with pytest.raises(ValueError, match="too small"):
        ops.cross_attn_kv_fwd(qb.to(DEV)[:, :H], kvb.to(DEV)[:, :2 * H], None, B, NH, 5, 13, 0.125)  # 39 > 27 + 8 rows


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pegasus_embed(dtype):
    from vcg_hip import _lib, ops
    V, NP, Hh, Bb, L = 101, 40, 128, 3, 7
    g = torch.Generator().manual_seed(5)
    tok, pos = torch.randn(V, Hh, generator=g), torch.randn(NP, Hh, generator=g)
    ids = torch.randint(0, V, (Bb, L), generator=g)
    scale = math.sqrt(Hh)  # (not a power of two: the product is not exact in fp32)
    s32 = float(np.float32(scale))
    for pos0 in (0, 33):
        out = ops.pegasus_embed_fwd(ids.to(DEV), tok.to(DEV), pos.to(DEV), Bb, L, Hh, dtype, scale, pos0)
        want = (s32 * tok.double()[ids] + pos.double()[pos0:pos0 + L][None]).float().to(dtype).view(Bb * L, Hh)
        assert torch.equal(_bits(out.cpu()), _bits(want))
    with pytest.raises(_lib.VcgError, match="position table"):
        ops.pegasus_embed_fwd(ids.to(DEV), tok.to(DEV), pos.to(DEV), Bb, L, Hh, dtype, scale, 34)
