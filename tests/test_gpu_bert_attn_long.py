"""Fused BERT self-attention for texts of 129 to 512 tokens (bert_attn_long.hip: 128 x 128 tiles, online softmax,
two-kernel deterministic backward) against an fp64 torch statement of HF BertSelfAttention (eager: scores * scale +
(1 - mask) * finfo(f32).min, softmax, dropout, PV; bert_hugface.py:20 -> BertModel), against the unfused kernels
(QK^T GEMM -> attn_softmax -> PV GEMM) it replaces at these lengths, packed against padded, and inside whole train steps.
The fp64 reference is tests/bert_attn_ref.py, shared with tests/test_gpu_bert_attn.py. L = 300: three key tiles, the last
with 44 keys, so its second 64-key half is skipped in the backward kernels and its first is partial.

Tolerance (bf16 operands, fp32 accumulation; the L <= 128 kernels' bounds): relative Frobenius error of ctx / dQ / dK /
dV vs fp64 <= 2e-2, and no worse than 1.25 x the unfused bf16 path's own error + 2e-3."""
import numpy as np
import pytest
import torch

from bert_attn_ref import ref_attention, rel

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _masks(kind, L):
    mask = torch.ones(3, L, dtype=torch.int64)
    if kind == "std":
        mask[0, L - L // 3:] = 0  # padded keys
        mask[1, :] = 0            # no key at all -> uniform rows (HF finfo.min)
        mask[2, :128] = 0         # the whole first key tile masked: the running max stays -inf through it
    else:  # "tile2": the second key tile entirely masked
        mask[0, 128:] = 0         # exactly keys 0 - 127 valid
        mask[2, :] = 0
        mask[2, 200] = 1          # one valid key, in the second tile
    return mask


@pytest.mark.parametrize("L,p,kind", [(129, 0.1, "std"), (192, 0.0, "std"), (250, 0.1, "std"), (256, 0.1, "std"),
                                      (512, 0.0, "std"), (512, 0.1, "std"), (256, 0.1, "tile2"),
                                      (300, 0.1, "std")])
def test_long_fused_attention_matches_fp64_and_unfused(L, p, kind):
    from vcg_hip import _lib
    from vcg_hip.bert import attention_bwd, attention_fwd
    _lib.call("vcg_init", 0)
    B, nh, H = 3, 12, 768
    Lp = (L + 7) // 8 * 8
    g = torch.Generator().manual_seed(B * 1000 + L)
    qkv = (torch.randn(B * L + 8, 3 * H, generator=g) * 1.5).to(torch.bfloat16).to(DEV)
    mask = _masks(kind, L).to(DEV)
    dctx = torch.randn(B * L, H, generator=g).to(torch.bfloat16).to(DEV)
    seed = 0x1234567890AB + L
    ref_ctx, ref_dqkv = ref_attention(qkv, mask, dctx, B, nh, L, Lp, p, seed)
    out = {}
    for fused in (True, False):
        ctx, att = attention_fwd(qkv, mask, B, nh, L, Lp, 64, 0.125, p, seed, fused)
        dqkv = attention_bwd(qkv, dctx, ctx, mask, att, B, nh, L, Lp, 64, 0.125, p, seed)
        if fused:  # only O(L) state per (sequence, head), and a deterministic backward
            assert set(att) == {"stats"}
            assert att["stats"].numel() * 4 == _lib.query("vcg_bert_attn_stats_bytes", B, nh, L) <= B * nh * 512 * 12
            again = attention_bwd(qkv, dctx, ctx, mask, att, B, nh, L, Lp, 64, 0.125, p, seed)
            assert torch.equal(again, dqkv)
        torch.cuda.synchronize()
        assert torch.isfinite(ctx).all() and torch.isfinite(dqkv).all()
        out[fused] = (ctx, dqkv)
    for name, sl in (("ctx", None), ("dQ", slice(0, H)), ("dK", slice(H, 2 * H)), ("dV", slice(2 * H, 3 * H))):
        f = out[True][0] if sl is None else out[True][1][:, sl]
        u = out[False][0] if sl is None else out[False][1][:, sl]
        r = ref_ctx if sl is None else ref_dqkv[:, sl]
        ef, eu = rel(f, r), rel(u, r)
        print(f"L={L} p={p} {kind} {name}: fused {ef:.3e} unfused {eu:.3e}")
        assert ef <= 2e-2 and ef <= 1.25 * eu + 2e-3, (name, ef, eu)


def test_lengths_past_512_stay_unsupported():
    from vcg_hip import _lib
    from vcg_hip.bert import attention_fwd
    _lib.call("vcg_init", 0)
    qkv = torch.zeros(520 + 8, 3 * 768, dtype=torch.bfloat16, device=DEV)
    mask = torch.ones(1, 520, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.VcgError, match="512"):
        attention_fwd(qkv, mask, 1, 12, 520, 520, 64, 0.125, 0.0, 1, True)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_long_varlen_attention_matches_padded(p):
    """Packed (unpadded) sequences at L = 256: the kept rows' ctx and dQ | dK | dV equal the padded kernels' bit for bit
    where the kept rows are a prefix of the padded ones (lengths on both sides of the 128-row tile and of one row), given
    the dropped rows' upstream gradient is zero as in the model; a sequence with a masked hole matches within rounding
    without dropout; a sequence without any key keeps all its rows."""
    from vcg_hip import _lib
    from vcg_hip.bert import Packing, attention_bwd, attention_fwd
    _lib.call("vcg_init", 0)
    B, L, nh, H = 7, 256, 12, 768
    Lp = L
    lens = [256, 129, 128, 1, 200]
    mask_np = np.zeros((B, L), np.int64)
    for b, n in enumerate(lens):
        mask_np[b, :n] = 1
    # sequence 5: no key at all, every row kept; sequence 6: a hole (kept rows 0-99, 140-229: positions shift when packed)
    mask_np[6, :100] = 1
    mask_np[6, 140:230] = 1
    pk = Packing(mask_np.copy(), DEV)
    rows = pk.rows.cpu()
    assert pk.R == sum(lens) + 256 + 190
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn(B * L + 8, 3 * H, generator=g) * 1.5).to(torch.bfloat16)
    dctx = torch.randn(B * L, H, generator=g).to(torch.bfloat16)
    drop = torch.ones(B * L, dtype=torch.bool)
    drop[rows] = False
    dctx[drop] = 0
    seed = 0xABCDEF + int(p * 10)
    mask = torch.from_numpy(mask_np).to(DEV)
    ctx_p, att_p = attention_fwd(qkv.to(DEV), mask, B, nh, L, Lp, 64, 0.125, p, seed, True)
    dqkv_p = attention_bwd(qkv.to(DEV), dctx.to(DEV), ctx_p, mask, att_p, B, nh, L, Lp, 64, 0.125, p, seed)
    qkv_k = torch.cat([qkv[rows], torch.zeros(8, 3 * H, dtype=qkv.dtype)]).to(DEV)
    ctx_k, att_k = attention_fwd(qkv_k, pk.keys, B, nh, L, Lp, 64, 0.125, p, seed, True, seq=pk.seq, rows=pk.R)
    dqkv_k = attention_bwd(qkv_k, dctx[rows].to(DEV), ctx_k, pk.keys, att_k, B, nh, L, Lp, 64, 0.125, p, seed,
                           seq=pk.seq, rows=pk.R)
    torch.cuda.synchronize()
    ctx_p, dqkv_p, ctx_k, dqkv_k = (t.cpu() for t in (ctx_p, dqkv_p, ctx_k, dqkv_k))
    assert torch.isfinite(ctx_k.float()).all() and torch.isfinite(dqkv_k.float()).all()
    seq = pk.seq.cpu().tolist()
    for b in range(B):
        kr = rows[seq[b]:seq[b + 1]]
        a, c = slice(seq[b], seq[b + 1]), kr
        if b == 6:  # (with dropout its shifted key positions draw other dropout counters: another valid sample)
            if p == 0:
                assert rel(ctx_k[a], ctx_p[c]) < 5e-3 and rel(dqkv_k[a], dqkv_p[c]) < 5e-3, b
        else:
            assert torch.equal(ctx_k[a], ctx_p[c]) and torch.equal(dqkv_k[a], dqkv_p[c]), b


def test_long_fused_attention_in_bert_step_matches_unfused(monkeypatch):
    """A whole bf16 text-only train step (BERT + head, dropout 0.1) at L = 256 with the fused kernels vs the unfused ones
    (same weights, inputs and dropout seeds): logits and every BERT parameter gradient within bf16 tolerance."""
    from vcg_hip import _lib, synth
    from vcg_hip.bert import BertEncoderEngine
    from vcg_hip.build import build_model
    from vcg_hip.functions import cross_entropy
    _lib.call("vcg_init", 0)
    _, ids, mask, labels = synth.clip_batch(4, 1, 8, 8, 256, seed=7, device=DEV)
    mask[1, 140:] = 0
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setattr(BertEncoderEngine, "fused_attn", flag == "1")
        m = build_model("text", seed=7, device=DEV, precision="bf16", dropout=0.1).train()
        torch.manual_seed(11)  # the dropout seeds (vcg_hip.nn.new_seed) come from torch's RNG
        logits, _ = m(ids, mask)
        cross_entropy(logits, labels).backward()
        torch.cuda.synchronize()
        res[flag] = (logits.detach().float().cpu(),
                     {n: p.grad.detach().float().cpu().clone() for n, p in m.named_parameters() if p.grad is not None})
    l1, g1 = res["1"]
    l0, g0 = res["0"]
    assert torch.isfinite(l1).all() and torch.isfinite(l0).all()
    print("logits max diff %.3e" % (l1 - l0).abs().max().item())
    assert (l1 - l0).abs().max().item() < 5e-2
    assert g1.keys() == g0.keys() and len(g1) > 100
    # the key bias gradient is zero in exact arithmetic (a row-constant score shift leaves the softmax unchanged):
    # both paths hold rounding noise there, compared by its size instead
    kb = [n for n in g1 if n.endswith("attention.self.key.bias")]
    assert len(kb) == 12
    for n in kb:
        ref = g1[n.replace("key.bias", "query.bias")].norm()
        assert g1[n].norm() < 5e-2 * ref and g0[n].norm() < 5e-2 * ref, (n, g1[n].norm(), g0[n].norm(), ref)
    errs = sorted((rel(g1[n], g0[n]), n) for n in g1 if n not in kb and g0[n].norm() > 0)
    print("grad rel errors: median %.3e, worst %s" % (errs[len(errs) // 2][0], errs[-3:]))
    assert errs[len(errs) // 2][0] < 3e-2 and errs[-1][0] < 1e-1


def test_long_unpadded_bert_in_two_stream_step(monkeypatch):
    """A whole bf16 TwoStream train step (dropout 0) at L = 256 with BERT's padded rows dropped (unpad) and its last
    layer past the attention on the position-0 rows only (cls_last) vs every row computed: prefix masks, so the logits
    are bit-identical and every parameter gradient is within fp32 summation-order rounding; the packed path must
    actually have run (fewer rows than B * L)."""
    from vcg_hip import _lib, synth
    from vcg_hip.bert import BertEncoderEngine, PackingRequest
    from vcg_hip.build import build_two_stream
    from vcg_hip.functions import cross_entropy
    _lib.call("vcg_init", 0)
    B, T, HW, L = 4, 2, 64, 256
    frames, ids, mask, labels = synth.clip_batch(B, T, HW, HW, L, seed=21, device=DEV)
    assert (mask == 0).any()
    res = {}
    for unpad in (True, False):  # (the reference arm also runs the last layer on every row: cls_last off)
        monkeypatch.setattr(BertEncoderEngine, "unpad", unpad)
        monkeypatch.setattr(BertEncoderEngine, "cls_last", unpad)
        PackingRequest._last = PackingRequest._mirror = None
        m = build_two_stream(clip_frame_num=T, seed=5, device=DEV, precision="bf16", dropout=0.0).train()
        logits, _ = m(frames, ids, mask)
        cross_entropy(logits, labels).backward()
        torch.cuda.synchronize()
        if unpad:
            assert PackingRequest._last is not None and PackingRequest._last[2].R < B * L
            assert PackingRequest._last[2].R == int(mask.sum())
        else:
            assert PackingRequest._last is None
        res[unpad] = (logits.detach().float().cpu(),
                      {n: p.grad.detach().double().cpu().clone() for n, p in m.named_parameters() if p.grad is not None})
    (l1, g1), (l0, g0) = res[True], res[False]
    assert torch.isfinite(l1).all()
    assert torch.equal(l1, l0)
    assert g1.keys() == g0.keys()
    errs = sorted((rel(g1[n], g0[n]), n) for n in g1 if g0[n].norm() > 1e-3 * max(v.norm() for v in g0.values()))
    print("unpadded vs padded grad rel errors: median %.3e, worst %s" % (errs[len(errs) // 2][0], errs[-3:]))
    assert errs[-1][0] < 2e-3, errs[-3:]
