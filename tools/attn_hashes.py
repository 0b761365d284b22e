"""SHA-256 of every output of the fused attention and Pegasus embedding kernels on seeded inputs, one `name hash` line
each, for the library VCG_LIB_PATH names (default: this tree's). Two builds compute the same bits iff their listings are
equal (profiles/attn_dkv_shared_ab.txt: the parent commit's library against this tree's, one process each).

  cross-attention (csrc/pegasus.hip), bf16 and fp32, p = 0 and 0.1: forward with statistics, backward (dq, dkv, the D
      workspace) at tests/test_gpu_pegasus_train_kernels.py's (Lq, Lk) pairs with its masks and NaN pads (B = 3, two
      heads), and once at the workload shape (B nh, Lq, Lk) = (256, 30, 512), bf16, p = 0.1;
  self-attention, L > 128 (csrc/bert_attn_long.hip), non-causal and causal, p = 0 and 0.1: ctx, dqkv and the whole
      stats buffer (zero-filled before the forward: (max, 1 / sum) of the rows q < L, then D) at
      tests/test_gpu_bert_attn_long.py's (L, kind) with B = 3, 12 heads; its varlen case (7 x 256) padded and packed;
      and once the workload shape B = 64, L = 512, p = 0.1 with prefix masks of seeded lengths;
  Pegasus embedding forward at tests/test_gpu_pegasus_kernels.py's shape, both dtypes, the inference entry and the
      training entry at p = 0 and 0.1.
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "video-chapter-generation_amd"))
from vcg_hip import _lib, ops  # noqa: E402
from vcg_hip.ops import P  # noqa: E402
from vcg_hip.bert import Packing  # noqa: E402

DEV = "cuda"
SEED = 0x1234567887654321


def emit(name, t):
    torch.cuda.synchronize()
    raw = t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
    print(f"{name} {hashlib.sha256(raw).hexdigest()}", flush=True)


def cross_mask(B, Lk):  # every key valid / two thirds valid with a hole / no valid key
    m = torch.zeros(B, Lk, dtype=torch.int64)
    m[0] = 1
    n = max(1, 2 * Lk // 3)
    m[1, :n] = 1
    if n >= 3:
        m[1, 1] = 0
    return m


def cross(tag, B, nh, Lq, Lk, dtype, p, mask, pad):
    H = nh * 64
    g = torch.Generator().manual_seed(7000 * Lq + Lk)
    qb = torch.full((B * Lq + pad, H + pad), float("nan"), dtype=dtype)
    kvb = torch.full((B * Lk + 8, 2 * H + pad), float("nan"), dtype=dtype)
    dob = torch.full((B * Lq + pad, H + pad), float("nan"), dtype=dtype)
    qb[:B * Lq, :H] = (torch.randn(B * Lq, H, generator=g) * 1.5).to(dtype)
    kvb[:B * Lk, :2 * H] = (torch.randn(B * Lk, 2 * H, generator=g) * 1.5).to(dtype)
    dob[:B * Lq, :H] = torch.randn(B * Lq, H, generator=g).to(dtype)
    q, kv, do = qb.to(DEV)[:, :H], kvb.to(DEV)[:, :2 * H], dob.to(DEV)[:, :H]
    md = None if mask is None else mask.to(DEV)
    stats = torch.zeros((B * nh, Lq, 2), dtype=torch.float32, device=DEV)
    ctx = ops.cross_attn_kv_fwd(q, kv, md, B, nh, Lq, Lk, 0.125, stats=stats, dropout_p=p, seed=SEED)
    dq = torch.zeros((B * Lq, H), dtype=dtype, device=DEV)
    dkv = torch.zeros((B * Lk, 2 * H), dtype=dtype, device=DEV)
    d_ws = torch.zeros(B * nh * Lq, dtype=torch.float32, device=DEV)
    _lib.call("vcg_cross_attn_kv_bwd", ops.dt_code(dtype), P(q), q.stride(0), P(kv), kv.stride(0), P(md), P(do),
              do.stride(0), P(stats), P(d_ws), P(dq), dq.stride(0), P(dkv), dkv.stride(0), B, nh, 64, Lq, Lk, 0.125,
              float(p), SEED, ops.stream())
    for name, t in (("ctx", ctx), ("stats", stats), ("dq", dq), ("dkv", dkv), ("D", d_ws)):
        emit(f"cross {tag} Lq={Lq} Lk={Lk} p={p} {name}", t)


def long_masks(kind, L):
    mask = torch.ones(3, L, dtype=torch.int64)
    if kind == "std":
        mask[0, L - L // 3:] = 0
        mask[1, :] = 0
        mask[2, :128] = 0
    else:
        mask[0, 128:] = 0
        mask[2, :] = 0
        mask[2, 200] = 1
    return mask


def self_attn(tag, qkv, dctx, mask, B, nh, L, p, seed, causal, seq=None, rows=None):
    H = nh * 64
    rows = B * L if rows is None else rows
    ctx = torch.zeros((rows, H), dtype=torch.bfloat16, device=DEV)
    dqkv = torch.zeros((rows, 3 * H), dtype=torch.bfloat16, device=DEV)
    stats = ops.bert_attn_stats(B, nh, L, DEV).zero_()
    Lp = (L + 7) // 8 * 8
    ops.bert_attn_fwd(qkv, mask, ctx, stats, B, nh, L, Lp, 0.125, p, seed, seq=seq, causal=causal)
    emit(f"self {tag} ctx", ctx)
    emit(f"self {tag} stats_fwd", stats)
    ops.bert_attn_bwd(qkv, dctx, ctx, mask, stats, dqkv, B, nh, L, Lp, 0.125, p, seed, seq=seq, causal=causal)
    emit(f"self {tag} dqkv", dqkv)
    emit(f"self {tag} stats_bwd", stats)


def main():
    _lib.call("vcg_init", 0)
    print(f"# library: {os.path.basename(_lib.LIB_PATH)}", flush=True)
    # ---- cross-attention
    for dtype, dn in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        for Lq, Lk in ((1, 300), (16, 128), (17, 31), (31, 129), (130, 1), (130, 300)):
            for p in (0.0, 0.1):
                cross(dn, 3, 2, Lq, Lk, dtype, p, cross_mask(3, Lk), 8)
    cross("bf16 workload B=16 nh=16", 16, 16, 30, 512, torch.bfloat16, 0.1, None, 0)
    # ---- long self-attention, padded
    nh, H = 12, 768
    for L, kind in ((129, "std"), (192, "std"), (250, "std"), (256, "std"), (512, "std"), (256, "tile2"), (300, "std")):
        B = 3
        g = torch.Generator().manual_seed(B * 1000 + L)
        qkv = (torch.randn(B * L + 8, 3 * H, generator=g) * 1.5).to(torch.bfloat16).to(DEV)
        dctx = torch.randn(B * L, H, generator=g).to(torch.bfloat16).to(DEV)
        mask = long_masks(kind, L).to(DEV)
        for causal in (False, True):
            for p in (0.0, 0.1):
                self_attn(f"L={L} {kind} causal={int(causal)} p={p}", qkv, dctx, mask, B, nh, L, p, 0x1234567890AB + L,
                          causal)
    # ---- the varlen case, padded and packed
    B, L = 7, 256
    mask_np = np.zeros((B, L), np.int64)
    for b, n in enumerate([256, 129, 128, 1, 200]):
        mask_np[b, :n] = 1
    mask_np[6, :100] = 1
    mask_np[6, 140:230] = 1
    pk = Packing(mask_np.copy(), DEV)
    rows = pk.rows.cpu()
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn(B * L + 8, 3 * H, generator=g) * 1.5).to(torch.bfloat16)
    dctx = torch.randn(B * L, H, generator=g).to(torch.bfloat16)
    qkv_k = torch.cat([qkv[rows], torch.zeros(8, 3 * H, dtype=qkv.dtype)]).to(DEV)
    dctx_k = dctx[rows].to(DEV)
    qkv, dctx, mask = qkv.to(DEV), dctx.to(DEV), torch.from_numpy(mask_np).to(DEV)
    for causal in (False, True):
        for p in (0.0, 0.1):
            self_attn(f"varlen padded causal={int(causal)} p={p}", qkv, dctx, mask, B, nh, L, p, 0xABCDEF, causal)
            self_attn(f"varlen packed causal={int(causal)} p={p}", qkv_k, dctx_k, pk.keys, B, nh, L, p, 0xABCDEF, causal,
                      seq=pk.seq, rows=pk.R)
    # ---- the workload shape
    B, L = 64, 512
    g = torch.Generator().manual_seed(64512)
    qkv = (torch.randn(B * L + 8, 3 * H, generator=g) * 1.5).to(torch.bfloat16).to(DEV)
    dctx = torch.randn(B * L, H, generator=g).to(torch.bfloat16).to(DEV)
    n = torch.randint(L // 2, L + 1, (B,), generator=g)
    mask = (torch.arange(L)[None, :] < n[:, None]).to(torch.int64).to(DEV)
    self_attn("workload B=64 L=512 causal=0 p=0.1", qkv, dctx, mask, B, nh, L, 0.1, 5, False)
    # ---- Pegasus embedding forward
    V, NP, Hh, Bb, Le = 101, 40, 128, 3, 7
    g = torch.Generator().manual_seed(5)
    tok, pos = torch.randn(V, Hh, generator=g).to(DEV), torch.randn(NP, Hh, generator=g).to(DEV)
    ids = torch.randint(0, V, (Bb, Le), generator=g).to(DEV)
    for dtype, dn in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        for p in (None, 0.0, 0.1):
            out = ops.pegasus_embed_fwd(ids, tok, pos, Bb, Le, Hh, dtype, Hh ** 0.5, 3, p=p, seed=SEED)
            emit(f"embed {dn} p={p}", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
