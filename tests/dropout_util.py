"""The library's dropout mask restated in numpy (test helper).

`keep_mask(seed, idx, p)` is `dropout_keep` of csrc/common.h, vectorised: a 32-bit murmur3 finaliser of
(idx * golden ratio) ^ seed, kept when the top 24 bits as a fraction of 2^24 are >= p. The fp64 references of the
GPU tests drop exactly the elements the kernels drop. Element index spaces, as the kernels use them:
`row * H + c` (embed_ln, ln) and `(z * L + row) * Lp + j` (attention softmax / fused attention).
"""
import numpy as np


def keep_mask(seed, idx, p):
    """common.h dropout_keep, vectorised (uint32 wrap-around arithmetic). idx: integer ndarray -> bool ndarray."""
    idx = np.asarray(idx)
    if p <= 0:
        return np.ones(idx.shape, bool)
    with np.errstate(over="ignore"):
        h = (idx.astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32) * np.uint32(0x9E3779B1)
        h ^= np.uint32(seed & 0xFFFFFFFF)
        h += np.uint32((seed >> 32) & 0xFFFFFFFF)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0) >= np.float32(p)


def row_keep(seed, rows, H, p):
    """Mask [rows][H] of the row-major element space row * H + c (vcg_embed_ln_fwd, vcg_ln_fwd)."""
    return keep_mask(seed, np.arange(rows * H, dtype=np.int64).reshape(rows, H), p)


def score_keep(seed, Z, L, Lp, p):
    """Mask [Z][L][Lp] of the score space (z * L + row) * Lp + j (vcg_attn_softmax_fwd; pad columns included)."""
    return keep_mask(seed, np.arange(Z * L * Lp, dtype=np.int64).reshape(Z, L, Lp), p)
