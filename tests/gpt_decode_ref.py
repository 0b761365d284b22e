"""fp64 statements of what csrc/gpt_decode.hip computes (test helper, no GPU):

  * attn_one_query: one query row over a cache, softmax(scale q K^T) V;
  * keep_set / sample_ref / greedy_ref: the reference sampler (common_utils/language_model_utils.py: logits /
    temperature, top_k_logits whose `out < v[:, [-1]]` cut keeps every tie at the k-th value, softmax) with the draw
    stated as an inverse CDF in vocabulary order: the first kept index whose running probability exceeds u.
"""
import numpy as np


def attn_one_query(q, K, V, scale):
    """q [dh], K / V [n, dh] -> ctx [dh], all fp64."""
    s = (K.astype(np.float64) @ q.astype(np.float64)) * scale
    w = np.exp(s - s.max())
    return (w / w.sum()) @ V.astype(np.float64)


def keep_set(logits, temperature, top_k):
    """(z fp64 [V], keep bool [V]) of one row; top_k 0 / None: no cut."""
    z = np.asarray(logits, dtype=np.float64) / float(temperature)
    if not top_k or top_k >= z.size:
        return z, np.ones(z.size, dtype=bool)
    kth = np.sort(z)[::-1][top_k - 1]
    return z, z >= kth


def cdf_ref(logits, temperature, top_k):
    """(kept indices in vocabulary order, their running probabilities fp64, total = 1)"""
    z, keep = keep_set(logits, temperature, top_k)
    idx = np.flatnonzero(keep)
    e = np.exp(z[idx] - z[idx].max())
    return idx, np.cumsum(e / e.sum())


def sample_ref(logits, temperature, top_k, u):
    """(token, its probability): the first kept index whose running probability exceeds u (u in [0, 1))."""
    idx, cdf = cdf_ref(logits, temperature, top_k)
    j = int(np.searchsorted(cdf, u, side="right"))
    j = min(j, idx.size - 1)  # (the fp64 running sum may end a rounding below 1)
    return int(idx[j]), float(cdf[j] - (cdf[j - 1] if j else 0.0))


def greedy_ref(logits):
    """argmax, lowest index on equal values"""
    return int(np.argmax(np.asarray(logits, dtype=np.float64)))


def midpoints(logits, temperature, top_k, min_width=1e-4):
    """u at the midpoint of every CDF step wider than min_width, with the token each must give."""
    idx, cdf = cdf_ref(logits, temperature, top_k)
    lo = np.concatenate([[0.0], cdf[:-1]])
    wide = np.flatnonzero(cdf - lo > min_width)
    return 0.5 * (lo[wide] + cdf[wide]), idx[wide]
