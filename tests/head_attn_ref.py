"""The attention fusion head (csrc/head_attn.hip) restated in plain torch (test helper), with the shapes, dropout
seeds and LDS arithmetic that tests/test_cpu_head_attn_ref.py and tests/test_gpu_head_attn_kernels.py share.

`head_attn_ref` is SelfAttention.forward of the reference head over X = cat([Vout, Lout]) per window, all query
rows, in the dtype of its inputs (fp64 for the references, fp32 for the error yardstick); attn_drop acts on query
row 0 only, the one row that reaches the output, with the library's counter-hash mask (tests/dropout_util.py) at
element (b * nh + h) * T1 * T1 + j of the reference's [B, nh, T1, T1] attention tensor. Every gradient comes from
autograd through it (`head_attn_grads`).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from dropout_util import keep_mask

PARAMS = ("Wq", "bq", "Wk", "bk", "Wv", "bv", "Wp", "bp")
LDS_LIMIT = 64 * 1024

# (B, T, hid, n_head, O): each the smallest that reaches its edge
SHAPES = [
    (1, 1, 8, 1, 1),        # minimum: T1 = 2, one head, O = 1
    (3, 7, 24, 4, 2),       # T1 = 8, exactly one full pass of 8 tokens; hs = 6; hid < one wave
    (2, 8, 96, 3, 5),       # T1 = 9, second pass with a one-token tail; hs = 32; O = 5 > 4 waves: the proj loop wraps
    (5, 16, 128, 4, 2),     # the fusion head as benchmarked: T1 = 17, three passes
    (2, 16, 256, 16, 256),  # hid, nh and O at their maxima; 3 * hid > 256 threads; the window "self_attn" form
    (2, 19, 256, 4, 2),     # largest T that fits at hid 256 (63 808 B of LDS)
    (1, 40, 128, 4, 2),     # largest T that fits at hid 128 (64 656 B), six passes
]
# one step outside the LDS limit, and the advertised maximum of the other limits
REFUSED_LDS = [(1, 20, 256, 4, 2), (1, 41, 128, 4, 2), (1, 63, 256, 16, 2)]
P_DROP = 0.3
# attn_drop seed per shape at p = 0.3: drops 10 % .. 50 % of the B * nh * T1 row-0 elements and leaves every head a
# key in every window (checked by tests/test_cpu_head_attn_ref.py)
SEEDS = {
    (1, 1, 8, 1, 1): 2,  # two elements: one of them dropped
    (3, 7, 24, 4, 2): 11,
    (2, 8, 96, 3, 5): 12,
    (5, 16, 128, 4, 2): 13,
    (2, 16, 256, 16, 256): 14,
    (2, 19, 256, 4, 2): 15,
    (1, 40, 128, 4, 2): 16,
}


def fwd_lds_bytes(T, hid, nh):
    """Dynamic LDS of vcg_head_attn_fwd: X, K, V [T1][hid], q0 / y0 [hid], P [nh][T1], f32."""
    T1 = T + 1
    return (3 * T1 * hid + 2 * hid + nh * T1) * 4


def bwd_lds_bytes(T, hid, nh):
    """Dynamic LDS of vcg_head_attn_bwd: dK, dV [T1][hid], dy0 / dq0 [hid], P, dS [nh][T1], f32."""
    T1 = T + 1
    return (2 * T1 * hid + 2 * hid + 2 * nh * T1) * 4


def row0_keep(B, nh, T1, p, seed):
    """Keep mask [B][nh][T1] of attention row 0 (bool ndarray)."""
    idx = (np.arange(B * nh, dtype=np.int64).reshape(B, nh, 1) * (T1 * T1) + np.arange(T1, dtype=np.int64))
    return keep_mask(seed, idx, p)


def make_inputs(shape, dtype):
    """Vout / Lout as the ReLU projections leave them, except that negatives stay in too (about a third each of
    exact zeros, negatives and positives, rounded to the storage dtype), so that relu_mask = 1 and 0 give different
    gradients; weights scaled by hid ** -0.5, non-zero biases, random dlogits. Returns a dict of CPU tensors
    (Vout / Lout in `dtype`, everything else fp32)."""
    B, T, hid, nh, O = shape
    g = torch.Generator().manual_seed(B * 1009 + T * 101 + hid * 7 + nh * 3 + O)

    def act(n):
        a = torch.randn(n, hid, generator=g)
        a[torch.rand(n, hid, generator=g) < 0.3] = 0.0
        return a.to(dtype)
    d = {"Vout": act(B * T), "Lout": act(B)}
    for w in ("q", "k", "v"):
        d["W" + w] = torch.randn(hid, hid, generator=g) * hid ** -0.5
        d["b" + w] = torch.randn(hid, generator=g) * 0.5
    d["Wp"] = torch.randn(O, hid, generator=g) * hid ** -0.5
    d["bp"] = torch.randn(O, generator=g) * 0.5
    d["dlogits"] = torch.randn(B, O, generator=g)
    return d


def head_attn_ref(Vout, Lout, Wq, bq, Wk, bk, Wv, bv, Wp, bp, n_head, p=0.0, seed=0):
    """One forward in the dtype of Vout. Returns a dict: logits, prob [B, O], and the intermediates the kernel saves:
    X, K, V [B, T1, hid], q0, y0 [B, hid], P [B, nh, T1] (row 0 of the softmax, before dropout). bp may be None."""
    B, hid = Lout.shape
    T = Vout.numel() // (B * hid)
    T1, nh, hs = T + 1, n_head, hid // n_head
    X = torch.cat([Vout.view(B, T, hid), Lout[:, None]], 1)
    K, Q, V = F.linear(X, Wk, bk), F.linear(X, Wq, bq), F.linear(X, Wv, bv)

    def heads(t):
        return t.view(B, T1, nh, hs).transpose(1, 2)
    att = torch.softmax((heads(Q) @ heads(K).transpose(-2, -1)) * (1.0 / math.sqrt(hs)), dim=-1)  # [B, nh, T1, T1]
    P0 = att[:, :, 0, :]
    if p > 0:
        keep = torch.from_numpy(row0_keep(B, nh, T1, p, seed)).to(att.dtype)
        att = torch.cat([(P0 * keep * (1.0 / (1.0 - p)))[:, :, None, :], att[:, :, 1:, :]], 2)
    y = (att @ heads(V)).transpose(1, 2).reshape(B, T1, hid)
    y0 = y[:, 0]
    logits = F.linear(y0, Wp, bp)
    return {"logits": logits, "prob": torch.softmax(logits, 1), "X": X, "K": K, "V": V, "q0": Q[:, 0], "y0": y0,
            "P": P0}


def head_attn_grads(inp, n_head, p, seed, relu_mask, dtype=torch.float64, bias_p=True):
    """Forward and autograd backward of `inp` (a make_inputs dict) computed in `dtype`. Returns (forward dict,
    gradient dict with dVout, dLout, dWq .. dbp and dK, the gradient of the key block)."""
    leaves = {k: inp[k].to(dtype).clone().requires_grad_() for k in ("Vout", "Lout") + PARAMS}
    out = head_attn_ref(leaves["Vout"], leaves["Lout"], *(leaves[k] for k in PARAMS[:-1]),
                        leaves["bp"] if bias_p else None, n_head, p, seed)
    names = [k for k in leaves if bias_p or k != "bp"]
    gr = torch.autograd.grad(out["logits"], [leaves[k] for k in names] + [out["K"]], inp["dlogits"].to(dtype),
                             allow_unused=True)
    grads = {"d" + k: g for k, g in zip(names + ["K"], gr)}
    if relu_mask:
        grads["dVout"] = grads["dVout"] * (leaves["Vout"].detach() > 0)
        grads["dLout"] = grads["dLout"] * (leaves["Lout"].detach() > 0)
    return {k: v.detach() for k, v in out.items()}, grads
