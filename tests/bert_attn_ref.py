"""The fused BERT self-attention kernels' fp64 reference (test helper), shared by tests/test_gpu_bert_attn.py (L <= 128)
and tests/test_gpu_bert_attn_long.py (128 < L <= 512).

`ref_attention` is HF BertSelfAttention (eager: scores * scale + (1 - mask) * finfo(f32).min, softmax, dropout, PV;
bert_hugface.py:20 -> BertModel) in plain fp64 torch on the CPU over the packed [rows][3 H] q | k | v layout of the
kernels, head dim 64; its dropout mask is the library's counter hash (tests/dropout_util.py) at element
(z * L + q) * Lp + key, so it drops exactly the probabilities the kernels drop. The gradients come from autograd.
"""
import numpy as np
import torch

from dropout_util import keep_mask


def ref_attention(qkv, mask, dctx, B, nh, L, Lp, p, seed):
    """-> (ctx [B * L][H], dQ | dK | dV [B * L][3 H]) in fp64 for the upstream gradient dctx."""
    H = nh * 64
    x = qkv[:B * L].double().cpu().view(B, L, 3, nh, 64).permute(2, 0, 3, 1, 4)  # [3, B, nh, L, 64]
    q, k, v = (t.clone().requires_grad_(True) for t in x)
    add = (1.0 - mask.double().cpu())[:, None, None, :] * torch.finfo(torch.float32).min
    P = torch.softmax(q @ k.transpose(-1, -2) / 8.0 + add, dim=-1)
    z = np.arange(B * nh)[:, None, None]
    qi = np.arange(L)[None, :, None]
    kj = np.arange(L)[None, None, :]
    keep = torch.from_numpy(keep_mask(seed, (z * L + qi) * Lp + kj, p)).view(B, nh, L, L)
    Pd = P * keep / (1.0 - p)
    o = Pd @ v
    do = dctx.double().cpu().view(B, L, nh, 64).permute(0, 2, 1, 3)
    (o * do).sum().backward()
    ctx = o.permute(0, 2, 1, 3).reshape(B * L, H)
    dqkv = torch.stack([q.grad, k.grad, v.grad]).permute(1, 3, 0, 2, 4).reshape(B * L, 3 * H)
    return ctx, dqkv


def rel(a, b):
    """Relative Frobenius error of a against b, in fp64."""
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()
