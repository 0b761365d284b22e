"""A torch statement of transformers.OpenAIGPTModel + a bias-free vocabulary head + cross-entropy (test helper; the
reference model/lang/gpt_hugface.py:82-101), written from a parameter dict {name: tensor} with transformers' names so it
runs in whatever dtype the dict holds (fp64: exact; fp32: the reference's arithmetic; fp32 under torch.autocast).

HF's arithmetic is written literally: the causal fill `w * b + -1e4 * (1 - b)`, the padding bias
`(1 - mask) * finfo(float32).min`, the tanh GELU of NewGELUActivation. Dropout (p > 0, `seed` = the engine's base seed)
drops exactly what the library's counter hash drops (tests/dropout_util.keep_mask) at the sites and with the per-site
seeds of vcg_hip/bert.py.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from dropout_util import keep_mask, row_keep


def causal_attention_ref(qkv, mask, dctx, B, nh, L, Lp, p, seed):
    """tests/bert_attn_ref.ref_attention with OpenAIGPT's causal fill: -> (ctx [B L][H], dQ | dK | dV [B L][3 H]) in
    fp64 for the upstream gradient dctx (head dim 64, scale 1 / 8)."""
    H = nh * 64
    x = qkv[:B * L].double().cpu().view(B, L, 3, nh, 64).permute(2, 0, 3, 1, 4)  # [3, B, nh, L, 64]
    q, k, v = (t.clone().requires_grad_(True) for t in x)
    w = q @ k.transpose(-1, -2) / 8.0
    b = torch.tril(torch.ones(L, L, dtype=torch.float64))
    w = w * b + -1e4 * (1 - b)
    w = w + (1.0 - mask.double().cpu())[:, None, None, :] * torch.finfo(torch.float32).min
    P = torch.softmax(w, dim=-1)
    z = np.arange(B * nh)[:, None, None]
    qi = np.arange(L)[None, :, None]
    kj = np.arange(L)[None, None, :]
    keep = torch.from_numpy(keep_mask(seed, (z * L + qi) * Lp + kj, p)).view(B, nh, L, L)
    o = (P * keep / (1.0 - p)) @ v
    do = dctx.double().cpu().view(B, L, nh, 64).permute(0, 2, 1, 3)
    (o * do).sum().backward()
    ctx = o.permute(0, 2, 1, 3).reshape(B * L, H)
    dqkv = torch.stack([q.grad, k.grad, v.grad]).permute(1, 3, 0, 2, 4).reshape(B * L, 3 * H)
    return ctx, dqkv


def new_gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def new_gelu_grad(x):
    t = torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))
    return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * math.sqrt(2.0 / math.pi) * (1 + 3 * 0.044715 * x * x)


def _site_seed(base, layer, site):  # vcg_hip/bert.py _seed
    return (base * 0x9E3779B1 + layer * 7919 + site * 104729) & ((1 << 63) - 1)


def _drop(x2d, p, seed):
    if p <= 0:
        return x2d
    rows, H = x2d.shape
    return x2d * torch.from_numpy(row_keep(seed, rows, H, p)).to(x2d.dtype) / (1.0 - p)


def gpt_hidden(P, ids, mask, n_head, prefix="", eps=1e-5, p_drop=0.0, seed=0):
    """transformers OpenAIGPTModel.forward -> last hidden state [B, L, H]."""
    B, L = ids.shape
    tok, pos = P[prefix + "tokens_embed.weight"], P[prefix + "positions_embed.weight"]
    H = tok.shape[1]
    dh = H // n_head
    Lp = (L + 7) // 8 * 8
    h = tok[ids] + pos[torch.arange(L)][None]
    h = _drop(h.reshape(B * L, H), p_drop, _site_seed(seed, 0, 0)).view(B, L, H)
    fdt = h.dtype
    add = ((1.0 - mask.to(fdt)) * torch.finfo(torch.float32).min)[:, None, None, :]
    tril = torch.tril(torch.ones(L, L, dtype=fdt))
    n_layer = 1 + max(int(k[len(prefix) + 2:].split(".")[0]) for k in P if k.startswith(prefix + "h."))
    for i in range(n_layer):
        g = lambda n: P[f"{prefix}h.{i}.{n}"]  # noqa: E731
        x = h @ g("attn.c_attn.weight") + g("attn.c_attn.bias")
        q, k, v = (t.view(B, L, n_head, dh).permute(0, 2, 1, 3) for t in x.split(H, dim=2))
        w = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
        w = w * tril + -1e4 * (1 - tril)
        w = torch.softmax(w + add, dim=-1)
        if p_drop > 0:
            z = np.arange(B * n_head)[:, None, None]
            idx = (z * L + np.arange(L)[None, :, None]) * Lp + np.arange(L)[None, None, :]
            keep = torch.from_numpy(keep_mask(_site_seed(seed, i + 1, 1), idx, p_drop)).view(B, n_head, L, L)
            w = w * keep.to(w.dtype) / (1.0 - p_drop)
        a = (w.to(v.dtype) @ v).permute(0, 2, 1, 3).reshape(B, L, H)
        a = a @ g("attn.c_proj.weight") + g("attn.c_proj.bias")
        a = _drop(a.reshape(B * L, H), p_drop, _site_seed(seed, i + 1, 2)).view(B, L, H)
        n = F.layer_norm(h + a, (H,), g("ln_1.weight"), g("ln_1.bias"), eps)
        m = new_gelu(n @ g("mlp.c_fc.weight") + g("mlp.c_fc.bias")) @ g("mlp.c_proj.weight") + g("mlp.c_proj.bias")
        m = _drop(m.reshape(B * L, H), p_drop, _site_seed(seed, i + 1, 3)).view(B, L, H)
        h = F.layer_norm(n + m, (H,), g("ln_2.weight"), g("ln_2.bias"), eps)
    return h


def gpt_lm(P, ids, mask, targets, n_head, autocast=False, **kw):
    """GPTHugface.forward: (logits [B, L, V], mean cross-entropy over targets != -1)."""
    h = gpt_hidden(P, ids, mask, n_head, prefix="base_model.", **kw)
    logits = F.linear(h, P["head.weight"])
    sel = targets != -1
    loss = F.cross_entropy(logits[sel].float() if autocast else logits[sel], targets[sel])
    return logits, loss
