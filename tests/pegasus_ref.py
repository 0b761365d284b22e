"""A torch statement of transformers.PegasusForConditionalGeneration (eval mode, eager attention; test helper for the
reference's model/lang/pegasus_hugface.py:89-102), written from a parameter dict {name: tensor} with transformers' names
so it runs in whatever dtype the dict holds (fp64: exact; fp32: the reference's arithmetic; fp32 under torch.autocast).

HF's arithmetic is written literally: the embedding scale sqrt(d_model) and the lookup of the sinusoidal table by
position, pre-LayerNorm blocks (h + Attn(LN(h)), h + FFN(LN(h))), the query scaled by dh^-0.5, the padding bias
finfo(float32).min, the causal mask of the decoder's self-attention (the same fill; a position that is both future and
padded keeps one fill), ReLU, the final LayerNorm of each stack, the bias-free head.
"""
import math

import torch
import torch.nn.functional as F

FMIN = torch.finfo(torch.float32).min


def _attn(P, pre, xq, xkv, bias, nh):
    """HF PegasusAttention (eager): xq [B, Lq, H] queries' input, xkv [B, Lk, H] keys' / values' input, bias
    [B, 1, Lq | 1, Lk] additive or None"""
    B, Lq, H = xq.shape
    Lk = xkv.shape[1]
    dh = H // nh
    lin = lambda n, x: F.linear(x, P[f"{pre}.{n}.weight"], P[f"{pre}.{n}.bias"])  # noqa: E731
    q = (lin("q_proj", xq) * dh ** -0.5).view(B, Lq, nh, dh).transpose(1, 2)
    k = lin("k_proj", xkv).view(B, Lk, nh, dh).transpose(1, 2)
    v = lin("v_proj", xkv).view(B, Lk, nh, dh).transpose(1, 2)
    w = q @ k.transpose(-1, -2)
    if bias is not None:
        w = w + bias.to(w.dtype)
    w = torch.softmax(w, dim=-1)
    o = (w.to(v.dtype) @ v).transpose(1, 2).reshape(B, Lq, H)
    return lin("out_proj", o)


def _ln(P, pre, x, eps):
    return F.layer_norm(x, (x.shape[-1],), P[pre + ".weight"], P[pre + ".bias"], eps)


def _n_layers(P, pre):
    return 1 + max(int(k[len(pre):].split(".")[0]) for k in P if k.startswith(pre))


def _embed(P, stack, ids, scale):
    L = ids.shape[1]
    return P["model.shared.weight"][ids] * scale + P[f"model.{stack}.embed_positions.weight"][torch.arange(L)][None]


def _pad_bias(mask):
    """[B, 1, 1, Lk]: finfo(float32).min at the masked keys"""
    return ((mask == 0).to(torch.float64) * FMIN)[:, None, None, :]


def pegasus_encoder(P, ids, mask, nh, eps=1e-5, scale_embedding=True):
    """-> the encoder's last hidden state [B, Ls, H]"""
    H = P["model.shared.weight"].shape[1]
    h = _embed(P, "encoder", ids, math.sqrt(H) if scale_embedding else 1.0)
    bias = _pad_bias(mask)
    for i in range(_n_layers(P, "model.encoder.layers.")):
        pre = f"model.encoder.layers.{i}"
        x = _ln(P, pre + ".self_attn_layer_norm", h, eps)
        h = h + _attn(P, pre + ".self_attn", x, x, bias, nh)
        x = _ln(P, pre + ".final_layer_norm", h, eps)
        h = h + F.linear(torch.relu(F.linear(x, P[pre + ".fc1.weight"], P[pre + ".fc1.bias"])),
                         P[pre + ".fc2.weight"], P[pre + ".fc2.bias"])
    return _ln(P, "model.encoder.layer_norm", h, eps)


def pegasus_decoder(P, dec_ids, dec_mask, enc, enc_mask, nh, eps=1e-5, scale_embedding=True):
    """-> the decoder's last hidden state [B, Ld, H]"""
    B, Ld = dec_ids.shape
    H = P["model.shared.weight"].shape[1]
    h = _embed(P, "decoder", dec_ids, math.sqrt(H) if scale_embedding else 1.0)
    future = torch.triu(torch.ones(Ld, Ld, dtype=torch.bool), 1)[None, None]
    blocked = future | (dec_mask == 0)[:, None, None, :]
    self_bias = blocked.to(torch.float64) * FMIN  # [B, 1, Ld, Ld]
    cross_bias = _pad_bias(enc_mask)
    for i in range(_n_layers(P, "model.decoder.layers.")):
        pre = f"model.decoder.layers.{i}"
        x = _ln(P, pre + ".self_attn_layer_norm", h, eps)
        h = h + _attn(P, pre + ".self_attn", x, x, self_bias, nh)
        x = _ln(P, pre + ".encoder_attn_layer_norm", h, eps)
        h = h + _attn(P, pre + ".encoder_attn", x, enc, cross_bias, nh)
        x = _ln(P, pre + ".final_layer_norm", h, eps)
        h = h + F.linear(torch.relu(F.linear(x, P[pre + ".fc1.weight"], P[pre + ".fc1.bias"])),
                         P[pre + ".fc2.weight"], P[pre + ".fc2.bias"])
    return _ln(P, "model.decoder.layer_norm", h, eps)


def pegasus_logits(P, ids, mask, dec_ids, dec_mask, nh, **kw):
    """PegasusHugface.forward: the logits [B, Ld, V] (lm_head without a bias; final_logits_bias is zero)"""
    enc = pegasus_encoder(P, ids, mask, nh, **kw)
    h = pegasus_decoder(P, dec_ids, dec_mask, enc, mask, nh, **kw)
    return F.linear(h, P["lm_head.weight"])


def title_loss_ref(logits, dec_mask, targets):
    """(mean cross-entropy over the decoder positions with mask 1, number correct, number valid) -- what
    train_chapter_title_gen.py:158-169 computes from the logits"""
    sel = dec_mask != 0
    z, t = logits[sel].double(), targets[sel]
    return F.cross_entropy(z, t), int((z.argmax(-1) == t).sum()), int(sel.sum())


def greedy_ref(P, ids, mask, nh, max_len, start=0, **kw):
    """The reference's greedy loop in this statement, for a batch: -> (tokens [B, max_len], top-2 logit margins
    [B, max_len], the last decoder position's hidden state of every step [B, max_len, H]); every sequence runs all
    max_len steps."""
    B = ids.shape[0]
    enc = pegasus_encoder(P, ids, mask, nh, **kw)
    dec = torch.full((B, 1), start, dtype=torch.int64)
    margins, hidden = [], []
    for _ in range(max_len):
        h = pegasus_decoder(P, dec, torch.ones_like(dec), enc, mask, nh, **kw)
        z = F.linear(h[:, -1], P["lm_head.weight"])
        top = z.topk(2, dim=-1).values
        margins.append(top[:, 0] - top[:, 1])
        hidden.append(h[:, -1])
        dec = torch.cat([dec, z.argmax(-1, keepdim=True)], 1)
    return dec[:, 1:], torch.stack(margins, 1), torch.stack(hidden, 1)


def cross_attention_ref(q, kv, mask, B, nh, Lq, Lk, scale=0.125):
    """fp64 cross-attention of q [B Lq (+), >= H] over kv [B Lk (+), >= 2 H] = K | V with the key mask [B, Lk] (None: all
    valid), head dim 64, HF's arithmetic: -> (ctx [B Lq, H], row max [B nh, Lq] of the scaled scores over the valid
    keys, row sum [B nh, Lq] of exp(score - max) over them). A sequence without a valid key: uniform over its Lk keys
    (what the finfo.min bias gives), reported as max = -inf, sum = Lk."""
    H = nh * 64
    qd = q[:B * Lq, :H].double().cpu().view(B, Lq, nh, 64).transpose(1, 2)
    kd = kv[:B * Lk, :H].double().cpu().view(B, Lk, nh, 64).transpose(1, 2)
    vd = kv[:B * Lk, H:2 * H].double().cpu().view(B, Lk, nh, 64).transpose(1, 2)
    s = qd @ kd.transpose(-1, -2) * scale  # [B, nh, Lq, Lk]
    valid = torch.ones(B, Lk, dtype=torch.bool) if mask is None else mask.cpu() != 0
    w = torch.softmax(s + _pad_bias(valid.to(torch.int64)), dim=-1)
    ctx = (w @ vd).transpose(1, 2).reshape(B * Lq, H)
    sv = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    mx = sv.max(-1).values
    sm = torch.exp(sv - mx[..., None]).sum(-1)
    nokey = ~valid.any(1)
    sm[nokey] = float(Lk)  # (mx is -inf there already; exp(-inf + inf) above was NaN)
    return ctx, mx.reshape(B * nh, Lq), sm.reshape(B * nh, Lq)
