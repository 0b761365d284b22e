"""The statement of tests/pegasus_ref.py extended to training (test helper): transformers'
PegasusForConditionalGeneration in train() mode as the reference's train_chapter_title_gen.py drives it, written so
that every random decision is an explicit argument.

What changes against the eval statement, and only that, is written here (everything else is imported from pegasus_ref):
  * the embedding is F.embedding(ids, shared, padding_idx=pad): row `pad` of the table receives no gradient;
  * the dropout sites of transformers' Pegasus layers, each as `x * keep / (1 - p)` with an explicit keep mask:
      rate `dropout`             the embedding of both stacks; after out_proj of every attention; after fc2
      rate `attention_dropout`   the attention probabilities of self- and cross-attention
      rate `activation_dropout`  after the activation
    `Sites` hands out the masks by site name and records (rate, shape) of every site it is asked for;
  * the loss is the mean cross-entropy over the decoder positions with mask 1 (pegasus_ref.title_loss_ref).

Site names (`Sites.keep(name, shape)`): ("enc" | "dec", "embed"), ("enc", i, "self_p" | "self_out" | "act" | "ffn_out"),
("dec", i, "self_p" | "self_out" | "cross_p" | "cross_out" | "act" | "ffn_out"). Shapes: [B, L, H] for the stream
sites, [B, nh, Lq, Lk] for the probabilities, [B, L, ffn] for the activation.
"""
import math

import torch
import torch.nn.functional as F

import pegasus_ref as ref
from pegasus_ref import FMIN, _ln, _n_layers, _pad_bias


class Sites:
    """rates = (dropout, attention_dropout, activation_dropout); keeps: None (no dropout: every site passes through),
    or a callable (name, shape, p) -> bool tensor of `shape` (True: kept)."""
    KIND = {"embed": 0, "self_out": 0, "cross_out": 0, "ffn_out": 0, "self_p": 1, "cross_p": 1, "act": 2}

    def __init__(self, rates=(0.0, 0.0, 0.0), keeps=None):
        self.rates, self.keeps, self.seen = rates, keeps, []

    def __call__(self, name, x):
        p = self.rates[self.KIND[name[-1]]]
        self.seen.append((p, tuple(x.shape)))
        if self.keeps is None or p <= 0:
            return x
        keep = self.keeps(name, tuple(x.shape), p)
        return x * keep.to(x.dtype) / (1.0 - p)


def _attn(P, pre, xq, xkv, bias, nh, drop, name):
    """pegasus_ref._attn with the dropout on the probabilities (site name) -- HF PegasusAttention, eager"""
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
    w = drop(name, torch.softmax(w, dim=-1))
    o = (w.to(v.dtype) @ v).transpose(1, 2).reshape(B, Lq, H)
    return lin("out_proj", o)


def _embed(P, stack, ids, scale, pad):
    L = ids.shape[1]
    return (F.embedding(ids, P["model.shared.weight"], padding_idx=pad) * scale
            + P[f"model.{stack}.embed_positions.weight"][torch.arange(L)][None])


def _ffn(P, pre, x, drop, stack, i):
    f = drop((stack, i, "act"), torch.relu(F.linear(x, P[pre + ".fc1.weight"], P[pre + ".fc1.bias"])))
    return drop((stack, i, "ffn_out"), F.linear(f, P[pre + ".fc2.weight"], P[pre + ".fc2.bias"]))


def encoder(P, ids, mask, nh, drop, pad=0, eps=1e-5, scale_embedding=True):
    H = P["model.shared.weight"].shape[1]
    h = drop(("enc", "embed"), _embed(P, "encoder", ids, math.sqrt(H) if scale_embedding else 1.0, pad))
    bias = _pad_bias(mask)
    for i in range(_n_layers(P, "model.encoder.layers.")):
        pre = f"model.encoder.layers.{i}"
        x = _ln(P, pre + ".self_attn_layer_norm", h, eps)
        h = h + drop(("enc", i, "self_out"), _attn(P, pre + ".self_attn", x, x, bias, nh, drop, ("enc", i, "self_p")))
        h = h + _ffn(P, pre, _ln(P, pre + ".final_layer_norm", h, eps), drop, "enc", i)
    return _ln(P, "model.encoder.layer_norm", h, eps)


def decoder(P, dec_ids, dec_mask, enc, enc_mask, nh, drop, pad=0, eps=1e-5, scale_embedding=True):
    B, Ld = dec_ids.shape
    H = P["model.shared.weight"].shape[1]
    h = drop(("dec", "embed"), _embed(P, "decoder", dec_ids, math.sqrt(H) if scale_embedding else 1.0, pad))
    future = torch.triu(torch.ones(Ld, Ld, dtype=torch.bool), 1)[None, None]
    self_bias = (future | (dec_mask == 0)[:, None, None, :]).to(torch.float64) * FMIN
    cross_bias = _pad_bias(enc_mask)
    for i in range(_n_layers(P, "model.decoder.layers.")):
        pre = f"model.decoder.layers.{i}"
        x = _ln(P, pre + ".self_attn_layer_norm", h, eps)
        h = h + drop(("dec", i, "self_out"), _attn(P, pre + ".self_attn", x, x, self_bias, nh, drop, ("dec", i, "self_p")))
        x = _ln(P, pre + ".encoder_attn_layer_norm", h, eps)
        h = h + drop(("dec", i, "cross_out"),
                     _attn(P, pre + ".encoder_attn", x, enc, cross_bias, nh, drop, ("dec", i, "cross_p")))
        h = h + _ffn(P, pre, _ln(P, pre + ".final_layer_norm", h, eps), drop, "dec", i)
    return _ln(P, "model.decoder.layer_norm", h, eps)


def title_loss(P, ids, mask, dec_ids, dec_mask, targets, nh, drop=None, pad=0, **kw):
    """-> (loss, logits): the masked mean cross-entropy of the training forward, differentiable in P's tensors"""
    drop = drop or Sites()
    enc = encoder(P, ids, mask, nh, drop, pad, **kw)
    h = decoder(P, dec_ids, dec_mask, enc, mask, nh, drop, pad, **kw)
    logits = F.linear(h, P["lm_head.weight"])
    sel = dec_mask != 0
    return F.cross_entropy(logits[sel].to(torch.float64 if logits.dtype == torch.float64 else torch.float32),
                           targets[sel]), logits


def cross_attention_train(q, kv, mask, B, nh, Lq, Lk, keep=None, p=0.0, scale=0.125):
    """pegasus_ref.cross_attention_ref's ctx [B Lq, H] in fp64 with the probabilities dropped by keep [B nh, Lq, Lk]
    (None: no dropout), differentiable in q [B Lq, H] and kv [B Lk, 2 H]"""
    H = nh * 64
    qd = q[:B * Lq, :H].double().view(B, Lq, nh, 64).transpose(1, 2)
    kd = kv[:B * Lk, :H].double().view(B, Lk, nh, 64).transpose(1, 2)
    vd = kv[:B * Lk, H:2 * H].double().view(B, Lk, nh, 64).transpose(1, 2)
    valid = torch.ones(B, Lk, dtype=torch.int64) if mask is None else (mask != 0).to(torch.int64)
    w = torch.softmax(qd @ kd.transpose(-1, -2) * scale + _pad_bias(valid), dim=-1)
    if keep is not None:
        w = w * torch.as_tensor(keep).view(B, nh, Lq, Lk).to(w.dtype) / (1.0 - p)
    return (w @ vd).transpose(1, 2).reshape(B * Lq, H)


__all__ = ["Sites", "encoder", "decoder", "title_loss", "cross_attention_train", "ref"]
