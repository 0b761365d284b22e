"""Pegasus encoder-decoder on libvcg_hip (transformers PegasusForConditionalGeneration semantics), inference.

Reference use: PegasusHugface.forward -> base_model(input_ids, attention_mask, decoder_input_ids,
decoder_attention_mask).logits (model/lang/pegasus_hugface.py:89-102) with base_model =
PegasusForConditionalGeneration('google/pegasus-large') (:23). What differs from the BERT / GPT layer loop
(vcg_hip/bert.py) is why this is an engine of its own:

  * the blocks are pre-LayerNorm: h += Attn(LN(h)); h += FFN(LN(h)), one final LayerNorm per stack. The LayerNorm is
    vcg_ln_fwd without a residual, the residual add is the GEMM's residual epilogue on out_proj and fc2. The residual
    stream h stays fp32 in the bf16 mode too, as torch.autocast keeps it (its LayerNorms read and write fp32): the
    embedding is written in fp32, the LayerNorm output is cast to bf16 for the GEMMs, and out_proj / fc2 add their
    bf16 product onto the fp32 stream (the wide engine's fp32-residual class, VCG_ACT_FLAG_F32_OUT). A bf16 stream
    rounds |h| ~ 1 at every add, which is several times the error of the branches themselves;
  * the activation is ReLU (the GEMM's VCG_ACT_RELU epilogue: the 128 x 128 engine -- the wide-tile engine has no ReLU
    class and hands the call over);
  * the embedding is sqrt(d_model) * shared[id] + sinusoidal[t] (vcg_pegasus_embed_fwd), no LayerNorm behind it;
  * the decoder has a cross-attention over the encoder output with Lq != Lk and separate Q and K | V buffers
    (vcg_cross_attn_kv_fwd, csrc/pegasus.hip); K | V of the encoder output are projected once per source (cross_kv) and
    serve every decoder pass over it.

Shared with BertEncoderEngine: the Linear routing (_lin_fwd) and attention_fwd -- the fused self-attention kernels for
bf16 and L <= 512, the unfused chain above that and in the fp32 parity mode; the encoder's is non-causal, the decoder's
causal. Eval mode only: no dropout site is applied and nothing is saved for a backward.
"""
import math

import torch

from . import ops
from .bert import BertEncoderEngine, _Lin, attention_fwd


class PegasusEngine:
    wt = None  # (nn.Linear weights are stored K-contiguous: _lin_fwd needs no transposed copy)
    _lin_fwd = BertEncoderEngine._lin_fwd
    # q | k | v (self-attention) and k | v (cross-attention) as ONE GEMM where the flat buffer holds the members back
    # to back (every parameter a multiple of 256 elements: d_model % 256 == 0); False: a GEMM per member into the
    # column slices of the same buffer (tests compare both)
    fuse_proj = True

    def __init__(self, model, flat, dtype):
        self.m, self.flat, self.dtype = model, flat, dtype
        c = model.config
        self.cfg = c
        self.H = c.d_model
        self.eps = c.layer_norm_eps
        self.embed_scale = math.sqrt(c.d_model) if c.scale_embedding else 1.0

    # ------------------------------------------------------------------ Linear layers
    def _lin(self, d):
        return _Lin(self.flat.compute_view(d.weight, self.dtype), d.bias, None, None, d.in_features, d.out_features,
                    train=False)

    def _adjacent(self, plist):
        o = self.flat.offset_of(plist[0])
        for p in plist:
            if self.flat.offset_of(p) != o:
                return False
            o += p.numel()
        return True

    def _proj(self, mods, x, M, out):
        """out[:, j H:(j + 1) H] = mods[j](x) for the Linear modules `mods` (all H -> H); out: [M (+ pad), len(mods) H]"""
        H, n = self.H, len(mods)
        ws, bs = [d.weight for d in mods], [d.bias for d in mods]
        if PegasusEngine.fuse_proj and self._adjacent(ws) and self._adjacent(bs):
            lin = _Lin(self.flat.compute_contiguous(ws, (n * H, H), self.dtype),
                       self.flat.contiguous_view(bs, (n * H,), "data"), None, None, H, n * H, train=False)
            self._lin_fwd(lin, x, M, out=out, ldc=n * H)
        else:
            for j, d in enumerate(mods):
                self._lin_fwd(self._lin(d), x, M, out=out[:, j * H:], ldc=n * H)
        return out

    def _ln(self, ln, h, rows):
        """LayerNorm of the fp32 residual stream, in the compute dtype (the operand of the GEMMs behind it)"""
        x = ops.ln_fwd(h, None, ln.weight, ln.bias, rows, self.H, self.eps)[0]
        return x if self.dtype == torch.float32 else ops.cast_from_f32(x, self.dtype)

    def _res_lin(self, d, x, rows, h):
        """h + d(x): the Linear's residual epilogue, fp32 in and out (bf16: the wide engine's fp32-output class)"""
        lin = self._lin(d)
        if self.dtype == torch.float32:
            return self._lin_fwd(lin, x, rows, residual=h, ldr=self.H)
        out = torch.empty((rows, lin.n_out), dtype=torch.float32, device=x.device)
        return ops.gemm(x, lin.W, rows, lin.n_out, lin.n_in, lin.n_in, lin.n_in, out=out, ldc=lin.n_out, bias=lin.b,
                        act=ops.ACT_FLAG_WIDE | ops.ACT_FLAG_F32_OUT, residual=h, ldr=self.H)

    def _ffn(self, layer, h, rows):
        x = self._ln(layer.final_layer_norm, h, rows)
        f = self._lin_fwd(self._lin(layer.fc1), x, rows, act=ops.ACT_RELU)
        return self._res_lin(layer.fc2, f, rows, h)

    def _self_attn(self, layer, h, mask, B, L, nh, causal):
        H, dt = self.H, self.dtype
        rows = B * L
        at = layer.self_attn
        x = self._ln(layer.self_attn_layer_norm, h, rows)
        qkv_buf = torch.empty((rows + 8, 3 * H), dtype=dt, device=h.device)  # +8 rows: padded key reads
        self._proj((at.q_proj, at.k_proj, at.v_proj), x, rows, qkv_buf)
        Lp = (L + 7) // 8 * 8
        fused = dt == torch.bfloat16 and L <= 512 and BertEncoderEngine.fused_attn
        ctx, _ = attention_fwd(qkv_buf, mask, B, nh, L, Lp, 64, 0.125, 0.0, 0, fused, causal=causal)
        return self._res_lin(at.out_proj, ctx, rows, h)

    def _embed(self, stack, ids, B, L, pos0=0):
        return ops.pegasus_embed_fwd(ids.contiguous(), self.m.model.shared.weight.data,
                                     stack.embed_positions.weight.data, B, L, self.H, torch.float32, self.embed_scale,
                                     pos0)

    @staticmethod
    def _mask(mask, ids):
        return (torch.ones_like(ids) if mask is None else mask).to(torch.int64).contiguous()

    # ------------------------------------------------------------------ the three passes
    @torch.no_grad()
    def encode(self, ids, mask=None):
        """ids, mask [B, Ls] -> the encoder's last hidden state [B Ls, H] (after its final LayerNorm)"""
        B, L = ids.shape
        self.m.check_text_len(L, "source")
        enc = self.m.model.encoder
        mask = self._mask(mask, ids)
        h = self._embed(enc, ids, B, L)
        for layer in enc.layers:
            h = self._self_attn(layer, h, mask, B, L, self.cfg.encoder_attention_heads, causal=False)
            h = self._ffn(layer, h, B * L)
        return self._ln(enc.layer_norm, h, B * L)

    @torch.no_grad()
    def cross_kv(self, enc):
        """The decoder layers' K | V projections of the encoder state: a list of [B Ls + 8, 2 H] buffers (the pad rows
        are never read by vcg_cross_attn_kv_fwd; they keep the layout of the self-attention's buffers)"""
        rows = enc.shape[0]
        out = []
        for layer in self.m.model.decoder.layers:
            buf = torch.empty((rows + 8, 2 * self.H), dtype=self.dtype, device=enc.device)
            at = layer.encoder_attn
            out.append(self._proj((at.k_proj, at.v_proj), enc, rows, buf))
        return out

    @torch.no_grad()
    def decode(self, dec_ids, dec_mask, enc_mask, kv):
        """dec_ids, dec_mask [B, Ld]; enc_mask [B, Ls] (None: every source position valid); kv: cross_kv's buffers ->
        the decoder's last hidden state [B Ld, H]"""
        B, L = dec_ids.shape
        self.m.check_text_len(L, "decoder")
        dec = self.m.model.decoder
        nh, H = self.cfg.decoder_attention_heads, self.H
        rows = B * L
        Ls = (kv[0].shape[0] - 8) // B
        dec_mask = self._mask(dec_mask, dec_ids)
        if enc_mask is not None:
            enc_mask = enc_mask.to(torch.int64).contiguous()
            if tuple(enc_mask.shape) != (B, Ls):
                raise ValueError(f"decode: enc_mask {tuple(enc_mask.shape)} does not match the encoder state {(B, Ls)}")
        h = self._embed(dec, dec_ids, B, L)
        for layer, kvb in zip(dec.layers, kv):
            h = self._self_attn(layer, h, dec_mask, B, L, nh, causal=True)
            x = self._ln(layer.encoder_attn_layer_norm, h, rows)
            q = self._lin_fwd(self._lin(layer.encoder_attn.q_proj), x, rows)
            ctx = ops.cross_attn_kv_fwd(q, kvb, enc_mask, B, nh, L, Ls, 0.125)
            h = self._res_lin(layer.encoder_attn.out_proj, ctx, rows, h)
            h = self._ffn(layer, h, rows)
        return self._ln(dec.layer_norm, h, rows)
