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
causal. encode / cross_kv / decode are the inference path: no dropout site is applied and nothing is saved.

Training (train_forward / train_backward, driven by PegasusFn under PegasusHugface.title_loss): the same layer loop with
transformers' dropout sites and everything the backward reads saved per sublayer.
  * Dropout: the embedding of both stacks, after out_proj of every attention and after fc2 (config.dropout), the
    attention probabilities of self- and cross-attention (attention_dropout), after the ReLU (activation_dropout); all
    zero unless the model is in train() mode. The residual adds and the ReLU are then the streaming kernels
    vcg_dropout_add_* / vcg_relu_dropout_* instead of GEMM epilogues (also at p = 0: one code path). Seeds:
    bert._seed(seed, layer, site) with layer = 1 + i for encoder layer i, 1001 + i for decoder layer i (0 / 1000: the
    embeddings) and site 0 embedding, 1 self-attention P, 2 self-attention output, 3 cross-attention P, 4 cross-attention
    output, 5 activation, 6 FFN output. Index spaces: row * H + c (row * ffn + c for the activation) =
    dropout_util.row_keep; (z * Lq + q) * Lk + k = dropout_util.score_keep for the cross-attention; the self-attention's
    is bert_attn's (z * L + q) * Lp + k.
  * The residual stream and its gradient stay fp32 (bf16 mode too): each sublayer's input gradient goes through
    vcg_ln_bwd_acc, which adds LN'(dx) onto the fp32 stream gradient in one pass.
  * The encoder output's gradient is the sum over the decoder layers of dKV @ W_kv, accumulated in fp32 in backward
    layer order (vcg_dropout_add_fwd at p = 0 is the fp32 += of a compute-dtype branch); it enters the encoder's final
    LayerNorm backward.
  * Weight gradients: q | k | v and the cross-attention's k | v as ONE split-K GEMM and one column sum where the flat
    buffer holds the members back to back, else one per member. A parameter with requires_grad False gets none.
  * Input-gradient GEMMs dX = dY W read the stored weight [out][in] as the N-contiguous operand (transB): the engine
    keeps no transposed copy (bert._LinearT would be 1.1 GB of bf16 for pegasus-large, refreshed every step), and
    their outputs are in the compute dtype because vcg_ln_bwd_acc does the fp32 accumulation -- the fp32-output GEMM
    class that needs the resident W^T is not used.
  * fused_cross = False runs the cross-attention as a chain of stock torch ops (bmm, fp32 softmax with the finfo.min
    bias, the same keep mask, bmm) under autograd with P saved: the A/B arm and a second statement for the tests.
"""
import math

import torch

from . import ops
from .bert import BertEncoderEngine, _Lin, _seed, attention_bwd, attention_fwd

FMIN = torch.finfo(torch.float32).min


class PegasusEngine:
    wt = None  # (nn.Linear weights are stored K-contiguous: _lin_fwd needs no transposed copy)
    _lin_fwd = BertEncoderEngine._lin_fwd
    # q | k | v (self-attention) and k | v (cross-attention) as ONE GEMM where the flat buffer holds the members back
    # to back (every parameter a multiple of 256 elements: d_model % 256 == 0); False: a GEMM per member into the
    # column slices of the same buffer (tests compare both)
    fuse_proj = True
    # training: the fused cross-attention kernels (vcg_cross_attn_kv_fwd_ex / _bwd); False: the unfused chain on stock
    # torch ops with P saved (tests and tools/bench_pegasus_train.py compare both)
    fused_cross = True

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

    # ------------------------------------------------------------------ training
    def _rates(self):
        c = self.cfg
        return (c.dropout, c.attention_dropout, c.activation_dropout) if self.m.training else (0.0, 0.0, 0.0)

    def _grouped(self, mods):
        ws, bs = [d.weight for d in mods], [d.bias for d in mods]
        return PegasusEngine.fuse_proj and len(mods) > 1 and self._adjacent(ws) and self._adjacent(bs)

    def _ln_t(self, ln, h, rows):
        """-> (LN(h) in the compute dtype, (ln, h, mean, rstd) for _ln_bwd)"""
        x, mean, rstd = ops.ln_fwd(h, None, ln.weight, ln.bias, rows, self.H, self.eps)
        x = x if self.dtype == torch.float32 else ops.cast_from_f32(x, self.dtype)
        return x, (ln, h, mean, rstd)

    def _ln_bwd(self, saved, dx, dh, rows):
        """dh (fp32 stream gradient) += LN'(dx); the LayerNorm's own gradients unless it is frozen"""
        ln, h, mean, rstd = saved
        ops.ln_bwd_acc(dx, h, ln.weight, mean, rstd, dh, ln.weight.grad if ln.weight.requires_grad else None,
                       ln.bias.grad if ln.bias.requires_grad else None, rows, self.H)

    def _add(self, h, branch, p, seed):
        """a new stream h + dropout(branch) (h itself is saved by the LayerNorm before it)"""
        return ops.dropout_add_fwd(h.clone(), branch, p, seed)

    def _dx(self, dy, ldy, W, M, n_in, n_out):
        """dy [M, n_out] (row pitch ldy) @ W [n_out][n_in] -> [M, n_in], compute dtype"""
        return ops.gemm(dy, W, M, n_in, n_out, ldy, n_in, transB=True)

    def _proj_bwd(self, mods, dy, x, M, want_dx=True):
        """backward of _proj: dy [M, n H] (contiguous) and the input x [M, H] -> the members' weight / bias gradients
        (trainable members only) and dy W [M, H] (None unless want_dx)"""
        H, n = self.H, len(mods)
        if self._grouped(mods):
            ws, bs = [d.weight for d in mods], [d.bias for d in mods]
            if all(d.weight.requires_grad for d in mods):
                ops.gemm_splitk(dy, x, self.flat.contiguous_view(ws, (n * H, H), "grad"), n * H, H, M, n * H, H,
                                transA=True, transB=True)
            if all(d.bias.requires_grad for d in mods):
                ops.colsum(dy, n * H, M, n * H, self.flat.contiguous_view(bs, (n * H,), "grad"))
            mixed = [d for d in mods if d.weight.requires_grad != mods[0].weight.requires_grad
                     or d.bias.requires_grad != mods[0].bias.requires_grad]
            if mixed:
                raise NotImplementedError("native Pegasus: q | k | v (k | v) projections frozen in part")
            if not want_dx:
                return None
            return self._dx(dy, n * H, self.flat.compute_contiguous(ws, (n * H, H), self.dtype), M, H, n * H)
        dx = None
        for j, d in enumerate(mods):
            dyj = dy[:, j * H:]
            if d.weight.requires_grad:
                ops.gemm_splitk(dyj, x, d.weight.grad, H, H, M, n * H, H, transA=True, transB=True)
            if d.bias.requires_grad:
                ops.colsum(dyj, n * H, M, H, d.bias.grad)
            if want_dx:
                t = self._dx(dyj, n * H, self.flat.compute_view(d.weight, self.dtype), M, H, H)
                dx = t if dx is None else dx.add_(t)
        return dx

    def _lin_bwd(self, d, dy, x, M):
        """one Linear: its gradients (if trainable) and dy W"""
        if d.weight.requires_grad:
            ops.gemm_splitk(dy, x, d.weight.grad, d.out_features, d.in_features, M, d.out_features, d.in_features,
                            transA=True, transB=True)
        if d.bias.requires_grad:
            ops.colsum(dy, d.out_features, M, d.out_features, d.bias.grad)
        return self._dx(dy, d.out_features, self.flat.compute_view(d.weight, self.dtype), M, d.in_features,
                        d.out_features)

    # ---- sublayers: forward returns (new h, saved); backward takes the stream gradient dh (fp32, updated in place)
    def _self_attn_t(self, layer, h, mask, B, L, nh, causal, rates, seed, li):
        H, dt = self.H, self.dtype
        rows = B * L
        at = layer.self_attn
        x, lns = self._ln_t(layer.self_attn_layer_norm, h, rows)
        qkv_buf = torch.zeros((rows + 8, 3 * H), dtype=dt, device=h.device)  # +8 rows: padded key reads
        self._proj((at.q_proj, at.k_proj, at.v_proj), x, rows, qkv_buf)
        Lp = (L + 7) // 8 * 8
        fused = dt == torch.bfloat16 and L <= 512 and BertEncoderEngine.fused_attn
        sa, so = _seed(seed, li, 1), _seed(seed, li, 2)
        ctx, att = attention_fwd(qkv_buf, mask, B, nh, L, Lp, 64, 0.125, rates[1], sa, fused, causal=causal)
        o = self._lin_fwd(self._lin(at.out_proj), ctx, rows)
        return self._add(h, o, rates[0], so), dict(lns=lns, x=x, qkv_buf=qkv_buf, att=att, ctx=ctx, mask=mask, B=B, L=L,
                                                   Lp=Lp, nh=nh, causal=causal, sa=sa, so=so)

    def _self_attn_b(self, layer, s, dh, rates):
        at = layer.self_attn
        rows = s["B"] * s["L"]
        do = ops.dropout_add_bwd(dh, self.dtype, rates[0], s["so"])
        dctx = self._lin_bwd(at.out_proj, do, s["ctx"], rows)
        dqkv = attention_bwd(s["qkv_buf"], dctx, None, s["mask"], s["att"], s["B"], s["nh"], s["L"], s["Lp"], 64, 0.125,
                             rates[1], s["sa"], causal=s["causal"])
        dx = self._proj_bwd((at.q_proj, at.k_proj, at.v_proj), dqkv, s["x"], rows)
        self._ln_bwd(s["lns"], dx, dh, rows)

    def _ffn_t(self, layer, h, rows, rates, seed, li):
        x, lns = self._ln_t(layer.final_layer_norm, h, rows)
        sa, so = _seed(seed, li, 5), _seed(seed, li, 6)
        f = self._lin_fwd(self._lin(layer.fc1), x, rows)
        ops.relu_dropout_fwd(f, rates[2], sa, out=f)
        o = self._lin_fwd(self._lin(layer.fc2), f, rows)
        return self._add(h, o, rates[0], so), dict(lns=lns, x=x, f=f, sa=sa, so=so)

    def _ffn_b(self, layer, s, dh, rows, rates):
        do = ops.dropout_add_bwd(dh, self.dtype, rates[0], s["so"])
        df = self._lin_bwd(layer.fc2, do, s["f"], rows)
        ops.relu_dropout_bwd(df, s["f"], rates[2], out=df)
        dx = self._lin_bwd(layer.fc1, df, s["x"], rows)
        self._ln_bwd(s["lns"], dx, dh, rows)

    def _cross_chain(self, q, kvb, enc_mask, B, nh, L, Ls, p, seed):
        """the unfused arm: stock torch ops under autograd, P saved -> (ctx, (ctx with its graph, q leaf, kv leaf))"""
        H = self.H
        with torch.enable_grad():
            ql = q.detach().requires_grad_()
            kvl = kvb[:B * Ls].detach().requires_grad_()
            qh = ql.view(B, L, nh, 64).transpose(1, 2)
            kh = kvl[:, :H].reshape(B, Ls, nh, 64).transpose(1, 2)
            vh = kvl[:, H:].reshape(B, Ls, nh, 64).transpose(1, 2)
            sc = (qh @ kh.transpose(-1, -2)).float() * 0.125
            if enc_mask is not None:
                sc = sc + ((enc_mask == 0).float() * FMIN)[:, None, None, :]
            w = torch.softmax(sc, dim=-1)
            if p > 0:  # the fused kernel's keep mask: dropout'(1) in the score space (z Lq + q) Lk + k
                ones = torch.ones(B * nh * L * Ls, dtype=torch.float32, device=q.device)
                w = w * ops.dropout_add_bwd(ones, torch.float32, p, seed).view(B, nh, L, Ls)
            ctx = (w.to(q.dtype) @ vh).transpose(1, 2).reshape(B * L, H)
        return ctx.detach(), (ctx, ql, kvl)

    def _cross_t(self, layer, h, enc, kvb, enc_mask, B, L, Ls, nh, rates, seed, li):
        rows = B * L
        at = layer.encoder_attn
        x, lns = self._ln_t(layer.encoder_attn_layer_norm, h, rows)
        q = self._lin_fwd(self._lin(at.q_proj), x, rows)
        sa, so = _seed(seed, li, 3), _seed(seed, li, 4)
        if PegasusEngine.fused_cross:
            stats = torch.empty((B * nh, L, 2), dtype=torch.float32, device=h.device)
            ctx = ops.cross_attn_kv_fwd(q, kvb, enc_mask, B, nh, L, Ls, 0.125, stats=stats, dropout_p=rates[1], seed=sa)
            att = stats
        else:
            ctx, att = self._cross_chain(q, kvb, enc_mask, B, nh, L, Ls, rates[1], sa)
        o = self._lin_fwd(self._lin(at.out_proj), ctx, rows)
        return self._add(h, o, rates[0], so), dict(lns=lns, x=x, q=q, kvb=kvb, att=att, ctx=ctx, sa=sa, so=so)

    def _cross_b(self, layer, s, dh, d_enc, enc, enc_mask, B, L, Ls, nh, rates):
        rows = B * L
        at = layer.encoder_attn
        do = ops.dropout_add_bwd(dh, self.dtype, rates[0], s["so"])
        dctx = self._lin_bwd(at.out_proj, do, s["ctx"], rows)
        if isinstance(s["att"], tuple):
            ctx, ql, kvl = s["att"]
            dq, dkv = torch.autograd.grad(ctx, (ql, kvl), dctx)
            dq, dkv = dq.contiguous(), dkv.contiguous()
        else:
            dq, dkv = ops.cross_attn_kv_bwd(s["q"], s["kvb"], enc_mask, dctx, s["att"], B, nh, L, Ls, 0.125, rates[1],
                                            s["sa"])
        dx = self._lin_bwd(at.q_proj, dq, s["x"], rows)
        self._ln_bwd(s["lns"], dx, dh, rows)
        # K | V of the encoder output: the weights' gradients, and the encoder output's, summed in fp32
        want = d_enc is not None
        de = self._proj_bwd((at.k_proj, at.v_proj), dkv, enc, B * Ls, want_dx=want)
        if want:
            ops.dropout_add_fwd(d_enc, de, 0.0, 0)

    def _trainable(self, mod):
        return any(p.requires_grad for p in mod.parameters())

    def train_forward(self, ids, mask, dec_ids, dec_mask, seed, need_grad=True):
        """ids, mask [B, Ls]; dec_ids, dec_mask [B, Ld] -> (the decoder's last hidden state [B Ld, H] in the compute
        dtype, what train_backward reads -- None unless need_grad)"""
        B, Ls = ids.shape
        Ld = dec_ids.shape[1]
        self.m.check_text_len(Ls, "source")
        self.m.check_text_len(Ld, "decoder")
        enc_m, dec_m = self.m.model.encoder, self.m.model.decoder
        nhe, nhd = self.cfg.encoder_attention_heads, self.cfg.decoder_attention_heads
        rates = self._rates()
        ids, dec_ids = ids.contiguous(), dec_ids.contiguous()
        mask, dec_mask = self._mask(mask, ids), self._mask(dec_mask, dec_ids)
        tok = self.m.model.shared.weight.data
        se, sd = _seed(seed, 0, 0), _seed(seed, 1000, 0)
        h = ops.pegasus_embed_fwd(ids, tok, enc_m.embed_positions.weight.data, B, Ls, self.H, torch.float32,
                                  self.embed_scale, 0, p=rates[0], seed=se)
        enc_saved = []
        for i, layer in enumerate(enc_m.layers):
            h, s1 = self._self_attn_t(layer, h, mask, B, Ls, nhe, False, rates, seed, 1 + i)
            h, s2 = self._ffn_t(layer, h, B * Ls, rates, seed, 1 + i)
            enc_saved.append((s1, s2))
        enc, enc_ln = self._ln_t(enc_m.layer_norm, h, B * Ls)
        h = ops.pegasus_embed_fwd(dec_ids, tok, dec_m.embed_positions.weight.data, B, Ld, self.H, torch.float32,
                                  self.embed_scale, 0, p=rates[0], seed=sd)
        dec_saved = []
        for i, layer in enumerate(dec_m.layers):
            h, s1 = self._self_attn_t(layer, h, dec_mask, B, Ld, nhd, True, rates, seed, 1001 + i)
            at = layer.encoder_attn
            kvb = torch.zeros((B * Ls + 8, 2 * self.H), dtype=self.dtype, device=h.device)
            self._proj((at.k_proj, at.v_proj), enc, B * Ls, kvb)
            h, s2 = self._cross_t(layer, h, enc, kvb, mask, B, Ld, Ls, nhd, rates, seed, 1001 + i)
            h, s3 = self._ffn_t(layer, h, B * Ld, rates, seed, 1001 + i)
            dec_saved.append((s1, s2, s3))
        hidden, dec_ln = self._ln_t(dec_m.layer_norm, h, B * Ld)
        if not need_grad:
            return hidden, None
        return hidden, dict(ids=ids, dec_ids=dec_ids, mask=mask, B=B, Ls=Ls, Ld=Ld, rates=rates, se=se, sd=sd, enc=enc,
                            enc_ln=enc_ln, dec_ln=dec_ln, enc_saved=enc_saved, dec_saved=dec_saved)

    def train_backward(self, d_hidden, sv):
        """d_hidden [B Ld, H]: the gradient of train_forward's output. Adds every trainable parameter's gradient onto
        its .grad (the flat buffer's views)."""
        B, Ls, Ld, rates = sv["B"], sv["Ls"], sv["Ld"], sv["rates"]
        enc_m, dec_m = self.m.model.encoder, self.m.model.decoder
        nhd = self.cfg.decoder_attention_heads
        dev = d_hidden.device
        shared = self.m.model.shared.weight
        enc_train = self._trainable(enc_m)  # (shared included: the encoder's embedding)
        dh = torch.zeros((B * Ld, self.H), dtype=torch.float32, device=dev)
        self._ln_bwd(sv["dec_ln"], d_hidden.contiguous(), dh, B * Ld)
        d_enc = torch.zeros((B * Ls, self.H), dtype=torch.float32, device=dev) if enc_train else None
        for i in reversed(range(len(dec_m.layers))):
            layer = dec_m.layers[i]
            s1, s2, s3 = sv["dec_saved"].pop()
            self._ffn_b(layer, s3, dh, B * Ld, rates)
            self._cross_b(layer, s2, dh, d_enc, sv["enc"], sv["mask"], B, Ld, Ls, nhd, rates)
            self._self_attn_b(layer, s1, dh, rates)
        pad = self.m.model.shared.padding_idx
        pad = -1 if pad is None else pad
        if shared.requires_grad:
            ops.pegasus_embed_bwd(dh, sv["dec_ids"], shared.grad, B, Ld, self.H, self.embed_scale, pad, rates[0],
                                  sv["sd"])
        if not enc_train:
            return
        dh = torch.zeros((B * Ls, self.H), dtype=torch.float32, device=dev)
        self._ln_bwd(sv["enc_ln"], d_enc, dh, B * Ls)
        for i in reversed(range(len(enc_m.layers))):
            layer = enc_m.layers[i]
            s1, s2 = sv["enc_saved"].pop()
            self._ffn_b(layer, s2, dh, B * Ls, rates)
            self._self_attn_b(layer, s1, dh, rates)
        if shared.requires_grad:
            ops.pegasus_embed_bwd(dh, sv["ids"], shared.grad, B, Ls, self.H, self.embed_scale, pad, rates[0], sv["se"])


class PegasusFn(torch.autograd.Function):
    """The whole encoder-decoder as one autograd node: forward = PegasusEngine.train_forward, backward =
    train_backward, which writes the parameters' gradients itself (they are not Function inputs, as in
    vcg_hip/functions.py); `anchor` is what connects the node to the graph."""

    @staticmethod
    def forward(ctx, anchor, engine, ids, mask, dec_ids, dec_mask, seed):
        ctx.set_materialize_grads(False)
        hidden, saved = engine.train_forward(ids, mask, dec_ids, dec_mask, seed, need_grad=True)
        ctx.engine, ctx.saved = engine, saved
        return hidden

    @staticmethod
    def backward(ctx, d_hidden):
        if d_hidden is not None:
            if ctx.saved is None:
                raise RuntimeError("PegasusFn: a second backward would need the activations the first one released")
            ctx.engine.train_backward(d_hidden, ctx.saved)
            ctx.saved = None
        return (None,) * 7
