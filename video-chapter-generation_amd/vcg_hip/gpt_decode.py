"""KV-cached text generation for GPTHugface on csrc/gpt_decode.hip.

The reference writes text with common_utils/language_model_utils.py:token_idx_sample, which re-runs the whole decoder
on the whole prefix for every token. Here the prompt runs once through the training engine's forward
(GptEncoderEngine, whose per-layer fused QKV output fills the K / V caches), and every further token is ONE call of
vcg_gpt_decode_step: embedding of the newest token, per layer QKV -> decode attention over the cache (which appends the
new K / V) -> projection -> LayerNorm -> FFN -> LayerNorm, the vocabulary head, and the sampler, which writes the
chosen token into the device token matrix the next step reads. Neither Python nor the host reads anything back between
tokens.

Indexing: with prompt lengths len0[b], generated token g = 0 .. steps-1 of sequence b lands in column len0[b] + g of
`seq`. g = 0 is drawn from the prompt's own forward (prefill); step(t) embeds column len0 + t and draws g = t + 1.
Row g of the uniforms `u`, column g of `forced` / `chosen`.

`plan_generation` and `check_prefix_mask` are pure host functions (tests/test_cpu_gpt_generate.py).
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops

MAX_LAYERS = 48  # VCG_GPT_MAX_LAYERS (include/vcg_gpt_decode.h)

_vp = ctypes.c_void_p


class _Layer(ctypes.Structure):
    _fields_ = [("w", _vp * 4), ("b", _vp * 4), ("ln_g", _vp * 2), ("ln_b", _vp * 2), ("kcache", _vp), ("vcache", _vp)]


class _Desc(ctypes.Structure):
    """include/vcg_gpt_decode.h: vcg_gpt_decode_desc, field for field."""
    _fields_ = ([(n, ctypes.c_int) for n in ("dtype", "B", "H", "nh", "n_layer", "n_inner", "V", "Tcap", "n_pos",
                                             "max_len0", "steps", "w_stored_in_out", "top_k", "greedy",
                                             "use_skinny")]
                + [("temperature", ctypes.c_float), ("ln_eps", ctypes.c_float), ("ldz", ctypes.c_longlong)]
                + [(n, _vp) for n in ("tok", "pos", "head_w", "seq", "len0", "u", "forced", "chosen", "prob", "h", "qkv",
                                      "ctx", "ao", "h1", "ff", "fo", "h2", "logits", "ln_stat")]
                + [("layers", _Layer * MAX_LAYERS)])


def plan_generation(len0, steps, block_size):
    """(cached, sliding): how many of the `steps` generated tokens are drawn on the KV cache, and how many afterwards
    on the sliding window. Token g is drawn from a context of max(len0) + g tokens; while that is within block_size
    the cache serves it. Beyond, the reference crops to the last block_size tokens (x[:, -block_size:]), which shifts
    every learned position, so the cached K / V no longer apply and those tokens re-run the forward on the window."""
    lens = np.asarray(len0, dtype=np.int64).reshape(-1)
    if lens.size == 0 or lens.min() < 1:
        raise ValueError("plan_generation: every sequence needs at least one prompt token")
    if steps < 0 or block_size < 1:
        raise ValueError("plan_generation: steps >= 0 and block_size >= 1")
    cached = int(min(steps, max(0, block_size - int(lens.max()) + 1)))
    return cached, int(steps) - cached


def check_prefix_mask(mask):
    """len0 (int64 numpy [B]) of a right-padded attention mask [B, L]: each row is ones followed by zeros, with at least
    one token. Left padding, holes and empty rows are a ValueError (the cache holds a valid prefix per sequence; there
    is no mask argument on the decode path)."""
    m = np.asarray(mask) != 0
    if m.ndim != 2 or m.shape[0] == 0:
        raise ValueError("attention_mask must be [B, L] with B >= 1")
    lens = m.sum(1)
    if (lens < 1).any():
        raise ValueError(f"attention_mask: sequence {int(np.flatnonzero(lens < 1)[0])} has no token")
    prefix = np.arange(m.shape[1])[None, :] < lens[:, None]
    if (m != prefix).any():
        b = int(np.flatnonzero((m != prefix).any(1))[0])
        raise ValueError(f"attention_mask: sequence {b} is not a right-padded prefix of ones (left padding and holes "
                         "are not supported by the KV-cached path)")
    return lens.astype(np.int64)


def sample(logits, V, temperature=1.0, top_k=0, greedy=False, u=None, seq=None, len0=None, max_len0=0, col_off=0,
           forced=None, forced_ld=0, chosen=None, chosen_ld=1, prob=None):
    """vcg_sample_topk on fp32 logits [B, ldz] (V valid columns). Returns `chosen` (int64 [B], allocated if None)."""
    ops._chk(logits, torch.float32, "logits")
    B, ldz = logits.shape
    if chosen is None:
        chosen = torch.empty(B, dtype=torch.int64, device=logits.device)
    if u is not None:
        ops._chk(u, torch.float32, "u")
    Tcap = 0
    if seq is not None:
        ops._chk(seq, torch.int64, "seq")
        Tcap = seq.shape[1]
    _lib.call("vcg_sample_topk", ops.P(logits), ldz, B, V, float(temperature), int(top_k or 0), int(bool(greedy)),
              ops.P(u), ops.P(seq), Tcap, ops.P(len0), int(max_len0), int(col_off), ops.P(forced), int(forced_ld),
              ops.P(chosen), int(chosen_ld), ops.P(prob), ops.stream())
    return chosen


def attn_decode(qkv_new, kcache, vcache, len0, max_len0, t, nh, scale=None, dh=None):
    """vcg_attn_decode: ctx [B, H] from this step's qkv_new [B, 3H]; kcache / vcache [B, nh, Tcap, dh] gain row
    len0 + t."""
    B, nh_c, Tcap, dh_c = kcache.shape
    dh = dh_c if dh is None else dh
    ctx = torch.empty((B, nh * dh), dtype=qkv_new.dtype, device=qkv_new.device)
    _lib.call("vcg_attn_decode", ops.dt_code(qkv_new.dtype), ops.P(qkv_new), ops.P(kcache), ops.P(vcache), ops.P(len0),
              int(max_len0), int(t), ops.P(ctx), B, nh, dh, Tcap, float(scale if scale is not None else dh ** -0.5),
              ops.stream())
    return ctx


def gpt_embed_at(seq, len0, max_len0, t, tok, pos, dtype):
    """out [B, H] = tok[seq[b, len0[b] + t]] + pos[len0[b] + t]."""
    B, Tcap = seq.shape
    V, H = tok.shape
    out = torch.empty((B, H), dtype=dtype, device=seq.device)
    _lib.call("vcg_gpt_embed_at", ops.dt_code(dtype), ops.P(seq), Tcap, ops.P(len0), int(max_len0), int(t), ops.P(tok),
              ops.P(pos), ops.P(out), B, H, V, pos.shape[0], ops.stream())
    return out


def gemm_skinny(x, W, bias=None, act=ops.ACT_NONE, f32_out=False, out=None):
    """vcg_gemm_skinny: act(x [M <= 16, K] W [N, K]^T + bias) -> bf16 [M, N], or fp32 with f32_out."""
    ops._chk(x, torch.bfloat16, "x")
    ops._chk(W, torch.bfloat16, "W")
    M, K = x.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32 if f32_out else torch.bfloat16, device=x.device)
    _lib.call("vcg_gemm_skinny", ops.P(x), ops.P(W), ops.P(bias), ops.P(out), M, N, K, out.stride(0), int(act),
              int(bool(f32_out)), ops.stream())
    return out


def head_logits(hsel, head_w):
    """fp32 logits [rows, ldz] of hidden rows in the compute dtype; head_w: bf16 [V, H], or fp32 [ldz, H] with zero pad
    rows (vcg_hip.mlm._head_weights)."""
    hsel = hsel.contiguous()
    if hsel.dtype == torch.bfloat16:
        return ops.mlm_logits(hsel, head_w)
    M, H = hsel.shape
    return ops.gemm(hsel, head_w, M, head_w.shape[0], H, H, H)


class GptDecoder:
    """KV-cached decoding of a GPTHugface (vocabulary head) in the model's precision. max_len: the longest context
    (prompt + generated tokens that are fed back) the caches hold, capped by the position table."""

    # bf16 with B <= 16: the chain's Linear layers and the head run on vcg_gemm_skinny (weights streamed straight to
    # the MFMA's registers); False: the existing GEMM engines at every B (tests and tools/bench_gpt_generate.py
    # compare both). fp32 parity mode and B > 16 always use the existing engines.
    skinny_gemm = True

    def __init__(self, model, max_len):
        gpt = model.base_model
        cfg = gpt.config
        if not model._is_vocab_head():
            raise RuntimeError("GptDecoder needs the vocabulary head (build_chapter_head replaced it)")
        if cfg.n_embd != cfg.n_head * 64:
            raise NotImplementedError("GptDecoder: the decode attention kernel needs head dim 64")
        if cfg.n_layer > MAX_LAYERS:
            raise NotImplementedError(f"GptDecoder: at most {MAX_LAYERS} layers")
        if _lib.query("vcg_gpt_decode_desc_bytes") != ctypes.sizeof(_Desc):
            raise _lib.VcgError("vcg_gpt_decode_desc: the Python mirror does not match the library's struct")
        self.model, self.gpt, self.cfg = model, gpt, cfg
        self.cap = int(min(max_len, cfg.n_positions))
        if self.cap < 1:
            raise ValueError("GptDecoder: max_len must be at least 1")
        self.Tcap = self.cap + 1  # (seq holds the last generated token as well)
        self.dtype = model.compute_dtype()
        self.V, self.H, self.nh, self.nl = model.vocab_size, cfg.n_embd, cfg.n_head, cfg.n_layer
        self.ldz = ops.mlm_vp(self.V)
        self.B = 0
        self._wkey = None
        self.desc = None

    # ------------------------------------------------------------------ weights
    def _bind_weights(self):
        """The engine (with the Conv1D weights' transposed copies of this weight generation) and the head operand;
        True when the weight pointers / copies were rebuilt."""
        model, dt = self.model, self.dtype
        flat = model.native_flat()
        from .gpt import GptEncoderEngine
        eng = GptEncoderEngine(self.gpt, flat, dt)
        if eng.wt is not None:
            eng.wt.refresh()  # (the chain reads the transposed copies: this weight generation's)
        key = (id(flat), flat.generation, flat._version(), dt)
        fresh = key != self._wkey
        if fresh:
            from .mlm import _head_weights
            W, Wp = _head_weights(model, model.head, dt)
            self.head_w = W if Wp is None else Wp
            self._wkey = key
        self.eng, self.flat = eng, flat
        return fresh

    def _alloc(self, B, dev):
        if B == self.B:
            return
        dt, H, I = self.dtype, self.H, 4 * self.H
        e = lambda *s, dtype=dt: torch.empty(s, dtype=dtype, device=dev)  # noqa: E731
        self.kc = [torch.zeros((B, self.nh, self.Tcap, 64), dtype=dt, device=dev) for _ in range(self.nl)]
        self.vc = [torch.zeros((B, self.nh, self.Tcap, 64), dtype=dt, device=dev) for _ in range(self.nl)]
        self.ws = dict(h=e(B, H), qkv=e(B, 3 * H), ctx=e(B, H), ao=e(B, H), h1=e(B, H), ff=e(B, I), fo=e(B, H),
                       h2=e(B, H), logits=e(B, self.ldz, dtype=torch.float32), ln_stat=e(2, B, dtype=torch.float32))
        self.seq = torch.zeros((B, self.Tcap), dtype=torch.int64, device=dev)
        self.len0_dev = torch.zeros(B, dtype=torch.int32, device=dev)
        self.B = B
        self.desc = None

    def _build_desc(self):
        d = _Desc()
        eng, arch, dt = self.eng, self.eng.arch, self.dtype
        d.dtype, d.B, d.H, d.nh, d.n_layer, d.n_inner = ops.dt_code(dt), self.B, self.H, self.nh, self.nl, 4 * self.H
        d.V, d.Tcap, d.n_pos, d.ldz, d.ln_eps = self.V, self.Tcap, self.cfg.n_positions, self.ldz, float(arch.eps)
        d.w_stored_in_out = int(eng.wt is None)
        d.tok, d.pos = self.gpt.tokens_embed.weight.data_ptr(), self.gpt.positions_embed.weight.data_ptr()
        d.head_w = self.head_w.data_ptr()
        d.seq, d.len0 = self.seq.data_ptr(), self.len0_dev.data_ptr()
        for k, v in self.ws.items():
            setattr(d, k, v.data_ptr())
        for i, blk in enumerate(arch.layers):
            L = d.layers[i]
            lins = arch.lins(blk, self.flat, dt)
            if lins[2].n_out != 4 * self.H:
                raise NotImplementedError("GptDecoder: the FFN width must be 4 x n_embd")
            for j, lin in enumerate(lins):
                w = eng.wt.get(lin.W) if eng.wt is not None else lin.W
                L.w[j], L.b[j] = w.data_ptr(), lin.b.data_ptr()
            for j, ln in enumerate(arch.lns(blk)):
                L.ln_g[j], L.ln_b[j] = ln.weight.data_ptr(), ln.bias.data_ptr()
            L.kcache, L.vcache = self.kc[i].data_ptr(), self.vc[i].data_ptr()
        self.desc = d

    # ------------------------------------------------------------------ the prompt
    @torch.no_grad()
    def prefill(self, x, attention_mask=None, steps=1, temperature=1.0, top_k=0, greedy=True, u=None, forced=None):
        """Run the prompt x [B, L] (right-padded, attention_mask [B, L] or None = all ones) through the engine forward,
        fill the caches with the K / V of its valid rows, draw generated token 0 into column len0 of `seq`, and return
        the logits of each sequence's last valid position, fp32 [B, V].

        steps: tokens this generation will draw in all (prefill's + steps - 1 calls of step); u fp32 [steps, B]
        (needed unless greedy); forced int64 [B, steps]: teacher forcing. Every check is made before any launch."""
        if x.dim() != 2 or not x.is_cuda:
            raise ValueError("prefill: x must be a [B, L] GPU tensor of token ids")
        B, L = x.shape
        dev = x.device
        mask_np = np.ones((B, L), dtype=np.int64) if attention_mask is None else attention_mask.detach().cpu().numpy()
        if mask_np.shape != (B, L):
            raise ValueError(f"attention_mask {mask_np.shape} does not match x {(B, L)}")
        lens = check_prefix_mask(mask_np)
        max_len0 = int(lens.max())
        if steps < 1:
            raise ValueError("prefill: steps must be at least 1")
        if max_len0 + steps - 1 > self.cap:
            raise ValueError(f"prefill: prompt {max_len0} + {steps} generated tokens needs a context of "
                             f"{max_len0 + steps - 1} > min(max_len, n_positions) = {self.cap}")
        if not greedy and (u is None or tuple(u.shape) != (steps, B)):
            raise ValueError("prefill: sampling needs uniforms u of shape [steps, B]")
        if forced is not None and tuple(forced.shape) != (B, steps):
            raise ValueError("prefill: forced must be [B, steps]")
        if not (temperature > 0) or not (0 <= int(top_k or 0) <= self.V):
            raise ValueError("prefill: temperature > 0 and top_k in 0..V")
        self.model.eval()
        self._alloc(B, dev)
        fresh = self._bind_weights()
        if fresh or self.desc is None:
            self._build_desc()
        d = self.desc
        self.skinny = bool(GptDecoder.skinny_gemm and self.dtype == torch.bfloat16 and self.eng.wt is not None
                           and B <= 16)
        d.use_skinny = int(self.skinny)
        self.steps, self.max_len0 = int(steps), max_len0
        self.u = None if u is None else u.to(dev, torch.float32).contiguous()
        self.forced = None if forced is None else forced.to(dev, torch.int64).contiguous()
        self.chosen = torch.zeros((B, steps), dtype=torch.int64, device=dev)
        self.prob = torch.zeros((steps, B), dtype=torch.float32, device=dev)
        d.steps, d.max_len0 = self.steps, max_len0
        d.top_k, d.greedy, d.temperature = int(top_k or 0), int(bool(greedy)), float(temperature)
        d.u = ops.P(self.u)
        d.forced = ops.P(self.forced)
        d.chosen, d.prob = self.chosen.data_ptr(), self.prob.data_ptr()

        mask = torch.from_numpy(mask_np).to(dev)
        self.len0_dev.copy_(torch.from_numpy(lens.astype(np.int32)))
        self.seq.zero_()
        Lc = min(L, self.Tcap)  # (every valid prompt column is below cap < Tcap)
        self.seq[:, :Lc] = (x * mask)[:, :Lc]  # (the padded columns are overwritten as the sequence grows)
        # K / V of the prompt rows: [B L, 3H] -> [B, nh, L, 64] per layer (torch indexing: once per generation). A padded
        # position p >= len0[b] is never read: the step that reaches it stores its own K / V there first.
        nh = self.nh

        def sink(i, qkv_buf):
            q = qkv_buf[:B * L].view(B, L, 3, nh, 64)
            self.kc[i][:, :, :Lc] = q[:, :Lc, 1].permute(0, 2, 1, 3)
            self.vc[i][:, :, :Lc] = q[:, :Lc, 2].permute(0, 2, 1, 3)

        _, hidden, _ = self.eng.forward(x.contiguous(), mask, False, 0, kv_sink=sink)
        last = torch.from_numpy((np.arange(B) * L + lens - 1).astype(np.int64)).to(dev)
        logits = head_logits(hidden.index_select(0, last), self.head_w)
        sample(logits, self.V, temperature, top_k, greedy, None if self.u is None else self.u[0], seq=self.seq,
               len0=self.len0_dev, max_len0=max_len0, col_off=0, forced=self.forced, forced_ld=steps,
               chosen=self.chosen, chosen_ld=steps, prob=self.prob[0])
        return logits[:, :self.V]

    # ------------------------------------------------------------------ one token
    def step(self, t):
        """Enqueue decode step t (0 .. steps-2): embeds column len0 + t, appends its K / V, draws generated token
        t + 1 into column len0 + t + 1. No host synchronisation."""
        if self.desc is None:
            raise RuntimeError("GptDecoder.step before prefill")
        _lib.call("vcg_gpt_decode_step", ctypes.addressof(self.desc), int(t), ops.stream())

    def step_logits(self, t):
        """step(t), then the logits it sampled from: fp32 [B, V] (a copy; tests)."""
        self.step(t)
        return self.ws["logits"][:, :self.V].clone()

    def sample(self, logits, **kw):
        """The sampler kernel on fp32 logits [B, ldz] (vcg_hip.gpt_decode.sample)."""
        return sample(logits, self.V, **kw)

    def result(self):
        """(seq [B, Tcap] int64 device tensor, chosen [B, steps], prob [steps, B])"""
        return self.seq, self.chosen, self.prob
