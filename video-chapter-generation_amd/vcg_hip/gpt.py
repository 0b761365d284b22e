"""OpenAI GPT decoder on libvcg_hip (transformers OpenAIGPTModel semantics), forward and hand-written backward.

Reference use: GPTHugface.forward -> base_model(input_ids, attention_mask).last_hidden_state
(model/lang/gpt_hugface.py:82-89) with base_model = OpenAIGPTModel('openai-gpt') (:18). A GPT block has the BERT
layer's dataflow -- fused QKV projection, attention, output projection, LN(dropout(.) + res), FFN1 with GELU, FFN2,
LN(dropout(.) + res) -- so the layer loop, its GEMM routing, the weight-gradient side stream and the fp32
residual-gradient stream are BertEncoderEngine's (vcg_hip/bert.py). What differs is stated by _GptArch:

  * the attention is causal (ops.ATTN_CAUSAL: the fused kernels skip the tiles above the diagonal; fp32 parity mode:
    the unfused softmax with the same rule);
  * the activation is the tanh form of GELU (ops.ACT_GELU_TANH / _BWD epilogues);
  * the embedding is dropout(tokens_embed[id] + positions_embed[t]): no token types, no LayerNorm
    (vcg_gpt_embed_fwd / _bwd);
  * LayerNorm eps 1e-5, no pooler;
  * the Linear weights are HF Conv1D, stored [in][out]: the stored weight is the K-contiguous operand of the
    input-gradient GEMMs, and the once-per-weight-generation transposed copy (bert._LinearT) serves the forward.
"""
from . import ops
from .bert import BertEncoderEngine, _Lin


class _GptArch:
    causal = True
    conv1d = True  # HF Conv1D weights, [in][out]: the forward reads the transposed copy
    act, act_bwd = ops.ACT_GELU_TANH, ops.ACT_GELU_TANH_BWD
    pooler = None

    def __init__(self, m):
        self.m = m
        cfg = m.config
        self.H, self.nh = cfg.n_embd, cfg.n_head
        self.max_pos, self.eps = cfg.n_positions, cfg.layer_norm_epsilon
        self.layers = m.h
        self.name = "OpenAIGPTModel"

    def dropouts(self):
        hid = [self.m.drop] + [d for blk in self.layers for d in (blk.attn.resid_dropout, blk.mlp.dropout)]
        return hid, [blk.attn.attn_dropout for blk in self.layers]

    def lins(self, blk, flat, dt):
        out = []
        for c in (blk.attn.c_attn, blk.attn.c_proj, blk.mlp.c_fc, blk.mlp.c_proj):
            out.append(_Lin(flat.compute_view(c.weight, dt), c.bias, c.weight.grad, c.bias.grad, c.nx, c.nf,
                            conv1d=True, train=c.weight.requires_grad))
        return out

    def lns(self, blk):
        return blk.ln_1, blk.ln_2

    def embed_fwd(self, ids, B, L, dt, p, seed):
        # (the kernels index the table by id, as BERT's do: ids are validated where they are made, on the host --
        # data.youtube_subtitle_dataset.encode_gpt)
        m = self.m
        return ops.gpt_embed_fwd(ids, m.tokens_embed.weight, m.positions_embed.weight, B, L, self.H, dt, p, seed), None

    def embed_bwd(self, dh, ids, saved, B, L, dt, p, seed):
        m = self.m
        ops.gpt_embed_bwd(dh, ids, m.tokens_embed.weight.grad, m.positions_embed.weight.grad, B, L, self.H, p, seed,
                          storage_dtype=dt)
        return [m.tokens_embed.weight, m.positions_embed.weight]


class GptEncoderEngine(BertEncoderEngine):
    arch_cls = _GptArch
