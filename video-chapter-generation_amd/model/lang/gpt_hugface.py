"""Drop-in for reference model/lang/gpt_hugface.py:12-101 (GPTHugface), the generative pre-training stage's model
(pretrain_lang_model_hugface.py, model_type "gpt").

`base_model` is an OpenAI GPT decoder with transformers' parameter names and Conv1D layouts, executed by libvcg_hip
(vcg_hip/gpt.py: causal fused attention, tanh-GELU epilogues). The reference's
`OpenAIGPTModel.from_pretrained('openai-gpt')` needs the network; here the model is built from the openai-gpt config
(random init) and a local HF-format state dict can be loaded via `checkpoint=` or $VCG_GPT_CHECKPOINT.

`forward` returns the reference's (logits [B, L, V], loss); `lm_loss` is the fused next-token loss the native driver
trains with, which projects only the positions with a target onto the vocabulary and stores no [R, V] fp32 logits
(vcg_hip/mlm.py, csrc/mlm_head.hip -- the masked-LM stage's head: rows = positions whose target is not -1).

Attention masks: see vcg_hip.nn.OpenAIGPTModel -- with a LEFT-padded mask the queries at the leading masked positions
diverge from transformers (which lets them attend to future valid keys); right padding, holes behind a valid position
0 and fully masked sequences agree.
"""
import logging
import os

import numpy as np
import torch
import torch.nn as nn

from vcg_hip.nn import NativeRoot, OpenAIGPTConfig, OpenAIGPTModel
from vcg_hip.optim import configure_adamw

logger = logging.getLogger(__name__)


def _load_hf_state(model, path):
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(path)
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if "model_state_dict" in sd:
            sd = sd["model_state_dict"]
    for pre in ("transformer.", "base_model."):  # (OpenAIGPTLMHeadModel's / this class's own state dict)
        if any(k.startswith(pre) for k in sd):
            sd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
    # (buffers of older transformers versions: the causal mask and the position ids)
    sd = {k: v for k, v in sd.items() if not k.endswith(".attn.bias") and not k.endswith("position_ids")
          and not k.startswith("lm_head.")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    if missing or unexpected:  # (a file of another model would otherwise load nothing, silently)
        raise ValueError(f"{path}: not an OpenAIGPTModel state dict for this config: missing {sorted(missing)[:3]} "
                         f"({len(missing)}), unexpected {sorted(unexpected)[:3]} ({len(unexpected)})")
    logger.info("loaded %s", path)


def no_decay(full_name, leaf_name):
    """gpt_hugface.py:51-64: biases and every name containing "ln" or "emb" take no weight decay."""
    return leaf_name.endswith("bias") or "ln" in full_name or "emb" in full_name


class GPTHugface(NativeRoot, nn.Module):
    def __init__(self, checkpoint=None, config=None):
        super().__init__()
        self.base_model = OpenAIGPTModel(config if config is not None else OpenAIGPTConfig())
        ckpt = checkpoint or os.environ.get("VCG_GPT_CHECKPOINT")
        if ckpt:
            self.load_checkpoint(ckpt)
        self.vocab_size = self.base_model.tokens_embed.num_embeddings
        self.embed_size = self.base_model.tokens_embed.embedding_dim
        self.head = nn.Linear(self.embed_size, self.vocab_size, bias=False)
        self.head.weight.data.normal_(mean=0.0, std=0.02)
        print("number of parameters: ", sum(p.numel() for p in self.base_model.parameters()))

    def load_checkpoint(self, path):
        """Load a local HF-format openai-gpt state dict (OpenAIGPTModel's keys, also under "transformer." or
        "base_model.") into the decoder; keys that do not match are a ValueError."""
        _load_hf_state(self.base_model, path)

    def build_chapter_head(self, output_size):
        self.head = nn.Linear(self.embed_size, output_size, bias=True)
        self.head.weight.data.normal_(mean=0.0, std=0.02)
        self.head.bias.data.zero_()

    def configure_optimizers(self, train_config):
        return configure_adamw(self, train_config, no_decay=no_decay)

    _vcg_hooks = None

    def set_grad_hooks(self, hooks):
        """hooks(params) is called from the backward when those parameters' gradients are final (DDP)."""
        object.__setattr__(self, "_vcg_hooks", hooks)

    def _last_hidden(self, x, attention_mask):
        """The decoder's last hidden state [B L, H] in the compute dtype (autograd-connected)."""
        self.native_flat()  # (the root's flat buffers, head included, before the decoder binds to them)
        return self.base_model.native_forward(x, attention_mask, hooks=self._vcg_hooks)

    def _is_vocab_head(self):
        return self.head.bias is None and self.head.out_features == self.vocab_size

    def _fused_loss(self, last, rows, tgt):
        """rows / tgt: select_targets' (the positions with a target, their targets), not empty."""
        from vcg_hip.mlm import MlmLossFn
        n_valid = rows.numel()
        dev = last.device
        loss, n_correct = MlmLossFn.apply(last, self._anchor(dev), self, self.head, rows.to(dev), tgt.to(dev),
                                          self._vcg_hooks)
        return loss, n_correct, n_valid

    def lm_loss(self, x, attention_mask, targets):
        """The next-token loss of pretrain_lang_model_hugface.py:127-141 without the logits: (mean cross-entropy over
        the positions with targets != -1, number of those whose argmax is the target, their number). Only those
        positions are projected onto the vocabulary (csrc/mlm_head.hip). No such position: a NaN loss (F.cross_entropy
        on an empty selection), no kernel launched, every gradient left as it is."""
        if not self._is_vocab_head():
            raise RuntimeError("lm_loss needs the vocabulary head (build_chapter_head replaced it)")
        from vcg_hip.mlm import select_targets
        dev = x.device
        rows, tgt = select_targets(targets, self.vocab_size)  # (one device-to-host copy per step)
        if rows.numel() == 0:
            return (torch.full((), float("nan"), device=dev, requires_grad=torch.is_grad_enabled()),
                    torch.zeros((), dtype=torch.int64, device=dev), 0)
        return self._fused_loss(self._last_hidden(x, attention_mask), rows, tgt)

    # generate(): draw the tokens whose context fits block_size on the KV cache (vcg_hip/gpt_decode.py); False: every
    # token re-runs the forward on its window, the reference's algorithm (tests and tools compare both)
    use_kv_cache = True

    @torch.no_grad()
    def generate(self, x, attention_mask=None, steps=1, temperature=1.0, sample=False, top_k=None, block_size=None,
                 generator=None, forced=None):
        """Text generation, the reference's common_utils/language_model_utils.py:token_idx_sample (temperature, top-k,
        multinomial or argmax) for a right-padded batch: x [B, L] token ids, attention_mask [B, L] (None: all ones;
        each row a prefix of ones with at least one token -- left padding, holes and empty rows are a ValueError).
        Returns (seq [B, max(len0) + steps] int64: row b holds its prompt and then its `steps` new tokens, zeros behind;
        new_tokens [B, steps]).

        The model is put in eval mode, as the reference does. While the context the model sees stays within block_size
        (default: the position table) the tokens are drawn on the KV cache (vcg_hip/gpt_decode.py: one enqueued chain
        per token, the next token chosen on the device, no host synchronisation). Beyond it the reference slides the
        window, x[:, -block_size:], which shifts every learned position: the cache is invalid there, so those tokens
        re-run the native forward on the cropped window and apply the sampler kernel to its last row
        (plan_generation says how many of each).

        sample=True draws by inverse CDF, in vocabulary order over the kept set, from uniforms made once by
        torch.rand((steps, B), generator=generator): reproducible for a seeded generator, but NOT torch.multinomial's
        random stream -- the tokens differ from the reference's for the same seed, their distribution does not.
        forced [B, steps] (tests): teacher forcing -- new_tokens still holds the sampler's choice, but the forced
        token is what is written to seq and fed back."""
        from vcg_hip import gpt_decode as gd
        from vcg_hip.mlm import _head_weights
        if not self._is_vocab_head():
            raise RuntimeError("generate needs the vocabulary head (build_chapter_head replaced it)")
        if x.dim() != 2 or not x.is_cuda:
            raise ValueError("generate: x must be a [B, L] GPU tensor of token ids (there is no CPU path)")
        B, L = x.shape
        dev = x.device
        n_pos = self.base_model.config.n_positions
        block = n_pos if block_size is None else int(block_size)
        if not 1 <= block <= n_pos:
            raise ValueError(f"generate: block_size {block} outside 1..n_positions = {n_pos}")
        steps = int(steps)
        if steps < 1:
            raise ValueError("generate: steps must be at least 1")
        mask_np = (np.ones((B, L), dtype=np.int64) if attention_mask is None
                   else attention_mask.detach().cpu().numpy())
        if mask_np.shape != (B, L):
            raise ValueError(f"attention_mask {mask_np.shape} does not match x {(B, L)}")
        lens = gd.check_prefix_mask(mask_np)
        if forced is not None and tuple(forced.shape) != (B, steps):
            raise ValueError("generate: forced must be [B, steps]")
        cached, sliding = gd.plan_generation(lens, steps, block)
        if not GPTHugface.use_kv_cache:
            cached, sliding = 0, steps
        self.eval()
        greedy = not sample
        u = None
        if sample:
            gdev = generator.device if generator is not None else "cpu"
            u = torch.rand((steps, B), generator=generator, device=gdev).to(dev, torch.float32)
        if forced is not None:
            forced = forced.to(dev, torch.int64).contiguous()
        max_len0 = int(lens.max())
        W = max_len0 + steps
        seq = torch.zeros((B, W), dtype=torch.int64, device=dev)
        mask_dev = torch.from_numpy(mask_np).to(dev)
        seq[:, :L] = (x * mask_dev)[:, :W]
        new_tokens = torch.zeros((B, steps), dtype=torch.int64, device=dev)
        len0_dev = torch.from_numpy(lens.astype(np.int32)).to(dev)
        if cached:
            dec = getattr(self, "_vcg_decoder", None)
            if dec is None or dec.cap != block or dec.dtype != self.compute_dtype():
                dec = gd.GptDecoder(self, block)
                object.__setattr__(self, "_vcg_decoder", dec)
            dec.prefill(x, attention_mask, steps=cached, temperature=temperature, top_k=top_k or 0, greedy=greedy,
                        u=None if u is None else u[:cached], forced=None if forced is None else forced[:, :cached])
            for t in range(cached - 1):
                dec.step(t)
            wc = min(W, dec.Tcap)
            seq[:, :wc] = dec.seq[:, :wc]  # (the one copy of the finished token matrix)
            new_tokens[:, :cached] = dec.chosen
        if sliding:
            head_w = None
            for g in range(cached, steps):
                cur = lens + g                      # each sequence's length before token g
                start = np.maximum(0, cur - block)  # its window: the last `block` tokens
                wl = cur - start
                Lw = int(wl.max())
                cols = start[:, None] + np.arange(Lw)[None, :]
                wmask = torch.from_numpy((np.arange(Lw)[None, :] < wl[:, None]).astype(np.int64)).to(dev)
                ids = seq.gather(1, torch.from_numpy(np.minimum(cols, W - 1)).to(dev)) * wmask
                last = self._last_hidden(ids, wmask)
                if head_w is None:
                    Wd, Wp = _head_weights(self, self.head, last.dtype)
                    head_w = Wd if Wp is None else Wp
                rows = torch.from_numpy((np.arange(B) * Lw + wl - 1).astype(np.int64)).to(dev)
                logits = gd.head_logits(last.index_select(0, rows), head_w)
                gd.sample(logits, self.vocab_size, temperature, top_k or 0, greedy, None if u is None else u[g],
                          seq=seq, len0=len0_dev, max_len0=max_len0, col_off=g,
                          forced=None if forced is None else forced[:, g:], forced_ld=steps,
                          chosen=new_tokens[:, g:], chosen_ld=steps)
        return seq, new_tokens

    def forward(self, x, attention_mask=None, targets=None):
        """gpt_hugface.py:82-101: (logits [B, L, V] fp32, autograd-connected; loss = the mean cross-entropy over the
        positions with targets != -1, or None without targets). With the chapter head: logits [B, L, output_size]."""
        B, L = x.shape
        last = self._last_hidden(x, attention_mask)
        if self._is_vocab_head():
            from vcg_hip.mlm import MlmLogitsFn
            z = MlmLogitsFn.apply(last, self._anchor(x.device), self, self.head, self._vcg_hooks)
            logits = z.view(B, L, -1)[..., :self.vocab_size]
            loss = None
            if targets is not None:
                # (the drop-in route: the head runs a second time inside the fused loss -- the logits above are a
                # returned value, the loss does not read them; the driver trains through lm_loss, one head pass)
                from vcg_hip.mlm import select_targets
                rows, tgt = select_targets(targets, self.vocab_size)
                loss = (self._fused_loss(last, rows, tgt)[0] if rows.numel()
                        else torch.full((), float("nan"), device=x.device))
            return logits, loss
        from vcg_hip.functions import cross_entropy
        from vcg_hip.linear_head import linear_head
        logits, _ = linear_head(self, self.head, last)
        loss = None
        if targets is not None:
            keep = torch.nonzero(targets.reshape(-1) != -1).reshape(-1)
            loss = cross_entropy(logits.index_select(0, keep), targets.reshape(-1).index_select(0, keep))
        return logits.view(B, L, -1), loss
