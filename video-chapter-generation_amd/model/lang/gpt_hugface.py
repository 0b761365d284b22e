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
