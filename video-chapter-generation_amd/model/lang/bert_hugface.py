"""Drop-in for reference model/lang/bert_hugface.py:13-132 (BertHugface).

`base_model` is a BERT-base encoder with HF parameter names, executed by libvcg_hip. The
reference's `BertModel.from_pretrained('bert-base-uncased')` needs the network; here the model
is built from the bert-base config (random init, 109,482,240 parameters as bert_hugface.py:31
reports) and a local HF-format state dict can be loaded via `checkpoint=` or $VCG_BERT_CHECKPOINT.

pretrain_stage=True is the masked-LM stage (pretrain_lang_model_hugface.py): `forward` returns the reference's
(logits [B, L, V], softmax over the sequence axis), and `mlm_loss` is the fused loss the native driver trains with,
which projects only the masked rows onto the vocabulary (vcg_hip/mlm.py, csrc/mlm_head.hip).
"""
import logging
import os

import torch
import torch.nn as nn

from vcg_hip.nn import BertConfig, BertModel, NativeRoot
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
    sd = {k[len("bert."):] if k.startswith("bert.") else k: v for k, v in sd.items()}
    sd = {k: v for k, v in sd.items() if not k.endswith("position_ids") and not k.endswith("token_type_ids")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    logger.info("loaded %s (missing %d, unexpected %d)", path, len(missing), len(unexpected))


class BertHugface(NativeRoot, nn.Module):
    def __init__(self, pretrain_stage=True, checkpoint=None, config=None):
        super().__init__()
        self.pretrain_stage = pretrain_stage
        config = config if config is not None else BertConfig(output_attentions=True)
        self.base_model = BertModel(config)
        ckpt = checkpoint or os.environ.get("VCG_BERT_CHECKPOINT")
        if ckpt:
            _load_hf_state(self.base_model, ckpt)
        self.vocab_size = self.base_model.config.vocab_size
        self.embed_size = self.base_model.config.hidden_size
        self.head = nn.Linear(self.embed_size, self.vocab_size, bias=False)
        self.head.weight.data.normal_(mean=0.0, std=0.02)
        print("backbone's parameters: ", sum(p.numel() for p in self.base_model.parameters()))

    def build_chapter_head(self):
        self.head = nn.Linear(self.embed_size, 2)

    def fix_backbone(self):
        for pn, p in self.named_parameters():
            if "pooler" in pn or "head" in pn:
                continue
            p.requires_grad = False

    def configure_optimizers(self, train_config):
        # pre-training: the pooler is outside the MLM graph, so the reference's AdamW never touches it (its
        # parameters have no gradient); the fused step skips them as it skips fix_backbone's frozen parameters
        skip = list(self.base_model.pooler.parameters()) if self.pretrain_stage and self.base_model.pooler else ()
        return configure_adamw(self, train_config, skip=skip)

    def _last_hidden(self, text_ids, attention_mask):
        """The encoder's last hidden state [B L, H] in the compute dtype (autograd-connected)."""
        self.native_flat()  # (the root's flat buffers, head included, before the encoder binds to them)
        _, last = self.base_model.native_forward(text_ids, attention_mask, hooks=self._vcg_hooks)
        return last

    _vcg_hooks = None

    def set_grad_hooks(self, hooks):
        """hooks(params) is called from the backward when those parameters' gradients are final (DDP)."""
        object.__setattr__(self, "_vcg_hooks", hooks)

    def mlm_loss(self, text_ids, attention_mask, targets):
        """Masked-LM loss of pretrain_lang_model_hugface.py:127-141 without the logits: (mean cross-entropy over the
        positions with targets != -1, number of those whose argmax is the target, their number). Only the masked rows
        are projected onto the vocabulary (csrc/mlm_head.hip). No masked position: a NaN loss (F.cross_entropy on an
        empty selection), no kernel launched, every gradient left as it is."""
        from vcg_hip.mlm import MlmLossFn, select_targets
        if not self.pretrain_stage:
            raise RuntimeError("mlm_loss needs pretrain_stage=True (the vocabulary head)")
        rows, tgt = select_targets(targets, self.vocab_size)
        n_valid = rows.numel()
        dev = text_ids.device
        if n_valid == 0:
            return (torch.full((), float("nan"), device=dev, requires_grad=torch.is_grad_enabled()),
                    torch.zeros((), dtype=torch.int64, device=dev), 0)
        rows, tgt = rows.to(dev), tgt.to(dev)
        last = self._last_hidden(text_ids, attention_mask)
        loss, n_correct = MlmLossFn.apply(last, self._anchor(dev), self, self.head, rows, tgt, self._vcg_hooks)
        return loss, n_correct, n_valid

    def forward(self, text_ids, attention_mask, get_attention=False):
        """bert_hugface.py:98-132. pretrain_stage: (logits [B, L, V] fp32, autograd-connected; prob = softmax over the
        sequence axis, the reference's F.softmax(logits, dim=1), detached); get_attention is accepted and ignored, as
        the reference computes the attentions and discards them."""
        from vcg_hip.linear_head import linear_head
        if self.pretrain_stage:
            from vcg_hip import ops
            from vcg_hip.mlm import MlmLogitsFn
            B, L = text_ids.shape
            last = self._last_hidden(text_ids, attention_mask)
            z = MlmLogitsFn.apply(last, self._anchor(text_ids.device), self, self.head, self._vcg_hooks)
            V = self.vocab_size
            prob = ops.seq_softmax_fwd(z.detach(), B, L, V, ldz=z.shape[1])
            return z.view(B, L, -1)[..., :V], prob
        base_output = self.base_model(input_ids=text_ids, attention_mask=attention_mask)
        return linear_head(self, self.head, base_output.pooler_output)
