"""Drop-in for reference model/lang/bert_hugface_listnet.py:18-199 (its BertHugface): the listwise (ListNet) stage of the
language model. A slate of one video's clips -- the boundary clip first -- is ranked against that boundary clip, and the
2-way boundary head is trained on a balanced selection of the slate's rows in the same step.

`base_model` is a `vcg_hip.nn.BertModel` with HF parameter names, executed by libvcg_hip; a local HF-format state dict
can be loaded via `checkpoint=` or $VCG_BERT_CHECKPOINT, as in bert_hugface.py. `train_forward` runs ONE BertFn pass
over the B S sequences that reads only the pooler output (unpadded rows, the last layer on the CLS rows), then the fused
loss of vcg_hip/listnet.py (csrc/listnet.hip). State-dict names are the reference's: `base_model.*`, `head.*` and, after
`build_chapter_head()`, `surrogate_head.*`, which the reference builds and never uses in a forward.

Not carried over: `get_attention=True` (the fused attention never forms the probabilities) and `train_forward` with
pretrain_stage=True (the reference's branch indexes [B S, L, V] logits with [B, S] targets and no driver runs it; the
masked-LM stage is model/lang/bert_hugface.py's `mlm_loss`). Both raise NotImplementedError.
"""
import logging
import os

import torch
import torch.nn as nn

from vcg_hip.nn import BertConfig, BertModel, NativeRoot

from .bert_hugface import _load_hf_state
from .bert_hugface_constrast import _no_decay  # (the same grouping rule, reference :83-98)

logger = logging.getLogger(__name__)


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
        print("number of parameters: ", sum(p.numel() for p in self.base_model.parameters()))

    def build_chapter_head(self):
        """:42-54 -- the (unused) surrogate head and the 2-way boundary head, normal(0, 0.02) weights, zero biases."""
        dev = self.head.weight.device
        self.surrogate_head = nn.Linear(self.embed_size, 1, bias=True).to(dev)
        self.surrogate_head.weight.data.normal_(mean=0.0, std=0.02)
        self.surrogate_head.bias.data.zero_()
        self.head = nn.Linear(self.embed_size, 2, bias=True).to(dev)
        self.head.weight.data.normal_(mean=0.0, std=0.02)
        self.head.bias.data.zero_()

    def load_constrast_checkpoint(self, checkpoint_path):
        """:57-65 -- base_model starts from the contrastive stage's encoder_q.*, strictly."""
        from vcg_hip.build import load_contrast_pretrain
        load_contrast_pretrain(self.base_model, checkpoint_path)

    def fix_backbone(self):
        for pn, p in self.named_parameters():
            if "pooler" in pn or "head" in pn:
                continue
            p.requires_grad = False

    # ------------------------------------------------------------------ optimiser
    def param_groups(self, weight_decay):
        """[decay group, no-decay group] over every parameter, each sorted by name (:83-112)."""
        named = dict(self.named_parameters())
        decay = sorted(n for n in named if not _no_decay(n, n.rsplit(".", 1)[-1]))
        no_decay = sorted(n for n in named if _no_decay(n, n.rsplit(".", 1)[-1]))
        return [{"params": [named[n] for n in decay], "weight_decay": weight_decay},
                {"params": [named[n] for n in no_decay], "weight_decay": 0.0}]

    def configure_optimizers(self, train_config):
        # surrogate_head takes no part in any forward: it has no gradient in the reference, so its AdamW gives it no
        # update and no decay. The fused step skips it, as it skips fix_backbone's frozen parameters.
        from vcg_hip.optim import FusedAdamW
        sh = getattr(self, "surrogate_head", None)
        skip = list(sh.parameters()) if sh is not None else []
        return FusedAdamW(self.param_groups(train_config.weight_decay), lr=train_config.learning_rate,
                          betas=train_config.betas, model=self, skip=skip)

    # ------------------------------------------------------------------ forward
    _vcg_hooks = None

    def set_grad_hooks(self, hooks):
        """hooks(params) is called from the backward when those parameters' gradients are final (DDP)."""
        object.__setattr__(self, "_vcg_hooks", hooks)

    def _pooled(self, text_ids, attention_mask):
        """The pooler output [N, H] of N sequences in the compute dtype (autograd-connected); nothing else is read, so
        padded token rows are dropped and the last layer past its attention runs on the CLS rows only."""
        from vcg_hip.bert import BertEncoderEngine, PackingRequest
        from vcg_hip.functions import BertFn
        from vcg_hip.nn import new_seed
        self.base_model.check_text_len(text_ids.shape[-1])
        f = self.native_flat()  # (the root's flat buffers, heads included)
        if attention_mask is None:
            attention_mask = torch.ones_like(text_ids)
        bert = BertEncoderEngine(self.base_model, f, self.compute_dtype())
        bert.pooled_only = True
        if bert.packs(text_ids):
            bert.packing = PackingRequest(attention_mask)
        pooled, _ = BertFn.apply(text_ids, attention_mask, self._anchor(text_ids.device), bert,
                                 torch.is_grad_enabled(), new_seed(), self._vcg_hooks)
        return pooled

    def _chapter_head(self):
        if getattr(self, "surrogate_head", None) is None or tuple(self.head.weight.shape) != (2, self.embed_size):
            raise RuntimeError("call build_chapter_head() first")
        return self.head

    def train_forward(self, x, attention_mask, targets, balance_selected_indices, binary_cls_label,
                      get_attention=False):
        """:116-181. x, attention_mask [B, S, L]; targets [B, S] (column 0, the boundary clip's own, is not read);
        balance_selected_indices [M] rows of the [B S, H] pooled output and binary_cls_label [M] in {0, 1}: host
        lists / CPU tensors are checked as they are, device tensors cost one small device-to-host copy. Returns
        binary_logits [M, 2], binary_prob [M, 2] (fp32, detached) and loss = surrogate + binary (also
        surrogate_loss and binary_loss on their own)."""
        from vcg_hip import ops
        from vcg_hip.listnet import ListNetLossFn
        if get_attention:
            raise NotImplementedError("get_attention=True: the fused attention kernels never form the attention "
                                      "probabilities, so there is nothing to return")
        if self.pretrain_stage:
            raise NotImplementedError("train_forward with pretrain_stage=True: the masked-LM stage is "
                                      "model.lang.bert_hugface.BertHugface.mlm_loss (the reference's branch here "
                                      "indexes [B S, L, V] logits with [B, S] targets and no driver runs it)")
        head = self._chapter_head()
        B, S, L = x.shape
        if tuple(targets.shape) != (B, S):
            raise ValueError(f"train_forward: targets {tuple(targets.shape)} against a [{B}, {S}] slate batch")
        # every refusal before the encoder runs
        idx = ops.ListnetIndices(balance_selected_indices, binary_cls_label, B * S, x.device)
        ops.listnet_check_shape(B, S, self.embed_size, idx.M)
        pooled = self._pooled(x.reshape(-1, L), attention_mask.reshape(-1, L) if attention_mask is not None else None)
        t = targets.to(device=x.device, dtype=torch.float32).contiguous()
        loss, logits, prob, parts = ListNetLossFn.apply(pooled, self._anchor(x.device), head, t, idx, self._vcg_hooks)
        return {"binary_logits": logits, "binary_prob": prob, "loss": loss, "surrogate_loss": parts[0],
                "binary_loss": parts[1]}

    def test_forward(self, x, attention_mask, targets):
        """:183-199 -- x, attention_mask [N, L], targets [N]: the boundary head on every clip, plain cross-entropy."""
        from vcg_hip.functions import cross_entropy
        from vcg_hip.linear_head import linear_head
        head = self._chapter_head()
        pooled = self._pooled(x, attention_mask)
        logits, prob = linear_head(self, head, pooled)
        return {"binary_logits": logits, "binary_prob": prob, "loss": cross_entropy(logits, targets)}
