"""Drop-in for reference model/lang/bert_hugface_constrast.py:12-165 (BertHugfaceConstrast): the shot-contrastive (MoCo)
stage of the language model -- a query BERT, a momentum key BERT and a queue of K keys at temperature T.

The two encoders are `vcg_hip.nn.BertModel`s with HF parameter names, executed by libvcg_hip. The reference's
`BertModel.from_pretrained('bert-base-uncased')` needs the network; here the model is built from the bert-base config
and a local HF-format state dict can be loaded into both encoders via `checkpoint=` or $VCG_BERT_CHECKPOINT.

`forward` returns the reference's (logits [N, 1 + K], labels); `contrast_loss` is the fused route the native driver
trains with (csrc/contrast.hip, vcg_hip/contrast.py): nothing N x K is stored in fp32, the momentum update is one
launch over the key encoder's span of the flat parameter buffer, and the queue's operand copy is key-major in the
compute dtype. Both routes run the reference's order (:97-165): the query encode, then without gradient the momentum
update, the candidate encode through encoder_q, the selection, the key encode through encoder_k; then the logits and
the enqueue. All of it happens in eval mode too, as in the reference.
"""
import logging
import os

import torch
import torch.nn as nn
from torch.nn import functional as F

from vcg_hip.nn import BertConfig, BertModel, NativeRoot

from .bert_hugface import _load_hf_state

logger = logging.getLogger(__name__)


def _no_decay(full_name, leaf_name):
    """This class's grouping rule (reference :66-79): biases, and names containing "ln" or "emb". HF's
    `LayerNorm.weight` contains no "ln", so outside `embeddings.` it IS decayed -- unlike TwoStream / BertHugface."""
    return leaf_name.endswith("bias") or "ln" in full_name or "emb" in full_name


class BertHugfaceConstrast(NativeRoot, nn.Module):
    def __init__(self, K=65536, m=0.999, T=0.07, config=None, checkpoint=None):
        super().__init__()
        self.K = K
        self.m = m
        self.T = T
        config = config if config is not None else BertConfig()
        self.encoder_q = BertModel(config)
        self.encoder_k = BertModel(config)
        ckpt = checkpoint or os.environ.get("VCG_BERT_CHECKPOINT")
        if ckpt:
            _load_hf_state(self.encoder_q, ckpt)
        # (the reference loads the same pretrained weights into both)
        self.encoder_k.load_state_dict(self.encoder_q.state_dict())
        self.vocab_size = self.encoder_q.config.vocab_size
        self.embed_size = self.encoder_q.config.hidden_size
        self.register_buffer("queue", F.normalize(torch.randn(self.embed_size, K), dim=0))
        self.register_buffer("queue_ptr", torch.zeros(1, dtype=torch.long))
        print("number of parameters: ", sum(p.numel() for p in self.encoder_q.parameters()))

    # ------------------------------------------------------------------ optimiser
    def param_groups(self, weight_decay):
        """[decay group, no-decay group] over every parameter (encoder_k included, as the reference's), each sorted by
        name."""
        named = dict(self.named_parameters())
        decay = sorted(n for n in named if not _no_decay(n, n.rsplit(".", 1)[-1]))
        no_decay = sorted(n for n in named if _no_decay(n, n.rsplit(".", 1)[-1]))
        return [{"params": [named[n] for n in decay], "weight_decay": weight_decay},
                {"params": [named[n] for n in no_decay], "weight_decay": 0.0}]

    def configure_optimizers(self, train_config):
        # encoder_k has no gradient in the reference, so its AdamW gives it no update and no decay: the fused step
        # skips its span
        from vcg_hip.optim import FusedAdamW
        return FusedAdamW(self.param_groups(train_config.weight_decay), lr=train_config.learning_rate,
                          betas=train_config.betas, model=self, skip=list(self.encoder_k.parameters()))

    # ------------------------------------------------------------------ key encoder
    def _key_span(self, flat):
        """(offset of encoder_q's span, offset of encoder_k's span, length) in the flat buffer. The single-launch
        momentum update needs both encoders laid out alike; checked once per flat buffer."""
        c = getattr(self, "_vcg_key_span", None)
        if c is not None and c[0] is flat:
            return c[1]
        qs = [(n, o) for n, o in zip(flat.names, flat.offsets) if n.startswith("encoder_q.")]
        ks = [(n, o) for n, o in zip(flat.names, flat.offsets) if n.startswith("encoder_k.")]
        assert qs and len(qs) == len(ks) and len(qs) + len(ks) == len(flat.names), "unexpected flat layout"
        oq, ok = qs[0][1], ks[0][1]
        n = ok - oq
        assert flat.total - ok == n, "the two encoders' spans differ in length"
        for (nq, a), (nk, b) in zip(qs, ks):
            assert nq[len("encoder_q."):] == nk[len("encoder_k."):] and a - oq == b - ok, \
                f"encoder_q / encoder_k are laid out differently at {nq} / {nk}"
        object.__setattr__(self, "_vcg_key_span", (flat, (oq, ok, n)))
        return oq, ok, n

    @torch.no_grad()
    def _momentum_update_key_encoder(self):
        """param_k = param_k * m + param_q * (1 - m) for every pair (:39-40), one launch; the key encoder's bf16 shadow
        is rewritten in the same pass."""
        from vcg_hip import ops
        f = self.native_flat()
        oq, ok, n = self._key_span(f)
        ops.momentum_update(f.data[ok:ok + n], f.data[oq:oq + n], self.m,
                            f.shadow[ok:ok + n] if f.shadow is not None else None)

    # ------------------------------------------------------------------ queue
    def _operand_queue(self):
        """queue_km [K rounded up to 8, H]: the key-major copy of `queue` in the compute dtype. Rebuilt on first use,
        after load_state_dict / .to() / a precision change, and when `queue`'s version counter shows an outside
        write."""
        from vcg_hip import ops
        q = self.queue
        if q.dtype != torch.float32 or not q.is_cuda or not q.is_contiguous():
            raise RuntimeError("BertHugfaceConstrast: `queue` must be a contiguous fp32 GPU buffer")
        key = (q.data_ptr(), q._version, self.compute_dtype(), q.device)
        if getattr(self, "_vcg_km_key", None) != key:
            km = ops.queue_rebuild(q, self.compute_dtype(), out=getattr(self, "_vcg_km", None))
            object.__setattr__(self, "_vcg_km", km)
            object.__setattr__(self, "_vcg_km_key", key)
        return self._vcg_km

    @torch.no_grad()
    def _dequeue_and_enqueue(self, keys):
        """:42-52 -- the keys go into `queue` and its operand copy at the device pointer, which then advances."""
        from vcg_hip import ops
        km = self._operand_queue()
        ops.queue_enqueue(keys.contiguous(), self.queue, km, self.queue_ptr)
        # (the kernel's write is the module's own: the version counter does not move)

    # ------------------------------------------------------------------ forward
    last_k0 = None

    def _pooled(self, enc, ids, mask):
        pooled, _ = enc.native_forward(ids, mask)
        return pooled

    def _embed(self, query_ids, query_mask, cand_ids, cand_mask):
        """(q with gradient, k without) [N, H], both normalised, in the compute dtype (:100-145)."""
        from vcg_hip import ops
        from vcg_hip.contrast import L2NormFn
        B, C, L = cand_ids.shape
        if self.K % B != 0:
            raise ValueError(f"BertHugfaceConstrast: the queue size {self.K} must be a multiple of the batch size {B}")
        self.native_flat()  # (the root's flat buffers before the encoders bind to them)
        pooled_q = self._pooled(self.encoder_q, query_ids, query_mask)
        q = L2NormFn.apply(pooled_q)
        with torch.no_grad():
            self._momentum_update_key_encoder()
            cand = self._pooled(self.encoder_q, cand_ids.reshape(-1, L), cand_mask.reshape(-1, L))
            k0 = ops.contrast_select(pooled_q.detach().contiguous(), cand.view(B, C, -1))
            rows = torch.arange(B, device=k0.device)
            k_pooled = self._pooled(self.encoder_k, cand_ids[rows, k0], cand_mask[rows, k0])
            k, _ = ops.l2norm_fwd(k_pooled.contiguous())
        object.__setattr__(self, "last_k0", k0)
        return q, k

    def contrast_loss(self, query_clip_text_id, query_att_mask, pos_candidates_text_id, pos_candidates_att_mask,
                      device=None):
        """The fused route: (mean InfoNCE loss, number of rows whose argmax is the positive, N). `last_k0` holds the
        selected candidate indices."""
        from vcg_hip.contrast import InfoNceLossFn
        q, k = self._embed(query_clip_text_id, query_att_mask, pos_candidates_text_id, pos_candidates_att_mask)
        loss, n_correct = InfoNceLossFn.apply(q, k, self._operand_queue(), self.K, 1.0 / self.T)
        self._dequeue_and_enqueue(k)
        return loss, n_correct, q.shape[0]

    def forward(self, query_clip_text_id, query_att_mask, pos_candidates_text_id, pos_candidates_att_mask, device=None):
        """:97-165 -> (logits fp32 [N, 1 + K] with the positive in column 0, labels int64 zeros [N])."""
        from vcg_hip.contrast import InfoNceLogitsFn
        q, k = self._embed(query_clip_text_id, query_att_mask, pos_candidates_text_id, pos_candidates_att_mask)
        logits = InfoNceLogitsFn.apply(q, k, self._operand_queue(), self.K, 1.0 / self.T)
        labels = torch.zeros(logits.shape[0], dtype=torch.long, device=logits.device)
        self._dequeue_and_enqueue(k)
        return logits, labels
