"""Drop-in for reference model/lang/pegasus_hugface.py:19-146 (PegasusHugface), the chapter-title model of stage 2
(train_chapter_title_gen.py, test_chapter_title_gen.py, test_whole_pipeline_per_video.py).

`base_model` is a Pegasus encoder-decoder with transformers' state-dict keys, executed by libvcg_hip
(vcg_hip/pegasus.py: pre-LayerNorm blocks, fused self- and cross-attention). The reference's
`PegasusForConditionalGeneration.from_pretrained('google/pegasus-large')` needs the network; here the model is built
from the pegasus-large config (random init) and a local fine-tuned or HF-format state dict is loaded via `checkpoint=`
or $VCG_PEGASUS_CHECKPOINT.

`forward` returns the reference's logits [B, Ld, V]; `title_loss` is what the reference's drivers compute from them
(mean cross-entropy over the decoder positions with mask 1, and the number of correct argmaxes) without storing any
[R, V] logits; `generate` is the reference's single-text loop and `generate_ids` its batched form. Both generators run
the encoder and the cross-attention K | V projections once per source and re-run only the decoder per token (the
reference re-runs the whole model, pegasus_hugface.py:120-122).

Training goes through `title_loss`, which is differentiable (vcg_hip.pegasus.PegasusFn: the engine as one autograd node
in front of the fused vocabulary loss; dropout in train() mode only). `forward` refuses to run where a gradient would be
expected: the logits are not differentiated.
"""
import logging
import os

import numpy as np
import torch
import torch.nn as nn

from vcg_hip.nn import NativeRoot, PegasusConfig, PegasusForConditionalGeneration
from vcg_hip.optim import configure_adamw

logger = logging.getLogger(__name__)

_PREFIXES = ("module.base_model.", "base_model.")  # (a DDP-wrapped PegasusHugface's / this class's own state dict)


def _load_hf_state(model, path):
    """Load HF Pegasus keys -- bare, under "base_model." or "module.base_model.", or inside a dict with
    "model_state_dict" -- into `model` (PegasusForConditionalGeneration); anything that does not match its keys is a
    ValueError."""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(path)
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if "model_state_dict" in sd:
            sd = sd["model_state_dict"]
    for pre in _PREFIXES:
        if any(k.startswith(pre) for k in sd):
            sd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
            break
    own = model.state_dict()
    tied = model.lm_head.weight is model.model.shared.weight
    # (a file may leave out the tied aliases of `shared`, as safetensors files do, and the non-trained tables)
    optional = {"model.encoder.embed_tokens.weight", "model.decoder.embed_tokens.weight",
                "model.encoder.embed_positions.weight", "model.decoder.embed_positions.weight", "final_logits_bias"}
    if tied:
        optional.add("lm_head.weight")
    missing = sorted(k for k in own if k not in sd and k not in optional)
    unexpected = sorted(k for k in sd if k not in own)
    shapes = sorted(k for k in sd if k in own and tuple(sd[k].shape) != tuple(own[k].shape))
    if missing or unexpected or shapes:
        raise ValueError(f"{path}: not a PegasusForConditionalGeneration state dict for this config: missing "
                         f"{missing[:3]} ({len(missing)}), unexpected {unexpected[:3]} ({len(unexpected)}), shape "
                         f"mismatch {shapes[:3]} ({len(shapes)})")
    if tied:
        # one tensor, several names: they must agree, and the copy goes through `shared`
        names = [k for k in ("model.shared.weight", "model.encoder.embed_tokens.weight",
                             "model.decoder.embed_tokens.weight", "lm_head.weight") if k in sd]
        for k in names[1:]:
            if not torch.equal(sd[k], sd[names[0]]):
                raise ValueError(f"{path}: {k} differs from {names[0]} but this model ties them (reinit_head=True "
                                 "unties the head)")
    model.load_state_dict(sd, strict=False)
    model.check_supported()
    logger.info("loaded %s", path)


def no_decay(full_name, leaf_name):
    """pegasus_hugface.py:58-72: biases and every name containing "layer_norm", "bn" or "emb" take no weight decay."""
    return leaf_name.endswith("bias") or any(tag in full_name for tag in ("layer_norm", "bn", "emb"))


class PegasusHugface(NativeRoot, nn.Module):
    def __init__(self, reinit_head=False, checkpoint=None, config=None):
        super().__init__()
        self.base_model = PegasusForConditionalGeneration(config if config is not None else PegasusConfig())
        self.vocab_size = self.base_model.config.vocab_size
        self.embed_size = self.base_model.config.hidden_size
        if reinit_head:  # (pegasus_hugface.py:29-33: a fresh head, no longer tied to the embedding)
            self.base_model.lm_head = nn.Linear(self.embed_size, self.vocab_size, bias=False)
            self.base_model.lm_head.weight.data.normal_(mean=0.0, std=0.02)
        ckpt = checkpoint or os.environ.get("VCG_PEGASUS_CHECKPOINT")
        if ckpt:
            self.load_checkpoint(ckpt)
        print("number of parameters: ", sum(p.numel() for p in self.base_model.parameters()))

    def load_checkpoint(self, path):
        _load_hf_state(self.base_model, path)

    def fix_backbone(self):
        for pn, p in self.named_parameters():
            if "pooler" in pn or "head" in pn:
                continue
            p.requires_grad = False

    def configure_optimizers(self, train_config):
        return configure_adamw(self, train_config, no_decay=no_decay)

    # ------------------------------------------------------------------ forward
    def _check_inference(self):
        if self.training or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(
                f"PegasusHugface.forward: the logits [B, Ld, {self.vocab_size}] are not differentiated (call .eval() "
                "and run under torch.no_grad()); training goes through title_loss, which never stores them")

    def _check_ids(self, ids, what):
        """Token ids index the embedding table in the forward and its gradient in the backward (the scatter kernel
        writes row `id` of .grad): an id outside [0, vocab_size) -- a tokenizer with another vocabulary -- is refused
        here, on the host, before anything is launched."""
        if ids.dtype != torch.int64:
            raise ValueError(f"title_loss: {what} must be int64 token ids, not {ids.dtype}")
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.vocab_size):
            raise ValueError(f"title_loss: {what} holds a token id outside [0, {self.vocab_size})")

    def _engine(self):
        return self.base_model.engine(root=self)

    def _head_w(self, dtype):
        from vcg_hip.mlm import _head_weights
        W, Wp = _head_weights(self, self.base_model.lm_head, dtype)
        return W if Wp is None else Wp

    def _decoder_hidden(self, x, attention_mask, decoder_input_ids, decoder_attention_mask):
        if decoder_input_ids is None:
            raise ValueError("PegasusHugface.forward needs decoder_input_ids (the reference always passes them)")
        eng = self._engine()
        enc = eng.encode(x, attention_mask)
        return eng.decode(decoder_input_ids, decoder_attention_mask, attention_mask, eng.cross_kv(enc))

    def forward(self, x, attention_mask=None, decoder_input_ids=None, decoder_attention_mask=None):
        """pegasus_hugface.py:89-102: the logits [B, Ld, V], fp32."""
        self._check_inference()
        from vcg_hip import gpt_decode as gd
        hidden = self._decoder_hidden(x, attention_mask, decoder_input_ids, decoder_attention_mask)
        B, Ld = decoder_input_ids.shape
        z = gd.head_logits(hidden, self._head_w(hidden.dtype))
        return z.view(B, Ld, -1)[..., :self.vocab_size]

    def title_loss(self, x, attention_mask, decoder_input_ids, decoder_attention_mask, targets):
        """train_chapter_title_gen.py:158-169 / test_chapter_title_gen.py:170-180 without the logits: (mean
        cross-entropy over the decoder positions whose decoder_attention_mask is 1, number of those whose argmax is
        the target, their number). Only those rows are projected onto the vocabulary (csrc/mlm_head.hip). This is the
        training entry: with gradients enabled (or in train() mode, where the dropout sites are active) the engine runs
        as ONE autograd node (vcg_hip.pegasus.PegasusFn) whose output feeds MlmLossFn; loss.backward() adds every
        trainable parameter's gradient onto its .grad -- with the tied head, the embedding's and the head's onto the
        same one. In eval mode under torch.no_grad() it is the inference path. No position with mask 1: a NaN loss,
        nothing launched, every gradient left as it is."""
        from vcg_hip.mlm import MlmLossFn
        dev = x.device
        self._check_ids(x, "x")
        if decoder_input_ids is not None:
            self._check_ids(decoder_input_ids, "decoder_input_ids")
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        keep = decoder_attention_mask.detach().to("cpu").reshape(-1).numpy() != 0
        rows = np.flatnonzero(keep).astype(np.int64)
        if rows.size == 0:  # (F.cross_entropy on an empty selection; nothing is launched, no gradient is touched)
            return (torch.full((), float("nan"), device=dev, requires_grad=grad),
                    torch.zeros((), dtype=torch.int64, device=dev), 0)
        tgt = targets.detach().to("cpu", torch.int64).reshape(-1).numpy()[rows]
        if ((tgt < 0) | (tgt >= self.vocab_size)).any():
            raise ValueError(f"title_loss: a target outside [0, {self.vocab_size}) at a position with mask 1")
        rows_d, tgt_d = torch.from_numpy(rows).to(dev), torch.from_numpy(tgt.copy()).to(dev)
        if not self.training and not grad:  # the inference path, as before
            hidden = self._decoder_hidden(x, attention_mask, decoder_input_ids, decoder_attention_mask)
            with torch.no_grad():
                loss, n_correct = MlmLossFn.apply(hidden, self._anchor(dev), self, self.base_model.lm_head, rows_d,
                                                  tgt_d, None)
            return loss, n_correct, int(rows.size)
        from vcg_hip.nn import new_seed
        from vcg_hip.pegasus import PegasusFn
        if decoder_input_ids is None:
            raise ValueError("PegasusHugface.title_loss needs decoder_input_ids")
        eng = self._engine()
        seed = new_seed()
        if grad and any(p.requires_grad for p in self.base_model.model.parameters()):
            hidden = PegasusFn.apply(self._anchor(dev), eng, x, attention_mask, decoder_input_ids,
                                     decoder_attention_mask, seed)
        else:  # only the head trains (fix_backbone), or no gradient at all: nothing is saved, no engine backward
            with torch.no_grad():
                hidden, _ = eng.train_forward(x, attention_mask, decoder_input_ids, decoder_attention_mask, seed,
                                              need_grad=False)
        loss, n_correct = MlmLossFn.apply(hidden, self._anchor(dev), self, self.base_model.lm_head, rows_d, tgt_d, None)
        return loss, n_correct, int(rows.size)

    # ------------------------------------------------------------------ generation
    def _check_sampling(self, max_len, temperature, top_k):
        c = self.base_model.config
        if max_len < 1 or max_len + 1 > c.max_position_embeddings:
            raise ValueError(f"generate: max_len {max_len} outside 1..max_position_embeddings - 1")
        if not temperature > 0:
            raise ValueError("generate: temperature must be positive")
        if top_k is not None and not 1 <= int(top_k) <= self.vocab_size:
            raise ValueError(f"generate: top_k {top_k} outside 1..{self.vocab_size}")

    @torch.no_grad()
    def generate_ids(self, input_ids, attention_mask=None, max_len=30, temperature=1.0, sample=False, top_k=None,
                     generator=None):
        """Titles for a right-padded batch of chapters: input_ids, attention_mask [B, Ls] -> (tokens int64 [B, n],
        n <= max_len: row b holds its generated tokens up to and including its EOS, pad ids behind; lengths int64
        [B]). The encoder and the cross-attention K | V run once; each of the max_len steps re-runs the decoder on the
        tokens so far and draws with the fused sampler (vcg_hip.gpt_decode.sample: argmax = lowest index, or an
        inverse-CDF draw from uniforms made once by torch.rand((max_len, B), generator=generator)). Nothing is read
        back between steps: sequences that have finished keep stepping and are cut at their EOS here."""
        from vcg_hip import gpt_decode as gd
        self.eval()
        self._check_inference()
        self._check_sampling(max_len, temperature, top_k)
        c = self.base_model.config
        B = input_ids.shape[0]
        dev = input_ids.device
        eng = self._engine()
        kv = eng.cross_kv(eng.encode(input_ids, attention_mask))
        head_w = self._head_w(eng.dtype)
        u = None
        if sample:
            gdev = generator.device if generator is not None else "cpu"
            u = torch.rand((max_len, B), generator=generator, device=gdev).to(dev, torch.float32)
        dec = torch.full((B, max_len + 1), c.decoder_start_token_id, dtype=torch.int64, device=dev)
        for t in range(max_len):
            Ld = t + 1
            hidden = eng.decode(dec[:, :Ld].contiguous(), None, attention_mask, kv)
            logits = gd.head_logits(hidden.view(B, Ld, -1)[:, -1], head_w)
            gd.sample(logits, self.vocab_size, temperature, top_k or 0, not sample, None if u is None else u[t],
                      seq=dec, col_off=Ld)
        return cut_at_eos(dec[:, 1:].cpu(), c.eos_token_id, c.pad_token_id)

    @torch.no_grad()
    def generate(self, text, tokenizer, device, max_text_len=512, max_len=30, temperature=1.0, sample=False,
                 top_k=None):
        """pegasus_hugface.py:105-146: (gen_text, sentence_logits [1, 1 + 2 + ... + n, V]) for one text -- tokenised by
        tokenize + convert_tokens_to_ids (no EOS appended), cropped to max_text_len tokens; the loop stops after
        emitting EOS or max_len tokens; every step's logits of all its decoder positions are concatenated. The encoder
        runs once, not once per token."""
        self.eval()
        self._check_inference()
        self._check_sampling(max_len, temperature, top_k)
        c = self.base_model.config
        tokens = tokenizer.tokenize(text)[:max_text_len]
        ids = tokenizer.convert_tokens_to_ids(tokens)
        input_ids = torch.from_numpy(np.array(ids)).long().to(device).unsqueeze(0)
        dec = torch.full((1, max_len + 1), c.decoder_start_token_id, dtype=torch.int64, device=device)
        memory = self._encode_once(input_ids)
        sentence_ids, sentence_logits = [], []
        for t in range(max_len):
            logits = self._step_logits(memory, dec[:, :t + 1])  # [1, t + 1, V]
            sentence_logits.append(logits)
            tok = self._draw(logits[:, -1], temperature, top_k, sample)
            dec[:, t + 1] = tok
            sentence_ids.append(int(tok.item()))
            if sentence_ids[-1] == c.eos_token_id:
                break
        return tokenizer.decode(sentence_ids), torch.cat(sentence_logits, dim=1)

    # (the device steps of generate, apart so that the host logic can be tested without a GPU)
    def _encode_once(self, input_ids):
        eng = self._engine()
        return eng, eng.cross_kv(eng.encode(input_ids, None)), self._head_w(eng.dtype)

    def _step_logits(self, memory, dec_ids):
        from vcg_hip import gpt_decode as gd
        eng, kv, head_w = memory
        B, Ld = dec_ids.shape
        hidden = eng.decode(dec_ids.contiguous(), None, None, kv)
        return gd.head_logits(hidden, head_w).view(B, Ld, -1)[..., :self.vocab_size]


    def _draw(self, z, temperature, top_k, sample):
        """one token per row of the fp32 logits z [B, V]: int64 [B] (the fused sampler)"""
        from vcg_hip import gpt_decode as gd
        u = torch.rand(z.shape[0]).to(z.device, torch.float32) if sample else None
        return gd.sample(_padded_rows(z), self.vocab_size, temperature, top_k or 0, not sample, u)


def _padded_rows(z):
    """fp32 logits [B, V] -> a contiguous [B, ldz] copy with 16-byte rows for the sampler (the pad columns are not
    read)"""
    B, V = z.shape
    out = torch.zeros((B, (V + 7) // 8 * 8), dtype=torch.float32, device=z.device)
    out[:, :V] = z
    return out


def cut_at_eos(tokens, eos, pad):
    """Host side of generate_ids: tokens int64 [B, n] (CPU) -> (tokens cut behind each row's first EOS and cropped to the
    longest row, `pad` behind the cut; lengths [B], the EOS included)."""
    tokens = tokens.clone()
    B, n = tokens.shape
    is_eos = tokens == eos
    first = torch.where(is_eos.any(1), is_eos.to(torch.int64).argmax(1) + 1, torch.full((B,), n, dtype=torch.int64))
    tokens[torch.arange(n)[None, :] >= first[:, None]] = pad
    return tokens[:, :int(first.max())], first
