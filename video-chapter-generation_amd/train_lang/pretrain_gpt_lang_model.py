"""Generative (GPT) pre-training of the language model: the `gpt` path of the reference's
`pretrain_lang_model_hugface.py` (its default `model_type`, :27, :232-234), with the MI355X engines underneath.

`pretrain_lang_model_hugface.py --model_type gpt` and `YoutubeClipSubtitleDatasetForHugFace(..., "gpt", ...)` keep
refusing (INTEGRATION.md says why); this driver is the stage's entry point, next to the contrastive and listwise ones.

`TrainerConfig` / `Trainer` are the masked-LM driver's (same fields and call protocol, checkpoints
`<ckpt_path>/pretrain_<epoch>.pth` with epoch / best_loss / model_state_dict / optimizer_state_dict / tokens, the test
split every 20 epochs, the token-driven learning rate, scalars Loss/train, Loss/test, Acc/test); only the step differs:

- The step is `GPTHugface.lm_loss` (causal fused attention, csrc/bert_attn*.hip; only the positions with a target meet
  the vocabulary, csrc/mlm_head.hip) instead of logits over every position followed by a gather; clip + AdamW is one
  fused device pass (`FusedAdamW.clip_and_step`).
- Single GPU. Without `--data_file` the driver trains on `data.synthetic_dataset`'s corpus. `--vocab_file` and
  `--merges_file` select a local transformers.OpenAIGPTTokenizer; without them a deterministic stub tokenizer with ids
  in [0, V) stands in (data.synthetic_dataset.HashGPTTokenizer). `--checkpoint` (or $VCG_GPT_CHECKPOINT) loads a local
  HF openai-gpt state dict into the decoder after the seeded init; token ids are checked against V in the dataset.
"""
import argparse
import logging
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import pretrain_lang_model_hugface as _mlm  # noqa: E402  (the same trainer, schedule and checkpoint format)
from pretrain_lang_model_hugface import lr_multiplier  # noqa: E402,F401

logger = logging.getLogger(__name__)


class TrainerConfig(_mlm.TrainerConfig):
    model_type = "gpt"


class Trainer(_mlm.Trainer):
    def step_loss(self, x, attention_mask, y):
        return self.model.lm_loss(x, attention_mask, y)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="generative (GPT) pre-training of the language model (MI355X)")
    p.add_argument("--gpu", default=0, type=int)
    p.add_argument("--epoch", default=3001, type=int)
    p.add_argument("--batch_size", default=64, type=int)
    p.add_argument("--lr_decay_type", default="cosine", type=str)
    p.add_argument("--max_text_len", default=50, type=int)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--seed", default=123, type=int)
    p.add_argument("--n_layer", default=12, type=int, help="decoder blocks (12: openai-gpt)")
    p.add_argument("--dropout", default=None, type=float, help="every dropout rate (default: the config's 0.1)")
    p.add_argument("--learning_rate", default=1e-4, type=float)
    p.add_argument("--checkpoint", default=None, help="a local HF openai-gpt state dict for the decoder")
    p.add_argument("--ckpt_path", default=None, help="directory of pretrain_<epoch>.pth (none: no checkpoint)")
    p.add_argument("--vocab_file", default=None, help="openai-gpt's vocab.json")
    p.add_argument("--merges_file", default=None, help="openai-gpt's merges.txt")
    p.add_argument("--videos", default=8, type=int, help="synthetic corpus size (no --data_file)")
    p.add_argument("--data_file", default=None)
    p.add_argument("--vid_file", default=None, help="the training split's vid list")
    p.add_argument("--test_vid_file", default=None, help="the validation split's vid list")
    p.add_argument("--subtitle_dir", default=None)
    p.add_argument("--num_workers", default=0, type=int)
    p.add_argument("--tensorboard_log", default=None)
    args = p.parse_args(argv)
    if args.lr_decay_type not in ("cosine", "exp"):
        p.error(f"--lr_decay_type {args.lr_decay_type}: cosine or exp")
    if bool(args.data_file) != bool(args.vid_file):
        p.error("--data_file and --vid_file go together")
    if bool(args.vocab_file) != bool(args.merges_file):
        p.error("--vocab_file and --merges_file go together")
    if args.n_layer < 1:
        p.error("--n_layer must be at least 1")
    if args.dropout is not None and not 0.0 <= args.dropout < 1.0:
        p.error("--dropout must be in [0, 1)")
    return args


def make_tokenizer(vocab_file, merges_file, vocab_size):
    if vocab_file:
        from transformers import OpenAIGPTTokenizer
        return OpenAIGPTTokenizer(vocab_file=vocab_file, merges_file=merges_file)
    from data.synthetic_dataset import HashGPTTokenizer
    return HashGPTTokenizer(vocab_size)


def datasets(args, tok, vocab_size):
    from data.youtube_subtitle_dataset import SyntheticSubtitleDatasetForGPT, YoutubeClipSubtitleDatasetForGPT
    if args.data_file:
        mk = lambda vf: YoutubeClipSubtitleDatasetForGPT(  # noqa: E731
            args.data_file, vf, tok, clip_frame_num=16, max_text_len=args.max_text_len, subtitle_dir=args.subtitle_dir,
            vocab_size=vocab_size)
        return mk(args.vid_file), (mk(args.test_vid_file) if args.test_vid_file else None)
    from data.synthetic_dataset import SyntheticVideoCorpus
    mk = lambda n, seed: SyntheticSubtitleDatasetForGPT(  # noqa: E731
        SyntheticVideoCorpus(n, H=8, W=8, seed=seed), tok, 16, args.max_text_len, vocab_size=vocab_size)
    return mk(args.videos, args.seed), mk(max(2, args.videos // 4), args.seed + 1)


def main(argv=None):
    args = parse_args(argv)
    from common_utils import set_random_seed
    from vcg_hip import synth
    from vcg_hip.build import build_gpt_model
    from vcg_hip.nn import OpenAIGPTConfig, check_max_text_len

    set_random_seed.use_fix_random_seed(args.seed)
    model = build_gpt_model(precision=args.precision, dropout=args.dropout,
                            config=OpenAIGPTConfig(n_layer=args.n_layer))  # (on the CPU until the arguments are checked)
    check_max_text_len(model, args.max_text_len)
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    model = model.to(device)
    synth.init_params(model, args.seed)  # (on the GPU: the HIP generator)
    ckpt = args.checkpoint or os.environ.get("VCG_GPT_CHECKPOINT")
    if ckpt:  # (after the seeded init, which covers every parameter)
        model.load_checkpoint(ckpt)
    tok = make_tokenizer(args.vocab_file, args.merges_file, model.vocab_size)
    train_ds, test_ds = datasets(args, tok, model.vocab_size)
    writer = None
    if args.tensorboard_log:
        from common_utils.scalar_log import summary_writer
        writer = summary_writer(args.tensorboard_log)
    L = args.max_text_len
    conf = TrainerConfig(max_epochs=args.epoch, batch_size=args.batch_size, learning_rate=args.learning_rate,
                         block_size=L, lr_decay_type=args.lr_decay_type, lr_decay=True,
                         warmup_tokens=args.epoch // 100 * len(train_ds) * L,
                         final_tokens=args.epoch // 10 * 9 * len(train_ds) * L, num_workers=args.num_workers,
                         ckpt_path=args.ckpt_path, tensorboard_writer=writer)
    trainer = Trainer(model, tok, train_ds, test_ds, conf)
    trainer.device = device
    trainer.train()
    return trainer


if __name__ == "__main__":
    main()
