"""Masked-LM pre-training of the language model: the reference's `pretrain_lang_model_hugface.py`, with the MI355X
engines underneath. Its checkpoint is what the scorer driver starts BERT from
(`train_video_segment_point.py --lang_pretrain_ckpt`, reference :308,326-330).

`TrainerConfig` / `Trainer(model, tokenizer, train_dataset, test_dataset, config)` keep the reference's names, fields
and call protocol (`pretrain_lang_model_hugface.py:25-199`): `.device` set by attribute, `.train()`,
`.run_epoch(split, epoch)`, `.save_checkpoint(epoch, best_loss)` writing `<ckpt_path>/pretrain_<epoch>.pth` with the
keys epoch / best_loss / model_state_dict / optimizer_state_dict / tokens; the test split every 20 epochs and a
checkpoint whenever the test loss improved (always, without a test set); the learning rate follows the number of
attended tokens seen (`lr_multiplier`, :152-185); scalars Loss/train, Loss/test, Acc/test.

Differences:
- The step is `BertHugface.mlm_loss` (only the masked rows meet the vocabulary, csrc/mlm_head.hip) instead of logits
  over every position followed by a gather; clip + AdamW is one fused device pass (`FusedAdamW.clip_and_step`).
- A batch without any masked position (the reference's F.cross_entropy returns NaN there) is counted in the loss list
  as NaN but takes no optimiser step.
- `bert` only; the corpus paths are flags (the reference hard-codes them, :216-223). Without `--data_file` the
  driver trains on `data.synthetic_dataset`'s corpus (no network here).
"""
import argparse
import logging
import math
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

logger = logging.getLogger(__name__)


class TrainerConfig:
    model_type = "bert"
    max_epochs = 10
    block_size = 512
    batch_size = 64
    learning_rate = 3e-4
    betas = (0.9, 0.95)
    grad_norm_clip = 1.0
    weight_decay = 0.01
    lr_decay = False
    lr_decay_type = "cosine"
    warmup_tokens = 375e6
    final_tokens = 260e9
    ckpt_path = None
    num_workers = 0
    tensorboard_writer = None

    def __init__(self, **kwargs):
        for k, v in kwargs.items():
            setattr(self, k, v)


def lr_multiplier(config, tokens):
    """LR multiplier after `tokens` attended tokens (`pretrain_lang_model_hugface.py:156-179`): linear warm-up over
    warmup_tokens, then by progress towards final_tokens a cosine floored at 0.001, or the "exp" staircase
    1 / 0.1 / 0.01 / 0.001 at fifths of the progress (a progress exactly on a step edge falls to 0.001, as there)."""
    if tokens < config.warmup_tokens:
        return float(tokens) / float(max(1, config.warmup_tokens))
    progress = float(tokens - config.warmup_tokens) / float(max(1, config.final_tokens - config.warmup_tokens))
    if config.lr_decay_type == "cosine":
        return max(0.001, 0.5 * (1.0 + math.cos(math.pi * progress)))
    if config.lr_decay_type == "exp":
        th = 1 / 5
        if progress < th:
            return 1
        if th < progress < th * 2:
            return 0.1
        if th * 2 < progress < th * 3:
            return 0.01
        return 0.001
    raise RuntimeError("Unknown learning rate decay type")


class Trainer:
    def __init__(self, model, tokenizer, train_dataset, test_dataset, config):
        self.model = model
        self.tokenizer = tokenizer
        self.train_dataset = train_dataset
        self.test_dataset = test_dataset
        self.config = config
        self.device = "cuda"
        self.optimizer = None
        self.tokens = 0
        self.history = []

    def save_checkpoint(self, epoch, best_loss):
        raw = self.model.module if hasattr(self.model, "module") else self.model
        os.makedirs(self.config.ckpt_path, exist_ok=True)
        path = os.path.join(self.config.ckpt_path, f"pretrain_{epoch}.pth")
        print(f"Saving checkpoint at epoch {epoch} with loss {best_loss:.5f} to {path}")
        torch.save({"epoch": epoch, "best_loss": best_loss, "model_state_dict": raw.state_dict(),
                    "optimizer_state_dict": self.optimizer.state_dict(), "tokens": int(self.tokens)}, path)
        return path

    def train(self):
        raw = self.model.module if hasattr(self.model, "module") else self.model
        self.optimizer = raw.configure_optimizers(self.config)
        best_loss = test_loss = float("inf")
        self.tokens = 0
        for epoch in range(self.config.max_epochs):
            self.run_epoch("train", epoch)
            if self.test_dataset is not None and epoch % 20 == 0:
                test_loss = self.run_epoch("test", epoch)
            good = self.test_dataset is None or test_loss < best_loss
            if self.config.ckpt_path is not None and good:
                best_loss = test_loss
                self.save_checkpoint(epoch, best_loss)
        return best_loss

    def step_loss(self, x, attention_mask, y):
        """(loss, n_correct, n_valid) of one batch (the generative stage's trainer states its own)."""
        return self.model.mlm_loss(x, attention_mask, y)

    def run_epoch(self, split, epoch):
        is_train = split == "train"
        self.model.train(is_train)
        data = self.train_dataset if is_train else self.test_dataset
        loader = torch.utils.data.DataLoader(data, shuffle=True, pin_memory=True, batch_size=self.config.batch_size,
                                             num_workers=self.config.num_workers)
        w = self.config.tensorboard_writer
        losses, accs = [], []
        for it, (x, y, attention_mask) in enumerate(loader):
            n_tokens = int((attention_mask > 0).sum())
            x = x.to(self.device)
            attention_mask = attention_mask.to(self.device)
            with torch.set_grad_enabled(is_train):
                loss, n_correct, n_valid = self.step_loss(x, attention_mask, y)
            if is_train and n_valid:
                self.model.zero_grad()
                loss.backward()
                self.optimizer.clip_and_step(self.config.grad_norm_clip)
            loss_v = loss.item()
            losses.append(loss_v)
            if n_valid:
                accs.append(int(n_correct) / n_valid)
            if is_train:
                lr = self.config.learning_rate
                if self.config.lr_decay:
                    self.tokens += n_tokens
                    lr = self.config.learning_rate * lr_multiplier(self.config, self.tokens)
                    for g in self.optimizer.param_groups:
                        g["lr"] = lr
                self.history.append({"epoch": epoch, "it": it, "loss": loss_v, "lr": lr, "tokens": self.tokens})
                if w is not None:
                    w.add_scalar("Loss/train", loss_v, epoch * len(loader) + it)
        if is_train:
            logger.info("epoch %d: train loss %.5f", epoch + 1, float(np.mean(losses)) if losses else float("nan"))
            return None
        test_loss = float(np.mean(losses))
        test_acc = float(np.mean(accs)) if accs else float("nan")
        print("test loss: %f, acc: %f" % (test_loss, test_acc))
        if w is not None:
            w.add_scalar("Loss/test", test_loss, epoch)
            w.add_scalar("Acc/test", test_acc, epoch)
        return test_loss


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="pretrain language model (MI355X)")
    p.add_argument("--gpu", default=0, type=int)
    p.add_argument("--model_type", default="bert", type=str)
    p.add_argument("--epoch", default=3001, type=int)
    p.add_argument("--batch_size", default=64, type=int)
    p.add_argument("--lr_decay_type", default="cosine", type=str)
    p.add_argument("--max_text_len", default=50, type=int)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--seed", default=123, type=int)
    p.add_argument("--ckpt_path", default=None, help="directory of pretrain_<epoch>.pth (none: no checkpoint)")
    p.add_argument("--vocab_file", default=None, help="BERT WordPiece vocab.txt (bert-base-uncased's)")
    p.add_argument("--videos", default=8, type=int, help="synthetic corpus size (no --data_file)")
    # the reference's on-disk corpus (its hard-coded paths, :216-223)
    p.add_argument("--data_file", default=None)
    p.add_argument("--vid_file", default=None, help="the training split's vid list")
    p.add_argument("--test_vid_file", default=None, help="the validation split's vid list")
    p.add_argument("--subtitle_dir", default=None)
    p.add_argument("--num_workers", default=0, type=int)
    p.add_argument("--tensorboard_log", default=None)
    args = p.parse_args(argv)
    if args.model_type != "bert":
        p.error(f"--model_type {args.model_type}: only 'bert' (masked-LM pre-training) is built; GPT is out of scope")
    if args.lr_decay_type not in ("cosine", "exp"):
        p.error(f"--lr_decay_type {args.lr_decay_type}: cosine or exp")
    if bool(args.data_file) != bool(args.vid_file):
        p.error("--data_file and --vid_file go together")
    return args


def datasets(args, tok):
    from data.youtube_subtitle_dataset import (SyntheticSubtitleDatasetForHugFace,
                                               YoutubeClipSubtitleDatasetForHugFace)
    if args.data_file:
        mk = lambda vf: YoutubeClipSubtitleDatasetForHugFace(  # noqa: E731
            args.data_file, vf, args.model_type, tok, clip_frame_num=16, max_text_len=args.max_text_len,
            subtitle_dir=args.subtitle_dir)
        return mk(args.vid_file), (mk(args.test_vid_file) if args.test_vid_file else None)
    from data.synthetic_dataset import SyntheticVideoCorpus
    mk = lambda n, seed: SyntheticSubtitleDatasetForHugFace(  # noqa: E731
        SyntheticVideoCorpus(n, H=8, W=8, seed=seed), args.model_type, tok, 16, args.max_text_len)
    return mk(args.videos, args.seed), mk(max(2, args.videos // 4), args.seed + 1)


def main(argv=None):
    args = parse_args(argv)
    from common_utils import set_random_seed
    from train_video_segment_point import make_tokenizer
    from vcg_hip import synth
    from vcg_hip.build import build_mlm_model
    from vcg_hip.nn import check_max_text_len

    set_random_seed.use_fix_random_seed(args.seed)
    model = build_mlm_model(precision=args.precision)  # (on the CPU until the arguments are checked)
    check_max_text_len(model, args.max_text_len)
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    model = model.to(device)
    synth.init_params(model, args.seed)  # (on the GPU: the HIP generator)
    tok = make_tokenizer(args.vocab_file)
    train_ds, test_ds = datasets(args, tok)
    writer = None
    if args.tensorboard_log:
        from common_utils.scalar_log import summary_writer
        writer = summary_writer(args.tensorboard_log)
    L = args.max_text_len
    conf = TrainerConfig(model_type=args.model_type, max_epochs=args.epoch, batch_size=args.batch_size,
                         learning_rate=1e-4, block_size=L, lr_decay_type=args.lr_decay_type, lr_decay=True,
                         warmup_tokens=args.epoch // 100 * len(train_ds) * L,
                         final_tokens=args.epoch // 10 * 9 * len(train_ds) * L, num_workers=args.num_workers,
                         ckpt_path=args.ckpt_path, tensorboard_writer=writer)
    trainer = Trainer(model, tok, train_ds, test_ds, conf)
    trainer.device = device
    trainer.train()
    return trainer


if __name__ == "__main__":
    main()
