"""Shot-contrastive (MoCo) pre-training of the language model: the reference's
`train_lang/pretrain_constrast_lang_model.py`, with the MI355X engines underneath. Its checkpoint is what the scorer
driver can start BERT from (`train_video_segment_point.py --lang_contrast_ckpt`).

`TrainerConfig` / `Trainer(model, tokenizer, train_dataset, test_dataset, config)` keep the reference's names, fields
and call protocol (:26-178): `.device` set by attribute, `.train()`, `.run_epoch(split, epoch)`, `.save_checkpoint()`
writing the bare `state_dict()` to `ckpt_path`; loaders with drop_last=True; the test split every 20 epochs and a
checkpoint whenever the test loss improved (always, without a test set); the learning rate follows the number of
attended query tokens seen (`lr_multiplier`, :131-162); scalars Train/loss, Train/acc, Test/loss, Test/acc.

Differences:
- The step is `BertHugfaceConstrast.contrast_loss` (fused InfoNCE, csrc/contrast.hip) instead of N x (1 + K) logits
  followed by F.cross_entropy and a top-1; clip + AdamW is one fused device pass (`FusedAdamW.clip_and_step`).
- Paths are flags (the reference hard-codes them, :192-195). Without `--data_file` the driver trains on
  `data.synthetic_dataset`'s corpus. `--lang_pretrain_ckpt` starts both encoders from the masked-LM stage's checkpoint.
- Single GPU, as the reference's driver is.
"""
import argparse
import logging
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from pretrain_lang_model_hugface import lr_multiplier  # noqa: E402  (the same token-driven schedule)

logger = logging.getLogger(__name__)


class TrainerConfig:
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

    def save_checkpoint(self):
        raw = self.model.module if hasattr(self.model, "module") else self.model
        d = os.path.dirname(self.config.ckpt_path)
        if d:
            os.makedirs(d, exist_ok=True)
        print("saving %s" % self.config.ckpt_path)
        torch.save(raw.state_dict(), self.config.ckpt_path)

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
                self.save_checkpoint()
        return best_loss

    def run_epoch(self, split, epoch):
        is_train = split == "train"
        self.model.train(is_train)
        data = self.train_dataset if is_train else self.test_dataset
        loader = torch.utils.data.DataLoader(data, shuffle=True, pin_memory=True, batch_size=self.config.batch_size,
                                             num_workers=self.config.num_workers, drop_last=True)
        w = self.config.tensorboard_writer
        losses, accs = [], []
        for it, (q_ids, q_mask, c_ids, c_mask) in enumerate(loader):
            n_tokens = int((q_mask > 0).sum())
            q_ids, q_mask = q_ids.to(self.device), q_mask.to(self.device)
            c_ids, c_mask = c_ids.to(self.device), c_mask.to(self.device)
            with torch.set_grad_enabled(is_train):
                loss, n_correct, n = self.model.contrast_loss(q_ids, q_mask, c_ids, c_mask, device=self.device)
            if is_train:
                self.model.zero_grad()
                loss.backward()
                self.optimizer.clip_and_step(self.config.grad_norm_clip)
            loss_v = loss.item()
            acc = int(n_correct) / n
            losses.append(loss_v)
            accs.append(acc)
            if is_train:
                lr = self.config.learning_rate
                if self.config.lr_decay:
                    self.tokens += n_tokens
                    lr = self.config.learning_rate * lr_multiplier(self.config, self.tokens)
                    for g in self.optimizer.param_groups:
                        g["lr"] = lr
                n_iter = epoch * len(loader) + it
                self.history.append({"epoch": epoch, "it": it, "loss": loss_v, "acc": acc, "lr": lr,
                                     "tokens": self.tokens})
                if w is not None:
                    w.add_scalar("Train/loss", loss_v, n_iter)
                    w.add_scalar("Train/acc", acc, n_iter)
        if is_train:
            logger.info("epoch %d: train loss %.5f", epoch + 1, float(np.mean(losses)) if losses else float("nan"))
            return None
        test_loss = float(np.mean(losses))
        test_acc = float(np.mean(accs))
        print("test loss: %f, acc %f" % (test_loss, test_acc))
        if w is not None:
            w.add_scalar("Test/loss", test_loss, epoch)
            w.add_scalar("Test/acc", test_acc, epoch)
        return test_loss


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="contrastive pre-training of the language model (MI355X)")
    p.add_argument("--gpu", default=0, type=int)
    p.add_argument("--epoch", default=3000, type=int)
    p.add_argument("--batch_size", default=64, type=int)
    p.add_argument("--lr_decay_type", default="cosine", type=str)
    p.add_argument("--clip_frame_num", default=10, type=int)
    p.add_argument("--max_text_len", default=50, type=int)
    p.add_argument("--neighbor_size", default=3, type=int, help="candidate clips on each side of the query clip")
    p.add_argument("--queue_size", default=65536, type=int, help="K, a multiple of --batch_size")
    p.add_argument("--momentum", default=0.999, type=float)
    p.add_argument("--temperature", default=0.07, type=float)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--seed", default=123, type=int)
    p.add_argument("--ckpt_path", default=None, help="file the state dict is saved to (none: no checkpoint)")
    p.add_argument("--lang_pretrain_ckpt", default=None,
                   help="pretrain_lang_model_hugface.py checkpoint both encoders start from")
    p.add_argument("--vocab_file", default=None, help="BERT WordPiece vocab.txt (bert-base-uncased's)")
    p.add_argument("--videos", default=8, type=int, help="synthetic corpus size (no --data_file)")
    p.add_argument("--data_file", default=None)
    p.add_argument("--vid_file", default=None, help="the training split's vid list")
    p.add_argument("--test_vid_file", default=None, help="the test split's vid list")
    p.add_argument("--subtitle_dir", default=None)
    p.add_argument("--num_workers", default=0, type=int)
    p.add_argument("--tensorboard_log", default=None)
    args = p.parse_args(argv)
    if args.lr_decay_type not in ("cosine", "exp"):
        p.error(f"--lr_decay_type {args.lr_decay_type}: cosine or exp")
    if bool(args.data_file) != bool(args.vid_file):
        p.error("--data_file and --vid_file go together")
    if args.batch_size <= 0 or args.queue_size % args.batch_size != 0:
        p.error(f"--queue_size {args.queue_size} must be a multiple of --batch_size {args.batch_size}")
    return args


def datasets(args, tok):
    from data.youtube_subtitle_dataset import (SyntheticClipConstrastSubtitleDataset,
                                               YoutubeClipConstrastSubtitleDataset)
    T, L, nb = args.clip_frame_num, args.max_text_len, args.neighbor_size
    if args.data_file:
        mk = lambda vf: YoutubeClipConstrastSubtitleDataset(  # noqa: E731
            args.data_file, vf, tok, T, L, nb, subtitle_dir=args.subtitle_dir)
        return mk(args.vid_file), (mk(args.test_vid_file) if args.test_vid_file else None)
    from data.synthetic_dataset import SyntheticVideoCorpus
    n_test = max(args.batch_size, args.videos // 4)  # (drop_last: a split smaller than a batch yields nothing)
    mk = lambda n, seed: SyntheticClipConstrastSubtitleDataset(  # noqa: E731
        SyntheticVideoCorpus(n, min_len=(2 * nb + 2) * T, max_len=max(200, (2 * nb + 4) * T), H=8, W=8, seed=seed),
        tok, T, L, nb)
    return mk(max(args.videos, args.batch_size), args.seed), mk(n_test, args.seed + 1)


def load_encoders_from_mlm(model, path):
    """Both encoders start from the masked-LM stage's base_model.* (the reference starts both from the same pretrained
    weights)."""
    from vcg_hip.build import load_lang_pretrain
    load_lang_pretrain(model.encoder_q, path)
    model.encoder_k.load_state_dict(model.encoder_q.state_dict())


def main(argv=None):
    args = parse_args(argv)
    from common_utils import set_random_seed
    from train_video_segment_point import make_tokenizer
    from vcg_hip import synth
    from vcg_hip.build import build_contrast_model
    from vcg_hip.nn import check_max_text_len

    set_random_seed.use_fix_random_seed(args.seed)
    model = build_contrast_model(precision=args.precision, K=args.queue_size, m=args.momentum, T=args.temperature)
    check_max_text_len(model, args.max_text_len)  # (on the CPU until the arguments are checked)
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    model = model.to(device)
    synth.init_params(model.encoder_q, args.seed, prefix="encoder_q.")  # (on the GPU: the HIP generator)
    model.encoder_k.load_state_dict(model.encoder_q.state_dict())
    if args.lang_pretrain_ckpt:
        load_encoders_from_mlm(model, args.lang_pretrain_ckpt)
    tok = make_tokenizer(args.vocab_file)
    train_ds, test_ds = datasets(args, tok)
    writer = None
    if args.tensorboard_log:
        from common_utils.scalar_log import summary_writer
        writer = summary_writer(args.tensorboard_log)
    L = args.max_text_len
    conf = TrainerConfig(max_epochs=args.epoch, batch_size=args.batch_size, learning_rate=1e-4, block_size=L,
                         lr_decay_type=args.lr_decay_type, lr_decay=True,
                         warmup_tokens=args.epoch // 100 * len(train_ds) * L // 2,
                         final_tokens=args.epoch // 5 * 4 * len(train_ds) * L // 2, num_workers=args.num_workers,
                         ckpt_path=args.ckpt_path, tensorboard_writer=writer)
    trainer = Trainer(model, tok, train_ds, test_ds, conf)
    trainer.device = device
    trainer.train()
    return trainer


if __name__ == "__main__":
    main()
