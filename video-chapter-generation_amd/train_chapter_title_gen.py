"""Drop-in for reference train_chapter_title_gen.py: fine-tune Pegasus on chapter titles (stage 2), on the MI355X engines.

`TrainerConfig` and `Trainer` keep the reference's fields and protocol: `train()` runs epochs start_epoch + 1 ..
max_epochs, the test split every 20 epochs, and writes `checkpoint_{epoch}_{best_result:.4f}.pth` (epoch, best_result,
model_state_dict, optimizer_state_dict) plus the `checkpoint_best.pth` link to it whenever the test accuracy improved
(without a test split: after every epoch); the learning rate is set after every step from the EPOCH -- linear warm-up
over warmup_epochs (floor 1e-2), then cosine (floor 1e-3) or the stepped "exp" decay over final_epochs
(`lr_multiplier`). Scalars Train/loss, Train/acc, Test/loss, Test/acc.

What differs:
  * the step is `PegasusHugface.title_loss` -- the masked mean cross-entropy and the accuracy without any [R, V]
    logits, differentiable through the native engine -- and clip + AdamW is one fused pass
    (`FusedAdamW.clip_and_step(grad_norm_clip)`), as in train_lang/pretrain_gpt_lang_model.py;
  * single GPU (the reference wraps the model in DataParallel over two);
  * nothing is fetched: `--pegasus_ckpt` (or $VCG_PEGASUS_CHECKPOINT) names a local pegasus-large state dict loaded
    before the head is re-initialised (reinit_head=True, the reference's setting), `--tokenizer` a local
    transformers.PegasusTokenizer directory; without it data.synthetic_dataset.HashPegasusTokenizer stands in. The
    data arguments are the reference's hard-coded paths made options.
The saved checkpoint loads through `PegasusHugface(checkpoint=...)`.
"""
import argparse
import logging
import math
import os
import sys

import numpy as np
import torch
from torch.utils.data import DataLoader

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

logger = logging.getLogger(__name__)


class TrainerConfig:
    # optimization parameters
    max_epochs = 10
    start_epoch = 0
    best_result = float("-inf")
    block_size = 512
    batch_size = 64
    learning_rate = 3e-4
    betas = (0.9, 0.95)
    grad_norm_clip = 1.0
    weight_decay = 0.01  # only applied on matmul weights
    # learning rate decay: linear warm-up, then cosine or stepped decay
    lr_decay = False
    lr_decay_type = "cosine"
    warmup_epochs = 30
    final_epochs = 2700
    # checkpoint settings
    ckpt_dir = None
    num_workers = 0  # for DataLoader
    tensorboard_writer = None

    def __init__(self, **kwargs):
        for k, v in kwargs.items():
            setattr(self, k, v)


def lr_multiplier(config, epoch):
    """train_chapter_title_gen.py:190-216: the factor on learning_rate in `epoch`."""
    if epoch < config.warmup_epochs:
        return max(epoch / config.warmup_epochs, 1e-2)
    progress = epoch / config.final_epochs if epoch < config.final_epochs else 1.0
    if config.lr_decay_type == "cosine":
        return max(0.001, 0.5 * (1.0 + math.cos(math.pi * progress)))
    if config.lr_decay_type == "exp":
        t = 1 / 5
        if progress < t:
            return 1
        if t < progress < 2 * t:
            return 0.1
        if 2 * t < progress < 3 * t:
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
        self.device = None
        self.optimizer = None
        self.history = []  # one record per epoch and split: split, epoch, loss, acc, lr

    def checkpoint_path(self, epoch, best_result):
        return os.path.join(self.config.ckpt_dir, f"checkpoint_{epoch}_{best_result:.4f}.pth")

    def save_checkpoint(self, epoch, best_result):
        os.makedirs(self.config.ckpt_dir, exist_ok=True)
        path = self.checkpoint_path(epoch, best_result)
        logger.info("saving checkpoint to %s", path)
        torch.save({"epoch": epoch, "best_result": best_result, "model_state_dict": self.model.state_dict(),
                    "optimizer_state_dict": self.optimizer.state_dict()}, path)
        link = os.path.join(self.config.ckpt_dir, "checkpoint_best.pth")
        if os.path.lexists(link):
            os.remove(link)
        os.symlink(os.path.abspath(path), link)
        return path

    def train(self):
        c = self.config
        self.optimizer = self.model.configure_optimizers(c)
        best_result = c.best_result
        test_result = float("-inf")
        for epoch in range(c.start_epoch + 1, c.max_epochs + 1):
            self.run_epoch("train", epoch)
            if self.test_dataset is not None and epoch % 20 == 0:
                test_result = self.run_epoch("test", epoch)
            # early stopping on the test accuracy, or always if there is no test split
            if c.ckpt_dir is not None and (self.test_dataset is None or test_result > best_result):
                best_result = test_result
                self.save_checkpoint(epoch, best_result)

    def step(self, batch, is_train):
        """One batch on the device -> (loss, number correct, number of valid positions) as Python numbers; the train
        split's also clips and steps."""
        x, mask, dec, dmask, tgt = (t.to(self.device, non_blocking=True) for t in batch)
        with torch.set_grad_enabled(is_train):
            loss, n_correct, n_valid = self.model.title_loss(x, mask, dec, dmask, tgt)
        if is_train and n_valid > 0:
            self.model.zero_grad()
            loss.backward()
            self.optimizer.clip_and_step(self.config.grad_norm_clip)
        return float(loss.item()), int(n_correct.item()), n_valid

    def run_epoch(self, split, epoch):
        c = self.config
        is_train = split == "train"
        self.model.train(is_train)
        data = self.train_dataset if is_train else self.test_dataset
        loader = DataLoader(data, shuffle=True, pin_memory=True, batch_size=c.batch_size, num_workers=c.num_workers)
        losses, accs = [], []
        lr = c.learning_rate
        for it, batch in enumerate(loader):
            loss, correct, count = self.step(batch, is_train)
            acc = correct / count if count else float("nan")
            losses.append(loss)
            accs.append(acc)
            if not is_train:
                continue
            lr = c.learning_rate * lr_multiplier(c, epoch) if c.lr_decay else c.learning_rate
            if c.lr_decay:
                for group in self.optimizer.param_groups:
                    group["lr"] = lr
            if c.tensorboard_writer is not None:
                n_iter = epoch * len(loader) + it
                c.tensorboard_writer.add_scalar("Train/loss", loss, n_iter)
                c.tensorboard_writer.add_scalar("Train/acc", acc, n_iter)
            logger.info("epoch %d iter %d: train loss %.5f, acc %.5f. lr %e", epoch, it, loss, acc, lr)
        mean_loss, mean_acc = float(np.mean(losses)), float(np.mean(accs))
        self.history.append(dict(split=split, epoch=epoch, loss=mean_loss, acc=mean_acc, lr=lr))
        if not is_train:
            print("test loss: %f, acc %f" % (mean_loss, mean_acc))
            if c.tensorboard_writer is not None:
                c.tensorboard_writer.add_scalar("Test/loss", mean_loss, epoch)
                c.tensorboard_writer.add_scalar("Test/acc", mean_acc, epoch)
        return mean_acc


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="video chapter title generation model (MI355X)")
    p.add_argument("--gpu", default=0, type=int)
    p.add_argument("--epoch", default=3000, type=int)
    p.add_argument("--batch_size", default=4, type=int)
    p.add_argument("--lr_decay_type", default="cosine", type=str)
    p.add_argument("--model_type", default="pegasus", type=str)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--seed", default=123, type=int)
    p.add_argument("--pegasus_ckpt", default=None, help="a local pegasus-large state dict (or $VCG_PEGASUS_CHECKPOINT)")
    p.add_argument("--tokenizer", default=None, help="a local transformers.PegasusTokenizer directory")
    p.add_argument("--ckpt_dir", default=None, help="default: ./checkpoint/chapter_title_gen/<model>_text_batch_<B>")
    p.add_argument("--data_file", default="./dataset/all_in_one_with_subtitle_final.csv")
    p.add_argument("--subtitle_dir", default="../video_chapter_youtube_dataset/dataset")
    p.add_argument("--train_vid_file", default="./dataset/final_train.txt")
    p.add_argument("--test_vid_file", default="./dataset/final_validation.txt")
    p.add_argument("--max_text_len", default=512, type=int)
    p.add_argument("--chapter_title_text_len", default=30, type=int)
    p.add_argument("--num_workers", default=16, type=int)
    args = p.parse_args(argv)
    if args.model_type != "pegasus":
        p.error(f"--model_type {args.model_type}: only pegasus is native (the BigBird title model is not ported)")
    if args.lr_decay_type not in ("cosine", "exp"):
        p.error(f"--lr_decay_type {args.lr_decay_type}: cosine or exp")
    return args


def make_tokenizer(path, vocab_size):
    if path:
        from transformers import PegasusTokenizer
        return PegasusTokenizer.from_pretrained(path, local_files_only=True)
    from data.synthetic_dataset import HashPegasusTokenizer
    return HashPegasusTokenizer(vocab_size)


def main(argv=None):
    args = parse_args(argv)
    from common_utils import set_random_seed
    from common_utils.scalar_log import summary_writer
    from data.youtube_chapter_title_dataset import YoutubeChapterTitleDataset
    from model.lang import pegasus_hugface

    ckpt_dir = args.ckpt_dir or f"./checkpoint/chapter_title_gen/{args.model_type}_text_batch_{args.batch_size}"
    set_random_seed.use_fix_random_seed(args.seed)
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    model = pegasus_hugface.PegasusHugface(reinit_head=True, checkpoint=args.pegasus_ckpt)
    model.base_model.check_text_len(args.max_text_len, "source")
    model.base_model.check_text_len(args.chapter_title_text_len, "decoder")
    model = model.to(device)
    model.precision = args.precision
    tok = make_tokenizer(args.tokenizer, model.vocab_size)
    mk = lambda vid_file: YoutubeChapterTitleDataset(  # noqa: E731
        args.data_file, vid_file, tok, args.max_text_len, args.chapter_title_text_len, subtitle_dir=args.subtitle_dir)
    train_ds, test_ds = mk(args.train_vid_file), mk(args.test_vid_file)
    conf = TrainerConfig(max_epochs=args.epoch, start_epoch=0, best_result=float("-inf"), batch_size=args.batch_size,
                         learning_rate=1e-5, block_size=args.max_text_len, lr_decay_type=args.lr_decay_type,
                         lr_decay=True, warmup_epochs=args.epoch // 100, final_epochs=args.epoch // 100 * 90,
                         num_workers=args.num_workers, ckpt_dir=ckpt_dir, tensorboard_writer=summary_writer(ckpt_dir))
    trainer = Trainer(model, tok, train_ds, test_ds, conf)
    trainer.device = device
    trainer.train()
    return trainer


if __name__ == "__main__":
    main()
