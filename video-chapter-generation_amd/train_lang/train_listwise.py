"""Listwise (ListNet) fine-tuning of the language model: the reference's `train_lang/train_listwise.py`, with the
MI355X engines underneath. Its checkpoint is what the scorer driver can start BERT from
(`train_video_segment_point.py --lang_listnet_ckpt`).

`TrainerConfig` / `Trainer(model, tokenizer, train_dataset, test_dataset, config)` keep the reference's names, fields
and call protocol (:29-243): `.device` set by attribute, `.train()`, `.run_epoch(split, epoch, dataset)`,
`.save_checkpoint()` writing the bare `state_dict()` to `ckpt_path`; one shuffled pass over the slates per epoch; every
5 epochs the test pass over EVERY video of test_dataset["infer_test"] (`manual_choose_vid`, one loader per video) and
the mean of the videos' mAP; a checkpoint whenever that improved (always, without a test set); the epoch-driven
warm-up with cosine / exp decay (:186-216, `train_video_segment_point.lr_multiplier`: the same rule); scalars
Train/loss, Train/auc, Train/m_ap, <split>/loss, <split>/auc, <split>/m_ap.

Differences:
- The step is `BertHugface.train_forward` on the fused slate loss (csrc/listnet.hip) and clip + AdamW is one fused
  device pass (`FusedAdamW.clip_and_step`).
- The balanced selection (:144-152) is `balance_selection(batch_size, slate_length)`: the same `random.randint` draws
  in the same order, so a seeded run picks the reference's rows. It stays on the host, where the rows are checked.
- Paths are flags (the reference hard-codes them, :256-261). Without `--data_file` the driver trains on
  `data.synthetic_dataset`'s corpus. `--pretrained_ckpt` takes the masked-LM stage's checkpoint (:277),
  `--lang_contrast_ckpt` the contrastive stage's through `load_constrast_checkpoint` (:278).
- A video whose labels are all of one class has no AUC / mAP (sklearn raises in the reference); it counts as 0.
- Single GPU, as the reference's driver is.
"""
import argparse
import logging
import os
import sys
from random import randint

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from train_video_segment_point import _binary_auc_map, lr_multiplier  # noqa: E402  (the same epoch-driven schedule)

logger = logging.getLogger(__name__)


class TrainerConfig:
    data_mode = "text"
    model_type = "gpt"
    max_epochs = 10
    block_size = 512
    batch_size = 64
    learning_rate = 3e-4
    betas = (0.9, 0.95)
    grad_norm_clip = 1.0
    weight_decay = 0.01
    lr_decay = False
    lr_decay_type = "cosine"
    warmup_epochs = 200
    final_epochs = 2500
    ckpt_path = None
    num_workers = 0
    tensorboard_writer = None

    def __init__(self, **kwargs):
        for k, v in kwargs.items():
            setattr(self, k, v)


def balance_selection(batch_size, slate_length):
    """:144-152 -- the boundary head's rows of the [B S, H] pooled output and their labels: one of the two positive
    clips of each slate in the first half of the batch, one of the negatives of each slate in the second half. Host
    lists; the draws are the reference's, in its order."""
    pos_num = batch_size // 2
    indices = []
    for ix in range(batch_size):
        lo, hi = (0, 1) if ix < pos_num else (2, slate_length - 1)
        indices.append(slate_length * ix + randint(lo, hi))
    labels = [1] * pos_num + [0] * (batch_size - pos_num)
    return indices, labels


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
        best_result = test_result = float("-inf")
        self.tokens = 0
        for epoch in range(self.config.max_epochs):
            self.run_epoch("train", epoch, self.train_dataset)
            if self.test_dataset is not None and epoch % 5 == 0:
                test_result = self.run_epoch("infer_test", epoch, self.test_dataset["infer_test"])
            good = self.test_dataset is None or test_result > best_result
            if self.config.ckpt_path is not None and good:
                best_result = test_result
                self.save_checkpoint()
        return best_result

    def run_epoch(self, split, epoch, dataset):
        if self.config.data_mode != "text":
            raise RuntimeError(f"have not yet implemented data mode {self.config.data_mode}")
        is_train = split == "train"
        self.model.train(is_train)
        cfg, w = self.config, self.config.tensorboard_writer
        run_time = 1 if is_train else len(dataset.vids)
        losses, test_aucs, test_m_aps = [], [], []
        for i in range(run_time):
            if not is_train:
                dataset.manual_choose_vid(dataset.vids[i])
            pred_scores, gt_labels = [], []
            loader = torch.utils.data.DataLoader(dataset, shuffle=is_train, pin_memory=True, batch_size=cfg.batch_size,
                                                 num_workers=cfg.num_workers)
            for it, (_img_clip, text_ids, attention_mask, label) in enumerate(loader):
                text_ids = text_ids.to(self.device)
                attention_mask = attention_mask.to(self.device)
                label = label.to(self.device)
                with torch.set_grad_enabled(is_train):
                    if is_train:
                        batch_size, slate_length, _ = text_ids.size()
                        sel, cpu_y = balance_selection(batch_size, slate_length)
                        output = self.model.train_forward(text_ids, attention_mask, label, sel, cpu_y)
                    else:
                        cpu_y = label.cpu().tolist()
                        output = self.model.test_forward(text_ids, attention_mask, targets=label)
                loss = output["loss"]
                if is_train:
                    self.model.zero_grad()
                    loss.backward()
                    self.optimizer.clip_and_step(cfg.grad_norm_clip)
                loss_v = loss.item()
                losses.append(loss_v)
                scores = output["binary_prob"][:, 1].detach().cpu().numpy()
                gt_labels.extend(cpu_y)
                pred_scores.extend(scores)
                if is_train:
                    auc, m_ap = _binary_auc_map(list(cpu_y), scores)
                    lr = cfg.learning_rate
                    if cfg.lr_decay:
                        lr = cfg.learning_rate * lr_multiplier(cfg, epoch)
                        for g in self.optimizer.param_groups:
                            g["lr"] = lr
                    n_iter = epoch * len(loader) + it
                    self.history.append({"epoch": epoch, "it": it, "loss": loss_v, "auc": auc, "m_ap": m_ap, "lr": lr})
                    if w is not None:
                        w.add_scalar("Train/loss", loss_v, n_iter)
                        w.add_scalar("Train/auc", auc, n_iter)
                        w.add_scalar("Train/m_ap", m_ap, n_iter)
            if not is_train:
                auc, m_ap = _binary_auc_map(list(gt_labels), pred_scores)
                test_aucs.append(auc)
                test_m_aps.append(m_ap)
        if is_train:
            logger.info("epoch %d: train loss %.5f", epoch + 1, float(np.mean(losses)) if losses else float("nan"))
            return None
        test_loss, test_auc, test_m_ap = float(np.mean(losses)), float(np.mean(test_aucs)), float(np.mean(test_m_aps))
        print(f"{split}, loss: {test_loss}, auc {test_auc}, m_ap {test_m_ap}")
        if w is not None:
            w.add_scalar(f"{split}/loss", test_loss, epoch)
            w.add_scalar(f"{split}/auc", test_auc, epoch)
            w.add_scalar(f"{split}/m_ap", test_m_ap, epoch)
        return test_m_ap


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="listwise fine-tuning of the language model (MI355X)")
    p.add_argument("--gpu", default=0, type=int)
    p.add_argument("--model_type", default="bert", type=str)
    p.add_argument("--epoch", default=300, type=int)
    p.add_argument("--batch_size", default=64, type=int)
    p.add_argument("--lr_decay_type", default="cosine", type=str)
    p.add_argument("--clip_frame_num", default=8, type=int)
    p.add_argument("--max_text_len", default=50, type=int)
    p.add_argument("--negative_clip_num", default=10, type=int, help="negative clips per slate (slate length - 2)")
    p.add_argument("--bert_layers", default=None, type=int, help="encoder layers (default: bert-base's 12)")
    p.add_argument("--fix_backbone", action="store_true", help="train the pooler and the heads only")
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--seed", default=123, type=int)
    p.add_argument("--ckpt_path", default=None, help="file the state dict is saved to (none: no checkpoint)")
    p.add_argument("--pretrained_ckpt", default=None,
                   help="pretrain_lang_model_hugface.py checkpoint the language model starts from")
    p.add_argument("--lang_contrast_ckpt", default=None,
                   help="train_lang/pretrain_constrast_lang_model.py checkpoint the language model starts from instead")
    p.add_argument("--vocab_file", default=None, help="BERT WordPiece vocab.txt (bert-base-uncased's)")
    p.add_argument("--videos", default=8, type=int, help="synthetic corpus size (no --data_file)")
    p.add_argument("--img_dir", default=None, help="frames <img_dir>/<vid>/%%05d.jpg (they give the videos' lengths)")
    p.add_argument("--data_file", default=None)
    p.add_argument("--vid_file", default=None, help="the training split's vid list")
    p.add_argument("--test_vid_file", default=None, help="the test split's vid list")
    p.add_argument("--subtitle_dir", default=None)
    p.add_argument("--num_workers", default=0, type=int)
    p.add_argument("--tensorboard_log", default=None)
    args = p.parse_args(argv)
    if args.lr_decay_type not in ("cosine", "exp"):
        p.error(f"--lr_decay_type {args.lr_decay_type}: cosine or exp")
    if bool(args.data_file) != bool(args.vid_file) or bool(args.data_file) != bool(args.img_dir):
        p.error("--img_dir, --data_file and --vid_file go together")
    if args.pretrained_ckpt and args.lang_contrast_ckpt:
        p.error("--pretrained_ckpt and --lang_contrast_ckpt: one starting checkpoint at most")
    if args.batch_size < 2:
        p.error("--batch_size: at least 2 (the boundary head takes one half positive, one half negative)")
    if args.negative_clip_num < 1:
        p.error("--negative_clip_num: at least 1")
    return args


def datasets(args, tok):
    """(train slates, {"infer_train", "infer_test"} or None)."""
    T, L, neg = args.clip_frame_num, args.max_text_len, args.negative_clip_num
    if args.data_file:
        from data.infer_youtube_video_dataset import InferYoutubeVideoDataset
        from data.youtube_dataset import YoutubeListwiseClipDataset
        train = YoutubeListwiseClipDataset(args.img_dir, args.data_file, args.vid_file, tok, T, L,
                                           negative_clip_num=neg, mode="text", subtitle_dir=args.subtitle_dir)
        if not args.test_vid_file:
            return train, None
        mk = lambda vf: InferYoutubeVideoDataset(  # noqa: E731
            args.img_dir, args.data_file, vf, tok, T, L, mode="text", subtitle_dir=args.subtitle_dir)
        return train, {"infer_train": mk(args.vid_file), "infer_test": mk(args.test_vid_file)}
    from data.synthetic_dataset import InferYoutubeVideoDataset, SyntheticVideoCorpus, YoutubeListwiseClipDataset
    # (a chapter about every 40 s gives ~3 positive clips each; 4 (neg + 2) T seconds leave enough negatives)
    mk = lambda n, seed: SyntheticVideoCorpus(n, min_len=max(120, 4 * (neg + 2) * T),  # noqa: E731
                                              max_len=max(200, 6 * (neg + 2) * T), H=8, W=8, seed=seed)
    train_c, test_c = mk(max(args.videos, args.batch_size), args.seed), mk(max(2, args.videos // 4), args.seed + 1)
    train = YoutubeListwiseClipDataset(train_c, tok, T, L, negative_clip_num=neg, mode="text")
    return train, {"infer_train": InferYoutubeVideoDataset(train_c, tok, T, L, mode="text"),
                   "infer_test": InferYoutubeVideoDataset(test_c, tok, T, L, mode="text")}


def main(argv=None):
    args = parse_args(argv)
    from common_utils import set_random_seed
    from train_video_segment_point import make_tokenizer
    from vcg_hip import synth
    from vcg_hip.build import build_listnet_model, load_lang_pretrain
    from vcg_hip.nn import BertConfig, check_max_text_len

    set_random_seed.use_fix_random_seed(args.seed)
    cfg = BertConfig(output_attentions=True)
    if args.bert_layers is not None:
        cfg.num_hidden_layers = args.bert_layers
    model = build_listnet_model(precision=args.precision, config=cfg)
    check_max_text_len(model, args.max_text_len)  # (on the CPU until the arguments are checked)
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    model = model.to(device)
    synth.init_params(model, args.seed)  # (on the GPU: the HIP generator)
    if args.pretrained_ckpt:
        load_lang_pretrain(model.base_model, args.pretrained_ckpt)
    if args.lang_contrast_ckpt:
        model.load_constrast_checkpoint(args.lang_contrast_ckpt)
    if args.fix_backbone:
        model.fix_backbone()
    tok = make_tokenizer(args.vocab_file)
    train_ds, test_ds = datasets(args, tok)
    writer = None
    if args.tensorboard_log:
        from common_utils.scalar_log import summary_writer
        writer = summary_writer(args.tensorboard_log)
    conf = TrainerConfig(data_mode="text", model_type=args.model_type, max_epochs=args.epoch,
                         batch_size=args.batch_size, learning_rate=1e-5, block_size=args.max_text_len,
                         lr_decay_type=args.lr_decay_type, lr_decay=True, warmup_epochs=args.epoch // 10,
                         final_epochs=args.epoch // 10 * 9, num_workers=args.num_workers, ckpt_path=args.ckpt_path,
                         tensorboard_writer=writer)
    trainer = Trainer(model, tok, train_ds, test_ds, conf)
    trainer.device = device
    trainer.train()
    return trainer


if __name__ == "__main__":
    main()
