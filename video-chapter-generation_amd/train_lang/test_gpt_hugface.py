"""Reads the generative stage's checkpoint back: the reference's `train_lang/test_gpt_hugface.py` (its `gpt` path) on
the native model.

It takes `pretrain_gpt_lang_model.py`'s arguments (`--vocab_file` / `--merges_file` or the hash tokenizer, `--ckpt_path`,
`--precision`, `--n_layer`, the synthetic corpus without `--data_file`), loads `<ckpt_path>/pretrain_<epoch>.pth` (the
newest, or `--ckpt_epoch`), and then, as the reference script:

1. for a few single-sequence batches prints a top-3 sample of every position beside the ground truth, and the
   next-token accuracy of the argmax;
2. writes text from initial prompts with `common_utils.language_model_utils.token_idx_sample` (temperature 1.0,
   sample=True, top_k=10, `--max_text_len` new tokens) -- here `GPTHugface.generate`: KV-cached decode and the fused
   top-k sampler. The draws are torch.rand's, seeded by `--seed`, not torch.multinomial's.

With the hash tokenizer there is no decoder for ids: the ids themselves are printed.
"""
import argparse
import glob
import os
import re
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from train_lang import pretrain_gpt_lang_model as _train  # noqa: E402

INIT_TEXTS = ["today we are going to look at", "the next step is to add the"]  # (subtitle-like openings)


def parse_args(argv=None):
    extra = argparse.ArgumentParser(add_help=False)
    extra.add_argument("--ckpt_epoch", default=None, type=int, help="which pretrain_<epoch>.pth (default: the newest)")
    extra.add_argument("--batches", default=6, type=int, help="single-sequence batches to evaluate")
    extra.add_argument("--generate_num", default=2, type=int, help="texts generated per initial text")
    own, rest = extra.parse_known_args(argv)
    args = _train.parse_args(rest)
    if not args.ckpt_path:
        raise SystemExit("error: --ckpt_path (the directory pretrain_gpt_lang_model.py wrote) is required")
    for k, v in vars(own).items():
        setattr(args, k, v)
    return args


def find_checkpoint(ckpt_path, epoch=None):
    if epoch is not None:
        path = os.path.join(ckpt_path, f"pretrain_{epoch}.pth")
        if not os.path.exists(path):
            raise SystemExit(f"error: {path} does not exist")
        return path
    found = []
    for p in glob.glob(os.path.join(ckpt_path, "pretrain_*.pth")):
        m = re.fullmatch(r"pretrain_(\d+)\.pth", os.path.basename(p))
        if m:
            found.append((int(m.group(1)), p))
    if not found:
        raise SystemExit(f"error: no pretrain_<epoch>.pth under {ckpt_path}")
    return max(found)[1]


def encode(tok, text):
    if hasattr(tok, "encode"):
        return list(tok.encode(text))
    return list(tok(text).data["input_ids"])


def decode(tok, ids):
    ids = [int(i) for i in ids]
    if hasattr(tok, "decode"):
        return tok.decode(ids)
    return " ".join(str(i) for i in ids)


def evaluate(model, tok, dataset, device, batches, generator):
    """The reference's per-batch report; returns (correct, count) over the batches."""
    from common_utils import language_model_utils
    loader = torch.utils.data.DataLoader(dataset, shuffle=True, batch_size=1, num_workers=0, generator=generator)
    total = [0, 0]
    for n, (x, y, attention_mask) in enumerate(loader):
        if n >= batches:
            break
        x, attention_mask = x.to(device), attention_mask.to(device)
        with torch.no_grad():
            logits, loss = model(x, attention_mask, y)
        z = logits[0].float().cpu()
        probs = torch.softmax(language_model_utils.top_k_logits(z, 3), dim=-1)
        drawn = torch.multinomial(probs, 1, generator=generator)[:, 0].numpy()
        gt = y[0].numpy()
        keep = gt != -1
        first = int(x[0, 0])
        print(f"Gen: {decode(tok, [first] + list(drawn[keep]))}")
        print(f"GT: {decode(tok, [first] + list(gt[keep]))}")
        top1 = z.argmax(-1).numpy()
        correct, count = int((top1[keep] == gt[keep]).sum()), int(keep.sum())
        total[0] += correct
        total[1] += count
        print(f"loss {float(loss):.5f} acc {correct}/{count}, {correct / max(count, 1)}\n")
    return tuple(total)


def generate(model, tok, device, steps, num, generator, init_texts=INIT_TEXTS):
    from common_utils import language_model_utils
    out = []
    for text in init_texts:
        ids = torch.tensor([encode(tok, text)], dtype=torch.int64, device=device)
        for _ in range(num):
            _, new_ids = language_model_utils.token_idx_sample(model, ids, steps, temperature=1.0, sample=True,
                                                               top_k=10, generator=generator)
            print(text + " * " + decode(tok, new_ids))
            out.append(new_ids)
    return out


def main(argv=None):
    args = parse_args(argv)
    from common_utils import set_random_seed
    from vcg_hip.build import build_gpt_model
    from vcg_hip.nn import OpenAIGPTConfig, check_max_text_len

    set_random_seed.use_fix_random_seed(args.seed)
    model = build_gpt_model(precision=args.precision, dropout=args.dropout,
                            config=OpenAIGPTConfig(n_layer=args.n_layer))
    check_max_text_len(model, args.max_text_len)
    path = find_checkpoint(args.ckpt_path, args.ckpt_epoch)
    state = torch.load(path, map_location="cpu", weights_only=True)
    model.load_state_dict(state["model_state_dict"])
    print(f"loaded {path} (epoch {state.get('epoch')}, loss {state.get('best_loss')})")
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    model = model.to(device)
    model.eval()
    tok = _train.make_tokenizer(args.vocab_file, args.merges_file, model.vocab_size)
    train_ds, test_ds = _train.datasets(args, tok, model.vocab_size)
    generator = torch.Generator().manual_seed(args.seed)
    correct, count = evaluate(model, tok, test_ds if test_ds is not None else train_ds, device, args.batches, generator)
    print(f"next-token accuracy over {args.batches} batches: {correct}/{count}")
    print("\n\nGenerate self-defined sentence...")
    texts = generate(model, tok, device, args.max_text_len, args.generate_num, generator)
    return {"checkpoint": path, "correct": correct, "count": count, "generated": texts}


if __name__ == "__main__":
    main()
