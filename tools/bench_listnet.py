"""Listwise (ListNet) fine-tuning, the fused loss against the same loss from stock ops, at the reference's workload:
batch 64 slates of 12 clips, H = 768, 64 selected rows, bf16 (profiles/listnet_ab.txt).

The chain arm writes reference bert_hugface_listnet.py:148-176 on what the project had before csrc/listnet.hip: torch
bmm / softmax / log / sum / mean with autograd for the slate loss, an index_select, `linear_head` (the fused head kernel
with its own backward) and the vcg::cross_entropy op for the boundary head. The fused arm is vcg_hip.listnet's
ListNetLossFn: one forward launch (plus a one-workgroup mean) and one backward launch.

Two comparisons, the baseline always the chain:
  loss   the loss forward + backward alone (dP, dW, db), from the same pooled input;
  step   the full train step at L = 50 (BERT-base over the 768 sequences, loss, backward, fused clip + AdamW).

The parent starts one process per (section, arm), alternating the arms over `--reps` rounds, each under its own time
limit; a child times `--steps` calls after `--warmup` one by one with device events and prints their median.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "video-chapter-generation_amd"))

B, S, L, H, M = 64, 12, 50, 768, 64
SECTIONS = ("loss", "step")
LIMIT = {"loss": 120, "step": 240}  # seconds per child, model build included


def timed(fn, warmup, steps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(ms), min(ms), max(ms)


def chain_loss(root, head, pooled, targets, sel, cls):
    """The reference's formulation on stock ops; pooled [B S, H] in the compute dtype, sel / cls device int64."""
    import torch
    import torch.nn.functional as F

    from vcg_hip.functions import cross_entropy
    from vcg_hip.linear_head import linear_head
    x = pooled.float()
    emb = x.view(targets.shape[0], targets.shape[1], -1)
    z = torch.bmm(emb[:, :1], emb[:, 1:].transpose(1, 2)).squeeze(1)
    log_p = torch.log(F.softmax(z, dim=1) + 1e-10)
    surrogate = torch.mean(-torch.sum(targets[:, 1:] * log_p, dim=1))
    logits, prob = linear_head(root, head, x.index_select(0, sel))
    return surrogate + cross_entropy(logits, cls), prob


def selection(dev):
    import random

    import torch
    rng = random.Random(7)
    sel = [S * b + (rng.randint(0, 1) if b < B // 2 else rng.randint(2, S - 1)) for b in range(M)]
    cls = [1] * (M // 2) + [0] * (M - M // 2)
    return sel, cls, torch.tensor(sel, device=dev), torch.tensor(cls, device=dev)


def child(args):
    import torch

    from vcg_hip import _lib, synth
    from vcg_hip.build import build_listnet_model
    from vcg_hip.listnet import ListNetLossFn
    from vcg_hip.nn import BertConfig
    _lib.call("vcg_init", 0)
    dev = torch.device("cuda", 0)
    fused = args.arm == "fused"
    out = {"section": args.section, "arm": args.arm}
    sel, cls, sel_d, cls_d = selection(dev)
    targets = torch.zeros((B, S), device=dev)
    targets[:, :2] = 1
    if args.section == "loss":
        # (only the head and the flat gradient buffer are used: one encoder layer keeps the build short)
        model = build_listnet_model(seed=123, device=dev, precision="bf16", config=BertConfig(num_hidden_layers=1))
        model.native_flat()
        g = torch.Generator().manual_seed(5)
        pooled = torch.tanh(torch.randn((B * S, H), generator=g) * 0.2).to(dev, torch.bfloat16).requires_grad_()
        from vcg_hip import ops
        idx = ops.ListnetIndices(sel, cls, B * S, dev)

        def fn():
            pooled.grad = None
            model.zero_grad()
            if fused:
                loss = ListNetLossFn.apply(pooled, model._anchor(dev), model.head, targets, idx, None)[0]
            else:
                loss = chain_loss(model, model.head, pooled, targets, sel_d, cls_d)[0]
            loss.backward()
            return loss
        loss = fn()
        out["loss"] = loss.item()
        out["dP_norm"], out["dW_norm"] = pooled.grad.float().norm().item(), model.head.weight.grad.norm().item()
    else:
        from train_lang.train_listwise import TrainerConfig
        model = build_listnet_model(seed=123, device=dev, precision="bf16").train()
        _, ids, mask, _ = synth.clip_batch(B * S, 1, 8, 8, L, seed=3, device=dev)
        ids, mask = ids.view(B, S, L), mask.view(B, S, L)
        opt = model.configure_optimizers(TrainerConfig(learning_rate=1e-5))
        losses = []

        def fn():
            model.zero_grad()
            if fused:
                loss = model.train_forward(ids, mask, targets, sel, cls)["loss"]
            else:
                pooled = model._pooled(ids.view(-1, L), mask.view(-1, L))
                loss = chain_loss(model, model.head, pooled, targets, sel_d, cls_d)[0]
            loss.backward()
            opt.clip_and_step(1.0)
            losses.append(loss.detach())
        fn()
        out["first_loss"] = losses[0].item()
    med, lo, hi = timed(fn, args.warmup, args.steps)
    out.update(median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4), steps=args.steps,
               peak_mib=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))
    print("RESULT " + json.dumps(out), flush=True)


def parent(args):
    results = []
    for section in args.sections:
        for rep in range(args.reps):
            for arm in (("fused", "chain") if rep % 2 == 0 else ("chain", "fused")):  # alternating
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--section", section, "--arm", arm,
                       "--steps", str(args.steps), "--warmup", str(args.warmup)]
                try:
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT[section])
                except subprocess.TimeoutExpired:
                    print(f"{section}/{arm}: no result within {LIMIT[section]} s; stopping", flush=True)
                    return 1
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    print(f"{section}/{arm}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
                    return 1  # (nothing more is started on the GPU after a failure)
                r = json.loads(line[0][len("RESULT "):])
                r["rep"] = rep
                results.append(r)
                print(f"{section:5s} {arm:6s} rep {rep}: median {r['median_ms']:9.4f} ms  (min {r['min_ms']:.4f}, max "
                      f"{r['max_ms']:.4f}, {r['steps']} steps)  peak {r['peak_mib']:.0f} MiB  "
                      + " ".join(f"{k}={v:.6g}" for k, v in r.items() if k in ("loss", "dP_norm", "dW_norm",
                                                                                 "first_loss")), flush=True)
    print(f"\nB={B} S={S} H={H} M={M} (step: L={L}, BERT-base) bf16; median of {args.steps} device-event timings after "
          f"{args.warmup} warm-ups; per arm the median, minimum and maximum of the {args.reps} processes' medians")
    summary = {}
    for section in args.sections:
        meds = {arm: [r["median_ms"] for r in results if r["section"] == section and r["arm"] == arm]
                for arm in ("fused", "chain")}
        med = {arm: statistics.median(v) for arm, v in meds.items()}
        summary[section] = {"fused_ms": med["fused"], "chain_ms": med["chain"],
                            "chain_over_fused": round(med["chain"] / med["fused"], 3)}
        print(f"{section:5s} fused {med['fused']:9.4f} ms [{min(meds['fused']):.4f}, {max(meds['fused']):.4f}]   chain "
              f"{med['chain']:9.4f} ms [{min(meds['chain']):.4f}, {max(meds['chain']):.4f}]   chain / fused = "
              f"{med['chain'] / med['fused']:.2f}")
    print(json.dumps(summary))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--section", choices=SECTIONS)
    ap.add_argument("--arm", choices=("fused", "chain"))
    ap.add_argument("--sections", nargs="+", default=list(SECTIONS), choices=SECTIONS)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    return parent(args)


if __name__ == "__main__":
    sys.exit(main())
