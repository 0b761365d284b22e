"""The generative (GPT) stage's two measurements, batch 64, GPT-base shapes (12 heads of 64), bf16, dropout 0.1
(profiles/gpt_ab.txt):

  attn128 / attn512   the fused attention forward + backward with the causal flag against the same kernels without it
                      (non-causal), at L = 128 (bert_attn.hip) and L = 512 (bert_attn_long.hip): what skipping the
                      tiles above the diagonal buys;
  step50 / step512    the full train step (GPTHugface.lm_loss, backward, fused clip + AdamW) with the fused causal
                      attention against the unfused causal chain (QK^T GEMM -> softmax -> PV GEMM), at L = 50 (the
                      reference's max_text_len) and L = 512.

The parent starts one process per (section, arm), alternating the arms over `--reps` rounds, each under its own time
limit; a child times `--steps` calls after `--warmup` one by one with device events and prints their median. The
summary gives, per arm, the median of the processes' medians with their minimum and maximum -- the spread of repeated
identical runs -- next to the ratio.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "video-chapter-generation_amd"))

B, NH, H, P_DROP = 64, 12, 768, 0.1
SECTIONS = {"attn128": ("attn", 128), "attn512": ("attn", 512), "step50": ("step", 50), "step512": ("step", 512)}
ARMS = {"attn": ("causal", "noncausal"), "step": ("fused", "unfused")}
LIMIT = {"attn": 120, "step": 300}  # seconds per child, model build included


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


def child(args):
    import torch

    from vcg_hip import _lib
    _lib.call("vcg_init", 0)
    dev = torch.device("cuda", 0)
    kind, L = SECTIONS[args.section]
    out = {"section": args.section, "arm": args.arm}
    if kind == "attn":
        from vcg_hip.bert import attention_bwd, attention_fwd
        causal = args.arm == "causal"
        Lp = (L + 7) // 8 * 8
        g = torch.Generator().manual_seed(5)
        qkv = (torch.randn(B * L + 8, 3 * H, generator=g) * 1.5).to(torch.bfloat16).to(dev)
        dctx = torch.randn(B * L, H, generator=g).to(torch.bfloat16).to(dev)
        mask = torch.ones(B, L, dtype=torch.int64, device=dev)

        def fn():
            ctx, att = attention_fwd(qkv, mask, B, NH, L, Lp, 64, 0.125, P_DROP, 77, True, causal=causal)
            return attention_bwd(qkv, dctx, ctx, mask, att, B, NH, L, Lp, 64, 0.125, P_DROP, 77, causal=causal)
        out["dqkv_norm"] = fn().float().norm().item()
    else:
        from train_lang.pretrain_gpt_lang_model import TrainerConfig
        from vcg_hip.bert import BertEncoderEngine
        from vcg_hip.build import build_gpt_model
        BertEncoderEngine.fused_attn = args.arm == "fused"
        model = build_gpt_model(seed=123, device=dev, precision="bf16", dropout=P_DROP).train()
        g = torch.Generator().manual_seed(3)
        ids = torch.randint(0, model.vocab_size, (B, L + 1), generator=g)
        x, y = ids[:, :-1].contiguous().to(dev), ids[:, 1:].contiguous()
        mask = torch.ones(B, L, dtype=torch.int64, device=dev)
        opt = model.configure_optimizers(TrainerConfig(learning_rate=1e-5))
        losses = []

        def fn():
            model.zero_grad()
            loss = model.lm_loss(x, mask, y)[0]
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
        kind = SECTIONS[section][0]
        a0, a1 = ARMS[kind]
        for rep in range(args.reps):
            for arm in ((a0, a1) if rep % 2 == 0 else (a1, a0)):  # alternating
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--section", section, "--arm", arm,
                       "--steps", str(args.steps), "--warmup", str(args.warmup)]
                try:
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT[kind])
                except subprocess.TimeoutExpired:
                    print(f"{section}/{arm}: no result within {LIMIT[kind]} s; stopping", flush=True)
                    return 1
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    print(f"{section}/{arm}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
                    return 1  # (nothing more is started on the GPU after a failure)
                r = json.loads(line[0][len("RESULT "):])
                r["rep"] = rep
                results.append(r)
                print(f"{section:8s} {arm:9s} rep {rep}: median {r['median_ms']:9.4f} ms  (min {r['min_ms']:.4f}, max "
                      f"{r['max_ms']:.4f}, {r['steps']} steps)  peak {r['peak_mib']:.0f} MiB  "
                      + " ".join(f"{k}={v:.6g}" for k, v in r.items() if k in ("dqkv_norm", "first_loss")), flush=True)
    print(f"\nB={B} nh={NH} H={H} dropout {P_DROP} bf16 (step: GPT-base, V=40478); median of {args.steps} device-event "
          f"timings after {args.warmup} warm-ups; per arm the median [minimum, maximum] of the {args.reps} processes' "
          "medians")
    summary = {}
    for section in args.sections:
        a0, a1 = ARMS[SECTIONS[section][0]]
        meds = {arm: [r["median_ms"] for r in results if r["section"] == section and r["arm"] == arm]
                for arm in (a0, a1)}
        med = {arm: statistics.median(v) for arm, v in meds.items()}
        summary[section] = {f"{a0}_ms": med[a0], f"{a1}_ms": med[a1], f"{a1}_over_{a0}": round(med[a1] / med[a0], 3)}
        print(f"{section:8s} {a0} {med[a0]:9.4f} ms [{min(meds[a0]):.4f}, {max(meds[a0]):.4f}]   {a1} "
              f"{med[a1]:9.4f} ms [{min(meds[a1]):.4f}, {max(meds[a1]):.4f}]   {a1} / {a0} = {med[a1] / med[a0]:.2f}")
    print(json.dumps(summary))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--section", choices=list(SECTIONS))
    ap.add_argument("--arm", choices=("causal", "noncausal", "fused", "unfused"))
    ap.add_argument("--sections", nargs="+", default=list(SECTIONS), choices=list(SECTIONS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    return parent(args)


if __name__ == "__main__":
    sys.exit(main())
