"""GPT text generation, GPT-base, bf16 (profiles/gpt_generate_ab.txt): a prompt of 8 tokens extended greedily to 50
(the reference's block size) and to 512 tokens, at batch 1, 16 and 64, on three arms:

  recompute   the reference's algorithm on the native forward: every token re-runs the decoder on the whole prefix
              (GPTHugface.use_kv_cache = False) -- what the project could do before the KV cache;
  cached      KV-cached decode, one enqueued chain per token, Linear layers on the existing GEMM engines
              (GptDecoder.skinny_gemm = False);
  skinny      the same with vcg_gemm_skinny for the Linear layers and the head (B <= 16 only; at B = 64 the routing
              sends the arm to the existing engines, so it is not run there).

The parent starts one process per (section, arm), the arms in alternating order over `--reps` rounds, each under its own
time limit; a child builds the model, generates once to warm up and then times `--runs` whole generations one by one
with device events (recorded before generate() and after it, followed by a synchronise) and prints their median. The
summary gives per arm the median of the processes' medians with their minimum and maximum -- the spread of repeated
identical runs -- as tokens/s and ms per token step.

Byte floor per token step (printed, a floor and not a target): the bf16 decoder weights and the vocabulary head that
must be read once per step, plus the K / V rows read at the mean context length, over the peak HBM bandwidth; and the
number of kernel launches per step.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "video-chapter-generation_amd"))

PROMPT, H, NH, NL, V = 8, 768, 12, 12, 40478
PEAK_GBS = 8000.0  # MI355X HBM3E peak
SECTIONS = {f"b{b}_t{t}": (b, t) for t in (50, 512) for b in (1, 16, 64)}
ARMS = ("recompute", "cached", "skinny")
LIMIT = 420  # seconds per child, model build included


def floor(B, total):
    steps = total - PROMPT
    weights = NL * 12 * H * H * 2
    head = V * H * 2
    mean_ctx = (PROMPT + total) / 2.0
    cache = B * NL * 2 * NH * 64 * 2 * mean_ctx
    byt = weights + head + cache
    return {"steps": steps, "weight_mb": weights / 1e6, "head_mb": head / 1e6, "cache_mb": cache / 1e6,
            "floor_us": byt / (PEAK_GBS * 1e9) * 1e6, "launches": 1 + NL * 7 + 2}


def child(args):
    import torch

    from model.lang.gpt_hugface import GPTHugface
    from vcg_hip import _lib
    from vcg_hip.build import build_gpt_model
    from vcg_hip.gpt_decode import GptDecoder
    _lib.call("vcg_init", 0)
    dev = torch.device("cuda", 0)
    B, total = SECTIONS[args.section]
    steps = total - PROMPT
    GPTHugface.use_kv_cache = args.arm != "recompute"
    GptDecoder.skinny_gemm = args.arm == "skinny"
    model = build_gpt_model(seed=123, device=dev, precision="bf16", dropout=0.0).eval()
    x = torch.randint(0, V, (B, PROMPT), generator=torch.Generator().manual_seed(3)).to(dev)

    def gen():
        return model.generate(x, None, steps=steps, block_size=total)[1]
    first = gen()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = gen()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    med = statistics.median(ms)
    print("RESULT " + json.dumps({
        "section": args.section, "arm": args.arm, "median_ms": round(med, 3), "min_ms": round(min(ms), 3),
        "max_ms": round(max(ms), 3), "runs": args.runs, "ms_per_step": round(med / steps, 4),
        "tokens_per_s": round(B * steps / med * 1e3, 1), "same": bool(torch.equal(first, out)),
        "checksum": int(out.sum().item()), "peak_mib": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}),
        flush=True)


def parent(args):
    results = []
    for section in args.sections:
        B, total = SECTIONS[section]
        arms = [a for a in args.arms if not (a == "skinny" and B > 16)]
        f = floor(B, total)
        print(f"{section}: B={B} prompt {PROMPT} -> {total} tokens ({f['steps']} steps); per step weights "
              f"{f['weight_mb']:.0f} MB + head {f['head_mb']:.0f} MB + cache rows {f['cache_mb']:.1f} MB at "
              f"{PEAK_GBS / 1000:.0f} TB/s = {f['floor_us']:.1f} us floor; {f['launches']} launches per step", flush=True)
        for rep in range(args.reps):
            for arm in (arms if rep % 2 == 0 else arms[::-1]):  # alternating
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--section", section, "--arm", arm,
                       "--runs", str(args.runs)]
                try:
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
                except subprocess.TimeoutExpired:
                    print(f"{section}/{arm}: no result within {LIMIT} s; stopping", flush=True)
                    return 1
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    print(f"{section}/{arm}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
                    return 1  # (nothing more is started on the GPU after a failure)
                r = json.loads(line[0][len("RESULT "):])
                r["rep"] = rep
                results.append(r)
                print(f"{section:9s} {arm:9s} rep {rep}: median {r['median_ms']:10.3f} ms (min {r['min_ms']:.3f}, max "
                      f"{r['max_ms']:.3f}, {r['runs']} runs)  {r['ms_per_step']:8.4f} ms/step  "
                      f"{r['tokens_per_s']:10.1f} tokens/s  peak {r['peak_mib']:.0f} MiB  checksum {r['checksum']}"
                      f"{'' if r['same'] else '  NOT REPEATABLE'}", flush=True)
    print(f"\nGPT-base bf16 greedy, prompt {PROMPT}; median of {args.runs} device-event timings of whole generations "
          f"after one warm-up; per arm the median [minimum, maximum] of the {args.reps} processes' medians, ms per step")
    summary = {}
    for section in args.sections:
        B, total = SECTIONS[section]
        steps = total - PROMPT
        row, txt = {}, []
        for arm in args.arms:
            meds = [r["ms_per_step"] for r in results if r["section"] == section and r["arm"] == arm]
            if not meds:
                continue
            m = statistics.median(meds)
            row[arm] = {"ms_per_step": m, "min": min(meds), "max": max(meds), "tokens_per_s": round(B / m * 1e3, 1)}
            txt.append(f"{arm} {m:8.4f} [{min(meds):.4f}, {max(meds):.4f}] = {B / m * 1e3:9.1f} tok/s")
        summary[section] = row
        ratios = []
        if "recompute" in row and "cached" in row:
            ratios.append(f"recompute / cached = {row['recompute']['ms_per_step'] / row['cached']['ms_per_step']:.2f}")
        if "skinny" in row and "cached" in row:
            ratios.append(f"cached / skinny = {row['cached']['ms_per_step'] / row['skinny']['ms_per_step']:.2f}")
        print(f"{section:9s} " + "   ".join(txt) + "   " + "  ".join(ratios))
    print(json.dumps(summary))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--section", choices=list(SECTIONS))
    ap.add_argument("--arm", choices=ARMS)
    ap.add_argument("--sections", nargs="+", default=list(SECTIONS), choices=list(SECTIONS))
    ap.add_argument("--arms", nargs="+", default=list(ARMS), choices=ARMS)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    return parent(args)


if __name__ == "__main__":
    sys.exit(main())
