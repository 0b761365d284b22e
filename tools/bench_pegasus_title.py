"""Chapter-title generation, pegasus-large shapes, bf16, random weights (profiles/pegasus_title_ab.txt).

(a) Titles for B chapters of 512 source tokens, 30 greedy tokens each, at B = 1 and 16, on two arms:

  reference    the reference's algorithm (model/lang/pegasus_hugface.py:105-146) on the native forward: one chapter at
               a time, and every token re-runs the whole model -- encoder, the decoder layers' K | V projections of its
               output, and the decoder -- on the tokens so far;
  encode_once  PegasusHugface.generate_ids: the encoder and the K | V projections once for the whole batch, then only
               the decoder per token.

(b) vcg_cross_attn_kv_fwd at (B nh, Lq, Lk) = (256, 31, 512) -- 16 chapters' last decoder pass -- and (16, 1, 512) --
one chapter's first -- against the unfused chain in torch (bmm, softmax in fp32, bmm; the scores and the probabilities
go through HBM), arms `fused` and `unfused`.

The parent starts one process per (section, arm), the arms in alternating order over `--reps` rounds, each under its own
time limit; a child warms up once and then times `--runs` repetitions one by one with device events (followed by a
synchronise) and prints their median. The summary gives per arm the median of the processes' medians with their minimum
and maximum -- the spread of repeated identical runs. After a child that fails or runs out of time nothing more is
started.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "video-chapter-generation_amd"))

SRC, STEPS, H, NH, V = 512, 30, 1024, 16, 96103
SECTIONS = {"titles_b1": ("titles", 1), "titles_b16": ("titles", 16),
            "attn_256x31x512": ("attn", (16, 31, 512)), "attn_16x1x512": ("attn", (1, 1, 512))}
ARMS = {"titles": ("reference", "encode_once"), "attn": ("unfused", "fused")}
LIMIT = 600  # seconds per child, model build included


def _timed(fn, runs):
    import torch
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return out, ms


def child_titles(args, B):
    import torch

    from model.lang.pegasus_hugface import PegasusHugface
    dev = torch.device("cuda", 0)
    torch.manual_seed(123)
    with torch.device(dev):
        model = PegasusHugface()
    model.precision = "bf16"
    model.eval()
    x = torch.randint(2, V, (B, SRC), generator=torch.Generator().manual_seed(3)).to(dev)
    mask = torch.ones_like(x)

    def encode_once():
        # (every sequence runs all 30 steps in both arms: a random model's EOS says nothing about the cost)
        eng = model._engine()
        kv = eng.cross_kv(eng.encode(x, mask))
        head_w = model._head_w(eng.dtype)
        from vcg_hip import gpt_decode as gd
        dec = torch.zeros((B, STEPS + 1), dtype=torch.int64, device=dev)
        for t in range(STEPS):
            hidden = eng.decode(dec[:, :t + 1].contiguous(), None, mask, kv)
            gd.sample(gd.head_logits(hidden.view(B, t + 1, -1)[:, -1], head_w), V, greedy=True, seq=dec, col_off=t + 1)
        return dec[:, 1:]

    def reference():
        rows = []
        with torch.no_grad():
            for b in range(B):
                dec = torch.zeros((1, 1), dtype=torch.int64, device=dev)
                for _ in range(STEPS):
                    logits = model(x[b:b + 1], None, decoder_input_ids=dec)
                    dec = torch.cat([dec, model._draw(logits[:, -1], 1.0, None, False)[None]], 1)
                rows.append(dec[:, 1:])
        return torch.cat(rows)

    fn = encode_once if args.arm == "encode_once" else reference
    with torch.no_grad():
        out, ms = _timed(fn, args.runs)
    return {"unit_ms": statistics.median(ms) / B, "unit": "ms per title", "ms": ms, "checksum": int(out.sum().item()),
            "peak_mib": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}


def child_attn(args, shape):
    import torch

    from vcg_hip import ops
    B, Lq, Lk = shape
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B * Lq, H, generator=g).to(dev, torch.bfloat16)
    kv = torch.randn(B * Lk + 8, 2 * H, generator=g).to(dev, torch.bfloat16)
    ctx = torch.empty((B * Lq, H), dtype=torch.bfloat16, device=dev)
    iters = 200

    def fused():
        for _ in range(iters):
            ops.cross_attn_kv_fwd(q, kv, None, B, NH, Lq, Lk, 0.125, ctx=ctx)
        return ctx

    def unfused():
        out = None
        for _ in range(iters):
            qh = q.view(B, Lq, NH, 64).transpose(1, 2)
            kh = kv[:B * Lk, :H].view(B, Lk, NH, 64).transpose(1, 2)
            vh = kv[:B * Lk, H:].view(B, Lk, NH, 64).transpose(1, 2)
            p = torch.softmax((qh @ kh.transpose(-1, -2)).float() * 0.125, dim=-1).to(torch.bfloat16)
            out = (p @ vh).transpose(1, 2).reshape(B * Lq, H)
        return out

    out, ms = _timed(fused if args.arm == "fused" else unfused, args.runs)
    return {"unit_ms": statistics.median(ms) / iters, "unit": "ms per call", "ms": [m / iters for m in ms],
            "checksum": float(out.float().abs().sum().item()), "peak_mib": 0.0}


def child(args):
    from vcg_hip import _lib
    _lib.call("vcg_init", 0)
    kind, what = SECTIONS[args.section]
    r = child_titles(args, what) if kind == "titles" else child_attn(args, what)
    r.update(section=args.section, arm=args.arm)
    print("RESULT " + json.dumps(r), flush=True)


def parent(args):
    results = []
    for section in args.sections:
        arms = ARMS[SECTIONS[section][0]]
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
                results.append(r)
                print(f"{section:16s} {arm:12s} rep {rep}: {r['unit_ms']:10.4f} {r['unit']} (runs "
                      f"{', '.join(f'{m:.4f}' for m in r['ms'])} ms)  peak {r['peak_mib']:.0f} MiB  checksum "
                      f"{r['checksum']}", flush=True)
    print(f"\npegasus-large shapes, bf16, {SRC} source tokens, {STEPS} greedy tokens; median of {args.runs} device-event "
          f"timings after one warm-up; per arm the median [minimum, maximum] of the {args.reps} processes' medians")
    summary = {}
    for section in args.sections:
        arms = ARMS[SECTIONS[section][0]]
        row, txt = {}, []
        for arm in arms:
            meds = [r["unit_ms"] for r in results if r["section"] == section and r["arm"] == arm]
            if meds:
                row[arm] = {"ms": statistics.median(meds), "min": min(meds), "max": max(meds)}
                txt.append(f"{arm} {row[arm]['ms']:9.4f} [{min(meds):.4f}, {max(meds):.4f}]")
        summary[section] = row
        ratio = f"{arms[0]} / {arms[1]} = {row[arms[0]]['ms'] / row[arms[1]]['ms']:.2f}" if len(row) == 2 else ""
        print(f"{section:16s} " + "   ".join(txt) + "   " + ratio)
    print(json.dumps(summary))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--section", choices=list(SECTIONS))
    ap.add_argument("--arm")
    ap.add_argument("--sections", nargs="+", default=list(SECTIONS), choices=list(SECTIONS))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    return parent(args)


if __name__ == "__main__":
    sys.exit(main())
