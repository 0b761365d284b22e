"""Pegasus training kernels, pegasus-large shapes (16 heads of 64), bf16, Ls = 512 keys, Ld = 30 queries, attention
dropout 0.1 (profiles/pegasus_train_ab.txt).

The cross-attention backward alone at (B nh, Lq, Lk) = (64, 30, 512) and (256, 30, 512) -- batch 4, the reference
driver's default, and batch 16 -- on two arms, alternating in one process:

  fused    vcg_cross_attn_kv_bwd (csrc/pegasus.hip): dQ and dK | dV from q, K | V, dO and the saved row statistics;
           nothing Lq x Lk in HBM;
  unfused  the backward of the chain on stock torch ops (bmm -> fp32 softmax -> dropout -> bmm) through autograd, with
           the probabilities and the dropout mask saved by its forward.

and the forward beside it (vcg_cross_attn_kv_fwd_ex with the statistics against the chain's forward). Then the
streaming kernels of the dropout sites at the encoder's batch-16 shapes (8192 rows x 4096 for the activation, x 1024 for
the residual add, p = 0.1) with the bytes they move per second. Every figure is
the median of `--runs` device-event timings of `--iters` back-to-back calls after one warm-up; per arm the median
[minimum, maximum] over `--reps` alternating rounds.

Last, the train step of the whole model (random pegasus-large weights, bf16, train() mode with the three dropout rates
at 0.1, Ls = 512, Ld = 30, every mask one): title_loss + backward + the fused AdamW step at batch 4 and 16, with
PegasusEngine.fused_cross on and off alternating in this process: ms per step (median of `--steps` device-event timings
after one warm-up step per arm) and the peak allocated memory of the arm's steps.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "video-chapter-generation_amd"))

H, NH, LQ, LK, P = 1024, 16, 30, 512, 0.1
SHAPES = {"bwd_64x30x512": 4, "bwd_256x30x512": 16}


def _timed(fn, runs):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(ms)


def arms(B, iters):
    """{(pass, arm): callable running `iters` calls}"""
    import torch
    import torch.nn.functional as F

    from vcg_hip import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B * LQ, H, generator=g).to(dev, torch.bfloat16)
    kv = torch.randn(B * LK + 8, 2 * H, generator=g).to(dev, torch.bfloat16)
    dO = torch.randn(B * LQ, H, generator=g).to(dev, torch.bfloat16)
    ctx = torch.empty((B * LQ, H), dtype=torch.bfloat16, device=dev)
    stats = torch.empty((B * NH, LQ, 2), dtype=torch.float32, device=dev)
    dq, dkv = torch.empty_like(q), torch.empty((B * LK, 2 * H), dtype=torch.bfloat16, device=dev)

    def fused_fwd():
        for _ in range(iters):
            ops.cross_attn_kv_fwd(q, kv, None, B, NH, LQ, LK, 0.125, ctx=ctx, stats=stats, dropout_p=P, seed=7)

    def fused_bwd():
        for _ in range(iters):
            ops.cross_attn_kv_bwd(q, kv, None, dO, stats, B, NH, LQ, LK, 0.125, P, 7, dq=dq, dkv=dkv)

    qa, kva = q.clone().requires_grad_(), kv[:B * LK].clone().requires_grad_()

    def chain():
        qh = qa.view(B, LQ, NH, 64).transpose(1, 2)
        kh = kva[:, :H].view(B, LK, NH, 64).transpose(1, 2)
        vh = kva[:, H:].view(B, LK, NH, 64).transpose(1, 2)
        p = F.dropout(torch.softmax((qh @ kh.transpose(-1, -2)).float() * 0.125, dim=-1), P, True).to(torch.bfloat16)
        return (p @ vh).transpose(1, 2).reshape(B * LQ, H)

    def unfused_fwd():
        with torch.no_grad():
            for _ in range(iters):
                chain()

    out = chain()

    def unfused_bwd():
        for _ in range(iters):
            qa.grad = kva.grad = None
            out.backward(dO, retain_graph=True)

    fused_fwd()  # (the statistics the backward reads)
    return {("fwd", "fused"): fused_fwd, ("fwd", "unfused"): unfused_fwd, ("bwd", "fused"): fused_bwd,
            ("bwd", "unfused"): unfused_bwd}


def streaming(iters):
    """{name: (callable running `iters` calls, bytes moved per call)}"""
    import torch

    from vcg_hip import ops
    dev = torch.device("cuda", 0)
    rows = 16 * LK
    pre = torch.randn(rows, 4096, device=dev).to(torch.bfloat16)
    f, dy = torch.empty_like(pre), torch.randn(rows, 4096, device=dev).to(torch.bfloat16)
    h, br = torch.zeros(rows, H, device=dev), torch.randn(rows, H, device=dev).to(torch.bfloat16)

    def rep(fn):
        def run():
            for _ in range(iters):
                fn()
        return run

    ops.relu_dropout_fwd(pre, 0.1, 7, out=f)
    return {"relu_dropout_fwd 8192x4096": (rep(lambda: ops.relu_dropout_fwd(pre, 0.1, 7, out=f)), 4 * pre.numel()),
            "relu_dropout_bwd 8192x4096": (rep(lambda: ops.relu_dropout_bwd(dy, f, 0.1, out=dy)), 6 * pre.numel()),
            "dropout_add_fwd 8192x1024": (rep(lambda: ops.dropout_add_fwd(h, br, 0.1, 7)), 10 * br.numel()),
            "dropout_add_bwd 8192x1024": (rep(lambda: ops.dropout_add_bwd(h, torch.bfloat16, 0.1, 7)), 6 * br.numel())}


def train_steps(args, summary):
    import torch

    from model.lang.pegasus_hugface import PegasusHugface
    from vcg_hip.pegasus import PegasusEngine

    class Cfg:
        learning_rate, weight_decay, betas = 1e-5, 0.01, (0.9, 0.95)

    dev = torch.device("cuda", 0)
    torch.manual_seed(123)
    with torch.device(dev):
        model = PegasusHugface(reinit_head=True)
    model.precision = "bf16"
    model.train()
    opt = model.configure_optimizers(Cfg())
    V = model.vocab_size
    g = torch.Generator().manual_seed(3)
    try:
        for B in (4, 16):
            x = torch.randint(2, V, (B, LK), generator=g).to(dev)
            dec = torch.randint(2, V, (B, LQ), generator=g).to(dev)
            tgt = torch.randint(2, V, (B, LQ), generator=g).to(dev)
            ones, dones = torch.ones_like(x), torch.ones_like(dec)

            def step():
                model.zero_grad()
                loss, _, _ = model.title_loss(x, ones, dec, dones, tgt)
                loss.backward()
                opt.step()
                return loss

            res = {True: [], False: []}
            peak = {}
            for rep in range(2):
                for fused in ((True, False) if rep == 0 else (False, True)):  # alternating
                    PegasusEngine.fused_cross = fused
                    step()
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    for _ in range(args.steps):
                        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                        ev[0].record()
                        loss = step()
                        ev[1].record()
                        torch.cuda.synchronize()
                        res[fused].append(ev[0].elapsed_time(ev[1]))
                    peak[fused] = max(peak.get(fused, 0), torch.cuda.max_memory_allocated() / 2 ** 30)
                    if not torch.isfinite(loss).item():
                        raise RuntimeError("train step: the loss is not finite")
            for fused in (True, False):
                r = res[fused]
                summary[f"train_step_b{B}_fused_cross_{int(fused)}"] = {"ms": statistics.median(r), "peak_gib": peak[fused]}
                print(f"train step batch {B:2d} fused_cross={fused!s:5s}: {statistics.median(r):8.1f} [{min(r):.1f}, "
                      f"{max(r):.1f}] ms   peak {peak[fused]:.1f} GiB", flush=True)
    finally:
        PegasusEngine.fused_cross = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--fused-only", action="store_true",
                    help="only the fused cross-attention arms (A/B of two builds of the library through VCG_LIB_PATH)")
    args = ap.parse_args()
    from vcg_hip import _lib
    _lib.call("vcg_init", 0)
    summary = {}
    print(f"pegasus-large heads (16 x 64), bf16, Lq = {LQ}, Lk = {LK}, attention dropout {P}; us per call: median of "
          f"{args.runs} device-event timings of {args.iters} calls after one warm-up; per arm the median [minimum, "
          f"maximum] of {args.reps} alternating rounds")
    for name, B in SHAPES.items():
        fns = arms(B, args.iters)
        if args.fused_only:
            fns = {k: f for k, f in fns.items() if k[1] == "fused"}
        res = {k: [] for k in fns}
        for rep in range(args.reps):
            order = list(fns) if rep % 2 == 0 else list(fns)[::-1]  # alternating
            for k in order:
                res[k].append(1e3 * _timed(fns[k], args.runs) / args.iters)
        for ps in ("fwd", "bwd"):
            if args.fused_only:
                f = res[(ps, "fused")]
                print(f"{name:16s} {ps}: fused {statistics.median(f):8.1f} [{min(f):.1f}, {max(f):.1f}]", flush=True)
                continue
            f, u = res[(ps, "fused")], res[(ps, "unfused")]
            mf, mu = statistics.median(f), statistics.median(u)
            summary[f"{name}_{ps}"] = {"fused_us": mf, "unfused_us": mu}
            print(f"{name:16s} {ps}: fused {mf:8.1f} [{min(f):.1f}, {max(f):.1f}]   unfused {mu:8.1f} "
                  f"[{min(u):.1f}, {max(u):.1f}]   unfused / fused = {mu / mf:.2f}", flush=True)
    if args.fused_only:
        return 0
    for name, (fn, nbytes) in streaming(args.iters).items():
        us = [1e3 * _timed(fn, args.runs) / args.iters for _ in range(args.reps)]
        m = statistics.median(us)
        summary[name] = {"us": m, "gb_per_s": nbytes / m / 1e3}
        print(f"{name:28s} {m:8.1f} [{min(us):.1f}, {max(us):.1f}] us   {nbytes / m / 1e3:7.0f} GB/s", flush=True)
    train_steps(args, summary)
    print(json.dumps(summary))
    return 0


if __name__ == "__main__":
    sys.exit(main())
