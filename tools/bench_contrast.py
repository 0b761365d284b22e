"""Contrastive (MoCo) pre-training, fused route against the chain route, at the reference's workload: batch 64,
6 candidates, 50 tokens, K = 65536, bf16 (profiles/contrast_ab.txt).

Both routes run the same native BERT engines. The chain route writes the MoCo part as the reference does, on stock
PyTorch ops: the momentum update as a loop over the 199 parameter pairs with three elementwise launches each (and one
cast that brings the key encoder's span of the bf16 shadow up to date), F.normalize, bmm / argmax / gather,
`queue.clone()`, the two einsums under autocast(bf16), cat, the divide, F.cross_entropy with autograd, and the strided
column write of the enqueue behind `int(queue_ptr)`. The fused route is BertHugfaceConstrast.contrast_loss (csrc/contrast.hip).

Three comparisons, the baseline always the chain:
  step      the full train step (loss, backward, fused clip + AdamW);
  momentum  the momentum update alone;
  infonce   the loss forward + d loss / dq alone, from the same normalised q, k and queue.

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

B, C, L, K, H = 64, 6, 50, 65536, 768
SECTIONS = ("step", "momentum", "infonce")
LIMIT = {"step": 240, "momentum": 180, "infonce": 120}  # seconds per child, model build included


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


class Chain:
    """The reference's formulation of the MoCo part (bert_hugface_constrast.py:34-52, :97-165) on torch ops, around the
    model's native encoders."""

    def __init__(self, model):
        self.m = model

    def momentum(self):
        import torch

        from vcg_hip import ops
        m = self.m
        with torch.no_grad():
            for pq, pk in zip(m.encoder_q.parameters(), m.encoder_k.parameters()):
                torch.add(pk.data * m.m, pq.data * (1. - m.m), out=pk.data)  # (in place: the flat buffer stays bound)
            f = m.native_flat()
            _, ok, n = m._key_span(f)  # (.data writes move no version counter: cast the key encoder's span)
            ops.cast_from_f32(f.data[ok:ok + n], torch.bfloat16, out=f.shadow[ok:ok + n])

    def logits(self, q, k, queue):
        import torch
        with torch.autocast("cuda", dtype=torch.bfloat16):
            l_pos = torch.einsum("nc,nc->n", [q, k]).unsqueeze(-1)
            l_neg = torch.einsum("nc,ck->nk", [q, queue.clone().detach()])
        logits = torch.cat([l_pos, l_neg], dim=1).float()
        logits /= self.m.T
        return logits

    def loss(self, q_ids, q_mask, c_ids, c_mask):
        import torch
        import torch.nn.functional as F
        m = self.m
        Bn, Cn, Ln = c_ids.shape
        m.native_flat()
        q = F.normalize(m.encoder_q.native_forward(q_ids, q_mask)[0].float(), dim=1)
        with torch.no_grad():
            self.momentum()
            cand = F.normalize(m.encoder_q.native_forward(c_ids.view(-1, Ln), c_mask.view(-1, Ln))[0].float(), dim=1)
            k0 = torch.argmax(torch.bmm(cand.view(Bn, Cn, -1), q.detach().unsqueeze(2)).squeeze(2), dim=1)
            idx = k0.unsqueeze(1).unsqueeze(2).expand(Bn, 1, Ln)
            k = F.normalize(m.encoder_k.native_forward(torch.gather(c_ids, 1, idx).squeeze(1),
                                                       torch.gather(c_mask, 1, idx).squeeze(1))[0].float(), dim=1)
        logits = self.logits(q, k, m.queue)
        labels = torch.zeros(Bn, dtype=torch.long, device=logits.device)
        loss = F.cross_entropy(logits, labels)
        with torch.no_grad():
            ptr = int(m.queue_ptr)
            m.queue[:, ptr:ptr + Bn] = k.T
            m.queue_ptr[0] = (ptr + Bn) % m.K
        return loss, (logits.detach().argmax(1) == 0).sum()


def child(args):
    import torch
    import torch.nn.functional as F

    from vcg_hip import _lib, ops, synth
    from vcg_hip.build import build_contrast_model
    _lib.call("vcg_init", 0)
    dev = torch.device("cuda", 0)
    fused = args.arm == "fused"
    out = {"section": args.section, "arm": args.arm}
    if args.section == "infonce":
        g = torch.Generator().manual_seed(5)
        q = F.normalize(torch.randn((B, H), generator=g), dim=1).to(dev)
        k = F.normalize(torch.randn((B, H), generator=g), dim=1).to(dev)
        queue = F.normalize(torch.randn((H, K), generator=g), dim=0).to(dev)
        if fused:
            qb, kb = q.to(torch.bfloat16), k.to(torch.bfloat16)
            km = ops.queue_rebuild(queue, torch.bfloat16)

            def fn():
                r = ops.infonce(qb, kb, km, K, 1 / 0.07, want_dq=True)
                return r[2], r[4]
        else:
            class _M:
                T = 0.07
            chain = Chain(_M())
            qa = q.clone().requires_grad_()

            def fn():
                qa.grad = None
                loss = F.cross_entropy(chain.logits(qa, k, queue), torch.zeros(B, dtype=torch.long, device=dev))
                loss.backward()
                return loss, qa.grad
        loss, dq = fn()
        out["loss"], out["dq_norm"] = loss.item(), dq.float().norm().item()
    else:
        model = build_contrast_model(seed=123, device=dev, precision="bf16", K=K).train()
        _, ids, mask, _ = synth.clip_batch(B * (1 + C), 1, 8, 8, L, seed=3, device=dev)
        batch = (ids[:B], mask[:B], ids[B:].view(B, C, L), mask[B:].view(B, C, L))
        chain = Chain(model)
        if args.section == "momentum":
            model.native_flat()
            fn = model._momentum_update_key_encoder if fused else chain.momentum
            fn()
            out["key_sum"] = sum(p.double().sum().item() for p in model.encoder_k.parameters())
        else:
            from train_lang.pretrain_constrast_lang_model import TrainerConfig
            opt = model.configure_optimizers(TrainerConfig(learning_rate=1e-4))
            losses = []

            def fn():
                model.zero_grad()
                loss, _ = (model.contrast_loss(*batch)[:2] if fused else chain.loss(*batch))
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
                print(f"{section:9s} {arm:6s} rep {rep}: median {r['median_ms']:9.3f} ms  (min {r['min_ms']:.3f}, max "
                      f"{r['max_ms']:.3f}, {r['steps']} steps)  peak {r['peak_mib']:.0f} MiB  "
                      + " ".join(f"{k}={v:.6g}" for k, v in r.items() if k in ("loss", "dq_norm", "first_loss",
                                                                                 "key_sum")), flush=True)
    print(f"\nB={B} C={C} L={L} K={K} bf16; median of {args.steps} device-event timings after {args.warmup} warm-ups")
    summary = {}
    for section in args.sections:
        med = {arm: statistics.median(r["median_ms"] for r in results if r["section"] == section and r["arm"] == arm)
               for arm in ("fused", "chain")}
        summary[section] = {"fused_ms": med["fused"], "chain_ms": med["chain"],
                            "chain_over_fused": round(med["chain"] / med["fused"], 3)}
        print(f"{section:9s} fused {med['fused']:9.3f} ms   chain {med['chain']:9.3f} ms   chain / fused = "
              f"{med['chain'] / med['fused']:.2f}")
    print(json.dumps(summary))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--section", choices=SECTIONS)
    ap.add_argument("--arm", choices=("fused", "chain"))
    ap.add_argument("--sections", nargs="+", default=list(SECTIONS), choices=SECTIONS)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    return parent(args)


if __name__ == "__main__":
    sys.exit(main())
