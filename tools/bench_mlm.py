"""Masked-LM head, forward + backward of the loss path from the same last hidden state, bf16, B = 64, L = 50, ~15 %
masked (the reference's pre-training shape), in one process (profiles/mlm_head_ab.txt):

  (a) the fused BertHugface.mlm_loss path (vcg_hip.mlm.MlmLossFn: only the masked rows meet the vocabulary);
  (b) the drop-in forward's logits of every position (MlmLogitsFn), gather, F.cross_entropy;
  (c) the reference's formulation on stock PyTorch ops: F.linear on all rows under autocast(bf16), softmax(dim=1),
      gather, F.cross_entropy, autograd -- the baseline; (c32) the same without autocast (the reference runs fp32).

Device-event time over 20 iterations after 5 warm-ups, torch.cuda.max_memory_allocated above the resident state, then
the whole pre-training step (mlm_loss + backward + fused clip + AdamW) in sequences/s and the head's share of it."""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "video-chapter-generation_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vcg_hip import _lib, synth  # noqa: E402
from vcg_hip.build import build_mlm_model  # noqa: E402
from vcg_hip.mlm import MlmLogitsFn, MlmLossFn  # noqa: E402

B, L, V, H = 64, 50, 30522, 768
WARM, ITERS = 5, 20


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(ITERS):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / ITERS, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    _lib.call("vcg_init", 0)
    dev = torch.device("cuda", 0)
    model = build_mlm_model(seed=123, device=dev, precision="bf16").train()
    _, ids, mask, _ = synth.clip_batch(B, 1, 8, 8, L, seed=3, device=dev)
    g = torch.Generator().manual_seed(3)
    masked = (torch.rand((B, L), generator=g) < 0.15) & (mask.cpu() > 0)
    masked[:, 0] = False
    targets = torch.where(masked, torch.randint(1000, V, (B, L), generator=g), -1)
    rows = torch.nonzero(targets.reshape(-1) != -1)[:, 0].to(dev)
    tgt = targets.reshape(-1)[targets.reshape(-1) != -1].to(dev)
    tdev = targets.to(dev)
    R = rows.numel()
    model.native_flat()
    with torch.no_grad():
        last = model._last_hidden(ids, mask).detach()
    anchor = model._anchor(dev)
    hid = last.clone().requires_grad_()

    def path_a():  # (head.weight.grad accumulates across the iterations, as x32 / w32's are dropped in (c))
        hid.grad = None
        loss, _ = MlmLossFn.apply(hid, anchor, model, model.head, rows, tgt, None)
        loss.backward()
        return loss

    def path_b():
        hid.grad = None
        z = MlmLogitsFn.apply(hid, anchor, model, model.head, None).view(B, L, -1)[..., :V]
        idx = torch.nonzero(tdev != -1)
        loss = F.cross_entropy(z[idx[:, 0], idx[:, 1], :], tdev[idx[:, 0], idx[:, 1]])
        loss.backward()
        return loss

    w32 = model.head.weight.detach().clone().requires_grad_()
    x32 = last.float().view(B, L, H).clone().requires_grad_()

    def stock(autocast):
        def run():
            w32.grad = x32.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                logits = F.linear(x32, w32)
                prob = F.softmax(logits, dim=1)  # noqa: F841  (returned by the reference's forward)
                idx = torch.nonzero(tdev != -1)
                valid = logits[idx[:, 0], idx[:, 1], :]
                loss = F.cross_entropy(valid.view(-1, V), tdev[idx[:, 0], idx[:, 1]].view(-1))
            loss.backward()
            return loss
        return run

    res = {"B": B, "L": L, "R": R, "V": V}
    print(f"B={B} L={L} masked rows R={R} V={V} bf16; two fp32 B L x V tensors = {2 * B * L * V * 4 / 2 ** 20:.0f} MiB")
    for key, fn, what in (("a", path_a, "fused mlm_loss"), ("b", path_b, "drop-in forward + gather + CE"),
                          ("c", stock(True), "stock PyTorch, autocast(bf16)"),
                          ("c32", stock(False), "stock PyTorch, fp32")):
        loss = fn().item()
        ms, mib = timed(fn)
        res[key] = {"ms": round(ms, 4), "peak_mib": round(mib, 1), "loss": loss}
        print(f"({key:3s}) {what:34s} fwd+bwd {ms * 1e3:9.1f} us   peak above resident {mib:8.1f} MiB   loss {loss:.4f}",
              flush=True)
    print(f"(a) vs (c): {res['c']['ms'] / res['a']['ms']:.1f}x faster, {res['c']['peak_mib'] - res['a']['peak_mib']:.0f} "
          f"MiB less; vs (c32): {res['c32']['ms'] / res['a']['ms']:.1f}x, "
          f"{res['c32']['peak_mib'] - res['a']['peak_mib']:.0f} MiB less")

    # the whole pre-training step
    from pretrain_lang_model_hugface import TrainerConfig
    opt = model.configure_optimizers(TrainerConfig(learning_rate=1e-4))

    def step():
        model.zero_grad()
        loss, _, _ = model.mlm_loss(ids, mask, targets)
        loss.backward()
        opt.clip_and_step(1.0)

    ms, mib = timed(step)
    res["step"] = {"ms": round(ms, 3), "seq_per_s": round(B / ms * 1e3, 1), "head_share": round(res["a"]["ms"] / ms, 4),
                   "peak_mib": round(mib, 1)}
    print(f"pre-training step (mlm_loss + backward + clip + AdamW): {ms:.2f} ms = {B / ms * 1e3:.0f} sequences/s; the "
          f"head's loss path is {100 * res['a']['ms'] / ms:.1f} % of it")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
