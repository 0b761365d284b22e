"""BertHugface(pretrain_stage=True) on the GPU against the CPU oracle: BERT-base, B = 4, L = 32, the full vocabulary,
dropout 0, parameters from synth.init_params, targets from a fixed seed (2 to 5 masked positions per text).

Oracle: oracle.model.bert(..., prefix="base_model.")'s last hidden state, F.linear with head.weight, the masked rows
gathered, F.cross_entropy -- in fp32 (the reference's arithmetic), fp64 (exact) and fp32 under torch.autocast(bf16).

fp32 mode: forward's logits and prob (softmax over dim 1) within 1e-3 of exact, mlm_loss within 1e-4, every parameter
gradient by tests/test_gpu_single_modes.py's `_check_grads` criterion (copied), pooler gradients zero, and the gradient
reached through forward + F.cross_entropy on gathered logits by the same criterion.
bf16 mode: logits within 5e-2, loss within 1e-2; head.weight's gradient within 1.5 x the autocast oracle's error of
exact, and the last encoder layer's gradients within 1.5 x autocast's as tests/test_gpu_bf16_train.py measures BERT's
(median and 90th percentile over the layer's tensors, no floor).
"""
import argparse
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, L = 4, 32


def _oracle_params(model_cpu, dtype=torch.float32):
    sd = model_cpu.state_dict()
    names = [n for n, _ in model_cpu.named_parameters()]
    params = {n: sd[n].detach().to(dtype).clone().requires_grad_() for n in names}
    p = {n: (sd[n].detach().to(dtype).clone() if sd[n].is_floating_point() else sd[n]) for n in sd if n not in params}
    p.update(params)
    return p, params


def _check_grads(model, ref32, ref64):
    """tests/test_gpu_single_modes.py: ours vs exact within max(5 x |oracle fp32 - exact|, 2e-3) and 5e-2 (relative
    Frobenius) per tensor; analytically zero gradients (attention key biases) must be tiny."""
    gmax = max(v.grad.double().norm().item() for v in ref64.values() if v.grad is not None)
    bad, ratios = [], []
    for n, prm in model.named_parameters():
        r64 = ref64[n].grad
        if r64 is None:
            continue
        a, b = prm.grad.detach().double().cpu().reshape(-1), r64.double().reshape(-1)
        nb = b.norm().item()
        if nb <= 1e-6 * gmax:
            assert a.norm().item() <= 1e-5 * gmax, n
            continue
        e = (a - b).norm().item() / nb
        e_ref = (ref32[n].grad.double().reshape(-1) - b).norm().item() / nb
        ratios.append(e / max(e_ref, 2e-3 / 5))
        if e > max(5 * e_ref, 2e-3) or e > 5e-2:
            bad.append((n, e, e_ref))
    print(f"grad error ratio ours / oracle-fp32: median {np.median(ratios):.2f} max {max(ratios):.2f}")
    assert not bad, f"{len(bad)} of {len(ratios)} gradients off (ours, oracle fp32): {bad[:5]}"


def _batch():
    """ids / mask of synth.clip_batch and seeded targets: ~15 % of each text's positions after [CLS], random ids."""
    from vcg_hip import synth
    _, ids, mask, _ = synth.clip_batch(B, 1, 8, 8, L, seed=21)
    g = torch.Generator().manual_seed(7)
    targets = torch.full((B, L), -1, dtype=torch.int64)
    for b in range(B):
        n = int(mask[b].sum())
        pos = 1 + torch.randperm(n - 1, generator=g)[:max(1, round((n - 1) * 0.15))]
        targets[b, pos] = torch.randint(1000, 30522, (len(pos),), generator=g)
    return ids, mask, targets


@pytest.fixture(scope="module")
def oracle():
    """Computed once for the module and only read by the tests."""
    from oracle import model as om
    from vcg_hip.build import build_mlm_model
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    ids, mask, targets = _batch()
    sel = targets != -1
    tgt = targets[sel]
    cpu = build_mlm_model(seed=123, precision="fp32", dropout=0.0)
    out = {"ids": ids, "mask": mask, "targets": targets, "R": int(sel.sum())}
    for key, dt, ac in (("f32", torch.float32, False), ("f64", torch.float64, False), ("ac", torch.float32, True)):
        p, params = _oracle_params(cpu, dt)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=ac):
            _, h = om.bert(p, ids, mask, prefix="base_model.")
            logits = F.linear(h, p["head.weight"])
            loss = F.cross_entropy(logits[sel].float() if ac else logits[sel], tgt)
        loss.backward()
        out[key] = dict(logits=logits.detach(), loss=loss.item(), params=params)
    return out


def _model(precision):
    from vcg_hip.build import build_mlm_model
    return build_mlm_model(seed=123, device=DEV, precision=precision, dropout=0.0).train()


def _rel(a, b):
    return (a.detach().double().cpu() - b.double()).norm().item() / max(b.double().norm().item(), 1e-300)


def test_fp32_forward_loss_and_gradients(oracle):
    ids, mask, targets = (oracle[k].to(DEV) for k in ("ids", "mask", "targets"))
    ref = oracle["f64"]
    m = _model("fp32")
    logits, prob = m(ids, mask)
    assert logits.shape == prob.shape == (B, L, 30522) and logits.dtype == torch.float32
    assert logits.requires_grad and not prob.requires_grad
    e_logits = (logits.detach().double().cpu() - ref["logits"]).abs().max().item()
    e_prob = (prob.double().cpu() - torch.softmax(ref["logits"], dim=1)).abs().max().item()
    print(f"fp32 logits err {e_logits:.3e} prob err {e_prob:.3e}")
    assert e_logits <= 1e-3 and e_prob <= 1e-3
    m(ids, mask, get_attention=True)  # accepted and ignored
    # the fused loss
    m.zero_grad()
    loss, n_correct, n_valid = m.mlm_loss(ids, mask, targets)
    loss.backward()
    torch.cuda.synchronize()
    print(f"fp32 mlm_loss {loss.item():.6f} exact {ref['loss']:.6f}")
    assert abs(loss.item() - ref["loss"]) <= 1e-4
    sel = oracle["targets"] != -1
    assert n_valid == oracle["R"] == int(sel.sum())
    assert int(n_correct) == int((ref["logits"][sel].argmax(1) == oracle["targets"][sel]).sum())
    _check_grads(m, oracle["f32"]["params"], ref["params"])
    for n, p in m.named_parameters():
        if n.startswith("base_model.pooler."):
            assert ref["params"][n].grad is None and not p.grad.any(), n  # outside the graph
    g_fused = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    # the reference trainer's route: forward, gather, F.cross_entropy (pretrain_lang_model_hugface.py:127-133)
    m.zero_grad()
    logits, _ = m(ids, mask)
    idx = torch.nonzero(targets != -1)
    valid = logits[idx[:, 0], idx[:, 1], :]
    F.cross_entropy(valid.view(-1, valid.size(-1)), targets[idx[:, 0], idx[:, 1]].view(-1)).backward()
    torch.cuda.synchronize()
    _check_grads(m, oracle["f32"]["params"], ref["params"])
    worst = max(_rel(p.grad, g_fused[n].cpu()) for n, p in m.named_parameters()
                if g_fused[n].any() and not n.endswith("key.bias"))  # (key.bias: analytically zero, rounding noise)
    print(f"forward + F.cross_entropy vs mlm_loss gradients: worst relative difference {worst:.3e}")


def test_bf16_forward_loss_and_gradients(oracle):
    ids, mask, targets = (oracle[k].to(DEV) for k in ("ids", "mask", "targets"))
    ref, ac = oracle["f64"], oracle["ac"]
    m = _model("bf16")
    logits, prob = m(ids, mask)
    e_logits = (logits.detach().double().cpu() - ref["logits"]).abs().max().item()
    e_ac = (ac["logits"].double() - ref["logits"]).abs().max().item()
    print(f"bf16 logits err {e_logits:.3e} (autocast {e_ac:.3e})")
    assert logits.dtype == torch.float32 and e_logits <= 5e-2
    assert (prob.double().sum(1) - 1).abs().max().item() <= 1e-5
    m.zero_grad()
    loss, n_correct, n_valid = m.mlm_loss(ids, mask, targets)
    loss.backward()
    torch.cuda.synchronize()
    print(f"bf16 mlm_loss {loss.item():.6f} exact {ref['loss']:.6f} autocast {ac['loss']:.6f}")
    assert abs(loss.item() - ref["loss"]) <= 1e-2 and n_valid == oracle["R"]
    grads = dict(m.named_parameters())
    err = lambda n: _rel(grads[n].grad, ref["params"][n].grad)                    # noqa: E731
    err_ac = lambda n: _rel(ac["params"][n].grad, ref["params"][n].grad)          # noqa: E731
    print(f"head.weight grad rel err {err('head.weight'):.3e} (autocast {err_ac('head.weight'):.3e})")
    assert err("head.weight") <= 1.5 * err_ac("head.weight")
    gmax = max(v.grad.norm().item() for v in ref["params"].values() if v.grad is not None)
    last = [n for n in grads if n.startswith("base_model.encoder.layer.11.")
            and ref["params"][n].grad.norm().item() > 1e-6 * gmax]  # (key.bias: analytically zero)
    assert len(last) == 15
    e16, eac = np.array([err(n) for n in last]), np.array([err_ac(n) for n in last])
    print(f"last layer grads: bf16 median {np.median(e16):.2e} / q90 {np.quantile(e16, 0.9):.2e}, autocast "
          f"{np.median(eac):.2e} / {np.quantile(eac, 0.9):.2e}")
    assert np.median(e16) <= 1.5 * np.median(eac)
    assert np.quantile(e16, 0.9) <= 1.5 * np.quantile(eac, 0.9)
    for n, p in m.named_parameters():
        if n.startswith("base_model.pooler."):
            assert not p.grad.any(), n


def _one_step(oracle, precision="bf16"):
    from pretrain_lang_model_hugface import TrainerConfig
    ids, mask, targets = (oracle[k].to(DEV) for k in ("ids", "mask", "targets"))
    m = _model(precision)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = m.configure_optimizers(TrainerConfig(learning_rate=1e-4))
    m.zero_grad()
    loss, _, _ = m.mlm_loss(ids, mask, targets)
    loss.backward()
    opt.clip_and_step(1.0)
    torch.cuda.synchronize()
    return before, {n: p.detach().clone() for n, p in m.named_parameters()}


def test_one_optimizer_step(oracle):
    before, after = _one_step(oracle)
    for n in before:
        if n.startswith("base_model.pooler."):
            assert torch.equal(before[n], after[n]), n  # no gradient in the reference: no update, no decay
    assert not torch.equal(before["head.weight"], after["head.weight"])
    assert not torch.equal(before["base_model.encoder.layer.0.attention.self.query.weight"],
                           after["base_model.encoder.layer.0.attention.self.query.weight"])
    _, again = _one_step(oracle)
    diff = [n for n in after if not torch.equal(after[n], again[n])]
    assert not diff, f"not bit-identical run to run: {diff[:5]}"


def test_empty_batch_and_bad_target(oracle):
    ids, mask = oracle["ids"].to(DEV), oracle["mask"].to(DEV)
    m = _model("bf16")
    m.native_flat()
    m.zero_grad()
    loss, n_correct, n_valid = m.mlm_loss(ids, mask, torch.full((B, L), -1, dtype=torch.int64))
    assert torch.isnan(loss).item() and n_valid == 0 and int(n_correct) == 0
    loss.backward()
    torch.cuda.synchronize()
    assert all(p.grad is None or not p.grad.any() for p in m.parameters())
    for bad in (30522, -2):
        t = oracle["targets"].clone()
        t[0, 1] = bad
        with pytest.raises(ValueError):
            m.mlm_loss(ids, mask, t)
    from vcg_hip.build import build_model
    with pytest.raises(RuntimeError):  # the chapter-head model has no vocabulary head
        build_model("text", device=DEV).mlm_loss(ids, mask, oracle["targets"])


def test_driver_round_trip(tmp_path):
    """Two synthetic epochs of the pre-training driver, its checkpoint, and the scorer driver starting from it."""
    import pretrain_lang_model_hugface as pre
    import train_video_segment_point as drv
    ck_dir, tb = tmp_path / "ck", tmp_path / "tb"
    tr = pre.main(["--epoch", "2", "--batch_size", "4", "--videos", "4", "--max_text_len", "32", "--ckpt_path",
                   str(ck_dir), "--tensorboard_log", str(tb)])
    assert len(tr.history) == 2 and all(np.isfinite(h["loss"]) for h in tr.history)
    assert tr.history[0]["tokens"] > 0 and tr.history[1]["tokens"] > tr.history[0]["tokens"]
    assert sorted(f.name for f in ck_dir.iterdir()) == ["pretrain_0.pth"]  # (epoch 1 did not improve the test loss)
    path = str(ck_dir / "pretrain_0.pth")
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"epoch", "best_loss", "model_state_dict", "optimizer_state_dict", "tokens"}
    assert ck["epoch"] == 0 and np.isfinite(ck["best_loss"]) and ck["tokens"] == tr.history[0]["tokens"]
    assert ck["model_state_dict"]["head.weight"].shape == (30522, 768)
    assert any(tb.iterdir())
    if (tb / "scalars.jsonl").exists():  # (common_utils/scalar_log.py's writer where tensorboard is not installed)
        with open(tb / "scalars.jsonl") as f:
            assert {json.loads(line)["tag"] for line in f} == {"Loss/train", "Loss/test", "Acc/test"}
    # the hand-off: the scorer's language model starts from the checkpoint
    tiny = ["--clip_frame_num", "4", "--resolution", "64", "--max_text_len", "32", "--videos", "2"]
    drv.main(tiny + ["--epoch", "0", "--lang_pretrain_ckpt", path])  # (the flag parses; no epoch runs)
    args = argparse.Namespace(data_mode="all", clip_frame_num=4, head_type="mlp", model_type="r50tsm", seed=123,
                              precision="bf16", lang_pretrain_ckpt=path)
    model = drv.build_model(args, torch.device("cuda", 0))
    sd = model.lang_model.state_dict()
    want = {k[len("base_model."):]: v for k, v in ck["model_state_dict"].items() if k.startswith("base_model.")}
    assert set(sd) == set(want) and len(sd) > 190
    assert all(torch.equal(sd[k].cpu(), want[k]) for k in sd)
    args.lang_pretrain_ckpt = None
    plain = drv.build_model(args, torch.device("cuda", 0)).lang_model.state_dict()
    k = "encoder.layer.0.output.dense.weight"
    assert not torch.equal(plain[k].cpu(), want[k])  # (without the flag: the seeded init, as before)
