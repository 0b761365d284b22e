"""model/lang/bert_hugface_listnet.py's BertHugface on the GPU against the CPU oracle: a 2-layer BERT, B = 3 slates of
S = 4 clips, L = 16 tokens, dropout 0, parameters from build_listnet_model(seed=123); the boundary head reads rows
sel = [1, 4, 11] with labels [1, 1, 0].

Oracle (restated from reference model/lang/bert_hugface_listnet.py:148-176 and :183-199): oracle.model.bert with prefix
"base_model.", the bmm of the boundary clip against the slate's other clips, softmax, log(p + 1e-10), the mean slate
loss, plus F.cross_entropy of the head on the selected rows -- in fp32 (the reference's arithmetic), fp64 (exact) and
fp32 under torch.autocast(bf16), computed once for the module.

fp32 mode: loss within 1e-4 of exact, binary_logits within 1e-3, every base_model / head gradient by
tests/test_gpu_single_modes.py's `_check_grads` criterion (copied). bf16 mode: the loss within 1e-2, the pooler's and the
last layer's gradients within 1.5 x autocast's error (median and 90th percentile, no floor).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, S, L, H = 3, 4, 16, 768
SEL, CLS = [1, 4, 11], [1, 1, 0]


def _check_grads(named, ref32, ref64):
    """tests/test_gpu_single_modes.py: ours vs exact within max(5 x |oracle fp32 - exact|, 2e-3) and 5e-2 (relative
    Frobenius) per tensor; analytically zero gradients (attention key biases) must be tiny."""
    gmax = max(v.grad.double().norm().item() for v in ref64.values() if v.grad is not None)
    bad, ratios = [], []
    for n, g in named:
        r64 = ref64[n].grad
        if r64 is None:
            continue
        a, b = g.detach().double().cpu().reshape(-1), r64.double().reshape(-1)
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
    return len(ratios)


class _G:  # a gradient holder with the `.grad` the criterion reads
    def __init__(self, g):
        self.grad = g


def _as_params(grads):
    return {n: _G(g) for n, g in grads.items()}


def _config():
    from vcg_hip.nn import BertConfig
    return BertConfig(num_hidden_layers=2)


def _model(precision, dropout=0.0):
    from vcg_hip.build import build_listnet_model
    return build_listnet_model(seed=123, device=DEV, precision=precision, dropout=dropout, config=_config()).train()


def _batch():
    from vcg_hip import synth
    _, ids, mask, _ = synth.clip_batch(B * S, 1, 8, 8, L, seed=47)
    targets = torch.tensor([[1, 1, 0, 0]] * B)
    return ids.view(B, S, L), mask.view(B, S, L), targets


def _oracle(cpu_sd, names, batch, dtype, autocast):
    from oracle import model as om
    ids, mask, targets = batch
    p = {n: v.detach().to(dtype).clone() if v.is_floating_point() else v for n, v in cpu_sd.items()}
    for n in names:
        p[n].requires_grad_()
    sel, cls = torch.tensor(SEL), torch.tensor(CLS)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        pool_output = om.bert(p, ids.view(-1, L), mask.view(-1, L), prefix="base_model.", n_layers=2)[0]
        emb = pool_output.view(B, S, H)
        pos_emb = emb[:, 0, :].unsqueeze(1)
        contrast_emb = torch.transpose(emb[:, 1:, :], 1, 2)
        logits = torch.bmm(pos_emb, contrast_emb).squeeze(1)
        prob = F.softmax(logits, dim=1)
        preds_log = torch.log(prob + 1e-10)
        surrogate = torch.mean(-torch.sum(targets[:, 1:].to(preds_log.dtype) * preds_log, dim=1))
        binary_logits = F.linear(pool_output[sel], p["head.weight"], p["head.bias"])
        binary_prob = F.softmax(binary_logits, dim=1)
        binary = F.cross_entropy(binary_logits, cls)
        loss = surrogate + binary
        # test_forward (:183-199) on the same clips
        all_logits = F.linear(pool_output, p["head.weight"], p["head.bias"])
        test_loss = F.cross_entropy(all_logits, targets.reshape(-1))
    loss.backward()
    return dict(loss=loss.item(), surrogate=surrogate.item(), binary=binary.item(), logits=binary_logits.detach(),
                prob=binary_prob.detach(), test_logits=all_logits.detach(), test_loss=test_loss.item(),
                grads={n: p[n].grad.detach().clone() for n in names if p[n].grad is not None})


@pytest.fixture(scope="module")
def oracle():
    """Computed once for the module and only read by the tests."""
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    m = _model("fp32")
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    names = [n for n, _ in m.named_parameters() if n.startswith(("base_model.", "head."))]
    batch = _batch()
    out = {"batch": batch, "sd": sd}
    for key, dt, ac in (("f32", torch.float32, False), ("f64", torch.float64, False), ("ac", torch.float32, True)):
        out[key] = _oracle(sd, names, batch, dt, ac)
    return out


def _dev(batch):
    return tuple(t.to(DEV) for t in batch)


def test_fp32_loss_logits_and_gradients(oracle):
    ids, mask, targets = _dev(oracle["batch"])
    ref, ref32 = oracle["f64"], oracle["f32"]
    m = _model("fp32")
    m.zero_grad()
    out = m.train_forward(ids, mask, targets, SEL, CLS)
    assert set(out) >= {"binary_logits", "binary_prob", "loss"}
    out["loss"].backward()
    torch.cuda.synchronize()
    e_logits = (out["binary_logits"].double().cpu() - ref["logits"]).abs().max().item()
    e_prob = (out["binary_prob"].double().cpu() - ref["prob"]).abs().max().item()
    print(f"fp32 loss {out['loss'].item():.6f} exact {ref['loss']:.6f} (surrogate {out['surrogate_loss'].item():.6f} / "
          f"{ref['surrogate']:.6f}, binary {out['binary_loss'].item():.6f} / {ref['binary']:.6f}); logits err "
          f"{e_logits:.3e}, prob err {e_prob:.3e}")
    assert abs(out["loss"].item() - ref["loss"]) <= 1e-4
    assert e_logits <= 1e-3 and e_prob <= 1e-3
    assert out["binary_logits"].shape == (3, 2) and out["binary_logits"].dtype == torch.float32
    named = [(n, p.grad) for n, p in m.named_parameters() if n.startswith(("base_model.", "head."))]
    n_checked = _check_grads(named, _as_params(ref32["grads"]), _as_params(ref["grads"]))
    assert n_checked >= len(named) - 2  # (the 2 layers' key biases: analytically zero)
    assert not m.surrogate_head.weight.grad.any() and not m.surrogate_head.bias.grad.any()
    # device index tensors (the reference driver's) give the same bits
    m.zero_grad()
    out2 = m.train_forward(ids, mask, targets, torch.tensor(SEL, device=DEV), torch.tensor(CLS, device=DEV))
    assert torch.equal(out2["loss"], out["loss"]) and torch.equal(out2["binary_logits"], out["binary_logits"])


def test_bf16_loss_and_gradients(oracle):
    ids, mask, targets = _dev(oracle["batch"])
    ref, ac = oracle["f64"], oracle["ac"]
    m = _model("bf16")
    m.zero_grad()
    out = m.train_forward(ids, mask, targets, SEL, CLS)
    out["loss"].backward()
    torch.cuda.synchronize()
    print(f"bf16 loss {out['loss'].item():.6f} exact {ref['loss']:.6f} autocast {ac['loss']:.6f}")
    assert abs(out["loss"].item() - ref["loss"]) <= 1e-2
    grads = {n: p.grad for n, p in m.named_parameters()}
    rel = lambda a, b: (a.detach().double().cpu() - b.double()).norm().item() / b.double().norm().item()  # noqa: E731
    gmax = max(g.norm().item() for g in ref["grads"].values())
    names = [n for n in ref["grads"] if n.startswith(("base_model.pooler.", "base_model.encoder.layer.1."))
             and ref["grads"][n].norm().item() > 1e-6 * gmax]  # (key.bias: analytically zero)
    assert len(names) == 17
    e16 = np.array([rel(grads[n], ref["grads"][n]) for n in names])
    eac = np.array([rel(ac["grads"][n], ref["grads"][n]) for n in names])
    print(f"pooler + last layer grads: bf16 median {np.median(e16):.2e} / q90 {np.quantile(e16, 0.9):.2e}, autocast "
          f"{np.median(eac):.2e} / {np.quantile(eac, 0.9):.2e}")
    assert np.median(e16) <= 1.5 * np.median(eac)
    assert np.quantile(e16, 0.9) <= 1.5 * np.quantile(eac, 0.9)


def test_test_forward_and_eval_mode(oracle):
    ids, mask, targets = _dev(oracle["batch"])
    ref = oracle["f64"]
    m = _model("fp32")
    out = m.test_forward(ids.view(-1, L), mask.view(-1, L), targets.view(-1))
    e = (out["binary_logits"].double().cpu() - ref["test_logits"]).abs().max().item()
    print(f"test_forward loss {out['loss'].item():.6f} exact {ref['test_loss']:.6f}, logits err {e:.3e}")
    assert set(out) == {"binary_logits", "binary_prob", "loss"}
    assert e <= 1e-3 and abs(out["loss"].item() - ref["test_loss"]) <= 1e-4
    assert torch.allclose(out["binary_prob"], F.softmax(out["binary_logits"], dim=1), atol=1e-6)
    train = m.train_forward(ids, mask, targets, SEL, CLS)
    m.eval()
    with torch.no_grad():
        ev = m.train_forward(ids, mask, targets, SEL, CLS)
    assert not ev["loss"].requires_grad and train["loss"].requires_grad
    assert torch.allclose(ev["binary_logits"], train["binary_logits"], atol=1e-6)
    assert abs(ev["loss"].item() - train["loss"].item()) <= 1e-6


def _key_bias(n):
    return n.endswith("key.bias")  # (analytically zero gradient: rounding noise)


def test_optimizer_skips_surrogate_head_and_frozen_backbone(oracle):
    from train_lang.train_listwise import TrainerConfig
    ids, mask, targets = _dev(oracle["batch"])
    m = _model("fp32")
    opt = m.configure_optimizers(TrainerConfig(learning_rate=1e-4))
    m.zero_grad()
    m.train_forward(ids, mask, targets, SEL, CLS)["loss"].backward()
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt.clip_and_step(1.0)
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        if n.startswith("surrogate_head."):
            assert torch.equal(p.detach(), before[n]), n  # no update, no decay
        elif not _key_bias(n):
            assert not torch.equal(p.detach(), before[n]), n
    # fix_backbone: only the pooler and the boundary head move
    m = _model("fp32")
    m.fix_backbone()
    opt = m.configure_optimizers(TrainerConfig(learning_rate=1e-4))
    m.zero_grad()
    m.train_forward(ids, mask, targets, SEL, CLS)["loss"].backward()
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt.clip_and_step(1.0)
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        if "pooler" in n or n.startswith("head."):
            assert not torch.equal(p.detach(), before[n]), n
        else:
            assert torch.equal(p.detach(), before[n]), n


def test_four_steps_lower_the_loss(oracle):
    from train_lang.train_listwise import TrainerConfig
    ids, mask, targets = _dev(oracle["batch"])
    m = _model("bf16")
    opt = m.configure_optimizers(TrainerConfig(learning_rate=1e-4))
    losses = []
    for _ in range(5):
        m.zero_grad()
        loss = m.train_forward(ids, mask, targets, SEL, CLS)["loss"]
        losses.append(loss.item())
        loss.backward()
        opt.clip_and_step(1.0)
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[4] < losses[0]


def test_state_dict_keys_and_refusals(oracle):
    from model.lang.bert_hugface_listnet import BertHugface
    ids, mask, targets = _dev(oracle["batch"])
    m = _model("bf16")
    assert [k for k in m.state_dict() if not k.startswith("base_model.")] == [
        "head.weight", "head.bias", "surrogate_head.weight", "surrogate_head.bias"]
    assert tuple(m.head.weight.shape) == (2, H) and tuple(m.surrogate_head.weight.shape) == (1, H)
    with pytest.raises(NotImplementedError, match="attention"):
        m.train_forward(ids, mask, targets, SEL, CLS, get_attention=True)
    pre = BertHugface(pretrain_stage=True, config=_config())
    assert tuple(pre.head.weight.shape) == (pre.vocab_size, H) and pre.head.bias is None
    with pytest.raises(NotImplementedError, match="mlm_loss"):
        pre.train_forward(ids, mask, targets, SEL, CLS)
    with pytest.raises(ValueError, match="selected row 12"):
        m.train_forward(ids, mask, targets, [1, 12, 3], CLS)
    with pytest.raises(ValueError, match="binary label 2"):
        m.train_forward(ids, mask, targets, SEL, [1, 2, 0])


def test_driver_round_trip(tmp_path, monkeypatch):
    """Two synthetic epochs of the listwise driver with a 2-layer BERT, its checkpoint, and the hand-off into the
    scorer's text model."""
    import common_utils.scalar_log as scalar_log
    import train_lang.train_listwise as tl
    from vcg_hip import build
    from vcg_hip import nn as vnn
    scalars = []

    class Recorder:  # (what --tensorboard_log hands to TrainerConfig.tensorboard_writer, recording)
        def __init__(self, log_dir):
            pass

        def add_scalar(self, tag, value, step):
            scalars.append((tag, float(value), int(step)))

    monkeypatch.setattr(scalar_log, "summary_writer", Recorder)
    ck = tmp_path / "ck" / "checkpoint.pth"
    tr = tl.main(["--epoch", "2", "--batch_size", "4", "--videos", "8", "--negative_clip_num", "3", "--max_text_len",
                  "16", "--bert_layers", "2", "--ckpt_path", str(ck), "--tensorboard_log", str(tmp_path / "tb")])
    assert len(tr.history) == 4 and all(np.isfinite(h["loss"]) for h in tr.history)
    sd = torch.load(str(ck), map_location="cpu", weights_only=True)  # a bare state dict
    assert tuple(sd["head.weight"].shape) == (2, H) and "surrogate_head.weight" in sd
    tags = {}
    for tag, _, step in scalars:
        tags.setdefault(tag, []).append(step)
    assert set(tags) == {"Train/loss", "Train/auc", "Train/m_ap", "infer_test/loss", "infer_test/auc",
                         "infer_test/m_ap"}
    assert tags["Train/loss"] == [0, 1, 2, 3] and tags["infer_test/m_ap"] == [0]
    # the hand-off: the scorer's text model starts BERT from the checkpoint
    real = vnn.BertConfig
    monkeypatch.setattr(vnn, "BertConfig", lambda **kw: real(num_hidden_layers=2, **kw))
    scorer = build.build_model(data_mode="text", seed=5, device=DEV, lang_listnet_ckpt=str(ck))
    for n, p in scorer.base_model.named_parameters():
        assert torch.equal(p.detach().cpu(), sd["base_model." + n]), n
    assert not torch.equal(scorer.head.weight.detach().cpu(), sd["head.weight"])  # (the scorer's own head)
    # another stage's checkpoint is refused
    contrast = build.build_contrast_model(config=real(num_hidden_layers=2), K=64)
    cpath, mpath = tmp_path / "contrast.pth", tmp_path / "mlm.pth"
    torch.save(contrast.state_dict(), str(cpath))
    torch.save({"model_state_dict": {"base_model." + k: v for k, v in contrast.encoder_q.state_dict().items()}
                | {"head.weight": torch.zeros(30522, 8)}}, str(mpath))
    for bad in (cpath, mpath):
        with pytest.raises(ValueError, match="not a listwise"):
            build.build_model(data_mode="text", device=DEV, lang_listnet_ckpt=str(bad))
    with pytest.raises(ValueError, match="one language-model checkpoint"):
        build.build_model(data_mode="text", device=DEV, lang_listnet_ckpt=str(ck), lang_contrast_ckpt=str(cpath))
