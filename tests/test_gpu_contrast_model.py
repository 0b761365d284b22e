"""BertHugfaceConstrast on the GPU against the CPU oracle: BERT-base, B = 4 queries, C = 2 candidates, L = 16 tokens,
K = 320 keys, dropout 0, parameters and queue from build_contrast_model(seed, copy_key=False), so the two encoders
differ and a mix-up of them shows.

Oracle (restated from reference model/lang/bert_hugface_constrast.py:97-165): oracle.model.bert with prefix "encoder_q."
/ "encoder_k.", F.normalize, bmm, argmax, gather, the two einsums, / T, F.cross_entropy -- in fp32 (the reference's
arithmetic), fp64 (exact) and fp32 under torch.autocast(bf16). It carries the reference's state from step to step: the
momentum update of the key encoder's parameters, the queue and its pointer.

fp32 mode: forward's logits within 1e-3 of exact, contrast_loss within 1e-4, the selection equal to exact, every
encoder_q gradient by tests/test_gpu_single_modes.py's `_check_grads` criterion (copied), encoder_k's gradients zero,
its parameters the momentum formula bit for bit, the enqueued keys within 1e-5.
bf16 mode: the loss within 1e-2; a selected candidate's exact cosine within 1.5 x the autocast oracle's cosine error of
the best one (the oracle then follows the native selection); the pooler's and the last layer's gradients within 1.5 x
autocast's error as tests/test_gpu_bf16_train.py measures BERT's (median and 90th percentile, no floor).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, C, L, K, H = 4, 2, 16, 320, 768
M, T = 0.999, 0.07


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


def _batch():
    from vcg_hip import synth
    _, ids, mask, _ = synth.clip_batch(B * (1 + C), 1, 8, 8, L, seed=31)
    return ids[:B], mask[:B], ids[B:].view(B, C, L), mask[B:].view(B, C, L)


class Oracle:
    """The reference's forward, state included, on the CPU in one arithmetic."""

    def __init__(self, cpu_model, dtype, autocast):
        sd = cpu_model.state_dict()
        self.names_q = [n for n, _ in cpu_model.named_parameters() if n.startswith("encoder_q.")]
        self.p = {n: sd[n].detach().to(dtype).clone() for n, _ in cpu_model.named_parameters()}
        for n in self.names_q:
            self.p[n].requires_grad_()
        self.queue = sd["queue"].detach().to(dtype).clone()
        self.ptr, self.ac = 0, autocast

    def step(self, batch, k0=None):
        from oracle import model as om
        q_ids, q_mask, c_ids, c_mask = batch
        p = self.p
        for n in self.names_q:
            p[n].grad = None
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=self.ac):
            q = F.normalize(om.bert(p, q_ids, q_mask, prefix="encoder_q.")[0], dim=1)
            with torch.no_grad():
                for n in self.names_q:  # the momentum update (:39-40)
                    nk = "encoder_k." + n[len("encoder_q."):]
                    p[nk] = p[nk] * M + p[n] * (1. - M)
                cand = F.normalize(om.bert(p, c_ids.view(-1, L), c_mask.view(-1, L), prefix="encoder_q.")[0], dim=1)
                cos = torch.bmm(cand.view(B, C, H), q.unsqueeze(2)).squeeze(2)
                if k0 is None:
                    k0 = torch.argmax(cos, dim=1)
                idx = k0.unsqueeze(1).unsqueeze(2).expand(B, 1, L)
                k = F.normalize(om.bert(p, torch.gather(c_ids, 1, idx).squeeze(1),
                                        torch.gather(c_mask, 1, idx).squeeze(1), prefix="encoder_k.")[0], dim=1)
            l_pos = torch.einsum("nc,nc->n", [q, k]).unsqueeze(-1)
            l_neg = torch.einsum("nc,ck->nk", [q, self.queue.clone().detach()])
            logits = torch.cat([l_pos, l_neg], dim=1) / T
            loss = F.cross_entropy(logits.float() if self.ac else logits, torch.zeros(B, dtype=torch.long))
        loss.backward()
        self.queue[:, self.ptr:self.ptr + B] = k.detach().to(self.queue.dtype).T
        self.ptr = (self.ptr + B) % K
        return dict(logits=logits.detach(), loss=loss.item(), cos=cos.detach(), k0=k0, k=k.detach(),
                    grads={n: p[n].grad.detach().clone() for n in self.names_q})


def _cpu_model():
    """A CPU copy of the seeded model (the HIP generator is bit-identical to its numpy twin and much faster)."""
    from vcg_hip.build import build_contrast_model
    cpu = build_contrast_model(precision="fp32", dropout=0.0, K=K, m=M, T=T)
    cpu.load_state_dict({k: v.cpu() for k, v in _model("fp32").state_dict().items()}, strict=True)
    return cpu


class _G:  # a gradient holder with the `.grad` the criterion reads
    def __init__(self, g):
        self.grad = g


def _as_params(grads):
    return {n: _G(g) for n, g in grads.items()}


@pytest.fixture(scope="module")
def oracle():
    """Computed once for the module and only read by the tests: two steps of the fp32 and fp64 oracles."""
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    cpu = _cpu_model()
    batch = _batch()
    out = {"batch": batch, "cpu": cpu}
    for key, dt in (("f32", torch.float32), ("f64", torch.float64)):
        o = Oracle(cpu, dt, False)
        out[key] = [o.step(batch), o.step(batch)]
    return out


def _model(precision, dropout=0.0):
    from vcg_hip.build import build_contrast_model
    return build_contrast_model(seed=123, device=DEV, precision=precision, dropout=dropout, K=K, copy_key=False, m=M,
                                T=T).train()


def _rel(a, b):
    return (a.detach().double().cpu() - b.double()).norm().item() / max(b.double().norm().item(), 1e-300)


def _momentum_once(cpu, times=1):
    sd = cpu.state_dict()
    out = {}
    for n, _ in cpu.encoder_k.named_parameters():
        v = sd["encoder_k." + n].clone()
        for _ in range(times):
            v = v * M + sd["encoder_q." + n] * (1. - M)
        out["encoder_k." + n] = v
    return out


def test_fp32_forward_loss_and_gradients(oracle):
    batch = tuple(t.to(DEV) for t in oracle["batch"])
    ref, ref32 = oracle["f64"][0], oracle["f32"][0]
    # the fused route
    m = _model("fp32")
    m.zero_grad()
    loss, n_correct, n = m.contrast_loss(*batch, device=DEV)
    loss.backward()
    torch.cuda.synchronize()
    print(f"fp32 contrast_loss {loss.item():.6f} exact {ref['loss']:.6f}")
    assert n == B and abs(loss.item() - ref["loss"]) <= 1e-4
    assert int(n_correct) == int((ref["logits"].argmax(1) == 0).sum())
    assert torch.equal(m.last_k0.cpu(), ref["k0"])
    named = [(n, p.grad) for n, p in m.named_parameters() if n.startswith("encoder_q.")]
    assert _check_grads(named, _as_params(ref32["grads"]), _as_params(ref["grads"])) > 180  # (199 less 12 key biases)
    for n, p in m.named_parameters():
        if n.startswith("encoder_k."):
            assert not p.grad.any(), n
    want_k = _momentum_once(oracle["cpu"])
    for n, p in m.named_parameters():  # the momentum formula applied once, bit for bit
        if n.startswith("encoder_k."):
            assert torch.equal(p.detach().cpu(), want_k[n]), n
    e_keys = (m.queue[:, 0:B].t().double().cpu() - ref["k"]).abs().max().item()
    print(f"enqueued keys err {e_keys:.3e}")
    assert e_keys <= 1e-5 and m.queue_ptr.item() == B
    assert torch.equal(m.queue[:, B:].cpu(), oracle["cpu"].queue[:, B:])  # the rest of the queue is untouched
    g_fused = {n: g.detach().clone() for n, g in named}
    # the reference trainer's route: forward + F.cross_entropy (pretrain_constrast_lang_model.py:110-112)
    m = _model("fp32")
    m.zero_grad()
    logits, labels = m(*batch, device=DEV)
    assert logits.shape == (B, 1 + K) and logits.dtype == torch.float32 and logits.requires_grad
    assert labels.dtype == torch.int64 and not labels.any() and labels.device.type == "cuda"
    e_logits = (logits.detach().double().cpu() - ref["logits"]).abs().max().item()
    print(f"fp32 logits err {e_logits:.3e}")
    assert e_logits <= 1e-3
    F.cross_entropy(logits, labels).backward()
    torch.cuda.synchronize()
    named = [(n, p.grad) for n, p in m.named_parameters() if n.startswith("encoder_q.")]
    _check_grads(named, _as_params(ref32["grads"]), _as_params(ref["grads"]))
    _check_grads(named, _as_params(ref32["grads"]), _as_params({n: g.cpu() for n, g in g_fused.items()}))
    assert m.queue_ptr.item() == B and torch.equal(m.last_k0.cpu(), ref["k0"])
    for n, p in m.named_parameters():
        if n.startswith("encoder_k."):
            assert not p.grad.any() and torch.equal(p.detach().cpu(), want_k[n]), n


def test_bf16_loss_selection_and_gradients(oracle):
    batch = tuple(t.to(DEV) for t in oracle["batch"])
    m = _model("bf16")
    m.zero_grad()
    loss, n_correct, n = m.contrast_loss(*batch, device=DEV)
    loss.backward()
    torch.cuda.synchronize()
    k0 = m.last_k0.cpu()
    # the oracles follow the native selection, so a legitimate near-tie does not turn into a loss mismatch
    ref = Oracle(oracle["cpu"], torch.float64, False).step(oracle["batch"], k0=k0)
    ac = Oracle(oracle["cpu"], torch.float32, True).step(oracle["batch"], k0=k0)
    e_cos = (ac["cos"].double() - ref["cos"]).abs().max().item()
    short = ref["cos"].max(1).values - ref["cos"].gather(1, k0[:, None])[:, 0]
    print(f"bf16 loss {loss.item():.6f} exact {ref['loss']:.6f} autocast {ac['loss']:.6f}; selection short of the "
          f"best cosine by {short.max().item():.3e} (autocast cosine err {e_cos:.3e})")
    assert (short <= 1.5 * e_cos).all()
    assert abs(loss.item() - ref["loss"]) <= 1e-2 and n == B
    grads = {n: p.grad for n, p in m.named_parameters()}
    err = lambda n: _rel(grads[n], ref["grads"][n])              # noqa: E731
    err_ac = lambda n: _rel(ac["grads"][n], ref["grads"][n])     # noqa: E731
    gmax = max(g.norm().item() for g in ref["grads"].values())
    names = [n for n in ref["grads"] if n.startswith(("encoder_q.pooler.", "encoder_q.encoder.layer.11."))
             and ref["grads"][n].norm().item() > 1e-6 * gmax]  # (key.bias: analytically zero)
    assert len(names) == 17
    e16, eac = np.array([err(n) for n in names]), np.array([err_ac(n) for n in names])
    print(f"pooler + last layer grads: bf16 median {np.median(e16):.2e} / q90 {np.quantile(e16, 0.9):.2e}, autocast "
          f"{np.median(eac):.2e} / {np.quantile(eac, 0.9):.2e}")
    assert np.median(e16) <= 1.5 * np.median(eac)
    assert np.quantile(e16, 0.9) <= 1.5 * np.quantile(eac, 0.9)
    for n, p in m.named_parameters():
        if n.startswith("encoder_k."):
            assert not p.grad.any(), n
    # the key encoder's bf16 shadow followed the momentum update
    f = m.native_flat()
    p = m.encoder_k.pooler.dense.weight
    assert torch.equal(f.compute_view(p, torch.bfloat16), p.detach().to(torch.bfloat16))
    assert torch.equal(p.detach().cpu(), _momentum_once(oracle["cpu"])["encoder_k.pooler.dense.weight"])


def test_second_step_and_optimizer(oracle):
    from train_lang.pretrain_constrast_lang_model import TrainerConfig
    batch = tuple(t.to(DEV) for t in oracle["batch"])
    ref = oracle["f64"]
    m = _model("fp32")
    opt = m.configure_optimizers(TrainerConfig(learning_rate=1e-4))
    l1, _, _ = m.contrast_loss(*batch, device=DEV)
    m.zero_grad()
    l2, _, _ = m.contrast_loss(*batch, device=DEV)
    print(f"step 1 {l1.item():.6f} (exact {ref[0]['loss']:.6f})  step 2 {l2.item():.6f} (exact {ref[1]['loss']:.6f})")
    assert abs(l1.item() - ref[0]["loss"]) <= 1e-4
    assert abs(l2.item() - ref[1]["loss"]) <= 1e-4  # the oracle's queue holds the first step's keys
    assert abs(ref[1]["loss"] - ref[0]["loss"]) > 1e-3  # (and that changes the loss by more than the bound)
    assert m.queue_ptr.item() == 2 * B
    want_k = _momentum_once(oracle["cpu"], times=2)
    for n, p in m.named_parameters():
        if n.startswith("encoder_k."):
            assert torch.equal(p.detach().cpu(), want_k[n]), n
    l2.backward()
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt.clip_and_step(1.0)
    torch.cuda.synchronize()
    moved = 0
    for n, p in m.named_parameters():
        if n.startswith("encoder_k."):
            assert torch.equal(p.detach(), before[n]), n  # no update, no decay
        elif p.grad.any() and not n.endswith("key.bias"):  # (key.bias: analytically zero, rounding noise)
            assert not torch.equal(p.detach(), before[n]), n
            moved += 1
    assert moved > 180


def test_train_mode_with_dropout(oracle):
    batch = tuple(t.to(DEV) for t in oracle["batch"])
    m = _model("bf16", dropout=0.1)
    m.zero_grad()
    loss, _, _ = m.contrast_loss(*batch, device=DEV)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    assert m.encoder_q.pooler.dense.weight.grad.any()
    assert all(not p.grad.any() for p in m.encoder_k.parameters())
    with pytest.raises(ValueError, match="multiple"):  # K % N != 0, before anything is touched
        m.contrast_loss(batch[0][:3], batch[1][:3], batch[2][:3], batch[3][:3])
    # eval mode without gradient runs the whole sequence too, as the reference does
    m.eval()
    ptr = m.queue_ptr.item()
    k_before = m.encoder_k.pooler.dense.weight.detach().clone()
    with torch.no_grad():
        logits, labels = m(*batch, device=DEV)
    assert logits.shape == (B, 1 + K) and not logits.requires_grad and m.queue_ptr.item() == (ptr + B) % K
    assert not torch.equal(m.encoder_k.pooler.dense.weight.detach(), k_before)


def test_driver_round_trip(tmp_path, monkeypatch):
    """Two synthetic epochs of the contrastive driver with a 2-layer BERT and K = 64, its checkpoint, and the hand-off
    into a scorer's language model."""
    import train_lang.pretrain_constrast_lang_model as pre
    from vcg_hip import build
    from vcg_hip.nn import BertConfig, BertModel
    small = lambda: BertConfig(num_hidden_layers=2)  # noqa: E731
    real = build.build_contrast_model
    monkeypatch.setattr(build, "build_contrast_model", lambda **kw: real(config=small(), **kw))
    import common_utils.scalar_log as scalar_log
    scalars = []

    class Recorder:  # (what --tensorboard_log hands to TrainerConfig.tensorboard_writer, recording)
        def __init__(self, log_dir):
            pass

        def add_scalar(self, tag, value, step):
            scalars.append((tag, float(value), int(step)))

    monkeypatch.setattr(scalar_log, "summary_writer", Recorder)
    ck, tb = tmp_path / "ck" / "pretrain.pth", tmp_path / "tb"
    tr = pre.main(["--epoch", "2", "--batch_size", "4", "--videos", "8", "--queue_size", "64", "--clip_frame_num", "4",
                   "--max_text_len", "16", "--neighbor_size", "1", "--ckpt_path", str(ck), "--tensorboard_log",
                   str(tb)])
    assert len(tr.history) == 4 and all(np.isfinite(h["loss"]) and 0 <= h["acc"] <= 1 for h in tr.history)
    assert tr.history[-1]["tokens"] > tr.history[0]["tokens"] > 0
    assert tr.model.queue_ptr.item() == (4 * 4 + 1 * 4) % 64  # 4 train batches and epoch 0's test batch, 4 keys each
    sd = torch.load(str(ck), map_location="cpu", weights_only=True)  # a bare state dict
    fresh = real(config=small(), K=64)
    fresh.load_state_dict(sd, strict=True)
    assert tuple(sd["queue"].shape) == (768, 64)
    tags = {}
    for tag, _, step in scalars:
        tags.setdefault(tag, []).append(step)
    assert set(tags) == {"Train/loss", "Train/acc", "Test/loss", "Test/acc"}  # the reference's scalars
    assert tags["Train/loss"] == tags["Train/acc"] == [0, 1, 2, 3] and tags["Test/loss"] == tags["Test/acc"] == [0]
    bert = BertModel(small()).to(DEV)
    build.load_contrast_pretrain(bert, str(ck))
    assert torch.equal(bert.pooler.dense.weight.detach().cpu(), sd["encoder_q.pooler.dense.weight"])
    bert.precision = "bf16"
    ids, mask = oracle_ids()
    out = bert(input_ids=ids.to(DEV), attention_mask=mask.to(DEV))
    assert out.pooler_output.shape == (B, 768) and torch.isfinite(out.pooler_output.float()).all()


def oracle_ids():
    q_ids, q_mask, _, _ = _batch()
    return q_ids, q_mask
