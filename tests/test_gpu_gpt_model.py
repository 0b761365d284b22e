"""GPTHugface on the GPU against tests/gpt_ref.py (transformers.OpenAIGPTModel + head + cross-entropy, checked against
transformers in tests/test_cpu_gpt.py): GPT-base, B = 4, L = 32, the full vocabulary 40478, dropout 0, parameters from
synth.init_params, next-token targets, right padding plus one empty text. Mirrors tests/test_gpu_mlm_model.py.

Oracle in fp32 (the reference's arithmetic), fp64 (exact) and fp32 under torch.autocast(bf16).
fp32 mode: logits within 1e-3 of exact, loss within 1e-4, every parameter gradient by `_check_grads`
(tests/test_gpu_mlm_model.py's criterion, copied).
bf16 mode: logits within 5e-2, loss within 1e-2; head.weight's gradient and the last block's gradients within 1.5 x the
autocast oracle's error of exact (median and 90th percentile).
lm_loss against forward + F.cross_entropy on the gathered logits (fp32, 1e-4), n_correct / n_valid against the oracle;
a 2-layer model at L = 160 on the tiled attention kernels by the same criteria; train mode with dropout 0.1, fused
against unfused attention from the same seeds; a bf16 forward under no_grad on a fresh model and after an optimizer
step (the transposed Conv1D weights follow the weights); two identical steps bit-identical; build_chapter_head(2) logits; a fully
ignored batch.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpt_ref import gpt_hidden, gpt_lm

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, L, V = 4, 32, 40478


def _check_grads(model, ref32, ref64):
    """tests/test_gpu_mlm_model.py: ours vs exact within max(5 x |oracle fp32 - exact|, 2e-3) and 5e-2 (relative
    Frobenius) per tensor; analytically zero gradients (the key third of c_attn.bias) must be tiny."""
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


def _batch(Bn, Ln, lens, vocab=V, seed=7):
    """x / y / mask as the dataset makes them: next-token pairs, right padding (X_PAD 0, Y_PAD -1); lens[b] = 0 is an
    empty text (mask all zero, every target ignored)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(Bn, Ln, dtype=torch.int64)
    y = torch.full((Bn, Ln), -1, dtype=torch.int64)
    mask = torch.zeros(Bn, Ln, dtype=torch.int64)
    for b, n in enumerate(lens):
        ids = torch.randint(0, vocab, (n + 1,), generator=g)
        x[b, :n], y[b, :n], mask[b, :n] = ids[:-1], ids[1:], 1
    return x, y, mask


def _build(precision, device=None, dropout=0.0, **cfg):
    from vcg_hip.build import build_gpt_model
    from vcg_hip.nn import OpenAIGPTConfig
    return build_gpt_model(seed=123, device=device, precision=precision, dropout=dropout,
                           config=OpenAIGPTConfig(**cfg)).train()


def _oracle_params(model_cpu, dtype):
    return {n: p.detach().to(dtype).clone().requires_grad_() for n, p in model_cpu.named_parameters()}


def _oracle(x, y, mask, **cfg):
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    cpu = _build("fp32", **cfg)
    nh = cpu.base_model.config.n_head
    out = {"x": x, "y": y, "mask": mask, "R": int((y != -1).sum())}
    for key, dt, ac in (("f32", torch.float32, False), ("f64", torch.float64, False), ("ac", torch.float32, True)):
        params = _oracle_params(cpu, dt)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=ac):
            logits, loss = gpt_lm(params, x, mask, y, nh, autocast=ac)
        loss.backward()
        out[key] = dict(logits=logits.detach(), loss=loss.item(), params=params)
    return out


@pytest.fixture(scope="module")
def oracle():
    """GPT-base; computed once for the module and only read by the tests."""
    return _oracle(*_batch(B, L, [32, 20, 0, 9]))


@pytest.fixture(scope="module")
def oracle_long():
    """2 layers at L = 160: the tiled attention kernels inside the model."""
    return _oracle(*_batch(2, 160, [160, 131], seed=9), n_layer=2)


@pytest.fixture(scope="module", autouse=True)
def _init():
    from vcg_hip import _lib
    _lib.call("vcg_init", 0)


def _rel(a, b):
    return (a.detach().double().cpu() - b.double()).norm().item() / max(b.double().norm().item(), 1e-300)


def _no_key_bias(name, g):
    """A gradient without what is analytically zero: the key third of c_attn.bias (a row-constant score shift leaves
    the softmax unchanged) holds rounding noise only and is compared by its size instead (_key_bias_small)."""
    if not name.endswith("attn.c_attn.bias"):
        return g
    H = g.numel() // 3
    return torch.cat([g[:H], g[2 * H:]])


def _key_bias_small(grads):
    """tests/test_gpu_bert_attn.py's bound on the key bias gradient: below 5e-2 of the query third's norm."""
    for n, g in grads.items():
        if n.endswith("attn.c_attn.bias"):
            H = g.numel() // 3
            assert g[H:2 * H].norm() < 5e-2 * g[:H].norm(), (n, g[H:2 * H].norm(), g[:H].norm())


def _dev(o):
    return (o[k].to(DEV) for k in ("x", "mask", "y"))


def _fp32_checks(o, m):
    x, mask, y = _dev(o)
    ref = o["f64"]
    logits, loss_f = m(x, mask, y)
    assert logits.shape == ref["logits"].shape and logits.dtype == torch.float32 and logits.requires_grad
    e_logits = (logits.detach().double().cpu() - ref["logits"]).abs().max().item()
    print(f"fp32 logits err {e_logits:.3e}; forward loss {loss_f.item():.6f} exact {ref['loss']:.6f}")
    assert e_logits <= 1e-3 and abs(loss_f.item() - ref["loss"]) <= 1e-4
    assert m(x, mask)[1] is None
    m.zero_grad()
    loss, n_correct, n_valid = m.lm_loss(x, mask, y)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - ref["loss"]) <= 1e-4
    sel = o["y"] != -1
    assert n_valid == o["R"] == int(sel.sum())
    assert int(n_correct) == int((ref["logits"][sel].argmax(1) == o["y"][sel]).sum())
    _check_grads(m, o["f32"]["params"], ref["params"])
    # lm_loss against the reference trainer's route: forward, gather, F.cross_entropy
    g_fused = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    m.zero_grad()
    logits, _ = m(x, mask)
    idx = torch.nonzero(y != -1)
    valid = logits[idx[:, 0], idx[:, 1], :]
    ce = F.cross_entropy(valid.view(-1, valid.size(-1)), y[idx[:, 0], idx[:, 1]].view(-1))
    ce.backward()
    torch.cuda.synchronize()
    assert abs(ce.item() - loss.item()) <= 1e-4
    _check_grads(m, o["f32"]["params"], ref["params"])
    # the two routes compute the same fp32 gradient with other summation orders (the head over R rows against B L
    # rows, dz in one piece against autograd's): sums of at most V = 40478 fp32 terms, relative rounding about
    # sqrt(V) 2^-24 = 1.2e-5 per tensor; 1e-4 bounds it with room for the chain through twelve blocks
    gmax = max(v.norm().item() for v in g_fused.values())
    worst = max(_rel(_no_key_bias(n, p.grad), _no_key_bias(n, g_fused[n]).cpu()) for n, p in m.named_parameters()
                if g_fused[n].norm().item() > 1e-6 * gmax)
    print(f"forward + F.cross_entropy vs lm_loss gradients: worst relative difference {worst:.3e}")
    assert worst <= 1e-4


def _bf16_checks(o, m, last_prefix, n_last):
    x, mask, y = _dev(o)
    ref, ac = o["f64"], o["ac"]
    logits, _ = m(x, mask)
    e_logits = (logits.detach().double().cpu() - ref["logits"]).abs().max().item()
    e_ac = (ac["logits"].double() - ref["logits"]).abs().max().item()
    print(f"bf16 logits err {e_logits:.3e} (autocast {e_ac:.3e})")
    assert logits.dtype == torch.float32 and e_logits <= 5e-2
    m.zero_grad()
    loss, n_correct, n_valid = m.lm_loss(x, mask, y)
    loss.backward()
    torch.cuda.synchronize()
    print(f"bf16 lm_loss {loss.item():.6f} exact {ref['loss']:.6f} autocast {ac['loss']:.6f}")
    assert abs(loss.item() - ref["loss"]) <= 1e-2 and n_valid == o["R"]
    grads = dict(m.named_parameters())
    err = lambda n: _rel(grads[n].grad, ref["params"][n].grad)                    # noqa: E731
    err_ac = lambda n: _rel(ac["params"][n].grad, ref["params"][n].grad)          # noqa: E731
    print(f"head.weight grad rel err {err('head.weight'):.3e} (autocast {err_ac('head.weight'):.3e})")
    assert err("head.weight") <= 1.5 * err_ac("head.weight")
    last = [n for n in grads if n.startswith(last_prefix)]
    assert len(last) == n_last
    e16, eac = np.array([err(n) for n in last]), np.array([err_ac(n) for n in last])
    print(f"last block grads: bf16 median {np.median(e16):.2e} / q90 {np.quantile(e16, 0.9):.2e}, autocast "
          f"{np.median(eac):.2e} / {np.quantile(eac, 0.9):.2e}")
    assert np.median(e16) <= 1.5 * np.median(eac)
    assert np.quantile(e16, 0.9) <= 1.5 * np.quantile(eac, 0.9)


def test_fp32_forward_loss_and_gradients(oracle):
    _fp32_checks(oracle, _build("fp32", DEV))


def test_bf16_forward_loss_and_gradients(oracle):
    _bf16_checks(oracle, _build("bf16", DEV), "base_model.h.11.", 12)


def test_tiled_attention_inside_the_model(oracle_long):
    _fp32_checks(oracle_long, _build("fp32", DEV, n_layer=2))
    _bf16_checks(oracle_long, _build("bf16", DEV, n_layer=2), "base_model.h.1.", 12)


def test_dropout_fused_matches_unfused(monkeypatch):
    """Train mode, dropout 0.1, the same seeds: the causal fused kernels against the unfused causal chain, within the
    bf16 tolerance of tests/test_gpu_bert_attn.py::test_fused_attention_in_bert_step_matches_unfused."""
    from vcg_hip.bert import BertEncoderEngine
    x, y, mask = (t.to(DEV) for t in _batch(4, 128, [128, 70, 100, 33], seed=3))
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(BertEncoderEngine, "fused_attn", fused)
        m = _build("bf16", DEV, dropout=0.1, n_layer=4)
        torch.manual_seed(11)  # the dropout seeds (vcg_hip.nn.new_seed) come from torch's RNG
        logits, _ = m(x, mask)
        torch.manual_seed(11)
        m.zero_grad()
        m.lm_loss(x, mask, y)[0].backward()
        torch.cuda.synchronize()
        res[fused] = (logits.detach().float().cpu(),
                      {n: p.grad.detach().float().cpu().clone() for n, p in m.named_parameters()})
    (l1, g1), (l0, g0) = res[True], res[False]
    assert (l1 - l0).abs().max().item() < 5e-2
    gmax = max(v.norm().item() for v in g0.values())
    _key_bias_small(g1)
    _key_bias_small(g0)
    errs = sorted((_rel(_no_key_bias(n, g1[n]), _no_key_bias(n, g0[n])), n) for n in g1
                  if g0[n].norm().item() > 1e-6 * gmax)
    print("grad rel errors: median %.3e, worst %s" % (errs[len(errs) // 2][0], errs[-3:]))
    assert errs[len(errs) // 2][0] < 3e-2 and errs[-1][0] < 1e-1


def test_dropout_matches_the_oracle_fp32():
    """fp32 parity mode in train mode with dropout 0.1 (the unfused causal softmax): the oracle drops what the counter
    hash drops at every site, so the logits agree as without dropout."""
    x, y, mask = _batch(2, 24, [24, 11], vocab=500, seed=5)
    cpu = _build("fp32", dropout=0.1, n_layer=2, vocab_size=500)
    m = _build("fp32", DEV, dropout=0.1, n_layer=2, vocab_size=500)
    torch.manual_seed(5)
    logits, _ = m(x.to(DEV), mask.to(DEV))
    torch.manual_seed(5)
    from vcg_hip.nn import new_seed
    seed = new_seed()
    params = {n: p.detach().double() for n, p in cpu.named_parameters()}
    h = gpt_hidden(params, x, mask, cpu.base_model.config.n_head, prefix="base_model.", p_drop=0.1, seed=seed)
    want = F.linear(h, params["head.weight"])
    err = (logits.detach().double().cpu() - want).abs().max().item()
    print(f"fp32 dropout 0.1 logits err {err:.3e}")
    assert err <= 1e-3


def test_bf16_forward_without_grad_after_a_step(oracle):
    """The bf16 forward reads the transposed copy of the Conv1D weights, so it must follow the weights also where no
    backward follows (torch.no_grad: the driver's test split): on a fresh model, and after an optimizer step, the
    no_grad logits equal the grad-enabled forward's bit for bit and sit within the bf16 tolerance of the oracle on the
    SAME weights."""
    from train_lang.pretrain_gpt_lang_model import TrainerConfig
    x, mask, y = _dev(oracle)
    m = _build("bf16", DEV, n_layer=2)
    with torch.no_grad():  # (the first forward of a fresh model: nothing has filled the copy before)
        first = m(x, mask)[0].clone()
    assert torch.equal(first, m(x, mask)[0].detach())
    opt = m.configure_optimizers(TrainerConfig(learning_rate=1e-3))  # (a step that shows in the logits)
    m.zero_grad()
    m.lm_loss(x, mask, y)[0].backward()
    opt.clip_and_step(1.0)
    with torch.no_grad():
        after = m(x, mask)[0].clone()
    with_grad = m(x, mask)[0].detach()
    torch.cuda.synchronize()
    assert torch.equal(after, with_grad)
    assert not torch.equal(after, first)  # (the step moved the logits: a stale copy would have given `first` again)
    p = {n: v.detach().double().cpu() for n, v in m.named_parameters()}
    h = gpt_hidden(p, oracle["x"], oracle["mask"], 12, prefix="base_model.")
    want = F.linear(h, p["head.weight"])
    err = (after.double().cpu() - want).abs().max().item()
    print(f"bf16 no_grad logits after a step: err {err:.3e}, moved {(after - first).abs().max().item():.3e}")
    assert err <= 5e-2


def test_two_steps_bit_identical(oracle):
    from train_lang.pretrain_gpt_lang_model import TrainerConfig
    x, mask, y = _dev(oracle)
    runs = []
    for _ in range(2):
        m = _build("bf16", DEV, n_layer=3)
        opt = m.configure_optimizers(TrainerConfig(learning_rate=1e-4))
        m.zero_grad()
        m.lm_loss(x, mask, y)[0].backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
        before = {n: p.detach().clone() for n, p in m.named_parameters()}
        opt.clip_and_step(1.0)
        torch.cuda.synchronize()
        runs.append((grads, {n: p.detach().clone() for n, p in m.named_parameters()}, before))
    diff = [n for n in runs[0][0] if not torch.equal(runs[0][0][n], runs[1][0][n])]
    assert not diff, f"gradients not bit-identical run to run: {diff[:5]}"
    assert all(torch.equal(runs[0][1][n], runs[1][1][n]) for n in runs[0][1])
    assert all(not torch.equal(runs[0][1][n], runs[0][2][n]) for n in ("head.weight", "base_model.h.0.attn.c_attn.weight",
                                                                     "base_model.tokens_embed.weight"))


def test_chapter_head_logits(oracle):
    x, mask, _ = _dev(oracle)
    m = _build("fp32", DEV)
    m.build_chapter_head(2)
    m = m.to(DEV)
    with torch.no_grad():
        m.head.bias.copy_(torch.tensor([0.25, -0.5]))
    logits, loss = m(x, mask)
    assert loss is None and logits.shape == (B, L, 2)
    p = {n: v.detach().double().cpu() for n, v in m.named_parameters()}
    h = gpt_hidden(p, oracle["x"], oracle["mask"], 12, prefix="base_model.")
    want = F.linear(h, p["head.weight"], p["head.bias"])
    err = (logits.detach().double().cpu() - want).abs().max().item()
    print(f"chapter head logits err {err:.3e}")
    assert err <= 1e-3
    with pytest.raises(RuntimeError):
        m.lm_loss(x, mask, oracle["y"].to(DEV))


def test_fully_ignored_batch(oracle):
    x, mask, _ = _dev(oracle)
    m = _build("bf16", DEV, n_layer=1)
    m.native_flat()
    m.zero_grad()
    loss, n_correct, n_valid = m.lm_loss(x, mask, torch.full((B, L), -1, dtype=torch.int64))
    assert torch.isnan(loss).item() and n_valid == 0 and int(n_correct) == 0
    loss.backward()
    torch.cuda.synchronize()
    assert all(p.grad is None or not p.grad.any() for p in m.parameters())
    for bad in (V, -2):
        t = oracle["y"].clone()
        t[0, 1] = bad
        with pytest.raises(ValueError):
            m.lm_loss(x, mask, t)
