"""PegasusHugface.title_loss as the training entry (vcg_hip/pegasus.py: train_forward / train_backward) on the tiny
config of tests/test_gpu_pegasus_model.py, against tests/pegasus_train_ref.py. Eval mode with gradients enabled (p = 0)
unless stated.

  * fp32: the loss within the existing title_loss bound; every parameter gradient within 4 x the error of the statement
    in fp32 on the CPU + 1e-6 x max|ref| (both against fp64), with the tied and with an untied head. The gradient of
    a k_proj.bias is identically zero in exact arithmetic (a constant added to every key shifts a row's scores
    equally, and every dS row sums to zero), so its fp64 reference is rounding noise (about 1e-19: asserted) and a floor
    relative to it collapses; there the floor is 1e-6 x max|ref| of the same attention's q_proj.bias, which is made of the same
    dS at the same scale;
  * bf16: per-parameter relative gradient error against fp64 beside the statement's under torch.autocast(bfloat16) on
    the CPU: median and 90th percentile each <= 1.5 x autocast's (both printed);
  * fused_cross on and off: p = 0 gradients within 5e-3 relative (Frobenius, all parameters together) in bf16; train
    mode with p = 0.1 and the same seed: both arms drop the same elements, the losses within 5e-2;
  * fp32 train mode with three distinct dropout rates: loss and gradients against the statement under the restated masks
    (dropout_util with the engine's seeds and index spaces), <= 1e-3 relative;
  * fix_backbone: only lm_head.weight.grad changes, and the backward launches no GEMM of the engine (ops.gemm_census:
    only the head's);
  * two identical steps from the same state give bit-identical parameters, and a no_grad eval title_loss after a step
    matches the statement on the updated weights;
  * a padded source's extra columns change no gradient; a batch without targets gives NaN and touches no gradient.
"""
import copy

import numpy as np
import pytest
import torch

import pegasus_train_ref as tref
from dropout_util import keep_mask
from test_gpu_pegasus_model import CFG, NH, _batch, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _init():
    from vcg_hip import _lib
    _lib.call("vcg_init", 0)


def _gpu(m, precision, train=False):
    g = copy.deepcopy(m).to(DEV)
    g.precision = precision
    return g.train() if train else g.eval()


def _leaves(m, dtype):
    """the statement's parameter dict: a leaf per trained parameter (a tied head is the same leaf)"""
    P = {k: v.detach().cpu().to(dtype).clone() for k, v in m.base_model.state_dict().items()}
    names = [n for n, p in m.base_model.named_parameters() if p.requires_grad]
    for n in names:
        P[n].requires_grad_()
    if "lm_head.weight" not in names:
        P["lm_head.weight"] = P["model.shared.weight"]
    return P, names


def _ref_grads(m, batch, dtype, autocast=False, drop=None):
    ids, mask, dec, dmask, tgt = batch
    P, names = _leaves(m, dtype)
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            loss, _ = tref.title_loss(P, ids, mask, dec, dmask, tgt, NH, drop=drop)
    else:
        loss, _ = tref.title_loss(P, ids, mask, dec, dmask, tgt, NH, drop=drop)
    loss.backward()
    return loss.detach().double(), {n: P[n].grad.double() for n in names}


def _step_grads(g, batch, seed=None):
    ids, mask, dec, dmask, tgt = (t.to(DEV) for t in batch)
    g.zero_grad()
    if seed is not None:
        torch.manual_seed(seed)
    loss, n_correct, n_valid = g.title_loss(ids, mask, dec, dmask, tgt)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu().double().clone() for n, p in g.base_model.named_parameters() if p.requires_grad}
    return loss.detach().cpu().double(), grads


_REF = {}


def _oracle(reinit):
    if reinit not in _REF:
        m = _model(reinit_head=reinit)
        b = _batch()
        _REF[reinit] = dict(model=m, batch=b, f64=_ref_grads(m, b, torch.float64), f32=_ref_grads(m, b, torch.float32))
    return _REF[reinit]


@pytest.mark.parametrize("reinit", [False, True])
def test_fp32_gradients(reinit):
    o = _oracle(reinit)
    loss, grads = _step_grads(_gpu(o["model"], "fp32"), o["batch"])
    l64, g64 = o["f64"]
    l32, g32 = o["f32"]
    el, el32 = abs(loss - l64).item(), abs(l32 - l64).item()
    print(f"fp32 loss {loss.item():.7f} exact {l64.item():.7f}: err {el:.3e}, the statement in fp32 {el32:.3e}")
    assert el <= 4 * el32 + 1e-6 * abs(l64.item())
    assert set(grads) == set(g64)
    worst = 0.0
    for n in g64:
        e, e32 = (grads[n] - g64[n]).abs().max().item(), (g32[n] - g64[n]).abs().max().item()
        scale_of = n.replace("k_proj.bias", "q_proj.bias")  # (docstring: a k_proj.bias gradient is exactly zero)
        if scale_of != n:  # the premise of the substitution: the fp64 reference is rounding noise
            assert g64[n].abs().max().item() <= 1e-12 * max(1.0, g64[scale_of].abs().max().item()), n
        bound = 4 * e32 + 1e-6 * g64[scale_of].abs().max().item()
        worst = max(worst, e / bound if bound > 0 else float(e > 0))
        assert e <= bound, (n, e, e32)
    print(f"reinit_head={reinit}: worst gradient error / bound {worst:.2f} over {len(g64)} parameters")
    if reinit:
        assert bool((grads["model.shared.weight"][0] == 0).all())  # the padding row


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def test_bf16_gradients():
    o = _oracle(False)
    loss, grads = _step_grads(_gpu(o["model"], "bf16"), o["batch"])
    _, g64 = o["f64"]
    _, gac = _ref_grads(o["model"], o["batch"], torch.float32, autocast=True)
    e16 = np.array([_rel(grads[n], g64[n]) for n in g64])
    eac = np.array([_rel(gac[n], g64[n]) for n in g64])
    print(f"bf16 gradient errors: median {np.median(e16):.3e} / q90 {np.quantile(e16, 0.9):.3e}; autocast "
          f"{np.median(eac):.3e} / {np.quantile(eac, 0.9):.3e}")
    assert np.isfinite(e16).all()
    assert np.median(e16) <= 1.5 * np.median(eac)
    assert np.quantile(e16, 0.9) <= 1.5 * np.quantile(eac, 0.9)


def test_fused_cross_switch():
    from vcg_hip.pegasus import PegasusEngine
    o = _oracle(False)
    try:
        out = {}
        for fused in (True, False):
            PegasusEngine.fused_cross = fused
            out[fused] = _step_grads(_gpu(o["model"], "bf16"), o["batch"])
            out[fused, "train"] = _step_grads(_gpu(_model(dropout=0.1, attention_dropout=0.1, activation_dropout=0.1),
                                                   "bf16", train=True), o["batch"], seed=5)
    finally:
        PegasusEngine.fused_cross = True
    a = torch.cat([out[True][1][n].reshape(-1) for n in sorted(out[True][1])])
    b = torch.cat([out[False][1][n].reshape(-1) for n in sorted(out[False][1])])
    print(f"fused_cross on / off: gradients differ by {_rel(a, b):.3e}; train-mode losses "
          f"{out[True, 'train'][0].item():.5f} / {out[False, 'train'][0].item():.5f}")
    assert _rel(a, b) <= 5e-3
    assert abs(out[True, "train"][0] - out[False, "train"][0]).item() <= 5e-2


def _engine_keeps(seed):
    """pegasus_train_ref.Sites' keeps callable restating the engine's seeds and index spaces"""
    from vcg_hip.bert import _seed
    site = {"embed": 0, "self_p": 1, "self_out": 2, "cross_p": 3, "cross_out": 4, "act": 5, "ffn_out": 6}

    def keeps(name, shape, p):
        layer = (0 if name[0] == "enc" else 1000) + (0 if name[-1] == "embed" else 1 + name[1])
        s = _seed(seed, layer, site[name[-1]])
        if name[-1] == "self_p":  # (z L + q) Lp + k, Lp = L rounded up to 8
            Bz, nh, L, _ = shape
            Lp = (L + 7) // 8 * 8
            idx = np.arange(Bz * nh * L * Lp, dtype=np.int64).reshape(Bz, nh, L, Lp)[..., :L]
        else:  # the element index of the row-major tensor
            idx = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
        return torch.from_numpy(keep_mask(s, idx, p))
    return keeps


def test_fp32_train_mode_dropout(monkeypatch):
    rates = dict(dropout=0.1, attention_dropout=0.15, activation_dropout=0.2)
    m = _model(**rates)
    b = _batch()
    import vcg_hip.nn as vnn
    monkeypatch.setattr(vnn, "new_seed", lambda: 424242)
    loss, grads = _step_grads(_gpu(m, "fp32", train=True), b)
    sites = tref.Sites((0.1, 0.15, 0.2), _engine_keeps(424242))
    l64, g64 = _ref_grads(m, b, torch.float64, drop=sites)
    print(f"train-mode fp32 loss {loss.item():.6f}, the statement under the restated masks {l64.item():.6f}")
    assert abs(loss - l64).item() <= 1e-3 * abs(l64.item())
    a = torch.cat([grads[n].reshape(-1) for n in sorted(g64)])
    w = torch.cat([g64[n].reshape(-1) for n in sorted(g64)])
    print(f"train-mode fp32 gradients: relative error {_rel(a, w):.3e}")
    assert _rel(a, w) <= 1e-3


def test_fix_backbone():
    from vcg_hip import ops
    m = _model(reinit_head=True)
    g = _gpu(m, "fp32")
    g.fix_backbone()
    ids, mask, dec, dmask, tgt = (t.to(DEV) for t in _batch())
    g.native_flat()
    for p in g.parameters():
        p.grad.fill_(3.0)
    loss, _, _ = g.title_loss(ids, mask, dec, dmask, tgt)
    ops.gemm_census_enable(True)
    try:
        loss.backward()
        torch.cuda.synchronize()
        census = ops.gemm_census()
    finally:
        ops.gemm_census_enable(False)
    for n, p in g.named_parameters():
        if n == "base_model.lm_head.weight":
            assert not bool((p.grad == 3.0).all())
        else:
            assert bool((p.grad == 3.0).all()), n
    n_gemm = sum(c for c in (census.values() if isinstance(census, dict) else [len(census)]))
    print("GEMM launches of the backward:", census)
    assert n_gemm <= 2  # the head's dX and dW; nothing of the engine


def test_determinism_and_state():
    import pegasus_ref as ref

    class Cfg:
        learning_rate, weight_decay, betas = 1e-3, 0.01, (0.9, 0.95)

    o = _oracle(False)
    batch = o["batch"]
    ends = []
    for _ in range(2):
        g = _gpu(o["model"], "fp32")
        opt = g.configure_optimizers(Cfg())
        ids, mask, dec, dmask, tgt = (t.to(DEV) for t in batch)
        for _ in range(2):
            g.zero_grad()
            loss, _, _ = g.title_loss(ids, mask, dec, dmask, tgt)
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        ends.append((g, {n: p.detach().cpu().clone() for n, p in g.named_parameters()}))
    assert all(torch.equal(ends[0][1][n].view(torch.int32), ends[1][1][n].view(torch.int32)) for n in ends[0][1])
    assert any(not torch.equal(ends[0][1][n], p.detach()) for n, p in o["model"].named_parameters())
    g = ends[0][0]
    with torch.no_grad():
        ids, mask, dec, dmask, tgt = (t.to(DEV) for t in batch)
        loss, _, _ = g.title_loss(ids, mask, dec, dmask, tgt)
        P = {k: v.detach().cpu().double() for k, v in g.base_model.state_dict().items()}
        want = ref.title_loss_ref(ref.pegasus_logits(P, *batch[:4], NH), batch[3], batch[4])[0]
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_padded_source_columns_change_no_gradient(precision):
    o = _oracle(False)
    ids, mask, dec, dmask, tgt = o["batch"]
    _, ga = _step_grads(_gpu(o["model"], precision), o["batch"])
    junk = torch.randint(2, CFG["vocab_size"], ids.shape, generator=torch.Generator().manual_seed(9))
    ids2 = torch.where(mask != 0, ids, junk)
    _, gb = _step_grads(_gpu(o["model"], precision), (ids2, mask, dec, dmask, tgt))
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def test_no_target_batch():
    g = _gpu(_oracle(False)["model"], "fp32")
    ids, mask, dec, dmask, tgt = (t.to(DEV) for t in _batch())
    g.native_flat()
    for p in g.parameters():
        p.grad.fill_(2.0)
    loss, n_correct, n_valid = g.title_loss(ids, mask, dec, torch.zeros_like(dmask), tgt)
    assert torch.isnan(loss) and n_valid == 0 and loss.requires_grad
    loss.backward()
    torch.cuda.synchronize()
    assert all(bool((p.grad == 2.0).all()) for p in g.parameters())


def test_token_ids_outside_the_vocabulary_are_refused():
    """the forward clamps an id, the embedding backward would write row `id` of the gradient: refused on the host"""
    g = _gpu(_oracle(False)["model"], "fp32")
    ids, mask, dec, dmask, tgt = (t.to(DEV) for t in _batch())
    g.native_flat()
    for p in g.parameters():
        p.grad.fill_(2.0)
    bad = ids.clone()
    bad[0, 0] = CFG["vocab_size"]
    with pytest.raises(ValueError, match="x holds a token id outside"):
        g.title_loss(bad, mask, dec, dmask, tgt)
    bad = dec.clone()
    bad[1, 1] = -1
    with pytest.raises(ValueError, match="decoder_input_ids holds a token id outside"):
        g.title_loss(ids, mask, bad, dmask, tgt)
    torch.cuda.synchronize()
    assert all(bool((p.grad == 2.0).all()) for p in g.parameters())
