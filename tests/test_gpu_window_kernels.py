"""Kernel-level numerics of the window inference kernels (csrc/window_attn.hip) through the C ABI, against plain fp64
torch on the CPU: vcg_rowdot_fwd / _bwd and vcg_mul_fwd (the bilinear and multiplication window heads),
vcg_ln_act_fwd, vcg_cross_attn_fwd and vcg_window_attn_fwd.

The references restate the semantics include/vcg_hip.h documents, in this file; weights are packed by
pack_window_weights / pack_cross_attn_weights from modules built in fp32, and the fp64 reference reads the same
module's parameters cast to double.

Bounds: single products (vcg_mul_fwd, dU of vcg_rowdot_bwd) are bit-equal to torch fp32. Dot products
(vcg_rowdot_fwd, dx of vcg_rowdot_bwd): max abs error <= 2e-5 x max|ref|. The three chained kernels (window,
cross-attention, ln_act): max(3 x the error of the same reference run in torch fp32 against its fp64 run,
2e-5 x max|ref|): the fp32 run of the reference is the yardstick for how far six LayerNorm / GELU layers drift in
fp32, never the kernel's own output.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
SENTINEL = -7.25


def _close(out, ref, what=""):
    """max abs error <= 2e-5 x max|ref| (fp32 accumulation of exact operands)."""
    out = out.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    scale = ref.abs().max().item() + 1e-6
    err = (out - ref).abs().max().item()
    print(f"ERRSTAT {what} | {err / (2e-5 * scale):.4f} of bound")
    assert err <= 2e-5 * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _close32(out, ref64, ref32, what=""):
    """error vs fp64 <= max(3 x torch-fp32's error vs fp64, 2e-5 x max|ref|)"""
    out, ref64, ref32 = out.detach().double().cpu(), ref64.detach().double(), ref32.detach().double()
    assert out.shape == ref64.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref64.shape)}"
    assert torch.isfinite(out).all(), f"{what}: not finite"
    err = (out - ref64).abs().max().item()
    err32 = (ref32 - ref64).abs().max().item()
    floor = 2e-5 * ref64.abs().max().item()
    tol = max(3 * err32, floor)
    rule = "3x-fp32" if 3 * err32 > floor else "2e-5"
    print(f"ERRSTAT {what} | {err / max(tol, 1e-300):.4f} of bound ({rule}; {err / max(floor, 1e-300):.4f} of 2e-5 x max|ref|, "
          f"torch-fp32 {err32 / max(floor, 1e-300):.4f})")
    assert err <= tol, f"{what}: err {err:.3e} > tol {tol:.3e} (torch-fp32 err {err32:.3e})"


@pytest.fixture(scope="module")
def K():
    from vcg_hip import ops, _lib
    _lib.call("vcg_init", 0)
    return ops


def _randomise(module, seed):
    """Every parameter redrawn from a seeded generator: matrices at fan_in ** -0.5, LayerNorm gains in [0.5, 1.5],
    non-zero biases (the constructors leave them 0), window_pos_bias at 0.5."""
    g = torch.Generator().manual_seed(seed)
    norms = {n for n, m in module.named_modules() if isinstance(m, torch.nn.LayerNorm)}
    with torch.no_grad():
        for n, p in module.named_parameters():
            owner = n.rsplit(".", 1)[0]
            if owner in norms and n.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif n.endswith("window_pos_bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
    return module


def _params(module, dtype):
    return {n: p.detach().to(dtype) for n, p in module.named_parameters()}


def _lin(p, name, x):
    return F.linear(x, p[name + ".weight"], p[name + ".bias"])


def _ln(p, name, x, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), p[name + ".weight"], p[name + ".bias"], eps)


# ============================================================================ rowdot (nn.Bilinear's second contraction)
# (B, R, K): minimum; B * R = 15 leaves a ragged last block of 4 waves and K is no multiple of 64; the bilinear
# head; K > 256: the backward's grid.x is 2
ROWDOT_SHAPES = [(1, 1, 1), (3, 5, 70), (7, 128, 128), (2, 3, 300)]


def _rowdot_inputs(B, R, K):
    g = torch.Generator().manual_seed(B * 977 + R * 31 + K)
    return (torch.randn(B, R, K, generator=g), torch.randn(B, K, generator=g), torch.randn(R, generator=g),
            torch.randn(B, R, generator=g))


@pytest.mark.parametrize("shape", ROWDOT_SHAPES, ids=str)
def test_rowdot_fwd(K, shape):
    """out[b][r] = sum_i U[b][r][i] x[b][i] + bias[r] against fp64; bias = NULL adds nothing."""
    from vcg_hip import _lib
    B, R, Kd = shape
    U, x, bias, _ = _rowdot_inputs(B, R, Kd)
    ref = torch.einsum("bri,bi->br", U.double(), x.double())
    Ug, xg, bg = U.to(DEV), x.to(DEV), bias.to(DEV)
    for b, r, tag in ((bg, ref + bias.double(), "bias"), (None, ref, "no bias")):
        out = torch.full((B, R), float("nan"), device=DEV)
        _lib.call("vcg_rowdot_fwd", K.P(Ug), K.P(xg), K.P(b), K.P(out), B, R, Kd, K.stream())
        _close(out, r, f"rowdot_fwd {shape} ({tag})")


@pytest.mark.parametrize("shape", ROWDOT_SHAPES, ids=str)
def test_rowdot_bwd(K, shape):
    """dx[b][i] = sum_r dy[b][r] U[b][r][i] against fp64; dU[b][r][i] = dy[b][r] x[b][i], a single product, bit-equal
    to torch fp32. dx = NULL (then U may be NULL too): dU unchanged, and a dx buffer that is not passed stays as
    it was."""
    from vcg_hip import _lib
    B, R, Kd = shape
    U, x, _, dy = _rowdot_inputs(B, R, Kd)
    dx_ref = torch.einsum("br,bri->bi", dy.double(), U.double())
    dU_ref = dy[:, :, None] * x[:, None, :]
    Ug, xg, dyg = U.to(DEV), x.to(DEV), dy.to(DEV)
    dU = torch.full((B, R, Kd), float("nan"), device=DEV)
    dx = torch.full((B, Kd), float("nan"), device=DEV)
    _lib.call("vcg_rowdot_bwd", K.P(Ug), K.P(xg), K.P(dyg), K.P(dU), K.P(dx), B, R, Kd, K.stream())
    assert torch.equal(dU.cpu(), dU_ref), "dU is not the fp32 product dy * x"
    _close(dx, dx_ref, f"rowdot_bwd dx {shape}")
    spare = torch.full((B, Kd), SENTINEL, device=DEV)
    for u in (Ug, None):
        dU2 = torch.full((B, R, Kd), float("nan"), device=DEV)
        _lib.call("vcg_rowdot_bwd", K.P(u), K.P(xg), K.P(dyg), K.P(dU2), None, B, R, Kd, K.stream())
        assert torch.equal(dU2.cpu(), dU_ref), "dx = NULL changed dU"
    assert (spare == SENTINEL).all(), "dx = NULL wrote to a dx buffer"


# ============================================================================ mul
@pytest.mark.parametrize("n", [4, 4 * (4096 * 256 + 1)], ids=["n4", "wraps"])
def test_mul_fwd(K, n):
    """out = a * b, bit-equal to torch fp32; the larger n is one float4 more than 4096 blocks of 256 threads cover
    in one pass, so the grid-stride loop wraps."""
    from vcg_hip import _lib
    g = torch.Generator().manual_seed(n % 1000 + 3)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    out = torch.full((n,), float("nan"), device=DEV)
    ag, bg = a.to(DEV), b.to(DEV)
    _lib.call("vcg_mul_fwd", K.P(ag), K.P(bg), K.P(out), n, K.stream())
    assert torch.equal(out.cpu(), a * b)


def test_mul_fwd_refuses_ragged_n(K):
    from vcg_hip import _lib
    from vcg_hip._lib import VcgError
    a = torch.ones(8, device=DEV)
    out = torch.full((8,), SENTINEL, device=DEV)
    with pytest.raises(VcgError, match=r"\(-1\).*multiple of 4"):
        _lib.call("vcg_mul_fwd", K.P(a), K.P(a), K.P(out), 6, K.stream())
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ============================================================================ LayerNorm + activation
def _ln_act_ref(x, gamma, beta, eps, act):
    y = F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
    return F.relu(y) if act == 1 else F.gelu(y) if act == 2 else y


def _ln_act_case(K, rows, D, act, eps):
    from vcg_hip import _lib
    g = torch.Generator().manual_seed(rows * 131 + D * 7 + act)
    # a mean of 100 over a spread of 3: E[x^2] - E[x]^2 in fp32 would lose the variance
    x = 3 * torch.randn(rows, D, generator=g) + 100
    gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.5
    ref64 = _ln_act_ref(x.double(), gamma.double(), beta.double(), eps, act)
    ref32 = _ln_act_ref(x, gamma, beta, eps, act)
    xg, gg, bg = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    out = torch.full((rows, D), float("nan"), device=DEV)
    _lib.call("vcg_ln_act_fwd", K.P(xg), K.P(gg), K.P(bg), K.P(out), rows, D, float(eps), act, K.stream())
    _close32(out, ref64, ref32, f"ln_act_fwd rows={rows} D={D} act={act} eps={eps:g}")


@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "relu", "gelu"])
@pytest.mark.parametrize("D", [1, 8, 63, 65, 96, 1024])
def test_ln_act_fwd(K, D, act):
    """act(LayerNorm(x) * gamma + beta) over 1 and 5 rows (5: a second block of 4 waves, one row in it); D = 1
    (variance 0), either side of one wave, and 16 strides of a wave."""
    for rows in (1, 5):
        _ln_act_case(K, rows, D, act, 1e-5)


def test_ln_act_fwd_small_eps(K):
    """eps = 1e-12 (BERT's): the eps argument reaches the kernel."""
    _ln_act_case(K, 5, 96, 2, 1e-12)
    from vcg_hip import _lib
    x = torch.tensor([[1.0, 1.0 + 2 ** -10, 1.0 - 2 ** -10, 1.0]])  # variance 4.8e-7: eps 1e-5 vs 1e-12 differ 4x
    one, zero = torch.ones(4), torch.zeros(4)
    out = torch.empty(1, 4, device=DEV)
    xg, og, zg = x.to(DEV), one.to(DEV), zero.to(DEV)
    _lib.call("vcg_ln_act_fwd", K.P(xg), K.P(og), K.P(zg), K.P(out), 1, 4, 1e-12, 0, K.stream())
    _close(out, _ln_act_ref(x.double(), one.double(), zero.double(), 1e-12, 0), "ln_act_fwd tiny variance eps=1e-12")


# ============================================================================ cross-attention
def _cross_ref(p, lang, vis, nh):
    """vcg_cross_attn_fwd as include/vcg_hip.h and the kernel's comment state it, in the dtype of its inputs."""
    B, T, H = vis.shape
    hd = H // nh
    l = _ln(p, "lang_norm", lang)
    t = (torch.arange(T, dtype=vis.dtype) / (T - 1)).unsqueeze(-1)
    v = _ln(p, "vision_norm", vis) + _lin(p, "frame_pos_encoding", t)
    q = _lin(p, "query_proj", l).view(B, 1, nh, hd).transpose(1, 2)
    k = _lin(p, "key_proj", v).view(B, T, nh, hd).transpose(1, 2)
    vv = _lin(p, "value_proj", v).view(B, T, nh, hd).transpose(1, 2)
    a = torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(hd), dim=-1)
    return _lin(p, "out_proj", (a @ vv).transpose(1, 2).reshape(B, H))


# (T, H, nh, B): minimum; hd = 9; production; hd = 1; T * H at the 2048 limit with H > 256 threads
CROSS_SHAPES = [(2, 4, 1, 1), (3, 72, 8, 2), (16, 128, 16, 3), (16, 128, 128, 2), (2, 1024, 16, 1)]


@pytest.mark.parametrize("shape", CROSS_SHAPES, ids=str)
def test_cross_attn_fwd(K, shape):
    from model.fusion.two_stream_window import CrossAttention
    from vcg_hip import _lib
    from vcg_hip.window import pack_cross_attn_weights
    T, H, nh, B = shape
    ca = _randomise(CrossAttention(H, nh), T * 1000 + H + nh)
    g = torch.Generator().manual_seed(T * 7 + H + B)
    lang, vis = torch.rand(B, H, generator=g), torch.rand(B, T, H, generator=g)  # post-ReLU-like inputs
    vis[torch.rand(B, T, H, generator=g) < 0.3] = 0.0
    ref64 = _cross_ref(_params(ca, F64), lang.double(), vis.double(), nh)
    ref32 = _cross_ref(_params(ca, torch.float32), lang, vis, nh)
    W = pack_cross_attn_weights(ca).to(DEV)
    assert W.numel() == _lib.query("vcg_cross_attn_weight_floats", H)
    out = torch.full((B, H), float("nan"), device=DEV)
    lg, vg = lang.to(DEV), vis.to(DEV)
    _lib.call("vcg_cross_attn_fwd", K.P(lg), K.P(vg), K.P(W), W.numel(), K.P(out), B, T, H, nh, K.stream())
    _close32(out, ref64, ref32, f"cross_attn_fwd {shape}")


# ============================================================================ window transformer
def _window_ref(p, emb, nh, n_layers=6):
    """vcg_window_attn_fwd as include/vcg_hip.h and the kernel's opening comment state it (6 pre-LN blocks with the
    window position encoding and window_pos_bias[h][j], final LayerNorm of the middle clip S / 2, the classifier
    chain), in the dtype of its inputs. -> logits, prob [B, 2]."""
    B, S, H = emb.shape
    hd, mid = H // nh, S // 2
    pos = ((torch.arange(S) - mid).to(emb.dtype) / (mid + 1e-6)).unsqueeze(-1)

    def heads(t):
        return t.view(B, S, nh, hd).permute(0, 2, 1, 3)
    x = emb
    for l in range(n_layers):
        pre = f"layers.{l}."
        n = _ln(p, pre + "attention_norm", x) + _lin(p, pre + "attention.position_encoding", pos)
        q, k, v = (heads(_lin(p, pre + "attention." + w, n)) for w in ("query", "key", "value"))
        sc = q @ k.transpose(-1, -2) / math.sqrt(hd) + p[pre + "attention.window_pos_bias"][:, :, :, :S]
        ctx = (torch.softmax(sc, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, S, H)
        x = x + _lin(p, pre + "attention.out_proj", ctx)
        h = _ln(p, pre + "ffn_norm", x)
        for i in (0, 3, 6):
            h = F.gelu(_lin(p, pre + f"ffn.{i}", h))
        x = x + _lin(p, pre + "ffn.9", h)
    x = _ln(p, "final_layer_norm", x[:, mid])
    for c in (0, 4, 8, 12):
        x = F.gelu(_ln(p, f"classifier.{c + 1}", _lin(p, f"classifier.{c}", x)))
    logits = _lin(p, "classifier.16", x)
    return logits, torch.softmax(logits, dim=-1)


def _window_module(H, nh, P, seed):
    """A StackedVideoChapterAttention with window_pos_bias of P entries per head (2w + 1 from the constructor; an
    even P by replacing the parameter), every parameter redrawn."""
    from model.fusion.stacked_window_self_attention import StackedVideoChapterAttention
    cfg = type("Config", (), {"hidden_size": H, "num_attention_heads": nh, "attention_probs_dropout_prob": 0.1,
                              "window_size": (P - 1) // 2})
    m = StackedVideoChapterAttention(cfg)
    if P % 2 == 0:
        for layer in m.layers:
            layer.attention.window_pos_bias = torch.nn.Parameter(torch.zeros(1, nh, 1, P))
    return _randomise(m, seed).eval()


# (H, S, nh, P, B), windows per workgroup (VCG_WINDOW_G; None: the library's choice, 1 at these batch sizes):
# H / 4 = 1: the last LayerNorm runs over one feature; production; P > S and a ragged last workgroup of one window;
# even S at the S * H = 2048 limit; 16 rows
WINDOW_SHAPES = [((4, 1, 1, 1, 1), None), ((128, 5, 16, 5, 3), None), ((64, 3, 8, 7, 11), "5"),
                 ((256, 8, 16, 9, 2), None), ((128, 16, 16, 16, 1), None)]


@pytest.mark.parametrize("shape,G", WINDOW_SHAPES, ids=lambda v: str(v) if isinstance(v, tuple) else f"G{v}")
def test_window_attn_fwd(K, shape, G, monkeypatch):
    """logits and prob of the whole window stack against fp64; prob = NULL is accepted and leaves the logits as
    they were."""
    from vcg_hip import _lib
    from vcg_hip.window import pack_window_weights
    if G is not None:
        monkeypatch.setenv("VCG_WINDOW_G", G)
    H, S, nh, P, B = shape
    m = _window_module(H, nh, P, H * 13 + S)
    emb = torch.randn(B, S, H, generator=torch.Generator().manual_seed(H + S * 17 + B))
    lg64, pr64 = _window_ref(_params(m, F64), emb.double(), nh)
    lg32, pr32 = _window_ref(_params(m, torch.float32), emb, nh)
    W = pack_window_weights(m).to(DEV)
    assert W.numel() == _lib.query("vcg_window_attn_weight_floats", H, nh, P)
    eg = emb.to(DEV)
    logits = torch.full((B, 2), float("nan"), device=DEV)
    prob = torch.full((B, 2), float("nan"), device=DEV)
    _lib.call("vcg_window_attn_fwd", K.P(eg), K.P(W), W.numel(), K.P(logits), K.P(prob), B, S, H, nh, P, K.stream())
    _close32(logits, lg64, lg32, f"window_attn_fwd logits {shape}")
    _close32(prob, pr64, pr32, f"window_attn_fwd prob {shape}")
    only = torch.full((B, 2), float("nan"), device=DEV)
    _lib.call("vcg_window_attn_fwd", K.P(eg), K.P(W), W.numel(), K.P(only), None, B, S, H, nh, P, K.stream())
    assert torch.equal(only, logits), "prob = NULL changed the logits"


def test_window_attn_depends_on_every_window(K, monkeypatch):
    """Five windows per workgroup: changing one window's clips changes that window's logits only (each window
    attends to its own keys)."""
    from vcg_hip import _lib
    from vcg_hip.window import pack_window_weights
    monkeypatch.setenv("VCG_WINDOW_G", "5")
    H, S, nh, P, B = 64, 3, 8, 7, 11
    m = _window_module(H, nh, P, 99)
    W = pack_window_weights(m).to(DEV)
    emb = torch.randn(B, S, H, generator=torch.Generator().manual_seed(4)).to(DEV)
    emb2 = emb.clone()
    emb2[0] += 1.0  # the first window of the first workgroup
    outs = []
    for e in (emb, emb2):
        logits = torch.full((B, 2), float("nan"), device=DEV)
        _lib.call("vcg_window_attn_fwd", K.P(e), K.P(W), W.numel(), K.P(logits), None, B, S, H, nh, P, K.stream())
        outs.append(logits)
    assert torch.equal(outs[0][1:], outs[1][1:]), "a window's logits depend on another window's clips"
    assert not torch.equal(outs[0][0], outs[1][0])


# ============================================================================ refusals
def test_window_attn_refusals(K):
    """S = 17, S * H = 2052 and P < S: VCG_ERR_INVALID with the message, before any launch (outputs untouched)."""
    from vcg_hip import _lib
    from vcg_hip._lib import VcgError
    for (H, S, nh, P), msg in (((4, 17, 1, 17), r"S must be in \[1, 16\]"), ((228, 9, 4, 9), "hidden must be <= 2048"),
                               ((32, 5, 4, 3), "window_pos_bias length must cover the window")):
        B = 2
        W = torch.zeros(_lib.query("vcg_window_attn_weight_floats", H, nh, P), device=DEV)
        emb = torch.zeros(B, S, H, device=DEV)
        logits = torch.full((B, 2), SENTINEL, device=DEV)
        prob = torch.full((B, 2), SENTINEL, device=DEV)
        with pytest.raises(VcgError, match=rf"vcg_window_attn_fwd failed \(-1\).*{msg}"):
            _lib.call("vcg_window_attn_fwd", K.P(emb), K.P(W), W.numel(), K.P(logits), K.P(prob), B, S, H, nh, P,
                      K.stream())
        torch.cuda.synchronize()
        assert (logits == SENTINEL).all() and (prob == SENTINEL).all()


def test_cross_attn_refusals(K):
    """T = 1 (the frame position t / (T - 1) is undefined) and T * H = 2052 > 2048."""
    from vcg_hip import _lib
    from vcg_hip._lib import VcgError
    for (T, H, nh), msg in (((1, 8, 2), r"T must be in \[2, 16\]"), ((3, 684, 4), "bad hidden size / heads")):
        B = 2
        W = torch.zeros(_lib.query("vcg_cross_attn_weight_floats", H), device=DEV)
        lang, vis = torch.zeros(B, H, device=DEV), torch.zeros(B, T, H, device=DEV)
        out = torch.full((B, H), SENTINEL, device=DEV)
        with pytest.raises(VcgError, match=rf"vcg_cross_attn_fwd failed \(-1\).*{msg}"):
            _lib.call("vcg_cross_attn_fwd", K.P(lang), K.P(vis), K.P(W), W.numel(), K.P(out), B, T, H, nh, K.stream())
        torch.cuda.synchronize()
        assert (out == SENTINEL).all()
