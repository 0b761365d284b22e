"""The kernels of KV-cached GPT generation (csrc/gpt_decode.hip) against the fp64 statements of tests/gpt_decode_ref.py.

Decode attention (B = 3, nh = 12, head dim 64; key counts p + 1 on either side of the per-wave strips of 8 / 4 keys,
the rounds of 32 / 16 and of the 4-deep unroll; the sequences of a batch have different len0):
  * bf16: relative Frobenius error of ctx against fp64 <= 2e-2 and <= 1.25 x the error of the causal fused kernel's row
    p on the same Q / K / V + 2e-3 (tests/test_gpu_gpt_kernels.py's measure);
  * fp32: within 2e-5 x max|ref|, the project's fp32 bound;
  * the appended K / V rows equal the qkv_new slices bit for bit, every other cache row keeps its sentinel (NaN bit
    patterns: a read of a row that is not a key would also poison ctx), bit-identical on a second run;
  * p >= Tcap and head dim != 64 are refused with nothing written.
Sampler (B = 4; V in {40478, 17, 8}, ldz = V rounded up to 8 with +1e30 in the pad columns; top_k in {0, 1, 3, 10, V};
temperature in {1.0, 0.7}): u at the midpoints of the helper's CDF steps wider than 1e-4, u = 0 and u = 1 - 2^-24 give
exactly the helper's token; ties at the k-th value are all kept and a tied entry is reached; greedy is the argmax,
lowest index on ties; the token (or the forced one) goes to column len0 + col_off of seq and nothing else changes.
Embedding at a position: tok[id] + pos[p], exactly.
Skinny GEMM (M in {1, 3, 16}, the five Linear / head shapes of GPT-base): see test_skinny_gemm.
"""
import numpy as np
import pytest
import torch

import gpt_decode_ref as ref
from bert_attn_ref import rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, NH, DH, H, TCAP = 3, 12, 64, 768, 520
KEY_COUNTS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512]


@pytest.fixture(scope="module", autouse=True)
def _init():
    from vcg_hip import _lib
    _lib.call("vcg_init", 0)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _attn_case(n, dtype):
    """key counts (n, n - 1, n - 2) (clamped at 1) through different len0 at one host step index t"""
    t = 1 if n >= 4 else 0
    counts = [n, max(1, n - 1), max(1, n - 2)]
    len0 = [c - 1 - t for c in counts]
    if n < 4:
        len0 = [n - 1, 0, max(0, n - 2)]
        counts = [l + 1 for l in len0]
    g = torch.Generator().manual_seed(1000 + n)
    qkv_new = (torch.randn(B, 3 * H, generator=g) * 1.5).to(dtype)
    kc = torch.full((B, NH, TCAP, DH), float("nan"), dtype=dtype)
    vc = torch.full((B, NH, TCAP, DH), float("nan"), dtype=dtype)
    for b, c in enumerate(counts):
        kc[b, :, :c - 1] = (torch.randn(NH, c - 1, DH, generator=g) * 1.5).to(dtype)
        vc[b, :, :c - 1] = (torch.randn(NH, c - 1, DH, generator=g) * 1.5).to(dtype)
    return qkv_new, kc, vc, len0, counts, t


def _attn_ref(qkv_new, kc, vc, counts):
    out = np.zeros((B, H))
    q3 = qkv_new.double().view(B, 3, NH, DH).numpy()
    for b, c in enumerate(counts):
        for h in range(NH):
            K = np.concatenate([kc[b, h, :c - 1].double().numpy(), q3[b, 1, h][None]])
            V = np.concatenate([vc[b, h, :c - 1].double().numpy(), q3[b, 2, h][None]])
            out[b, h * DH:(h + 1) * DH] = ref.attn_one_query(q3[b, 0, h], K, V, 0.125)
    return torch.from_numpy(out)


def _run_decode(qkv_new, kc, vc, len0, t):
    from vcg_hip.gpt_decode import attn_decode
    kd, vd = kc.to(DEV), vc.to(DEV)
    ctx = attn_decode(qkv_new.to(DEV), kd, vd, torch.tensor(len0, dtype=torch.int32, device=DEV), max(len0), t, NH)
    torch.cuda.synchronize()
    return ctx.cpu(), kd.cpu(), vd.cpu()


def _fused_rows(qkv_new, kc, vc, counts):
    """ctx row p of the causal fused kernel on full sequences holding the same keys (rows behind p: zeros, unseen)"""
    from vcg_hip.bert import attention_fwd
    L = max(counts)
    Lp = (L + 7) // 8 * 8
    qkv = torch.zeros(B * L + 8, 3 * H, dtype=torch.bfloat16)
    v3 = qkv[:B * L].view(B, L, 3, NH, DH)
    for b, c in enumerate(counts):
        v3[b, :c - 1, 1] = kc[b, :, :c - 1].permute(1, 0, 2)
        v3[b, :c - 1, 2] = vc[b, :, :c - 1].permute(1, 0, 2)
        v3[b, c - 1] = qkv_new[b].view(3, NH, DH)
    ctx, _ = attention_fwd(qkv.to(DEV), torch.ones(B, L, dtype=torch.int64, device=DEV), B, NH, L, Lp, DH, 0.125, 0.0,
                           1, True, causal=True)
    torch.cuda.synchronize()
    return torch.stack([ctx.cpu()[b * L + c - 1] for b, c in enumerate(counts)])


@pytest.mark.parametrize("n", KEY_COUNTS)
def test_decode_attention_bf16(n):
    qkv_new, kc, vc, len0, counts, t = _attn_case(n, torch.bfloat16)
    want = _attn_ref(qkv_new, kc, vc, counts)
    ctx, kd, vd = _run_decode(qkv_new, kc, vc, len0, t)
    assert torch.isfinite(ctx).all()
    e, e_fused = rel(ctx, want), rel(_fused_rows(qkv_new, kc, vc, counts), want)
    print(f"keys {counts}: decode err {e:.3e}, causal fused kernel row p {e_fused:.3e}")
    assert e <= 2e-2 and e <= 1.25 * e_fused + 2e-3
    _check_cache(qkv_new, kc, vc, kd, vd, counts)
    ctx2, kd2, vd2 = _run_decode(qkv_new, kc, vc, len0, t)
    assert torch.equal(_bits(ctx), _bits(ctx2)) and torch.equal(_bits(kd), _bits(kd2))


@pytest.mark.parametrize("n", KEY_COUNTS)
def test_decode_attention_fp32(n):
    qkv_new, kc, vc, len0, counts, t = _attn_case(n, torch.float32)
    want = _attn_ref(qkv_new, kc, vc, counts)
    ctx, kd, vd = _run_decode(qkv_new, kc, vc, len0, t)
    err = (ctx.double() - want).abs().max().item()
    print(f"keys {counts}: fp32 max err {err:.3e} (bound {2e-5 * want.abs().max().item():.3e})")
    assert err <= 2e-5 * want.abs().max().item()
    _check_cache(qkv_new, kc, vc, kd, vd, counts)
    ctx2, _, _ = _run_decode(qkv_new, kc, vc, len0, t)
    assert torch.equal(_bits(ctx), _bits(ctx2))


def _check_cache(qkv_new, kc, vc, kd, vd, counts):
    q3 = qkv_new.view(B, 3, NH, DH)
    for b, c in enumerate(counts):
        p = c - 1
        assert torch.equal(_bits(kd[b, :, p]), _bits(q3[b, 1])) and torch.equal(_bits(vd[b, :, p]), _bits(q3[b, 2]))
        for got, was in ((kd, kc), (vd, vc)):  # every other row, the sentinel rows included, bit for bit
            assert torch.equal(_bits(got[b, :, :p]), _bits(was[b, :, :p]))
            assert torch.equal(_bits(got[b, :, p + 1:]), _bits(was[b, :, p + 1:]))


def test_decode_attention_refusals():
    from vcg_hip import _lib
    from vcg_hip.gpt_decode import attn_decode
    qkv_new, kc, vc, len0, counts, t = _attn_case(5, torch.bfloat16)
    kd, vd, qd = kc.to(DEV), vc.to(DEV), qkv_new.to(DEV)
    l0 = torch.tensor(len0, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.VcgError, match="Tcap"):
        attn_decode(qd, kd, vd, l0, TCAP - 1, 1, NH)  # max_len0 + t = Tcap
    with pytest.raises(_lib.VcgError, match="head dim"):
        attn_decode(qd, kd, vd, l0, max(len0), t, NH, dh=32)
    torch.cuda.synchronize()
    assert torch.equal(_bits(kd.cpu()), _bits(kc)) and torch.equal(_bits(vd.cpu()), _bits(vc))


# ---------------------------------------------------------------------------------------------- sampler
SB = 4


def _logits(V, top_k, seed):
    """fp32 logits [4, ldz], +1e30 in the pad columns; row 2 has two more entries equal to its k-th largest value"""
    ldz = (V + 7) // 8 * 8
    g = torch.Generator().manual_seed(seed)
    z = torch.full((SB, ldz), 1e30, dtype=torch.float32)
    z[:, :V] = torch.randn(SB, V, generator=g) * 2
    k = max(1, min(top_k, V)) if top_k else 3
    kth = z[2, :V].topk(k).values[-1]
    below = torch.nonzero(z[2, :V] < kth)[:, 0]
    ties = below[[0, -1]] if below.numel() >= 2 else below
    z[2, ties] = kth
    return z, ties.tolist()


def _u_cases(z, V, temperature, top_k, ties, per_row=10):
    """[n, 4] uniforms: per row up to per_row midpoints of wide CDF steps (the tied entries' first), then u = 0 and
    u = 1 - 2^-24; and the tokens the helper gives for each"""
    rows = []
    for b in range(SB):
        us, toks = ref.midpoints(z[b, :V].numpy(), temperature, top_k)
        order = list(range(len(us)))
        if b == 2:
            order.sort(key=lambda i: toks[i] not in ties)
        pick = order[:2] + order[2::max(1, (len(order) - 2) // (per_row - 2))][:per_row - 2] if len(order) > 2 else order
        rows.append([us[i] for i in pick] or [0.5])
    n = max(len(r) for r in rows)
    U = np.array([[r[i % len(r)] for r in rows] for i in range(n)] + [[0.0] * SB, [1.0 - 2.0 ** -24] * SB])
    U32 = U.astype(np.float32)
    want = np.array([[ref.sample_ref(z[b, :V].numpy(), temperature, top_k, float(U32[i, b]))[0] for b in range(SB)]
                     for i in range(U32.shape[0])])
    return U32, want


# top_k in {0, 1, 3, 10, V} where it is a legal value (0 or 1..V: 10 does not exist at V = 8)
V_TOPK = [(V, k) for V in (40478, 17, 8) for k in sorted({0, 1, 3, 10, V}) if k <= V]


@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("V,top_k", V_TOPK)
def test_sampler_matches_helper(V, top_k, temperature):
    from vcg_hip.gpt_decode import sample
    z, ties = _logits(V, top_k, seed=V + 7 * top_k)
    if 0 < top_k < V and ties:
        _, keep = ref.keep_set(z[2, :V].numpy(), temperature, top_k)
        assert keep.sum() > top_k and all(keep[i] for i in ties)  # the kept count exceeds k
    U, want = _u_cases(z, V, temperature, top_k, ties)
    zd = z.to(DEV)
    got, probs = [], []
    for i in range(U.shape[0]):
        prob = torch.zeros(SB, device=DEV)
        got.append(sample(zd, V, temperature, top_k, False, torch.from_numpy(U[i]).to(DEV), prob=prob).cpu().numpy())
        probs.append(prob.cpu().numpy())
    got = np.stack(got)
    assert (got < V).all() and (got >= 0).all()  # never a pad column
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])
    if 0 < top_k < V and ties:
        assert any(tok in ties for tok in got[:, 2])  # a tied entry is reached
    for i in (0, U.shape[0] - 1):
        for b in range(SB):
            p = ref.sample_ref(z[b, :V].numpy(), temperature, top_k, float(U[i, b]))[1]
            assert abs(probs[i][b] - p) <= 1e-4 * p + 1e-12
    again = sample(zd, V, temperature, top_k, False, torch.from_numpy(U[0]).to(DEV)).cpu().numpy()
    assert np.array_equal(again, got[0])


@pytest.mark.parametrize("V", [40478, 17, 8])
def test_sampler_greedy_and_seq_column(V):
    from vcg_hip.gpt_decode import sample
    z, _ = _logits(V, 3, seed=V)
    hi = z[1, :V].max() + 1.0
    z[1, [V - 1, V // 2, 2]] = hi  # three equal maxima: the lowest index wins
    z[3, :V] = 0.25                # a constant row: index 0
    zd = z.to(DEV)
    want = np.array([ref.greedy_ref(z[b, :V].numpy()) for b in range(SB)])
    assert want[1] == 2 and want[3] == 0
    tcap, len0, col_off = 9, [0, 3, 5, 2], 2
    seq = torch.full((SB, tcap), -1, dtype=torch.int64, device=DEV)
    l0 = torch.tensor(len0, dtype=torch.int32, device=DEV)
    got = sample(zd, V, 0.7, 3, True, None, seq=seq, len0=l0, max_len0=5, col_off=col_off).cpu().numpy()
    assert np.array_equal(got, want)
    exp = torch.full((SB, tcap), -1, dtype=torch.int64)
    for b in range(SB):
        exp[b, len0[b] + col_off] = int(want[b])
    assert torch.equal(seq.cpu(), exp)
    # teacher forcing: the choice is returned, the forced token is what seq receives; no len0: column col_off
    forced = torch.tensor([[7, 70], [8, 80], [9, 90], [10, 100]], dtype=torch.int64, device=DEV)
    seq2 = torch.full((SB, tcap), -1, dtype=torch.int64, device=DEV)
    got2 = sample(zd, V, 1.0, 0, True, None, seq=seq2, col_off=4, forced=forced[:, 1:], forced_ld=2).cpu().numpy()
    assert np.array_equal(got2, want)
    exp2 = torch.full((SB, tcap), -1, dtype=torch.int64)
    exp2[:, 4] = forced[:, 1].cpu()
    assert torch.equal(seq2.cpu(), exp2)


def test_sampler_refusals():
    from vcg_hip import _lib
    from vcg_hip.gpt_decode import sample
    z = torch.zeros(SB, 24, device=DEV)
    u = torch.zeros(SB, device=DEV)
    seq = torch.full((SB, 6), -1, dtype=torch.int64, device=DEV)
    for kw in (dict(temperature=0.0), dict(top_k=18), dict(u=None), dict(seq=seq, max_len0=4, col_off=2)):
        args = dict(temperature=1.0, top_k=3, greedy=False, u=u)
        args.update(kw)
        with pytest.raises(_lib.VcgError):
            sample(z, 17, **args)
    torch.cuda.synchronize()
    assert bool((seq == -1).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_embed_at_position(dtype):
    from vcg_hip import _lib
    from vcg_hip.gpt_decode import gpt_embed_at
    V, P, Hh, tcap = 101, 40, 768, 24
    g = torch.Generator().manual_seed(3)
    tok, pos = torch.randn(V, Hh, generator=g), torch.randn(P, Hh, generator=g)
    seq = torch.randint(0, V, (4, tcap), generator=g)
    len0, t = [1, 7, 20, 3], 2
    out = gpt_embed_at(seq.to(DEV), torch.tensor(len0, dtype=torch.int32, device=DEV), max(len0), t, tok.to(DEV),
                       pos.to(DEV), dtype)
    want = torch.stack([tok[seq[b, len0[b] + t]] + pos[len0[b] + t] for b in range(4)]).to(dtype)
    assert torch.equal(_bits(out.cpu()), _bits(want))
    with pytest.raises(_lib.VcgError):  # position 22 + 2 is outside seq
        gpt_embed_at(seq.to(DEV), torch.tensor(len0, dtype=torch.int32, device=DEV), 22, t, tok.to(DEV), pos.to(DEV),
                     dtype)


# ---------------------------------------------------------------------------------------------- skinny GEMM
SKINNY_SHAPES = [(2304, 768), (768, 768), (3072, 768), (768, 3072), (40478, 768)]


def _skinny_case(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    W = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).to(DEV)
    b = (torch.randn(N, generator=g) * 0.1).to(DEV)
    return x, W, b, x.double() @ W.double().t()


@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("N,K", SKINNY_SHAPES)
def test_skinny_gemm(M, N, K):
    """Bias, bias + tanh-GELU and fp32-out forms: error against fp64 < 1.5 x the existing engine's on the same operands
    + 4e-3 (tests/test_gpu_wide.py's criterion; the existing engines: vcg_gemm on the wide-tile route for the bf16
    outputs, vcg_mlm_logits for the fp32 one); bit-identical on a second run; the census names the kernel."""
    from gpt_ref import new_gelu
    from vcg_hip import ops
    from vcg_hip.gpt_decode import gemm_skinny
    x, W, b, prod = _skinny_case(M, N, K)
    ld = (N + 7) // 8 * 8  # (a 16-B aligned row pitch for the existing engine at N = 40478)
    for act, ref in ((ops.ACT_NONE, prod + b.double()), (ops.ACT_GELU_TANH, new_gelu(prod + b.double()))):
        out = torch.zeros(M, ld, dtype=torch.bfloat16, device=DEV)
        ops.gemm_census_enable(True)
        gemm_skinny(x, W, b, act=act, out=out)
        torch.cuda.synchronize()
        keys = list(ops.gemm_census())
        ops.gemm_census_enable(False)
        assert keys == [f"gemm_skinny M={M} N={N} K={K}"], keys
        # (vcg_gemm needs N a multiple of 8: at N = 40478 it gets the same operands with two zero rows appended)
        Wp, bp = torch.zeros(ld, K, dtype=W.dtype, device=DEV), torch.zeros(ld, device=DEV)
        Wp[:N], bp[:N] = W, b
        old = ops.gemm(x, Wp, M, ld, K, K, K, bias=bp, act=act | ops.ACT_FLAG_WIDE)
        e_s, e_o = rel(out[:, :N], ref), rel(old[:, :N], ref)
        print(f"M={M} N={N} K={K} act={act}: skinny {e_s:.3e}, existing engine {e_o:.3e}")
        assert e_s < 1.5 * e_o + 4e-3
        assert not out[:, N:].any()  # the pitch columns are not written
        again = torch.zeros_like(out)
        gemm_skinny(x, W, b, act=act, out=again)
        assert torch.equal(_bits(out), _bits(again))
    z = gemm_skinny(x, W, None, f32_out=True)
    old = ops.mlm_logits(x, W)[:, :N]
    e_s, e_o = rel(z, prod), rel(old, prod)
    print(f"M={M} N={N} K={K} fp32 out: skinny {e_s:.3e}, existing engine {e_o:.3e}")
    assert z.dtype == torch.float32 and e_s < 1.5 * e_o + 4e-3
    assert torch.equal(_bits(z), _bits(gemm_skinny(x, W, None, f32_out=True)))


def test_skinny_gemm_refusals():
    from vcg_hip import _lib
    from vcg_hip.gpt_decode import gemm_skinny
    x, W, b, _ = _skinny_case(17, 64, 64)
    with pytest.raises(_lib.VcgError, match="1..16"):
        gemm_skinny(x, W, b)
    with pytest.raises(_lib.VcgError, match="multiple of 32"):
        gemm_skinny(x[:4, :48].contiguous(), W[:, :48].contiguous(), b)


def test_chain_routes_to_skinny_gemm():
    """bf16 with B <= 16: every Linear of a decode step and the head run on gemm_skinny; GptDecoder.skinny_gemm = False
    sends them to the existing engines, and the logits agree within the bf16 tolerance."""
    from vcg_hip import ops
    from vcg_hip.build import build_gpt_model
    from vcg_hip.gpt_decode import GptDecoder
    from vcg_hip.nn import OpenAIGPTConfig
    m = build_gpt_model(seed=123, device=DEV, precision="bf16", dropout=0.0, config=OpenAIGPTConfig(n_layer=2)).eval()
    x = torch.randint(0, 40478, (3, 6), generator=torch.Generator().manual_seed(1)).to(DEV)
    logits = {}
    for on in (True, False):
        GptDecoder.skinny_gemm = on
        try:
            dec = GptDecoder(m, 16)
            dec.prefill(x, None, steps=3, greedy=True)
            ops.gemm_census_enable(True)
            logits[on] = dec.step_logits(0)
            torch.cuda.synchronize()
            keys = ops.gemm_census()
            ops.gemm_census_enable(False)
        finally:
            GptDecoder.skinny_gemm = True
        skinny = {k: v for k, v in keys.items() if k.startswith("gemm_skinny")}
        if on:
            assert sum(skinny.values()) == 2 * 4 + 1 and len(keys) == len(skinny), keys
            assert "gemm_skinny M=3 N=40478 K=768" in skinny
        else:
            assert not skinny and keys, keys
    assert (logits[True] - logits[False]).abs().max().item() <= 5e-2
