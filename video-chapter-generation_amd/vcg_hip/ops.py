"""Tensor-level wrappers over the libvcg_hip C ABI.

Every wrapper checks device / dtype / contiguity, passes raw device pointers plus sizes, and
launches on torch's current HIP stream. There is no CPU or ATen fallback: a non-GPU tensor or
a missing library raises.
"""
import os

import torch

from . import _lib

F32, BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_GELU, ACT_TANH, ACT_GELU_BWD = 0, 1, 2, 3, 4
ACT_GELU_TANH, ACT_GELU_TANH_BWD = 5, 6  # the tanh form of GELU (OpenAIGPT's afn) and its derivative of a residual
ATTN_CAUSAL = 1  # vcg_bert_attn_*_ex / vcg_attn_softmax_fwd_ex flag (vcg_hip.h VCG_ATTN_CAUSAL)
ACT_FLAG_ROUND_PRE = 0x100  # gemm: round alpha*AB + bias to the storage dtype before the residual (vcg_hip.h)
ACT_FLAG_WIDE = 0x200  # gemm: the wide-tile engine (BERT's Linear layers, the downsample dgrad; vcg_hip.h VCG_ACT_FLAG_WIDE)
ACT_FLAG_F32_OUT = 0x400  # gemm (wide, bf16 operands): fp32 residual and output (vcg_hip.h VCG_ACT_FLAG_F32_OUT)
GRAD_F32 = 0x10  # ln_bwd dtype flag: fp32 dout / dres beside bf16 x / res / dx (vcg_hip.h VCG_GRAD_F32)

_DT = {torch.float32: F32, torch.bfloat16: BF16}


def dt_code(dtype):
    try:
        return _DT[dtype]
    except KeyError:
        raise TypeError(f"unsupported storage dtype {dtype}; expected float32 or bfloat16")


def torch_dtype(precision):
    return {"fp32": torch.float32, "bf16": torch.bfloat16}[precision]


def stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    """Device pointer of a contiguous GPU tensor (None passes NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libvcg_hip ops need GPU tensors (no CPU fallback)")
    return t.data_ptr()


def _chk(t, dtype=None, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be on the GPU (libvcg_hip has no CPU path)")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"{name} has dtype {t.dtype}, expected {dtype}")


def ws(nbytes, device):
    return torch.empty((max(int(nbytes), 4) + 3) // 4, dtype=torch.float32, device=device)


# ----------------------------------------------------------------------------- engine
def conv_out_hw(H, W, KH, KW, stride, pad):
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


TIMING_FAST_GEMM, TIMING_WGRAD, TIMING_GENERIC_GEMM, TIMING_PATCH_CONV, TIMING_WIDE_GEMM = 0, 1, 2, 3, 4


def gemm_census_enable(on):
    """Start (or stop) counting GEMM-class launches per (kernel, shape); clears the counts."""
    _lib.call("vcg_gemm_census_enable", int(bool(on)))


def gemm_census():
    """{"<kernel tag> M=.. N=.. K=..": launches} since gemm_census_enable(True)."""
    import ctypes
    out = {}
    for i in range(_lib.query("vcg_gemm_census_size")):
        buf = ctypes.create_string_buffer(256)
        n = ctypes.c_longlong()
        _lib.call("vcg_gemm_census_get", i, buf, 256, ctypes.addressof(n))
        out[buf.value.decode()] = n.value
    return out


def timing_enable(on):
    """Bracket every fast-GEMM / wgrad launch with HIP events (clears earlier records)."""
    _lib.call("vcg_timing_enable", int(bool(on)))


def timing_query(kernel_id):
    """(total ms, launches, algorithmic FLOPs) of the recorded launches of one kernel."""
    import ctypes
    ms, n, fl = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
    _lib.call("vcg_timing_query", int(kernel_id), ctypes.addressof(ms), ctypes.addressof(n), ctypes.addressof(fl))
    return ms.value, n.value, fl.value


def timing_roofline(kernel_id, peak_tflops, peak_gbs):
    """(total ms, ideal ms, algorithmic bytes, flops) of the recorded launches of one kernel; ideal = sum of
    max(flops / peak, bytes / HBM peak) per launch."""
    import ctypes
    ms, ideal, nb, fl = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    _lib.call("vcg_timing_roofline", int(kernel_id), float(peak_tflops), float(peak_gbs), ctypes.addressof(ms),
              ctypes.addressof(ideal), ctypes.addressof(nb), ctypes.addressof(fl))
    return ms.value, ideal.value, nb.value, fl.value


def stats_tiles(M):
    return _lib.query("vcg_conv_stats_tiles", M)


def stats_buffer(Cout, M, device):
    """BN statistics buffer of vcg_conv_fwd: float2 [Cout + 1][slots] — (mean, M2) per column and
    slot, then the count row (rows per slot; 0 = unused slot)."""
    return torch.empty((Cout + 1, stats_tiles(M), 2), dtype=torch.float32, device=device)


def conv_fwd(x, w, N, H, W, C, Cout, KH, KW, stride, pad, tsm_T=0, tsm_fold=0, stats=None, out=None):
    """x: NHWC [N,H,W,C]; w: [Cout,KH,KW,C] (same storage dtype). Returns y [N,OH,OW,Cout].
    stats: None or a stats_buffer(Cout, N*OH*OW)."""
    _chk(x, name="x")
    if stats is not None:
        OH_, OW_ = conv_out_hw(H, W, KH, KW, stride, pad)
        if stats.numel() < (Cout + 1) * stats_tiles(N * OH_ * OW_) * 2:
            raise ValueError("stats buffer too small: use ops.stats_buffer(Cout, M)")
    _chk(w, x.dtype, "w")
    OH, OW = conv_out_hw(H, W, KH, KW, stride, pad)
    y = out if out is not None else torch.empty((N, OH, OW, Cout), dtype=x.dtype, device=x.device)
    _lib.call("vcg_conv_fwd", dt_code(x.dtype), P(x), P(w), P(y), P(stats), N, H, W, C, Cout, KH, KW, stride, pad,
              tsm_T, tsm_fold, stream())
    return y


def conv_fwd_bias_act(x, w, bias, act, N, H, W, C, Cout, KH, KW, stride, pad, tsm_T=0, tsm_fold=0, out=None):
    """act(conv(x, w) + bias) (vcg_conv_fwd_bias_act): w carries a folded running-statistics BN, bias its shift."""
    _chk(x, name="x")
    _chk(w, x.dtype, "w")
    _chk(bias, torch.float32, "bias")
    OH, OW = conv_out_hw(H, W, KH, KW, stride, pad)
    y = out if out is not None else torch.empty((N, OH, OW, Cout), dtype=x.dtype, device=x.device)
    _lib.call("vcg_conv_fwd_bias_act", dt_code(x.dtype), P(x), P(w), P(bias), int(act), P(y), N, H, W, C, Cout, KH,
              KW, stride, pad, tsm_T, tsm_fold, stream())
    return y


def conv_dgrad(dy, wt, N, H, W, C, Cout, KH, KW, stride, pad, out=None):
    """dy: NHWC [N,OH,OW,Cout]; wt: [C,KH,KW,Cout]. Returns dx [N,H,W,C]."""
    _chk(dy, name="dy")
    _chk(wt, dy.dtype, "wt")
    dx = out if out is not None else torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    _lib.call("vcg_conv_dgrad", dt_code(dy.dtype), P(dy), P(wt), P(dx), N, H, W, C, Cout, KH, KW, stride, pad,
              stream())
    return dx


def conv_dgrad_bwd(dy, wt, N, H, W, C, Cout, KH, KW, stride, pad, tsm_T=0, tsm_fold=0, res=None, res_stride=1,
                   bits=None, y=None, mean=None, invstd=None, mscale=None, mshift=None, y2=None, mean2=None, invstd2=None, sums=None,
                   sum_gx2=None, dgamma=None, dbeta=None, dgamma2=None, dbeta2=None, out=None, workspace=None, a2=None,
                   pg=None):
    """Conv input gradient fused with the trunk backward's next steps (vcg_conv_dgrad_bwd, igemm.h BwdEpi):
    g = mask(tsm_adjoint(dgrad) + res) and the BN-backward sums of g against y (sums [2, C] = sum_g,
    sum_gx) and y2 (res_stride 2: res is the compact [N, H/2, W/2, C] gradient of a 1x1 / stride-2 conv) (sum_gx2 [C]); dgamma/dbeta (dgamma2/dbeta2) accumulate. Returns g, or None where the
    fused engine does not apply (fp32 / unsupported shape): the caller then runs the unfused ops.
    a2 (bf16 [N, H, W, a2_c], a2_c 64) with pg (f32 [C, a2_c]): also pg = g^T a2 from the stored g tiles; then
    the return value is (g, done) -- done False where that product does not apply (g computed without it)."""
    OH, OW = conv_out_hw(H, W, KH, KW, stride, pad)
    _chk(dy, None, "dy")
    assert dy.numel() == N * OH * OW * Cout and wt.numel() == C * KH * KW * Cout
    g = out if out is not None else torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    nbytes = _lib.query("vcg_conv_dgrad_bwd_ws_bytes", C, Cout, KH, KW)
    if workspace is None or workspace.numel() * 4 < nbytes:
        workspace = ws(nbytes, dy.device)
    for t in (res, y, y2):
        if t is not None:
            _chk(t, dy.dtype)
            assert t.numel() == (N * ((H + 1) // 2) * ((W + 1) // 2) * C if t is res and res_stride == 2
                                 else N * H * W * C)
    def call(a2_, pg_, pws_):
        return _lib.query("vcg_conv_dgrad_bwd", dt_code(dy.dtype), P(dy), P(wt), P(g), N, H, W, C, Cout, KH, KW,
                          stride, pad, tsm_T, tsm_fold, P(res), int(res_stride), P(bits), P(y), P(mean), P(invstd),
                          P(mscale), P(mshift), P(y2), P(mean2), P(invstd2), P(workspace), workspace.numel() * 4,
                          P(sums[0]) if sums is not None else None, P(sums[1]) if sums is not None else None,
                          P(dgamma), P(dbeta), P(sum_gx2), P(dgamma2), P(dbeta2), P(a2_),
                          a2_.shape[-1] if a2_ is not None else 0, P(pg_), P(pws_),
                          pws_.numel() * 4 if pws_ is not None else 0, stream())
    done = False
    rc = -2
    if a2 is not None:
        _chk(a2, torch.bfloat16, "a2")
        _chk(pg, torch.float32, "pg")
        assert a2.numel() == N * H * W * a2.shape[-1] and pg.numel() == C * a2.shape[-1]
        pws = ws(_lib.query("vcg_conv_dgrad_bwd_p_ws_bytes", C, a2.shape[-1]), dy.device)
        rc = call(a2, pg, pws)
        done = rc == 0
    if rc == -2:  # VCG_ERR_UNSUPPORTED (with a2: retried without the P product)
        rc = call(None, None, None)
    if rc == -2:
        return (None, False) if a2 is not None else None
    if rc != 0:
        raise _lib.VcgError(f"vcg_conv_dgrad_bwd failed ({rc}): {_lib.last_error()}")
    return (g, done) if a2 is not None else g


def bn_apply_colsum(y, scale, shift, C, relu=True):
    """(bn_apply(y, scale, shift, relu), its column sums f32 [C]) in one pass (vcg_bn_apply_colsum, bf16)."""
    _chk(y, torch.bfloat16, "y")
    out = torch.empty_like(y)
    cs = torch.empty(C, dtype=torch.float32, device=y.device)
    P_ = y.numel() // C
    w = ws(_lib.query("vcg_bn_apply_colsum_ws_bytes", P_, C), y.device)
    _lib.call("vcg_bn_apply_colsum", P(y), P(scale), P(shift), int(relu), P(out), P(cs), P(w), w.numel() * 4, P_, C,
              stream())
    return out, cs


def bn_apply_gram(y, scale, shift, C, mean, invstd):
    """(relu(bn_apply(y)), its column sums f32 [C], its Gram matrix out^T out f32 [C, C], and g64: the same Gram
    matrix and column sums accumulated centred per channel, with the centres, double [C * C + 2 C]) in one pass
    (vcg_bn_apply_gram, bf16, C in 64 / 128 / 256; mean / invstd: the BN statistics scale / shift fold; g64 is what
    bn_stats_from_gram reads)."""
    _chk(y, torch.bfloat16, "y")
    out = torch.empty_like(y)
    cs = torch.empty(C, dtype=torch.float32, device=y.device)
    gram = torch.empty((C, C), dtype=torch.float32, device=y.device)
    g64 = torch.empty(C * C + 2 * C, dtype=torch.float64, device=y.device)
    P_ = y.numel() // C
    w = ws(_lib.query("vcg_bn_apply_gram_ws_bytes", P_, C), y.device)
    _lib.call("vcg_bn_apply_gram", P(y), P(scale), P(shift), P(mean), P(invstd), P(out), P(cs), P(gram), P(g64),
              P(w), w.numel() * 4, P_, C, stream())
    return out, cs, gram, g64


def bn_stats_from_gram(g64, w, M, N, C, stats):
    """BN statistics of x w^T (w bf16 [N, C]) from x's centred (Gram matrix, column sums, centres) g64 [C * C + 2 C]
    of bn_apply_gram into a stats_buffer(N, M) (vcg_bn_stats_from_gram; one used slot, for bn_finalize)."""
    _chk(w, torch.bfloat16, "w")
    _chk(g64, torch.float64, "g64")
    assert g64.numel() == C * C + 2 * C
    _lib.call("vcg_bn_stats_from_gram", P(g64), P(w), M, N, C, P(stats), stats.shape[1], stream())
    return stats


def bn_finalize_from_gram(g64, w, M, N, C, gamma, beta, mean, invstd, scale, shift, running_mean=None,
                          running_var=None, momentum=0.1, eps=1e-5, w32=None, wfold=None):
    """bn_stats_from_gram + bn_finalize (+ weight_fold of the f32 master weight w32 [N, C] by the new scale into wfold,
    bf16) in one launch (vcg_bn_finalize_from_gram; the same values as the three calls). C <= 256, C % 16 == 0."""
    _chk(w, torch.bfloat16, "w")
    _chk(g64, torch.float64, "g64")
    assert g64.numel() == C * C + 2 * C and C <= 256 and C % 16 == 0
    if w32 is not None:
        _chk(w32, torch.float32, "w32")
        _chk(wfold, torch.bfloat16, "wfold")
        assert w32.numel() == N * C and wfold.numel() == N * C
    _lib.call("vcg_bn_finalize_from_gram", P(g64), P(w), M, N, C, P(gamma), P(beta), P(mean), P(invstd), P(scale),
              P(shift), P(running_mean), P(running_var), float(momentum), float(eps), P(w32), P(wfold), stream())


def conv1x1_stats(x, w, stats, M, N, K):
    """BatchNorm statistics of x [M, K] @ w [N, K]^T without storing the product (vcg_conv1x1_stats). False where
    the fused engine does not apply."""
    _chk(x, torch.bfloat16, "x")
    _chk(w, torch.bfloat16, "w")
    rc = _lib.query("vcg_conv1x1_stats", P(x), P(w), P(stats), M, N, K, stream())
    if rc == -2:
        return False
    if rc != 0:
        raise _lib.VcgError(f"vcg_conv1x1_stats failed ({rc}): {_lib.last_error()}")
    return True


def bn_bwd_sumgx_from_wgrad(Pg, w, K, C, mean, invstd, sum_g, sum_gx, dgamma=None):
    """sum_gx of a BN whose input y3 = a2 w^T was not stored, from Pg = g^T a2 (vcg_bn_bwd_sumgx_from_wgrad)."""
    _chk(Pg, torch.float32, "Pg")
    _chk(w, torch.bfloat16, "w")
    _lib.call("vcg_bn_bwd_sumgx_from_wgrad", P(Pg), P(w), K, C, P(mean), P(invstd), P(sum_g), P(sum_gx), P(dgamma),
              stream())


def conv1x1_bn_res_relu(x, wfold, bias, res, M, N, K, res_scale=None, res_shift=None):
    """(out, bits): relu(bf16(x @ wfold^T + bias) + res') and its ReLU mask bits (vcg_conv1x1_bn_res_relu), res' =
    res or res * res_scale + res_shift per column; None where the fused engine does not apply."""
    _chk(x, torch.bfloat16, "x")
    _chk(res, torch.bfloat16, "res")
    out = torch.empty_like(res)
    bits = torch.empty(res.numel() // 8, dtype=torch.uint8, device=res.device)
    rc = _lib.query("vcg_conv1x1_bn_res_relu", P(x), P(wfold), P(bias), P(res), P(res_scale), P(res_shift), P(out),
                    P(bits), M, N, K, stream())
    if rc == -2:
        return None
    if rc != 0:
        raise _lib.VcgError(f"vcg_conv1x1_bn_res_relu failed ({rc}): {_lib.last_error()}")
    return out, bits


def bn_bwd_fold_weights(wt, N, K, mean, invstd, gamma, sum_g, sum_gx, count):
    """(wfold [N, 2K] bf16, bias [N] f32) of a batch-statistics BN backward folded into the dgrad whose B operand is
    wt [N, K] (vcg_bn_bwd_fold_weights)."""
    _chk(wt, torch.bfloat16, "wt")
    wfold = torch.empty((N, 2 * K), dtype=torch.bfloat16, device=wt.device)
    bias = torch.empty(N, dtype=torch.float32, device=wt.device)
    _lib.call("vcg_bn_bwd_fold_weights", P(wt), N, K, P(mean), P(invstd), P(gamma), P(sum_g), P(sum_gx),
              float(1.0 / count), P(wfold), P(bias), stream())
    return wfold, bias


def conv_dgrad_bwd_bnfold(g, yg, wfold, bias, N, H, W, C, Cout, y=None, mean=None, invstd=None, mscale=None,
                          mshift=None, sums=None, dgamma=None, dbeta=None, out=None, workspace=None, Ky=None):
    """Input gradient of a 1x1 conv whose output gradient is the folded BN backward (vcg_conv_dgrad_bwd_bnfold; the
    light epilogue of conv_dgrad_bwd): one GEMM over [g | yg], yg = the BN input y (Ky = Cout, bn_bwd_fold_weights) or
    the conv's input a2 (Ky = C, bn_bwd_fold_weights_a2). Returns the masked gradient, or None where the engine does
    not apply."""
    Ky = Cout if Ky is None else Ky
    _chk(g, torch.bfloat16, "g")
    _chk(yg, torch.bfloat16, "yg")
    assert g.numel() == N * H * W * Cout and yg.numel() == N * H * W * Ky and wfold.numel() == C * (Cout + Ky)
    gout = out if out is not None else torch.empty((N, H, W, C), dtype=g.dtype, device=g.device)
    nbytes = _lib.query("vcg_conv_dgrad_bwd_ws_bytes", C, Cout + Ky, 1, 1)
    if workspace is None or workspace.numel() * 4 < nbytes:
        workspace = ws(nbytes, g.device)
    rc = _lib.query("vcg_conv_dgrad_bwd_bnfold", P(g), P(yg), int(Ky), P(wfold), P(bias), P(gout), N, H, W, C, Cout, P(y),
                    P(mean), P(invstd), P(mscale), P(mshift), P(workspace), workspace.numel() * 4,
                    P(sums[0]) if sums is not None else None, P(sums[1]) if sums is not None else None, P(dgamma),
                    P(dbeta), stream())
    if rc == -2:
        return None
    if rc != 0:
        raise _lib.VcgError(f"vcg_conv_dgrad_bwd_bnfold failed ({rc}): {_lib.last_error()}")
    return gout


def bn_bwd_fold_weights_a2(wt, C, K, invstd, gamma, sum_g, sum_gx, count, colsum_a):
    """(wfold [C, K + C] bf16, bias [C] f32) of the BN backward folded into the dgrad with the conv input a2 as the
    second source (vcg_bn_bwd_fold_weights_a2)."""
    _chk(wt, torch.bfloat16, "wt")
    wfold = torch.empty((C, K + C), dtype=torch.bfloat16, device=wt.device)
    bias = torch.empty(C, dtype=torch.float32, device=wt.device)
    _lib.call("vcg_bn_bwd_fold_weights_a2", P(wt), C, K, P(invstd), P(gamma), P(sum_g), P(sum_gx), float(1.0 / count),
              P(colsum_a), P(wfold), P(bias), stream())
    return wfold, bias


def bn_bwd_fold_wgrad_a2(Pg, G, w3, K, C, mean, invstd, gamma, sum_g, sum_gx, count, colsum_a, dw, accumulate=True):
    """dw [K, C] (+)= A Pg + B (w3 G) + Cc colsum_a (vcg_bn_bwd_fold_wgrad_a2)."""
    for t, n in ((Pg, "Pg"), (G, "G"), (w3, "w3"), (dw, "dw")):
        _chk(t, torch.float32, n)
    _lib.call("vcg_bn_bwd_fold_wgrad_a2", P(Pg), P(G), P(w3), K, C, P(mean), P(invstd), P(gamma), P(sum_g), P(sum_gx),
              float(1.0 / count), P(colsum_a), P(dw), int(accumulate), stream())


def conv_wgrad_bnfold(x, g, yg, mean, invstd, gamma, sum_g, sum_gx, count, colsum_x, dw, N, H, W, C, Cout,
                      accumulate=True, workspace=None):
    """dw [Cout, C] (+)= weight gradient of a 1x1 conv over x whose output gradient is the folded BN backward
    (vcg_conv_wgrad_bnfold). Returns False where the engine does not apply."""
    _chk(x, torch.bfloat16, "x")
    _chk(dw, torch.float32, "dw")
    nbytes = _lib.query("vcg_conv_wgrad_bnfold_ws_bytes", N, H, W, C, Cout)
    if workspace is None or workspace.numel() * 4 < nbytes:
        workspace = ws(nbytes, x.device)
    rc = _lib.query("vcg_conv_wgrad_bnfold", P(x), P(g), P(yg), P(mean), P(invstd), P(gamma), P(sum_g), P(sum_gx),
                    float(1.0 / count), P(colsum_x), P(dw), int(accumulate), P(workspace), workspace.numel() * 4, N, H,
                    W, C, Cout, stream())
    if rc == -2:
        return False
    if rc != 0:
        raise _lib.VcgError(f"vcg_conv_wgrad_bnfold failed ({rc}): {_lib.last_error()}")
    return True


def conv_wgrad(x, dy, dw, N, H, W, C, Cin, Cout, KH, KW, stride, pad, tsm_T=0, tsm_fold=0, accumulate=True,
               workspace=None):
    """dw (fp32 OIHW [Cout,Cin,KH,KW]) += wgrad. x: NHWC with C (padded) channels."""
    _chk(x, name="x")
    _chk(dy, x.dtype, "dy")
    _chk(dw, torch.float32, "dw")
    nbytes = _lib.query("vcg_conv_wgrad_ws_bytes", dt_code(x.dtype), N, H, W, C, Cout, KH, KW, stride, pad)
    if workspace is None or workspace.numel() * 4 < nbytes:
        workspace = ws(nbytes, x.device)
    _lib.call("vcg_conv_wgrad", dt_code(x.dtype), P(x), P(dy), P(dw), int(accumulate), P(workspace),
              workspace.numel() * 4, N, H, W, C, Cin, Cout, KH, KW, stride, pad, tsm_T, tsm_fold, stream())
    return workspace


def conv_wgrad_ws_bytes(dtype, N, H, W, C, Cout, KH, KW, stride, pad):
    return _lib.query("vcg_conv_wgrad_ws_bytes", dt_code(dtype), N, H, W, C, Cout, KH, KW, stride, pad)


def gemm(A, B, M, N, K, lda, ldb, transA=False, transB=False, out=None, ldc=None, bias=None, act=ACT_NONE,
         residual=None, ldr=None, aux=None, alpha=1.0):
    """C[M,N] = act(alpha * op(A) @ op(B)^T + bias (+ residual)). A/B/C share the storage dtype.
    transA=False: A is [M][lda]; True: A is [K][lda]. transB=False: B is [N][ldb]; True: [K][ldb]."""
    if out is None:
        out = torch.empty((M, N), dtype=A.dtype, device=A.device)
        ldc = N
    ldc = ldc if ldc is not None else N
    _lib.call("vcg_gemm", dt_code(A.dtype), int(transA), int(transB), M, N, K, P(A), lda, P(B), ldb, P(out), ldc,
              P(bias), act, P(residual), ldr if ldr is not None else ldc, P(aux), float(alpha), stream())
    return out


def gemm_batched(A, B, C, M, N, K, lda, ldb, ldc, a_so, a_si, b_so, b_si, c_so, c_si, batch_outer, batch_inner,
                 transA=False, transB=False, bias=None, act=ACT_NONE, alpha=1.0):
    _lib.call("vcg_gemm_batched", dt_code(A.dtype), int(transA), int(transB), M, N, K, P(A), lda, a_so, a_si, P(B),
              ldb, b_so, b_si, P(C), ldc, c_so, c_si, batch_outer, batch_inner, P(bias), act, float(alpha), stream())
    return C


def gemm_splitk(A, B, out, M, N, K, lda, ldb, transA=False, transB=False, accumulate=True, workspace=None):
    """out (fp32 [M,N]) (+)= op(A) @ op(B)^T, split over K."""
    _chk(out, torch.float32, "out")
    nbytes = _lib.query("vcg_gemm_splitk_ws_bytes", dt_code(A.dtype), M, N, K)
    if workspace is None or workspace.numel() * 4 < nbytes:
        workspace = ws(nbytes, A.device)
    _lib.call("vcg_gemm_splitk", dt_code(A.dtype), int(transA), int(transB), M, N, K, P(A), lda, P(B), ldb, P(out),
              int(accumulate), P(workspace), workspace.numel() * 4, stream())
    return workspace


# ----------------------------------------------------------------------------- vision
def bn_finalize(stats, mtiles, M, C, gamma, beta, mean, invstd, scale, shift, running_mean=None, running_var=None,
                momentum=0.1, eps=1e-5):
    _lib.call("vcg_bn_finalize", P(stats), mtiles, M, C, P(gamma), P(beta), P(mean), P(invstd), P(scale), P(shift),
              P(running_mean), P(running_var), float(momentum), float(eps), stream())


def bn_eval_params(gamma, beta, rm, rv, eps, C, mean, invstd, scale, shift):
    _lib.call("vcg_bn_eval_params", P(gamma), P(beta), P(rm), P(rv), float(eps), C, P(mean), P(invstd), P(scale),
              P(shift), stream())


def bn_apply(y, scale, shift, C, relu, res=None, rscale=None, rshift=None, out=None, bits=False):
    """act(y*scale + shift [+ res*rscale + rshift | + res]). bits=True also returns the ReLU mask
    bits of the output (one byte per 16-B vector) for the backward (mask mode 2)."""
    out = out if out is not None else torch.empty_like(y)
    b = torch.empty(y.numel() * y.element_size() // 16, dtype=torch.uint8, device=y.device) if bits else None
    _lib.call("vcg_bn_apply", dt_code(y.dtype), P(y), P(scale), P(shift), P(res), P(rscale), P(rshift), int(relu),
              P(out), P(b), y.numel() // C, C, stream())
    return (out, b) if bits else out


def _mask_mode(mask, mbits, mscale):
    if mbits is not None:
        return 2
    if mscale is not None:
        return 3
    return 1 if mask is not None else 0


def bn_bwd_reduce(dout, mask, y, mean, invstd, C, sum_g, sum_gx, dgamma=None, dbeta=None, workspace=None,
                  mbits=None, mscale=None, mshift=None):
    """Per-channel sums of g and g*xhat, g = dout masked by the ReLU: `mask` tensor (> 0), `mbits`
    (from bn_apply(bits=True)) or the affine recompute fma(y, mscale, mshift) > 0."""
    Pn = y.numel() // C
    nbytes = _lib.query("vcg_bn_bwd_ws_bytes", Pn, C)
    if workspace is None or workspace.numel() * 4 < nbytes:
        workspace = ws(nbytes, y.device)
    _lib.call("vcg_bn_bwd_reduce", dt_code(y.dtype), P(dout), _mask_mode(mask, mbits, mscale), P(mask), P(mbits),
              P(mscale), P(mshift), P(y), P(mean), P(invstd), Pn, C, P(workspace), workspace.numel() * 4, P(sum_g),
              P(sum_gx), P(dgamma), P(dbeta), 1, stream())
    return workspace


def bn_bwd_apply(dout, mask, y, mean, invstd, gamma, sum_g, sum_gx, C, train_stats, gout=None, out=None,
                 mbits=None, mscale=None, mshift=None):
    Pn = y.numel() // C
    dy = out if out is not None else torch.empty_like(y)
    _lib.call("vcg_bn_bwd_apply", dt_code(y.dtype), P(dout), _mask_mode(mask, mbits, mscale), P(mask), P(mbits),
              P(mscale), P(mshift), P(y), P(mean), P(invstd), P(gamma), P(sum_g), P(sum_gx), Pn, int(train_stats),
              P(dy), P(gout), Pn, C, stream())
    return dy


def bn_bwd_apply_dual(g, y, mean, invstd, gamma, sum_g, sum_gx, yd, mean_d, invstd_d, gamma_d, sum_g_d, sum_gx_d,
                      C):
    """Batch-stat BN backward applies of two BNs on one (masked) gradient g: (dy, dyd), g read once."""
    Pn = y.numel() // C
    dy, dyd = torch.empty_like(y), torch.empty_like(yd)
    _lib.call("vcg_bn_bwd_apply_dual", dt_code(y.dtype), P(g), P(y), P(mean), P(invstd), P(gamma), P(sum_g),
              P(sum_gx), P(yd), P(mean_d), P(invstd_d), P(gamma_d), P(sum_g_d), P(sum_gx_d), Pn, P(dy), P(dyd), Pn, C,
              stream())
    return dy, dyd


def maxpool_fwd(x, N, H, W, C):
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((N, OH, OW, C), dtype=x.dtype, device=x.device)
    idx = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=x.device)
    _lib.call("vcg_maxpool_fwd", dt_code(x.dtype), P(x), P(y), P(idx), N, H, W, C, stream())
    return y, idx


def maxpool_bwd(dy, idx, N, H, W, C):
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    _lib.call("vcg_maxpool_bwd", dt_code(dy.dtype), P(dy), P(idx), P(dx), N, H, W, C, stream())
    return dx


def maxpool_bwd_bn(dy, idx, N, H, W, C, y, mean, invstd, mscale, mshift, sums, dgamma=None, dbeta=None,
                   store_g=True):
    """maxpool backward + the stem BN + ReLU mask + BN-backward sums (sums [2, C] = sum_g, sum_gx). Returns the
    masked gradient g, or None with store_g=False (sums only: maxpool_bwd_bn_apply recomputes g)."""
    g = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device) if store_g else None
    w = ws(_lib.query("vcg_maxpool_bwd_bn_ws_bytes", C), dy.device)
    _lib.call("vcg_maxpool_bwd_bn", dt_code(dy.dtype), P(dy), P(idx), P(g), N, H, W, C, P(y), P(mean), P(invstd),
              P(mscale), P(mshift), P(w), w.numel() * 4, P(sums[0]), P(sums[1]), P(dgamma), P(dbeta), stream())
    return g


def maxpool_bwd_bn_sums_pooled(dy, mp, idx, y, N, H, W, C, mean, invstd, mscale, mshift, sums, dgamma=None,
                               dbeta=None):
    """The stem BN-backward sums of maxpool_bwd_bn(store_g=False) from the pooled activation mp (no pass over the
    pre-pool y [N, H, W, C], which -- with the argmax bytes idx -- is read only for channels with a zero or tiny BN
    weight; vcg_maxpool_bwd_bn_sums_pooled)."""
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert tuple(mp.shape) == (N, OH, OW, C) and idx.shape == mp.shape and tuple(y.shape) == (N, H, W, C)
    w = ws(_lib.query("vcg_maxpool_bwd_bn_ws_bytes", C), dy.device)
    _lib.call("vcg_maxpool_bwd_bn_sums_pooled", dt_code(dy.dtype), P(dy), P(mp), P(idx), P(y), N, H, W, C, P(mean),
              P(invstd), P(mscale), P(mshift), P(w), w.numel() * 4, P(sums[0]), P(sums[1]), P(dgamma), P(dbeta),
              stream())


def maxpool_bwd_bn_apply(dy, idx, N, H, W, C, y, mean, invstd, mscale, mshift, gamma, sums, count, train_stats):
    """The stem's BN-backward apply on g = mask(maxpool_bwd(dy)) recomputed in the same pass (sums from
    maxpool_bwd_bn(store_g=False)): returns the gradient of the stem conv output y."""
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    _lib.call("vcg_maxpool_bwd_bn_apply", dt_code(dy.dtype), P(dy), P(idx), P(dx), N, H, W, C, P(y), P(mean),
              P(invstd), P(mscale), P(mshift), P(gamma), P(sums[0]), P(sums[1]), int(count), int(bool(train_stats)),
              stream())
    return dx


def stem_bwd_fused(dy, idx, y, x, N, H, W, mean, invstd, mscale, mshift, gamma, sums, count, train_stats, dw,
                   accumulate=True):
    """The stem backward after the max-pool in one pass (bf16): maxpool_bwd_bn_apply's dy0 contracted with the
    pair-packed frames x [N][2H][2W][4] into dw [64][3][7][7] (vcg_stem_bwd_fused; dy0 is never stored)."""
    for t, n in ((dy, "dy"), (y, "y"), (x, "x")):
        _chk(t, torch.bfloat16, n)
    _chk(dw, torch.float32, "dw")
    assert tuple(y.shape) == (N, H, W, 64) and tuple(x.shape) == (N, 2 * H, 2 * W, 4) and dw.numel() == 64 * 147
    assert tuple(dy.shape) == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64) and idx.shape == dy.shape
    w = ws(_lib.query("vcg_stem_bwd_fused_ws_bytes"), dy.device)
    _lib.call("vcg_stem_bwd_fused", P(dy), P(idx), P(y), P(x), N, H, W, P(mean), P(invstd), P(mscale), P(mshift),
              P(gamma), P(sums[0]), P(sums[1]), int(count), int(bool(train_stats)), P(w), w.numel() * 4, P(dw),
              int(bool(accumulate)), stream())


def stem_bwd_fused_fits(N, H, W):
    """stem_bwd_fused takes a [N][H][W][64] conv output: every operand below 4 GB (32-bit buffer offsets; host-side
    predicate of the library, vcg_stem_bwd_fused_fits)."""
    return bool(_lib.query("vcg_stem_bwd_fused_fits", int(N), int(H), int(W)))


def bn_relu_maxpool(y, scale, shift, N, H, W, C):
    """maxpool3x3/2(relu(y * scale + shift)) with the activation rounded to y's dtype (the values and argmax of
    bn_apply + maxpool_fwd, without the activation tensor). Returns (pooled, idx)."""
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((N, OH, OW, C), dtype=y.dtype, device=y.device)
    idx = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=y.device)
    _lib.call("vcg_bn_relu_maxpool", dt_code(y.dtype), P(y), P(scale), P(shift), P(out), P(idx), N, H, W, C, stream())
    return out, idx


def avgpool_fwd(x, N, HW, C):
    y = torch.empty((N, C), dtype=torch.float32, device=x.device)
    _lib.call("vcg_avgpool_fwd", dt_code(x.dtype), P(x), P(y), N, HW, C, stream())
    return y


def avgpool_bwd(dy, N, HW, C, dtype):
    dx = torch.empty((N, HW, C), dtype=dtype, device=dy.device)
    _lib.call("vcg_avgpool_bwd", dt_code(dtype), P(dy), P(dx), N, HW, C, stream())
    return dx


IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def stem_cpad(dtype):
    """Channels of the stem's NHWC input: 4 (RGB0; bf16: the pair-packed stem, two stride-2 taps per 16-B chunk,
    vcg_conv_fwd)."""
    return 4


def window_frames_u8(frames, idx, dtype, mean=IMAGENET_MEAN, std=IMAGENET_STD, cpad=8):
    """u8 RGB frames [F,H,W,3] gathered by an int64 frame table `idx` (any shape, 0-based) ->
    normalised NHWC stem input [idx.numel(),H,W,cpad] (channels 3.. zero; cpad 4 or 8)."""
    import ctypes

    _chk(frames, torch.uint8, "frames")
    _chk(idx, torch.int64, "idx")
    F, H, W, C = frames.shape
    if C != 3:
        raise ValueError("frames must be [F,H,W,3] RGB")
    n = idx.numel()
    dst = torch.empty((n, H, W, cpad), dtype=dtype, device=frames.device)
    m = (ctypes.c_float * 3)(*mean)
    sd = (ctypes.c_float * 3)(*std)
    _lib.call("vcg_window_frames_u8_cpad", dt_code(dtype), P(frames), P(idx), P(dst), n, F, H, W, cpad,
              ctypes.addressof(m), ctypes.addressof(sd), stream())
    return dst


def frames_to_nhwc(src, N, C, H, W, Cpad, dtype):
    _chk(src, torch.float32, "frames")
    dst = torch.empty((N, H, W, Cpad), dtype=dtype, device=src.device)
    _lib.call("vcg_frames_to_nhwc", dt_code(dtype), P(src), P(dst), N, C, H, W, Cpad, stream())
    return dst


def pair_taps(KW, pad):
    """(KWp, pwp) of the pair-packed stem (igemm.hip pair_taps): super-pixel taps and pad."""
    lo = (-pad) // 2
    return (KW - 1 - pad) // 2 - lo + 1, -lo


def weight_prep(w, Cpad, dtype, transposed=False, out=None, pair_pad=None):
    """GEMM operand of a conv weight; pair_pad (bf16, Cpad = 4): the pair-packed stem layout for that pad."""
    _chk(w, torch.float32, "weight")
    Cout, Cin, KH, KW = w.shape
    mode = int(transposed)
    if pair_pad is not None:
        shape, mode = (Cout, KH, pair_taps(KW, pair_pad)[0], 8), 2 + pair_pad
    else:
        shape = (Cin, KH, KW, Cout) if transposed else (Cout, KH, KW, Cpad)
    out = out if out is not None else torch.empty(shape, dtype=dtype, device=w.device)
    _lib.call("vcg_weight_prep", dt_code(dtype), P(w), P(out), Cout, Cin, KH, KW, Cpad, mode, stream())
    return out


def weight_fold(w2d, scale, dtype, out=None):
    """[rows, cols] f32 weight with row r scaled by scale[r], cast to dtype (vcg_weight_fold): a running-statistics BN
    folded into the 1x1 conv before it."""
    _chk(w2d, torch.float32, "weight")
    rows, cols = w2d.shape
    out = out if out is not None else torch.empty((rows, cols), dtype=dtype, device=w2d.device)
    _lib.call("vcg_weight_fold", dt_code(dtype), P(w2d), P(scale), P(out), rows, cols, stream())
    return out


def weight_prep_multi(desc, n):
    """One launch of vcg_weight_prep_multi over a DEVICE int64 descriptor table [n, 8]."""
    _chk(desc, torch.int64, "desc")
    assert desc.numel() >= 8 * n
    _lib.call("vcg_weight_prep_multi", BF16, P(desc), int(n), stream())


def transpose_multi(desc, n, total_tiles):
    """One launch of vcg_transpose_multi over a DEVICE int64 descriptor table [n, 5] (src, dst, rows, cols, first
    tile): bf16 [rows][cols] -> [cols][rows]."""
    _chk(desc, torch.int64, "desc")
    assert desc.numel() >= 5 * n
    _lib.call("vcg_transpose_multi", P(desc), int(n), int(total_tiles), stream())


def transpose(x, out=None):
    """[rows, cols] -> [cols, rows] (contiguous)."""
    _chk(x, None, "x")
    rows, cols = x.shape
    out = out if out is not None else torch.empty((cols, rows), dtype=x.dtype, device=x.device)
    _lib.call("vcg_transpose", dt_code(x.dtype), P(x), P(out), rows, cols, cols, rows, stream())
    return out


def cast_from_f32(x, dtype, out=None):
    _chk(x, torch.float32, "x")
    out = out if out is not None else torch.empty(x.shape, dtype=dtype, device=x.device)
    _lib.call("vcg_cast_from_f32", dt_code(dtype), P(x), P(out), x.numel(), stream())
    return out


def cast_to_f32(x, out=None):
    out = out if out is not None else torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _lib.call("vcg_cast_to_f32", dt_code(x.dtype), P(x), P(out), x.numel(), stream())
    return out


def tsm_shift(x, n_segment, fold_div, direction=0):
    """Reference TemporalShift.shift on an NCHW tensor [n_batch*T, C, H, W] (direction 1 = adjoint)."""
    _chk(x, name="x")
    nt, c, h, w = x.shape
    y = torch.empty_like(x)
    _lib.call("vcg_tsm_shift", dt_code(x.dtype), P(x), P(y), nt // n_segment, n_segment, c, h * w, fold_div,
              direction, stream())
    return y


def tsm_unshift_add(dshift, other, NT, T, HW, C, fold, other_bits=None):
    """dx = unshift(dshift) + other (other masked by `other_bits` when given)."""
    dx = torch.empty_like(dshift)
    _lib.call("vcg_tsm_unshift_add", dt_code(dshift.dtype), P(dshift), P(other), P(other_bits), P(dx), NT, T, HW, C,
              fold, stream())
    return dx


# ----------------------------------------------------------------------------- text
def embed_ln_fwd(ids, word, pos, typ, gamma, beta, B, L, H, eps, dtype, p=0.0, seed=0):
    out = torch.empty((B * L, H), dtype=dtype, device=ids.device)
    mean = torch.empty(B * L, dtype=torch.float32, device=ids.device)
    rstd = torch.empty(B * L, dtype=torch.float32, device=ids.device)
    _lib.call("vcg_embed_ln_fwd", dt_code(dtype), P(ids), P(word), P(pos), P(typ), P(gamma), P(beta), P(out), P(mean),
              P(rstd), B, L, H, float(eps), float(p), int(seed) & (2**64 - 1), stream())
    return out, mean, rstd


def embed_ln_bwd(dout, ids, word, pos, typ, gamma, mean, rstd, word_grad, pos_grad, type_grad, gamma_grad, beta_grad,
                 B, L, H, p=0.0, seed=0, pad_idx=-1):
    nbytes = _lib.query("vcg_ln_bwd_ws_bytes", B * L, H)
    w = ws(nbytes, dout.device)
    _lib.call("vcg_embed_ln_bwd", dt_code(dout.dtype), P(dout), P(ids), P(word), P(pos), P(typ), P(gamma), P(mean),
              P(rstd), P(word_grad), P(pos_grad), P(type_grad), P(gamma_grad), P(beta_grad), P(w), w.numel() * 4, B, L,
              H, float(p), int(seed) & (2**64 - 1), int(pad_idx), stream())


def ln_fwd(x, res, gamma, beta, rows, H, eps, p=0.0, seed=0):
    out = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    _lib.call("vcg_ln_fwd", dt_code(x.dtype), P(x), P(res), P(gamma), P(beta), P(out), P(mean), P(rstd), rows, H,
              float(eps), float(p), int(seed) & (2**64 - 1), stream())
    return out, mean, rstd


def ln_bwd(dout, x, res, gamma, mean, rstd, gamma_grad, beta_grad, rows, H, p=0.0, seed=0, want_dx=True,
           want_dres=True, bias_grad=None):
    """LayerNorm(dropout(x) + res) backward. bias_grad (optional, accumulated): column sums of dx, i.e. the
    bias gradient of the dense layer that produced x. dx has x's dtype, dres dout's: a bf16 x with an fp32 dout keeps
    the residual gradient in fp32 (VCG_GRAD_F32)."""
    dx = torch.empty_like(x) if want_dx else None
    dres = torch.empty_like(dout) if want_dres else None
    nbytes = _lib.query("vcg_ln_bwd_ws_bytes", rows, H)
    w = ws(nbytes, dout.device)
    code = dt_code(x.dtype)
    if dout.dtype != x.dtype:
        if not (x.dtype == torch.bfloat16 and dout.dtype == torch.float32):
            raise TypeError(f"ln_bwd: dout {dout.dtype} with x {x.dtype}")
        code |= GRAD_F32
    _lib.call("vcg_ln_bwd", code, P(dout), P(x), P(res), P(gamma), P(mean), P(rstd), P(dx), P(dres),
              P(gamma_grad), P(beta_grad), P(bias_grad), P(w), w.numel() * 4, rows, H, float(p),
              int(seed) & (2**64 - 1), stream())
    return dx, dres


def colsum(x, ld, rows, N, out, accumulate=True):
    nbytes = _lib.query("vcg_colsum_ws_bytes", rows, N)
    w = ws(nbytes, x.device)
    _lib.call("vcg_colsum", dt_code(x.dtype), P(x), ld, rows, N, P(out), int(accumulate), P(w), w.numel() * 4,
              stream())


def gpt_embed_fwd(ids, tok, pos, B, L, H, dtype, p=0.0, seed=0):
    """OpenAIGPT's embedding: dropout(tok[ids] + pos[t]) -> [B*L, H] (no token types, no LayerNorm)."""
    out = torch.empty((B * L, H), dtype=dtype, device=ids.device)
    _lib.call("vcg_gpt_embed_fwd", dt_code(dtype), P(ids), P(tok), P(pos), P(out), B, L, H, float(p),
              int(seed) & (2**64 - 1), stream())
    return out


def gpt_embed_bwd(dout, ids, tok_grad, pos_grad, B, L, H, p=0.0, seed=0, storage_dtype=None):
    """Backward of gpt_embed_fwd: fp32 token / position gradients ADDED onto tok_grad / pos_grad (either may be None),
    fixed order, no atomics. dout: the forward's dtype, or fp32 (the residual-gradient stream of a bf16 forward)."""
    nbytes = _lib.query("vcg_ln_bwd_ws_bytes", B * L, H)
    w = ws(nbytes, dout.device)
    code = dt_code(dout.dtype)
    if storage_dtype is not None and storage_dtype != dout.dtype:
        if not (storage_dtype == torch.bfloat16 and dout.dtype == torch.float32):
            raise TypeError(f"gpt_embed_bwd: dout {dout.dtype} with a {storage_dtype} forward")
        code = BF16 | GRAD_F32
    _lib.call("vcg_gpt_embed_bwd", code, P(dout), P(ids), P(tok_grad), P(pos_grad), P(w), w.numel() * 4, B, L, H,
              float(p), int(seed) & (2**64 - 1), stream())


def pegasus_embed_fwd(ids, tok, pos, B, L, H, dtype, scale, pos0=0, p=None, seed=0):
    """Pegasus' embedding: scale * tok[ids] + pos[pos0 + t] -> [B*L, H] (fp32 tables, one rounding). p (None: the
    inference entry): dropout on the result, counter row * H + c (dropout_util.row_keep(seed, B * L, H, p))."""
    _chk(ids, torch.int64, "ids")
    _chk(tok, torch.float32, "tok")
    _chk(pos, torch.float32, "pos")
    out = torch.empty((B * L, H), dtype=dtype, device=ids.device)
    if p is None:
        _lib.call("vcg_pegasus_embed_fwd", dt_code(dtype), P(ids), P(tok), P(pos), P(out), B, L, H, tok.shape[0],
                  pos.shape[0], float(scale), int(pos0), stream())
    else:
        _lib.call("vcg_pegasus_embed_fwd_ex", dt_code(dtype), P(ids), P(tok), P(pos), P(out), B, L, H, tok.shape[0],
                  pos.shape[0], float(scale), int(pos0), float(p), int(seed) & (2**64 - 1), stream())
    return out


def cross_attn_kv_fwd(q, kv, key_mask, B, nh, Lq, Lk, scale, ctx=None, stats=None, dh=64, dropout_p=None, seed=0):
    """Fused cross-attention forward (csrc/pegasus.hip): q [B*Lq, ldq], kv [B*Lk (+pad), ldkv] = K | V, key_mask int64
    [B, Lk] or None -> ctx [B*Lq, nh*dh]; stats (optional fp32 [B*nh, Lq, 2]) receives (row max, row sum).
    dropout_p (None: the inference entry vcg_cross_attn_kv_fwd): the training entry vcg_cross_attn_kv_fwd_ex, P dropped
    in the score space (z * Lq + q) * Lk + k = dropout_util.score_keep(seed, B * nh, Lq, Lk, p); 0 gives the inference
    entry's bits."""
    for t, name in ((q, "q"), (kv, "kv")):  # (row-major with any row pitch: column slices of a fused buffer are fine)
        if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or t.dtype != q.dtype:
            raise RuntimeError(f"{name} must be a 2-D GPU tensor with unit column stride, in q's dtype")
    if q.shape[0] < B * Lq or kv.shape[0] < B * Lk or q.shape[1] < nh * dh or kv.shape[1] < 2 * nh * dh:
        raise ValueError(f"cross_attn_kv_fwd: q {tuple(q.shape)} / kv {tuple(kv.shape)} too small for B={B} nh={nh} "
                         f"Lq={Lq} Lk={Lk}")
    if key_mask is not None:
        _chk(key_mask, torch.int64, "key_mask")
        if key_mask.numel() < B * Lk:
            raise ValueError("cross_attn_kv_fwd: key_mask smaller than [B, Lk]")
    if ctx is not None and (ctx.numel() < B * Lq * nh * dh or ctx.dtype != q.dtype):
        raise ValueError("cross_attn_kv_fwd: ctx must be [B*Lq, nh*dh] in q's dtype")
    if stats is not None and stats.numel() < 2 * B * nh * Lq:
        raise ValueError("cross_attn_kv_fwd: stats smaller than [B*nh, Lq, 2]")
    if ctx is None:
        ctx = torch.empty((B * Lq, nh * dh), dtype=q.dtype, device=q.device)
    if stats is not None:
        _chk(stats, torch.float32, "stats")
    if dropout_p is None:
        _lib.call("vcg_cross_attn_kv_fwd", dt_code(q.dtype), P(q), q.stride(0), P(kv), kv.stride(0), P(key_mask),
                  P(ctx), P(stats), B, nh, dh, Lq, Lk, float(scale), stream())
    else:
        _lib.call("vcg_cross_attn_kv_fwd_ex", dt_code(q.dtype), P(q), q.stride(0), P(kv), kv.stride(0), P(key_mask),
                  P(ctx), P(stats), B, nh, dh, Lq, Lk, float(scale), float(dropout_p), int(seed) & (2**64 - 1),
                  stream())
    return ctx


def cross_attn_kv_bwd(q, kv, key_mask, dctx, stats, B, nh, Lq, Lk, scale, dropout_p=0.0, seed=0, dq=None, dkv=None,
                      dh=64):
    """Backward of cross_attn_kv_fwd (two kernels, deterministic): q, kv, key_mask, dropout_p, seed as in the forward,
    stats [B*nh, Lq, 2] what it wrote, dctx [B*Lq, lddo] the gradient of ctx -> (dq [B*Lq, nh*dh], dkv [B*Lk, 2*nh*dh]
    = dK | dV); dq / dkv may be given (row-major with any row pitch: column slices are fine)."""
    H = nh * dh
    for t, name, rows, cols in ((q, "q", B * Lq, H), (kv, "kv", B * Lk, 2 * H), (dctx, "dctx", B * Lq, H),
                                (dq, "dq", B * Lq, H), (dkv, "dkv", B * Lk, 2 * H)):
        if t is None:
            continue
        if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or t.dtype != q.dtype:
            raise RuntimeError(f"{name} must be a 2-D GPU tensor with unit column stride, in q's dtype")
        if t.shape[0] < rows or t.shape[1] < cols:
            raise ValueError(f"cross_attn_kv_bwd: {name} {tuple(t.shape)} too small for B={B} nh={nh} Lq={Lq} Lk={Lk}")
    _chk(stats, torch.float32, "stats")
    if stats.numel() < 2 * B * nh * Lq:
        raise ValueError("cross_attn_kv_bwd: stats smaller than [B*nh, Lq, 2]")
    if key_mask is not None:
        _chk(key_mask, torch.int64, "key_mask")
        if key_mask.numel() < B * Lk:
            raise ValueError("cross_attn_kv_bwd: key_mask smaller than [B, Lk]")
    if dq is None:
        dq = torch.empty((B * Lq, H), dtype=q.dtype, device=q.device)
    if dkv is None:
        dkv = torch.empty((B * Lk, 2 * H), dtype=q.dtype, device=q.device)
    d_ws = torch.empty(B * nh * Lq, dtype=torch.float32, device=q.device)
    _lib.call("vcg_cross_attn_kv_bwd", dt_code(q.dtype), P(q), q.stride(0), P(kv), kv.stride(0), P(key_mask),
              P(dctx), dctx.stride(0), P(stats), P(d_ws), P(dq), dq.stride(0), P(dkv), dkv.stride(0), B, nh, dh, Lq, Lk,
              float(scale), float(dropout_p), int(seed) & (2**64 - 1), stream())
    return dq, dkv


def pegasus_embed_bwd(dout, ids, tok_grad, B, L, H, scale, pad_idx, p=0.0, seed=0, storage_dtype=None):
    """Backward of pegasus_embed_fwd(..., p, seed): tok_grad[id] += scale * dropout'(dout), fp32, ADDED, fixed order,
    no atomics; rows whose id is pad_idx add nothing (nn.Embedding(padding_idx)). dout: the forward's dtype, or fp32
    behind a bf16 forward (storage_dtype=torch.bfloat16: the VCG_GRAD_F32 class)."""
    _chk(ids, torch.int64, "ids")
    _chk(tok_grad, torch.float32, "tok_grad")
    if ids.numel() < B * L or dout.numel() < B * L * H or not dout.is_contiguous():
        raise ValueError("pegasus_embed_bwd: ids / dout smaller than [B, L] / [B*L, H], or dout not contiguous")
    if tok_grad.dim() != 2 or tok_grad.shape[1] != H or not tok_grad.is_contiguous():
        raise ValueError("pegasus_embed_bwd: tok_grad must be a contiguous [V, H]")
    w = ws(_lib.query("vcg_ln_bwd_ws_bytes", B * L, H), dout.device)
    code = dt_code(dout.dtype)
    if storage_dtype is not None and storage_dtype != dout.dtype:
        if not (storage_dtype == torch.bfloat16 and dout.dtype == torch.float32):
            raise TypeError(f"pegasus_embed_bwd: dout {dout.dtype} with a {storage_dtype} forward")
        code = BF16 | GRAD_F32
    _lib.call("vcg_pegasus_embed_bwd", code, P(dout), P(ids), P(tok_grad), P(w), w.numel() * 4, B, L, H, float(scale),
              int(pad_idx), float(p), int(seed) & (2**64 - 1), stream())


def ln_bwd_acc(dout, x, gamma, mean, rstd, dh, gamma_grad, beta_grad, rows, H):
    """dh (fp32 gradient stream, in place) += LN'(dout) for y = LN(x) of an fp32 x without a residual (ln_fwd(x, None,
    ...)'s mean / rstd); dout in the compute dtype or fp32; gamma_grad / beta_grad (fp32, ADDED) may be None."""
    _chk(x, torch.float32, "x")
    _chk(dh, torch.float32, "dh")
    _chk(dout, name="dout")
    if min(dout.numel(), x.numel(), dh.numel()) < rows * H or mean.numel() < rows or rstd.numel() < rows:
        raise ValueError(f"ln_bwd_acc: an operand is smaller than [{rows}, {H}]")
    w = ws(_lib.query("vcg_ln_bwd_ws_bytes", rows, H), dout.device)
    _lib.call("vcg_ln_bwd_acc", dt_code(dout.dtype), P(dout), P(x), P(gamma), P(mean), P(rstd), P(dh), P(gamma_grad),
              P(beta_grad), P(w), w.numel() * 4, rows, H, stream())
    return dh


def _ew_check(name, n, *ts):
    for t in ts:
        if not t.is_cuda or not t.is_contiguous() or t.numel() < n:
            raise ValueError(f"{name}: every operand must be a contiguous GPU tensor of at least {n} elements")


def dropout_add_fwd(h, branch, p=0.0, seed=0):
    """h (fp32 residual stream, in place) += dropout(branch); counter = the element index row * H + c
    (dropout_util.row_keep)."""
    _chk(h, torch.float32, "h")
    n = branch.numel()
    _ew_check("dropout_add_fwd", n, h, branch)
    _lib.call("vcg_dropout_add_fwd", dt_code(branch.dtype), P(h), P(branch), n, float(p), int(seed) & (2**64 - 1),
              stream())
    return h


def dropout_add_bwd(dh, dtype, p=0.0, seed=0):
    """The branch's gradient dropout'(dh) in `dtype` (dh, fp32, passes through to the stream unchanged)"""
    _chk(dh, torch.float32, "dh")
    _ew_check("dropout_add_bwd", dh.numel(), dh)
    out = torch.empty(dh.shape, dtype=dtype, device=dh.device)
    _lib.call("vcg_dropout_add_bwd", dt_code(dtype), P(dh), P(out), dh.numel(), float(p), int(seed) & (2**64 - 1),
              stream())
    return out


def relu_dropout_fwd(pre, p=0.0, seed=0, out=None):
    """f = dropout(relu(pre)) (out may be pre: in place); counter = the element index"""
    out = torch.empty_like(pre) if out is None else out
    if out.dtype != pre.dtype:
        raise TypeError("relu_dropout_fwd: out must have pre's dtype")
    _ew_check("relu_dropout_fwd", pre.numel(), pre, out)
    _lib.call("vcg_relu_dropout_fwd", dt_code(pre.dtype), P(pre), P(out), pre.numel(), float(p),
              int(seed) & (2**64 - 1), stream())
    return out


def relu_dropout_bwd(dy, f, p=0.0, out=None):
    """dpre = dy * (f > 0 ? 1 / (1 - p) : 0) from the saved post-dropout activation f (out may be dy: in place)"""
    out = torch.empty_like(dy) if out is None else out
    if f.dtype != dy.dtype or out.dtype != dy.dtype:
        raise TypeError("relu_dropout_bwd: dy, f and out must share a dtype")
    _ew_check("relu_dropout_bwd", dy.numel(), dy, f, out)
    _lib.call("vcg_relu_dropout_bwd", dt_code(dy.dtype), P(dy), P(f), P(out), dy.numel(), float(p), stream())
    return out


def attn_softmax_fwd(S, mask, P_out, Pd_out, B, nh, L, Lp, scale, p=0.0, seed=0, causal=False):
    if causal:
        _lib.call("vcg_attn_softmax_fwd_ex", dt_code(S.dtype), P(S), P(mask), P(P_out), P(Pd_out), B, nh, L, Lp,
                  float(scale), float(p), int(seed) & (2**64 - 1), ATTN_CAUSAL, stream())
        return
    _lib.call("vcg_attn_softmax_fwd", dt_code(S.dtype), P(S), P(mask), P(P_out), P(Pd_out), B, nh, L, Lp,
              float(scale), float(p), int(seed) & (2**64 - 1), stream())


def attn_softmax_bwd(dPd, Pm, dS, Z, L, Lp, scale, p=0.0, seed=0, causal=False):
    if causal:
        _lib.call("vcg_attn_softmax_bwd_ex", dt_code(dPd.dtype), P(dPd), P(Pm), P(dS), Z, L, Lp, float(scale),
                  float(p), int(seed) & (2**64 - 1), ATTN_CAUSAL, stream())
        return
    _lib.call("vcg_attn_softmax_bwd", dt_code(dPd.dtype), P(dPd), P(Pm), P(dS), Z, L, Lp, float(scale), float(p),
              int(seed) & (2**64 - 1), stream())


def bert_attn_stats(B, nh, L, device):
    """The fused attention's saved state (f32, vcg_bert_attn_stats_bytes: the row statistics the forward writes; at
    L > 128 also the backward's D vector)."""
    return torch.empty(_lib.query("vcg_bert_attn_stats_bytes", B, nh, L) // 4, dtype=torch.float32, device=device)


def bert_attn_fwd(qkv, mask, ctx, stats, B, nh, L, Lp, scale, p=0.0, seed=0, seq=None, causal=False):
    """Fused attention forward (bf16, L <= 512, head dim 64; L > 128: the tiled online-softmax kernels): qkv
    [B*L(+pad), 3H] -> ctx [B*L, H]; stats: bert_attn_stats(B, nh, L).
    seq (int32 [B+1]): packed sequences, rows seq[b] .. seq[b+1]-1 (L = the longest, mask = the packed rows' key
    flags; vcg_bert_attn_fwd_varlen). causal: key j is visible to query i iff j <= i and mask[j] != 0; tiles above the
    diagonal are skipped (vcg_bert_attn_fwd_ex)."""
    if causal:
        _lib.call("vcg_bert_attn_fwd_ex", P(qkv), P(mask), P(seq), P(ctx), P(stats), B, nh, L, Lp, float(scale),
                  float(p), int(seed) & (2**64 - 1), ATTN_CAUSAL, stream())
    elif seq is None:
        _lib.call("vcg_bert_attn_fwd", P(qkv), P(mask), P(ctx), P(stats), B, nh, L, Lp, float(scale), float(p),
                  int(seed) & (2**64 - 1), stream())
    else:
        _lib.call("vcg_bert_attn_fwd_varlen", P(qkv), P(mask), P(seq), P(ctx), P(stats), B, nh, L, Lp, float(scale),
                  float(p), int(seed) & (2**64 - 1), stream())


def bert_attn_bwd(qkv, dctx, ctx, mask, stats, dqkv, B, nh, L, Lp, scale, p=0.0, seed=0, seq=None, causal=False):
    """Backward of bert_attn_fwd: dqkv [B*L, 3H] = dQ | dK | dV (deterministic; ctx may be None). At L > 128 it writes
    its D vector into the tail of `stats`. causal: as the forward's."""
    if causal:
        _lib.call("vcg_bert_attn_bwd_ex", P(qkv), P(dctx), P(mask), P(seq), P(stats), P(dqkv), B, nh, L, Lp,
                  float(scale), float(p), int(seed) & (2**64 - 1), ATTN_CAUSAL, stream())
    elif seq is None:
        _lib.call("vcg_bert_attn_bwd", P(qkv), P(dctx), P(ctx), P(mask), P(stats), P(dqkv), B, nh, L, Lp, float(scale),
                  float(p), int(seed) & (2**64 - 1), stream())
    else:
        _lib.call("vcg_bert_attn_bwd_varlen", P(qkv), P(dctx), P(mask), P(seq), P(stats), P(dqkv), B, nh, L, Lp,
                  float(scale), float(p), int(seed) & (2**64 - 1), stream())


def tanh_bwd(dy, t):
    dx = torch.empty_like(dy)
    _lib.call("vcg_tanh_bwd", dt_code(dy.dtype), P(dy), P(t), P(dx), dy.numel(), stream())
    return dx


# ----------------------------------------------------------------------------- head / loss
def head_mlp_fwd(Vout, Lout, W, bias, B, T, hid, O):
    logits = torch.empty((B, O), dtype=torch.float32, device=Vout.device)
    prob = torch.empty((B, O), dtype=torch.float32, device=Vout.device)
    _lib.call("vcg_head_mlp_fwd", dt_code(Vout.dtype), P(Vout), P(Lout), P(W), P(bias), P(logits), P(prob), B, T,
              hid, O, stream())
    return logits, prob


def head_mlp_bwd(Vout, Lout, W, dlogits, dW, dbias, B, T, hid, O, relu_mask=True):
    dV = torch.empty_like(Vout)
    dL = torch.empty_like(Lout)
    _lib.call("vcg_head_mlp_bwd", dt_code(Vout.dtype), P(Vout), P(Lout), P(W), P(dlogits), P(dV), P(dL), P(dW),
              P(dbias), B, T, hid, O, int(relu_mask), stream())
    return dV, dL


def head_attn_fwd(Vout, Lout, query, key, value, proj, B, T, hid, n_head, p=0.0, seed=0):
    """SelfAttention head (two_stream.py:31-48) over cat([Vout [B*T,hid], Lout [B,hid]]) per window:
    logits / prob [B, O] fp32 and the f32 state the backward needs (vcg_head_attn_saved_floats)."""
    _chk(Vout, name="Vout")
    _chk(Lout, Vout.dtype, "Lout")
    assert Vout.numel() == B * T * hid and Lout.numel() == B * hid
    O = proj.weight.shape[0]
    for lin in (query, key, value, proj):
        _chk(lin.weight, torch.float32, "head weight")
    saved = torch.empty(_lib.query("vcg_head_attn_saved_floats", B, T, hid, n_head), dtype=torch.float32,
                        device=Vout.device)
    logits = torch.empty((B, O), dtype=torch.float32, device=Vout.device)
    prob = torch.empty((B, O), dtype=torch.float32, device=Vout.device)
    _lib.call("vcg_head_attn_fwd", dt_code(Vout.dtype), P(Vout), P(Lout), P(query.weight), P(query.bias),
              P(key.weight), P(key.bias), P(value.weight), P(value.bias), P(proj.weight), P(proj.bias), P(saved),
              saved.numel(), P(logits), P(prob), B, T, hid, n_head, O, float(p), int(seed) & (2**64 - 1), stream())
    return logits, prob, saved


def head_attn_bwd(saved, query, key, value, proj, dlogits, Vout, Lout, B, T, hid, n_head, p=0.0, seed=0,
                  relu_mask=True):
    """Backward of head_attn_fwd: returns the ReLU-masked gradients of Vout / Lout; accumulates the
    query / key / value / proj parameter gradients into their .grad (when they require grad)."""
    O = proj.weight.shape[0]
    dV = torch.empty_like(Vout)
    dL = torch.empty_like(Lout)
    w = torch.empty(_lib.query("vcg_head_attn_bwd_ws_floats", B, T, hid), dtype=torch.float32, device=Vout.device)

    def g(t):
        return P(t.grad) if t.requires_grad else None
    _lib.call("vcg_head_attn_bwd", dt_code(Vout.dtype), P(saved), P(query.weight), P(key.weight), P(value.weight),
              P(proj.weight), P(dlogits), P(dV), P(dL), g(query.weight), g(query.bias), g(key.weight), g(key.bias),
              g(value.weight), g(value.bias), g(proj.weight), g(proj.bias), P(w), w.numel(), B, T, hid, n_head, O,
              float(p), int(seed) & (2**64 - 1), int(relu_mask), stream())
    return dV, dL


def cross_entropy_fwd(logits, labels):
    B, C = logits.shape
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    _lib.call("vcg_cross_entropy_fwd", P(logits), P(labels), P(loss), B, C, stream())
    return loss


def cross_entropy_bwd(logits, labels, dloss):
    B, C = logits.shape
    dlogits = torch.empty_like(logits)
    _lib.call("vcg_cross_entropy_bwd", P(logits), P(labels), P(dloss), P(dlogits), B, C, stream())
    return dlogits


# ----------------------------------------------------------------------------- masked-LM head (mlm_head.hip)
def mlm_vp(V):
    """Row stride of the dZ / logits buffers: V rounded up to 16-byte rows."""
    return (V + 7) // 8 * 8


def _mlm_outputs(R, device):
    return (torch.empty(R, dtype=torch.float32, device=device), torch.empty(R, dtype=torch.float32, device=device),
            torch.empty((), dtype=torch.float32, device=device), torch.empty((), dtype=torch.int64, device=device))


def mlm_loss_fwd(hidden, rows, W, targets, workspace=None):
    """Fused masked-LM loss of hidden[rows] (bf16 [rows_total, H], rows int64 [R] or None) against W (bf16 [V, H]) and
    targets (int64 [R], in [0, V)): (lse [R], row_loss [R], mean_loss [], n_correct [] int64)."""
    _chk(hidden, torch.bfloat16, "hidden")
    _chk(W, torch.bfloat16, "W")
    _chk(targets, torch.int64, "targets")
    if rows is not None:
        _chk(rows, torch.int64, "rows")
    R, (V, H) = targets.numel(), W.shape
    nbytes = _lib.query("vcg_mlm_loss_ws_bytes", R, V, H)
    if workspace is None:
        workspace = ws(nbytes, hidden.device)
    lse, row_loss, loss, n_correct = _mlm_outputs(R, hidden.device)
    _lib.call("vcg_mlm_loss_fwd", P(hidden), hidden.shape[0], P(rows), P(W), P(targets), R, V, H, P(workspace),
              workspace.numel() * 4, P(lse), P(row_loss), P(loss), P(n_correct), stream())
    return lse, row_loss, loss, n_correct


def mlm_loss_bwd(hidden, rows, W, targets, lse, dloss):
    """dZ (bf16 [R, mlm_vp(V)], pad columns zero) = (softmax(z) - onehot(target)) * dloss / R; dloss a device scalar."""
    _chk(dloss, torch.float32, "dloss")
    R, (V, H) = targets.numel(), W.shape
    dZ = torch.empty((R, mlm_vp(V)), dtype=torch.bfloat16, device=hidden.device)
    _lib.call("vcg_mlm_loss_bwd", P(hidden), hidden.shape[0], P(rows), P(W), P(targets), P(lse), P(dloss), R, V, H,
              P(dZ), dZ.shape[1], stream())
    return dZ


def mlm_logits(hidden, W):
    """fp32 logits [rows, mlm_vp(V)] (pad columns zero) = hidden W^T, bf16 operands."""
    _chk(hidden, torch.bfloat16, "hidden")
    _chk(W, torch.bfloat16, "W")
    V, H = W.shape
    out = torch.empty((hidden.shape[0], mlm_vp(V)), dtype=torch.float32, device=hidden.device)
    _lib.call("vcg_mlm_logits", P(hidden), hidden.shape[0], P(W), V, H, P(out), out.shape[1], stream())
    return out


def mlm_reduce_f32(logits, V, targets):
    """The fused loss' outputs from fp32 logits [R, ld >= V] that are in memory (the fp32 parity mode)."""
    _chk(logits, torch.float32, "logits")
    _chk(targets, torch.int64, "targets")
    R, ld = logits.shape
    workspace = ws(7 * R * 4, logits.device)  # 5 floats per row of partials + 2 of row results
    lse, row_loss, loss, n_correct = _mlm_outputs(R, logits.device)
    _lib.call("vcg_mlm_reduce_f32", P(logits), ld, P(targets), R, V, P(workspace), workspace.numel() * 4, P(lse),
              P(row_loss), P(loss), P(n_correct), stream())
    return lse, row_loss, loss, n_correct


def mlm_dz_f32(logits, V, lse, targets, dloss):
    """In place: logits [R, ld] -> dZ (columns V .. ld - 1 zeroed)."""
    _chk(logits, torch.float32, "logits")
    _chk(dloss, torch.float32, "dloss")
    R, ld = logits.shape
    _lib.call("vcg_mlm_dz_f32", P(logits), ld, P(lse), P(targets), P(dloss), R, V, stream())
    return logits


def seq_softmax_fwd(logits, B, L, V, ldz=None):
    """prob [B, L, V] = softmax over L of fp32 logits [B, L, ldz] (F.softmax(logits, dim=1))."""
    if logits.dtype != torch.float32 or not logits.is_cuda:
        raise RuntimeError("seq_softmax_fwd: fp32 GPU logits")
    ldz = ldz if ldz is not None else V
    prob = torch.empty((B, L, V), dtype=torch.float32, device=logits.device)
    _lib.call("vcg_seq_softmax_fwd", P(logits), ldz, P(prob), V, B, L, V, stream())
    return prob


# ----------------------------------------------------------------------------- MoCo pre-training (contrast.hip)
NORM_EPS = 1e-12  # F.normalize's default


def momentum_update(k, q, m, k_shadow=None):
    """k = k * m + q * (1. - m) in place over two flat fp32 spans, bit for bit torch's expression: m and 1. - m are
    formed in double and rounded to fp32 once. k_shadow (bf16, same length) receives the rounded result."""
    import numpy as np
    _chk(k, torch.float32, "k")
    _chk(q, torch.float32, "q")
    if k.numel() != q.numel() or (k_shadow is not None and k_shadow.numel() != k.numel()):
        raise ValueError("momentum_update: the spans differ in length")
    if k_shadow is not None:
        _chk(k_shadow, torch.bfloat16, "k_shadow")
    _lib.call("vcg_momentum_update", P(k), P(q), k.numel(), float(np.float32(m)), float(np.float32(1. - m)),
              P(k_shadow), stream())
    return k


def l2norm_fwd(x, eps=NORM_EPS):
    """F.normalize(x, dim=1) on [N, H] -> (y in x's dtype, denom fp32 [N] = max(||x||, eps))."""
    _chk(x, None, "x")
    N, H = x.shape
    y = torch.empty_like(x)
    denom = torch.empty(N, dtype=torch.float32, device=x.device)
    _lib.call("vcg_l2norm_fwd", dt_code(x.dtype), P(x), P(y), P(denom), N, H, float(eps), stream())
    return y, denom


def l2norm_bwd(g, x, denom):
    """dx fp32 [N, H] = (g - y (y . g)) / denom."""
    _chk(g, torch.float32, "g")
    _chk(x, None, "x")
    N, H = x.shape
    dx = torch.empty((N, H), dtype=torch.float32, device=x.device)
    _lib.call("vcg_l2norm_bwd", dt_code(x.dtype), P(g), P(x), P(denom), P(dx), N, H, stream())
    return dx


def contrast_select(q, cand, eps=NORM_EPS):
    """k0 int64 [B]: the candidate of cand [B, C, H] with the largest cosine to q [B, H] (lowest index on a tie)."""
    _chk(q, None, "q")
    _chk(cand, q.dtype, "cand")
    B, C, H = cand.shape
    if q.shape != (B, H):
        raise ValueError(f"contrast_select: q {tuple(q.shape)} against candidates {tuple(cand.shape)}")
    k0 = torch.empty(B, dtype=torch.int64, device=q.device)
    _lib.call("vcg_contrast_select", dt_code(q.dtype), P(q), P(cand), B, C, H, float(eps), P(k0), stream())
    return k0


def queue_kp(K):
    """Rows of queue_km / row stride of the dZ buffer: K rounded up to 8."""
    return (K + 7) // 8 * 8


def queue_enqueue(keys, queue, queue_km, queue_ptr):
    """keys [N, H] -> queue[:, ptr:ptr+N] (fp32 [H, K]) and queue_km[ptr:ptr+N] ([queue_kp(K), H]); queue_ptr (device
    int64 [1]) advances to (ptr + N) % K. K % N != 0 raises with nothing written."""
    _chk(keys, None, "keys")
    _chk(queue, torch.float32, "queue")
    _chk(queue_km, None, "queue_km")
    _chk(queue_ptr, torch.int64, "queue_ptr")
    N, H = keys.shape
    K = queue.shape[1]
    if queue.shape[0] != H or tuple(queue_km.shape) != (queue_kp(K), H):
        raise ValueError("queue_enqueue: shapes of queue / queue_km / keys do not agree")
    _lib.call("vcg_queue_enqueue", dt_code(keys.dtype), dt_code(queue_km.dtype), P(keys), P(queue), P(queue_km),
              P(queue_ptr), N, K, H, stream())


def queue_rebuild(queue, dtype, out=None):
    """queue fp32 [H, K] -> queue_km [queue_kp(K), H] in `dtype` (transpose + cast; the pad rows are zeros)."""
    _chk(queue, torch.float32, "queue")
    H, K = queue.shape
    if out is None or out.dtype != dtype or tuple(out.shape) != (queue_kp(K), H) or out.device != queue.device:
        out = torch.zeros((queue_kp(K), H), dtype=dtype, device=queue.device)
    _lib.call("vcg_queue_rebuild", dt_code(dtype), P(queue), P(out), K, H, stream())
    return out


def rowdot(a, b, scale=1.0, out=None, ldo=1):
    """out[n * ldo] = scale * a[n] . b[n] (fp32)."""
    _chk(a, None, "a")
    _chk(b, a.dtype, "b")
    N, H = a.shape
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=a.device)
    _lib.call("vcg_rowdot", dt_code(a.dtype), P(a), P(b), N, H, float(scale), P(out), int(ldo), stream())
    return out


def _nce_outputs(N, device):
    return (torch.empty(N, dtype=torch.float32, device=device), torch.empty(N, dtype=torch.float32, device=device),
            torch.empty((), dtype=torch.float32, device=device), torch.empty((), dtype=torch.int64, device=device))


def infonce_logits_buffer(N, K, device):
    """(buf fp32 [N, 4 + queue_kp(K)], the [N, 1 + K] logits view buf[:, 3:4+K]): the positive in column 3, the key
    columns from the 16-byte aligned column 4."""
    buf = torch.empty((N, 4 + queue_kp(K)), dtype=torch.float32, device=device)
    return buf, buf[:, 3:4 + K]


def infonce(q, k, queue_km, K, inv_T, want_dq=False, want_logits=False):
    """InfoNCE of normalised q, k [N, H] against the first K rows of queue_km, logits [q.k, q queue_km^T] * inv_T,
    label 0 -> (lse [N], row_loss [N], mean loss [], n_correct [] int64, dq fp32 [N, H] or None = d mean loss / dq,
    logits view [N, 1 + K] or None). bf16: the fused tile kernel (nothing N x K in fp32 unless the logits are asked
    for); fp32: the logits by vcg_gemm, then reduced."""
    _chk(q, None, "q")
    _chk(k, q.dtype, "k")
    _chk(queue_km, q.dtype, "queue_km")
    N, H = q.shape
    Kp = queue_kp(K)
    if k.shape != q.shape or tuple(queue_km.shape) != (Kp, H):
        raise ValueError("infonce: shapes of q / k / queue_km do not agree")
    dev, s = q.device, stream()
    lse, row_loss, loss, n_correct = _nce_outputs(N, dev)
    omp0 = torch.empty(N, dtype=torch.float32, device=dev) if want_dq else None  # 1 - p0, free of cancellation
    scale = inv_T / N
    logits = dq = None
    if q.dtype == torch.bfloat16:
        lpos = rowdot(q, k, inv_T)
        work = ws(_lib.query("vcg_infonce_ws_bytes", N, K, H), dev)
        _lib.call("vcg_infonce_fwd", P(q), P(queue_km), P(lpos), N, K, H, float(inv_T), P(work), work.numel() * 4,
                  P(lse), P(row_loss), P(omp0), P(loss), P(n_correct), s)
        if want_logits:
            buf, logits = infonce_logits_buffer(N, K, dev)
            buf[:, 3].copy_(lpos)
            _lib.call("vcg_infonce_logits", P(q), P(queue_km), N, K, H, float(inv_T), buf.data_ptr() + 16,
                      buf.shape[1], s)
        if want_dq:
            dz = torch.empty((N, Kp), dtype=torch.bfloat16, device=dev)
            _lib.call("vcg_infonce_dz", P(q), P(queue_km), P(lse), N, K, H, float(inv_T), float(scale), P(dz), Kp, s)
            dq = torch.empty((N, H), dtype=torch.float32, device=dev)
            gemm_splitk(dz, queue_km, dq, N, H, K, Kp, H, transA=False, transB=True, accumulate=False)
    else:
        buf, view = infonce_logits_buffer(N, K, dev)
        rowdot(q, k, inv_T, out=buf[:, 3], ldo=buf.shape[1])
        lpos = buf[:, 3].contiguous()
        keyz = buf.data_ptr() + 16
        _lib.call("vcg_gemm", F32, 0, 0, N, Kp, H, P(q), H, P(queue_km), H, keyz, buf.shape[1], None, ACT_NONE, None,
                  buf.shape[1], None, float(inv_T), s)
        work = ws(6 * N * 4, dev)
        _lib.call("vcg_infonce_reduce_f32", keyz, buf.shape[1], P(lpos), N, K, P(work), work.numel() * 4, P(lse),
                  P(row_loss), P(omp0), P(loss), P(n_correct), s)
        if want_logits:
            logits = view.clone() if want_dq else view  # (the gradient below overwrites the key columns)
        if want_dq:
            _lib.call("vcg_infonce_dz_f32", keyz, buf.shape[1], P(lse), float(scale), N, K, s)
            dq = torch.empty((N, H), dtype=torch.float32, device=dev)
            _lib.call("vcg_gemm", F32, 0, 1, N, H, Kp, keyz, buf.shape[1], P(queue_km), H, P(dq), H, None, ACT_NONE,
                      None, H, None, 1.0, s)
    if want_dq:
        _lib.call("vcg_infonce_dq_pos", dt_code(q.dtype), P(dq), P(k), P(omp0), float(scale), N, H, s)
    return lse, row_loss, loss, n_correct, dq, logits


# ----------------------------------------------------------------------------- listwise fine-tuning (listnet.hip)
def listnet_limits():
    """(largest slate length S, largest hidden size H) of the listnet kernels; H must also be a multiple of 8."""
    return _lib.query("vcg_listnet_max_slate"), _lib.query("vcg_listnet_max_hidden")


def listnet_check_shape(B, S, H, M):
    """The kernels' shape rules as ValueErrors, before anything is launched."""
    max_s, max_h = listnet_limits()
    if B < 1:
        raise ValueError(f"listnet: batch size {B}, need at least 1 slate")
    if S < 2 or S > max_s:
        raise ValueError(f"listnet: slate length {S} outside [2, {max_s}] (the boundary clip and at least one other; "
                         f"one lane of a wave per contrast clip)")
    if H < 8 or H > max_h or H % 8 != 0:
        raise ValueError(f"listnet: hidden size {H} must be a multiple of 8 in [8, {max_h}] (16-byte rows)")
    if M < 1:
        raise ValueError(f"listnet: {M} selected rows, need at least 1")


class ListnetIndices:
    """The boundary head's rows `sel` [M] (rows of P, duplicates allowed) and labels `cls` [M] in {0, 1}, checked on the
    host against rows = B S -- an index out of range never reaches a kernel -- and their int64 device copies. Host
    lists / arrays / CPU tensors are checked as they are; device tensors cost one small device-to-host copy."""

    def __init__(self, sel, cls, rows, device):
        sel, cls = (t if isinstance(t, torch.Tensor) else torch.as_tensor(t) for t in (sel, cls))
        if sel.dim() != 1 or cls.shape != sel.shape:
            raise ValueError(f"listnet: sel {tuple(sel.shape)} and cls {tuple(cls.shape)} must be two vectors of one "
                             f"length")
        if sel.dtype.is_floating_point or cls.dtype.is_floating_point:
            raise ValueError("listnet: sel and cls must be integer tensors")
        if sel.is_cuda or cls.is_cuda:
            host = torch.stack([sel.to(device, torch.int64), cls.to(device, torch.int64)]).cpu()
            sel_h, cls_h = host[0], host[1]
        else:
            sel_h, cls_h = sel.to(torch.int64), cls.to(torch.int64)
        self.M = sel_h.numel()
        if self.M:
            lo, hi = int(sel_h.min()), int(sel_h.max())
            if lo < 0 or hi >= rows:
                raise ValueError(f"listnet: selected row {lo if lo < 0 else hi} outside [0, {rows})")
            bad = cls_h[(cls_h != 0) & (cls_h != 1)]
            if bad.numel():
                raise ValueError(f"listnet: binary label {int(bad[0])} outside {{0, 1}}")
        self.rows = rows
        self.sel = sel_h.contiguous().to(device)
        self.cls = cls_h.contiguous().to(device)


def _listnet_args(P_, targets, idx):
    _chk(P_, None, "P")
    _chk(targets, torch.float32, "targets")
    if P_.dim() != 2 or targets.dim() != 2:
        raise ValueError(f"listnet: P {tuple(P_.shape)} must be [B S, H] and targets {tuple(targets.shape)} [B, S]")
    B, S = targets.shape
    H = P_.shape[1]
    listnet_check_shape(B, S, H, idx.M)
    if P_.shape[0] != B * S or idx.rows != B * S:
        raise ValueError(f"listnet: P has {P_.shape[0]} rows and the indices were checked against {idx.rows}; targets "
                         f"[{B}, {S}] need {B * S}")
    return B, S, H, idx.M


def listnet_fwd(P_, targets, sel, cls, W, bias):
    """The ListNet slate loss and the boundary head over the pooled output P [B S, H] (fp32 or bf16), targets fp32
    [B, S], W fp32 [2, H], bias fp32 [2] -> (loss3 fp32 [3] = loss, surrogate, binary; binary_logits fp32 [M, 2];
    binary_prob fp32 [M, 2]; p fp32 [B, S - 1]; the checked ListnetIndices for listnet_bwd). Every refusal is a
    ValueError raised before the launch."""
    if not isinstance(sel, ListnetIndices) and P_.dim() == 2 and targets.dim() == 2:
        listnet_check_shape(targets.shape[0], targets.shape[1], P_.shape[1], len(sel))  # (the shape before the rows)
    idx = sel if isinstance(sel, ListnetIndices) else ListnetIndices(sel, cls, P_.shape[0], P_.device)
    B, S, H, M = _listnet_args(P_, targets, idx)
    _chk(W, torch.float32, "W")
    _chk(bias, torch.float32, "bias")
    if tuple(W.shape) != (2, H) or bias.numel() != 2:
        raise ValueError(f"listnet: the boundary head must be W [2, {H}] and bias [2], got {tuple(W.shape)} and "
                         f"{tuple(bias.shape)}")
    dev = P_.device
    p = torch.empty((B, S - 1), dtype=torch.float32, device=dev)
    logits = torch.empty((M, 2), dtype=torch.float32, device=dev)
    prob = torch.empty((M, 2), dtype=torch.float32, device=dev)
    part = torch.empty(B + M, dtype=torch.float32, device=dev)
    loss3 = torch.empty(3, dtype=torch.float32, device=dev)
    _lib.call("vcg_listnet_fwd", dt_code(P_.dtype), P(P_), P(targets), P(idx.sel), P(idx.cls), P(W), P(bias), B, S, H, M,
              P(p), P(logits), P(prob), P(part), P(loss3), stream())
    return loss3, logits, prob, p, idx


def listnet_bwd(P_, targets, idx, W, p, prob, dloss, dW=None, db=None, out=None):
    """dP fp32 [B S, H] (into `out` if given: every row is written exactly once) for the device scalar dloss; dW [2, H]
    and db [2] (both or neither) are added to. idx: the ListnetIndices listnet_fwd returned."""
    if not isinstance(idx, ListnetIndices):
        raise TypeError("listnet_bwd: idx must be the ListnetIndices that listnet_fwd checked")
    B, S, H, M = _listnet_args(P_, targets, idx)
    _chk(W, torch.float32, "W")
    _chk(p, torch.float32, "p")
    _chk(prob, torch.float32, "prob")
    _chk(dloss, torch.float32, "dloss")
    if tuple(W.shape) != (2, H) or tuple(p.shape) != (B, S - 1) or tuple(prob.shape) != (M, 2) or dloss.numel() != 1:
        raise ValueError("listnet_bwd: shapes of W / p / prob / dloss do not agree with P and targets")
    if (dW is None) != (db is None):
        raise ValueError("listnet_bwd: dW and db go together")
    if dW is not None:
        _chk(dW, torch.float32, "dW")
        _chk(db, torch.float32, "db")
        if tuple(dW.shape) != (2, H) or db.numel() != 2:
            raise ValueError("listnet_bwd: dW must be [2, H] and db [2]")
    if out is None:
        out = torch.empty((B * S, H), dtype=torch.float32, device=P_.device)
    _chk(out, torch.float32, "out")
    if tuple(out.shape) != (B * S, H):
        raise ValueError(f"listnet_bwd: out {tuple(out.shape)} must be [{B * S}, {H}]")
    _lib.call("vcg_listnet_bwd", dt_code(P_.dtype), P(P_), P(targets), P(idx.sel), P(idx.cls), P(W), P(p), P(prob),
              P(dloss), B, S, H, M, P(out), P(dW), P(db), stream())
    return out


# ----------------------------------------------------------------------------- optimiser
def sumsq(x, out, workspace=None):
    if workspace is None:
        workspace = ws(_lib.query("vcg_sumsq_ws_bytes"), x.device)
    _lib.call("vcg_sumsq", P(x), x.numel(), P(workspace), P(out), stream())
    return workspace


def adamw(p, g, m, v, wd_flags, flag_shift, lr, beta1, beta2, eps, wd, step, sumsq_dev=None, max_norm=1.0,
          grad_scale=1.0, shadow=None):
    import math
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    step_size = lr / bc1
    bc2_sqrt = math.sqrt(bc2)
    _lib.call("vcg_adamw", P(p), P(g), P(m), P(v), P(wd_flags), flag_shift, p.numel(), float(lr), float(beta1),
              float(beta2), float(eps), float(wd), float(step_size), float(bc2_sqrt), P(sumsq_dev), float(max_norm),
              float(grad_scale), P(shadow), stream())


# ----------------------------------------------------------------------------- synthetic data
def synth(out, kind, key, a, b):
    _lib.call("vcg_synth", int(kind), P(out), out.numel(), int(key) & (2**64 - 1), float(a), float(b), stream())
    return out
