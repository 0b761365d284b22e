// Fused BERT self-attention for the bf16 train / scoring path: one workgroup per (sequence, head), L <= 128 keys
// (128 < L <= 512: the tiled kernels of bert_attn_long.hip, dispatched by the entry points below), head dim 64, HF
// BertModel eager-attention semantics (model/lang/bert_hugface.py:20 via two_stream.py:172-179):
//
//   forward : S = Q K^T, P = softmax(scale * S + mask_add) (a row with no valid key is uniform over the L keys, as
//             HF's finfo.min bias gives), Pd = dropout(P), ctx = Pd V; saved: (row max, 1 / row sum) per query
//   backward: S and P recomputed from Q, K and the saved row statistics, dPd = dO V^T, dP = dropout'(dPd),
//             D = rowsum(dP o P) from the fp32 products (not rowsum(dO o O) of the bf16-rounded ctx: the same dP
//             then enters both terms of dP - D, so each dS row sums to zero as the exact softmax gradient does and the
//             rounding of O does not leak into dQ / dK), dS = scale * P o (dP - D); dQ = dS K, dK = dS^T Q, dV = Pd^T dO
//
// Nothing of size L x L touches HBM (the unfused path writes S, P and Pd per layer and reads them back): the
// forward reads Q, K, V once and writes ctx; the backward reads Q, K, V, dO, O once and writes dQ, dK, dV.
// Dropout regenerates the unfused kernels' mask exactly (same counter-hash index (z * L + q) * Lp + key).
//
// The kernels are built from the steps of bert_attn_steps.h (workgroup coordinates, tile and fragment loads, score
// tiles, the recomputed probability, dropout to fragment, the PV and dV / dK accumulations, the row store), which the
// tiled kernels share; the MFMA fragment layout is described there. What is written out here is this algorithm's own:
// the whole-row softmax (normalise, then dropout), D through LDS, and dQ from the LDS copy of dS -- only dS crosses
// waves in the backward.
#include "bert_attn_host.h"

using namespace vcg;
using namespace vcg::attn;

namespace {

// ------------------------------------------------------------------------------------------------ forward
// 4 waves; wave w owns queries 32 w .. 32 w + 31. S^T = K Q^T (A = K rows from LDS, B = Q rows from HBM), the
// softmax over the lane's 32 keys and the 4 lane groups, O^T = V^T Pd^T (A = V^T from LDS, B = Pd from registers).
// CAUSAL (bert_attn_steps.h, the causal rule): the 16 x 16 score tiles and the PV k-steps past the wave's last query
// are skipped, every element pays the key <= query compare (the whole row is unrolled in registers here).
template <bool CAUSAL>
__global__ __launch_bounds__(256) void bert_attn_fwd_kernel(const bf16_t* __restrict__ qkv,
                                                            const long long* __restrict__ mask,
                                                            bf16_t* __restrict__ ctx, float2* __restrict__ stats,
                                                            const int* __restrict__ seq, int nh, int Lmax, int Lp,
                                                            float scale, float p, uint64_t seed) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[LT * DH];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[DH * TP];
  __shared__ uint8_t kval[LT];
  const Head hd(nh, 1, seq, Lmax, Lp);
  const int L = hd.L, H = hd.H, tid = hd.tid, w = hd.w, g = hd.g, i = hd.i;
  const bf16_t* base = qkv + hd.qo;  // Q of (b, h); K at + H, V at + 2 H

  load_rm(base + H, hd.ld, L, Ks, tid);
  load_transpose(base + 2 * H, hd.ld, L, Vt, nullptr, tid);
  load_key_flags(kval, mask, hd.row0, L, tid);
  s16x8 qf[2][2];
  load_frags(qf, base, hd.ld, 32 * w, L, g, i);
  __syncthreads();
  // (a packed sequence shorter than 128 rows: tiles of keys / queries past its end add nothing and are skipped)
  if (32 * w >= L) return;  // every query of this wave is past the end (no barrier follows)

  f32x4 sacc[2][8];  // lane holds S^T[key 16 kt + 4 g + r][query 32 w + 16 qt + i]
  const bool skip = CAUSAL && causal_skip(mask, hd.row0, L);
  key_tiles<8, CAUSAL>(sacc, Ks, 0, L, qf, g, i, skip ? 32 * w : NOSKIP);
  const uint32_t vb = key_bits<8>(kval, 0, g);
  const float rs = p > 0.f ? 1.f / (1.f - p) : 1.f;
  s16x8 pf[2][4];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = 32 * w + 16 * qt + i;
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool vis = visible<CAUSAL>((vb >> (4 * kt + r)) & 1u, 16 * kt + 4 * g + r, q);
        const float v = vis ? sacc[qt][kt][r] * scale : -INFINITY;
        sacc[qt][kt][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const bool none = mx == -INFINITY;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * kt + 4 * g + r;
        const float v = sacc[qt][kt][r];
        const float e = none ? (key < L ? 1.f : 0.f) : (v == -INFINITY ? 0.f : __expf(v - mx));
        sacc[qt][kt][r] = e;
        sum += e;
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;
    if (g == 0 && q < L) stats[hd.so + q] = make_float2(mx, inv);
    dropout_frags(pf[qt], sacc[qt], q < L, hd.drop_row(q), inv, rs, p, seed, g, skip ? 32 * w + 32 : NOSKIP);
  }

  f32x4 oacc[4][2];  // lane holds O^T[d 16 dt + 4 g + r][query 32 w + 16 qt + i]
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) oacc[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
  pv_step(oacc, Vt, pf, skip ? min(L, 32 * w + 32) : L, g, i);
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = 32 * w + 16 * qt + i;
    if (q < L) store_row64(ctx + hd.co + (long long)q * H + 4 * g, oacc, qt);
  }
}

// ------------------------------------------------------------------------------------------------ backward
// 4 waves; wave w owns keys 32 w .. 32 w + 31 for S, dPd, dV and dK (A = Q / dO rows, Q^T / dO^T from LDS, B = the
// wave's K / V rows from HBM, and its P / dS fragments from registers), then queries 32 w .. 32 w + 31 for dQ
// (A = K^T from LDS, B = dS rows from the LDS copy every wave wrote). The forward's ctx is not read.
// CAUSAL: the score tiles, the dropout hashes and the dV / dK k-steps of queries before the wave's first key, and the
// dQ k-steps of keys past the wave's last query, are skipped (their P, dP and dS are exact zeros).
template <bool CAUSAL>
__global__ __launch_bounds__(256) void bert_attn_bwd_kernel(const bf16_t* __restrict__ qkv,
                                                            const bf16_t* __restrict__ dctx,
                                                            const long long* __restrict__ mask,
                                                            const float2* __restrict__ stats,
                                                            bf16_t* __restrict__ dqkv, const int* __restrict__ seq,
                                                            int nh, int Lmax, int Lp, float scale, float p,
                                                            uint64_t seed) {
  __shared__ __attribute__((aligned(16))) bf16_t Qs[LT * DH];
  __shared__ __attribute__((aligned(16))) bf16_t dOs[LT * DH];
  __shared__ __attribute__((aligned(16))) bf16_t Qt[DH * TP];
  __shared__ __attribute__((aligned(16))) bf16_t dOt[DH * TP];
  __shared__ __attribute__((aligned(16))) bf16_t Kt[DH * TP];
  __shared__ __attribute__((aligned(16))) bf16_t dSm[LT * TP];
  __shared__ float2 st[LT];
  __shared__ float Dp[4 * LT];  // per-wave partial rowsum(dP o P) over the wave's 32 keys
  __shared__ uint8_t kval[LT];
  const Head hd(nh, 1, seq, Lmax, Lp);
  const int L = hd.L, H = hd.H, tid = hd.tid, w = hd.w, g = hd.g, i = hd.i;
  const long long ld = hd.ld;
  const bf16_t* base = qkv + hd.qo;
  const bf16_t* dob = dctx + hd.co;
  bf16_t* gq = dqkv + hd.qo;

  load_transpose(base, ld, L, Qt, Qs, tid);
  load_transpose(dob, H, L, dOt, dOs, tid);
  load_transpose(base + H, ld, L, Kt, nullptr, tid);
  load_key_flags(kval, mask, hd.row0, L, tid);
  if (tid < LT) st[tid] = tid < L ? stats[hd.so + tid] : make_float2(0.f, 0.f);
  s16x8 kf[2][2], vf[2][2];
  load_frags(kf, base + H, ld, 32 * w, L, g, i);
  load_frags(vf, base + 2 * H, ld, 32 * w, L, g, i);
  __syncthreads();

  // (tiles past the end of a packed sequence add nothing: skipped; a wave whose 32 keys are all past it keeps zeros,
  // so its dS entries -- read by every wave's dQ -- are exact zeros)
  const bool wkeys = 32 * w < L;
  f32x4 sacc[8][2], pacc[8][2];  // lane holds S / dPd [query 16 qt + 4 g + r][key 32 w + 16 kt + i]
  const bool skip = CAUSAL && causal_skip(mask, hd.row0, L);
  query_tiles<8, CAUSAL>(sacc, Qs, 0, wkeys ? L : 0, kf, g, i, skip ? 32 * w : -NOSKIP);
  query_tiles<8, CAUSAL>(pacc, dOs, 0, wkeys ? L : 0, vf, g, i, skip ? 32 * w : -NOSKIP);
  const float rs = p > 0.f ? 1.f / (1.f - p) : 1.f;
  bool kv[2];
  int keyi[2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    keyi[kt] = 32 * w + 16 * kt + i;
    kv[kt] = kval[keyi[kt]] != 0;
  }
  uint64_t keepb = 0;  // bit 8 qt + 2 r + kt: element (query 16 qt + 4 g + r, key keyi[kt]) kept by dropout
#pragma unroll
  for (int qt = 0; qt < 8; ++qt) {
    const bool dead = CAUSAL && skip && 16 * qt + 15 < 32 * w;  // (wave-uniform: every key of the wave is in the future)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = 16 * qt + 4 * g + r;
      const float2 mi = st[q];
      const uint64_t rowi = hd.drop_row(q);
      float part = 0.f;
      if (!dead) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          const int key = keyi[kt];
          const float P = attn_prob(sacc[qt][kt][r], scale, mi, visible<CAUSAL>(kv[kt], key, q), key < L, q < L);
          const bool keep = q < L && key < L && dropout_keep(seed, rowi + key, p);
          const float dP = keep ? pacc[qt][kt][r] * rs : 0.f;
          keepb |= keep ? (1ull << (8 * qt + 2 * r + kt)) : 0ull;
          sacc[qt][kt][r] = P;
          pacc[qt][kt][r] = dP;
          part = fmaf(P, dP, part);
        }
        part += __shfl_xor(part, 1, 64);
        part += __shfl_xor(part, 2, 64);
        part += __shfl_xor(part, 4, 64);
        part += __shfl_xor(part, 8, 64);
      }
      if (i == 0) Dp[w * LT + q] = part;
    }
  }
  __syncthreads();  // Dp complete
#pragma unroll
  for (int qt = 0; qt < 8; ++qt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = 16 * qt + 4 * g + r;
      const float D = (Dp[q] + Dp[LT + q]) + (Dp[2 * LT + q] + Dp[3 * LT + q]);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const float P = sacc[qt][kt][r];
        const float dS = causal_ds<CAUSAL>(scale * P * (pacc[qt][kt][r] - D), keyi[kt], q);
        sacc[qt][kt][r] = ((keepb >> (8 * qt + 2 * r + kt)) & 1ull) ? P * rs : 0.f;  // Pd
        pacc[qt][kt][r] = dS;
        dSm[q * TP + keyi[kt]] = f2bf(dS);
      }
    }

  // dV^T = dO^T Pd, dK^T = Q^T dS over the 128 queries (k-step s: queries {32 s + 4 g + r, 32 s + 16 + 4 g + r})
  f32x4 dv[4][2], dk[4][2];  // lane holds dV^T / dK^T [d 16 dt + 4 g + r][key 32 w + 16 kt + i]
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) dv[dt][kt] = dk[dt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (wkeys && 32 * s < L && !(skip && s < w))
      dvdk_step(dv, dk, sacc[2 * s], sacc[2 * s + 1], pacc[2 * s], pacc[2 * s + 1], dOt, Qt, 32 * s, g, i);
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = keyi[kt];
    if (key < L) {
      bf16_t* o = gq + (long long)key * ld + 4 * g;
      store_row64(o + H, dk, kt);
      store_row64(o + 2 * H, dv, kt);
    }
  }
  __syncthreads();  // dSm complete

  // dQ^T = K^T dS^T for queries 32 w + 16 qt + i (k-step s: keys 32 s + 8 g .. + 7)
  f32x4 dq[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) dq[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (32 * w >= L || 32 * s >= L || (skip && s > w)) continue;  // (the wave's queries / this step's keys past the
                                                                     // end, or keys all in the wave's future)
    s16x8 sbq[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
      sbq[qt] = *reinterpret_cast<const s16x8*>(dSm + (32 * w + 16 * qt + i) * TP + 32 * s + 8 * g);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const s16x8 ka = *reinterpret_cast<const s16x8*>(Kt + (16 * dt + i) * TP + 32 * s + 8 * g);
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) dq[dt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, sbq[qt], dq[dt][qt], 0, 0, 0);
    }
  }
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = 32 * w + 16 * qt + i;
    if (q < L) store_row64(gq + (long long)q * ld + 4 * g, dq, qt);
  }
}

// The one argument check of the four entry points (io: ctx / dqkv). *nT: the 128-row tiles of the stats rows, and
// the tiled kernels' grid is one workgroup per (sequence, head, tile)
int attn_check(const char* fn, const void* qkv, const void* io, const void* stats, int B, int nh, int L, int Lp,
               int* nT) {
  if (!qkv || !io || !stats || B < 0 || nh <= 0 || L < 0 || Lp < L) {
    set_error(std::string(fn) + ": invalid arguments");
    return VCG_ERR_INVALID;
  }
  if (L > LMAX) {
    set_error(std::string(fn) + ": L > 512 is not supported by the fused kernels");
    return VCG_ERR_UNSUPPORTED;
  }
  *nT = stats_tiles(L);
  if ((long long)B * nh * *nT > 0x7fffffffLL) {  // (more workgroups than a grid holds)
    set_error(std::string(fn) + ": the tiled kernels take 128 < L <= 512");
    return VCG_ERR_UNSUPPORTED;
  }
  return VCG_OK;
}

}  // namespace

// (the layout: bert_attn_host.h)
VCG_API long long vcg_bert_attn_stats_bytes(int B, int nh, int L) {
  if (B < 0 || nh < 0 || L < 0) return 0;
  return stats_rows(B, nh, L) * (long long)(L <= LT ? sizeof(float2) : sizeof(float2) + sizeof(float));
}

// Packed (unpadded) sequences: sequence b's rows are seq[b] .. seq[b + 1] - 1 of qkv / ctx (at most Lmax <= 512 of
// them; Lmax > 128: the tiled kernels of bert_attn_long.hip), mask the key flags of those rows (NULL: every row is a
// key); stats and the dropout counters keep the padded [B][nh][Lmax] index space, so a sequence whose kept rows are a
// prefix of its padded rows gets the padded result. seq NULL: padded, sequence b at rows b Lmax .. b Lmax + Lmax - 1.
// flags: VCG_ATTN_CAUSAL (bert_attn_steps.h, the causal rule); 0 is vcg_bert_attn_fwd_varlen.
VCG_API int vcg_bert_attn_fwd_ex(const void* qkv, const long long* mask, const int* seq, void* ctx, void* stats,
                                 int B, int nh, int Lmax, int Lp, float scale, float dropout_p,
                                 unsigned long long seed, int flags, hipStream_t s) {
  if (flags & ~VCG_ATTN_CAUSAL) {
    set_error("vcg_bert_attn_fwd: unknown flags");
    return VCG_ERR_INVALID;
  }
  const bool causal = (flags & VCG_ATTN_CAUSAL) != 0;
  if (B == 0 || Lmax == 0) return VCG_OK;
  int nT;
  const int rc = attn_check("vcg_bert_attn_fwd", qkv, ctx, stats, B, nh, Lmax, Lp, &nT);
  if (rc != VCG_OK) return rc;
  if (Lmax > LT)
    return bert_attn_long_fwd(qkv, mask, seq, ctx, stats, B, nh, Lmax, Lp, nT, scale, dropout_p, seed, causal, s);
  if (causal)
    hipLaunchKernelGGL(bert_attn_fwd_kernel<true>, dim3(B * nh), dim3(256), 0, s, (const bf16_t*)qkv, mask,
                       (bf16_t*)ctx, (float2*)stats, seq, nh, Lmax, Lp, scale, dropout_p, (uint64_t)seed);
  else
    hipLaunchKernelGGL(bert_attn_fwd_kernel<false>, dim3(B * nh), dim3(256), 0, s, (const bf16_t*)qkv, mask,
                       (bf16_t*)ctx, (float2*)stats, seq, nh, Lmax, Lp, scale, dropout_p, (uint64_t)seed);
  VCG_CHECK_HIP(hipGetLastError());
  return VCG_OK;
}

VCG_API int vcg_bert_attn_fwd_varlen(const void* qkv, const long long* mask, const int* seq, void* ctx, void* stats,
                                     int B, int nh, int Lmax, int Lp, float scale, float dropout_p,
                                     unsigned long long seed, hipStream_t s) {
  return vcg_bert_attn_fwd_ex(qkv, mask, seq, ctx, stats, B, nh, Lmax, Lp, scale, dropout_p, seed, 0, s);
}

VCG_API int vcg_bert_attn_fwd(const void* qkv, const long long* mask, void* ctx, void* stats, int B, int nh, int L,
                              int Lp, float scale, float dropout_p, unsigned long long seed, hipStream_t s) {
  return vcg_bert_attn_fwd_varlen(qkv, mask, nullptr, ctx, stats, B, nh, L, Lp, scale, dropout_p, seed, s);
}

VCG_API int vcg_bert_attn_bwd_ex(const void* qkv, const void* dctx, const long long* mask, const int* seq,
                                 const void* stats, void* dqkv, int B, int nh, int Lmax, int Lp, float scale,
                                 float dropout_p, unsigned long long seed, int flags, hipStream_t s) {
  if (flags & ~VCG_ATTN_CAUSAL) {
    set_error("vcg_bert_attn_bwd: unknown flags");
    return VCG_ERR_INVALID;
  }
  const bool causal = (flags & VCG_ATTN_CAUSAL) != 0;
  if (B == 0 || Lmax == 0) return VCG_OK;
  if (!dctx) {
    set_error("vcg_bert_attn_bwd: invalid arguments");
    return VCG_ERR_INVALID;
  }
  int nT;
  const int rc = attn_check("vcg_bert_attn_bwd", qkv, dqkv, stats, B, nh, Lmax, Lp, &nT);
  if (rc != VCG_OK) return rc;
  if (Lmax > LT)  // (the tiled backward keeps its D vector in the stats buffer's tail)
    return bert_attn_long_bwd(qkv, dctx, mask, seq, const_cast<void*>(stats), dqkv, B, nh, Lmax, Lp, nT, scale,
                              dropout_p, seed, causal, s);
  if (causal)
    hipLaunchKernelGGL(bert_attn_bwd_kernel<true>, dim3(B * nh), dim3(256), 0, s, (const bf16_t*)qkv,
                       (const bf16_t*)dctx, mask, (const float2*)stats, (bf16_t*)dqkv, seq, nh, Lmax, Lp, scale,
                       dropout_p, (uint64_t)seed);
  else
    hipLaunchKernelGGL(bert_attn_bwd_kernel<false>, dim3(B * nh), dim3(256), 0, s, (const bf16_t*)qkv,
                       (const bf16_t*)dctx, mask, (const float2*)stats, (bf16_t*)dqkv, seq, nh, Lmax, Lp, scale,
                       dropout_p, (uint64_t)seed);
  VCG_CHECK_HIP(hipGetLastError());
  return VCG_OK;
}

VCG_API int vcg_bert_attn_bwd_varlen(const void* qkv, const void* dctx, const long long* mask, const int* seq,
                                     const void* stats, void* dqkv, int B, int nh, int Lmax, int Lp, float scale,
                                     float dropout_p, unsigned long long seed, hipStream_t s) {
  return vcg_bert_attn_bwd_ex(qkv, dctx, mask, seq, stats, dqkv, B, nh, Lmax, Lp, scale, dropout_p, seed, 0, s);
}

VCG_API int vcg_bert_attn_bwd(const void* qkv, const void* dctx, const void* ctx, const long long* mask,
                              const void* stats, void* dqkv, int B, int nh, int L, int Lp, float scale,
                              float dropout_p, unsigned long long seed, hipStream_t s) {
  (void)ctx;  // (kept in the signature: the backward no longer needs the forward's output)
  return vcg_bert_attn_bwd_varlen(qkv, dctx, mask, nullptr, stats, dqkv, B, nh, L, Lp, scale, dropout_p, seed, s);
}
