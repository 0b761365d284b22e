// Fused BERT self-attention for texts of 129 to 512 tokens (bf16, head dim 64): bert_attn.hip's semantics (HF
// BertModel eager attention, model/lang/bert_hugface.py:20 via two_stream.py:172-179) on 128 x 128 tiles with an online
// softmax, so that nothing of size L x L touches HBM -- only float2 (row max, 1 / row sum) and float D per query.
//
//   forward  (grid: query tiles x sequences x heads): the workgroup sweeps the key tiles; per tile S^T = K Q^T, the
//             running row max m and sum l are updated (a lane holds S^T[key][query] and O^T[d][query], so m, l and the
//             rescale factor exp(m_old - m_new) are per-lane scalars), dropout acts on the unnormalised tile
//             probabilities exp(s - m), O^T += V^T Pd^T, and 1 / l is applied once at the end.
//   backward (deterministic, no atomics), two kernels:
//     dq : query-tile-owned like the forward, two sweeps over the key tiles. Sweep 1 builds D = rowsum(dP o P) from the
//          fp32 products (bert_attn.hip's header: not rowsum(dO o O)) and stores it; sweep 2 recomputes P and dP, forms
//          dS = scale P o (dP - D) and accumulates dQ^T = K^T dS^T in registers.
//     dkv: key-tile-owned (bert_attn.hip's backward without its dQ third), sweeps the query tiles with the saved row
//          statistics and D: dV^T += dO^T Pd, dK^T += Q^T dS.
//
// A sequence without any valid key attends uniformly over its L keys (HF's finfo.min bias): a property of the key
// mask, decided once per workgroup in the forward (every key then counts as valid with score 0) and saved as row
// max = -inf, 1 / sum = 1 / L, which is how the backward recognises it. While a row's running max is still -inf (a
// wholly masked tile before the first valid key) the exponentials are taken against 0 instead: every term is
// exp(-inf) = 0 and no inf - inf arises. Tiles past the end of a packed sequence are not visited; rows past it load
// as zeros. The dropout counter of (z, q, key) is (z Lmax + q) Lp + key, the unfused kernels' index.
//
// Budget per workgroup (256 threads = 4 waves, one per SIMD; registers as hipcc reports them for gfx950). Every kernel
// is built for two workgroups per CU (__launch_bounds__(256, 2): at most 256 registers, LDS at most 80 KiB); the
// kernels are bound by the per-element VALU work (exp, the dropout hash with its two quarter-rate 32-bit multiplies),
// not by the MFMAs, so the second workgroup -- its MFMAs and tile loads under the first one's VALU -- is what pays:
// the backward took 1.98 ms at one workgroup per CU and 0.98 ms at two (B = 64, L = 512, p = 0.1).
//   fwd: LDS 33.4 KiB (K 16 + V^T 17 + key flags); S^T 64 + O^T 32 accumulators; 225 VGPRs, no spill
//   dq : LDS 57.1 KiB (K, V row-major 32 + K^T 17 + dropout bits 8); a tile's keys in two halves of 64, so S^T 32 +
//        dPd^T 32 + dQ^T 32 accumulators; 256 VGPRs, no spill. The lane's dropout decisions of sweep 1 are kept as
//        bits in LDS (each thread rereads its own words) and sweep 2 does not hash again.
//   dkv: LDS 67.5 KiB (Q, dO row-major 32 + Q^T, dO^T 34 + stats, D 1.5); a tile's queries in two halves of 64, so S 32
//        + dPd 32 + dV^T, dK^T 64 accumulators; 256 VGPRs, 4 spilled (20 B of scratch per lane)
// The tiles are single-buffered (two barriers per tile); at L <= 512 a sweep is at most 4 tiles.
#include <type_traits>

#include "bert_attn_tiles.h"

using namespace vcg;
using namespace vcg::attn;

namespace {

// rows 0 .. 127 of a [nrows][ld] row-major source (rows >= nrows zero) -> the swizzled row-major tile rm[row][64]
__device__ __forceinline__ void load_rm(const bf16_t* src, long long ld, int nrows, bf16_t* rm, int tid) {
  for (int c = tid; c < LT * 8; c += 256) {
    const int r = c >> 3, ch = c & 7;
    *reinterpret_cast<uint4*>(rm + r * DH + 8 * swz(r, ch)) = ld16(src + (long long)r * ld + 8 * ch, r < nrows);
  }
}

// ------------------------------------------------------------------------------------------------ forward
// blockIdx.x = z * nT + query tile; wave w owns queries q0 + 32 w .. + 31 (fragments as bert_attn_fwd_kernel)
__global__ __launch_bounds__(256, 2) void bert_attn_long_fwd_kernel(const bf16_t* __restrict__ qkv,
                                                                 const long long* __restrict__ mask,
                                                                 bf16_t* __restrict__ ctx, float2* __restrict__ stats,
                                                                 const int* __restrict__ seq, int nh, int Lmax, int Lp,
                                                                 int nT, float scale, float p, uint64_t seed) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[LT * DH];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[DH * TP];
  __shared__ uint8_t kval[LT];
  const int z = blockIdx.x / nT, q0 = LT * (blockIdx.x - z * nT), b = z / nh, h = z - b * nh;
  const int H = nh * DH;
  const long long ld = 3LL * H;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, i = lane & 15;
  const int row0 = seq ? seq[b] : b * Lmax;
  const int L = seq ? seq[b + 1] - row0 : Lmax;
  if (q0 >= L) return;  // (a packed sequence that ends before this query tile; block-uniform, before any barrier)
  const bf16_t* base = qkv + (long long)row0 * ld + h * DH;  // Q of (b, h); K at + H, V at + 2 H

  int anyk = mask == nullptr;
  if (mask)
    for (int k = tid; k < L; k += 256) anyk |= mask[(long long)row0 + k] != 0;
  const bool none = !__syncthreads_or(anyk);  // no valid key in the whole sequence: uniform attention

  s16x8 qf[2][2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int q = q0 + 32 * w + 16 * qt + i;
      const uint4 u = ld16(base + (long long)q * ld + 8 * (4 * s + g), q < L);
      qf[qt][s] = __builtin_bit_cast(s16x8, u);
    }
  const bool wact = q0 + 32 * w < L;  // (else every query of this wave is past the end: it only loads and syncs)
  const float rs = p > 0.f ? 1.f / (1.f - p) : 1.f;
  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};
  f32x4 oacc[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) oacc[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < L; k0 += LT) {
    const int Lt = L - k0;  // keys of this tile (>= 128: a full tile)
    load_rm(base + (long long)k0 * ld + H, ld, Lt, Ks, tid);
    load_transpose(base + (long long)k0 * ld + 2 * H, ld, Lt, Vt, nullptr, tid);
    if (tid < LT) kval[tid] = tid < Lt && (none || mask == nullptr || mask[(long long)row0 + k0 + tid] != 0);
    __syncthreads();
    if (wact) {
      f32x4 sacc[2][8];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int kt = 0; kt < 8; ++kt) sacc[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < 8; ++kt)
        if (16 * kt < Lt) {
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const s16x8 kf = frag_rm(Ks, 16 * kt + i, 4 * s + g);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
              sacc[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[qt][s], sacc[qt][kt], 0, 0, 0);
          }
        }
      // lane holds S^T[key k0 + 16 kt + 4 g + r][query q0 + 32 w + 16 qt + i]
      uint32_t vb = 0;  // bit 4 kt + r: that key is valid
#pragma unroll
      for (int kt = 0; kt < 8; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) vb |= kval[16 * kt + 4 * g + r] ? (1u << (4 * kt + r)) : 0u;
      s16x8 pf[2][4];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + 32 * w + 16 * qt + i;
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = ((vb >> (4 * kt + r)) & 1u) ? (none ? 0.f : sacc[qt][kt][r] * scale) : -INFINITY;
            sacc[qt][kt][r] = v;
            mx = fmaxf(mx, v);
          }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m[qt], mx);
        const float ms = mn == -INFINITY ? 0.f : mn;  // (still no valid key: exp(-inf - 0) = 0, never inf - inf)
        const float alpha = __expf(m[qt] - ms);       // (m = -inf: 0, and O, l are 0)
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = __expf(sacc[qt][kt][r] - ms);
            sacc[qt][kt][r] = e;
            sum += e;
          }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        l[qt] = fmaf(l[qt], alpha, sum);
        m[qt] = mn;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r) oacc[dt][qt][r] *= alpha;
        const uint64_t rowi = ((uint64_t)z * Lmax + q) * (uint64_t)Lp + k0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          float a[4], c[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k1 = 32 * s + 4 * g + r, k2 = k1 + 16;
            a[r] = (q < L && dropout_keep(seed, rowi + k1, p)) ? sacc[qt][2 * s][r] * rs : 0.f;
            c[r] = (q < L && dropout_keep(seed, rowi + k2, p)) ? sacc[qt][2 * s + 1][r] * rs : 0.f;
          }
          pf[qt][s] = pack8(a, c);
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (32 * s < Lt) {
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            const s16x8 vf = frag_split(Vt, 16 * dt + i, 32 * s + 4 * g);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
              oacc[dt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qt][s], oacc[dt][qt], 0, 0, 0);
          }
        }
    }
    __syncthreads();  // every wave is done with this tile before the next one overwrites it
  }
  if (!wact) return;
  // lane holds O^T[d 16 dt + 4 g + r][query q0 + 32 w + 16 qt + i], unnormalised
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = q0 + 32 * w + 16 * qt + i;
    if (q < L) {
      const float inv = 1.f / l[qt];
      if (g == 0) stats[(long long)z * (nT * LT) + q] = make_float2(none ? -INFINITY : m[qt], inv);
      bf16_t* o = ctx + ((long long)row0 + q) * H + h * DH + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        *reinterpret_cast<uint2*>(o + 16 * dt) = make_uint2(pack2(oacc[dt][qt][0] * inv, oacc[dt][qt][1] * inv),
                                                            pack2(oacc[dt][qt][2] * inv, oacc[dt][qt][3] * inv));
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward: D, dQ
// blockIdx.x = z * nT + query tile; wave w owns queries q0 + 32 w .. + 31. S^T = K Q^T and dPd^T = V dO^T (A = K / V
// rows from LDS, B = the wave's Q / dO rows from HBM), dQ^T = K^T dS^T (A = K^T from LDS, B = dS from registers).
__global__ __launch_bounds__(256, 2) void bert_attn_long_dq_kernel(const bf16_t* __restrict__ qkv,
                                                                const bf16_t* __restrict__ dctx,
                                                                const long long* __restrict__ mask,
                                                                const float2* __restrict__ stats, float* __restrict__ Dv,
                                                                bf16_t* __restrict__ dqkv, const int* __restrict__ seq,
                                                                int nh, int Lmax, int Lp, int nT, float scale, float p,
                                                                uint64_t seed) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[LT * DH];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[LT * DH];
  __shared__ __attribute__((aligned(16))) bf16_t Kt[DH * TP];
  __shared__ uint32_t keepw[(LMAX / 64) * 256];  // [64-key half][thread]: each thread rereads only its own words
  __shared__ uint8_t kval[LT];
  const int z = blockIdx.x / nT, q0 = LT * (blockIdx.x - z * nT), b = z / nh, h = z - b * nh;
  const int H = nh * DH;
  const long long ld = 3LL * H;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, i = lane & 15;
  const int row0 = seq ? seq[b] : b * Lmax;
  const int L = seq ? seq[b + 1] - row0 : Lmax;
  if (q0 >= L) return;  // (block-uniform, before any barrier)
  const bf16_t* base = qkv + (long long)row0 * ld + h * DH;
  const bf16_t* dob = dctx + (long long)row0 * H + h * DH;
  const long long so = (long long)z * (nT * LT);

  s16x8 qf[2][2], df[2][2];
  float mrow[2], irow[2];
  bool nrow[2];  // the row of a sequence without any key: P = 1 / L on every key
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = q0 + 32 * w + 16 * qt + i;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      qf[qt][s] = __builtin_bit_cast(s16x8, ld16(base + (long long)q * ld + 8 * (4 * s + g), q < L));
      df[qt][s] = __builtin_bit_cast(s16x8, ld16(dob + (long long)q * H + 8 * (4 * s + g), q < L));
    }
    const float2 mi = q < L ? stats[so + q] : make_float2(0.f, 0.f);  // (q >= L: P = 0)
    nrow[qt] = mi.x == -INFINITY;
    mrow[qt] = nrow[qt] ? 0.f : mi.x;
    irow[qt] = mi.y;
  }
  const bool wact = q0 + 32 * w < L;
  const float rs = p > 0.f ? 1.f / (1.f - p) : 1.f;
  float D[2] = {0.f, 0.f};
  f32x4 dq[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) dq[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int sweep = 0; sweep < 2; ++sweep) {  // 0: D; 1: dS and dQ
    for (int k0 = 0; k0 < L; k0 += LT) {
      const int Lt = L - k0;
      if (sweep == 0) load_rm(base + (long long)k0 * ld + H, ld, Lt, Ks, tid);
      else load_transpose(base + (long long)k0 * ld + H, ld, Lt, Kt, Ks, tid);
      load_rm(base + (long long)k0 * ld + 2 * H, ld, Lt, Vs, tid);
      if (tid < LT) kval[tid] = tid < Lt && (mask == nullptr || mask[(long long)row0 + k0 + tid] != 0);
      __syncthreads();
      // one half (64 keys) of the tile; SW = the sweep, a compile-time constant inside
      auto half = [&](auto SW, int kh) {
        constexpr int sw = decltype(SW)::value;
        f32x4 sacc[2][4], pacc[2][4];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
          for (int kt = 0; kt < 4; ++kt) sacc[qt][kt] = pacc[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
          if (kh + 16 * kt < Lt) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
              const s16x8 kf = frag_rm(Ks, kh + 16 * kt + i, 4 * s + g);
              const s16x8 vf = frag_rm(Vs, kh + 16 * kt + i, 4 * s + g);
#pragma unroll
              for (int qt = 0; qt < 2; ++qt) {
                sacc[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[qt][s], sacc[qt][kt], 0, 0, 0);
                pacc[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, df[qt][s], pacc[qt][kt], 0, 0, 0);
              }
            }
          }
        // lane holds S^T / dPd^T [key k0 + kh + 16 kt + 4 g + r][query q0 + 32 w + 16 qt + i]
        uint32_t vb = 0;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) vb |= kval[kh + 16 * kt + 4 * g + r] ? (1u << (4 * kt + r)) : 0u;
        // the lane's 32 dropout decisions of this half (bit 16 qt + 4 kt + r): hashed in sweep 0, reread in sweep 1
        uint32_t* kw = keepw + ((k0 + kh) >> 6) * 256 + tid;
        uint32_t kb = sw == 0 ? 0u : *kw;
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          const int q = q0 + 32 * w + 16 * qt + i;
          const uint64_t rowi = ((uint64_t)z * Lmax + q) * (uint64_t)Lp + k0;
          float part = 0.f;
#pragma unroll
          for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int kl = kh + 16 * kt + 4 * g + r;
              float P;
              if (nrow[qt]) P = kl < Lt ? irow[qt] : 0.f;
              else P = ((vb >> (4 * kt + r)) & 1u) ? __expf(sacc[qt][kt][r] * scale - mrow[qt]) * irow[qt] : 0.f;
              const uint32_t bit = 1u << (16 * qt + 4 * kt + r);
              bool keep;
              if constexpr (sw == 0) {
                keep = q < L && kl < Lt && dropout_keep(seed, rowi + kl, p);
                kb |= keep ? bit : 0u;
              } else {
                keep = (kb & bit) != 0;
              }
              const float dP = keep ? pacc[qt][kt][r] * rs : 0.f;
              if constexpr (sw == 0) part = fmaf(P, dP, part);
              else sacc[qt][kt][r] = scale * P * (dP - D[qt]);  // dS
            }
          if constexpr (sw == 0) D[qt] += part;
        }
        if constexpr (sw == 0) *kw = kb;
        if constexpr (sw == 1) {
#pragma unroll
          for (int s = 0; s < 2; ++s)
            if (kh + 32 * s < Lt) {
              s16x8 sf[2];
#pragma unroll
              for (int qt = 0; qt < 2; ++qt) {
                float a[4], c[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  a[r] = sacc[qt][2 * s][r];
                  c[r] = sacc[qt][2 * s + 1][r];
                }
                sf[qt] = pack8(a, c);
              }
#pragma unroll
              for (int dt = 0; dt < 4; ++dt) {
                const s16x8 ka = frag_split(Kt, 16 * dt + i, kh + 32 * s + 4 * g);
#pragma unroll
                for (int qt = 0; qt < 2; ++qt)
                  dq[dt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, sf[qt], dq[dt][qt], 0, 0, 0);
              }
            }
        }
      };
#pragma unroll 1
      for (int kh = 0; kh < (wact ? LT : 0) && kh < Lt; kh += 64) {  // (a wave past the end only loads and syncs)
        if (sweep == 0) half(std::integral_constant<int, 0>{}, kh);
        else half(std::integral_constant<int, 1>{}, kh);
      }
      __syncthreads();
    }
    if (sweep == 0 && wact) {  // the lane groups' partial sums over their keys, in a fixed order
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + 32 * w + 16 * qt + i;
        D[qt] += __shfl_xor(D[qt], 16, 64);
        D[qt] += __shfl_xor(D[qt], 32, 64);
        if (g == 0 && q < L) Dv[so + q] = D[qt];
      }
    }
  }
  if (!wact) return;
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = q0 + 32 * w + 16 * qt + i;
    if (q < L) {
      bf16_t* o = dqkv + ((long long)row0 + q) * ld + h * DH + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        *reinterpret_cast<uint2*>(o + 16 * dt) =
            make_uint2(pack2(dq[dt][qt][0], dq[dt][qt][1]), pack2(dq[dt][qt][2], dq[dt][qt][3]));
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward: dK, dV
// blockIdx.x = z * nT + key tile; wave w owns keys k0 + 32 w .. + 31 (fragments as bert_attn_bwd_kernel: A = Q / dO
// rows, Q^T / dO^T from LDS, B = the wave's K / V rows from HBM and its Pd / dS fragments from registers).
__global__ __launch_bounds__(256, 2) void bert_attn_long_dkv_kernel(const bf16_t* __restrict__ qkv,
                                                                 const bf16_t* __restrict__ dctx,
                                                                 const long long* __restrict__ mask,
                                                                 const float2* __restrict__ stats,
                                                                 const float* __restrict__ Dv, bf16_t* __restrict__ dqkv,
                                                                 const int* __restrict__ seq, int nh, int Lmax, int Lp,
                                                                 int nT, float scale, float p, uint64_t seed) {
  __shared__ __attribute__((aligned(16))) bf16_t Qs[LT * DH];
  __shared__ __attribute__((aligned(16))) bf16_t dOs[LT * DH];
  __shared__ __attribute__((aligned(16))) bf16_t Qt[DH * TP];
  __shared__ __attribute__((aligned(16))) bf16_t dOt[DH * TP];
  __shared__ float2 st[LT];
  __shared__ float Ds[LT];
  const int z = blockIdx.x / nT, k0 = LT * (blockIdx.x - z * nT), b = z / nh, h = z - b * nh;
  const int H = nh * DH;
  const long long ld = 3LL * H;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, i = lane & 15;
  const int row0 = seq ? seq[b] : b * Lmax;
  const int L = seq ? seq[b + 1] - row0 : Lmax;
  if (k0 >= L) return;  // (block-uniform, before any barrier)
  const bf16_t* base = qkv + (long long)row0 * ld + h * DH;
  const bf16_t* dob = dctx + (long long)row0 * H + h * DH;
  bf16_t* gq = dqkv + (long long)row0 * ld + h * DH;
  const long long so = (long long)z * (nT * LT);

  s16x8 kf[2][2], vf[2][2];
  bool kv[2];
  int keyi[2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = k0 + 32 * w + 16 * kt + i;
    keyi[kt] = key;
    kv[kt] = key < L && (mask == nullptr || mask[(long long)row0 + key] != 0);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      kf[kt][s] = __builtin_bit_cast(s16x8, ld16(base + (long long)key * ld + H + 8 * (4 * s + g), key < L));
      vf[kt][s] = __builtin_bit_cast(s16x8, ld16(base + (long long)key * ld + 2 * H + 8 * (4 * s + g), key < L));
    }
  }
  const bool wact = k0 + 32 * w < L;
  const float rs = p > 0.f ? 1.f / (1.f - p) : 1.f;
  f32x4 dv[4][2], dk[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) dv[dt][kt] = dk[dt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int q0 = 0; q0 < L; q0 += LT) {
    const int Lq = L - q0;
    load_transpose(base + (long long)q0 * ld, ld, Lq, Qt, Qs, tid);
    load_transpose(dob + (long long)q0 * H, H, Lq, dOt, dOs, tid);
    if (tid < LT) {
      st[tid] = tid < Lq ? stats[so + q0 + tid] : make_float2(0.f, 0.f);
      Ds[tid] = tid < Lq ? Dv[so + q0 + tid] : 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int qh = 0; qh < (wact ? LT : 0) && qh < Lq; qh += 64) {  // the tile's queries in two halves of 64
      f32x4 sacc[4][2], pacc[4][2];
#pragma unroll
      for (int qt = 0; qt < 4; ++qt)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) sacc[qt][kt] = pacc[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int qt = 0; qt < 4; ++qt)
        if (qh + 16 * qt < Lq) {
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const s16x8 qa = frag_rm(Qs, qh + 16 * qt + i, 4 * s + g);
            const s16x8 da = frag_rm(dOs, qh + 16 * qt + i, 4 * s + g);
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
              sacc[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa, kf[kt][s], sacc[qt][kt], 0, 0, 0);
              pacc[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da, vf[kt][s], pacc[qt][kt], 0, 0, 0);
            }
          }
        }
      // lane holds S / dPd [query q0 + qh + 16 qt + 4 g + r][key k0 + 32 w + 16 kt + i]
#pragma unroll
      for (int qt = 0; qt < 4; ++qt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ql = qh + 16 * qt + 4 * g + r;
          const float2 mi = st[ql];
          const float D = Ds[ql];
          const uint64_t rowi = ((uint64_t)z * Lmax + q0 + ql) * (uint64_t)Lp;
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            const int key = keyi[kt];
            float P = 0.f;
            if (ql < Lq) {
              if (mi.x == -INFINITY) P = key < L ? mi.y : 0.f;
              else P = kv[kt] ? __expf(sacc[qt][kt][r] * scale - mi.x) * mi.y : 0.f;
            }
            const bool keep = ql < Lq && key < L && dropout_keep(seed, rowi + key, p);
            const float dP = keep ? pacc[qt][kt][r] * rs : 0.f;
            sacc[qt][kt][r] = keep ? P * rs : 0.f;    // Pd
            pacc[qt][kt][r] = scale * P * (dP - D);   // dS
          }
        }
      // dV^T += dO^T Pd, dK^T += Q^T dS (k-step s: queries {32 s + 4 g + r, 32 s + 16 + 4 g + r} of the half)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (qh + 32 * s >= Lq) continue;
        s16x8 pb[2], sb[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          float a[4], c[4], e[4], f[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            a[r] = sacc[2 * s][kt][r];
            c[r] = sacc[2 * s + 1][kt][r];
            e[r] = pacc[2 * s][kt][r];
            f[r] = pacc[2 * s + 1][kt][r];
          }
          pb[kt] = pack8(a, c);
          sb[kt] = pack8(e, f);
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const s16x8 oa = frag_split(dOt, 16 * dt + i, qh + 32 * s + 4 * g);
          const s16x8 qa = frag_split(Qt, 16 * dt + i, qh + 32 * s + 4 * g);
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            dv[dt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oa, pb[kt], dv[dt][kt], 0, 0, 0);
            dk[dt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa, sb[kt], dk[dt][kt], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  if (!wact) return;
  // lane holds dV^T / dK^T [d 16 dt + 4 g + r][key k0 + 32 w + 16 kt + i]
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = keyi[kt];
    if (key < L) {
      bf16_t* o = gq + (long long)key * ld + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        *reinterpret_cast<uint2*>(o + H + 16 * dt) =
            make_uint2(pack2(dk[dt][kt][0], dk[dt][kt][1]), pack2(dk[dt][kt][2], dk[dt][kt][3]));
        *reinterpret_cast<uint2*>(o + 2 * H + 16 * dt) =
            make_uint2(pack2(dv[dt][kt][0], dv[dt][kt][1]), pack2(dv[dt][kt][2], dv[dt][kt][3]));
      }
    }
  }
}

}  // namespace

namespace vcg {

static int long_tiles(const char* fn, int B, int nh, int Lmax, int* nT) {
  *nT = (Lmax + LT - 1) / LT;
  if (Lmax <= LT || Lmax > LMAX || (long long)B * nh * *nT > 0x7fffffffLL) {
    set_error(std::string(fn) + ": the tiled kernels take 128 < L <= 512");
    return VCG_ERR_UNSUPPORTED;
  }
  return VCG_OK;
}

int bert_attn_long_fwd(const void* qkv, const long long* mask, const int* seq, void* ctx, void* stats, int B, int nh,
                       int Lmax, int Lp, float scale, float dropout_p, unsigned long long seed, hipStream_t s) {
  int nT;
  const int rc = long_tiles("vcg_bert_attn_fwd", B, nh, Lmax, &nT);
  if (rc != VCG_OK) return rc;
  hipLaunchKernelGGL(bert_attn_long_fwd_kernel, dim3(B * nh * nT), dim3(256), 0, s, (const bf16_t*)qkv, mask,
                     (bf16_t*)ctx, (float2*)stats, seq, nh, Lmax, Lp, nT, scale, dropout_p, (uint64_t)seed);
  VCG_CHECK_HIP(hipGetLastError());
  return VCG_OK;
}

int bert_attn_long_bwd(const void* qkv, const void* dctx, const long long* mask, const int* seq, void* stats,
                       void* dqkv, int B, int nh, int Lmax, int Lp, float scale, float dropout_p,
                       unsigned long long seed, hipStream_t s) {
  int nT;
  const int rc = long_tiles("vcg_bert_attn_bwd", B, nh, Lmax, &nT);
  if (rc != VCG_OK) return rc;
  const float2* st = (const float2*)stats;
  float* Dv = (float*)(st + (long long)B * nh * nT * LT);  // (the buffer's tail: vcg_bert_attn_stats_bytes)
  hipLaunchKernelGGL(bert_attn_long_dq_kernel, dim3(B * nh * nT), dim3(256), 0, s, (const bf16_t*)qkv,
                     (const bf16_t*)dctx, mask, st, Dv, (bf16_t*)dqkv, seq, nh, Lmax, Lp, nT, scale, dropout_p,
                     (uint64_t)seed);
  VCG_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(bert_attn_long_dkv_kernel, dim3(B * nh * nT), dim3(256), 0, s, (const bf16_t*)qkv,
                     (const bf16_t*)dctx, mask, st, (const float*)Dv, (bf16_t*)dqkv, seq, nh, Lmax, Lp, nT, scale,
                     dropout_p, (uint64_t)seed);
  VCG_CHECK_HIP(hipGetLastError());
  return VCG_OK;
}

}  // namespace vcg
