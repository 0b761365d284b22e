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
//     dkv: key-tile-owned, sweeps the query tiles with the saved row statistics and D: dV^T += dO^T Pd,
//          dK^T += Q^T dS.
//
// The kernels are built from the steps of bert_attn_steps.h, shared with the L <= 128 kernels of bert_attn.hip: the
// forward and dq hold key-major tiles like that file's forward, dkv query-major tiles like its backward. What is
// written out here is this algorithm's own: the online softmax, dq's two sweeps with the dropout bits kept in LDS, and
// the sweeps in halves of 64. dkv's query-tile body (dkv_query_tile) is shared with pegasus.hip's cross-attention.
//
// A sequence without any valid key attends uniformly over its L keys (HF's finfo.min bias): a property of the key
// mask, decided once per workgroup in the forward (every key then counts as valid with score 0) and saved as row
// max = -inf, 1 / sum = 1 / L, which is how the backward recognises it (attn_prob). While a row's running max is still
// -inf (a wholly masked tile before the first valid key) the exponentials are taken against 0 instead: every term is
// exp(-inf) = 0 and no inf - inf arises. Tiles past the end of a packed sequence are not visited; rows past it load
// as zeros. The dropout counter of (z, q, key) is (z Lmax + q) Lp + key, the unfused kernels' index.
//
// Budget per workgroup (256 threads = 4 waves, one per SIMD; registers as hipcc reports them for gfx950). Every kernel
// is built for two workgroups per CU (__launch_bounds__(256, 2): at most 256 registers, LDS at most 80 KiB); the
// kernels are bound by the per-element VALU work (exp, the dropout hash with its two quarter-rate 32-bit multiplies),
// not by the MFMAs, so the second workgroup -- its MFMAs and tile loads under the first one's VALU -- is what pays:
// the backward took 1.98 ms at one workgroup per CU and 0.98 ms at two (B = 64, L = 512, p = 0.1).
//   fwd: LDS 33.4 KiB (K 16 + V^T 17 + key flags); S^T 64 + O^T 32 accumulators; 223 VGPRs, no spill
//   dq : LDS 57.1 KiB (K, V row-major 32 + K^T 17 + dropout bits 8); a tile's keys in two halves of 64, so S^T 32 +
//        dPd^T 32 + dQ^T 32 accumulators; 237 VGPRs, no spill. The lane's dropout decisions of sweep 1 are kept as
//        bits in LDS (each thread rereads its own words) and sweep 2 does not hash again.
//   dkv: LDS 67.5 KiB (Q, dO row-major 32 + Q^T, dO^T 34 + stats, D 1.5); a tile's queries in two halves of 64, so S 32
//        + dPd 32 + dV^T, dK^T 64 accumulators; 236 VGPRs (causal: 256 and 12 B of scratch), no spill otherwise
// The tiles are single-buffered (two barriers per tile); at L <= 512 a sweep is at most 4 tiles.
//
// CAUSAL instantiations (bert_attn_steps.h, the causal rule): the forward and dq visit key tiles up to their own query
// tile only, dkv query tiles from its own key tile on; inside the diagonal tile the 16 x 16 MFMA tiles, the 64-wide
// halves and the PV / dQ / dV / dK k-steps above the diagonal are skipped too, and only there does the key <= query
// compare decide anything. A query without a visible key exists iff the sequence's first key is masked: then nothing
// is skipped (causal_skip) and the forward finds the first valid key kfirst once per workgroup -- query q < kfirst has
// no visible key and is uniform over all L keys (score 0 for every key in range, saved as row max = -inf).
#include <type_traits>

#include "bert_attn_host.h"

using namespace vcg;
using namespace vcg::attn;

namespace {

// ------------------------------------------------------------------------------------------------ forward
// blockIdx.x = z * nT + query tile; wave w owns queries q0 + 32 w .. + 31
template <bool CAUSAL>
__global__ __launch_bounds__(256, 2) void bert_attn_long_fwd_kernel(const bf16_t* __restrict__ qkv,
                                                                 const long long* __restrict__ mask,
                                                                 bf16_t* __restrict__ ctx, float2* __restrict__ stats,
                                                                 const int* __restrict__ seq, int nh, int Lmax, int Lp,
                                                                 int nT, float scale, float p, uint64_t seed) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[LT * DH];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[DH * TP];
  __shared__ uint8_t kval[LT];
  const Head hd(nh, nT, seq, Lmax, Lp);
  const int L = hd.L, H = hd.H, q0 = hd.tile0, tid = hd.tid, w = hd.w, g = hd.g, i = hd.i;
  const long long ld = hd.ld;
  if (q0 >= L) return;  // (a packed sequence that ends before this query tile; block-uniform, before any barrier)
  const bf16_t* base = qkv + hd.qo;  // Q of (b, h); K at + H, V at + 2 H

  bool none;       // no valid key in the whole sequence: uniform attention
  int kfirst = 0;  // CAUSAL: the first valid key (L: none); queries before it have no visible key
  if constexpr (CAUSAL) {
    __shared__ int kfs;
    if (tid == 0) kfs = L;
    __syncthreads();
    if (mask) {
      int kf = L;
      for (int k = tid; k < L; k += 256)
        if (mask[(long long)hd.row0 + k] != 0) kf = min(kf, k);
      if (kf < L) atomicMin(&kfs, kf);
    } else if (tid == 0) {
      kfs = 0;
    }
    __syncthreads();
    kfirst = kfs;
    none = false;  // (decided per query below)
  } else {
    int anyk = mask == nullptr;  // (seq_has_key's rule, kept in this form: see there)
    if (mask)
      for (int k = tid; k < L; k += 256) anyk |= mask[(long long)hd.row0 + k] != 0;
    none = !__syncthreads_or(anyk);
  }
  const bool skip = CAUSAL && kfirst == 0;  // (= causal_skip: the first key is valid)

  s16x8 qf[2][2];
  load_frags(qf, base, ld, q0 + 32 * w, L, g, i);
  const bool wact = q0 + 32 * w < L;  // (else every query of this wave is past the end: it only loads and syncs)
  const float rs = p > 0.f ? 1.f / (1.f - p) : 1.f;
  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};
  f32x4 oacc[4][2];  // lane holds O^T[d 16 dt + 4 g + r][query q0 + 32 w + 16 qt + i], unnormalised
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) oacc[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int kend = skip ? min(L, q0 + LT) : L;  // (causal: the key tiles past the query tile are not visited)
  for (int k0 = 0; k0 < kend; k0 += LT) {
    const int Lt = L - k0;  // keys of this tile (>= 128: a full tile)
    load_rm(base + (long long)k0 * ld + H, ld, Lt, Ks, tid);
    load_transpose(base + (long long)k0 * ld + 2 * H, ld, Lt, Vt, nullptr, tid);
    load_key_flags(kval, none ? nullptr : mask, (long long)hd.row0 + k0, Lt, tid);
    __syncthreads();
    // one key tile; MK: the causal rule acts inside it -- the diagonal tile, or any tile of a sequence whose first key
    // is masked (!skip). A tile below the diagonal (MK false) is the non-causal tile body: every key before every query
    auto tile = [&](auto MASK) {
      constexpr bool MK = decltype(MASK)::value;
      const int qlo = MK && skip ? q0 + 32 * w - k0 : NOSKIP;  // the wave's first query in the tile's key coordinates
      f32x4 sacc[2][8];  // lane holds S^T[key k0 + 16 kt + 4 g + r][query q0 + 32 w + 16 qt + i]
      key_tiles<8, MK>(sacc, Ks, 0, Lt, qf, g, i, qlo);
      const uint32_t vb = key_bits<8>(kval, 0, g);
      s16x8 pf[2][4];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + 32 * w + 16 * qt + i;
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v;
            if constexpr (MK) {
              const int kl = 16 * kt + 4 * g + r;
              if (q < kfirst) v = kl < Lt ? 0.f : -INFINITY;  // no visible key: every key in range, score 0
              else v = visible<true>((vb >> (4 * kt + r)) & 1u, k0 + kl, q) ? sacc[qt][kt][r] * scale : -INFINITY;
            } else {
              v = ((vb >> (4 * kt + r)) & 1u) ? (none ? 0.f : sacc[qt][kt][r] * scale) : -INFINITY;
            }
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
        dropout_frags(pf[qt], sacc[qt], q < L, hd.drop_row(q) + k0, 1.f, rs, p, seed, g,
                      MK && skip ? qlo + 32 : NOSKIP);  // (1 / l: at the end)
      }
      pv_step(oacc, Vt, pf, MK && skip ? min(Lt, qlo + 32) : Lt, g, i);
    };
    if (wact) {
      if (CAUSAL && (!skip || k0 == q0)) tile(std::true_type{});
      else tile(std::false_type{});
    }
    __syncthreads();  // every wave is done with this tile before the next one overwrites it
  }
  if (!wact) return;
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = q0 + 32 * w + 16 * qt + i;
    if (q < L) {
      const float inv = 1.f / l[qt];
      if (g == 0) stats[hd.so + q] = make_float2((none || (CAUSAL && q < kfirst)) ? -INFINITY : m[qt], inv);
      store_row64(ctx + hd.co + (long long)q * H + 4 * g, oacc, qt, inv);
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward: D, dQ
// blockIdx.x = z * nT + query tile; wave w owns queries q0 + 32 w .. + 31. S^T = K Q^T and dPd^T = V dO^T (A = K / V
// rows from LDS, B = the wave's Q / dO rows from HBM), dQ^T = K^T dS^T (A = K^T from LDS, B = dS from registers).
template <bool CAUSAL>
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
  const Head hd(nh, nT, seq, Lmax, Lp);
  const int L = hd.L, H = hd.H, q0 = hd.tile0, tid = hd.tid, w = hd.w, g = hd.g, i = hd.i;
  const long long ld = hd.ld;
  if (q0 >= L) return;  // (block-uniform, before any barrier)
  const bf16_t* base = qkv + hd.qo;

  s16x8 qf[2][2], df[2][2];
  load_frags(qf, base, ld, q0 + 32 * w, L, g, i);
  load_frags(df, dctx + hd.co, H, q0 + 32 * w, L, g, i);
  float2 mi[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = q0 + 32 * w + 16 * qt + i;
    mi[qt] = q < L ? stats[hd.so + q] : make_float2(0.f, 0.f);
  }
  const bool wact = q0 + 32 * w < L;
  const float rs = p > 0.f ? 1.f / (1.f - p) : 1.f;
  float D[2] = {0.f, 0.f};
  f32x4 dq[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) dq[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const bool skip = CAUSAL && causal_skip(mask, hd.row0, L);
  const int kend = skip ? min(L, q0 + LT) : L;  // (causal: the key tiles past the query tile are not visited)
  for (int sweep = 0; sweep < 2; ++sweep) {  // 0: D; 1: dS and dQ
    for (int k0 = 0; k0 < kend; k0 += LT) {
      const int Lt = L - k0;
      const int qlo = skip ? q0 + 32 * w - k0 : NOSKIP;  // the wave's first query in the tile's key coordinates
      if (sweep == 0) load_rm(base + (long long)k0 * ld + H, ld, Lt, Ks, tid);
      else load_transpose(base + (long long)k0 * ld + H, ld, Lt, Kt, Ks, tid);
      load_rm(base + (long long)k0 * ld + 2 * H, ld, Lt, Vs, tid);
      load_key_flags(kval, mask, (long long)hd.row0 + k0, Lt, tid);
      __syncthreads();
      // one half (64 keys) of the tile; SW = the sweep, MASK = the causal rule acts inside the tile (the diagonal tile,
      // or any tile of a sequence whose first key is masked; otherwise the non-causal body), compile-time constants
      auto half = [&](auto SW, auto MASK, int kh) {
        constexpr int sw = decltype(SW)::value;
        constexpr bool MK = decltype(MASK)::value;
        f32x4 sacc[2][4], pacc[2][4];  // lane holds S^T / dPd^T [key k0 + kh + 16 kt + 4 g + r][query q0 + 32 w + 16 qt + i]
        key_tiles<4, MK>(sacc, Ks, kh, Lt, qf, g, i, qlo);
        key_tiles<4, MK>(pacc, Vs, kh, Lt, df, g, i, qlo);
        const uint32_t vb = key_bits<4>(kval, kh, g);
        // the lane's 32 dropout decisions of this half (bit 16 qt + 4 kt + r): hashed in sweep 0, reread in sweep 1
        uint32_t* kw = keepw + ((k0 + kh) >> 6) * 256 + tid;
        uint32_t kb = sw == 0 ? 0u : *kw;
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          const int q = q0 + 32 * w + 16 * qt + i;
          const uint64_t rowi = hd.drop_row(q) + k0;
          float part = 0.f;
#pragma unroll
          for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int kl = kh + 16 * kt + 4 * g + r;
              const float P = attn_prob(sacc[qt][kt][r], scale, mi[qt],
                                        visible<MK>((vb >> (4 * kt + r)) & 1u, k0 + kl, q), kl < Lt, q < L);
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
              else sacc[qt][kt][r] = causal_ds<MK>(scale * P * (dP - D[qt]), k0 + kl, q);  // dS
            }
          if constexpr (sw == 0) D[qt] += part;
        }
        if constexpr (sw == 0) *kw = kb;
        if constexpr (sw == 1) {
#pragma unroll
          for (int s = 0; s < 2; ++s)
            if (kh + 32 * s < Lt && (!MK || kh + 32 * s <= qlo + 31)) {
              s16x8 sf[2];
#pragma unroll
              for (int qt = 0; qt < 2; ++qt) sf[qt] = pack8(sacc[qt][2 * s], sacc[qt][2 * s + 1]);
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
        if (CAUSAL && kh > qlo + 31) break;  // (the half lies past the wave's last query)
        if (CAUSAL && (!skip || k0 == q0)) {
          if (sweep == 0) half(std::integral_constant<int, 0>{}, std::true_type{}, kh);
          else half(std::integral_constant<int, 1>{}, std::true_type{}, kh);
        } else {
          if (sweep == 0) half(std::integral_constant<int, 0>{}, std::false_type{}, kh);
          else half(std::integral_constant<int, 1>{}, std::false_type{}, kh);
        }
      }
      __syncthreads();
    }
    if (sweep == 0 && wact) {  // the lane groups' partial sums over their keys, in a fixed order
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + 32 * w + 16 * qt + i;
        D[qt] += __shfl_xor(D[qt], 16, 64);
        D[qt] += __shfl_xor(D[qt], 32, 64);
        if (g == 0 && q < L) Dv[hd.so + q] = D[qt];
      }
    }
  }
  if (!wact) return;
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = q0 + 32 * w + 16 * qt + i;
    if (q < L) store_row64(dqkv + hd.qo + (long long)q * ld + 4 * g, dq, qt);
  }
}

// ------------------------------------------------------------------------------------------------ backward: dK, dV
// blockIdx.x = z * nT + key tile; wave w owns keys k0 + 32 w .. + 31 (A = Q / dO rows, Q^T / dO^T from LDS, B = the
// wave's K / V rows from HBM and its Pd / dS fragments from registers). The body of a query tile is
// dkv_query_tile (bert_attn_steps.h), shared with the cross-attention dK | dV kernel; what is written out here is
// which query tiles are visited and which of them get the causal body.
template <bool CAUSAL>
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
  const Head hd(nh, nT, seq, Lmax, Lp);
  const int L = hd.L, H = hd.H, k0 = hd.tile0, tid = hd.tid, w = hd.w, g = hd.g, i = hd.i;
  const long long ld = hd.ld;
  if (k0 >= L) return;  // (block-uniform, before any barrier)
  const bf16_t* base = qkv + hd.qo;

  s16x8 kf[2][2], vf[2][2];
  load_frags(kf, base + H, ld, k0 + 32 * w, L, g, i);
  load_frags(vf, base + 2 * H, ld, k0 + 32 * w, L, g, i);
  bool kv[2];
  int keyi[2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = k0 + 32 * w + 16 * kt + i;
    keyi[kt] = key;
    kv[kt] = key < L && (mask == nullptr || mask[(long long)hd.row0 + key] != 0);
  }
  const bool wact = k0 + 32 * w < L;
  f32x4 dv[4][2], dk[4][2];  // lane holds dV^T / dK^T [d 16 dt + 4 g + r][key k0 + 32 w + 16 kt + i]
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) dv[dt][kt] = dk[dt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const DkvOperands op = {base, dctx + hd.co, ld, H, stats + hd.so, Dv + hd.so, L, L, hd.z, Lmax, Lp,
                          scale, p, seed};
  const DkvLds lds = {Qs, dOs, Qt, dOt, st, Ds};
  const bool skip = CAUSAL && causal_skip(mask, hd.row0, L);
  // (causal: the query tiles before the key tile are not visited; the masked body -- the causal rule acts inside the
  // tile -- runs on the diagonal tile only, or on every tile of a sequence whose first key is masked, where nothing
  // may be skipped; the other tiles take the non-causal body: every key of the workgroup lies before every query)
  int q0 = skip ? k0 : 0;
  if constexpr (CAUSAL) {
#pragma unroll 1
    for (const int qe = skip ? min(L, k0 + LT) : L; q0 < qe; q0 += LT)  // klo: the wave's first key, tile coordinates
      dkv_query_tile<true, false>(dv, dk, op, lds, q0, kf, vf, kv, keyi, wact, skip ? k0 + 32 * w - q0 : -NOSKIP, tid,
                                  g, i);
  }
#pragma unroll 1
  for (; q0 < L; q0 += LT)
    dkv_query_tile<false, false>(dv, dk, op, lds, q0, kf, vf, kv, keyi, wact, -NOSKIP, tid, g, i);
  if (!wact) return;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = keyi[kt];
    if (key < L) {
      bf16_t* o = dqkv + hd.qo + (long long)key * ld + 4 * g;
      store_row64(o + H, dk, kt);
      store_row64(o + 2 * H, dv, kt);
    }
  }
}

}  // namespace

namespace vcg {

int bert_attn_long_fwd(const void* qkv, const long long* mask, const int* seq, void* ctx, void* stats, int B, int nh,
                       int Lmax, int Lp, int nT, float scale, float dropout_p, unsigned long long seed, bool causal,
                       hipStream_t s) {
  hipLaunchKernelGGL(causal ? bert_attn_long_fwd_kernel<true> : bert_attn_long_fwd_kernel<false>, dim3(B * nh * nT),
                     dim3(256), 0, s, (const bf16_t*)qkv, mask, (bf16_t*)ctx, (float2*)stats, seq, nh, Lmax, Lp, nT,
                     scale, dropout_p, (uint64_t)seed);
  VCG_CHECK_HIP(hipGetLastError());
  return VCG_OK;
}

int bert_attn_long_bwd(const void* qkv, const void* dctx, const long long* mask, const int* seq, void* stats,
                       void* dqkv, int B, int nh, int Lmax, int Lp, int nT, float scale, float dropout_p,
                       unsigned long long seed, bool causal, hipStream_t s) {
  const float2* st = (const float2*)stats;
  float* Dv = (float*)(st + stats_rows(B, nh, Lmax));
  hipLaunchKernelGGL(causal ? bert_attn_long_dq_kernel<true> : bert_attn_long_dq_kernel<false>, dim3(B * nh * nT),
                     dim3(256), 0, s, (const bf16_t*)qkv, (const bf16_t*)dctx, mask, st, Dv, (bf16_t*)dqkv, seq, nh,
                     Lmax, Lp, nT, scale, dropout_p, (uint64_t)seed);
  VCG_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(causal ? bert_attn_long_dkv_kernel<true> : bert_attn_long_dkv_kernel<false>, dim3(B * nh * nT),
                     dim3(256), 0, s, (const bf16_t*)qkv, (const bf16_t*)dctx, mask, st, (const float*)Dv,
                     (bf16_t*)dqkv, seq, nh, Lmax, Lp, nT, scale, dropout_p, (uint64_t)seed);
  VCG_CHECK_HIP(hipGetLastError());
  return VCG_OK;
}

}  // namespace vcg
