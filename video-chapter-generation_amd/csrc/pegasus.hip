// Pegasus (encoder-decoder) kernels: what the engine's BERT / GPT kernels cannot express (reference
// model/lang/pegasus_hugface.py -> transformers PegasusForConditionalGeneration):
//   vcg_cross_attn_kv_fwd  decoder queries [B Lq] over one layer's encoder keys / values [B Lk], Lq != Lk, separate Q
//                          and K | V buffers, a key-padding mask; nothing Lq x Lk in HBM (_ex: dropout on P, training)
//   vcg_cross_attn_kv_bwd  its backward: dQ and dK | dV in two kernels from the saved row statistics
//   vcg_pegasus_embed_fwd  scale * tok[ids] + pos[pos0 + t] (the sinusoidal table is not learned and is not scaled;
//                          _ex: dropout; the backward, vcg_pegasus_embed_bwd, is in bert.hip beside its scatter kernel)
//   vcg_dropout_add_*, vcg_relu_dropout_*  the dropout sites of a pre-LayerNorm block, forward and backward
// Every reduction runs in a fixed order and there is no floating-point atomic: the results are bit-identical run to run.
#include "bert_attn_steps.h"

using namespace vcg;
using namespace vcg::attn;

namespace {

constexpr int QT = 16;  // queries of a workgroup: one MFMA tile

// The bf16 cross-attention kernels' coordinates (attn::Head's counterpart). Workgroup blockIdx.x = z * nT + tile of
// head z = b * nh + h, nT tiles per head (of 16 queries, or of 128 keys). Sequence b is rows b Lq .. of q / dctx / dq /
// ctx and rows b Lk .. of kv / dkv / the mask; the stats, D and the dropout counters are indexed [z][Lq]. (The fp32
// parity kernels, one wave per query or key row, keep their own few lines: they index single rows. The lane
// decomposition stays one line in each kernel.)
struct CrossHead {
  int z, h, H, Lq;       // H = nh * 64
  unsigned tile;         // (unsigned like blockIdx.x; the workgroup's first row is QT * tile or LT * tile)
  long long qrow, mrow;  // the first query row and the first key (mask) row of sequence b
  const bf16_t *Q, *K, *V;  // row 0 of (b, h) in q and in kv (V at K + H)

  __device__ __forceinline__ CrossHead(const bf16_t* q, long long ldq, const bf16_t* kv, long long ldkv, int nh, int Lq_,
                                       int Lk, int nT) : Lq(Lq_) {
    z = blockIdx.x / nT;
    tile = blockIdx.x - z * nT;
    const int b = z / nh;
    h = z - b * nh;
    H = nh * DH;
    qrow = (long long)b * Lq;
    mrow = (long long)b * Lk;
    Q = qrows(q, ldq);
    K = krows(kv, ldkv);
    V = K + H;
  }
  // the stats / D row of (z, query 0). Like the two below it is formed where it is used, not in the constructor: the
  // kernels then compile to what they were with these lines written out
  __device__ __forceinline__ long long srow() const { return (long long)z * Lq; }
  // (b, h)'s row r0 + r1 of a query-indexed buffer (q, dctx, dq, ctx) / row r of a key-indexed one (kv, dkv), pitch ld
  template <typename U>
  __device__ __forceinline__ U* qrows(U* p, long long ld, int r0 = 0, int r1 = 0) const {
    return p + (qrow + r0 + r1) * ld + h * DH;
  }
  template <typename U>
  __device__ __forceinline__ U* krows(U* p, long long ld, int r = 0) const { return p + (mrow + r) * ld + h * DH; }
};

// One workgroup (4 waves) per (sequence b, head h, 16-query tile). The keys go by in tiles of LT = 128: the workgroup
// transposes the tile's V into LDS (load_transpose: the A operand of O^T += V^T P^T), wave w owns the tile's keys
// 32 w .. 32 w + 31 and reads their K fragments straight from HBM (load_frags: every K byte is used once per
// workgroup). Per strip: S^T = K Q^T (4 MFMAs; a lane holds [key 32 w + 16 kt + 4 g + r][query i]), the online softmax
// (m, l, O) of the wave's keys, O^T += V^T P^T (4 MFMAs, P from registers: pack8). The four partials are combined
// through LDS in the order 0..3.
// Masking is attn_prob's rule: a masked key has P = 0; in a sequence without any valid key every key in range has the
// same weight (has_key false: the reference maximum is fixed at 0 and every in-range P is 1).
// DROP (training): P is dropped at counter drop_row(z, Lq, q, Lk) + key AFTER the row sum took it -- the statistics
// are those of the undropped row, as in the self-attention kernels; the DROP = false instantiation is the inference
// kernel, unchanged.
template <bool DROP>
__global__ __launch_bounds__(256) void cross_attn_kv_fwd_kernel(const bf16_t* __restrict__ q, long long ldq,
                                                                const bf16_t* __restrict__ kv, long long ldkv,
                                                                const long long* __restrict__ mask,
                                                                bf16_t* __restrict__ ctx, float2* __restrict__ stats,
                                                                int nh, int Lq, int Lk, int nQ, float scale, float pdrop,
                                                                uint64_t seed) {
  __shared__ __attribute__((aligned(16))) bf16_t Vt[DH * TP];
  __shared__ uint8_t kval[LT];
  __shared__ float sm[4][QT], sl[4][QT];
  __shared__ __attribute__((aligned(16))) float so[4][QT][DH];

  const CrossHead hd(q, ldq, kv, ldkv, nh, Lq, Lk, nQ);
  const int z = hd.z, q0 = QT * hd.tile, H = hd.H, tid = threadIdx.x, w = tid >> 6, g = (tid & 63) >> 4, i = tid & 15;
  const bf16_t *Qs = hd.Q, *Ks = hd.K, *Vs = hd.V;
  const long long mrow = hd.mrow;
  const bool has_key = seq_has_key(mask, mrow, Lk);
  const bool qrow = q0 + i < Lq;

  s16x8 qf[2][2];  // ([1]: the tile behind this one, unused)
  load_frags(qf, Qs, ldq, q0, Lq, g, i);

  float m = has_key ? -INFINITY : 0.f, l = 0.f;
  f32x4 oacc[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oacc[dt][0] = oacc[dt][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < Lk; k0 += LT) {
    const int kw = k0 + 32 * w;  // the wave's first key
    s16x8 kf[2][2];
    load_frags(kf, Ks, ldkv, kw, Lk, g, i);
    __syncthreads();  // (the previous tile's V fragments and flags have been read)
    load_transpose(Vs + (long long)k0 * ldkv, ldkv, Lk - k0, Vt, nullptr, tid);
    load_key_flags(kval, mask, mrow + k0, Lk - k0, tid);
    __syncthreads();
    if (kw >= Lk) continue;  // (wave-uniform; the barriers above are reached by every wave of every tile)
    f32x4 s[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kt][ks], qf[0][ks], s[kt], 0, 0, 0);
    }
    const uint32_t vb = key_bits<2>(kval, 32 * w, g);
    float mn = m;
    if (has_key) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (vb & (1u << (4 * kt + r))) mn = fmaxf(mn, s[kt][r] * scale);
      mn = fmaxf(mn, __shfl_xor(mn, 16, 64));
      mn = fmaxf(mn, __shfl_xor(mn, 32, 64));
    }
    // (no valid key so far: every P below is 0 whatever the reference, and l and O are still 0)
    const float corr = m == -INFINITY ? 0.f : __expf(m - mn);
    const float2 mi = make_float2(has_key ? (mn == -INFINITY ? 0.f : mn) : -INFINITY, 1.f);
    f32x4 p[2];
    float ps = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kw + 16 * kt + 4 * g + r;
        p[kt][r] = attn_prob(s[kt][r], scale, mi, (vb >> (4 * kt + r)) & 1u, key < Lk, qrow);
        ps += p[kt][r];
      }
    l = fmaf(l, corr, ps);
    m = mn;
    if constexpr (DROP) {
      const uint64_t rowi = drop_row(z, Lq, q0 + i, Lk);
      const float rs = 1.f / (1.f - pdrop);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          p[kt][r] = dropout_keep(seed, rowi + (kw + 16 * kt + 4 * g + r), pdrop) ? p[kt][r] * rs : 0.f;
    }
    const s16x8 pf = pack8(p[0], p[1]);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      oacc[dt][0] *= corr;
      oacc[dt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_split(Vt, 16 * dt + i, 32 * w + 4 * g), pf, oacc[dt][0],
                                                            0, 0, 0);
    }
  }
  // the lane groups' row sums (they share m), then the wave's partial: O^T[d = 16 dt + 4 g + r][query i]
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (g == 0) { sm[w][i] = m; sl[w][i] = l; }
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    *reinterpret_cast<f32x4*>(&so[w][i][16 * dt + 4 * g]) = oacc[dt][0];
  __syncthreads();
  // thread (query qi, 4 dims from d0) adds the four partials in the order 0..3
  const int qi = tid & 15, d0 = 4 * (tid >> 4);
  if (q0 + qi >= Lq) return;
  float mt = sm[0][qi];
#pragma unroll
  for (int ww = 1; ww < 4; ++ww) mt = fmaxf(mt, sm[ww][qi]);
  float lt = 0.f;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ww = 0; ww < 4; ++ww) {
    const float f = sm[ww][qi] == -INFINITY ? 0.f : __expf(sm[ww][qi] - mt);
    lt = fmaf(sl[ww][qi], f, lt);
    o += *reinterpret_cast<const f32x4*>(&so[ww][qi][d0]) * f;
  }
  const float inv = 1.f / lt;
  *reinterpret_cast<uint2*>(hd.qrows(ctx, H, q0, qi) + d0) =
      make_uint2(pack2(o[0] * inv, o[1] * inv), pack2(o[2] * inv, o[3] * inv));
  if (stats && d0 == 0) stats[hd.srow() + q0 + qi] = make_float2(has_key ? mt : -INFINITY, lt);
}

// The fp32 parity mode: one wave per (sequence, head, query). Lane j owns keys j, j + 64, ... with an online softmax
// over them (library expf); the 64 partials are added through LDS in lane order.
template <bool DROP>
__global__ __launch_bounds__(64) void cross_attn_kv_fwd_f32_kernel(const float* __restrict__ q, long long ldq,
                                                                   const float* __restrict__ kv, long long ldkv,
                                                                   const long long* __restrict__ mask,
                                                                   float* __restrict__ ctx, float2* __restrict__ stats,
                                                                   int nh, int Lq, int Lk, float scale, float pdrop,
                                                                   uint64_t seed) {
  __shared__ float sm[64], sl[64], so[64][DH + 1];
  __shared__ float sq[DH];
  const int z = blockIdx.x / Lq, qi = blockIdx.x - z * Lq;
  const int b = z / nh, h = z - b * nh;
  const int H = nh * DH;
  const int lane = threadIdx.x;
  const long long mrow = (long long)b * Lk;
  const bool has_key = seq_has_key(mask, mrow, Lk);
  sq[lane] = q[((long long)b * Lq + qi) * ldq + h * DH + lane];
  __syncthreads();
  float m = has_key ? -INFINITY : 0.f, l = 0.f, acc[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) acc[d] = 0.f;
  for (int k = lane; k < Lk; k += 64) {
    const bool valid = mask == nullptr || mask[mrow + k] != 0;
    if (has_key && !valid) continue;
    const float* kr = kv + (mrow + k) * ldkv + h * DH;
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < DH; ++d) s = fmaf(sq[d], kr[d], s);
    s *= scale;
    const float mn = has_key ? fmaxf(m, s) : 0.f;
    const float corr = expf(m - mn);  // (m = -inf: 0)
    const float p = has_key ? expf(s - mn) : 1.f;
    l = fmaf(l, corr, p);
    const float* vr = kr + H;
    float pd = p;  // (DROP: the row sum above keeps the undropped p)
    if constexpr (DROP) pd = dropout_keep(seed, drop_row(z, Lq, qi, Lk) + k, pdrop) ? p / (1.f - pdrop) : 0.f;
#pragma unroll
    for (int d = 0; d < DH; ++d) acc[d] = fmaf(acc[d], corr, pd * vr[d]);
    m = mn;
  }
  sm[lane] = m;
  sl[lane] = l;
#pragma unroll
  for (int d = 0; d < DH; ++d) so[lane][d] = acc[d];
  __syncthreads();
  float mt = sm[0];
  for (int j = 1; j < 64; ++j) mt = fmaxf(mt, sm[j]);
  float lt = 0.f, o = 0.f;
  for (int j = 0; j < 64; ++j) {
    const float f = sm[j] == -INFINITY ? 0.f : expf(sm[j] - mt);
    lt = fmaf(sl[j], f, lt);
    o = fmaf(so[j][lane], f, o);
  }
  ctx[((long long)b * Lq + qi) * H + h * DH + lane] = o / lt;
  if (stats && lane == 0) stats[(long long)z * Lq + qi] = make_float2(has_key ? mt : -INFINITY, lt);
}

// out[b, t] = scale * tok[ids[b, t]] + pos[pos0 + t]: the product and the sum in double (exact up to its own
// rounding), one rounding to fp32, and from there to the storage dtype. DROP (training): dropout of that fp32 value,
// counter row * H + c (the element index of out), 1 / (1 - p) in fp32
template <typename T, bool DROP>
__global__ void pegasus_embed_fwd_kernel(const long long* __restrict__ ids, const float* __restrict__ tok,
                                         const float* __restrict__ pos, T* __restrict__ out, int L, int H, int V,
                                         float scale, int pos0, float pdrop, uint64_t seed) {
  const long long row = blockIdx.x;
  const int t = (int)(row % L);
  long long id = ids[row];
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);  // (ids are validated where they are made; never read outside the table)
  const float* tr = tok + id * H;
  const float* pr = pos + (long long)(pos0 + t) * H;
  for (int c = threadIdx.x; c < H; c += blockDim.x) {
    float v = (float)((double)scale * (double)tr[c] + (double)pr[c]);
    if constexpr (DROP) v = dropout_keep(seed, (uint64_t)(row * H + c), pdrop) ? v / (1.f - pdrop) : 0.f;
    out[row * H + c] = from_f<T>(v);
  }
}

// ------------------------------------------------------------------------------------------------ training
// Cross-attention backward, bf16: two kernels, no atomics, nothing Lq x Lk in HBM. With Pd = dropout(P) the forward is
// O = Pd V, so dPd = dO V^T, dP = keep * dPd / (1 - p), dS = scale * P o (dP - D) with D[q] = sum_k P dP. D is taken
// from the fp32 products, as in bert_attn.hip (its header), not as sum_d dO[q][d] O[q][d] of the bf16-rounded context:
// the same dP then enters both terms of dP - D and every dS row sums to zero as the exact softmax gradient does. With
// few keys the two forms differ visibly (one key: dP = D exactly, dS = 0, while the rounding of O = Pd V would leak
// into dQ and dK). P comes back from the saved (row max, row sum) through attn_prob: a masked key has P = 0 and so
// dS = 0; a sequence without any valid key is saved as max = -inf and is uniform, P = 1 / Lk at every key in range.
// Rows past Lq and keys past Lk load as zeros (ld16's guard: nothing of a pad row is read) and carry P = 0.
//
// dQ: one workgroup per (sequence b, head h, 16-query tile), the forward's decomposition, two sweeps over the keys in
// tiles of 128. Wave w owns keys 32 w .. 32 w + 31 of a tile and reads their K and V fragments straight from HBM;
// S^T = K Q^T and dPd^T = V dO^T (4 MFMAs each; a lane holds [key][query i]). Sweep 0 sums P dP over the wave's keys;
// the four waves' partials meet in LDS in the order 0..3 and D is stored for the second kernel. Sweep 1 forms dS^T in
// registers and dQ^T += K^T dS^T (A = K^T from LDS: load_transpose; B = dS: pack8); the four partial dQ^T meet in LDS
// in the order 0..3.
__global__ __launch_bounds__(256) void cross_attn_kv_dq_kernel(const bf16_t* __restrict__ q, long long ldq,
                                                               const bf16_t* __restrict__ kv, long long ldkv,
                                                               const long long* __restrict__ mask,
                                                               const bf16_t* __restrict__ dctx, long long lddo,
                                                               const float2* __restrict__ stats, float* __restrict__ Dv,
                                                               bf16_t* __restrict__ dq, long long lddq, int nh, int Lq,
                                                               int Lk, int nQ, float scale, float pdrop, uint64_t seed) {
  __shared__ __attribute__((aligned(16))) bf16_t Kt[DH * TP];
  __shared__ uint8_t kval[LT];
  __shared__ float sD[4][QT];
  __shared__ __attribute__((aligned(16))) float so[4][QT][DH];

  const CrossHead hd(q, ldq, kv, ldkv, nh, Lq, Lk, nQ);
  const int z = hd.z, q0 = QT * hd.tile, tid = threadIdx.x, w = tid >> 6, g = (tid & 63) >> 4, i = tid & 15;
  const bf16_t *Qs = hd.Q, *dOs = hd.qrows(dctx, lddo), *Ks = hd.K, *Vs = hd.V;
  const long long mrow = hd.mrow;
  const bool qrow = q0 + i < Lq;

  float2 mi = make_float2(0.f, 0.f);  // (row max, 1 / row sum): attn_prob's form
  if (qrow) {
    mi = stats[hd.srow() + q0 + i];
    mi.y = 1.f / mi.y;
  }
  const float rs = pdrop > 0.f ? 1.f / (1.f - pdrop) : 1.f;
  const uint64_t rowi = drop_row(z, Lq, q0 + i, Lk);

  s16x8 qf[2][2], df[2][2];  // ([1]: the tile behind this one, unused)
  load_frags(qf, Qs, ldq, q0, Lq, g, i);
  load_frags(df, dOs, lddo, q0, Lq, g, i);
  float D = 0.f;
  f32x4 dqacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dqacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int sweep = 0; sweep < 2; ++sweep) {  // 0: D; 1: dS and dQ
#pragma unroll 1
    for (int k0 = 0; k0 < Lk; k0 += LT) {
      const int kw = k0 + 32 * w;  // the wave's first key
      s16x8 kf[2][2], vf[2][2];
      load_frags(kf, Ks, ldkv, kw, Lk, g, i);
      load_frags(vf, Vs, ldkv, kw, Lk, g, i);
      __syncthreads();  // (the previous tile's K^T fragments and flags have been read)
      if (sweep == 1) load_transpose(Ks + (long long)k0 * ldkv, ldkv, Lk - k0, Kt, nullptr, tid);
      load_key_flags(kval, mask, mrow + k0, Lk - k0, tid);
      __syncthreads();
      if (kw >= Lk) continue;  // (wave-uniform; the barriers above are reached by every wave of every tile)
      f32x4 s[2], dp[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        s[kt] = dp[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kt][ks], qf[0][ks], s[kt], 0, 0, 0);
          dp[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[kt][ks], df[0][ks], dp[kt], 0, 0, 0);
        }
      }
      const uint32_t vb = key_bits<2>(kval, 32 * w, g);
      float part = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kw + 16 * kt + 4 * g + r;
          const float P = attn_prob(s[kt][r], scale, mi, (vb >> (4 * kt + r)) & 1u, key < Lk, qrow);
          const bool keep = qrow && key < Lk && dropout_keep(seed, rowi + key, pdrop);
          const float dP = keep ? dp[kt][r] * rs : 0.f;
          part = fmaf(P, dP, part);
          s[kt][r] = scale * P * (dP - D);  // dS (sweep 1)
        }
      if (sweep == 0) {
        D += part;
        continue;
      }
      const s16x8 sf = pack8(s[0], s[1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        dqacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_split(Kt, 16 * dt + i, 32 * w + 4 * g), sf, dqacc[dt], 0,
                                                            0, 0);
    }
    if (sweep == 0) {  // the lane groups' partial sums over their keys, then the four waves', in a fixed order
      D += __shfl_xor(D, 16, 64);
      D += __shfl_xor(D, 32, 64);
      if (g == 0) sD[w][i] = D;
      __syncthreads();
      D = ((sD[0][i] + sD[1][i]) + sD[2][i]) + sD[3][i];
      if (w == 0 && g == 0 && qrow) Dv[hd.srow() + q0 + i] = D;
    }
  }
  // the wave's partial dQ^T[d = 16 dt + 4 g + r][query i]; thread (query qi, 4 dims from d0) adds the four in order
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4*>(&so[w][i][16 * dt + 4 * g]) = dqacc[dt];
  __syncthreads();
  const int qi = tid & 15, d0 = 4 * (tid >> 4);
  if (q0 + qi >= Lq) return;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ww = 0; ww < 4; ++ww) o += *reinterpret_cast<const f32x4*>(&so[ww][qi][d0]);
  *reinterpret_cast<uint2*>(hd.qrows(dq, lddq, q0, qi) + d0) =
      make_uint2(pack2(o[0], o[1]), pack2(o[2], o[3]));
}

// dK | dV: one workgroup per (sequence b, head h, 128-key tile); wave w owns keys k0 + 32 w .. + 31 and keeps their K
// and V fragments and the dV^T / dK^T accumulators in registers. It sweeps ALL query tiles with the self-attention dkv
// kernel's tile body, dkv_query_tile (bert_attn_steps.h: the non-causal instantiation, statistics saved as (max,
// sum)), with the first kernel's D. Every key's dK and dV row is written exactly once.
__global__ __launch_bounds__(256, 2) void cross_attn_kv_dkv_kernel(const bf16_t* __restrict__ q, long long ldq,
                                                                   const bf16_t* __restrict__ kv, long long ldkv,
                                                                   const long long* __restrict__ mask,
                                                                   const bf16_t* __restrict__ dctx, long long lddo,
                                                                   const float2* __restrict__ stats,
                                                                   const float* __restrict__ Dv, bf16_t* __restrict__ dkv,
                                                                   long long lddkv, int nh, int Lq, int Lk, int nK,
                                                                   float scale, float pdrop, uint64_t seed) {
  __shared__ __attribute__((aligned(16))) bf16_t Qr[LT * DH];
  __shared__ __attribute__((aligned(16))) bf16_t dOr[LT * DH];
  __shared__ __attribute__((aligned(16))) bf16_t Qt[DH * TP];
  __shared__ __attribute__((aligned(16))) bf16_t dOt[DH * TP];
  __shared__ float2 st[LT];
  __shared__ float Ds[LT];
  const CrossHead hd(q, ldq, kv, ldkv, nh, Lq, Lk, nK);
  const int k0 = LT * hd.tile, H = hd.H, tid = threadIdx.x, w = tid >> 6, g = (tid & 63) >> 4, i = tid & 15;

  s16x8 kf[2][2], vf[2][2];
  load_frags(kf, hd.K, ldkv, k0 + 32 * w, Lk, g, i);
  load_frags(vf, hd.V, ldkv, k0 + 32 * w, Lk, g, i);
  bool kvalid[2];
  int keyi[2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = k0 + 32 * w + 16 * kt + i;
    keyi[kt] = key;
    kvalid[kt] = key < Lk && (mask == nullptr || mask[hd.mrow + key] != 0);
  }
  const bool wact = k0 + 32 * w < Lk;  // (else the wave only loads and syncs)
  f32x4 dv[4][2], dk[4][2];  // lane holds dV^T / dK^T [d 16 dt + 4 g + r][key k0 + 32 w + 16 kt + i]
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) dv[dt][kt] = dk[dt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const DkvOperands op = {hd.Q, hd.qrows(dctx, lddo), ldq, lddo, stats + hd.srow(), Dv + hd.srow(), Lq, Lk, hd.z, Lq, Lk,
                          scale, pdrop, seed};
  const DkvLds lds = {Qr, dOr, Qt, dOt, st, Ds};
#pragma unroll 1
  for (int q0 = 0; q0 < Lq; q0 += LT)
    dkv_query_tile<false, true>(dv, dk, op, lds, q0, kf, vf, kvalid, keyi, wact, -NOSKIP, tid, g, i);
  if (!wact) return;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = keyi[kt];
    if (key < Lk) {
      bf16_t* o = hd.krows(dkv, lddkv, key) + 4 * g;
      store_row64(o, dk, kt);
      store_row64(o + H, dv, kt);
    }
  }
}

// The fp32 parity mode, dQ: one wave per (sequence, head, query); lane j owns keys j, j + 64, ... in two passes -- the
// first sums P dP (D, added over the lanes through LDS in lane order and stored for the second kernel), the second
// forms dS and the lane's partial dQ row; the 64 partial rows are added through LDS in lane order. (Library expf, the
// fp32 forward's arithmetic; the masking and no-key rule is attn_prob's: max = -inf -> uniform 1 / Lk, else a masked
// key 0.)
__global__ __launch_bounds__(64) void cross_attn_kv_dq_f32_kernel(const float* __restrict__ q, long long ldq,
                                                                  const float* __restrict__ kv, long long ldkv,
                                                                  const long long* __restrict__ mask,
                                                                  const float* __restrict__ dctx, long long lddo,
                                                                  const float2* __restrict__ stats,
                                                                  float* __restrict__ Dv, float* __restrict__ dq,
                                                                  long long lddq, int nh, int Lq, int Lk, float scale,
                                                                  float pdrop, uint64_t seed) {
  __shared__ float sq[DH], sdo[DH], red[64], so[64][DH + 1];
  const int z = blockIdx.x / Lq, qi = blockIdx.x - z * Lq;
  const int b = z / nh, h = z - b * nh;
  const int H = nh * DH;
  const int lane = threadIdx.x;
  const long long mrow = (long long)b * Lk, row = (long long)b * Lq + qi;
  sq[lane] = q[row * ldq + h * DH + lane];
  sdo[lane] = dctx[row * lddo + h * DH + lane];
  __syncthreads();
  const float2 st = stats[(long long)z * Lq + qi];
  const bool nokey = st.x == -INFINITY;
  const float inv = 1.f / st.y;
  const float rs = pdrop > 0.f ? 1.f / (1.f - pdrop) : 1.f;
  const uint64_t rowi = drop_row(z, Lq, qi, Lk);
  float D = 0.f, acc[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) acc[d] = 0.f;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    float part = 0.f;
    for (int k = lane; k < Lk; k += 64) {
      const bool valid = mask == nullptr || mask[mrow + k] != 0;
      if (!nokey && !valid) continue;  // P = 0: dS = 0
      const float* kr = kv + (mrow + k) * ldkv + h * DH;
      const float* vr = kr + H;
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) {
        s = fmaf(sq[d], kr[d], s);
        dp = fmaf(sdo[d], vr[d], dp);
      }
      const float P = nokey ? inv : expf(s * scale - st.x) * inv;
      const float dP = dropout_keep(seed, rowi + k, pdrop) ? dp * rs : 0.f;
      if (pass == 0) {
        part = fmaf(P, dP, part);
        continue;
      }
      const float dS = scale * P * (dP - D);
#pragma unroll
      for (int d = 0; d < DH; ++d) acc[d] = fmaf(dS, kr[d], acc[d]);
    }
    if (pass == 0) {
      red[lane] = part;
      __syncthreads();
      for (int j = 0; j < 64; ++j) D += red[j];
      if (lane == 0) Dv[(long long)z * Lq + qi] = D;
    }
  }
#pragma unroll
  for (int d = 0; d < DH; ++d) so[lane][d] = acc[d];
  __syncthreads();
  float o = 0.f;
  for (int j = 0; j < 64; ++j) o += so[j][lane];
  dq[row * lddq + h * DH + lane] = o;
}

// fp32 dK | dV: one wave per (sequence, head, key); lane j owns queries j, j + 64, ..., the 64 partial rows of each are
// added through LDS in lane order. A masked key of a sequence that has valid keys gets zeros.
__global__ __launch_bounds__(64) void cross_attn_kv_dkv_f32_kernel(const float* __restrict__ q, long long ldq,
                                                                   const float* __restrict__ kv, long long ldkv,
                                                                   const long long* __restrict__ mask,
                                                                   const float* __restrict__ dctx, long long lddo,
                                                                   const float2* __restrict__ stats,
                                                                   const float* __restrict__ Dv, float* __restrict__ dkv,
                                                                   long long lddkv, int nh, int Lq, int Lk, float scale,
                                                                   float pdrop, uint64_t seed) {
  __shared__ float sk[DH], sv[DH], so[64][DH + 1];
  const int z = blockIdx.x / Lk, k = blockIdx.x - z * Lk;
  const int b = z / nh, h = z - b * nh;
  const int H = nh * DH;
  const int lane = threadIdx.x;
  const long long mrow = (long long)b * Lk, srow = (long long)z * Lq;
  const float* kr = kv + (mrow + k) * ldkv + h * DH;
  sk[lane] = kr[lane];
  sv[lane] = kr[H + lane];
  __syncthreads();
  const bool valid = mask == nullptr || mask[mrow + k] != 0;
  const float rs = pdrop > 0.f ? 1.f / (1.f - pdrop) : 1.f;
  float dka[DH], dva[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) dka[d] = dva[d] = 0.f;
  for (int qq = lane; qq < Lq; qq += 64) {
    const float2 st = stats[srow + qq];
    const bool nokey = st.x == -INFINITY;
    if (!nokey && !valid) continue;  // P = 0
    const float* qr = q + ((long long)b * Lq + qq) * ldq + h * DH;
    const float* dor = dctx + ((long long)b * Lq + qq) * lddo + h * DH;
    float s = 0.f, dp = 0.f;
#pragma unroll
    for (int d = 0; d < DH; ++d) {
      s = fmaf(qr[d], sk[d], s);
      dp = fmaf(dor[d], sv[d], dp);
    }
    const float inv = 1.f / st.y;
    const float P = nokey ? inv : expf(s * scale - st.x) * inv;
    const bool keep = dropout_keep(seed, drop_row(z, Lq, qq, Lk) + k, pdrop);
    const float Pd = keep ? P * rs : 0.f;
    const float dS = scale * P * ((keep ? dp * rs : 0.f) - Dv[srow + qq]);
#pragma unroll
    for (int d = 0; d < DH; ++d) {
      dva[d] = fmaf(Pd, dor[d], dva[d]);
      dka[d] = fmaf(dS, qr[d], dka[d]);
    }
  }
  float* out = dkv + (mrow + k) * lddkv + h * DH;
#pragma unroll
  for (int d = 0; d < DH; ++d) so[lane][d] = dka[d];
  __syncthreads();
  float o = 0.f;
  for (int j = 0; j < 64; ++j) o += so[j][lane];
  out[lane] = o;
  __syncthreads();
#pragma unroll
  for (int d = 0; d < DH; ++d) so[lane][d] = dva[d];
  __syncthreads();
  o = 0.f;
  for (int j = 0; j < 64; ++j) o += so[j][lane];
  out[H + lane] = o;
}

// The pre-LayerNorm blocks' dropout sites as streaming kernels over n = rows * H elements, counter = the element index
// row * H + c. h is the fp32 residual stream, T the compute dtype. A thread owns 8 consecutive elements: 16-byte
// accesses (one per bf16 operand, two per fp32 operand) where `vec` says every pointer is 16-B aligned, element by
// element otherwise and in the last, partial group.
//   dropout_add fwd: h += dropout(branch)            bwd: dbranch = dropout'(dh)   (dh itself passes through)
//   relu_dropout fwd: f = dropout(relu(pre))         bwd: dpre = dy * (f > 0 ? 1 / (1 - p) : 0)
__device__ __forceinline__ void ld8(const float* p, float (&v)[8], bool fast, int cnt) {
  if (fast) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = e < cnt ? p[e] : 0.f;
}
__device__ __forceinline__ void ld8(const bf16_t* p, float (&v)[8], bool fast, int cnt) {
  if (fast) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[2 * e] = bf2f((bf16_t)(w[e] & 0xffffu));
      v[2 * e + 1] = bf2f((bf16_t)(w[e] >> 16));
    }
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = e < cnt ? bf2f(p[e]) : 0.f;
}
__device__ __forceinline__ void st8(float* p, const float (&v)[8], bool fast, int cnt) {
  if (fast) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (e < cnt) p[e] = v[e];
}
__device__ __forceinline__ void st8(bf16_t* p, const float (&v)[8], bool fast, int cnt) {
  if (fast) {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (e < cnt) p[e] = f2bf(v[e]);
}
// the thread's group: first element `base` (>= n: nothing to do), `cnt` elements, `fast`: a whole aligned group
#define VCG_EW_GROUP()                                                              \
  const long long base = 8 * ((long long)blockIdx.x * blockDim.x + threadIdx.x);    \
  if (base >= n) return;                                                            \
  const int cnt = n - base < 8 ? (int)(n - base) : 8;                               \
  const bool fast = vec && cnt == 8

template <typename T>
__global__ void dropout_add_fwd_kernel(float* __restrict__ h, const T* __restrict__ branch, long long n, float pdrop,
                                       uint64_t seed, bool vec) {
  VCG_EW_GROUP();
  float a[8], v[8];
  ld8(h + base, a, fast, cnt);
  ld8(branch + base, v, fast, cnt);
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] += dropout_keep(seed, (uint64_t)(base + e), pdrop) ? v[e] / (1.f - pdrop) : 0.f;
  st8(h + base, a, fast, cnt);
}

template <typename T>
__global__ void dropout_add_bwd_kernel(const float* __restrict__ dh, T* __restrict__ dbranch, long long n, float pdrop,
                                       uint64_t seed, bool vec) {
  VCG_EW_GROUP();
  float v[8];
  ld8(dh + base, v, fast, cnt);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = dropout_keep(seed, (uint64_t)(base + e), pdrop) ? v[e] / (1.f - pdrop) : 0.f;
  st8(dbranch + base, v, fast, cnt);
}

template <typename T>
__global__ void relu_dropout_fwd_kernel(const T* pre, T* f, long long n, float pdrop, uint64_t seed,
                                        bool vec) {  // (f may be pre: a thread reads its group before it writes it)
  VCG_EW_GROUP();
  float v[8];
  ld8(pre + base, v, fast, cnt);
#pragma unroll
  for (int e = 0; e < 8; ++e)
    v[e] = (v[e] > 0.f && dropout_keep(seed, (uint64_t)(base + e), pdrop)) ? v[e] / (1.f - pdrop) : 0.f;
  st8(f + base, v, fast, cnt);
}

template <typename T>
__global__ void relu_dropout_bwd_kernel(const T* dy, const T* f, T* dpre, long long n, float pdrop,
                                        bool vec) {  // (dpre may be dy)
  VCG_EW_GROUP();
  float d[8], a[8];
  ld8(dy + base, d, fast, cnt);
  ld8(f + base, a, fast, cnt);
#pragma unroll
  for (int e = 0; e < 8; ++e) d[e] = a[e] > 0.f ? d[e] / (1.f - pdrop) : 0.f;
  st8(dpre + base, d, fast, cnt);
}
#undef VCG_EW_GROUP

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// The checks the cross-attention entries share (bert_attn.hip's attn_check): head dim, the null test the caller made,
// dtype, shape, dropout_p, every buffer's row pitch against its least (H for a query-indexed one, 2 H for K | V) and,
// in bf16, the 16-B alignment of every buffer and pitch, in the entries' order: the grid test the caller made
// (grid_ok) comes before the alignment. fn: the entry's name; pitch_msg: its text for a short pitch; ctx_aligned: an
// output without a pitch argument.
struct CrossBuf {
  const void* p;
  long long ld;
  int nH;  // the pitch is at least nH * H
};
int cross_check(const char* fn, bool nonnull, int dtype, int B, int nh, int dh, int Lq, int Lk, float dropout_p,
                std::initializer_list<CrossBuf> bufs, const char* pitch_msg, bool grid_ok, bool ctx_aligned = true) {
  const char* msg = nullptr;
  bool pitch = true, align = ctx_aligned;
  for (const CrossBuf& b : bufs) {
    pitch = pitch && b.ld >= (long long)b.nH * nh * DH;
    align = align && b.ld % 8 == 0 && aligned16(b.p);
  }
  if (dh != DH) msg = "head dim must be 64";
  else if (!nonnull) msg = "null argument";
  else if (dtype != VCG_F32 && dtype != VCG_BF16) msg = "dtype must be VCG_F32 or VCG_BF16";
  else if (!(B > 0 && nh > 0 && Lq >= 1 && Lk >= 1)) msg = "bad shape";
  else if (!(dropout_p >= 0.f && dropout_p < 1.f)) msg = "dropout_p must be in [0, 1)";
  else if (!pitch) msg = pitch_msg;
  else if (!grid_ok) msg = "grid too large";
  else if (dtype == VCG_BF16 && !align) msg = "16-B alignment";
  if (msg == nullptr) return VCG_OK;
  set_error(std::string(fn) + ": " + msg);
  return VCG_ERR_INVALID;
}

}  // namespace

VCG_API int vcg_cross_attn_kv_fwd_ex(int dtype, const void* q, long long ldq, const void* kv, long long ldkv,
                                     const long long* key_mask, void* ctx, float* stats, int B, int nh, int dh, int Lq,
                                     int Lk, float scale, float dropout_p, unsigned long long seed, hipStream_t s) {
  const int rc = cross_check(__func__, q && kv && ctx, dtype, B, nh, dh, Lq, Lk, dropout_p,
                             {{q, ldq, 1}, {kv, ldkv, 2}}, "ldq < H or ldkv < 2 H",
                             (long long)B * nh * ((Lq + QT - 1) / QT) < (1LL << 31) &&
                                 (long long)B * nh * Lq < (1LL << 31),
                             aligned16(ctx));
  if (rc != VCG_OK) return rc;
  const bool drop = dropout_p > 0.f;  // (p = 0: the inference kernels, bit for bit)
  if (dtype == VCG_BF16) {
    const int nQ = (Lq + QT - 1) / QT;
    hipLaunchKernelGGL(drop ? cross_attn_kv_fwd_kernel<true> : cross_attn_kv_fwd_kernel<false>, dim3(B * nh * nQ),
                       dim3(256), 0, s, (const bf16_t*)q, ldq, (const bf16_t*)kv, ldkv, key_mask, (bf16_t*)ctx,
                       (float2*)stats, nh, Lq, Lk, nQ, scale, dropout_p, (uint64_t)seed);
  } else {
    hipLaunchKernelGGL(drop ? cross_attn_kv_fwd_f32_kernel<true> : cross_attn_kv_fwd_f32_kernel<false>,
                       dim3(B * nh * Lq), dim3(64), 0, s, (const float*)q, ldq, (const float*)kv, ldkv, key_mask,
                       (float*)ctx, (float2*)stats, nh, Lq, Lk, scale, dropout_p, (uint64_t)seed);
  }
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

// (the inference entry: the training entry without dropout, which holds the checks)
VCG_API int vcg_cross_attn_kv_fwd(int dtype, const void* q, long long ldq, const void* kv, long long ldkv,
                                  const long long* key_mask, void* ctx, float* stats, int B, int nh, int dh, int Lq,
                                  int Lk, float scale, hipStream_t s) {
  return vcg_cross_attn_kv_fwd_ex(dtype, q, ldq, kv, ldkv, key_mask, ctx, stats, B, nh, dh, Lq, Lk, scale, 0.f, 0, s);
}

VCG_API int vcg_cross_attn_kv_bwd(int dtype, const void* q, long long ldq, const void* kv, long long ldkv,
                                  const long long* key_mask, const void* dctx, long long lddo, const float* stats,
                                  float* d_ws, void* dq, long long lddq, void* dkv, long long lddkv,
                                  int B, int nh, int dh, int Lq, int Lk, float scale, float dropout_p,
                                  unsigned long long seed, hipStream_t s) {
  const int rc = cross_check(__func__, q && kv && dctx && stats && d_ws && dq && dkv, dtype, B, nh, dh, Lq, Lk,
                             dropout_p, {{q, ldq, 1}, {kv, ldkv, 2}, {dctx, lddo, 1}, {dq, lddq, 1}, {dkv, lddkv, 2}},
                             "a row pitch is below H (q, dctx, dq) or 2 H (kv, dkv)",
                             (long long)B * nh * Lq < (1LL << 31) && (long long)B * nh * Lk < (1LL << 31));
  if (rc != VCG_OK) return rc;
  const int nQ = (Lq + QT - 1) / QT, nK = (Lk + LT - 1) / LT;
  if (dtype == VCG_BF16) {
    hipLaunchKernelGGL(cross_attn_kv_dq_kernel, dim3(B * nh * nQ), dim3(256), 0, s, (const bf16_t*)q, ldq,
                       (const bf16_t*)kv, ldkv, key_mask, (const bf16_t*)dctx, lddo, (const float2*)stats, d_ws,
                       (bf16_t*)dq, lddq, nh, Lq, Lk, nQ, scale, dropout_p, (uint64_t)seed);
    VCG_LAUNCH_CHECK();
    hipLaunchKernelGGL(cross_attn_kv_dkv_kernel, dim3(B * nh * nK), dim3(256), 0, s, (const bf16_t*)q, ldq,
                       (const bf16_t*)kv, ldkv, key_mask, (const bf16_t*)dctx, lddo, (const float2*)stats,
                       (const float*)d_ws, (bf16_t*)dkv, lddkv, nh, Lq, Lk, nK, scale, dropout_p, (uint64_t)seed);
  } else {
    hipLaunchKernelGGL(cross_attn_kv_dq_f32_kernel, dim3(B * nh * Lq), dim3(64), 0, s, (const float*)q, ldq,
                       (const float*)kv, ldkv, key_mask, (const float*)dctx, lddo, (const float2*)stats, d_ws,
                       (float*)dq, lddq, nh, Lq, Lk, scale, dropout_p, (uint64_t)seed);
    VCG_LAUNCH_CHECK();
    hipLaunchKernelGGL(cross_attn_kv_dkv_f32_kernel, dim3(B * nh * Lk), dim3(64), 0, s, (const float*)q, ldq,
                       (const float*)kv, ldkv, key_mask, (const float*)dctx, lddo, (const float2*)stats,
                       (const float*)d_ws, (float*)dkv, lddkv, nh, Lq, Lk, scale, dropout_p, (uint64_t)seed);
  }
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

// (p = 0 launches the DROP = false instantiation: the inference kernel)
VCG_API int vcg_pegasus_embed_fwd_ex(int dtype, const long long* ids, const float* tok, const float* pos, void* out,
                                     int B, int L, int H, int V, int n_pos, float scale, int pos0, float dropout_p,
                                     unsigned long long seed, hipStream_t s) {
  VCG_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "dropout_p must be in [0, 1)");
  VCG_REQUIRE(ids && tok && pos && out, "null argument");
  VCG_REQUIRE(dtype == VCG_F32 || dtype == VCG_BF16, "dtype must be VCG_F32 or VCG_BF16");
  VCG_REQUIRE(B > 0 && L > 0 && H > 0 && V > 0 && n_pos > 0 && pos0 >= 0, "bad shape");
  VCG_REQUIRE((long long)pos0 + L <= n_pos, "position pos0 + L - 1 is outside the position table");
  VCG_REQUIRE((long long)B * L < (1LL << 31), "grid too large");
  const bool drop = dropout_p > 0.f;
  if (dtype == VCG_BF16)
    hipLaunchKernelGGL((drop ? pegasus_embed_fwd_kernel<bf16_t, true> : pegasus_embed_fwd_kernel<bf16_t, false>),
                       dim3(B * L), dim3(256), 0, s, ids, tok, pos, (bf16_t*)out, L, H, V, scale, pos0, dropout_p,
                       (uint64_t)seed);
  else
    hipLaunchKernelGGL((drop ? pegasus_embed_fwd_kernel<float, true> : pegasus_embed_fwd_kernel<float, false>),
                       dim3(B * L), dim3(256), 0, s, ids, tok, pos, (float*)out, L, H, V, scale, pos0, dropout_p,
                       (uint64_t)seed);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

// (the inference entry: the training entry without dropout, which holds the checks)
VCG_API int vcg_pegasus_embed_fwd(int dtype, const long long* ids, const float* tok, const float* pos, void* out, int B,
                                  int L, int H, int V, int n_pos, float scale, int pos0, hipStream_t s) {
  return vcg_pegasus_embed_fwd_ex(dtype, ids, tok, pos, out, B, L, H, V, n_pos, scale, pos0, 0.f, 0, s);
}

// the four streaming kernels of the dropout sites: one thread per 8 elements; T in the argument list is the element
// type, the last argument says whether every pointer is 16-B aligned
#define VCG_EW_LAUNCH(kernel, ...)                                                                 \
  do {                                                                                             \
    VCG_REQUIRE(dtype == VCG_F32 || dtype == VCG_BF16, "dtype must be VCG_F32 or VCG_BF16");       \
    VCG_REQUIRE(n >= 0 && (n + 255) / 256 < (1LL << 31), "bad element count");                     \
    VCG_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "dropout_p must be in [0, 1)");               \
    if (n == 0) return VCG_OK;                                                                     \
    const dim3 grid((unsigned)(((n + 7) / 8 + 255) / 256)); /* a thread per group of 8 */          \
    if (dtype == VCG_BF16) {                                                                       \
      typedef bf16_t T;                                                                            \
      hipLaunchKernelGGL(kernel<T>, grid, dim3(256), 0, s, __VA_ARGS__);                           \
    } else {                                                                                       \
      typedef float T;                                                                             \
      hipLaunchKernelGGL(kernel<T>, grid, dim3(256), 0, s, __VA_ARGS__);                           \
    }                                                                                              \
    VCG_LAUNCH_CHECK();                                                                            \
    return VCG_OK;                                                                                 \
  } while (0)

VCG_API int vcg_dropout_add_fwd(int dtype, float* h, const void* branch, long long n, float dropout_p,
                                unsigned long long seed, hipStream_t s) {
  VCG_REQUIRE(h && branch, "null argument");
  const bool vec = aligned16(h) && aligned16(branch);
  VCG_EW_LAUNCH(dropout_add_fwd_kernel, h, (const T*)branch, n, dropout_p, (uint64_t)seed, vec);
}

VCG_API int vcg_dropout_add_bwd(int dtype, const float* dh, void* dbranch, long long n, float dropout_p,
                                unsigned long long seed, hipStream_t s) {
  VCG_REQUIRE(dh && dbranch, "null argument");
  const bool vec = aligned16(dh) && aligned16(dbranch);
  VCG_EW_LAUNCH(dropout_add_bwd_kernel, dh, (T*)dbranch, n, dropout_p, (uint64_t)seed, vec);
}

VCG_API int vcg_relu_dropout_fwd(int dtype, const void* pre, void* f, long long n, float dropout_p,
                                 unsigned long long seed, hipStream_t s) {
  VCG_REQUIRE(pre && f, "null argument");
  const bool vec = aligned16(pre) && aligned16(f);
  VCG_EW_LAUNCH(relu_dropout_fwd_kernel, (const T*)pre, (T*)f, n, dropout_p, (uint64_t)seed, vec);
}

VCG_API int vcg_relu_dropout_bwd(int dtype, const void* dy, const void* f, void* dpre, long long n, float dropout_p,
                                 hipStream_t s) {
  VCG_REQUIRE(dy && f && dpre, "null argument");
  const bool vec = aligned16(dy) && aligned16(f) && aligned16(dpre);
  VCG_EW_LAUNCH(relu_dropout_bwd_kernel, (const T*)dy, (const T*)f, (T*)dpre, n, dropout_p, vec);
}
