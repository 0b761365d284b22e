// Pegasus (encoder-decoder) inference kernels: what the engine's BERT / GPT kernels cannot express (reference
// model/lang/pegasus_hugface.py -> transformers PegasusForConditionalGeneration):
//   vcg_cross_attn_kv_fwd  decoder queries [B Lq] over one layer's encoder keys / values [B Lk], Lq != Lk, separate Q
//                          and K | V buffers, a key-padding mask; nothing Lq x Lk in HBM
//   vcg_pegasus_embed_fwd  scale * tok[ids] + pos[pos0 + t] (the sinusoidal table is not learned and is not scaled)
// Every reduction runs in a fixed order and there is no floating-point atomic: the results are bit-identical run to run.
#include "bert_attn_steps.h"

using namespace vcg;
using namespace vcg::attn;

namespace {

constexpr int QT = 16;  // queries of a workgroup: one MFMA tile

// does sequence row `row` .. + Lk - 1 of the mask hold any valid key? (block-uniform; every thread must call it)
__device__ __forceinline__ bool seq_has_key(const long long* mask, long long row, int Lk) {
  if (mask == nullptr) return true;
  int any = 0;
  for (int k = threadIdx.x; k < Lk; k += blockDim.x) any |= mask[row + k] != 0;
  return __syncthreads_or(any) != 0;
}

// One workgroup (4 waves) per (sequence b, head h, 16-query tile). The keys go by in tiles of LT = 128: the workgroup
// transposes the tile's V into LDS (load_transpose: the A operand of O^T += V^T P^T), wave w owns the tile's keys
// 32 w .. 32 w + 31 and reads their K fragments straight from HBM (load_frags: every K byte is used once per
// workgroup). Per strip: S^T = K Q^T (4 MFMAs; a lane holds [key 32 w + 16 kt + 4 g + r][query i]), the online softmax
// (m, l, O) of the wave's keys, O^T += V^T P^T (4 MFMAs, P from registers: pack8). The four partials are combined
// through LDS in the order 0..3.
// Masking is attn_prob's rule: a masked key has P = 0; in a sequence without any valid key every key in range has the
// same weight (has_key false: the reference maximum is fixed at 0 and every in-range P is 1).
__global__ __launch_bounds__(256) void cross_attn_kv_fwd_kernel(const bf16_t* __restrict__ q, long long ldq,
                                                                const bf16_t* __restrict__ kv, long long ldkv,
                                                                const long long* __restrict__ mask,
                                                                bf16_t* __restrict__ ctx, float2* __restrict__ stats,
                                                                int nh, int Lq, int Lk, int nQ, float scale) {
  __shared__ __attribute__((aligned(16))) bf16_t Vt[DH * TP];
  __shared__ uint8_t kval[LT];
  __shared__ float sm[4][QT], sl[4][QT];
  __shared__ __attribute__((aligned(16))) float so[4][QT][DH];

  const int z = blockIdx.x / nQ, q0 = QT * (blockIdx.x - z * nQ);
  const int b = z / nh, h = z - b * nh;
  const int H = nh * DH;
  const int tid = threadIdx.x, w = tid >> 6, g = (tid & 63) >> 4, i = tid & 15;
  const bf16_t* Qs = q + (long long)b * Lq * ldq + h * DH;
  const bf16_t* Ks = kv + (long long)b * Lk * ldkv + h * DH;
  const bf16_t* Vs = Ks + H;
  const long long mrow = (long long)b * Lk;
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
  *reinterpret_cast<uint2*>(ctx + ((long long)b * Lq + q0 + qi) * H + h * DH + d0) =
      make_uint2(pack2(o[0] * inv, o[1] * inv), pack2(o[2] * inv, o[3] * inv));
  if (stats && d0 == 0) stats[(long long)z * Lq + q0 + qi] = make_float2(has_key ? mt : -INFINITY, lt);
}

// The fp32 parity mode: one wave per (sequence, head, query). Lane j owns keys j, j + 64, ... with an online softmax
// over them (library expf); the 64 partials are added through LDS in lane order.
__global__ __launch_bounds__(64) void cross_attn_kv_fwd_f32_kernel(const float* __restrict__ q, long long ldq,
                                                                   const float* __restrict__ kv, long long ldkv,
                                                                   const long long* __restrict__ mask,
                                                                   float* __restrict__ ctx, float2* __restrict__ stats,
                                                                   int nh, int Lq, int Lk, float scale) {
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
#pragma unroll
    for (int d = 0; d < DH; ++d) acc[d] = fmaf(acc[d], corr, p * vr[d]);
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
// rounding), one rounding to fp32, and from there to the storage dtype
template <typename T>
__global__ void pegasus_embed_fwd_kernel(const long long* __restrict__ ids, const float* __restrict__ tok,
                                         const float* __restrict__ pos, T* __restrict__ out, int L, int H, int V,
                                         float scale, int pos0) {
  const long long row = blockIdx.x;
  const int t = (int)(row % L);
  long long id = ids[row];
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);  // (ids are validated where they are made; never read outside the table)
  const float* tr = tok + id * H;
  const float* pr = pos + (long long)(pos0 + t) * H;
  for (int c = threadIdx.x; c < H; c += blockDim.x)
    out[row * H + c] = from_f<T>((float)((double)scale * (double)tr[c] + (double)pr[c]));
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace

VCG_API int vcg_cross_attn_kv_fwd(int dtype, const void* q, long long ldq, const void* kv, long long ldkv,
                                  const long long* key_mask, void* ctx, float* stats, int B, int nh, int dh, int Lq,
                                  int Lk, float scale, hipStream_t s) {
  VCG_REQUIRE(dh == DH, "head dim must be 64");
  VCG_REQUIRE(q && kv && ctx, "null argument");
  VCG_REQUIRE(dtype == VCG_F32 || dtype == VCG_BF16, "dtype must be VCG_F32 or VCG_BF16");
  VCG_REQUIRE(B > 0 && nh > 0 && Lq >= 1 && Lk >= 1, "bad shape");
  const long long H = (long long)nh * DH;
  VCG_REQUIRE(ldq >= H && ldkv >= 2 * H, "ldq < H or ldkv < 2 H");
  VCG_REQUIRE((long long)B * nh * ((Lq + QT - 1) / QT) < (1LL << 31) && (long long)B * nh * Lq < (1LL << 31),
              "grid too large");
  if (dtype == VCG_BF16) {
    VCG_REQUIRE(ldq % 8 == 0 && ldkv % 8 == 0 && aligned16(q) && aligned16(kv) && aligned16(ctx), "16-B alignment");
    const int nQ = (Lq + QT - 1) / QT;
    hipLaunchKernelGGL(cross_attn_kv_fwd_kernel, dim3(B * nh * nQ), dim3(256), 0, s, (const bf16_t*)q, ldq,
                       (const bf16_t*)kv, ldkv, key_mask, (bf16_t*)ctx, (float2*)stats, nh, Lq, Lk, nQ, scale);
  } else {
    hipLaunchKernelGGL(cross_attn_kv_fwd_f32_kernel, dim3(B * nh * Lq), dim3(64), 0, s, (const float*)q, ldq,
                       (const float*)kv, ldkv, key_mask, (float*)ctx, (float2*)stats, nh, Lq, Lk, scale);
  }
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_pegasus_embed_fwd(int dtype, const long long* ids, const float* tok, const float* pos, void* out, int B,
                                  int L, int H, int V, int n_pos, float scale, int pos0, hipStream_t s) {
  VCG_REQUIRE(ids && tok && pos && out, "null argument");
  VCG_REQUIRE(dtype == VCG_F32 || dtype == VCG_BF16, "dtype must be VCG_F32 or VCG_BF16");
  VCG_REQUIRE(B > 0 && L > 0 && H > 0 && V > 0 && n_pos > 0 && pos0 >= 0, "bad shape");
  VCG_REQUIRE((long long)pos0 + L <= n_pos, "position pos0 + L - 1 is outside the position table");
  VCG_REQUIRE((long long)B * L < (1LL << 31), "grid too large");
  if (dtype == VCG_BF16)
    hipLaunchKernelGGL(pegasus_embed_fwd_kernel<bf16_t>, dim3(B * L), dim3(256), 0, s, ids, tok, pos, (bf16_t*)out, L, H,
                       V, scale, pos0);
  else
    hipLaunchKernelGGL(pegasus_embed_fwd_kernel<float>, dim3(B * L), dim3(256), 0, s, ids, tok, pos, (float*)out, L, H, V,
                       scale, pos0);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}
