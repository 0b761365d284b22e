// GPT text generation on a KV cache (the consumer of the generative stage's checkpoint; reference
// train_lang/test_gpt_hugface.py -> common_utils/language_model_utils.py:token_idx_sample, which re-runs the whole
// decoder on the whole prefix for every token):
//   vcg_attn_decode      one query row per sequence over its cached keys, the new key / value appended by the kernel
//   vcg_sample_topk      temperature, top-k cut (ties at the k-th value kept), inverse-CDF draw or argmax, on the device
//   vcg_gpt_embed_at     tokens_embed[seq[b][len0[b] + t]] + positions_embed[len0[b] + t]
//   vcg_gpt_decode_step  one token of the whole decoder enqueued from C: nothing is read back between tokens
// Every reduction runs in a fixed order and there is no floating-point atomic: the results are bit-identical run to run.
#include "common.h"
#include "../../include/vcg_gpt_decode.h"

using namespace vcg;

extern "C" {
int vcg_gemm(int dtype, int transA, int transB, int M, int N, int K, const void* A, long long lda, const void* B,
             long long ldb, void* C, long long ldc, const float* bias, int act, const void* residual, long long ldr,
             void* aux, float alpha, hipStream_t stream);
int vcg_ln_fwd(int dtype, const void* x, const void* res, const float* gamma, const float* beta, void* out,
               float* mean, float* rstd, int rows, int H, float eps, float dropout_p, unsigned long long seed,
               hipStream_t s);
int vcg_mlm_logits(const void* hidden, int rows, const void* W, int V, int H, float* logits, long long ldz,
                   hipStream_t stream);
}

namespace {

enum { ACT_NONE = 0, ACT_GELU_TANH = 5, ACT_FLAG_WIDE = 0x200 };  // include/vcg_hip.h

// ---------------------------------------------------------------- decode attention
constexpr int DH = 64;        // head dim
constexpr int AD_WAVES = 4;   // waves of a workgroup: the keys are dealt to them in strips
constexpr int AD_UNROLL = 4;  // strips a wave has in flight (K and V: 2 x 4 16-B loads per lane)

template <typename T>
__device__ __forceinline__ void unpack16(const uint4& u, float (&out)[16 / sizeof(T)]) {
  if constexpr (sizeof(T) == 4) {
    out[0] = __uint_as_float(u.x); out[1] = __uint_as_float(u.y);
    out[2] = __uint_as_float(u.z); out[3] = __uint_as_float(u.w);
  } else {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      out[2 * i] = __uint_as_float(w[i] << 16);
      out[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
}
// exp of a non-positive argument: the fp32 parity mode keeps the library expf
template <typename T>
__device__ __forceinline__ float exp_t(float x) {
  if constexpr (sizeof(T) == 4) return expf(x);
  else return __expf(x);
}

// One workgroup per (sequence, head). A cache row (64 elements) is read by LPR = 64 sizeof(T) / 16 lanes with one 16-B
// load each, so a wave reads G = 64 / LPR keys per load instruction straight into VGPRs (nothing of the cache is staged in
// LDS: every element is used once). Strip c (G keys) belongs to wave c % 4; each lane group keeps an online softmax
// (max, sum, its E = 16 / sizeof(T) output dims) over its keys. The groups of a wave are combined by xor shuffles, the
// four waves through LDS in the order 0..3.
// The new key / value row p = len0[b] + t is taken from qkv_new (never read back from the cache) and stored at p.
template <typename T>
__global__ __launch_bounds__(AD_WAVES * 64) void attn_decode_kernel(const T* __restrict__ qkv, T* __restrict__ kcache,
                                                                    T* __restrict__ vcache,
                                                                    const int* __restrict__ len0, int t, T* __restrict__ ctx,
                                                                    int nh, int Tcap, float scale) {
  constexpr int E = 16 / sizeof(T);
  constexpr int LPR = DH / E;
  constexpr int G = 64 / LPR;
  const int b = blockIdx.x / nh, h = blockIdx.x % nh;
  const int H = nh * DH;
  const int p = len0[b] + t;
  if (p < 0 || p >= Tcap) return;  // (refused on the host from max_len0; a len0 that disagrees writes nothing)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % LPR, grp = lane / LPR;
  const T* qrow = qkv + (long long)b * 3 * H + h * DH + sub * E;
  float q[E];
  load16<T>(qrow, q);
  const uint4 kn_raw = *reinterpret_cast<const uint4*>(qrow + H);
  const uint4 vn_raw = *reinterpret_cast<const uint4*>(qrow + 2 * H);
#pragma unroll
  for (int e = 0; e < E; ++e) q[e] *= scale;
  const long long cbase = ((long long)b * nh + h) * Tcap * DH;
  const T* kc = kcache + cbase + sub * E;
  const T* vc = vcache + cbase + sub * E;
  if (wave == 0 && grp == 0) {  // the append: bit copies of this step's K and V slices
    *reinterpret_cast<uint4*>(kcache + cbase + (long long)p * DH + sub * E) = kn_raw;
    *reinterpret_cast<uint4*>(vcache + cbase + (long long)p * DH + sub * E) = vn_raw;
  }

  float m = -INFINITY, l = 0.f, acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.f;

  constexpr int ROUND = AD_WAVES * G;  // keys per round of strips
  for (int j0 = wave * G + grp; j0 <= p; j0 += ROUND * AD_UNROLL) {
    uint4 kr[AD_UNROLL], vr[AD_UNROLL];
#pragma unroll
    for (int u = 0; u < AD_UNROLL; ++u) {  // all loads first: a late wait
      const int j = j0 + u * ROUND;
      const int jc = j < p ? j : (p > 0 ? p - 1 : 0);  // (row p itself comes from qkv_new; clamped rows are discarded)
      kr[u] = *reinterpret_cast<const uint4*>(kc + (long long)jc * DH);
      vr[u] = *reinterpret_cast<const uint4*>(vc + (long long)jc * DH);
    }
#pragma unroll
    for (int u = 0; u < AD_UNROLL; ++u) {
      const int j = j0 + u * ROUND;
      if (j == p) { kr[u] = kn_raw; vr[u] = vn_raw; }
      float kf[E], vf[E];
      unpack16<T>(kr[u], kf);
      unpack16<T>(vr[u], vf);
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) s = fmaf(q[e], kf[e], s);
#pragma unroll
      for (int o = 1; o < LPR; o <<= 1) s += __shfl_xor(s, o, 64);
      if (j <= p) {  // (uniform over the lanes of a group)
        const float mn = fmaxf(m, s);
        const float corr = exp_t<T>(m - mn);  // (m = -inf: 0)
        const float pj = exp_t<T>(s - mn);
        l = fmaf(l, corr, pj);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = fmaf(acc[e], corr, pj * vf[e]);
        m = mn;
      }
    }
  }
  // the lane groups of a wave (a group without a key has m = -inf, l = 0)
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1) {
    const float mo = __shfl_xor(m, o, 64), lo = __shfl_xor(l, o, 64);
    const float mn = fmaxf(m, mo);
    const float fa = m == -INFINITY ? 0.f : exp_t<T>(m - mn);
    const float fb = mo == -INFINITY ? 0.f : exp_t<T>(mo - mn);
    l = l * fa + lo * fb;
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = acc[e] * fa + __shfl_xor(acc[e], o, 64) * fb;
    m = mn;
  }
  __shared__ float sm[AD_WAVES], sl[AD_WAVES], sacc[AD_WAVES][DH];
  if (grp == 0) {
    if (sub == 0) { sm[wave] = m; sl[wave] = l; }
#pragma unroll
    for (int e = 0; e < E; ++e) sacc[wave][sub * E + e] = acc[e];
  }
  __syncthreads();
  if (threadIdx.x < DH) {
    float mt = sm[0];
#pragma unroll
    for (int w = 1; w < AD_WAVES; ++w) mt = fmaxf(mt, sm[w]);
    float lt = 0.f, o = 0.f;
#pragma unroll
    for (int w = 0; w < AD_WAVES; ++w) {
      const float f = sm[w] == -INFINITY ? 0.f : exp_t<T>(sm[w] - mt);
      lt = fmaf(sl[w], f, lt);
      o = fmaf(sacc[w][threadIdx.x], f, o);
    }
    ctx[(long long)b * H + h * DH + threadIdx.x] = from_f<T>(o / lt);
  }
}

// ---------------------------------------------------------------- embedding at a position
template <typename T>
__global__ void gpt_embed_at_kernel(const long long* __restrict__ seq, int Tcap, const int* __restrict__ len0, int t,
                                    const float* __restrict__ tok, const float* __restrict__ pos, T* __restrict__ out,
                                    int H, int V, int n_pos) {
  const int b = blockIdx.x;
  const int p = len0[b] + t;
  if (p < 0 || p >= Tcap || p >= n_pos) return;  // (refused on the host from max_len0)
  long long id = seq[(long long)b * Tcap + p];
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);  // (ids are validated where they are made; never read outside the table)
  for (int c = threadIdx.x; c < H; c += blockDim.x)
    out[(long long)b * H + c] = from_f<T>(tok[id * H + c] + pos[(long long)p * H + c]);
}

// ---------------------------------------------------------------- sampler
constexpr int SP_THREADS = 1024;
constexpr int SP_WAVES = SP_THREADS / 64;

// order-preserving key of a float (-0 counted as +0, as a comparison does)
__device__ __forceinline__ uint32_t okey(float x) {
  const uint32_t u = __float_as_uint(x + 0.f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One workgroup per row of fp32 logits (V valid columns of ldz; the pad columns are never read).
//  1. argmax, lowest index on equal values (one 64-bit max of key : ~index) -- greedy stops here.
//  2. top_k in 1..V-1: the k-th largest key by a radix select, 4 passes of 8 bits over LDS histograms (integer counts:
//     order-free). The cut is made on the logits themselves: dividing by temperature > 0 keeps their order, and every
//     entry >= the k-th largest stays (ties included), as `out[out < v[:, [-1]]] = -inf` leaves them.
//  3. e_i = exp(z_i - max z), z = logit / temperature, summed in double in index order: wave w owns the w-th of 16
//     contiguous segments and scans it 64 entries at a time; the wave totals are added in the order 0..15.
//  4. the token is the first kept index whose running sum exceeds u * total (always found: the last kept entry's running
//     sum is the total and u < 1).
// The row (160 KB at V = 40478) is read 3 + 4 times and stays in L2.
__global__ __launch_bounds__(SP_THREADS) void sample_topk_kernel(const float* __restrict__ logits, long long ldz, int V,
                                                                 float temperature, int top_k, int greedy,
                                                                 const float* __restrict__ u_in,
                                                                 long long* __restrict__ seq, int Tcap,
                                                                 const int* __restrict__ len0, int col_off,
                                                                 const long long* __restrict__ forced, long long forced_ld,
                                                                 long long* __restrict__ chosen, long long chosen_ld,
                                                                 float* __restrict__ prob) {
  const int b = blockIdx.x;
  const float* z = logits + (long long)b * ldz;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ unsigned long long s_best[SP_WAVES];
  __shared__ unsigned int s_hist[256];
  __shared__ uint32_t s_prefix, s_rank;
  __shared__ double s_wtot[SP_WAVES];
  __shared__ int s_token;
  __shared__ float s_eprob;

  // 1. argmax
  unsigned long long best = 0;
  for (int i = tid; i < V; i += SP_THREADS) {
    const unsigned long long k = ((unsigned long long)okey(z[i]) << 32) | (uint32_t)(0xffffffffu - (uint32_t)i);
    best = k > best ? k : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if (lane == 0) s_best[wave] = best;
  __syncthreads();
  best = s_best[0];
#pragma unroll
  for (int w = 1; w < SP_WAVES; ++w) best = s_best[w] > best ? s_best[w] : best;
  const int imax = (int)(0xffffffffu - (uint32_t)(best & 0xffffffffu));
  const float zmax = z[imax] / temperature;

  int token = imax;
  float tprob = 1.f;
  if (!greedy) {
    // 2. the cut
    uint32_t thr = 0;  // keep every key >= thr
    if (top_k > 0 && top_k < V) {
      if (tid == 0) { s_prefix = 0; s_rank = (uint32_t)top_k; }
      for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        const uint32_t himask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
        for (int i = tid; i < V; i += SP_THREADS) {
          const uint32_t k = okey(z[i]);
          if ((k & himask) == prefix) atomicAdd(&s_hist[(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
          uint32_t r = s_rank, cum = 0;
          int d = 255;
          for (; d > 0; --d) {
            if (cum + s_hist[d] >= r) break;
            cum += s_hist[d];
          }
          s_rank = r - cum;
          s_prefix = prefix | ((uint32_t)d << shift);
        }
        __syncthreads();
      }
      thr = s_prefix;
    }
    // 3. running sums in index order
    const int seg = (V + SP_WAVES - 1) / SP_WAVES;
    const int i0 = wave * seg, i1 = i0 + seg < V ? i0 + seg : V;
    double carry = 0.0;
    for (int base = i0; base < i1; base += 64) {
      const int i = base + lane;
      double e = 0.0;
      if (i < i1) {
        const float x = z[i];
        if (okey(x) >= thr) e = (double)__expf(x / temperature - zmax);
      }
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(e, o, 64);
        if (lane >= o) e += up;
      }
      carry += __shfl(e, 63, 64);
    }
    if (lane == 0) s_wtot[wave] = carry;
    if (tid == 0) s_token = -1;
    __syncthreads();
    double before = 0.0, total = 0.0;
    for (int w = 0; w < SP_WAVES; ++w) {
      if (w == wave) before = total;
      total += s_wtot[w];
    }
    const double target = (double)u_in[b] * total;
    // 4. the wave whose segment holds the crossing walks it again
    if (before <= target && (before + s_wtot[wave] > target)) {
      carry = 0.0;  // (the same additions as pass 3: the segment's last running sum is its total, bit for bit)
      for (int base = i0; base < i1; base += 64) {
        const int i = base + lane;
        double e = 0.0;
        float ef = 0.f;
        if (i < i1) {
          const float x = z[i];
          if (okey(x) >= thr) { ef = __expf(x / temperature - zmax); e = (double)ef; }
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const double up = __shfl_up(e, o, 64);
          if (lane >= o) e += up;
        }
        const unsigned long long hit = __ballot(ef > 0.f && before + (carry + e) > target);
        if (hit) {
          const int first = __ffsll((long long)hit) - 1;
          if (lane == first) { s_token = i; s_eprob = (float)((double)ef / total); }
          break;
        }
        carry += __shfl(e, 63, 64);
      }
    }
    __syncthreads();
    token = s_token;
    tprob = s_eprob;
    if (token < 0) {  // (unreachable with u in [0, 1) and finite logits: fall back to the argmax, never a pad column)
      token = imax;
      tprob = (float)(1.0 / total);
    }
  }
  if (tid == 0) {
    if (chosen) chosen[(long long)b * chosen_ld] = token;
    if (prob) prob[b] = tprob;
    if (seq) {
      const int col = (len0 ? len0[b] : 0) + col_off;
      if (col >= 0 && col < Tcap)
        seq[(long long)b * Tcap + col] = forced ? forced[(long long)b * forced_ld] : (long long)token;
    }
  }
}

// ---------------------------------------------------------------- skinny GEMM (M <= 16, bf16)
constexpr int SK_WAVES = 4;   // the K range is dealt to the waves of a workgroup
constexpr int SK_UNROLL = 6;  // k-steps (32 deep) a wave has in flight: 6 weight + 6 activation 16-B loads per lane

// y[M][N] = act(x[M][K] W[N][K]^T + b), M <= 16: one v_mfma_f32_16x16x32_bf16 per 32-deep k-step with the weights as
// the 16-row operand, so a lane's weight fragment W[n0 + lane % 16][k0 + 8 (lane / 16) .. + 7] is ONE 16-B load of the
// K-contiguous row straight into the VGPRs the MFMA reads (no LDS staging: every weight byte is used once), and the
// activation fragment x[lane % 16][same k] is one 16-B load of an L2-resident row (rows >= M repeat row M - 1; their
// results are not stored). The loads of SK_UNROLL steps are issued before the first MFMA waits for any. A workgroup
// owns `cols` (16, 8 or 4) columns -- lanes of the other rows of the MFMA tile load nothing -- and its four waves a
// quarter of K each; their partial tiles are added through LDS in the order 0..3.
template <typename OutT, bool GELU>
__global__ __launch_bounds__(SK_WAVES * 64) void gemm_skinny_kernel(const bf16_t* __restrict__ x,
                                                                    const bf16_t* __restrict__ W,
                                                                    const float* __restrict__ bias, OutT* __restrict__ y,
                                                                    int M, int N, int K, long long ldc, int cols) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int n0 = blockIdx.x * cols;  // (< N: the grid is ceil(N / cols))
  const bool wok = c < cols && n0 + c < N;
  const int steps = K / 32;
  const int s0 = wave * steps / SK_WAVES, s1 = (wave + 1) * steps / SK_WAVES;
  const bf16_t* xp = x + (long long)(c < M ? c : M - 1) * K + 8 * g;
  const bf16_t* wp = W + (long long)(wok ? n0 + c : n0) * K + 8 * g;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  int s = s0;
  for (; s + SK_UNROLL <= s1; s += SK_UNROLL) {
    uint4 wf[SK_UNROLL], xf[SK_UNROLL];
#pragma unroll
    for (int u = 0; u < SK_UNROLL; ++u) {
      wf[u] = wok ? *reinterpret_cast<const uint4*>(wp + 32 * (s + u)) : zero;
      xf[u] = *reinterpret_cast<const uint4*>(xp + 32 * (s + u));
    }
#pragma unroll
    for (int u = 0; u < SK_UNROLL; ++u)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, wf[u]), __builtin_bit_cast(s16x8, xf[u]),
                                                    acc, 0, 0, 0);
  }
  for (; s < s1; ++s) {
    const uint4 wf = wok ? *reinterpret_cast<const uint4*>(wp + 32 * s) : zero;
    const uint4 xf = *reinterpret_cast<const uint4*>(xp + 32 * s);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, wf), __builtin_bit_cast(s16x8, xf), acc, 0,
                                                  0, 0);
  }
  __shared__ f32x4 red[SK_WAVES][64];
  red[wave][lane] = acc;
  __syncthreads();
  if (wave != 0 || c >= M) return;
  f32x4 t = red[0][lane];
#pragma unroll
  for (int w = 1; w < SK_WAVES; ++w) t += red[w][lane];
  // lane (g, c) holds row c, columns n0 + 4 g + r
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int col = 4 * g + r, n = n0 + col;
    if (col < cols && n < N) {
      float v = t[r] + (bias ? bias[n] : 0.f);
      if (GELU) v = gelu_tanh_fast(v);
      y[(long long)c * ldc + n] = from_f<OutT>(v);
    }
  }
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace

VCG_API int vcg_gemm_skinny(const void* x, const void* W, const float* bias, void* y, int M, int N, int K, long long ldc,
                            int act, int f32_out, hipStream_t s) {
  VCG_REQUIRE(x && W && y, "null argument");
  VCG_REQUIRE(M >= 1 && M <= 16, "M must be in 1..16 (vcg_gemm serves larger M)");
  VCG_REQUIRE(N >= 1 && K >= 32 && K % 32 == 0, "K must be a positive multiple of 32");
  VCG_REQUIRE(ldc >= N, "ldc < N");
  VCG_REQUIRE(aligned16(x) && aligned16(W), "x and W must be 16-B aligned");
  VCG_REQUIRE(act == ACT_NONE || act == ACT_GELU_TANH, "act must be VCG_ACT_NONE or VCG_ACT_GELU_TANH");
  VCG_REQUIRE(!(f32_out && act != ACT_NONE), "the fp32 output form has no activation");
  // the column slice: whole 16-column MFMA tiles where they fill at least half of the 256 CUs, else 8 or 4 columns
  const int cols = (N + 15) / 16 >= 128 ? 16 : ((N + 7) / 8 >= 128 ? 8 : 4);
  const dim3 grid((N + cols - 1) / cols), blk(SK_WAVES * 64);
  if (census_on()) census_add("gemm_skinny", M, N, K);
  const bf16_t* xb = (const bf16_t*)x;
  const bf16_t* wb = (const bf16_t*)W;
  if (f32_out)
    hipLaunchKernelGGL((gemm_skinny_kernel<float, false>), grid, blk, 0, s, xb, wb, bias, (float*)y, M, N, K, ldc, cols);
  else if (act == ACT_GELU_TANH)
    hipLaunchKernelGGL((gemm_skinny_kernel<bf16_t, true>), grid, blk, 0, s, xb, wb, bias, (bf16_t*)y, M, N, K, ldc, cols);
  else
    hipLaunchKernelGGL((gemm_skinny_kernel<bf16_t, false>), grid, blk, 0, s, xb, wb, bias, (bf16_t*)y, M, N, K, ldc, cols);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API long long vcg_gpt_decode_desc_bytes(void) { return (long long)sizeof(vcg_gpt_decode_desc); }

VCG_API int vcg_attn_decode(int dtype, const void* qkv_new, void* kcache, void* vcache, const int* len0, int max_len0,
                            int t, void* ctx, int B, int nh, int dh, int Tcap, float scale, hipStream_t s) {
  VCG_REQUIRE(qkv_new && kcache && vcache && len0 && ctx, "null argument");
  VCG_REQUIRE(dtype == VCG_F32 || dtype == VCG_BF16, "dtype must be VCG_F32 or VCG_BF16");
  if (dh != DH) {
    set_error("vcg_attn_decode: head dim must be 64");
    return VCG_ERR_UNSUPPORTED;
  }
  VCG_REQUIRE(B > 0 && nh > 0 && Tcap > 0 && t >= 0 && max_len0 >= 0, "bad shape");
  VCG_REQUIRE((long long)max_len0 + t < Tcap, "position len0 + t is outside the cache (Tcap)");
  VCG_REQUIRE(aligned16(qkv_new) && aligned16(kcache) && aligned16(vcache), "16-B alignment");
  const dim3 g(B * nh), blk(AD_WAVES * 64);
  if (dtype == VCG_BF16)
    hipLaunchKernelGGL(attn_decode_kernel<bf16_t>, g, blk, 0, s, (const bf16_t*)qkv_new, (bf16_t*)kcache,
                       (bf16_t*)vcache, len0, t, (bf16_t*)ctx, nh, Tcap, scale);
  else
    hipLaunchKernelGGL(attn_decode_kernel<float>, g, blk, 0, s, (const float*)qkv_new, (float*)kcache, (float*)vcache,
                       len0, t, (float*)ctx, nh, Tcap, scale);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_sample_topk(const float* logits, long long ldz, int B, int V, float temperature, int top_k, int greedy,
                            const float* u, long long* seq, int Tcap, const int* len0, int max_len0, int col_off,
                            const long long* forced, long long forced_ld, long long* chosen, long long chosen_ld,
                            float* prob, hipStream_t s) {
  VCG_REQUIRE(logits && B > 0 && V > 0 && ldz >= V, "bad logits shape");
  VCG_REQUIRE(temperature > 0.f, "temperature must be positive");
  VCG_REQUIRE(top_k >= 0 && top_k <= V, "top_k must be 0 (no cut) or in 1..V");
  VCG_REQUIRE(greedy || u, "sampling needs the uniforms u");
  VCG_REQUIRE(seq || chosen, "no output: seq or chosen");
  if (seq) VCG_REQUIRE(Tcap > 0 && col_off >= 0 && max_len0 >= 0 && (long long)max_len0 + col_off < Tcap,
                       "column len0 + col_off is outside seq (Tcap)");
  VCG_REQUIRE(!forced || seq, "forced tokens are written to seq");
  hipLaunchKernelGGL(sample_topk_kernel, dim3(B), dim3(SP_THREADS), 0, s, logits, ldz, V, temperature, top_k, greedy, u,
                     seq, Tcap, len0, col_off, forced, forced_ld, chosen, chosen_ld, prob);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_gpt_embed_at(int dtype, const long long* seq, int Tcap, const int* len0, int max_len0, int t,
                             const float* tok, const float* pos, void* out, int B, int H, int V, int n_pos,
                             hipStream_t s) {
  VCG_REQUIRE(seq && len0 && tok && pos && out, "null argument");
  VCG_REQUIRE(dtype == VCG_F32 || dtype == VCG_BF16, "dtype must be VCG_F32 or VCG_BF16");
  VCG_REQUIRE(B > 0 && H > 0 && V > 0 && Tcap > 0 && n_pos > 0 && t >= 0 && max_len0 >= 0, "bad shape");
  VCG_REQUIRE((long long)max_len0 + t < Tcap, "position len0 + t is outside seq (Tcap)");
  VCG_REQUIRE((long long)max_len0 + t < n_pos, "position len0 + t is outside the position table");
  if (dtype == VCG_BF16)
    hipLaunchKernelGGL(gpt_embed_at_kernel<bf16_t>, dim3(B), dim3(256), 0, s, seq, Tcap, len0, t, tok, pos,
                       (bf16_t*)out, H, V, n_pos);
  else
    hipLaunchKernelGGL(gpt_embed_at_kernel<float>, dim3(B), dim3(256), 0, s, seq, Tcap, len0, t, tok, pos, (float*)out,
                       H, V, n_pos);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

// y [B][n_out] = act(x [B][n_in] W^T + b) on the library's GEMM engines, as BertEncoderEngine._lin_fwd routes a
// Linear: the K-contiguous weight on the wide-tile engine, or the stored Conv1D weight as the N-contiguous operand
static int decode_linear(const vcg_gpt_decode_desc* d, const vcg_gpt_decode_layer& L, int i, const void* x, void* y,
                         int n_in, int n_out, int act, hipStream_t s) {
  if (d->use_skinny)  // (bf16, B <= 16, K-contiguous weights: checked by vcg_gpt_decode_step)
    return vcg_gemm_skinny(x, L.w[i], L.b[i], y, d->B, n_out, n_in, n_out, act, 0, s);
  if (d->w_stored_in_out)
    return vcg_gemm(d->dtype, 0, 1, d->B, n_out, n_in, x, n_in, L.w[i], n_out, y, n_out, L.b[i], act, nullptr, n_out,
                    nullptr, 1.f, s);
  return vcg_gemm(d->dtype, 0, 0, d->B, n_out, n_in, x, n_in, L.w[i], n_in, y, n_out, L.b[i], act | ACT_FLAG_WIDE,
                  nullptr, n_out, nullptr, 1.f, s);
}

VCG_API int vcg_gpt_decode_step(const vcg_gpt_decode_desc* d, int t, hipStream_t s) {
  VCG_REQUIRE(d, "null descriptor");
  VCG_REQUIRE(d->dtype == VCG_F32 || d->dtype == VCG_BF16, "dtype must be VCG_F32 or VCG_BF16");
  VCG_REQUIRE(d->B > 0 && d->nh > 0 && d->H == d->nh * DH, "head dim must be 64");
  VCG_REQUIRE(d->n_layer > 0 && d->n_layer <= VCG_GPT_MAX_LAYERS, "n_layer outside 1..VCG_GPT_MAX_LAYERS");
  VCG_REQUIRE(d->n_inner > 0 && d->V > 0 && d->ldz == ((long long)d->V + 7) / 8 * 8, "bad shape");
  VCG_REQUIRE(!d->use_skinny || (d->dtype == VCG_BF16 && d->B <= 16 && !d->w_stored_in_out && d->H % 32 == 0 &&
                                 d->n_inner % 32 == 0),
              "use_skinny needs bf16, B <= 16 and K-contiguous weights");
  VCG_REQUIRE(t >= 0 && t + 1 < d->steps, "step t writes generated token t + 1: t must be in 0..steps-2");
  VCG_REQUIRE(d->max_len0 >= 1, "every sequence needs a prompt token");
  // position len0 + t is embedded and cached; the sampled token goes to column len0 + t + 1
  VCG_REQUIRE((long long)d->max_len0 + t < d->n_pos, "position len0 + t is outside the position table");
  VCG_REQUIRE((long long)d->max_len0 + t + 1 < d->Tcap, "column len0 + t + 1 is outside seq / the cache (Tcap)");
  VCG_REQUIRE(d->temperature > 0.f && d->top_k >= 0 && d->top_k <= d->V, "bad sampling parameters");
  VCG_REQUIRE(d->tok && d->pos && d->head_w && d->seq && d->len0 && (d->u || d->greedy), "null argument");
  VCG_REQUIRE(d->h && d->qkv && d->ctx && d->ao && d->h1 && d->ff && d->fo && d->h2 && d->logits && d->ln_stat,
              "null workspace");
  for (int i = 0; i < d->n_layer; ++i) {
    const vcg_gpt_decode_layer& L = d->layers[i];
    VCG_REQUIRE(L.kcache && L.vcache && L.ln_g[0] && L.ln_b[0] && L.ln_g[1] && L.ln_b[1], "null layer argument");
    for (int j = 0; j < 4; ++j) VCG_REQUIRE(L.w[j] && L.b[j], "null layer weight");
  }
  const int B = d->B, H = d->H, I = d->n_inner, dt = d->dtype;
  const float scale = 0.125f;  // 1 / sqrt(64)
  float* mean = d->ln_stat;
  float* rstd = d->ln_stat + B;
  int rc;
#define VCG_STEP(call)                      \
  do {                                      \
    if ((rc = (call)) != VCG_OK) return rc; \
  } while (0)
  VCG_STEP(vcg_gpt_embed_at(dt, d->seq, d->Tcap, d->len0, d->max_len0, t, d->tok, d->pos, d->h, B, H, d->V, d->n_pos, s));
  const void* h = d->h;
  for (int i = 0; i < d->n_layer; ++i) {
    const vcg_gpt_decode_layer& L = d->layers[i];
    VCG_STEP(decode_linear(d, L, 0, h, d->qkv, H, 3 * H, ACT_NONE, s));
    VCG_STEP(vcg_attn_decode(dt, d->qkv, L.kcache, L.vcache, d->len0, d->max_len0, t, d->ctx, B, d->nh, DH, d->Tcap,
                             scale, s));
    VCG_STEP(decode_linear(d, L, 1, d->ctx, d->ao, H, H, ACT_NONE, s));
    VCG_STEP(vcg_ln_fwd(dt, d->ao, h, L.ln_g[0], L.ln_b[0], d->h1, mean, rstd, B, H, d->ln_eps, 0.f, 0, s));
    VCG_STEP(decode_linear(d, L, 2, d->h1, d->ff, H, I, ACT_GELU_TANH, s));
    VCG_STEP(decode_linear(d, L, 3, d->ff, d->fo, I, H, ACT_NONE, s));
    // the layer's output alternates between h2 and h: the next layer's residual is what this LayerNorm wrote
    void* out = (i & 1) ? d->h : d->h2;
    VCG_STEP(vcg_ln_fwd(dt, d->fo, d->h1, L.ln_g[1], L.ln_b[1], out, mean, rstd, B, H, d->ln_eps, 0.f, 0, s));
    h = out;
  }
  if (d->use_skinny)
    VCG_STEP(vcg_gemm_skinny(h, d->head_w, nullptr, d->logits, B, d->V, H, d->ldz, ACT_NONE, 1, s));
  else if (dt == VCG_BF16)
    VCG_STEP(vcg_mlm_logits(h, B, d->head_w, d->V, H, d->logits, d->ldz, s));
  else
    VCG_STEP(vcg_gemm(dt, 0, 0, B, (int)d->ldz, H, h, H, d->head_w, H, d->logits, d->ldz, nullptr, ACT_NONE, nullptr,
                      d->ldz, nullptr, 1.f, s));
  VCG_STEP(vcg_sample_topk(d->logits, d->ldz, B, d->V, d->temperature, d->top_k, d->greedy,
                           d->u ? d->u + (long long)(t + 1) * B : nullptr, d->seq, d->Tcap, d->len0, d->max_len0,
                           t + 1, d->forced ? d->forced + t + 1 : nullptr, d->steps,
                           d->chosen ? d->chosen + t + 1 : nullptr, d->steps,
                           d->prob ? d->prob + (long long)(t + 1) * B : nullptr, s));
#undef VCG_STEP
  return VCG_OK;
}
