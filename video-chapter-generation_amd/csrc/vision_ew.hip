// Streaming NHWC kernels of the vision trunk: BatchNorm apply (+residual, +ReLU), BatchNorm
// backward (reduce + apply), max-pool fwd/bwd, and the TSM gradient combine.
//
// All are HBM-bound. Layout rule used throughout: a tensor [P][C] is a stream of 16-byte vectors
// v = row * cpr + chunk (cpr = C / VN, a power of two). Blocks take contiguous runs of
// 256 * ITER vectors, so when cpr divides 256 a thread's channel chunk never changes and its
// per-channel parameters live in registers for the whole run; index math stays 32/64-bit
// shifts and masks (no 64-bit division).
//
// The steps shared with stem_bwd.hip and bn_gram.hip (the BN-backward affine map, the column-partials tail) are in
// bn_steps.h.
#include <climits>
#include <type_traits>

#include "bn_steps.h"

using namespace vcg;

namespace {

template <typename T> struct V { static constexpr int N = 16 / sizeof(T); };

#ifndef VCG_EW_SU
#define VCG_EW_SU 4
#endif
#ifndef VCG_EW_GRID
#define VCG_EW_GRID 2048
#endif
constexpr int SU = VCG_EW_SU;        // 16-B vectors per thread per batch (all loads issued before use)
constexpr int SB = 256 * SU;         // vectors per block per batch
constexpr long long GRID_MAX = VCG_EW_GRID;  // streaming grids: 8 blocks per CU, grid-stride beyond
constexpr int RED_ITER_MAX = 256;  // vectors per thread of bn_bwd_reduce (adaptive: >= ~1024 blocks)

// Which elements of the upstream gradient pass the ReLU (MODE = vcg_hip.h VCG_MASK_*, fixed per instantiation):
//   0 none; 1 tensor (mask[v] > 0); 2 bits (one byte per 16-B vector, bit e = element e);
//   3 affine (fma(y, mscale[c], mshift[c]) > 0: the forward's BN+ReLU decision recomputed from y).
struct MaskArgs {
  const void* t;
  const uint8_t* bits;
  const float* sc;
  const float* sh;
};

template <typename T, int MODE, int VN>
__device__ __forceinline__ void apply_mask(float (&d)[VN], const MaskArgs& m, long long v, const float (&yv)[VN],
                                           const float (&msc)[VN], const float (&msh)[VN]) {
  if constexpr (MODE == 1) {
    float mk[VN];
    load16<T>(reinterpret_cast<const T*>(m.t) + v * VN, mk);
#pragma unroll
    for (int e = 0; e < VN; ++e) d[e] = mk[e] > 0.f ? d[e] : 0.f;
  } else if constexpr (MODE == 2) {
    const unsigned b = m.bits[v];
#pragma unroll
    for (int e = 0; e < VN; ++e) d[e] = ((b >> e) & 1u) ? d[e] : 0.f;
  } else if constexpr (MODE == 3) {
#pragma unroll
    for (int e = 0; e < VN; ++e) d[e] = fmaf(yv[e], msc[e], msh[e]) > 0.f ? d[e] : 0.f;
  }
}

__host__ __device__ inline int ilog2i(int x) {
  int l = 0;
  while ((1 << l) < x) ++l;
  return l;
}

// ------------------------------------------------------------------ BN apply
// out = act(fma(y, scale, shift) + [fma(res, rscale, rshift) | res]); bits (optional): ReLU mask of
// out, one byte per 16-B vector (the backward's VCG_MASK_BITS). Grid-stride over batches of SU
// vectors per thread; every load of a batch is issued before the first use.
template <typename T, bool RES, bool RAFF, bool CS = false>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ y, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const T* __restrict__ res,
                                                       const float* __restrict__ rscale,
                                                       const float* __restrict__ rshift, int relu,
                                                       T* __restrict__ out, uint8_t* __restrict__ bits, long long TV,
                                                       int cpr, float* __restrict__ colpart = nullptr) {
  constexpr int VN = V<T>::N;
  const long long stride = (long long)gridDim.x * SB;
  long long base = (long long)blockIdx.x * SB + threadIdx.x;
  const bool fixed = cpr <= 256;
  float sc[VN], sh[VN], rs[VN], rb[VN];
  float csum[1][VN];  // colpart: this thread's column sums of the stored output (its channel chunk is fixed, cpr | 256)
#pragma unroll
  for (int e = 0; e < VN; ++e) csum[0][e] = 0.f;
  auto params = [&](long long v) {
    const int c0 = (int)(v & (cpr - 1)) * VN;
    load_params<VN>(scale, c0, sc);
    load_params<VN>(shift, c0, sh);
    if (RAFF) {
      load_params<VN>(rscale, c0, rs);
      load_params<VN>(rshift, c0, rb);
    }
  };
  params(base);
  for (; base < TV; base += stride) {
    float a[SU][VN], r[SU][VN];
#pragma unroll
    for (int u = 0; u < SU; ++u) {  // unconditional loads (clamped index): no per-vector branch + wait
      const long long v = min(base + u * 256, TV - 1);
      load16<T>(y + v * VN, a[u]);
      if (RES) load16<T>(res + v * VN, r[u]);
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const long long v = base + u * 256;
      if (v >= TV) break;
      if (!fixed) params(v);
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        float o = fmaf(a[u][e], sc[e], sh[e]);
        if (RES) o += RAFF ? fmaf(r[u][e], rs[e], rb[e]) : r[u][e];
        a[u][e] = relu ? fmaxf(o, 0.f) : o;
      }
      if (bits) {
        unsigned b = 0;
#pragma unroll
        for (int e = 0; e < VN; ++e) b |= (a[u][e] > 0.f ? 1u : 0u) << e;
        bits[v] = (uint8_t)b;
      }
      if constexpr (CS) {
#pragma unroll
        for (int e = 0; e < VN; ++e) csum[0][e] += to_f<T>(from_f<T>(a[u][e]));  // the stored (rounded) value
      }
      store16<T>(out + v * VN, a[u]);
    }
  }
  if constexpr (CS) {  // per-block column partials [block][C]
    __shared__ float red[256 * (VN + 1)];
    colpart_tail<1, VN, VN + 1>(red, csum, cpr, nullptr, colpart + (long long)blockIdx.x * cpr * VN);
  }
}

// Column sums of NP planes of per-block partials, 16 channels x 16 row stripes per 256-thread block: channel
// c = 16 blockIdx.x + tx, plane p of row i at part[i * ld + p * plane_off + c]. Thread ty sums rows ty, ty + 16, ... in
// double, then the thread ty == 0 of a channel adds the 16 stripes in order (deterministic) into a[] and gets true.
template <int NP>
__device__ __forceinline__ bool stripe_sum(const float* __restrict__ part, int nb, int C, long long ld, int plane_off,
                                           double (&a)[NP]) {
  __shared__ double sa[NP][16][16];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + tx;
#pragma unroll
  for (int p = 0; p < NP; ++p) a[p] = 0;
  if (c < C) {
    const float* q = part + c;
#pragma unroll 4
    for (int i = ty; i < nb; i += 16) {
#pragma unroll
      for (int p = 0; p < NP; ++p) a[p] += q[i * ld + p * plane_off];
    }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) sa[p][ty][tx] = a[p];
  __syncthreads();
  if (ty != 0 || c >= C) return false;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    a[p] = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) a[p] += sa[p][k][tx];
  }
  return true;
}

// out[c] = sum_b part[b][c] (stripe_sum's order)
__global__ __launch_bounds__(256) void colpart_reduce_kernel(const float* __restrict__ part, int nb, int C,
                                                             float* __restrict__ out) {
  double a[1];
  if (stripe_sum<1>(part, nb, C, C, 0, a)) out[blockIdx.x * 16 + (threadIdx.x & 15)] = (float)a[0];
}

// ------------------------------------------------------------------ BN backward
// partial[bx][2C]: per-channel sums of g and g*xhat over the block's rows, g = dout * mask.
// Each thread owns one 16-B channel chunk for the whole block (cpr <= 256: 256/cpr threads share a
// chunk and walk interleaved rows; cpr > 256: blockIdx.y selects 256 chunks, threads walk all rows),
// and threads sharing a chunk are combined through LDS in a fixed order: deterministic.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ dout, MaskArgs mk,
                                                            const T* __restrict__ y, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, long long P, int cpr,
                                                            int C, int rows_per_block, float* __restrict__ partial) {
  constexpr int VN = V<T>::N;
  __shared__ float part[2 * 256 * VN];
  const int tid = threadIdx.x;
  const bool narrow = cpr <= 256;
  const int chunk = narrow ? (tid & (cpr - 1)) : (blockIdx.y * 256 + tid);
  const int rstep = narrow ? 256 / cpr : 1;
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r1 = min(P, r0 + rows_per_block);
  const int c0 = chunk * VN;
  float mu[VN], is[VN], sum[2][VN], msc[VN], msh[VN];  // sum[0]: of g, sum[1]: of g * xhat
  load_params<VN>(mean, c0, mu);
  load_params<VN>(invstd, c0, is);
  if (MODE == 3) {
    load_params<VN>(mk.sc, c0, msc);
    load_params<VN>(mk.sh, c0, msh);
  }
#pragma unroll
  for (int e = 0; e < VN; ++e) { sum[0][e] = 0.f; sum[1][e] = 0.f; }
  for (long long r = r0 + (narrow ? tid / cpr : 0); r < r1; r += (long long)rstep * SU) {
    float d[SU][VN], yv[SU][VN];
#pragma unroll
    for (int u = 0; u < SU; ++u) {  // unconditional loads (clamped row): no per-vector branch + wait
      const long long rr = min(r + (long long)u * rstep, r1 - 1);
      const long long v = rr * cpr + chunk;
      load16<T>(dout + v * VN, d[u]);
      load16<T>(y + v * VN, yv[u]);
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const long long rr = r + (long long)u * rstep;
      if (rr >= r1) break;
      const long long v = rr * cpr + chunk;
      apply_mask<T, MODE, VN>(d[u], mk, v, yv[u], msc, msh);
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        sum[0][e] += d[u][e];
        sum[1][e] = fmaf(d[u][e] * (yv[u][e] - mu[e]), is[e], sum[1][e]);  // (explicit: every mode fuses the same)
      }
    }
  }
  float* out = partial + (long long)blockIdx.x * 2 * C;
  if (!narrow) {
#pragma unroll
    for (int e = 0; e < VN; ++e) {
      out[c0 + e] = sum[0][e];
      out[C + c0 + e] = sum[1][e];
    }
    return;
  }
  colpart_tail<2, VN, VN>(part, sum, cpr, nullptr, out);
}

// Column sums of partial[nb][2C] -> sum_g, sum_gx (+ dgamma/dbeta): stripe_sum over two planes, loads coalesced
// across channels and unrolled across rows. (It ran with 64 channels x 16 stripes per 1024-thread block: on a GPU busy
// with the side streams' kernels a 16-wave workgroup waited ~30 us for a CU to take it -- 53 of these per train step
// sit on the trunk's critical path, tools/queue_busy.py.)
// (row i of partial: sum_g at [i * ld + c], sum_gx at [i * ld + gx_off + c]; ld = 2C / gx_off = C for
// bn_bwd_reduce's partials)
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ partial, int nb, int C,
                                                              long long ld, int gx_off, float* sum_g, float* sum_gx,
                                                              float* dgamma, float* dbeta, int accumulate) {
  double a[2];
  if (!stripe_sum<2>(partial, nb, C, ld, gx_off, a)) return;
  const int c = blockIdx.x * 16 + (threadIdx.x & 15);
  sum_g[c] = (float)a[0];
  sum_gx[c] = (float)a[1];
  if (dbeta) dbeta[c] = (accumulate ? dbeta[c] : 0.f) + (float)a[0];
  if (dgamma) dgamma[c] = (accumulate ? dgamma[c] : 0.f) + (float)a[1];
}

// dy = A*g + B*y + Cc per channel, the batch-stat BN backward as an affine map of (g, y) (bn_steps.h bn_bwd_coefs /
// bn_bwd_map); running mode: dy = A*g. optionally gout = g (masked upstream gradient: the residual path)
template <typename T, int MODE, bool TRAIN>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dout, MaskArgs mk,
                                                           const T* __restrict__ y, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ sum_g,
                                                           const float* __restrict__ sum_gx, float inv_count,
                                                           T* __restrict__ dy, T* __restrict__ gout, long long TV,
                                                           int cpr) {
  constexpr int VN = V<T>::N;
  constexpr bool NEED_Y = TRAIN || MODE == 3;
  const long long stride = (long long)gridDim.x * SB;
  long long base = (long long)blockIdx.x * SB + threadIdx.x;
  const bool fixed = cpr <= 256;
  const BnBwdArgs bw{mean, invstd, gamma, sum_g, sum_gx};
  float A[VN], Bc[VN], Cc[VN], msc[VN], msh[VN];
  auto params = [&](long long v) {
    const int c0 = (int)(v & (cpr - 1)) * VN;
    bn_bwd_coefs<VN, TRAIN>(bw, c0, inv_count, A, Bc, Cc);
    if (MODE == 3) {
      load_params<VN>(mk.sc, c0, msc);
      load_params<VN>(mk.sh, c0, msh);
    }
  };
  params(base);
  for (; base < TV; base += stride) {
    float d[SU][VN], yv[SU][VN];
#pragma unroll
    for (int u = 0; u < SU; ++u) {  // unconditional loads (clamped index): no per-vector branch + wait
      const long long v = min(base + u * 256, TV - 1);
      load16<T>(dout + v * VN, d[u]);
      if (NEED_Y) load16<T>(y + v * VN, yv[u]);
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const long long v = base + u * 256;
      if (v >= TV) break;
      if (!fixed) params(v);
      apply_mask<T, MODE, VN>(d[u], mk, v, yv[u], msc, msh);
      if (gout) store16<T>(gout + v * VN, d[u]);
      float o[VN];
#pragma unroll
      for (int e = 0; e < VN; ++e) o[e] = bn_bwd_map(TRAIN, A[e], Bc[e], Cc[e], d[u][e], NEED_Y ? yv[u][e] : 0.f);
      store16<T>(dy + v * VN, o);
    }
  }
}

// Two batch-stat BN backward applies sharing the upstream gradient g (already masked): the first bottleneck of a
// ResNet layer, where bn3 and the downsample BN both follow the block's output ReLU. g is read once:
// dy = A g + B y + C (bn3) and dyd = Ad g + Bd yd + Cd (downsample BN), each bn_bwd_apply_kernel's map (bn_steps.h).
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_dual_kernel(const T* __restrict__ g, const T* __restrict__ y,
                                                                const T* __restrict__ yd, BnBwdArgs p1, BnBwdArgs p2,
                                                                float inv_count, T* __restrict__ dy,
                                                                T* __restrict__ dyd, long long TV, int cpr) {
  constexpr int VN = V<T>::N;
  const long long stride = (long long)gridDim.x * SB;
  long long base = (long long)blockIdx.x * SB + threadIdx.x;
  const bool fixed = cpr <= 256;
  float A[2][VN], Bc[2][VN], Cc[2][VN];
  auto params = [&](long long v) {
    const int c0 = (int)(v & (cpr - 1)) * VN;
    bn_bwd_coefs<VN>(p1, c0, inv_count, A[0], Bc[0], Cc[0]);
    bn_bwd_coefs<VN, true, true>(p2, c0, inv_count, A[1], Bc[1], Cc[1]);  // (the last channel: bn_bwd_coef's ALT)
  };
  params(base);
  for (; base < TV; base += stride) {
    float d[SU][VN], y1[SU][VN], y2[SU][VN];
#pragma unroll
    for (int u = 0; u < SU; ++u) {  // unconditional loads (clamped index)
      const long long v = min(base + u * 256, TV - 1);
      load16<T>(g + v * VN, d[u]);
      load16<T>(y + v * VN, y1[u]);
      load16<T>(yd + v * VN, y2[u]);
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const long long v = base + u * 256;
      if (v >= TV) break;
      if (!fixed) params(v);
      float o[VN], od[VN];
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        o[e] = bn_bwd_map(true, A[0][e], Bc[0][e], Cc[0][e], d[u][e], y1[u][e]);
        od[e] = bn_bwd_map(true, A[1][e], Bc[1][e], Cc[1][e], d[u][e], y2[u][e]);
      }
      store16<T>(dy + v * VN, o);
      store16<T>(dyd + v * VN, od);
    }
  }
}

// ------------------------------------------------------------------ max pool 3x3 / 2, pad 1
// thread = (output pixel, 16-B channel chunk); first max in (kh, kw) scan order (torch CPU semantics);
// the argmax bytes of a chunk are stored as one VN-byte word
template <int VN> struct IdxWord;
template <> struct IdxWord<8> { typedef uint2 t; };
template <> struct IdxWord<4> { typedef uint32_t t; };
template <int VN> __device__ __forceinline__ void idx_store(uint8_t* p, const uint8_t (&b)[VN]) {
  if constexpr (VN == 8) {
    uint2 q;
    q.x = b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
    q.y = b[4] | (b[5] << 8) | (b[6] << 16) | ((uint32_t)b[7] << 24);
    *reinterpret_cast<uint2*>(p) = q;
  } else {
    *reinterpret_cast<uint32_t*>(p) = b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
  }
}
template <int VN> __device__ __forceinline__ uint8_t idx_byte(const typename IdxWord<VN>::t& w, int e) {
  if constexpr (VN == 8) return (uint8_t)(((e < 4 ? w.x : w.y) >> (8 * (e & 3))) & 0xFF);
  else return (uint8_t)((w >> (8 * e)) & 0xFF);
}

// a = relu(fma(a, scale, shift)) rounded to T: the activation exactly as vcg_bn_apply stores it
template <typename T, int VN>
__device__ __forceinline__ void bn_relu_round(float (&a)[VN], const float (&sc)[VN], const float (&sh)[VN]) {
#pragma unroll
  for (int e = 0; e < VN; ++e) a[e] = to_f<T>(from_f<T>(fmaxf(fmaf(a[e], sc[e], sh[e]), 0.f)));
}

// The scan of output (oh, ow)'s window: taps k = 3 kh + kw in that order, padding taps skipped, first max, NaN wins.
// tap(k) gives tap k's VN values (called for the taps inside the image only).
template <int VN, typename Tap>
__device__ __forceinline__ void pool_scan(int oh, int ow, int H, int W, Tap tap, float (&best)[VN], uint8_t (&bi)[VN]) {
#pragma unroll
  for (int e = 0; e < VN; ++e) { best[e] = -INFINITY; bi[e] = 0; }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int ih = oh * 2 - 1 + k / 3, iw = ow * 2 - 1 + k % 3;
    if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
    const float(&a)[VN] = tap(k);
#pragma unroll
    for (int e = 0; e < VN; ++e)
      if (a[e] > best[e] || isnan(a[e])) { best[e] = a[e]; bi[e] = (uint8_t)k; }
  }
}

// BN: the input is the stem conv output y and the pooled values are a = bn_relu_round(y) (the fused stem: no a tensor
// in HBM, the pooled values and argmax of vcg_bn_apply then vcg_maxpool_fwd)
template <typename T, bool BN>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                          uint8_t* __restrict__ idx, int H, int W, int C, int OH,
                                                          int OW, int lcpr, long long TV, FastDiv fd_ow, FastDiv fd_oh,
                                                          const float* __restrict__ scale = nullptr,
                                                          const float* __restrict__ shift = nullptr) {
  constexpr int VN = V<T>::N;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= TV) return;
  const int chunk = (int)(v & ((1 << lcpr) - 1));
  float sc[VN], sh[VN];
  if (BN) {
    load_params<VN>(scale, chunk * VN, sc);
    load_params<VN>(shift, chunk * VN, sh);
  }
  const int pix = (int)(v >> lcpr);
  const int t = (int)fdiv((uint32_t)pix, fd_ow);
  const int ow = pix - t * OW;
  const int n = (int)fdiv((uint32_t)t, fd_oh);
  const int oh = t - n * OH;
  // all 9 window loads first, from clamped (always valid) pixels; padding taps are dropped after the load (a
  // load under a per-tap condition makes hipcc wait for each one separately)
  float a[9][VN];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int ih = min(max(oh * 2 - 1 + k / 3, 0), H - 1), iw = min(max(ow * 2 - 1 + k % 3, 0), W - 1);
    load16<T>(x + (((long long)n * H + ih) * W + iw) * C + chunk * VN, a[k]);
  }
  float best[VN];
  uint8_t bi[VN];
  pool_scan<VN>(oh, ow, H, W, [&](int k) -> const float(&)[VN] {
    if (BN) bn_relu_round<T, VN>(a[k], sc, sh);
    return a[k];
  }, best, bi);
  store16<T>(y + v * VN, best);
  idx_store<VN>(idx + v * VN, bi);
}

// Two horizontally adjacent outputs per thread (ow0 = 2 owp, ow0 + 1): their windows share the middle column, so
// the 3 x 5 input pixels are loaded (and, fused, BN + ReLU transformed) once -- 15 instead of 18 per 2 outputs. Each
// output's scan is pool_scan, as in maxpool_fwd_kernel: same values and argmax.
template <typename T, bool BN>
__global__ __launch_bounds__(256) void maxpool_fwd2_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                           uint8_t* __restrict__ idx, int H, int W, int C, int OH,
                                                           int OW, int lcpr, long long TV2, FastDiv fd_ow2,
                                                           FastDiv fd_oh, const float* __restrict__ scale = nullptr,
                                                           const float* __restrict__ shift = nullptr) {
  constexpr int VN = V<T>::N;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= TV2) return;
  const int chunk = (int)(v & ((1 << lcpr) - 1));
  float sc[VN], sh[VN];
  if (BN) {
    load_params<VN>(scale, chunk * VN, sc);
    load_params<VN>(shift, chunk * VN, sh);
  }
  const int pp = (int)(v >> lcpr);  // (n, oh, owp)
  const int t = (int)fdiv((uint32_t)pp, fd_ow2);
  const int owp = pp - t * (int)fd_ow2.d;
  const int n = (int)fdiv((uint32_t)t, fd_oh);
  const int oh = t - n * OH;
  const int ow0 = 2 * owp;
  float a[3][5][VN];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const int ih = min(max(oh * 2 - 1 + r, 0), H - 1), iw = min(max(ow0 * 2 - 1 + c, 0), W - 1);
      load16<T>(x + (((long long)n * H + ih) * W + iw) * C + chunk * VN, a[r][c]);
    }
  if (BN) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 5; ++c) bn_relu_round<T, VN>(a[r][c], sc, sh);
  }
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    const int ow = ow0 + o;
    if (ow >= OW) break;
    float best[VN];
    uint8_t bi[VN];
    pool_scan<VN>(oh, ow, H, W, [&](int k) -> const float(&)[VN] { return a[k / 3][k % 3 + 2 * o]; }, best, bi);
    const long long vo = ((((long long)n * OH + oh) * OW + ow) << lcpr) + chunk;
    store16<T>(y + vo * VN, best);
    idx_store<VN>(idx + vo * VN, bi);
  }
}

// Backward: dx of an input pixel = the sum of dy over the <= 4 windows whose argmax is this pixel. Grid-stride with a
// fixed chunk per thread (cpr <= 256). MODE (the stem's BN + ReLU backward around the pool):
//   MP_PLAIN: dx = that sum;
//   MP_RED / MP_RED_ONLY: g = the sum masked by the forward ReLU (fma(y, msc, msh) > 0), stored (MP_RED) or not,
//     and reduced into per-block partials part[block][2C] of sum g and sum g * (y - mean) * invstd (the
//     BatchNorm backward sums; bn_bwd_finalize_kernel) -- of g as stored (rounded to T);
//   MP_APPLY: the same g (rounded to T) through the BatchNorm backward apply of bn_bwd_apply_kernel (bn_steps.h),
//     dx = A g + B y + Cc (train statistics) or A g (running), so the stem needs no g tensor in HBM.
// BLK picks how a thread finds its windows; the prologue, the per-pixel finish and the tail are the same:
//   false: thread = (input pixel, chunk), the <= 2 x 2 windows with 2 oh - 1 <= ih <= 2 oh + 1;
//   true (even H and W): thread = (2x2 input block, chunk): the block's 4 pixels are reached by the 4 windows
//     (k + {0,1}, j + {0,1}) only, so the 4 windows' dy / argmax loads and the index math are shared by 4 pixels (9
//     pixel-window pairs: (0,0) <- 1 window, (0,1) / (1,0) <- 2, (1,1) <- 4), added in the per-pixel order.
enum { MP_PLAIN = 0, MP_RED = 1, MP_RED_ONLY = 2, MP_APPLY = 3 };
struct MpBn {
  BnBwdArgs b;  // mean, invstd; gamma, sum_g, sum_gx: MP_APPLY
  const float *msc, *msh;
  float* part;
  float inv_count;
  int train;
};
template <typename T, int MODE, bool BLK>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                          T* __restrict__ dx, int H, int W, int C, int OH, int OW,
                                                          int lcpr, long long TI, const T* __restrict__ yb, MpBn bn,
                                                          FastDiv fd_w, FastDiv fd_h) {
  constexpr int VN = V<T>::N;
  constexpr bool RED = MODE == MP_RED || MODE == MP_RED_ONLY;
  constexpr bool MASK = MODE != MP_PLAIN;
  typedef typename IdxWord<VN>::t IW;
  const int cpr = 1 << lcpr;
  const int chunk = threadIdx.x & (cpr - 1);
  const int c0 = chunk * VN;
  const int IW_ = BLK ? W >> 1 : W, IH_ = BLK ? H >> 1 : H;  // the item grid (fd_w, fd_h): pixels or 2x2 blocks
  float mu[VN], sc[VN], sh[VN], sum[2][VN], A[VN], Bc[VN], Cc[VN];
  if (MASK) {
    load_params<VN>(bn.msc, c0, sc);
    load_params<VN>(bn.msh, c0, sh);
  }
  if (RED) {
    load_params<VN>(bn.b.mean, c0, mu);
#pragma unroll
    for (int e = 0; e < VN; ++e) sum[0][e] = sum[1][e] = 0.f;
  }
  if (MODE == MP_APPLY) bn_bwd_coefs<VN>(bn.b, c0, bn.inv_count, A, Bc, Cc);
  // one pixel's finish: acc = its summed window gradients, yv = its conv output, v = its vector index
  auto finish = [&](float (&acc)[VN], const float (&yv)[VN], long long v) {
    if (MASK) {
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        acc[e] = fmaf(yv[e], sc[e], sh[e]) > 0.f ? acc[e] : 0.f;
        const float gr = to_f<T>(from_f<T>(acc[e]));  // the gradient as stored
        if (RED) {
          sum[0][e] += gr;
          sum[1][e] = fmaf(gr, yv[e] - mu[e], sum[1][e]);
        } else {
          acc[e] = bn_bwd_map(bn.train, A[e], Bc[e], Cc[e], gr, yv[e]);
        }
      }
    }
    if (MODE != MP_RED_ONLY) store16<T>(dx + v * VN, acc);
  };
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < TI; it += (long long)gridDim.x * 256) {
    const int item = (int)(it >> lcpr);
    const int t = (int)fdiv((uint32_t)item, fd_w);
    const int ix = item - t * IW_;
    const int n = (int)fdiv((uint32_t)t, fd_h);
    const int iy = t - n * IH_;
    float g[4][VN];
    IW w[4];
    bool use[4];
    if constexpr (!BLK) {
      const int ih = iy, iw = ix;
      float acc[VN];
#pragma unroll
      for (int e = 0; e < VN; ++e) acc[e] = 0.f;
      // the <= 2 x 2 windows with 2*oh-1 <= ih <= 2*oh+1: every candidate's loads are issued before any is used
      // (statement order matters to the register allocator: `want` before `use` costs <float, MP_RED_ONLY> a wave)
      const int oh0 = ih >> 1, oh1 = (ih + 1) >> 1;
      const int ow0 = iw >> 1, ow1 = (iw + 1) >> 1;
      float yv[VN];
      if (MASK) load16<T>(yb + it * VN, yv);
      uint8_t want[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int oh = (q & 2) ? oh1 : oh0, ow = (q & 1) ? ow1 : ow0;
        use[q] = (!(q & 2) || oh1 != oh0) && (!(q & 1) || ow1 != ow0) && oh < OH && ow < OW;
        want[q] = (uint8_t)((ih - (oh * 2 - 1)) * 3 + (iw - (ow * 2 - 1)));
        const long long o = (((long long)n * OH + min(oh, OH - 1)) * OW + min(ow, OW - 1)) * C + c0;
        load16<T>(dy + o, g[q]);  // unconditional (clamped) loads: see maxpool_fwd_kernel
        w[q] = *reinterpret_cast<const IW*>(idx + o);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (!use[q]) continue;
#pragma unroll
        for (int e = 0; e < VN; ++e)
          if (idx_byte<VN>(w[q], e) == want[q]) acc[e] += g[q][e];
      }
      finish(acc, yv, it);
    } else {
      const int k = iy, j = ix;
      // windows q = 2 dr + dc at (k + dr, j + dc)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int oh = k + (q >> 1), ow = j + (q & 1);
        use[q] = oh < OH && ow < OW;
        const long long o = (((long long)n * OH + min(oh, OH - 1)) * OW + min(ow, OW - 1)) * C + c0;
        load16<T>(dy + o, g[q]);  // unconditional (clamped) loads: see maxpool_fwd_kernel
        w[q] = *reinterpret_cast<const IW*>(idx + o);
      }
      float yv[4][VN];
      long long pv[4];
#pragma unroll
      for (int pp = 0; pp < 4; ++pp) {  // pixel (2k + a, 2j + c), pp = 2a + c
        pv[pp] = ((((long long)n * H + 2 * k + (pp >> 1)) * W + 2 * j + (pp & 1)) << lcpr) + chunk;
        if (MASK) load16<T>(yb + pv[pp] * VN, yv[pp]);
      }
#pragma unroll
      for (int pp = 0; pp < 4; ++pp) {
        const int a = pp >> 1, c = pp & 1;
        float acc[VN];
#pragma unroll
        for (int e = 0; e < VN; ++e) acc[e] = 0.f;
        // windows in the per-pixel order (oh0, ow0), (oh0, ow1), (oh1, ow0), (oh1, ow1): kh = a + 1 - 2 dr
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int dr = q >> 1, dc = q & 1;
          if ((dr && !a) || (dc && !c)) continue;  // window row / column does not contain this pixel
          if (!use[q]) continue;
          const uint8_t want = (uint8_t)((a + 1 - 2 * dr) * 3 + (c + 1 - 2 * dc));
#pragma unroll
          for (int e = 0; e < VN; ++e)
            if (idx_byte<VN>(w[q], e) == want) acc[e] += g[q][e];
        }
        finish(acc, yv[pp], pv[pp]);
      }
    }
  }
  if constexpr (RED) {
    __shared__ float red[2 * 256 * VN];
    colpart_tail<2, VN, VN>(red, sum, cpr, bn.b.invstd, bn.part + (long long)blockIdx.x * 2 * C);
  }
}

// The stem BatchNorm-backward sums from the POOLED activation instead of y: every window's gradient goes to one
// pixel (its argmax), whose ReLU output is the window's max mp -- so the pixel passes the ReLU mask iff mp > 0, and
// its normalised value is recovered from mp (z = y msc + msh => y - mean = (mp - msh) / msc - mean for mp > 0).
// Both sums are linear in the per-pixel gradient, so they are sums over windows: sum_g = sum [mp > 0] dy,
// sum_gx = invstd * sum [mp > 0] dy (y - mean). Reads dy and mp once (1/2 of the output rows' bytes each) instead
// of dy, the argmax bytes and the whole pre-pool y (the stem's conv output, 4x the pooled size). mp is the bf16
// max, so y - mean carries one bf16 rounding of the activation (the per-pixel path carries that of y).
// Degenerate channels -- msc == 0 (a zero BN weight: mp says nothing about y) or |msh| > 32 |gamma| (the recovery
// cancels: its error is ~2^-9 |msh| / |gamma| of a std) -- contribute no sum_gx here; maxpool_bn_sums_degen_kernel
// adds theirs from y at the windows' argmax pixels in a slot of its own. (A per-element gather branch inside this
// loop, never taken on the bench, cost the train step ~1 % on the same box: profiles/r05_degen_branch_ab.txt.)
__device__ __forceinline__ bool pooled_degen(float sc, float sh, float is) {
  return sc == 0.f || !(fabsf(sh) * is <= 32.f * fabsf(sc));
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_bn_sums_pooled_kernel(const T* __restrict__ dy, const T* __restrict__ mp,
                                                                     long long TV, int lcpr, MpBn bn) {
  constexpr int VN = V<T>::N;
  __shared__ float red[2 * 256 * VN];
  const int cpr = 1 << lcpr;
  const int chunk = threadIdx.x & (cpr - 1);
  const int c0 = chunk * VN;
  float mu[VN], sc[VN], sh[VN], is[VN], rsc[VN], off[VN], sum[2][VN];
  load_params<VN>(bn.b.mean, c0, mu);
  load_params<VN>(bn.msc, c0, sc);
  load_params<VN>(bn.msh, c0, sh);
  load_params<VN>(bn.b.invstd, c0, is);
#pragma unroll
  for (int e = 0; e < VN; ++e) {
    const bool dg = pooled_degen(sc[e], sh[e], is[e]);
    rsc[e] = dg ? 0.f : 1.f / sc[e];
    off[e] = dg ? 0.f : -sh[e] * rsc[e] - mu[e];  // y - mean = mp / msc + off
    sum[0][e] = sum[1][e] = 0.f;
  }
  const long long stride = (long long)gridDim.x * SB;
  for (long long base = (long long)blockIdx.x * SB + threadIdx.x; base < TV; base += stride) {
    float g[SU][VN], m[SU][VN];
#pragma unroll
    for (int u = 0; u < SU; ++u) {  // unconditional (clamped) loads, as bn_apply_kernel
      const long long v = min(base + u * 256, TV - 1);
      load16<T>(dy + v * VN, g[u]);
      load16<T>(mp + v * VN, m[u]);
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      if (base + u * 256 >= TV) break;
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        const float d = m[u][e] > 0.f ? g[u][e] : 0.f;
        sum[0][e] += d;
        sum[1][e] = fmaf(d, fmaf(m[u][e], rsc[e], off[e]), sum[1][e]);
      }
    }
  }
  colpart_tail<2, VN, VN>(red, sum, cpr, bn.b.invstd, bn.part + (long long)blockIdx.x * 2 * cpr * VN);
}

// sum_gx of the degenerate channels (pooled_degen) of maxpool_bn_sums_pooled_kernel, into the partial slot `slot`:
// one workgroup per channel; a regular channel writes zeros and returns at once (the bench's case: no channel is
// degenerate), a degenerate one sums dy (y - mean) over the windows that pass the mask, y read at the argmax pixel
// (idx byte k: pixel (2 oh - 1 + k / 3, 2 ow - 1 + k % 3) of the [N][H][W][C] pre-pool y), in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bn_sums_degen_kernel(const T* __restrict__ dy, const T* __restrict__ mp,
                                                                    const uint8_t* __restrict__ idx,
                                                                    const T* __restrict__ y, int H, int W, int OH,
                                                                    int OW, long long npix, int C, MpBn bn, int slot) {
  __shared__ float red[256];
  const int c = blockIdx.x, tid = threadIdx.x;
  const float sc = bn.msc[c], sh = bn.msh[c], is = bn.b.invstd[c], mu = bn.b.mean[c];
  float* out = bn.part + (long long)slot * 2 * C;
  if (!pooled_degen(sc, sh, is)) {
    if (tid == 0) out[c] = out[C + c] = 0.f;
    return;
  }
  float s2 = 0.f;
  for (long long v = tid; v < npix; v += 256) {
    const float m = to_f<T>(mp[v * C + c]);
    if (!(m > 0.f)) continue;
    const int ow = (int)(v % OW);
    const long long t = v / OW;
    const int oh = (int)(t % OH);
    const long long n = t / OH;
    const int k = idx[v * C + c];
    const int ih = 2 * oh - 1 + k / 3, iw = 2 * ow - 1 + k % 3;
    s2 = fmaf(to_f<T>(dy[v * C + c]), to_f<T>(y[((n * H + ih) * W + iw) * C + c]) - mu, s2);
  }
  red[tid] = s2;
  __syncthreads();
  if (tid == 0) {
    float a = 0.f;
    for (int t = 0; t < 256; ++t) a += red[t];
    out[c] = 0.f;  // (sum_g: the main pass counts every channel)
    out[C + c] = a * is;
  }
}

// ------------------------------------------------------------------ TSM gradient combine
// dx = unshift(dshift) + other over NHWC [N*T][H][W][C] (adjoint of ops/temporal_shift.py:45-47)
template <typename T, bool OTHER, bool BITS>
__global__ __launch_bounds__(256) void tsm_unshift_add_kernel(const T* __restrict__ dshift, const T* __restrict__ other,
                                                              const uint8_t* __restrict__ other_bits,
                                                              T* __restrict__ dx, unsigned TV, int lcpr,
                                                              unsigned row_vecs, int Tn, int fold_chunks) {
  constexpr int VN = V<T>::N;
  const unsigned stride = gridDim.x * SB;
  const int cmask = (1 << lcpr) - 1;
  for (unsigned base = blockIdx.x * SB + threadIdx.x; base < TV; base += stride) {
    float a[SU][VN], b[SU][VN];
    unsigned m[SU];
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const unsigned v = base + u * 256;
      if (v >= TV) continue;
      const int chunk = (int)(v & cmask);
      int dt = 0;
      if (chunk < fold_chunks) dt = -1;
      else if (chunk < 2 * fold_chunks) dt = 1;
      bool have = true;
      if (dt != 0) {
        const int t = (int)((v / row_vecs) % (unsigned)Tn);
        have = (t + dt >= 0) && (t + dt < Tn);
      }
      if (have) load16<T>(dshift + ((long long)v + dt * (long long)row_vecs) * VN, a[u]);
      else {
#pragma unroll
        for (int e = 0; e < VN; ++e) a[u][e] = 0.f;
      }
      if (OTHER) load16<T>(other + (long long)v * VN, b[u]);
      m[u] = BITS ? other_bits[v] : 0xFFu;  // residual gradient through the ReLU mask
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const unsigned v = base + u * 256;
      if (v >= TV) break;
      if (OTHER) {
#pragma unroll
        for (int e = 0; e < VN; ++e) a[u][e] += ((m[u] >> e) & 1u) ? b[u][e] : 0.f;
      }
      store16<T>(dx + (long long)v * VN, a[u]);
    }
  }
}

inline unsigned blocks_for(long long TV, int per_block) { return (unsigned)((TV + per_block - 1) / per_block); }
inline unsigned stream_grid(long long TV) {
  const long long b = (TV + SB - 1) / SB;
  return (unsigned)(b < GRID_MAX ? b : GRID_MAX);
}

}  // namespace

namespace vcg {
// column sums of EPI_BWD partials (igemm_fast.hip) -> sum_g / sum_gx (+ dgamma / dbeta, accumulated)
int bn_bwd_finalize_launch(const float* partial, int nb, int C, long long ld, int gx_off, float* sum_g, float* sum_gx,
                           float* dgamma, float* dbeta, int accumulate, hipStream_t s) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, s, partial, nb, C, ld, gx_off, sum_g,
                     sum_gx, dgamma, dbeta, accumulate);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}
}  // namespace vcg

// ==================================================================== host helpers

namespace {

// Declares VN, the 16-B vector width of dtype, and requires C to be a power-of-two multiple of it with at most
// max_cpr vectors per row (a macro: VCG_REQUIRE reports the entry point's own name).
#define VCG_EW_SHAPE(VN, dtype, C, max_cpr, msg) \
  const int VN = (dtype) == VCG_BF16 ? 8 : 4;    \
  VCG_REQUIRE((C) % VN == 0 && ((C) & ((C) - 1)) == 0 && (C) / VN <= (max_cpr), msg)
constexpr int ANY_CPR = INT_MAX;
constexpr const char* C_VEC_MSG = "C must be a power of two multiple of the vector width";

// 3x3 / stride 2 / pad 1 pool over [N][H][W][C]: output size, log2 of the vectors per pixel, the vector counts of the
// input and the output, and whether the pixel count fits the kernels' 32-bit pixel index
struct PoolGeo {
  int OH, OW, lcpr;
  long long TVin, TVout;
  bool fits;
};
PoolGeo pool_geo(int N, int H, int W, int C, int VN) {
  PoolGeo p;
  p.OH = (H + 2 - 3) / 2 + 1;
  p.OW = (W + 2 - 3) / 2 + 1;
  p.lcpr = ilog2i(C / VN);
  p.TVin = (long long)N * H * W * (C / VN);
  p.TVout = (long long)N * p.OH * p.OW * (C / VN);
  p.fits = (long long)N * H * W < (1LL << 31);
  return p;
}

// f(T{}) with T the storage type of dtype; f(Int<mode>{}) for a mask mode; yes / no for a bool template argument
template <typename F> void by_dtype(int dtype, F f) {
  if (dtype == VCG_BF16) f(bf16_t{});
  else f(float{});
}
template <int I> using Int = std::integral_constant<int, I>;
template <typename F> void by_mask_mode(int mode, F f) {
  switch (mode) {
    case 0: f(Int<0>{}); break;
    case 1: f(Int<1>{}); break;
    case 2: f(Int<2>{}); break;
    default: f(Int<3>{}); break;
  }
}
constexpr std::true_type yes{};
constexpr std::false_type no{};

// rows per block: enough blocks to fill the chip (~1024 in total) but at most RED_ITER_MAX vectors
// per thread (the per-block partials then stay small next to the streamed tensors)
long long bn_bwd_rows(long long P, int C, int VN) {
  const int cpr = C / VN;
  const long long TV = P * cpr;
  long long it = (TV + 256LL * 1024 - 1) / (256LL * 1024);
  if (it < 4) it = 4;
  if (it > RED_ITER_MAX) it = RED_ITER_MAX;
  return cpr <= 256 ? it * (256 / cpr) : it;
}
long long bn_bwd_blocks(long long P, int C, int VN) {
  const long long rows = bn_bwd_rows(P, C, VN);
  return (P + rows - 1) / rows;
}

int check_mask(int mode, const void* mask, const unsigned char* bits, const float* msc, const float* msh) {
  VCG_REQUIRE(mode >= 0 && mode <= 3, "mask_mode must be 0..3");
  VCG_REQUIRE(mode != 1 || mask, "mask_mode 1 needs the mask tensor");
  VCG_REQUIRE(mode != 2 || bits, "mask_mode 2 needs the mask bits");
  VCG_REQUIRE(mode != 3 || (msc && msh), "mask_mode 3 needs mscale/mshift");
  return VCG_OK;
}

void finalize(const float* ws, int nb, int C, float* sum_g, float* sum_gx, float* dgamma, float* dbeta, int accumulate,
              hipStream_t s) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, s, ws, nb, C, 2LL * C, C, sum_g, sum_gx,
                     dgamma, dbeta, accumulate);
}

MpBn mp_bn(const float* mean, const float* invstd, const float* mscale, const float* mshift, float* part) {
  MpBn bn{};
  bn.b.mean = mean; bn.b.invstd = invstd; bn.msc = mscale; bn.msh = mshift; bn.part = part;
  return bn;
}

// the max-pool backward in mode MODE; the stem modes take the 2x2-block gather when H and W are even
template <int MODE>
void pool_bwd(int dtype, const void* dy, const unsigned char* idx, void* dx, int H, int W, int C, const PoolGeo& p,
              const void* y, const MpBn& bn, hipStream_t s) {
  const unsigned nb = stream_grid(p.TVin);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    if (MODE != MP_PLAIN && (H & 1) == 0 && (W & 1) == 0)
      hipLaunchKernelGGL((maxpool_bwd_kernel<T, MODE, MODE != MP_PLAIN>), dim3(nb), dim3(256), 0, s, (const T*)dy, idx,
                         (T*)dx, H, W, C, p.OH, p.OW, p.lcpr, p.TVin / 4, (const T*)y, bn, make_fastdiv(W / 2),
                         make_fastdiv(H / 2));
    else
      hipLaunchKernelGGL((maxpool_bwd_kernel<T, MODE, false>), dim3(nb), dim3(256), 0, s, (const T*)dy, idx, (T*)dx, H,
                         W, C, p.OH, p.OW, p.lcpr, p.TVin, (const T*)y, bn, make_fastdiv(W), make_fastdiv(H));
  });
}

}  // namespace

// ==================================================================== C ABI

// vcg_bn_apply (no residual) that also returns the column sums of the stored output (the bn3 fold's colsum(a2)
// without a pass of its own); ws: vcg_bn_apply_colsum_ws_bytes
VCG_API long long vcg_bn_apply_colsum_ws_bytes(long long P, int C) {
  return (long long)stream_grid(P * C / 8) * C * 4 + 256;
}

VCG_API int vcg_bn_apply_colsum(const void* y, const float* scale, const float* shift, int relu, void* out,
                                float* colsum, float* ws, long long ws_bytes, long long P, int C, hipStream_t s) {
  VCG_REQUIRE(y && scale && shift && out && colsum && ws, "null argument");
  VCG_EW_SHAPE(VN, VCG_BF16, C, 256, "C must be a power of two in [8, 2048]");
  const long long TV = P * C / VN;
  if (TV == 0) return VCG_OK;
  const unsigned g = stream_grid(TV);
  VCG_REQUIRE(ws_bytes >= (long long)g * C * 4, "workspace too small");
  hipLaunchKernelGGL((bn_apply_kernel<bf16_t, false, false, true>), dim3(g), dim3(256), 0, s, (const bf16_t*)y, scale, shift,
                     (const bf16_t*)nullptr, (const float*)nullptr, (const float*)nullptr, relu, (bf16_t*)out,
                     (uint8_t*)nullptr, TV, C / VN, ws);
  VCG_LAUNCH_CHECK();
  hipLaunchKernelGGL(colpart_reduce_kernel, dim3((C + 15) / 16), dim3(256), 0, s, ws, (int)g, C, colsum);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_bn_apply(int dtype, const void* y, const float* scale, const float* shift, const void* res,
                         const float* rscale, const float* rshift, int relu, void* out, unsigned char* bits,
                         long long P, int C, hipStream_t s) {
  VCG_EW_SHAPE(VN, dtype, C, ANY_CPR, C_VEC_MSG);
  const long long TV = P * C / VN;
  const int cpr = C / VN;
  if (TV == 0) return VCG_OK;
  const unsigned g = stream_grid(TV);
  const bool raff = rscale != nullptr;
  VCG_REQUIRE(!raff || (res && rshift), "rscale needs res and rshift");
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    auto go = [&](auto R, auto A) {
      hipLaunchKernelGGL((bn_apply_kernel<T, decltype(R)::value, decltype(A)::value>), dim3(g), dim3(256), 0, s,
                         (const T*)y, scale, shift, (const T*)res, rscale, rshift, relu, (T*)out, bits, TV, cpr);
    };
    if (!res) go(no, no);
    else if (!raff) go(yes, no);
    else go(yes, yes);
  });
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API long long vcg_bn_bwd_ws_bytes(long long P, int C) {
  // one query serves both dtypes (vector width 4 for fp32, 8 for bf16)
  const long long nb = bn_bwd_blocks(P, C, 4) > bn_bwd_blocks(P, C, 8) ? bn_bwd_blocks(P, C, 4) : bn_bwd_blocks(P, C, 8);
  return nb * 2 * C * 4 + 64;
}

VCG_API int vcg_bn_bwd_reduce(int dtype, const void* dout, int mask_mode, const void* mask, const unsigned char* mbits,
                              const float* mscale, const float* mshift, const void* y, const float* mean,
                              const float* invstd, long long P, int C, float* ws, long long ws_bytes, float* sum_g,
                              float* sum_gx, float* dgamma, float* dbeta, int accumulate, hipStream_t s) {
  if (int rc = check_mask(mask_mode, mask, mbits, mscale, mshift)) return rc;
  const MaskArgs mk{mask, mbits, mscale, mshift};
  VCG_EW_SHAPE(VN, dtype, C, 2048 / VN, "C must be a power of two <= 2048");
  VCG_REQUIRE(ws_bytes >= vcg_bn_bwd_ws_bytes(P, C), "workspace too small");
  const int cpr = C / VN;
  const long long nb = bn_bwd_blocks(P, C, VN);
  const int rows = (int)bn_bwd_rows(P, C, VN);
  const dim3 grid((unsigned)nb, cpr > 256 ? cpr / 256 : 1);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    by_mask_mode(mask_mode, [&](auto M) {
      hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, decltype(M)::value>), grid, dim3(256), 0, s, (const T*)dout, mk,
                         (const T*)y, mean, invstd, P, cpr, C, rows, ws);
    });
  });
  VCG_LAUNCH_CHECK();
  finalize(ws, (int)nb, C, sum_g, sum_gx, dgamma, dbeta, accumulate, s);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_bn_bwd_apply(int dtype, const void* dout, int mask_mode, const void* mask, const unsigned char* mbits,
                             const float* mscale, const float* mshift, const void* y, const float* mean,
                             const float* invstd, const float* gamma, const float* sum_g, const float* sum_gx,
                             long long count, int train_stats, void* dy, void* gout, long long P, int C,
                             hipStream_t s) {
  if (int rc = check_mask(mask_mode, mask, mbits, mscale, mshift)) return rc;
  const MaskArgs mk{mask, mbits, mscale, mshift};
  VCG_EW_SHAPE(VN, dtype, C, ANY_CPR, C_VEC_MSG);
  const long long TV = P * C / VN;
  const float ic = 1.f / (float)count;
  const unsigned g = stream_grid(TV);
  const int cpr = C / VN;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    by_mask_mode(mask_mode, [&](auto M) {
      auto go = [&](auto TR) {
        hipLaunchKernelGGL((bn_bwd_apply_kernel<T, decltype(M)::value, decltype(TR)::value>), dim3(g), dim3(256), 0, s,
                           (const T*)dout, mk, (const T*)y, mean, invstd, gamma, sum_g, sum_gx, ic, (T*)dy, (T*)gout,
                           TV, cpr);
      };
      if (train_stats) go(yes);
      else go(no);
    });
  });
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_bn_bwd_apply_dual(int dtype, const void* g, const void* y, const float* mean, const float* invstd,
                                  const float* gamma, const float* sum_g, const float* sum_gx, const void* yd,
                                  const float* mean_d, const float* invstd_d, const float* gamma_d,
                                  const float* sum_g_d, const float* sum_gx_d, long long count, void* dy, void* dyd,
                                  long long P, int C, hipStream_t s) {
  VCG_EW_SHAPE(VN, dtype, C, ANY_CPR, C_VEC_MSG);
  const long long TV = P * C / VN;
  if (TV == 0) return VCG_OK;
  VCG_REQUIRE(g && y && yd && dy && dyd && mean && invstd && sum_g && sum_gx && mean_d && invstd_d && sum_g_d &&
                  sum_gx_d,
              "null operand");
  const BnBwdArgs p1{mean, invstd, gamma, sum_g, sum_gx}, p2{mean_d, invstd_d, gamma_d, sum_g_d, sum_gx_d};
  const float ic = 1.f / (float)count;
  const unsigned gr = stream_grid(TV);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(bn_bwd_apply_dual_kernel<T>, dim3(gr), dim3(256), 0, s, (const T*)g, (const T*)y, (const T*)yd,
                       p1, p2, ic, (T*)dy, (T*)dyd, TV, C / VN);
  });
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_maxpool_fwd(int dtype, const void* x, void* y, unsigned char* idx, int N, int H, int W, int C,
                            hipStream_t s) {
  VCG_EW_SHAPE(VN, dtype, C, ANY_CPR, C_VEC_MSG);
  const PoolGeo p = pool_geo(N, H, W, C, VN);
  VCG_REQUIRE(p.fits, "too many pixels");
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((maxpool_fwd_kernel<T, false>), dim3(blocks_for(p.TVout, 256)), dim3(256), 0, s, (const T*)x,
                       (T*)y, idx, H, W, C, p.OH, p.OW, p.lcpr, p.TVout, make_fastdiv(p.OW), make_fastdiv(p.OH));
  });
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_maxpool_bwd(int dtype, const void* dy, const unsigned char* idx, void* dx, int N, int H, int W, int C,
                            hipStream_t s) {
  VCG_EW_SHAPE(VN, dtype, C, 256, C_VEC_MSG);
  const PoolGeo p = pool_geo(N, H, W, C, VN);
  VCG_REQUIRE(p.fits, "too many pixels");
  pool_bwd<MP_PLAIN>(dtype, dy, idx, dx, H, W, C, p, nullptr, MpBn{}, s);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API long long vcg_maxpool_bwd_bn_ws_bytes(int C) { return (GRID_MAX + 1) * 2 * C * 4 + 64; }

// max-pool backward fused with the stem BatchNorm-backward reduction: g = maxpool_bwd(dy) masked by the
// forward ReLU (fma(y, mscale, mshift) > 0); sum_g / sum_gx finalized, dgamma / dbeta accumulated. g == NULL:
// the sums only (vcg_maxpool_bwd_bn_apply then recomputes g).
VCG_API int vcg_maxpool_bwd_bn(int dtype, const void* dy, const unsigned char* idx, void* g, int N, int H, int W,
                               int C, const void* y, const float* mean, const float* invstd, const float* mscale,
                               const float* mshift, float* ws, long long ws_bytes, float* sum_g, float* sum_gx,
                               float* dgamma, float* dbeta, hipStream_t s) {
  VCG_EW_SHAPE(VN, dtype, C, 256, C_VEC_MSG);
  VCG_REQUIRE(y && mean && invstd && mscale && mshift && sum_g && sum_gx, "BN arguments required");
  VCG_REQUIRE(ws_bytes >= vcg_maxpool_bwd_bn_ws_bytes(C), "workspace too small");
  const PoolGeo p = pool_geo(N, H, W, C, VN);
  VCG_REQUIRE(p.fits, "too many pixels");
  const MpBn bn = mp_bn(mean, invstd, mscale, mshift, ws);
  if (g) pool_bwd<MP_RED>(dtype, dy, idx, g, H, W, C, p, y, bn, s);
  else pool_bwd<MP_RED_ONLY>(dtype, dy, idx, g, H, W, C, p, y, bn, s);
  VCG_LAUNCH_CHECK();
  finalize(ws, (int)stream_grid(p.TVin), C, sum_g, sum_gx, dgamma, dbeta, 1, s);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

// The sums of vcg_maxpool_bwd_bn (g == NULL) from the pooled activation mp [N][OH][OW][C] (the fused stem's
// vcg_bn_relu_maxpool output) instead of the pre-pool y: see maxpool_bn_sums_pooled_kernel. idx (the forward's argmax
// bytes) and the pre-pool y [N][H][W][C] are read only for degenerate channels (zero or tiny BN weight).
VCG_API int vcg_maxpool_bwd_bn_sums_pooled(int dtype, const void* dy, const void* mp, const unsigned char* idx,
                                           const void* y, int N, int H, int W, int C, const float* mean,
                                           const float* invstd, const float* mscale, const float* mshift, float* ws,
                                           long long ws_bytes, float* sum_g, float* sum_gx, float* dgamma,
                                           float* dbeta, hipStream_t s) {
  VCG_EW_SHAPE(VN, dtype, C, 256, C_VEC_MSG);
  VCG_REQUIRE(dy && mp && idx && y && mean && invstd && mscale && mshift && sum_g && sum_gx, "BN arguments required");
  VCG_REQUIRE(ws_bytes >= vcg_maxpool_bwd_bn_ws_bytes(C), "workspace too small");
  const PoolGeo p = pool_geo(N, H, W, C, VN);
  if (p.TVout == 0) return VCG_OK;
  const unsigned nb = stream_grid(p.TVout);
  const MpBn bn = mp_bn(mean, invstd, mscale, mshift, ws);
  const long long npix = (long long)N * p.OH * p.OW;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(maxpool_bn_sums_pooled_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)dy, (const T*)mp, p.TVout,
                       p.lcpr, bn);
    hipLaunchKernelGGL(maxpool_bn_sums_degen_kernel<T>, dim3(C), dim3(256), 0, s, (const T*)dy, (const T*)mp, idx,
                       (const T*)y, H, W, p.OH, p.OW, npix, C, bn, (int)nb);
  });
  VCG_LAUNCH_CHECK();
  finalize(ws, (int)nb + 1, C, sum_g, sum_gx, dgamma, dbeta, 1, s);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

// The stem's BatchNorm backward apply fused with the max-pool backward: dx = bn_bwd_apply(g) with g =
// maxpool_bwd(dy) masked by the forward ReLU and rounded to the storage type (the value vcg_maxpool_bwd_bn
// would store), sums from vcg_maxpool_bwd_bn(g = NULL). Equals vcg_maxpool_bwd_bn + vcg_bn_bwd_apply (mask
// mode 0) on that g, without the g round trip through HBM.
VCG_API int vcg_maxpool_bwd_bn_apply(int dtype, const void* dy, const unsigned char* idx, void* dx, int N, int H,
                                     int W, int C, const void* y, const float* mean, const float* invstd,
                                     const float* mscale, const float* mshift, const float* gamma, const float* sum_g,
                                     const float* sum_gx, long long count, int train_stats, hipStream_t s) {
  VCG_EW_SHAPE(VN, dtype, C, 256, C_VEC_MSG);
  VCG_REQUIRE(y && mean && invstd && mscale && mshift && sum_g && sum_gx && count > 0, "BN arguments required");
  const PoolGeo p = pool_geo(N, H, W, C, VN);
  VCG_REQUIRE(p.fits, "too many pixels");
  MpBn bn = mp_bn(mean, invstd, mscale, mshift, nullptr);
  bn.b.gamma = gamma; bn.b.sum_g = sum_g; bn.b.sum_gx = sum_gx; bn.inv_count = 1.f / (float)count; bn.train = train_stats;
  pool_bwd<MP_APPLY>(dtype, dy, idx, dx, H, W, C, p, y, bn, s);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

// The stem's BatchNorm + ReLU fused into the max-pool: out / idx = maxpool(relu(fma(y, scale, shift))) with the
// activation rounded to the storage type first (the values and argmax of vcg_bn_apply then vcg_maxpool_fwd).
VCG_API int vcg_bn_relu_maxpool(int dtype, const void* y, const float* scale, const float* shift, void* out,
                                unsigned char* idx, int N, int H, int W, int C, hipStream_t s) {
  VCG_EW_SHAPE(VN, dtype, C, 256, C_VEC_MSG);
  VCG_REQUIRE(scale && shift, "scale / shift required");
  const PoolGeo p = pool_geo(N, H, W, C, VN);
  VCG_REQUIRE(p.fits, "too many pixels");
  if (dtype == VCG_BF16) {  // two outputs per thread (maxpool_fwd2_kernel)
    const int OW2 = (p.OW + 1) / 2;
    const long long TV2 = (long long)N * p.OH * OW2 * (C / VN);
    hipLaunchKernelGGL((maxpool_fwd2_kernel<bf16_t, true>), dim3(blocks_for(TV2, 256)), dim3(256), 0, s,
                       (const bf16_t*)y, (bf16_t*)out, idx, H, W, C, p.OH, p.OW, p.lcpr, TV2, make_fastdiv(OW2),
                       make_fastdiv(p.OH), scale, shift);
  } else {
    hipLaunchKernelGGL((maxpool_fwd_kernel<float, true>), dim3(blocks_for(p.TVout, 256)), dim3(256), 0, s,
                       (const float*)y, (float*)out, idx, H, W, C, p.OH, p.OW, p.lcpr, p.TVout, make_fastdiv(p.OW),
                       make_fastdiv(p.OH), scale, shift);
  }
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_tsm_unshift_add(int dtype, const void* dshift, const void* other, const unsigned char* other_bits,
                                void* dx, long long NT, int T, long long HW, int C, int fold, hipStream_t s) {
  constexpr const char* msg = "C / fold must be multiples of the vector width";
  VCG_EW_SHAPE(VN, dtype, C, ANY_CPR, msg);
  VCG_REQUIRE(fold % VN == 0, msg);
  const long long TV = NT * HW * C / VN;
  VCG_REQUIRE(TV < (1LL << 31), "tensor too large for 32-bit vector indices");
  const int lcpr = ilog2i(C / VN);
  const unsigned g = stream_grid(TV);
  const unsigned row_vecs = (unsigned)(HW * C / VN);
  by_dtype(dtype, [&](auto t) {
    using E = decltype(t);
    auto go = [&](auto O, auto B) {
      hipLaunchKernelGGL((tsm_unshift_add_kernel<E, decltype(O)::value, decltype(B)::value>), dim3(g), dim3(256), 0, s,
                         (const E*)dshift, (const E*)other, other_bits, (E*)dx, (unsigned)TV, lcpr, row_vecs, T,
                         fold / VN);
    };
    if (!other) go(no, no);
    else if (!other_bits) go(yes, no);
    else go(yes, yes);
  });
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}
