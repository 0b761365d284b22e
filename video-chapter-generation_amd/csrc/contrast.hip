// Shot-contrastive (MoCo) pre-training of the language model (reference: model/lang/bert_hugface_constrast.py,
// trained by train_lang/pretrain_constrast_lang_model.py). What is specific to MoCo, as kernels:
//
//   momentum_kernel          k = k m + q (1 - m) over the key encoder's whole span of the flat parameter buffer in ONE
//                            launch (the reference loops over 199 parameter pairs, :39-40), bit for bit torch's
//                            expression (two rounded products, one rounded sum, no FMA); the bf16 shadow of the key
//                            encoder is written in the same pass, as adamw_kernel does for the step.
//   l2norm_fwd / _bwd        F.normalize(x, dim=1), eps 1e-12, fp32 statistics.
//   select_kernel            argmax over a query's C candidates of the cosine to the query (:128-132), the candidates'
//                            norms folded in: nothing normalised [B C, H] is written. Lowest index on equal values.
//   enqueue / rebuild        the queue lives twice: `queue` [H][K] fp32 (the reference's buffer, for state dicts) and
//                            `queue_km` [K][H] in the compute dtype, key-major: the operand of the tile kernel and of
//                            the gradient GEMM. enqueue writes the N new keys into both at the DEVICE pointer and a
//                            second one-thread launch advances it (no host round trip); rebuild is transpose + cast.
//   infonce_tile_kernel      the fused InfoNCE: Z = q queue_km^T / T in 64 x 128 tiles, bf16 MFMA 16x16x32, fp32
//                            accumulators -- the main loop of mlm_head.hip's mlm_tile_kernel, written again here so
//                            that file stays as it is. LOSS keeps per-row online (max, sum, argmax) partials per split
//                            of the key axis; DZ writes P / (N T) in bf16 for the gradient GEMM; LOGITS stores fp32.
//                            The positive logit q . k / T (one per row, not a shared column) comes from rowdot_kernel
//                            and joins in infonce_finalize_rows_kernel as column 0 (so it wins an exact tie).
//   fixed reduction trees, no atomics: bit-identical run to run.
//
// The fp32 parity mode forms the logits with vcg_gemm; infonce_rows_f32_kernel / infonce_dz_f32_kernel reduce them.
#include "common.h"

#include <math.h>

namespace vcg {

namespace {

constexpr int NCE_BR = 64;           // rows per tile
constexpr int NCE_BV = 128;          // keys per tile
constexpr int NCE_BK = 64;           // k per stage
constexpr int NCE_LD = NCE_BK + 8;   // LDS row stride in bf16 (144 B)
constexpr int NCE_MAX_H = 4096;
constexpr int NCE_TARGET_WGS = 512;  // workgroups wanted from row blocks x splits (256 CUs, two per CU)
constexpr int SEL_MAX_C = 64;

enum { NCE_LOSS = 0, NCE_DZ = 1, NCE_LOGITS = 2 };

// ------------------------------------------------------------------------------------------------ momentum update
// (contraction off for this expression: HIP's __fmul_rn / __fadd_rn are plain operators, which -ffp-contract=fast fuses)
__device__ __forceinline__ float mom1(float k, float q, float m, float om) {
#pragma clang fp contract(off)
  const float a = k * m;
  const float b = q * om;
  return a + b;
}

__global__ __launch_bounds__(256) void momentum_kernel(float* __restrict__ k, const float* __restrict__ q, long long n,
                                                       float m, float om, bf16_t* __restrict__ shadow) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const bool aligned = ((reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(q)) & 15) == 0 &&
                       (reinterpret_cast<uintptr_t>(shadow) & 7) == 0;
  if (aligned) {
    // 16-B loads, 4 of each operand in flight per thread (as sumsq_part_kernel)
    const long long n4 = n >> 2;
    float4* k4 = reinterpret_cast<float4*>(k);
    const float4* q4 = reinterpret_cast<const float4*>(q);
    auto put = [&](long long i, float4 a, float4 b) {
      const float4 r = make_float4(mom1(a.x, b.x, m, om), mom1(a.y, b.y, m, om), mom1(a.z, b.z, m, om),
                                   mom1(a.w, b.w, m, om));
      k4[i] = r;
      if (shadow)
        *reinterpret_cast<uint2*>(shadow + 4 * i) =
            make_uint2((uint32_t)f2bf(r.x) | ((uint32_t)f2bf(r.y) << 16), (uint32_t)f2bf(r.z) | ((uint32_t)f2bf(r.w) << 16));
    };
    long long i = t0;
    for (; i + 3 * stride < n4; i += 4 * stride) {
      float4 a[4], b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[j] = k4[i + j * stride];
        b[j] = q4[i + j * stride];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) put(i + j * stride, a[j], b[j]);
    }
    for (; i < n4; i += stride) put(i, k4[i], q4[i]);
    for (long long j = 4 * n4 + t0; j < n; j += stride) {
      const float r = mom1(k[j], q[j], m, om);
      k[j] = r;
      if (shadow) shadow[j] = f2bf(r);
    }
  } else {
    for (long long i = t0; i < n; i += stride) {
      const float r = mom1(k[i], q[i], m, om);
      k[i] = r;
      if (shadow) shadow[i] = f2bf(r);
    }
  }
}

// ------------------------------------------------------------------------------------------------ normalisation
// one workgroup per row; y = x / max(||x||, eps); denom[row] = max(||x||, eps)
template <typename T>
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                         float* __restrict__ denom, int H, float eps) {
  __shared__ float red[16];
  const long long o = (long long)blockIdx.x * H;
  float s = 0.f;
  for (int h = threadIdx.x; h < H; h += 256) {
    const float v = to_f<T>(x[o + h]);
    s += v * v;
  }
  const float d = fmaxf(sqrtf(block_sum(s, red)), eps);
  for (int h = threadIdx.x; h < H; h += 256) y[o + h] = from_f<T>(to_f<T>(x[o + h]) / d);
  if (threadIdx.x == 0 && denom) denom[blockIdx.x] = d;
}

// dx = (g - y (y . g)) / denom with y = x / denom recomputed in fp32
template <typename T>
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ g, const T* __restrict__ x,
                                                         const float* __restrict__ denom, float* __restrict__ dx,
                                                         int H) {
  __shared__ float red[16];
  const long long o = (long long)blockIdx.x * H;
  const float d = denom[blockIdx.x];
  float s = 0.f;
  for (int h = threadIdx.x; h < H; h += 256) s += (to_f<T>(x[o + h]) / d) * g[o + h];
  const float yg = block_sum(s, red);
  for (int h = threadIdx.x; h < H; h += 256) dx[o + h] = (g[o + h] - (to_f<T>(x[o + h]) / d) * yg) / d;
}

// ------------------------------------------------------------------------------------------------ selection
// one workgroup per query b; wave w scores candidates w, w + 4, ...: score = q . c / max(||c||, eps) (the query's own
// norm is a positive factor common to a row's candidates). Thread 0 takes the first maximum.
template <typename T>
__global__ __launch_bounds__(256) void select_kernel(const T* __restrict__ q, const T* __restrict__ cand, int C, int H,
                                                     float eps, long long* __restrict__ k0) {
  __shared__ float score[SEL_MAX_C];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* qb = q + (long long)b * H;
  for (int c = wave; c < C; c += 4) {
    const T* cb = cand + ((long long)b * C + c) * H;
    float dot = 0.f, nn = 0.f;
    for (int h = lane; h < H; h += 64) {
      const float v = to_f<T>(cb[h]);
      dot += v * to_f<T>(qb[h]);
      nn += v * v;
    }
    dot = warp_sum(dot);
    nn = warp_sum(nn);
    if (lane == 0) score[c] = dot / fmaxf(sqrtf(nn), eps);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int best = 0;
    for (int c = 1; c < C; ++c)
      if (score[c] > score[best]) best = c;
    k0[b] = best;
  }
}

// ------------------------------------------------------------------------------------------------ queue
// keys [N][H] -> queue[h][ptr + n] (fp32, the value itself) and queue_km[ptr + n][h] (rounded to TQ). The pointer is
// read from the device; one that would write outside [0, K) writes nothing.
template <typename TK, typename TQ>
__global__ __launch_bounds__(256) void enqueue_kernel(const TK* __restrict__ keys, float* __restrict__ queue,
                                                      TQ* __restrict__ km, const long long* __restrict__ ptr, int N,
                                                      int K, int H) {
  const long long p = ptr[0];
  if (p < 0 || p + N > K) return;
  const long long total = (long long)N * H, stride = (long long)gridDim.x * 256;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += stride) {
    const int h = (int)(i / N), n = (int)(i % N);  // consecutive threads: consecutive columns of one queue row
    queue[(long long)h * K + p + n] = to_f<TK>(keys[(long long)n * H + h]);
  }
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += stride) {
    const int n = (int)(i / H), h = (int)(i % H);
    km[(p + n) * H + h] = from_f<TQ>(to_f<TK>(keys[i]));
  }
}

__global__ void advance_ptr_kernel(long long* ptr, int N, int K) {
  const long long p = ptr[0];
  if (p < 0 || p + N > K) return;
  ptr[0] = (p + N) % K;
}

// queue [H][K] fp32 -> km [K][H] in TQ, 64 x 64 tiles through LDS
template <typename TQ>
__global__ __launch_bounds__(256) void queue_rebuild_kernel(const float* __restrict__ queue, TQ* __restrict__ km, int K,
                                                            int H) {
  __shared__ float tile[64][65];
  const int k0 = blockIdx.x * 64, h0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) {
    const int h = h0 + r, k = k0 + tx;
    tile[r][tx] = (h < H && k < K) ? queue[(long long)h * K + k] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int k = k0 + r, h = h0 + tx;
    if (k < K && h < H) km[(long long)k * H + h] = from_f<TQ>(tile[tx][r]);
  }
}

// out[n * ldo] = scale * a[n] . b[n], one wave per row
template <typename T>
__global__ __launch_bounds__(256) void rowdot_kernel(const T* __restrict__ a, const T* __restrict__ b, int N, int H,
                                                     float scale, float* __restrict__ out, long long ldo) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const T* an = a + (long long)n * H;
  const T* bn = b + (long long)n * H;
  float s = 0.f;
  for (int h = lane; h < H; h += 64) s += to_f<T>(an[h]) * to_f<T>(bn[h]);
  s = warp_sum(s);
  if (lane == 0) out[(long long)n * ldo] = s * scale;
}

// ------------------------------------------------------------------------------------------------ InfoNCE
struct NceArgs {
  const bf16_t* X;  // q [N][H]
  const bf16_t* W;  // queue_km [K][H]
  int N, K, H, splits, tiles_per_split;
  float inv_T;
  float* part;       // NCE_LOSS: [4][splits][N] (max, sum, argmax value, argmax column bits; the column is 1 + key)
  const float* lse;  // NCE_DZ
  float scale;       // NCE_DZ: 1 / (N T)
  void* out;         // NCE_DZ: bf16 [N][ldo]; NCE_LOGITS: fp32 [N][ldo], the pointer at the first key column
  long long ldo;
  int kp;            // K rounded up to 8: the columns K .. kp - 1 are written as zeros
};

struct RowState {
  float m, s, av;
  int ai;
};

// a <- a merged with b over disjoint column sets; symmetric in (a, b) bit for bit (mlm_head.hip's state_merge)
__device__ __forceinline__ void state_merge(RowState& a, const RowState& b) {
  const float M = fmaxf(a.m, b.m);
  if (M > -INFINITY) {
    const float sa = a.m > -INFINITY ? a.s * expf(a.m - M) : 0.f;
    const float sb = b.m > -INFINITY ? b.s * expf(b.m - M) : 0.f;
    a.s = sa + sb;
    a.m = M;
  }
  if (b.ai >= 0 && (a.ai < 0 || b.av > a.av || (b.av == a.av && b.ai < a.ai))) {
    a.av = b.av;
    a.ai = b.ai;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void infonce_tile_kernel(NceArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t sX[NCE_BR * NCE_LD];
  __shared__ __attribute__((aligned(16))) bf16_t sW[NCE_BV * NCE_LD];
  __shared__ float sred[MODE == NCE_LOSS ? 16 * NCE_BR * 4 : 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int r0 = blockIdx.x * NCE_BR;
  const int ntv = (a.K + NCE_BV - 1) / NCE_BV;
  const int vt0 = blockIdx.y * a.tiles_per_split;
  const int vt1 = min(vt0 + a.tiles_per_split, ntv);
  const int nk = (a.H + NCE_BK - 1) / NCE_BK;

  // this thread's 16-B chunks of the X tile (2) and of the W tile (4): row = chunk / 8, k = 8 (chunk % 8)
  const bf16_t* xp[2];
  int xo[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = tid + j * 256, row = c >> 3;
    xo[j] = row * NCE_LD + (c & 7) * 8;
    const int r = r0 + row;
    xp[j] = r < a.N ? a.X + (long long)r * a.H + (c & 7) * 8 : nullptr;
  }

  float lse[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + i * 16 + li;
    lse[i] = 0.f;
    if constexpr (MODE == NCE_DZ)
      if (r < a.N) lse[i] = a.lse[r];
  }

  RowState st[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) st[i] = RowState{-INFINITY, 0.f, -INFINITY, -1};

  for (int vt = vt0; vt < vt1; ++vt) {
    const int v0 = vt * NCE_BV;
    const bf16_t* wp[4];
    int wo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = tid + j * 256, row = c >> 3;
      wo[j] = row * NCE_LD + (c & 7) * 8;
      const int v = v0 + row;
      wp[j] = v < a.K ? a.W + (long long)v * a.H + (c & 7) * 8 : nullptr;
    }
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int f = 0; f < 2; ++f) acc[i][f] = f32x4{0.f, 0.f, 0.f, 0.f};

    uint4 rx[2], rw[4];
    auto fetch = [&](int k0) {
      const int kc = k0 + (tid & 7) * 8;  // (H % 8 == 0: a chunk is inside the row or past it)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        rx[j] = (xp[j] && kc < a.H) ? *reinterpret_cast<const uint4*>(xp[j] + k0) : make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        rw[j] = (wp[j] && kc < a.H) ? *reinterpret_cast<const uint4*>(wp[j] + k0) : make_uint4(0, 0, 0, 0);
    };
    fetch(0);
    for (int kt = 0; kt < nk; ++kt) {
      __syncthreads();  // the previous stage's fragment reads are done
#pragma unroll
      for (int j = 0; j < 2; ++j) *reinterpret_cast<uint4*>(sX + xo[j]) = rx[j];
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<uint4*>(sW + wo[j]) = rw[j];
      __syncthreads();
      if (kt + 1 < nk) fetch((kt + 1) * NCE_BK);  // in flight during the MFMAs
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        s16x8 xf[4], wf[2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          xf[i] = *reinterpret_cast<const s16x8*>(sX + (i * 16 + li) * NCE_LD + s2 * 32 + g * 8);
#pragma unroll
        for (int f = 0; f < 2; ++f)
          wf[f] = *reinterpret_cast<const s16x8*>(sW + (wave * 32 + f * 16 + li) * NCE_LD + s2 * 32 + g * 8);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int f = 0; f < 2; ++f)
            acc[i][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[f], xf[i], acc[i][f], 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int f = 0; f < 2; ++f) acc[i][f] *= a.inv_T;

    // acc[i][f][r] = z(row r0 + 16 i + li, key v0 + 32 wave + 16 f + 4 g + r)
    const int vb = v0 + wave * 32 + g * 4;
    if constexpr (MODE == NCE_LOSS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float tmax = -INFINITY;
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int v = vb + f * 16 + r;
            if (v < a.K) {
              const float z = acc[i][f][r];
              tmax = fmaxf(tmax, z);
              if (z > st[i].av || st[i].ai < 0) {  // (keys come in ascending order: the first maximum stays)
                st[i].av = z;
                st[i].ai = 1 + v;
              }
            }
          }
        if (tmax > -INFINITY) {
          const float mn = fmaxf(st[i].m, tmax);
          float s = st[i].m > -INFINITY ? st[i].s * __expf(st[i].m - mn) : 0.f;
#pragma unroll
          for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (vb + f * 16 + r < a.K) s += __expf(acc[i][f][r] - mn);
          st[i].m = mn;
          st[i].s = s;
        }
      }
    } else if constexpr (MODE == NCE_DZ) {
      bf16_t* dz = reinterpret_cast<bf16_t*>(a.out);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = r0 + i * 16 + li;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const int v4 = vb + f * 16;
          if (row < a.N && v4 < a.kp) {  // (kp % 8 == 0, v4 % 4 == 0: the 4 columns are inside the padded row)
            uint32_t w[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              bf16_t b2[2];
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                const int r = 2 * h + e, v = v4 + r;
                b2[e] = f2bf(v < a.K ? __expf(acc[i][f][r] - lse[i]) * a.scale : 0.f);
              }
              w[h] = (uint32_t)b2[0] | ((uint32_t)b2[1] << 16);
            }
            *reinterpret_cast<uint2*>(dz + (long long)row * a.ldo + v4) = make_uint2(w[0], w[1]);
          }
        }
      }
    } else {
      float* zo = reinterpret_cast<float*>(a.out);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = r0 + i * 16 + li;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const int v4 = vb + f * 16;
          if (row < a.N && v4 < a.kp)  // (columns K .. kp - 1 are zeros: their W rows were zero-filled)
            *reinterpret_cast<float4*>(zo + (long long)row * a.ldo + v4) =
                make_float4(acc[i][f][0], acc[i][f][1], acc[i][f][2], acc[i][f][3]);
        }
      }
    }
  }

  if constexpr (MODE == NCE_LOSS) {
    // the 16 states of a row (4 waves x 4 lane groups), merged in that order by one thread per row
    const int src = wave * 4 + g;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float* d = sred + (src * NCE_BR + i * 16 + li) * 4;
      d[0] = st[i].m;
      d[1] = st[i].s;
      d[2] = st[i].av;
      d[3] = __int_as_float(st[i].ai);
    }
    __syncthreads();
    if (tid < NCE_BR && r0 + tid < a.N) {
      RowState t{-INFINITY, 0.f, -INFINITY, -1};
      for (int q = 0; q < 16; ++q) {
        const float* d = sred + (q * NCE_BR + tid) * 4;
        state_merge(t, RowState{d[0], d[1], d[2], __float_as_int(d[3])});
      }
      const long long SR = (long long)a.splits * a.N, o = (long long)blockIdx.y * a.N + r0 + tid;
      a.part[o] = t.m;
      a.part[SR + o] = t.s;
      a.part[2 * SR + o] = t.av;
      a.part[3 * SR + o] = __int_as_float(t.ai);
    }
  }
}

// One wave per row: lane l merges splits l, l + 64, ... in order, a butterfly over the lanes (state_merge is symmetric),
// then the positive logit as column 0. rowres [2][N]: the row's loss and whether its argmax is column 0.
__global__ __launch_bounds__(256) void infonce_finalize_rows_kernel(const float* part, int splits, int N,
                                                                    const float* lpos, float* lse, float* row_loss,
                                                                    float* omp0, float* rowres) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= N) return;
  const long long SR = (long long)splits * N;
  RowState t{-INFINITY, 0.f, -INFINITY, -1};
  for (int s = lane; s < splits; s += 64) {
    const long long o = (long long)s * N + r;
    state_merge(t, RowState{part[o], part[SR + o], part[2 * SR + o], __float_as_int(part[3 * SR + o])});
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    RowState u{__shfl_xor(t.m, o, 64), __shfl_xor(t.s, o, 64), __shfl_xor(t.av, o, 64), __shfl_xor(t.ai, o, 64)};
    state_merge(t, u);
  }
  if (lane == 0) {
    const float zp = lpos[r];
    if (omp0) {
      // 1 - p0 = (sum over the keys) / (that + e^zp), formed without the cancellation of 1 - exp(zp - lse): where the
      // positive wins, p0 is within 1e-2 of 1 and lse (~13) carries half an ulp of 1e-6
      const float M = fmaxf(t.m, zp);
      const float sn = t.m > -INFINITY ? t.s * expf(t.m - M) : 0.f;
      omp0[r] = sn / (sn + expf(zp - M));
    }
    state_merge(t, RowState{zp, 1.f, zp, 0});
    const float l = t.m + logf(t.s), rl = l - zp;
    if (lse) lse[r] = l;
    if (row_loss) row_loss[r] = rl;
    rowres[r] = rl;
    rowres[N + r] = t.ai == 0 ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(256) void infonce_mean_kernel(const float* rowres, int N, float* mean_loss,
                                                           long long* n_correct) {
  __shared__ double ssum[256];
  __shared__ int scnt[256];
  const int tid = threadIdx.x;
  double lsum = 0.0;
  int cnt = 0;
  for (int r = tid; r < N; r += 256) {
    lsum += (double)rowres[r];
    cnt += rowres[N + r] != 0.f ? 1 : 0;
  }
  ssum[tid] = lsum;
  scnt[tid] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      ssum[tid] += ssum[tid + o];
      scnt[tid] += scnt[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (mean_loss) mean_loss[0] = (float)(ssum[0] / (double)N);
    if (n_correct) n_correct[0] = scnt[0];
  }
}

// fp32 key logits z [N][ldz] (already divided by T) -> the partials of one split (one workgroup per row)
__global__ __launch_bounds__(256) void infonce_rows_f32_kernel(const float* z, long long ldz, int N, int K,
                                                               float* part) {
  __shared__ float sred[256 * 4];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* zr = z + (long long)r * ldz;
  RowState t{-INFINITY, 0.f, -INFINITY, -1};
  for (int v = tid; v < K; v += 256) {
    const float x = zr[v];
    if (x > t.av || t.ai < 0) {
      t.av = x;
      t.ai = 1 + v;
    }
    const float mn = fmaxf(t.m, x);
    t.s = (t.m > -INFINITY ? t.s * expf(t.m - mn) : 0.f) + expf(x - mn);
    t.m = mn;
  }
  float* d = sred + tid * 4;
  d[0] = t.m;
  d[1] = t.s;
  d[2] = t.av;
  d[3] = __int_as_float(t.ai);
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {  // fixed tree
    if (tid < o) {
      float* p = sred + tid * 4;
      const float* q = sred + (tid + o) * 4;
      RowState x{p[0], p[1], p[2], __float_as_int(p[3])};
      state_merge(x, RowState{q[0], q[1], q[2], __float_as_int(q[3])});
      p[0] = x.m;
      p[1] = x.s;
      p[2] = x.av;
      p[3] = __int_as_float(x.ai);
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[r] = sred[0];
    part[(long long)N + r] = sred[1];
    part[2LL * N + r] = sred[2];
    part[3LL * N + r] = sred[3];
  }
}

// in place: z[r][v] = exp(z - lse[r]) * scale for v < K, 0 for K <= v < kp
__global__ __launch_bounds__(256) void infonce_dz_f32_kernel(float* z, long long ldz, const float* lse, float scale,
                                                             int K, int kp) {
  const int r = blockIdx.y;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= kp) return;
  float* p = z + (long long)r * ldz + v;
  *p = v < K ? expf(*p - lse[r]) * scale : 0.f;
}

// dq[n][h] += (p0 - 1) * scale * k[n][h], omp0 = 1 - p0
template <typename T>
__global__ __launch_bounds__(256) void infonce_dq_pos_kernel(float* dq, const T* __restrict__ k, const float* omp0,
                                                             float scale, int N, int H) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= (long long)N * H) return;
  const int n = (int)(i / H);
  dq[i] -= omp0[n] * scale * to_f<T>(k[i]);
}

// splits of the key axis for N rows: a pure function of the shape (the reduction order follows it)
void nce_split(int N, int K, int* splits, int* tps) {
  const int ntv = (K + NCE_BV - 1) / NCE_BV, nrb = (N + NCE_BR - 1) / NCE_BR;
  int s = (NCE_TARGET_WGS + nrb - 1) / nrb;
  s = s < 1 ? 1 : (s > ntv ? ntv : s);
  *tps = (ntv + s - 1) / s;
  *splits = (ntv + *tps - 1) / *tps;
}

// workspace: 4 floats per (split, row), then 2 per row (rowres)
long long nce_ws_floats(int splits, int N) { return (4LL * splits + 2) * N; }

int nce_shape_ok(int N, int K, int H) {
  if (N <= 0 || K <= 0 || H <= 0) {
    set_error("infonce: empty shape");
    return VCG_ERR_INVALID;
  }
  if (H % 8 != 0 || H > NCE_MAX_H) {
    set_error("infonce: H must be a multiple of 8, at most 4096");
    return VCG_ERR_UNSUPPORTED;
  }
  return VCG_OK;
}

void nce_finalize(float* ws, int splits, int N, const float* lpos, float* lse, float* row_loss, float* omp0,
                  float* mean_loss, long long* n_correct, hipStream_t stream) {
  float* rowres = ws + 4LL * splits * N;
  hipLaunchKernelGGL(infonce_finalize_rows_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, ws, splits, N, lpos, lse,
                     row_loss, omp0, rowres);
  hipLaunchKernelGGL(infonce_mean_kernel, dim3(1), dim3(256), 0, stream, rowres, N, mean_loss, n_correct);
}

NceArgs nce_args(const void* q, const void* km, int N, int K, int H, float inv_T) {
  NceArgs a{};
  a.X = reinterpret_cast<const bf16_t*>(q);
  a.W = reinterpret_cast<const bf16_t*>(km);
  a.N = N; a.K = K; a.H = H;
  a.inv_T = inv_T;
  a.kp = (K + 7) / 8 * 8;
  nce_split(N, K, &a.splits, &a.tiles_per_split);
  return a;
}

}  // namespace

}  // namespace vcg

using namespace vcg;

VCG_API int vcg_momentum_update(float* k, const float* q, long long n, float m, float one_minus_m, void* k_shadow,
                                hipStream_t stream) {
  VCG_REQUIRE(k && q, "null argument");
  VCG_REQUIRE(n > 0, "empty span");
  long long nb = (n + 1023) / 1024;
  nb = nb < 1 ? 1 : (nb > 4096 ? 4096 : nb);
  hipLaunchKernelGGL(momentum_kernel, dim3((unsigned)nb), dim3(256), 0, stream, k, q, n, m, one_minus_m,
                     reinterpret_cast<bf16_t*>(k_shadow));
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_l2norm_fwd(int dtype, const void* x, void* y, float* denom, int N, int H, float eps,
                           hipStream_t stream) {
  VCG_REQUIRE(x && y, "null argument");
  VCG_REQUIRE(N > 0 && H > 0, "empty shape");
  if (dtype == VCG_BF16)
    hipLaunchKernelGGL(l2norm_fwd_kernel<bf16_t>, dim3(N), dim3(256), 0, stream, (const bf16_t*)x, (bf16_t*)y, denom,
                       H, eps);
  else
    hipLaunchKernelGGL(l2norm_fwd_kernel<float>, dim3(N), dim3(256), 0, stream, (const float*)x, (float*)y, denom, H,
                       eps);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_l2norm_bwd(int dtype, const float* g, const void* x, const float* denom, float* dx, int N, int H,
                           hipStream_t stream) {
  VCG_REQUIRE(g && x && denom && dx, "null argument");
  VCG_REQUIRE(N > 0 && H > 0, "empty shape");
  if (dtype == VCG_BF16)
    hipLaunchKernelGGL(l2norm_bwd_kernel<bf16_t>, dim3(N), dim3(256), 0, stream, g, (const bf16_t*)x, denom, dx, H);
  else
    hipLaunchKernelGGL(l2norm_bwd_kernel<float>, dim3(N), dim3(256), 0, stream, g, (const float*)x, denom, dx, H);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_contrast_select(int dtype, const void* q, const void* cand, int B, int C, int H, float eps,
                                long long* k0, hipStream_t stream) {
  VCG_REQUIRE(q && cand && k0, "null argument");
  VCG_REQUIRE(B > 0 && C > 0 && H > 0, "empty shape");
  VCG_REQUIRE(C <= SEL_MAX_C, "at most 64 candidates per query");
  if (dtype == VCG_BF16)
    hipLaunchKernelGGL(select_kernel<bf16_t>, dim3(B), dim3(256), 0, stream, (const bf16_t*)q, (const bf16_t*)cand, C,
                       H, eps, k0);
  else
    hipLaunchKernelGGL(select_kernel<float>, dim3(B), dim3(256), 0, stream, (const float*)q, (const float*)cand, C, H,
                       eps, k0);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_queue_enqueue(int key_dtype, int km_dtype, const void* keys, float* queue, void* queue_km,
                              long long* queue_ptr, int N, int K, int H, hipStream_t stream) {
  VCG_REQUIRE(keys && queue && queue_km && queue_ptr, "null argument");
  VCG_REQUIRE(N > 0 && K > 0 && H > 0, "empty shape");
  VCG_REQUIRE(N <= K && K % N == 0, "the queue size K must be a multiple of the batch size");
  const long long total = (long long)N * H;
  const unsigned nb = (unsigned)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256);
#define VCG_ENQ(TK, TQ)                                                                                         \
  hipLaunchKernelGGL((enqueue_kernel<TK, TQ>), dim3(nb), dim3(256), 0, stream, (const TK*)keys, queue, (TQ*)queue_km, \
                     queue_ptr, N, K, H)
  if (key_dtype == VCG_BF16 && km_dtype == VCG_BF16) VCG_ENQ(bf16_t, bf16_t);
  else if (key_dtype == VCG_BF16) VCG_ENQ(bf16_t, float);
  else if (km_dtype == VCG_BF16) VCG_ENQ(float, bf16_t);
  else VCG_ENQ(float, float);
#undef VCG_ENQ
  VCG_LAUNCH_CHECK();
  hipLaunchKernelGGL(advance_ptr_kernel, dim3(1), dim3(1), 0, stream, queue_ptr, N, K);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_queue_rebuild(int km_dtype, const float* queue, void* queue_km, int K, int H, hipStream_t stream) {
  VCG_REQUIRE(queue && queue_km, "null argument");
  VCG_REQUIRE(K > 0 && H > 0, "empty shape");
  const dim3 grid((K + 63) / 64, (H + 63) / 64);
  VCG_REQUIRE(grid.y <= 65535, "H too large");
  if (km_dtype == VCG_BF16)
    hipLaunchKernelGGL(queue_rebuild_kernel<bf16_t>, grid, dim3(256), 0, stream, queue, (bf16_t*)queue_km, K, H);
  else
    hipLaunchKernelGGL(queue_rebuild_kernel<float>, grid, dim3(256), 0, stream, queue, (float*)queue_km, K, H);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_rowdot(int dtype, const void* a, const void* b, int N, int H, float scale, float* out, long long ldo,
                       hipStream_t stream) {
  VCG_REQUIRE(a && b && out, "null argument");
  VCG_REQUIRE(N > 0 && H > 0 && ldo >= 1, "bad shape");
  if (dtype == VCG_BF16)
    hipLaunchKernelGGL(rowdot_kernel<bf16_t>, dim3((N + 3) / 4), dim3(256), 0, stream, (const bf16_t*)a,
                       (const bf16_t*)b, N, H, scale, out, ldo);
  else
    hipLaunchKernelGGL(rowdot_kernel<float>, dim3((N + 3) / 4), dim3(256), 0, stream, (const float*)a, (const float*)b,
                       N, H, scale, out, ldo);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API long long vcg_infonce_ws_bytes(int N, int K, int H) {
  (void)H;
  if (N <= 0 || K <= 0) return 0;
  int splits, tps;
  nce_split(N, K, &splits, &tps);
  return nce_ws_floats(splits, N) * 4;
}

VCG_API int vcg_infonce_fwd(const void* q, const void* queue_km, const float* lpos, int N, int K, int H, float inv_T,
                            float* ws, long long ws_bytes, float* lse, float* row_loss, float* one_minus_p0,
                            float* mean_loss, long long* n_correct, hipStream_t stream) {
  if (int rc = nce_shape_ok(N, K, H)) return rc;
  VCG_REQUIRE(q && queue_km && lpos && ws, "null argument");
  VCG_REQUIRE((((uintptr_t)q | (uintptr_t)queue_km) & 15) == 0, "q and queue_km must be 16-B aligned");
  VCG_REQUIRE(ws_bytes >= vcg_infonce_ws_bytes(N, K, H), "workspace too small");
  NceArgs a = nce_args(q, queue_km, N, K, H, inv_T);
  a.part = ws;
  hipLaunchKernelGGL(infonce_tile_kernel<NCE_LOSS>, dim3((N + NCE_BR - 1) / NCE_BR, a.splits), dim3(256), 0, stream, a);
  nce_finalize(ws, a.splits, N, lpos, lse, row_loss, one_minus_p0, mean_loss, n_correct, stream);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_infonce_dz(const void* q, const void* queue_km, const float* lse, int N, int K, int H, float inv_T,
                           float scale, void* dZ, long long ldz, hipStream_t stream) {
  if (int rc = nce_shape_ok(N, K, H)) return rc;
  VCG_REQUIRE(q && queue_km && lse && dZ, "null argument");
  VCG_REQUIRE((((uintptr_t)q | (uintptr_t)queue_km | (uintptr_t)dZ) & 15) == 0, "q, queue_km and dZ must be 16-B aligned");
  VCG_REQUIRE(ldz == ((long long)K + 7) / 8 * 8, "ldz must be K rounded up to a multiple of 8");
  NceArgs a = nce_args(q, queue_km, N, K, H, inv_T);
  a.lse = lse;
  a.scale = scale;
  a.out = dZ;
  a.ldo = ldz;
  hipLaunchKernelGGL(infonce_tile_kernel<NCE_DZ>, dim3((N + NCE_BR - 1) / NCE_BR, a.splits), dim3(256), 0, stream, a);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_infonce_logits(const void* q, const void* queue_km, int N, int K, int H, float inv_T, float* key_logits,
                               long long ldz, hipStream_t stream) {
  if (int rc = nce_shape_ok(N, K, H)) return rc;
  VCG_REQUIRE(q && queue_km && key_logits, "null argument");
  VCG_REQUIRE((((uintptr_t)q | (uintptr_t)queue_km | (uintptr_t)key_logits) & 15) == 0, "16-B alignment");
  VCG_REQUIRE(ldz % 4 == 0 && ldz >= ((long long)K + 7) / 8 * 8, "ldz: a multiple of 4, at least K rounded up to 8");
  NceArgs a = nce_args(q, queue_km, N, K, H, inv_T);
  a.out = key_logits;
  a.ldo = ldz;
  hipLaunchKernelGGL(infonce_tile_kernel<NCE_LOGITS>, dim3((N + NCE_BR - 1) / NCE_BR, a.splits), dim3(256), 0, stream,
                     a);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_infonce_reduce_f32(const float* key_logits, long long ldz, const float* lpos, int N, int K, float* ws,
                                   long long ws_bytes, float* lse, float* row_loss, float* one_minus_p0,
                                   float* mean_loss, long long* n_correct, hipStream_t stream) {
  VCG_REQUIRE(key_logits && lpos && ws, "null argument");
  VCG_REQUIRE(N > 0 && K > 0 && ldz >= K, "bad shape");
  VCG_REQUIRE(ws_bytes >= nce_ws_floats(1, N) * 4, "workspace too small");
  hipLaunchKernelGGL(infonce_rows_f32_kernel, dim3(N), dim3(256), 0, stream, key_logits, ldz, N, K, ws);
  nce_finalize(ws, 1, N, lpos, lse, row_loss, one_minus_p0, mean_loss, n_correct, stream);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_infonce_dz_f32(float* key_logits, long long ldz, const float* lse, float scale, int N, int K,
                               hipStream_t stream) {
  VCG_REQUIRE(key_logits && lse, "null argument");
  const int kp = (K + 7) / 8 * 8;
  VCG_REQUIRE(N > 0 && K > 0 && ldz >= kp && N <= 65535, "bad shape");
  hipLaunchKernelGGL(infonce_dz_f32_kernel, dim3((kp + 255) / 256, N), dim3(256), 0, stream, key_logits, ldz, lse,
                     scale, K, kp);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_infonce_dq_pos(int dtype, float* dq, const void* k, const float* one_minus_p0, float scale, int N,
                               int H, hipStream_t stream) {
  VCG_REQUIRE(dq && k && one_minus_p0, "null argument");
  VCG_REQUIRE(N > 0 && H > 0, "empty shape");
  const unsigned nb = (unsigned)(((long long)N * H + 255) / 256);
  if (dtype == VCG_BF16)
    hipLaunchKernelGGL(infonce_dq_pos_kernel<bf16_t>, dim3(nb), dim3(256), 0, stream, dq, (const bf16_t*)k,
                       one_minus_p0, scale, N, H);
  else
    hipLaunchKernelGGL(infonce_dq_pos_kernel<float>, dim3(nb), dim3(256), 0, stream, dq, (const float*)k,
                       one_minus_p0, scale, N, H);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}
