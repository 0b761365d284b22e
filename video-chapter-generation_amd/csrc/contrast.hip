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
//   softmax_tile_kernel      the fused InfoNCE: Z = q queue_km^T / T by the row-softmax tile engine of softmax_tile.h
//   <NcePolicy, .>           (shared with mlm_head.hip) under NcePolicy: no row gather, 1 / T applied to the
//                            accumulators, no target column, key v is column 1 + v. LOSS keeps per-row online (max,
//                            sum, argmax) partials per split of the key axis; DZ writes P / (N T) in bf16 for the
//                            gradient GEMM; LOGITS stores fp32. The positive logit q . k / T (one per row, not a
//                            shared column) comes from rowdot_kernel and joins in infonce_finalize_rows_kernel as
//                            column 0 (so it wins an exact tie).
//   fixed reduction trees, no atomics: bit-identical run to run.
//
// The fp32 parity mode forms the logits with vcg_gemm; softmax_rows_f32_kernel / infonce_dz_f32_kernel reduce them.
#include "softmax_tile.h"

namespace vcg {

namespace {

constexpr int SEL_MAX_C = 64;

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
struct NcePolicy {
  static constexpr bool GATHER = false, SCALED = true, TARGET = false;
  static constexpr int COL0 = 1;  // column 0 is the positive logit, joined in infonce_finalize_rows_kernel
  static __device__ __forceinline__ float dz_scale(const TileArgs& a) { return a.scale; }  // 1 / (N T)
  static __device__ __forceinline__ float dz(float z, float lse, bool, float scale) { return __expf(z - lse) * scale; }
};

// One wave per row: the splits merged, then the positive logit as column 0. rowres [2][N]: the row's loss and whether
// its argmax is column 0.
__global__ __launch_bounds__(256) void infonce_finalize_rows_kernel(const float* part, int splits, int N,
                                                                    const float* lpos, float* lse, float* row_loss,
                                                                    float* omp0, float* rowres) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= N) return;
  RowState<false> t = merge_splits<false>(part, splits, N, r, lane);
  if (lane == 0) {
    const float zp = lpos[r];
    if (omp0) {
      // 1 - p0 = (sum over the keys) / (that + e^zp), formed without the cancellation of 1 - exp(zp - lse): where the
      // positive wins, p0 is within 1e-2 of 1 and lse (~13) carries half an ulp of 1e-6
      const float M = fmaxf(t.m, zp);
      const float sn = t.m > -INFINITY ? t.s * expf(t.m - M) : 0.f;
      omp0[r] = sn / (sn + expf(zp - M));
    }
    RowState<false> pos;
    pos.m = zp; pos.s = 1.f; pos.av = zp; pos.ai = 0;
    state_merge(t, pos);
    const float l = t.m + logf(t.s), rl = l - zp;
    if (lse) lse[r] = l;
    if (row_loss) row_loss[r] = rl;
    rowres[r] = rl;
    rowres[N + r] = t.ai == 0 ? 1.f : 0.f;
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

void nce_finalize(float* ws, int splits, int N, const float* lpos, float* lse, float* row_loss, float* omp0,
                  float* mean_loss, long long* n_correct, hipStream_t stream) {
  float* rowres = ws + 4LL * splits * N;
  hipLaunchKernelGGL(infonce_finalize_rows_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, ws, splits, N, lpos, lse,
                     row_loss, omp0, rowres);
  hipLaunchKernelGGL(softmax_mean_kernel, dim3(1), dim3(256), 0, stream, rowres, N, mean_loss, n_correct);
}

TileArgs nce_args(const void* q, const void* km, int N, int K, int H, float inv_T) {
  TileArgs a = tile_args(q, km, N, K, H);
  a.zscale = inv_T;
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
  tile_split(N, K, &splits, &tps);
  return tile_ws_floats<NcePolicy>(splits, N) * 4;
}

VCG_API int vcg_infonce_fwd(const void* q, const void* queue_km, const float* lpos, int N, int K, int H, float inv_T,
                            float* ws, long long ws_bytes, float* lse, float* row_loss, float* one_minus_p0,
                            float* mean_loss, long long* n_correct, hipStream_t stream) {
  if (int rc = tile_shape_ok("infonce", N, K, H)) return rc;
  VCG_REQUIRE(q && queue_km && lpos && ws, "null argument");
  VCG_REQUIRE((((uintptr_t)q | (uintptr_t)queue_km) & 15) == 0, "q and queue_km must be 16-B aligned");
  VCG_REQUIRE(ws_bytes >= vcg_infonce_ws_bytes(N, K, H), "workspace too small");
  TileArgs a = nce_args(q, queue_km, N, K, H, inv_T);
  a.part = ws;
  tile_launch<NcePolicy, TILE_LOSS>(a, stream);
  nce_finalize(ws, a.splits, N, lpos, lse, row_loss, one_minus_p0, mean_loss, n_correct, stream);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_infonce_dz(const void* q, const void* queue_km, const float* lse, int N, int K, int H, float inv_T,
                           float scale, void* dZ, long long ldz, hipStream_t stream) {
  if (int rc = tile_shape_ok("infonce", N, K, H)) return rc;
  VCG_REQUIRE(q && queue_km && lse && dZ, "null argument");
  VCG_REQUIRE((((uintptr_t)q | (uintptr_t)queue_km | (uintptr_t)dZ) & 15) == 0, "q, queue_km and dZ must be 16-B aligned");
  VCG_REQUIRE(ldz == ((long long)K + 7) / 8 * 8, "ldz must be K rounded up to a multiple of 8");
  TileArgs a = nce_args(q, queue_km, N, K, H, inv_T);
  a.lse = lse;
  a.scale = scale;
  a.out = dZ;
  a.ldo = ldz;
  tile_launch<NcePolicy, TILE_DZ>(a, stream);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_infonce_logits(const void* q, const void* queue_km, int N, int K, int H, float inv_T, float* key_logits,
                               long long ldz, hipStream_t stream) {
  if (int rc = tile_shape_ok("infonce", N, K, H)) return rc;
  VCG_REQUIRE(q && queue_km && key_logits, "null argument");
  VCG_REQUIRE((((uintptr_t)q | (uintptr_t)queue_km | (uintptr_t)key_logits) & 15) == 0, "16-B alignment");
  VCG_REQUIRE(ldz % 4 == 0 && ldz >= ((long long)K + 7) / 8 * 8, "ldz: a multiple of 4, at least K rounded up to 8");
  TileArgs a = nce_args(q, queue_km, N, K, H, inv_T);
  a.out = key_logits;
  a.ldo = ldz;
  tile_launch<NcePolicy, TILE_LOGITS>(a, stream);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_infonce_reduce_f32(const float* key_logits, long long ldz, const float* lpos, int N, int K, float* ws,
                                   long long ws_bytes, float* lse, float* row_loss, float* one_minus_p0,
                                   float* mean_loss, long long* n_correct, hipStream_t stream) {
  VCG_REQUIRE(key_logits && lpos && ws, "null argument");
  VCG_REQUIRE(N > 0 && K > 0 && ldz >= K, "bad shape");
  VCG_REQUIRE(ws_bytes >= tile_ws_floats<NcePolicy>(1, N) * 4, "workspace too small");
  hipLaunchKernelGGL(softmax_rows_f32_kernel<NcePolicy>, dim3(N), dim3(256), 0, stream, key_logits, ldz, nullptr, N, K,
                     ws);
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
