// Masked-LM vocabulary head (reference: model/lang/bert_hugface.py:98-132 projects every position onto the vocabulary,
// softmaxes and only then gathers the masked rows for F.cross_entropy, pretrain_lang_model_hugface.py). Here only the
// R masked rows are projected, and the vocabulary axis is reduced on the fly by the row-softmax tile engine of
// softmax_tile.h (the tile product, the online softmax state, the partials and their merge are described there) under
// MlmPolicy: the rows are gathered from the hidden states, and a row's target logit travels with its state.
//
//   softmax_tile_kernel<MlmPolicy, .>  LOSS: one (max, sum, target logit, argmax) partial per (split, row); DZ: dZ =
//                                      (exp(z - lse) - onehot(target)) * dloss / R in bf16 as [R][ldz] (ldz = V rounded
//                                      up to 8); LOGITS: every row, fp32: the logits of the drop-in forward.
//   mlm_finalize_rows_kernel           a row's splits merged, then lse, lse - z_target and whether the argmax (lowest
//                                      index on equal values) is the target; softmax_mean_kernel: the mean, the count.
//
// The fp32 parity mode computes the masked rows' logits with vcg_gemm; softmax_rows_f32_kernel reduces them to the same
// partials (one split) for the same finalize kernel, and mlm_dz_f32_kernel turns them into dZ in place.
//
// seq_softmax_kernel: prob[b][l][v] = softmax over l (the reference's F.softmax(logits, dim=1) on [B, L, V],
// bert_hugface.py:114), one thread per (b, v), reads coalesced along v; L <= 64 is held in registers (one read).
#include "softmax_tile.h"

namespace vcg {

namespace {

struct MlmPolicy {
  static constexpr bool GATHER = true, SCALED = false, TARGET = true;
  static constexpr int COL0 = 0;
  static __device__ __forceinline__ float dz_scale(const TileArgs& a) { return a.dloss[0] / (float)a.R; }
  static __device__ __forceinline__ float dz(float z, float lse, bool is_target, float scale) {
    return (__expf(z - lse) - (is_target ? 1.f : 0.f)) * scale;
  }
};

// One wave per row. rowres [2][R]: the row's loss and whether its argmax is the target, for softmax_mean_kernel.
__global__ __launch_bounds__(256) void mlm_finalize_rows_kernel(const float* part, int splits, int R,
                                                                const long long* tgt, float* lse, float* row_loss,
                                                                float* rowres) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const RowState<true> t = merge_splits<true>(part, splits, R, r, lane);
  if (lane == 0) {
    const float l = t.m + logf(t.s), rl = l - t.zt;
    if (lse) lse[r] = l;
    if (row_loss) row_loss[r] = rl;
    rowres[r] = rl;
    rowres[R + r] = (long long)t.ai == tgt[r] ? 1.f : 0.f;
  }
}

// in place: z[r][v] = (exp(z - lse[r]) - onehot(target)) * dloss / R for v < V, 0 for V <= v < ldz
__global__ __launch_bounds__(256) void mlm_dz_f32_kernel(float* z, long long ldz, const float* lse,
                                                         const long long* tgt, const float* dloss, int R, int V) {
  const int r = blockIdx.y;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= ldz) return;
  float* p = z + (long long)r * ldz + v;
  const float scale = dloss[0] / (float)R;
  *p = v < V ? (expf(*p - lse[r]) - (v == tgt[r] ? 1.f : 0.f)) * scale : 0.f;
}

constexpr int SEQ_LREG = 64;

template <bool REG>
__global__ __launch_bounds__(256) void seq_softmax_kernel(const float* z, long long ldz, float* p, long long ldp, int L,
                                                          int V) {
  const int v = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (v >= V) return;
  const float* zb = z + (long long)b * L * ldz + v;
  float* pb = p + (long long)b * L * ldp + v;
  if constexpr (REG) {
    float x[SEQ_LREG];
    float m = -INFINITY;
#pragma unroll
    for (int l = 0; l < SEQ_LREG; ++l) {
      x[l] = l < L ? zb[(long long)l * ldz] : -INFINITY;
      m = fmaxf(m, x[l]);
    }
    float s = 0.f;
#pragma unroll
    for (int l = 0; l < SEQ_LREG; ++l) {
      x[l] = expf(x[l] - m);  // (exp(-inf) = 0 past L)
      s += x[l];
    }
    const float inv = 1.f / s;
#pragma unroll
    for (int l = 0; l < SEQ_LREG; ++l)
      if (l < L) pb[(long long)l * ldp] = x[l] * inv;
  } else {
    float m = -INFINITY, s = 0.f;
    for (int l = 0; l < L; ++l) {
      const float x = zb[(long long)l * ldz];
      const float mn = fmaxf(m, x);
      s = s * expf(m - mn) + expf(x - mn);
      m = mn;
    }
    const float inv = 1.f / s;
    for (int l = 0; l < L; ++l) pb[(long long)l * ldp] = expf(zb[(long long)l * ldz] - m) * inv;
  }
}

void mlm_finalize(float* ws, int splits, int R, const long long* tgt, float* lse, float* row_loss, float* mean_loss,
                  long long* n_correct, hipStream_t stream) {
  float* rowres = ws + 5LL * splits * R;
  hipLaunchKernelGGL(mlm_finalize_rows_kernel, dim3((R + 3) / 4), dim3(256), 0, stream, ws, splits, R, tgt, lse,
                     row_loss, rowres);
  hipLaunchKernelGGL(softmax_mean_kernel, dim3(1), dim3(256), 0, stream, rowres, R, mean_loss, n_correct);
}

TileArgs mlm_args(const void* hidden, int rows_total, const long long* rows, const void* W, const long long* targets,
                  int R, int V, int H) {
  TileArgs a = tile_args(hidden, W, R, V, H);
  a.rows_total = rows_total;
  a.rows = rows;
  a.tgt = targets;
  return a;
}

}  // namespace

}  // namespace vcg

using namespace vcg;

VCG_API long long vcg_mlm_loss_ws_bytes(int R, int V, int H) {
  (void)H;
  if (R <= 0 || V <= 0) return 0;
  int splits, tps;
  tile_split(R, V, &splits, &tps);
  return tile_ws_floats<MlmPolicy>(splits, R) * 4;
}

VCG_API int vcg_mlm_loss_fwd(const void* hidden, int rows_total, const long long* rows, const void* W,
                             const long long* targets, int R, int V, int H, float* ws, long long ws_bytes, float* lse,
                             float* row_loss, float* mean_loss, long long* n_correct, hipStream_t stream) {
  if (int rc = tile_shape_ok("mlm", R, V, H)) return rc;
  VCG_REQUIRE(hidden && W && targets && ws, "null argument");
  VCG_REQUIRE(rows_total > 0, "rows_total must be positive");
  VCG_REQUIRE((((uintptr_t)hidden | (uintptr_t)W) & 15) == 0, "hidden and W must be 16-B aligned");
  VCG_REQUIRE(ws_bytes >= vcg_mlm_loss_ws_bytes(R, V, H), "workspace too small");
  TileArgs a = mlm_args(hidden, rows_total, rows, W, targets, R, V, H);
  a.part = ws;
  tile_launch<MlmPolicy, TILE_LOSS>(a, stream);
  mlm_finalize(ws, a.splits, R, targets, lse, row_loss, mean_loss, n_correct, stream);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_mlm_loss_bwd(const void* hidden, int rows_total, const long long* rows, const void* W,
                             const long long* targets, const float* lse, const float* dloss, int R, int V, int H,
                             void* dZ, long long ldz, hipStream_t stream) {
  if (int rc = tile_shape_ok("mlm", R, V, H)) return rc;
  VCG_REQUIRE(hidden && W && targets && lse && dloss && dZ, "null argument");
  VCG_REQUIRE(rows_total > 0, "rows_total must be positive");
  VCG_REQUIRE((((uintptr_t)hidden | (uintptr_t)W | (uintptr_t)dZ) & 15) == 0, "hidden, W and dZ must be 16-B aligned");
  VCG_REQUIRE(ldz == ((long long)V + 7) / 8 * 8, "ldz must be V rounded up to a multiple of 8");
  TileArgs a = mlm_args(hidden, rows_total, rows, W, targets, R, V, H);
  a.lse = lse;
  a.dloss = dloss;
  a.out = dZ;
  a.ldo = ldz;
  tile_launch<MlmPolicy, TILE_DZ>(a, stream);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_mlm_logits(const void* hidden, int rows, const void* W, int V, int H, float* logits, long long ldz,
                           hipStream_t stream) {
  if (int rc = tile_shape_ok("mlm", rows, V, H)) return rc;
  VCG_REQUIRE(hidden && W && logits, "null argument");
  VCG_REQUIRE((((uintptr_t)hidden | (uintptr_t)W | (uintptr_t)logits) & 15) == 0, "16-B alignment");
  VCG_REQUIRE(ldz == ((long long)V + 7) / 8 * 8, "ldz must be V rounded up to a multiple of 8");
  TileArgs a = mlm_args(hidden, rows, nullptr, W, nullptr, rows, V, H);
  a.out = logits;
  a.ldo = ldz;
  tile_launch<MlmPolicy, TILE_LOGITS>(a, stream);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_mlm_reduce_f32(const float* logits, long long ldz, const long long* targets, int R, int V, float* ws,
                               long long ws_bytes, float* lse, float* row_loss, float* mean_loss,
                               long long* n_correct, hipStream_t stream) {
  VCG_REQUIRE(logits && targets && ws, "null argument");
  VCG_REQUIRE(R > 0 && V > 0 && ldz >= V, "bad shape");
  VCG_REQUIRE(ws_bytes >= tile_ws_floats<MlmPolicy>(1, R) * 4, "workspace too small");
  hipLaunchKernelGGL(softmax_rows_f32_kernel<MlmPolicy>, dim3(R), dim3(256), 0, stream, logits, ldz, targets, R, V, ws);
  mlm_finalize(ws, 1, R, targets, lse, row_loss, mean_loss, n_correct, stream);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_mlm_dz_f32(float* logits, long long ldz, const float* lse, const long long* targets,
                           const float* dloss, int R, int V, hipStream_t stream) {
  VCG_REQUIRE(logits && lse && targets && dloss, "null argument");
  VCG_REQUIRE(R > 0 && V > 0 && ldz >= V && R <= 65535, "bad shape");
  hipLaunchKernelGGL(mlm_dz_f32_kernel, dim3((unsigned)((ldz + 255) / 256), R), dim3(256), 0, stream, logits, ldz, lse,
                     targets, dloss, R, V);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_seq_softmax_fwd(const float* logits, long long ldz, float* prob, long long ldp, int B, int L, int V,
                                hipStream_t stream) {
  VCG_REQUIRE(logits && prob, "null argument");
  VCG_REQUIRE(B > 0 && B <= 65535 && L > 0 && V > 0 && ldz >= V && ldp >= V, "bad shape");
  const dim3 grid((V + 255) / 256, B);
  if (L <= SEQ_LREG)
    hipLaunchKernelGGL(seq_softmax_kernel<true>, grid, dim3(256), 0, stream, logits, ldz, prob, ldp, L, V);
  else
    hipLaunchKernelGGL(seq_softmax_kernel<false>, grid, dim3(256), 0, stream, logits, ldz, prob, ldp, L, V);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}
