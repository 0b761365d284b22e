// Listwise (ListNet) fine-tuning of the language model (reference: model/lang/bert_hugface_listnet.py:148-176, trained
// by train_lang/train_listwise.py): the slate loss and the 2-way boundary head over the pooled BERT output P [B S][H].
//
//   listnet_fwd_kernel       one workgroup per slate b (rows r0 = b S .. r0 + S - 1 of P). Its four waves form
//                            z_j = <P[r0], P[r0 + j]>, j = 1 .. S - 1 (16-byte loads, one wave per dot); wave 0 takes the
//                            softmax with the row maximum subtracted (P is a tanh output: |z| reaches H) and the slate's
//                            l_b = -sum_j t_j log(p_j + 1e-10). The same workgroup then scans `sel` for rows of ITS slate
//                            and runs the boundary head on them: y = W P[sel[m]] + bias, q = softmax(y), the row's
//                            cross-entropy logsumexp(y) - y[cls[m]]. One launch covers both losses.
//   listnet_finalize_kernel  one workgroup: surrogate = mean_b l_b, binary = mean_m ce_m, loss = their sum.
//   listnet_bwd_kernel       one workgroup per row of P writes that row of dP (fp32) exactly once: the slate term
//                            (row 0 of a slate: sum_j dz_j P[r0 + j]; row j: dz_j P[r0]) with
//                            dz_j = p_j (u_j - sum_k p_k u_k) g / B, u_j = -t_j / (p_j + 1e-10), plus W^T dy_m for every m
//                            with sel[m] equal to the row, in the order of m (duplicates add). Further workgroups of the
//                            same launch own 256 columns of dW each and add sum_m dy_m (x) P[sel[m]] in the order of m;
//                            the first of them adds db.
//   no atomics; every sum has a fixed order: bit-identical run to run.
#include "common.h"

namespace vcg {

namespace {

constexpr int LISTNET_MAX_S = 64;    // one lane of a wave per contrast clip
constexpr int LISTNET_MAX_H = 8192;  // (H a multiple of 8: 16-byte rows in both storage types)
constexpr float LISTNET_EPS = 1e-10f;

// <a, b> over H elements by one wave, 16-byte loads; every lane returns the sum
template <typename T>
__device__ __forceinline__ float wave_dot(const T* __restrict__ a, const T* __restrict__ b, int H, int lane) {
  constexpr int V = 16 / sizeof(T);
  float s = 0.f;
  for (int h = lane * V; h < H; h += 64 * V) {
    float x[V], y[V];
    load16<T>(a + h, x);
    load16<T>(b + h, y);
#pragma unroll
    for (int i = 0; i < V; ++i) s = fmaf(x[i], y[i], s);
  }
  return warp_sum(s);
}

// <w (fp32), x (T)> over H elements by one wave
template <typename T>
__device__ __forceinline__ float wave_dot_w(const float* __restrict__ w, const T* __restrict__ x, int H, int lane) {
  constexpr int V = 16 / sizeof(T);
  float s = 0.f;
  for (int h = lane * V; h < H; h += 64 * V) {
    float xv[V];
    load16<T>(x + h, xv);
#pragma unroll
    for (int i = 0; i < V; i += 4) {
      const float4 wv = *reinterpret_cast<const float4*>(w + h + i);
      s = fmaf(wv.x, xv[i], s);
      s = fmaf(wv.y, xv[i + 1], s);
      s = fmaf(wv.z, xv[i + 2], s);
      s = fmaf(wv.w, xv[i + 3], s);
    }
  }
  return warp_sum(s);
}

// part [B + M]: the slates' l_b, then the selected rows' cross-entropies
template <typename T>
__global__ __launch_bounds__(256) void listnet_fwd_kernel(const T* __restrict__ P, const float* __restrict__ targets,
                                                          const long long* __restrict__ sel,
                                                          const long long* __restrict__ cls,
                                                          const float* __restrict__ W, const float* __restrict__ bias,
                                                          int B, int S, int H, int M, float* __restrict__ p_out,
                                                          float* __restrict__ logits, float* __restrict__ prob,
                                                          float* __restrict__ part) {
  __shared__ float zs[LISTNET_MAX_S];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = (long long)b * S;
  const T* pos = P + r0 * H;
  for (int j = 1 + wave; j < S; j += 4) {
    const float z = wave_dot<T>(pos, P + (r0 + j) * H, H, lane);
    if (lane == 0) zs[j - 1] = z;
  }
  __syncthreads();
  if (wave == 0) {
    const bool on = lane < S - 1;
    const float z = on ? zs[lane] : -INFINITY;
    const float mx = warp_max(z);
    const float e = on ? expf(z - mx) : 0.f;
    const float p = e / warp_sum(e);
    float term = 0.f;
    if (on) {
      p_out[(long long)b * (S - 1) + lane] = p;
      term = targets[r0 + 1 + lane] * logf(p + LISTNET_EPS);
    }
    term = warp_sum(term);
    if (lane == 0) part[b] = -term;
  }
  // the boundary head on the selected rows of this slate
  for (int m = wave; m < M; m += 4) {
    const long long r = sel[m];
    if (r < r0 || r >= r0 + S) continue;  // (wave-uniform)
    const T* x = P + r * H;
    const float y0 = wave_dot_w<T>(W, x, H, lane) + bias[0];
    const float y1 = wave_dot_w<T>(W + H, x, H, lane) + bias[1];
    if (lane == 0) {
      const float mx = fmaxf(y0, y1);
      const float lse = mx + logf(expf(y0 - mx) + expf(y1 - mx));
      logits[2 * m] = y0;
      logits[2 * m + 1] = y1;
      prob[2 * m] = expf(y0 - lse);
      prob[2 * m + 1] = expf(y1 - lse);
      part[B + m] = lse - (cls[m] == 1 ? y1 : y0);
    }
  }
}

// out[0] = loss, out[1] = surrogate, out[2] = binary
__global__ __launch_bounds__(256) void listnet_finalize_kernel(const float* __restrict__ part, int B, int M,
                                                               float* __restrict__ out) {
  __shared__ float red[16];
  float s = 0.f, c = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) s += part[i];
  for (int i = threadIdx.x; i < M; i += 256) c += part[B + i];
  const float sur = block_sum(s, red) / (float)B;
  const float bin = block_sum(c, red) / (float)M;
  if (threadIdx.x == 0) {
    out[0] = sur + bin;
    out[1] = sur;
    out[2] = bin;
  }
}

// dy_m[c] = (q_m[c] - onehot(cls[m])[c]) * gm, gm = g / M
__device__ __forceinline__ void head_dy(const float* __restrict__ prob, const long long* __restrict__ cls, int m,
                                        float gm, float& dy0, float& dy1) {
  const bool one = cls[m] == 1;
  dy0 = (prob[2 * m] - (one ? 0.f : 1.f)) * gm;
  dy1 = (prob[2 * m + 1] - (one ? 1.f : 0.f)) * gm;
}

// workgroups [0, B S): one row of dP each; workgroups [B S, B S + ceil(H / 256)): 256 columns of dW each (dW != NULL)
template <typename T>
__global__ __launch_bounds__(256) void listnet_bwd_kernel(const T* __restrict__ P, const float* __restrict__ targets,
                                                          const long long* __restrict__ sel,
                                                          const long long* __restrict__ cls,
                                                          const float* __restrict__ W, const float* __restrict__ p_in,
                                                          const float* __restrict__ prob,
                                                          const float* __restrict__ dloss, int B, int S, int H, int M,
                                                          float* __restrict__ dP, float* __restrict__ dW,
                                                          float* __restrict__ db) {
  constexpr int V = 16 / sizeof(T);
  __shared__ float dzs[LISTNET_MAX_S];
  const float g = dloss[0];
  const float gm = g / (float)M;
  const long long rows = (long long)B * S;
  if ((long long)blockIdx.x >= rows) {
    // ---- dW / db, in the order of m
    const int h = ((int)(blockIdx.x - rows)) * 256 + threadIdx.x;
    if (h < H) {
      float a0 = 0.f, a1 = 0.f;
      for (int m = 0; m < M; ++m) {
        float dy0, dy1;
        head_dy(prob, cls, m, gm, dy0, dy1);
        const long long rm = sel[m];
        if (rm < 0 || rm >= rows) continue;  // (the host refuses such a row; nothing is read past P regardless)
        const float x = to_f<T>(P[rm * H + h]);
        a0 = fmaf(dy0, x, a0);
        a1 = fmaf(dy1, x, a1);
      }
      dW[h] += a0;
      dW[H + h] += a1;
    }
    if ((long long)blockIdx.x == rows && threadIdx.x == 0 && db) {
      float s0 = 0.f, s1 = 0.f;
      for (int m = 0; m < M; ++m) {
        float dy0, dy1;
        head_dy(prob, cls, m, gm, dy0, dy1);
        s0 += dy0;
        s1 += dy1;
      }
      db[0] += s0;
      db[1] += s1;
    }
    return;
  }
  const long long r = blockIdx.x;
  const int b = (int)(r / S), j = (int)(r % S), lane = threadIdx.x & 63;
  const long long r0 = (long long)b * S;
  if (threadIdx.x < 64) {
    const bool on = lane < S - 1;
    float p = 0.f, u = 0.f;
    if (on) {
      p = p_in[(long long)b * (S - 1) + lane];
      u = -targets[r0 + 1 + lane] / (p + LISTNET_EPS);
    }
    const float pu = warp_sum(p * u);
    if (on) dzs[lane] = p * (u - pu) * (g / (float)B);
  }
  __syncthreads();
  for (int h = threadIdx.x * V; h < H; h += 256 * V) {
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    if (j == 0) {
      for (int k = 1; k < S; ++k) {
        float x[V];
        load16<T>(P + (r0 + k) * H + h, x);
        const float dz = dzs[k - 1];
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = fmaf(dz, x[i], acc[i]);
      }
    } else {
      float x[V];
      load16<T>(P + r0 * H + h, x);
      const float dz = dzs[j - 1];
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] = dz * x[i];
    }
    for (int m = 0; m < M; ++m) {
      if (sel[m] != r) continue;  // (workgroup-uniform)
      float dy0, dy1;
      head_dy(prob, cls, m, gm, dy0, dy1);
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] += fmaf(W[h + i], dy0, W[H + h + i] * dy1);
    }
    float* o = dP + r * H + h;
#pragma unroll
    for (int i = 0; i < V; i += 4) *reinterpret_cast<float4*>(o + i) = make_float4(acc[i], acc[i + 1], acc[i + 2], acc[i + 3]);
  }
}

int listnet_shape_ok(const char* fn, int B, int S, int H, int M) {
  if (B < 1 || M < 1 || S < 2 || S > LISTNET_MAX_S || H < 8 || H > LISTNET_MAX_H || H % 8 != 0 ||
      (long long)B * S > 0x7fffffffLL) {
    set_error(std::string(fn) + ": needs B >= 1, M >= 1, 2 <= S <= 64, H a multiple of 8 in [8, 8192]; got B=" +
              std::to_string(B) + " S=" + std::to_string(S) + " H=" + std::to_string(H) + " M=" + std::to_string(M));
    return VCG_ERR_INVALID;
  }
  return VCG_OK;
}

}  // namespace

}  // namespace vcg

using namespace vcg;

VCG_API int vcg_listnet_max_slate(void) { return LISTNET_MAX_S; }
VCG_API int vcg_listnet_max_hidden(void) { return LISTNET_MAX_H; }

VCG_API int vcg_listnet_fwd(int dtype, const void* P, const float* targets, const long long* sel, const long long* cls,
                            const float* W, const float* bias, int B, int S, int H, int M, float* p, float* logits,
                            float* prob, float* part, float* loss3, hipStream_t stream) {
  if (int rc = listnet_shape_ok(__func__, B, S, H, M)) return rc;
  VCG_REQUIRE(P && targets && sel && cls && W && bias && p && logits && prob && part && loss3, "null argument");
  VCG_REQUIRE((((uintptr_t)P | (uintptr_t)W) & 15) == 0, "P and W must be 16-B aligned");
  if (dtype == VCG_BF16)
    hipLaunchKernelGGL(listnet_fwd_kernel<bf16_t>, dim3(B), dim3(256), 0, stream, (const bf16_t*)P, targets, sel, cls, W,
                       bias, B, S, H, M, p, logits, prob, part);
  else
    hipLaunchKernelGGL(listnet_fwd_kernel<float>, dim3(B), dim3(256), 0, stream, (const float*)P, targets, sel, cls, W,
                       bias, B, S, H, M, p, logits, prob, part);
  VCG_LAUNCH_CHECK();
  hipLaunchKernelGGL(listnet_finalize_kernel, dim3(1), dim3(256), 0, stream, part, B, M, loss3);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_listnet_bwd(int dtype, const void* P, const float* targets, const long long* sel, const long long* cls,
                            const float* W, const float* p, const float* prob, const float* dloss, int B, int S, int H,
                            int M, float* dP, float* dW, float* db, hipStream_t stream) {
  if (int rc = listnet_shape_ok(__func__, B, S, H, M)) return rc;
  VCG_REQUIRE(P && targets && sel && cls && W && p && prob && dloss && dP, "null argument");
  VCG_REQUIRE((dW == nullptr) == (db == nullptr), "dW and db go together");
  VCG_REQUIRE((((uintptr_t)P | (uintptr_t)W | (uintptr_t)dP) & 15) == 0, "P, W and dP must be 16-B aligned");
  const unsigned grid = (unsigned)((long long)B * S + (dW ? (H + 255) / 256 : 0));
  if (dtype == VCG_BF16)
    hipLaunchKernelGGL(listnet_bwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)P, targets, sel, cls,
                       W, p, prob, dloss, B, S, H, M, dP, dW, db);
  else
    hipLaunchKernelGGL(listnet_bwd_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)P, targets, sel, cls,
                       W, p, prob, dloss, B, S, H, M, dP, dW, db);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}
