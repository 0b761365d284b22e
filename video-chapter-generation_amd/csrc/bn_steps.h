// Device steps of the BatchNorm streaming kernels that more than one file uses (vision_ew.hip, stem_bwd.hip,
// bn_gram.hip): the batch-stat BN backward folded to an affine map of (g, y), and the per-block column-partials tail.
// The bit-exact tests between those files' kernels hold because each step is written here once.
#pragma once
#include "common.h"

namespace vcg {

// VN consecutive per-channel floats p[c0 .. c0 + VN) (16-B loads)
template <int VN>
__device__ __forceinline__ void load_params(const float* __restrict__ p, int c0, float (&out)[VN]) {
#pragma unroll
  for (int e = 0; e < VN; e += 4) {
    const float4 q = *reinterpret_cast<const float4*>(p + c0 + e);
    out[e] = q.x; out[e + 1] = q.y; out[e + 2] = q.z; out[e + 3] = q.w;
  }
}

// ------------------------------------------------------------------ BN backward coefficients
// dy = A g + B y + Cc per channel (the batch-stat BN backward as an affine map of the masked gradient g and input y):
//   A = gamma invstd, B = -A invstd sum_gx / N, Cc = -A sum_g / N - B mean; running statistics: dy = A g (A only).
// Cc's fma is explicit: of its two products either can be the fused one, and left to the compiler's contraction the
// choice changed from one instantiation (and one element of a chunk) to the next -- a last-bit difference between
// kernels that the tests compare with torch.equal. Every kernel fuses sum_g's product, fma(-A sum_g, 1 / N, -(B mean)).
// ALT fuses mean's instead, fma(-mean, B, -A sum_g / N): what bn_bwd_apply_dual_kernel has always computed for the
// last channel of its second BN's chunks (the compiler's choice there when the expression was contracted for it), kept
// so that a train step computes bit for bit what it did.
template <bool TRAIN = true, bool ALT = false>
__device__ __forceinline__ void bn_bwd_coef(float gamma, float is, float sgx, float sgg, float mu, float inv_count,
                                            float& A, float& Bc, float& Cc) {
  A = gamma * is;
  if (TRAIN) {
    Bc = -A * is * sgx * inv_count;
    Cc = ALT ? fmaf(-mu, Bc, -A * sgg * inv_count) : fmaf(-A * sgg, inv_count, -(Bc * mu));
  }
}
// the map's result for one element: train statistics, or running (A g)
__device__ __forceinline__ float bn_bwd_map(bool train, float A, float Bc, float Cc, float g, float y) {
  return train ? fmaf(A, g, fmaf(Bc, y, Cc)) : A * g;
}

struct BnBwdArgs {  // per-channel operands of the map (gamma == nullptr: 1)
  const float *mean, *invstd, *gamma, *sum_g, *sum_gx;
};
// the coefficients of the 16-B channel chunk at c0 (ALT_LAST: bn_bwd_coef's ALT form for the chunk's last channel)
template <int VN, bool TRAIN = true, bool ALT_LAST = false>
__device__ __forceinline__ void bn_bwd_coefs(const BnBwdArgs& b, int c0, float inv_count, float (&A)[VN],
                                             float (&Bc)[VN], float (&Cc)[VN]) {
  float is[VN], sgx[VN] = {}, sgg[VN] = {}, mu[VN] = {};
  load_params<VN>(b.invstd, c0, is);
  if (TRAIN) {
    load_params<VN>(b.sum_gx, c0, sgx);
    load_params<VN>(b.sum_g, c0, sgg);
    load_params<VN>(b.mean, c0, mu);
  }
#pragma unroll
  for (int e = 0; e < VN - 1; ++e)
    bn_bwd_coef<TRAIN>(b.gamma ? b.gamma[c0 + e] : 1.f, is[e], sgx[e], sgg[e], mu[e], inv_count, A[e], Bc[e], Cc[e]);
  constexpr int L = VN - 1;
  bn_bwd_coef<TRAIN, ALT_LAST>(b.gamma ? b.gamma[c0 + L] : 1.f, is[L], sgx[L], sgg[L], mu[L], inv_count, A[L], Bc[L],
                               Cc[L]);
}

// ------------------------------------------------------------------ column-partials tail
// Per-block column sums of a 256-thread block whose thread t owns the 16-B channel chunk t % cpr (cpr = C / VN a power
// of two <= 256) and holds PLANES sums s[plane][VN] per channel of it. The 256 / cpr threads of a chunk are combined
// through LDS in a fixed order (thread i adds red[ch], red[ch + cpr], ...: deterministic) and column c of plane p goes
// to dst[p * C + c]; plane 1 is multiplied by factor[c] first when factor is given.
// red: PLANES x 256 x LD floats of LDS (LD >= VN: the row stride).
template <int PLANES, int VN, int LD>
__device__ __forceinline__ void colpart_tail(float* red, const float (&s)[PLANES][VN], int cpr,
                                             const float* __restrict__ factor, float* __restrict__ dst) {
  const int tid = threadIdx.x, C = cpr * VN;
#pragma unroll
  for (int p = 0; p < PLANES; ++p)
#pragma unroll
    for (int e = 0; e < VN; ++e) red[(p * 256 + tid) * LD + e] = s[p][e];
  __syncthreads();
  for (int i = tid; i < PLANES * C; i += 256) {
    const int p = PLANES > 1 && i >= C, c = i - p * C;
    const int ch = c / VN, e = c - ch * VN;
    float acc = 0.f;
    for (int t = ch; t < 256; t += cpr) acc += red[(p * 256 + t) * LD + e];
    if (p && factor) acc *= factor[c];
    dst[i] = acc;
  }
}

}  // namespace vcg
