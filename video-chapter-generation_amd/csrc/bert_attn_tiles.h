// Tile constants and MFMA fragment helpers shared by the fused BERT attention kernels (bert_attn.hip: L <= 128, one
// workgroup per (sequence, head); bert_attn_long.hip: 128 < L <= 512, 128 x 128 tiles with an online softmax).
#pragma once
#include "common.h"

namespace vcg {
namespace attn {

constexpr int LT = 128;    // query / key tile
constexpr int LMAX = 512;  // longest sequence of the tiled kernels (BertConfig.max_position_embeddings)
constexpr int DH = 64;     // head dim
constexpr int TP = 136;    // row pitch (elements) of the transposed / square LDS tiles: 272-B rows, conflict-free
                           // b64 / b128 fragment reads of 16 consecutive rows

__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

__device__ __forceinline__ uint32_t pack2(float a, float b) { return (uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16); }

__device__ __forceinline__ uint32_t half16(const uint4& v, int j) {
  const uint32_t w = (j >> 1) == 0 ? v.x : (j >> 1) == 1 ? v.y : (j >> 1) == 2 ? v.z : v.w;
  return (j & 1) ? (w >> 16) : (w & 0xffffu);
}

__device__ __forceinline__ s16x8 frag_rm(const bf16_t* t, int row, int chunk) {  // swizzled [rows][64] tile
  return *reinterpret_cast<const s16x8*>(t + row * DH + 8 * swz(row, chunk));
}

// two 8-B halves (elements c0..c0+3 and c0+16..c0+19) of row `row` of a [rows][TP] tile
__device__ __forceinline__ s16x8 frag_split(const bf16_t* t, int row, int c0) {
  const uint2 lo = *reinterpret_cast<const uint2*>(t + row * TP + c0);
  const uint2 hi = *reinterpret_cast<const uint2*>(t + row * TP + c0 + 16);
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 u = {lo.x, lo.y, hi.x, hi.y};
  return __builtin_bit_cast(s16x8, u);
}

__device__ __forceinline__ s16x8 pack8(const float (&a)[4], const float (&b)[4]) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 u = {pack2(a[0], a[1]), pack2(a[2], a[3]), pack2(b[0], b[1]), pack2(b[2], b[3])};
  return __builtin_bit_cast(s16x8, u);
}

__device__ __forceinline__ uint4 ld16(const bf16_t* p, bool ok) {
  return ok ? *reinterpret_cast<const uint4*>(p) : make_uint4(0u, 0u, 0u, 0u);
}

// rows 4 kg .. 4 kg + 3, 8-element chunk dc of a [L][ld] row-major source (rows >= L zero) -> the transposed tile
// t[d][row] ([64][TP]); optionally also the swizzled row-major copy rm[row][64]
__device__ __forceinline__ void load_transpose(const bf16_t* src, long long ld, int L, bf16_t* t, bf16_t* rm, int tid) {
  const int kg = tid >> 3, dc = tid & 7;
  uint4 v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = ld16(src + (long long)(4 * kg + e) * ld + 8 * dc, 4 * kg + e < L);
  if (rm) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 4 * kg + e;
      *reinterpret_cast<uint4*>(rm + r * DH + 8 * swz(r, dc)) = v[e];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    uint2 q;
    q.x = half16(v[0], j) | (half16(v[1], j) << 16);
    q.y = half16(v[2], j) | (half16(v[3], j) << 16);
    *reinterpret_cast<uint2*>(t + (8 * dc + j) * TP + 4 * kg) = q;
  }
}

}  // namespace attn

// 128 < Lmax <= 512 (bert_attn_long.hip); the arguments are vcg_bert_attn_fwd/bwd_varlen's, already checked. stats:
// float2 [B * nh][Lr] (row max, 1 / row sum) then float [B * nh][Lr] (the backward's D), Lr = Lmax rounded up to 128.
int bert_attn_long_fwd(const void* qkv, const long long* mask, const int* seq, void* ctx, void* stats, int B, int nh,
                       int Lmax, int Lp, float scale, float dropout_p, unsigned long long seed, hipStream_t s);
int bert_attn_long_bwd(const void* qkv, const void* dctx, const long long* mask, const int* seq, void* stats,
                       void* dqkv, int B, int nh, int Lmax, int Lp, float scale, float dropout_p,
                       unsigned long long seed, hipStream_t s);

}  // namespace vcg
