// MFMA / LDS primitives shared by the bf16 GEMM engines (igemm_fast, igemm256, igemm_wide, igemm_wgrad, conv_patch,
// stem_bwd, bn_gram, stream1x1): one definition each of the LDS address cast, the bf16 pack / unpack of 16-B chunks,
// the XCD-aware workgroup decodes, the counted-vmcnt immediate, the transposed LDS read and its swizzle.
#pragma once
#include "common.h"

namespace vcg {

typedef __attribute__((address_space(3))) void lds_void_t;  // LDS-DMA destination (buffer_load ... lds)
typedef __attribute__((address_space(3))) char lds_char;
// 32-bit LDS address of a __shared__ pointer, for inline-asm ds_* accesses (a plain LDS access makes hipcc wait
// vmcnt(0) for in-flight LDS-DMA first; the engines order theirs with explicit lgkmcnt waits instead)
__device__ __forceinline__ uint32_t lds_u32(const void* p) { return (uint32_t)(uintptr_t)(const lds_char*)p; }

// 8 bf16 of a 16-B chunk -> fp32
__device__ __forceinline__ void unpack8(const uint4& u, float (&v)[8]) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
// two / eight fp32 -> bf16 (RNE), packed low element first
__device__ __forceinline__ uint32_t pack2bf(float a, float b) { return (uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16); }
__device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
  uint4 o;
  o.x = pack2bf(v[0], v[1]);
  o.y = pack2bf(v[2], v[3]);
  o.z = pack2bf(v[4], v[5]);
  o.w = pack2bf(v[6], v[7]);
  return o;
}

// Workgroups are dealt round-robin to the 8 XCDs by linear id (blocks b and b + 8 share an XCD).
// Bijective remap of n linear ids so that XCD x takes the contiguous range [x q + min(x, r), ...) of n = 8 q + r
// tiles / slots: the tiles running at once on one XCD are neighbours and share operand rows in its L2.
__device__ __forceinline__ int xcd_range(int b, int n) {
  const int q = n >> 3, r = n & 7, x = b & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}
// Decode of a (nx column tiles) x (gy tile rows) grid: when gy % 8 == 0 every column tile of an M-tile row runs on
// one XCD at the same time, so the A rows come from HBM once (L2 hits for the other column tiles).
__device__ __forceinline__ void xcd_row_decode(int nx, int gy, int& bx, int& by) {
  if ((gy & 7) == 0) {
    const int sidx = blockIdx.x >> 3;
    bx = sidx % nx;
    by = (sidx / nx) * 8 + (blockIdx.x & 7);
  } else {
    bx = blockIdx.x % nx;
    by = blockIdx.x / nx;
  }
}

__device__ __forceinline__ constexpr int waitcnt_vm(int n) {
  // s_waitcnt simm16 for gfx9-family: vmcnt[3:0] | expcnt 7 << 4 | lgkmcnt 15 << 8 | vmcnt[5:4] << 14
  return (n & 0xF) | (0x7 << 4) | (0xF << 8) | (((n >> 4) & 3) << 14);
}

// transposed LDS read: lanes 4q + pp of a 16-lane group address row q (4 consecutive rows), columns 4 pp .. + 3 and
// each lane receives 4 consecutive ROWS of one column (inline asm, see lds_u32)
__device__ __forceinline__ void lds_tr_b16(s16x4& v, uint32_t addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr) : "memory");
}
__device__ __forceinline__ void lds_tr_b16(s16x4& v, const bf16_t* p) { lds_tr_b16(v, lds_u32(p)); }
// 16-B slot of chunk c in row `row` of a [rows][64] bf16 tile read with lds_tr_b16 (an involution in c): the reads
// of 4 consecutive rows x 16 columns are conflict-free
__device__ __forceinline__ int tr_swz64(int row, int c) { return c ^ (2 * ((row >> 1) & 3)); }

}  // namespace vcg
