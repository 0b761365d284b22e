// The two streaming input-gradient bodies of igemm_fast_kernel (EPI_BWD_STREAM), built from one set of steps. Included
// by igemm_fast.hip only (after FAST_STAMP is defined): the bodies run under that kernel's symbol.
#pragma once
#include "fast_epilogue.h"

namespace vcg {

// ---- EPI_BWD_STREAM: the fused 1x1 conv input gradient (EPI_BWD) with K <= 128, as a streaming kernel ----------
// For the trunk's conv1 dgrads of layers 1-2 (K = 64 / 128 input channels of dy) the GEMM is a small part of the
// work: per 64 x 64 output tile the A rows are 8-16 KB, the epilogue reads the residual, y (the previous block's
// bn3 input) and the mask bits (16.5 KB, + 8 KB y2 after a downsample block) and writes 8 KB of g. The persistent
// 2-stage engine (igemm_fast.hip) issues those epilogue loads only after a tile's MFMAs (two dependent HBM round
// trips per tile: 3.6-4.3 TB/s). Here every operand of a tile is DMA'd into an LDS ring NBUF - 1 tiles ahead; the
// weight tile (64 columns x K) stays in LDS for the whole kernel.
// Tiles are DESTINATION rows d of g: the TSM adjoint moves the dgrad value of GEMM row m to d = m + s hw for the
// columns of shift s (+1: n < fold, -1: fold <= n < 2 fold, 0: the rest), so d's value is the product of the A row
// d - s hw (zero when that frame is outside the clip -- the wrap row of the adjoint -- and the clip-edge rows are
// never read, i.e. dropped). The shift is applied to the A rows (a wave's 32 columns have one shift: fold % 32 == 0;
// a workgroup whose 64 columns straddle two shifts loads two A tiles), so the residual / y / mask / g rows of a tile
// are plain contiguous rows (full 128-B lines; moving them instead costs 35 % at the layer-1 shape).
// Per tile: counted vmcnt (the ring's later tiles and the previous flushes' stores stay in flight), one barrier,
// MFMAs of a 16 x 32 block per wave, the bf16 value staged through LDS, one barrier, then each thread combines one
// 16-B chunk of stage + LDS operands and stores it. Same products, order and rounding as stage_flush_bwd
// (bit-identical g; per-thread column sums combined in a fixed order by bwd_finish).
constexpr int XF_HASY = 1;  // y + mask bits present (the BN sums of the previous block's bn3)
constexpr int XF_BITS = 4;  // mask bits without y: sum g only (the previous block's y3 is not stored, trunk.py)
constexpr int XF_Y2 = 2;    // y2 present (the previous block's downsample BN)
// with XF_BITS: P = g^T a2 of the previous block (a2 of 64 columns: layer 1) accumulated from the stored g tile, so
// the separate weight-gradient GEMM that re-read g and a2 for bn3's sum_gx (trunk.py) is gone; the weight fragments
// then sit in registers to keep the ring at 3-4 slots. (128 a2 columns -- layer 2 -- cost the dgrad as much as the
// GEMM they replace: tools/bench_dgrad_p.py, +212 us vs 225 us; not built.)
constexpr int XF_P64 = 8;
typedef unsigned int pk_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int bwd_tsm_shift(const BwdEpi& e, int n) {
  if (e.tsm_T <= 0) return 0;
  return n < e.tsm_fold ? 1 : (n < 2 * e.tsm_fold ? -1 : 0);
}

// K = 256 (KC = 4, layer 3): one A tile per slot (the host admits it only when no workgroup's 64 columns straddle two
// TSM shifts) and the weight fragments of a wave's 32 columns in registers (64 VGPRs) instead of LDS, so the ring
// keeps 3 slots (with the weights in LDS and one A tile per slot it had 2, measured step-neutral in round 4).
__host__ __device__ constexpr int bwd_stream_pj(int XF) { return (XF & XF_P64) ? 64 : 0; }
__host__ __device__ constexpr bool bwd_stream_breg(int KC, int XF) { return KC > 2 || bwd_stream_pj(XF) > 0; }
__host__ __device__ constexpr int bwd_stream_na(int KC, int XF) { return KC > 2 ? 1 : 2; }
// LDS bytes of one ring slot / of the fixed part (weights, stage, column parameters) and the ring depth
__host__ __device__ constexpr int bwd_stream_buf(int KC, int XF) {
  return bwd_stream_na(KC, XF) * KC * 8192 + 8192 + ((XF & XF_HASY) ? 8192 : 0) +
         ((XF & (XF_HASY | XF_BITS)) ? 8 * 256 : 0) + ((XF & XF_Y2) ? 8192 : 0) + bwd_stream_pj(XF) * 128;
}
#ifndef VCG_STREAM_NBUF
#define VCG_STREAM_NBUF 4  // ring slots at most (build knob for A/B builds)
#endif
__host__ __device__ constexpr int bwd_stream_fixed(int KC, int XF) {
  return (bwd_stream_breg(KC, XF) ? 0 : KC * 8192) + 8192 + 1024;
}
__host__ __device__ constexpr int bwd_stream_nbuf(int KC, int XF) {
  return (160 * 1024 - bwd_stream_fixed(KC, XF)) / bwd_stream_buf(KC, XF) >= VCG_STREAM_NBUF ? VCG_STREAM_NBUF
         : (160 * 1024 - bwd_stream_fixed(KC, XF)) / bwd_stream_buf(KC, XF);
}

// ---- steps shared by the two bodies (TM = 64 destination rows per tile, TN = 64 / 128 columns, 8 waves) ---------
// Workgroup -> its column tile n0, its first M-tile `by` of the gy tile rows, and how many tiles it walks.
template <int TM, int TN>
__device__ __forceinline__ int stream_decode(const GemmParams& p, int& n0, int& by, int& gy) {
  const int nx = p.N / TN;
  gy = gridDim.x / nx;
  int bx;
  xcd_row_decode(nx, gy, bx, by);
  n0 = bx * TN;
  const int mtiles = (p.M + TM - 1) / TM;
  return by < mtiles ? (mtiles - 1 - by) / gy + 1 : 0;
}

// a workgroup without rows: an all-zero partial slot
template <int TN>
__device__ __forceinline__ void stream_zero_part(const GemmParams& p, int by, int n0, int tid) {
  const BwdEpi& e = p.bwd;
  if (e.nred > 0 && tid < TN)
    for (int r = 0; r < e.nred; ++r) e.part[((long long)by * e.nred + r) * p.N + n0 + tid] = 0.f;
}

// cpar = mean | mean2 | invstd | invstd2 [TN] of the workgroup's columns
template <int TN>
__device__ __forceinline__ void stream_load_cpar(float* cpar, const BwdEpi& e, int n0, int tid) {
  if (tid < TN) {
    const int n = n0 + tid;
    cpar[tid] = e.mean ? e.mean[n] : 0.f;
    cpar[TN + tid] = e.mean2 ? e.mean2[n] : 0.f;
    cpar[2 * TN + tid] = e.invstd ? e.invstd[n] : 0.f;
    cpar[3 * TN + tid] = e.invstd2 ? e.invstd2[n] : 0.f;
  }
  __syncthreads();  // (no LDS-DMA issued yet)
}

// buffer descriptors of the residual (compact for a stride-2 conv) and the mask bits (offset beyond num_records ->
// zeros; nb_*: the descriptor's range = the offset that reads zeros)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t stream_res_rsrc(const GemmParams& p, uint32_t& nb_res) {
  const BwdEpi& e = p.bwd;
  const long long ld = p.ldc;
  const long long rrows = e.res_s > 1 ? (long long)(p.M / e.hw) * e.rH * e.rW : (long long)p.M;
  nb_res = (uint32_t)min(rrows * ld * 2, (long long)0xFFFFFF00LL);
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(e.res), 0, nb_res, 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t stream_bits_rsrc(const GemmParams& p, uint32_t& nb_bits) {
  const long long ld = p.ldc;
  nb_bits = (uint32_t)(((long long)p.M * ld) >> 3);
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.bwd.bits), 0, nb_bits, 0x00020000);
}

// The weight fragments of a wave's 32 columns col0 .. + 31 (column col0 + 16 j + ci, k = 64 kc + 32 s + 8 g .. + 7:
// fast_frag's lane map) straight into registers, retired before the ring's first DMA (so no wait inside the loop
// counts them)
template <int KC>
__device__ __forceinline__ void stream_load_bfrag(s16x8 (&bfr)[KC][2][2], const OpArgs& b, int col0, int lane) {
  const int g = lane >> 4, ci = lane & 15;
  const bf16_t* bp = reinterpret_cast<const bf16_t*>(b.ptr);
#pragma unroll
  for (int kc = 0; kc < KC; ++kc)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        bfr[kc][s][j] =
            *reinterpret_cast<const s16x8*>(bp + (long long)(col0 + 16 * j + ci) * b.ld + 64 * kc + 32 * s + 8 * g);
#pragma unroll
  for (int kc = 0; kc < KC; ++kc)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 2; ++j) asm volatile("" ::"v"(bfr[kc][s][j]));
}

// TSM-shifted A rows: destination row d reads GEMM row d - s hw, zero outside the clip.
// stream_clip_t: d's frame index within its clip (0 when none of the workgroup's columns is shifted);
// stream_a_off: the FastLoader row offset under shift s (-1: zeros)
__device__ __forceinline__ int stream_clip_t(const GemmParams& p, int d, bool shifted) {
  const BwdEpi& e = p.bwd;
  int f = 0, tt = 0;
  if (e.tsm_T > 0 && shifted) {
    f = (int)fdiv((uint32_t)min(d, p.M - 1), e.fd_hw);
    tt = f - (int)fdiv((uint32_t)f, e.fd_T) * e.tsm_T;
  }
  return tt;
}
__device__ __forceinline__ int stream_a_off(const GemmParams& p, int d, int tt, int s) {
  const BwdEpi& e = p.bwd;
  const bool ok = d < p.M && (unsigned)(tt - s) < (unsigned)max(e.tsm_T, 1);
  return ok ? (int)((long long)(d - s * e.hw) * p.a.ld) : -1;
}

// byte offset of the residual's 16-B chunk at column n of destination row dr (nb_res: zeros)
__device__ __forceinline__ uint32_t stream_res_off(const GemmParams& p, int dr, int n, uint32_t nb_res) {
  const BwdEpi& e = p.bwd;
  const long long ld = p.ldc;
  uint32_t roff = (uint32_t)((long long)dr * ld + n) * 2u;
  if (e.res_s > 1) {  // compact residual of a 1x1 / stride-2 conv: only even (h, w) rows carry one
    const uint32_t f2 = fdiv((uint32_t)dr, e.fd_hw), rr = (uint32_t)dr - f2 * (uint32_t)e.hw;
    const uint32_t h = fdiv(rr, e.fd_w), w = rr - h * e.fd_w.d;
    roff = ((h | w) & 1u) ? nb_res : (uint32_t)((((long long)(f2 * e.rH + (h >> 1)) * e.rW + (w >> 1)) * ld + n) * 2);
  }
  return dr < p.M ? roff : nb_res;
}

// Mask bytes of a tile, [8 waves][256 B] in the slot (rows 8 w .. + 7 x TN / 8 bytes, + pad): TN / 32 dwords per row,
// so lane < 8 (TN / 32) of wave w loads dword lane % (TN / 32) of row 8 w + lane / (TN / 32). stream_bits_addr: the
// LDS address of the byte of row `row`, 8-column chunk `chunk`
template <int TN>
__device__ __forceinline__ void stream_bits_piece(const GemmParams& p, __amdgpu_buffer_rsrc_t rs_bits, uint32_t nb_bits,
                                                  char* dst, int d0, int n0, int wave, int lane) {
  constexpr int LPR = TN / 32;
  const long long ld = p.ldc;
  const int dr = d0 + 8 * wave + ((lane & (8 * LPR - 1)) / LPR), n = n0 + 32 * (lane & (LPR - 1));
  const bool ok = lane < 8 * LPR && dr < p.M;
  const uint32_t boff = (uint32_t)(((long long)dr * ld + n) >> 3);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_bits, (lds_void_t*)(dst + wave * 256), 4, ok ? boff : nb_bits, 0, 0, 0);
}
template <int TN> __device__ __forceinline__ uint32_t stream_bits_addr(const uint8_t* Bt, int row, int chunk) {
  return lds_u32(Bt + (row >> 3) * 256 + (row & 7) * (TN / 8) + chunk);
}

// Tile t has landed once only the ring's later tiles (NBUF - 2) and the stores of the NBUF - 1 flushes since its DMA
// are outstanding (steady state: VMW VMEM instructions per wave, VMW2 with two A tiles per slot); the first / last
// tiles wait for everything
template <int NBUF, int VMW, int VMW2 = VMW>
__device__ __forceinline__ void stream_wait_tile(int t, int my_tiles, bool two = false) {
  if (t >= NBUF - 1 && t + NBUF - 2 < my_tiles) {
    if (two) __builtin_amdgcn_s_waitcnt(waitcnt_vm(VMW2));
    else __builtin_amdgcn_s_waitcnt(waitcnt_vm(VMW));
  } else {
    __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
  }
}

// ---- K = 64 / 128 / 256 with 64 x 64 tiles: the epilogue goes through the stage ---------------------------------
template <int KC, int XF>
__device__ __forceinline__ void bwd_stream_body(const GemmParams& p) {
  constexpr bool HASY = (XF & XF_HASY) != 0, Y2 = (XF & XF_Y2) != 0;
  constexpr bool HASB = HASY || (XF & XF_BITS) != 0;  // mask bits + sum g
  static_assert(!Y2 || HASY, "y2 comes with y");
  constexpr int TM = 64, TN = 64, NTH = 512, NW = 8;
  constexpr int PJ = bwd_stream_pj(XF);
  static_assert(PJ == 0 || ((XF & XF_BITS) && !HASY), "P = g^T a2 with the mask bits alone");
  constexpr bool BREG = bwd_stream_breg(KC, XF);  // weight fragments in registers
  constexpr int NA = bwd_stream_na(KC, XF);       // A tiles per slot
  constexpr int NBUF = bwd_stream_nbuf(KC, XF);
  static_assert(NBUF >= 2, "LDS ring");  // (WIDE: 3 without y2; the host keeps WIDE + y on the persistent engine)
  constexpr int AT = KC * TM * 64 * 2;  // one A tile ([64][64] swizzled sub-tiles, fast_frag layout); two per slot
  constexpr int OB = TM * TN * 2;       // one row-major [64][64] bf16 epilogue operand (res / y / y2)
  constexpr int OFF_R = NA * AT, OFF_Y = OFF_R + OB, OFF_BITS = OFF_Y + (HASY ? OB : 0);
  constexpr int OFF_Y2 = OFF_BITS + (HASB ? NW * 256 : 0);  // mask bytes (stream_bits_piece)
  constexpr int OFF_A2 = OFF_Y2 + (Y2 ? OB : 0);             // a2 rows [64][PJ], 16-B chunks swizzled (tr_swz64)
  constexpr int BUF = OFF_A2 + PJ * 128;
  static_assert(BUF == bwd_stream_buf(KC, XF), "slot layout");
  constexpr int BB = BREG ? 0 : KC * TN * 64 * 2;
  constexpr int SB = TM * TN * 2;
  constexpr int TOTAL = NBUF * BUF + BB + SB + 4 * TN * 4;
  static_assert(TOTAL <= 160 * 1024, "LDS budget");
  static_assert(NBUF * BUF >= 3 * NTH * 8 * 4, "bwd_finish scratch");
  // VMEM instructions per wave: one tile's DMA (A 1 per k tile and A tile, res 1, y 1 + bits 1, y2 1), one flush's
  // stores (1)
  constexpr int OPS1 = KC + 1 + (HASY ? 1 : 0) + (HASB ? 1 : 0) + (Y2 ? 1 : 0) + PJ / 64, OPS2 = OPS1 + KC;
  constexpr int VMW1 = (NBUF - 2) * OPS1 + (NBUF - 1), VMW2 = (NBUF - 2) * OPS2 + (NBUF - 1);
  static_assert(VMW2 < 64, "vmcnt field");
  __shared__ __attribute__((aligned(1024))) char smem[TOTAL];  // the ONLY LDS object (see FastLoader)
  char* ring = smem;
  bf16_t* Bs = reinterpret_cast<bf16_t*>(smem + NBUF * BUF);
  bf16_t* St = reinterpret_cast<bf16_t*>(smem + NBUF * BUF + BB);
  float* cpar = reinterpret_cast<float*>(smem + NBUF * BUF + BB + SB);  // mean | mean2 | invstd | invstd2 [TN]

  const BwdEpi& e = p.bwd;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int n0, by, gy;
  const int my_tiles = stream_decode<TM, TN>(p, n0, by, gy);
  if (my_tiles == 0) {
    stream_zero_part<TN>(p, by, n0, tid);
    if constexpr (PJ > 0)
      for (int i = tid; i < TN * PJ; i += NTH) e.ppart[((long long)by * p.N + n0) * PJ + i] = 0.f;
    return;
  }
  stream_load_cpar<TN>(cpar, e, n0, tid);
  const int cc = tid & 7;  // the flush's 16-B column chunk of this thread (fixed for the whole kernel)
  float mu[8], mu2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    mu[i] = cpar[8 * cc + i];
    mu2[i] = cpar[TN + 8 * cc + i];
  }
  // TSM shifts of the workgroup's two 32-column halves; two A tiles when they differ (never for WIDE: host check)
  const int sh0 = bwd_tsm_shift(e, n0), sh1 = bwd_tsm_shift(e, n0 + 32);
  const bool two = NA == 2 && sh0 != sh1;

  // buffer descriptors of the epilogue operands (offset beyond num_records -> zeros)
  const long long ld = p.ldc;
  const uint32_t nb_full = (uint32_t)min((long long)p.M * ld * 2, (long long)0xFFFFFF00LL);
  uint32_t nb_res, nb_bits = 0;
  const __amdgpu_buffer_rsrc_t rs_res = stream_res_rsrc(p, nb_res);
  __amdgpu_buffer_rsrc_t rs_y = rs_res, rs_y2 = rs_res, rs_bits = rs_res;
  if constexpr (HASY) rs_y = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(e.y), 0, nb_full, 0x00020000);
  if constexpr (HASB) rs_bits = stream_bits_rsrc(p, nb_bits);
  if constexpr (Y2) rs_y2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(e.y2), 0, nb_full, 0x00020000);
  uint32_t nb_a2 = 0;
  __amdgpu_buffer_rsrc_t rs_a2 = rs_res;
  if constexpr (PJ > 0) {
    nb_a2 = (uint32_t)min((long long)p.M * PJ * 2, (long long)0xFFFFFF00LL);
    rs_a2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(e.a2), 0, nb_a2, 0x00020000);
  }

  FastLoader<64, OP_DENSE_K, NW> la, lb;
  const int g = lane >> 4, ci = lane & 15;
  const int wr = wave & 3, wc = wave >> 2;  // MFMA block: rows 16 wr .. + 15, columns 32 wc .. + 31 of the tile
  s16x8 bfr[BREG ? KC : 1][2][2];
  if constexpr (BREG) {
    stream_load_bfrag<KC>(bfr, p.b, n0 + 32 * wc, lane);
  } else {
    lb.init(p.b, 0, n0, wave, lane);
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) lb.issue(p.b, kc * 64, p.K, Bs + kc * 4096, wave);
  }

  auto issue_tile = [&](int t) {
    const int d0 = (by + t * gy) * TM;
    char* buf = ring + (t % NBUF) * BUF;
    la.init(p.a, 0, d0, wave, lane);
    const int d = d0 + wave * 8 + (lane >> 3);  // FastLoader<64, dense, 8 waves>: one row per lane
    const int tt = stream_clip_t(p, d, (sh0 | sh1) != 0);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      if (a == 1 && !two) break;
      la.off[0] = stream_a_off(p, d, tt, a == 0 ? sh0 : sh1);
#pragma unroll
      for (int kc = 0; kc < KC; ++kc)
        la.issue(p.a, kc * 64, p.K, reinterpret_cast<bf16_t*>(buf + a * AT) + kc * 4096, wave);
    }
    // residual / y / y2 rows: this wave's instruction covers tile rows 8 wave .. + 7, lane -> (row, chunk)
    {
      const int r = wave * 8 + (lane >> 3);
      const int dr = d0 + r, n = n0 + 8 * (lane & 7);
      const bool ok = dr < p.M;
      const uint32_t yoff = (uint32_t)((long long)dr * ld + n) * 2u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_res, (lds_void_t*)(buf + OFF_R + wave * 1024), 16,
                                               stream_res_off(p, dr, n, nb_res), 0, 0, 0);
      if constexpr (HASY)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_y, (lds_void_t*)(buf + OFF_Y + wave * 1024), 16, ok ? yoff : nb_full,
                                                 0, 0, 0);
      if constexpr (Y2)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_y2, (lds_void_t*)(buf + OFF_Y2 + wave * 1024), 16,
                                                 ok ? yoff : nb_full, 0, 0, 0);
    }
    if constexpr (HASB) stream_bits_piece<TN>(p, rs_bits, nb_bits, buf + OFF_BITS, d0, n0, wave, lane);
    if constexpr (PJ > 0) {  // a2 rows [64][PJ]: 1 KB per instruction, the lane at slot q of row r loads chunk
#pragma unroll                // tr_swz64(r, q) (the transposed reads' swizzle)
      for (int h = 0; h < PJ / 64; ++h) {
        constexpr int CPRA = PJ / 8;  // 16-B chunks per a2 row
        const int r = (8 * h + wave) * (1024 / (PJ * 2)) + lane / CPRA, q = lane % CPRA;
        const int dr = d0 + r, c = tr_swz64(r, q);
        const uint32_t aoff = dr < p.M ? (uint32_t)(((long long)dr * PJ + 8 * c) * 2) : nb_a2;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a2, (lds_void_t*)(buf + OFF_A2 + (8 * h + wave) * 1024), 16,
                                                 aoff, 0, 0, 0);
      }
    }
  };

#pragma unroll
  for (int i = 0; i < NBUF - 1; ++i)
    if (i < my_tiles) issue_tile(i);

  float s1[8], s2[8], s3[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) s1[i] = s2[i] = s3[i] = 0.f;
  f32x4 accp[PJ > 0 ? PJ / 32 : 1];
#pragma unroll
  for (int i = 0; i < (PJ > 0 ? PJ / 32 : 1); ++i) accp[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16_t* Cout = reinterpret_cast<bf16_t*>(p.C);

  for (int t = 0; t < my_tiles; ++t) {
    FAST_STAMP(t, 0);
    stream_wait_tile<NBUF, VMW1, VMW2>(t, my_tiles, two);
    __builtin_amdgcn_s_barrier();  // tile t visible to every wave; every wave's reads of the ring slot below retired
    FAST_STAMP(t, 1);
    if (t + NBUF - 1 < my_tiles) issue_tile(t + NBUF - 1);
    const int d0 = (by + t * gy) * TM;
    const char* buf = ring + (t % NBUF) * BUF;
    const bf16_t* At = reinterpret_cast<const bf16_t*>(buf + ((two && wc == 1) ? AT : 0));
    f32x4 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < KC; ++kc)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const s16x8 af = fast_frag(At + kc * 4096, 16 * wr, lane, s);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          s16x8 bf;
          if constexpr (BREG) bf = bfr[kc][s][j];
          else bf = fast_frag(Bs + kc * 4096, 32 * wc + 16 * j, lane, s);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, af, acc[j], 0, 0, 0);
        }
      }
    // stage the bf16 GEMM value: row 16 wr + ci, columns 32 wc + 16 j + 4 g .. + 3
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = 16 * wr + ci, col = 32 * wc + 16 * j + 4 * g;
      uint2 q2;
      q2.x = pack2bf(acc[j][0], acc[j][1]);
      q2.y = pack2bf(acc[j][2], acc[j][3]);
      // (inline asm: a plain LDS store makes hipcc wait vmcnt(0) for the ring's in-flight DMA first)
      asm volatile("ds_write_b64 %0, %1" ::"v"(lds_u32(St + row * 64 + 8 * st_slot<64>(row, col >> 3) + (col & 7))),
                   "v"(q2) : "memory");
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    FAST_STAMP(t, 2);
    const bf16_t* R = reinterpret_cast<const bf16_t*>(buf + OFF_R);
    const bf16_t* Y = reinterpret_cast<const bf16_t*>(buf + OFF_Y);
    const bf16_t* Y2p = reinterpret_cast<const bf16_t*>(buf + OFF_Y2);
    const uint8_t* Bt = reinterpret_cast<const uint8_t*>(buf + OFF_BITS);
    {
      const int r = tid >> 3;
      const int d = d0 + r, n = n0 + 8 * cc;
      // (LDS reads as inline asm: hipcc would wait vmcnt(0) for the ring's in-flight DMA before plain ones)
      uint4 sv, rv, yv = make_uint4(0u, 0u, 0u, 0u), y2v = yv;
      uint32_t bits = 0xFFu;
      asm volatile("ds_read_b128 %0, %1" : "=v"(sv) : "v"(lds_u32(St + r * 64 + 8 * st_slot<64>(r, cc))) : "memory");
      asm volatile("ds_read_b128 %0, %1" : "=v"(rv) : "v"(lds_u32(R + r * 64 + 8 * cc)) : "memory");
      if constexpr (HASY)
        asm volatile("ds_read_b128 %0, %1" : "=v"(yv) : "v"(lds_u32(Y + r * 64 + 8 * cc)) : "memory");
      if constexpr (HASB)
        asm volatile("ds_read_u8 %0, %1" : "=v"(bits) : "v"(stream_bits_addr<TN>(Bt, r, cc)) : "memory");
      if constexpr (Y2)
        asm volatile("ds_read_b128 %0, %1" : "=v"(y2v) : "v"(lds_u32(Y2p + r * 64 + 8 * cc)) : "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      uint4 o = make_uint4(0u, 0u, 0u, 0u);  // (rows past M: zeros for the P product)
      if (d < p.M) {
        float v[8], rr[8];
        unpack8(sv, v);
        unpack8(rv, rr);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] += rr[i];
        if constexpr (HASB) {
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] = ((bits >> i) & 1u) ? v[i] : 0.f;
        }
        o = pack8(v);
        *reinterpret_cast<uint4*>(Cout + (long long)d * ld + n) = o;
        if constexpr (HASB && !HASY) {
          unpack8(o, v);  // sum of the stored (rounded) gradient
#pragma unroll
          for (int i = 0; i < 8; ++i) s1[i] += v[i];
        }
        if constexpr (HASY) {
          float yy[8];
          unpack8(o, v);  // statistics of the stored (rounded) gradient
          unpack8(yv, yy);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            s1[i] += v[i];
            s2[i] = fmaf(v[i], yy[i] - mu[i], s2[i]);
          }
          if constexpr (Y2) {
            float y2[8];
            unpack8(y2v, y2);
#pragma unroll
            for (int i = 0; i < 8; ++i) s3[i] = fmaf(v[i], y2[i] - mu2[i], s3[i]);
          }
        }
      }
      if constexpr (PJ > 0) {  // the stored g over its own stage chunk, for the P product below
        const pk_u32x4 ov = {o.x, o.y, o.z, o.w};
        asm volatile("ds_write_b128 %0, %1" ::"v"(lds_u32(St + r * 64 + 8 * st_slot<64>(r, cc))), "v"(ov) : "memory");
      }
    }
    if constexpr (PJ > 0) {
      // P[n][j] += sum_r g[r][n] a2[r][j] over the tile's 64 rows: both operands by transposed LDS reads
      // (lds_tr_b16, stem_bwd.hip's lane map: lanes 4q + pp of group g address row 4 g + q, columns 4 pp ..)
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's g chunks are in St
      __builtin_amdgcn_s_barrier();        // ... and every wave's
      const bf16_t* A2 = reinterpret_cast<const bf16_t*>(buf + OFF_A2);
      const int nb = wave & 3, q = ci >> 2, pp = ci & 3;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int k0 = 32 * ks + 4 * g + q, k1 = k0 + 16;
        const int cl = 16 * nb + 4 * pp;
        s16x4 gl, gh, al[PJ / 32], ah[PJ / 32];
        lds_tr_b16(gl, St + k0 * 64 + 8 * st_slot<64>(k0, cl >> 3) + (cl & 7));
        lds_tr_b16(gh, St + k1 * 64 + 8 * st_slot<64>(k1, cl >> 3) + (cl & 7));
#pragma unroll
        for (int i = 0; i < PJ / 32; ++i) {
          const int cj = 16 * ((wave >> 2) + 2 * i) + 4 * pp;
          lds_tr_b16(al[i], A2 + k0 * PJ + 8 * tr_swz64(k0, cj >> 3) + (cj & 7));
          lds_tr_b16(ah[i], A2 + k1 * PJ + 8 * tr_swz64(k1, cj >> 3) + (cj & 7));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        const s16x8 gf = s16x8{gl[0], gl[1], gl[2], gl[3], gh[0], gh[1], gh[2], gh[3]};
#pragma unroll
        for (int i = 0; i < PJ / 32; ++i)
          accp[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              s16x8{al[i][0], al[i][1], al[i][2], al[i][3], ah[i][0], ah[i][1], ah[i][2], ah[i][3]}, gf, accp[i], 0, 0,
              0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    FAST_STAMP(t, 3);
  }
  __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
  if constexpr (PJ > 0) {  // accp[i][rr] = P[n0 + 16 nb + ci][16 ((wave >> 2) + 2 i) + 4 g + rr] -> slab `by`
    float* pp = e.ppart + ((long long)by * p.N + n0 + 16 * (wave & 3) + ci) * PJ;
#pragma unroll
    for (int i = 0; i < PJ / 32; ++i)
      *reinterpret_cast<f32x4*>(pp + 16 * ((wave >> 2) + 2 * i) + 4 * g) = accp[i];
  }
  if constexpr (HASB) {
    if (e.nred > 0) bwd_finish<NTH, TN>(p, reinterpret_cast<float*>(smem), cpar + 2 * TN, s1, s2, s3, n0, by);
  }
}

// K = 256 with 64 x 128 tiles (the layer-3 conv1 input gradients: every 128-column tile inside one TSM shift, fold
// % 128 == 0, and the mask bits without y -- the previous block's y3 is not stored). Per-tile stamps of the 64 x 64
// form (tools/bench_dgrad.py, -DVCG_FAST_STAMPS) put ~2/3 of a tile in the phase that issues the next tile's LDS-DMA
// (6 1-KB pieces per wave) next to the MFMAs; here one A tile (32 KB) serves 128 columns (LDS-DMA per output byte
// 50 / 16 instead of 40.5 / 8), the next tile's A pieces are issued between the k-steps' MFMAs, and the epilogue runs
// in the MFMA lanes on the residual rows in LDS: g = mask(bf16(acc) + res) is written back over the residual (same
// lane, same bytes: no barrier, no separate stage), and the flush threads only copy 16-B chunks out and sum them.
// The residual rows land pre-swizzled (16-B chunk c of row r at slot c ^ (r & 15)), so the MFMA lanes' 8-B accesses
// (16 rows, one column group) and the flush's 16-B row reads are both conflict-free. The weight fragments of a wave's
// 32 columns stay in registers; 3 slots of 50 KB.
template <int XF>
__device__ __forceinline__ void bwd_stream128_body(const GemmParams& p) {
  constexpr bool HASB = (XF & XF_BITS) != 0;
  static_assert((XF & (XF_HASY | XF_Y2)) == 0, "the mask bits without y only");
  constexpr int KC = 4, TM = 64, TN = 128, NTH = 512, NW = 8;
  constexpr int AT = KC * TM * 64 * 2;               // A tile [4][64][64] swizzled (fast_frag layout), 32 KB
  constexpr int OB = TM * TN * 2;                    // residual rows -> g, [64][128] bf16 swizzled, 16 KB
  constexpr int OFF_R = AT, OFF_BITS = OFF_R + OB;  // mask bytes (stream_bits_piece)
  constexpr int BUF = OFF_BITS + (HASB ? NW * 256 : 0);
  constexpr int CP = 4 * TN * 4;
  constexpr int NBUF = (160 * 1024 - CP) / BUF;
  static_assert(NBUF >= 3 && NBUF * BUF + CP <= 160 * 1024, "LDS ring");
  static_assert(NBUF * BUF >= 3 * NTH * 8 * 4, "bwd_finish scratch");
  // VMEM instructions per wave: one tile's DMA (A 4, residual 2, bits 1), one flush's stores (2)
  constexpr int OPS = KC + 2 + (HASB ? 1 : 0), STO = 2;
  constexpr int VMW = (NBUF - 2) * OPS + (NBUF - 1) * STO;
  static_assert(VMW < 64, "vmcnt field");
  __shared__ __attribute__((aligned(1024))) char smem[NBUF * BUF + CP];  // the ONLY LDS object
  char* ring = smem;
  float* cpar = reinterpret_cast<float*>(smem + NBUF * BUF);  // mean | mean2 | invstd | invstd2 [TN]

  const BwdEpi& e = p.bwd;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int n0, by, gy;
  const int my_tiles = stream_decode<TM, TN>(p, n0, by, gy);
  if (my_tiles == 0) {
    stream_zero_part<TN>(p, by, n0, tid);
    return;
  }
  stream_load_cpar<TN>(cpar, e, n0, tid);
  const int cc = tid & 15;  // the flush's 16-B column chunk of this thread (fixed for the whole kernel)
  const int sh = bwd_tsm_shift(e, n0);  // one shift for the tile's 128 columns (host check)

  const long long ld = p.ldc;
  uint32_t nb_res, nb_bits = 0;
  const __amdgpu_buffer_rsrc_t rs_res = stream_res_rsrc(p, nb_res);
  __amdgpu_buffer_rsrc_t rs_bits = rs_res;
  if constexpr (HASB) rs_bits = stream_bits_rsrc(p, nb_bits);

  FastLoader<64, OP_DENSE_K, NW> la;
  const int g = lane >> 4, ci = lane & 15;
  const int wr = wave & 1, wc = wave >> 1;  // MFMA block: rows 32 wr .. + 31, columns 32 wc .. + 31 of the tile
  s16x8 bfr[KC][2][2];
  stream_load_bfrag<KC>(bfr, p.b, n0 + 32 * wc, lane);

  // tile t's A rows (piece kc) / residual rows + mask bytes into its ring slot
  auto a_init = [&](int t) {
    const int d0 = (by + t * gy) * TM;
    la.init(p.a, 0, d0, wave, lane);
    const int d = d0 + wave * 8 + (lane >> 3);  // FastLoader<64, dense, 8 waves>: one row per lane
    la.off[0] = stream_a_off(p, d, stream_clip_t(p, d, sh != 0), sh);
  };
  auto a_piece = [&](int t, int kc) {
    la.issue(p.a, kc * 64, p.K, reinterpret_cast<bf16_t*>(ring + (t % NBUF) * BUF) + kc * 4096, wave);
  };
  // residual rows: instruction h of this wave covers tile rows 32 h + 4 wave .. + 3; the lane at LDS slot q of row
  // r loads chunk q ^ (r & 15)
  auto res_piece = [&](int t, int h) {
    const int d0 = (by + t * gy) * TM;
    char* buf = ring + (t % NBUF) * BUF;
    const int r = 32 * h + 4 * wave + (lane >> 4);
    const int dr = d0 + r, n = n0 + 8 * ((lane & 15) ^ (r & 15));
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_res, (lds_void_t*)(buf + OFF_R + (8 * h + wave) * 1024), 16,
                                             stream_res_off(p, dr, n, nb_res), 0, 0, 0);
  };
  auto bits_piece = [&](int t) {
    if constexpr (HASB)
      stream_bits_piece<TN>(p, rs_bits, nb_bits, ring + (t % NBUF) * BUF + OFF_BITS, (by + t * gy) * TM, n0, wave, lane);
  };

#pragma unroll
  for (int i = 0; i < NBUF - 1; ++i)
    if (i < my_tiles) {
      a_init(i);
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) a_piece(i, kc);
      res_piece(i, 0);
      res_piece(i, 1);
      bits_piece(i);
    }

  float s1[8], s0[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) s1[i] = s0[i] = 0.f;
  bf16_t* Cout = reinterpret_cast<bf16_t*>(p.C);

  for (int t = 0; t < my_tiles; ++t) {
    FAST_STAMP(t, 0);
    stream_wait_tile<NBUF, VMW>(t, my_tiles);
    // tile t visible to every wave; every wave's reads of the slot refilled below (tile t - 1's) retired
    __builtin_amdgcn_s_barrier();
    FAST_STAMP(t, 1);
    const bool nxt = t + NBUF - 1 < my_tiles;
    if (nxt) a_init(t + NBUF - 1);
    const int d0 = (by + t * gy) * TM;
    char* buf = ring + (t % NBUF) * BUF;
    const bf16_t* At = reinterpret_cast<const bf16_t*>(buf);
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      if (nxt) {  // the next tile's DMA pieces spread over the k-steps' MFMAs (7 per wave, as the prologue's)
        a_piece(t + NBUF - 1, kc);
        if (kc < 2) res_piece(t + NBUF - 1, kc);
        if (kc == 2) bits_piece(t + NBUF - 1);
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const s16x8 a0 = fast_frag(At + kc * 4096, 32 * wr, lane, s);
        const s16x8 a1 = fast_frag(At + kc * 4096, 32 * wr + 16, lane, s);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[kc][s][j], a0, acc[0][j], 0, 0, 0);
          acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[kc][s][j], a1, acc[1][j], 0, 0, 0);
        }
      }
    }
    FAST_STAMP(t, 2);
    // epilogue in the MFMA lanes: row 32 wr + 16 i + ci, columns 32 wc + 16 j + 4 g .. + 3 of the residual / g rows
    bf16_t* Rg = reinterpret_cast<bf16_t*>(buf + OFF_R);
    const uint8_t* Bt = reinterpret_cast<const uint8_t*>(buf + OFF_BITS);
    uint2 rv[2][2];
    uint32_t bw[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = 32 * wr + 16 * i + ci, col = 32 * wc + 16 * j + 4 * g;
        // (LDS reads / writes as inline asm: hipcc would wait vmcnt(0) for the ring's in-flight DMA first)
        asm volatile("ds_read_b64 %0, %1"
                     : "=v"(rv[i][j])
                     : "v"(lds_u32(Rg + row * TN + 8 * st_slot<TN>(row, col >> 3) + (col & 7)))
                     : "memory");
        bw[i][j] = 0xFFu;
        if constexpr (HASB)
          asm volatile("ds_read_u8 %0, %1" : "=v"(bw[i][j]) : "v"(stream_bits_addr<TN>(Bt, row, col >> 3)) : "memory");
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = 32 * wr + 16 * i + ci, col = 32 * wc + 16 * j + 4 * g;
        const uint32_t rw[2] = {rv[i][j].x, rv[i][j].y};
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float r = __uint_as_float((q & 1) ? (rw[q >> 1] & 0xffff0000u) : (rw[q >> 1] << 16));
          v[q] = bf2f(f2bf(acc[i][j][q])) + r;  // the staged bf16 GEMM value + residual (stage_flush_bwd order)
          if constexpr (HASB) v[q] = ((bw[i][j] >> ((col & 7) + q)) & 1u) ? v[q] : 0.f;
        }
        uint2 o;
        o.x = pack2bf(v[0], v[1]);
        o.y = pack2bf(v[2], v[3]);
        asm volatile("ds_write_b64 %0, %1" ::"v"(lds_u32(Rg + row * TN + 8 * st_slot<TN>(row, col >> 3) + (col & 7))),
                     "v"(o) : "memory");
      }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    FAST_STAMP(t, 3);
    // flush: each thread copies row chunks (r, cc) of g out and sums them
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = (tid >> 4) + 32 * h;
      const int d = d0 + r, n = n0 + 8 * cc;
      uint4 o;
      asm volatile("ds_read_b128 %0, %1" : "=v"(o) : "v"(lds_u32(Rg + r * TN + 8 * st_slot<TN>(r, cc))) : "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      if (d < p.M) {
        *reinterpret_cast<uint4*>(Cout + (long long)d * ld + n) = o;
        if constexpr (HASB) {
          float v[8];
          unpack8(o, v);  // sum of the stored (rounded) gradient
#pragma unroll
          for (int i = 0; i < 8; ++i) s1[i] += v[i];
        }
      }
    }
  }
  __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
  if constexpr (HASB) {
    if (e.nred > 0) bwd_finish<NTH, TN>(p, reinterpret_cast<float*>(smem), cpar + 2 * TN, s1, s0, s0, n0, by);
  }
}

}  // namespace vcg
