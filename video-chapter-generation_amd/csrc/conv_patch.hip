// The LDS-patch convolution kernels of the bf16 fast GEMM path: the layer-1 3x3 convs (forward, input gradient) and
// the pair-packed 7x7 stem read their im2col operand from an input patch kept in LDS instead of gathering it through
// L2. run_fast_gemm (igemm_fast.hip) tries them first through run_patch_conv; the output stage and the finishers are
// the fast engine's (fast_epilogue.h).
#include "fast_epilogue.h"

namespace vcg {

// ---- 3x3 / stride 1 / pad 1 convolutions over C = 64 channels (layer 1): LDS-resident input patch -------------
// An M-tile is R whole output rows of one image (TM = R * W <= 128 GEMM rows; rows TM..127 of the 128-row MFMA
// tile read clamped addresses and are never stored). The (R + 2) x (W + 2) input pixels that the tile's 9 taps
// read (zero border included) go to LDS ONCE by LDS-DMA -- 64 channels = one 128-B pixel row, swizzled like a
// [rows][64] tile with the pixel index as the row -- and the 9 taps read shifted fragments from it. The im2col
// gather fetches every input pixel 9 times through L2, the patch (R + 2)(W + 2) / (R W) times (1.04x at W = 56,
// R = 2). The filter (64 output columns x 576 = 72 KiB per workgroup) stays in registers: every wave keeps the
// B fragments of its 32 columns for all 9 taps (36 x 16 B per lane), so a tile is one barrier-free run of 144
// MFMAs per wave. That needs > 256 registers per lane: ONE 4-wave workgroup per CU (the 512-entry register file
// of a SIMD for one wave, 160 KiB of LDS for one workgroup), so latency is hidden by depth instead of by other
// waves: patches are issued two tiles ahead into a 3-buffer ring (the dgrad epilogue's y tile rides along), and
// the output goes out through the finished tile's patch buffer. Epilogues: EPI_STORE / EPI_STATS (shared staged
// flushes) and EPI_BWD_AFF with y read from LDS (the fused dgrad of the trunk: BN1 ReLU mask + BN1 sums).
// DG (dgrad): dx pixel (y, x) reads dy (y + 1 - kh, x + 1 - kw), the flipped tap map over the same patch.
// Measured history (trunk shape M = 1024 x 56 x 56): B through a 2-stage LDS ring with a barrier per tap 586 us
// fwd (im2col: 451-495); register B at 2 workgroups per CU spills (256 VGPRs) and lost to im2col.
constexpr int PATCH_MAXPIX = 256;               // (R + 2) PW <= 256 pixels: 32 KiB per patch buffer
constexpr int PATCH_SLICES = PATCH_MAXPIX / 8;  // 1-KiB (8-pixel) LDS-DMA slices per patch
// Patch rows have a fixed pitch PW (32 or 64 pixels >= W + 2; the kernel's template parameter): the chunk swizzle
// depends on the pixel index mod 8 only, so a tap's row offset kh * PW moves a fragment address by a compile-time
// constant (the ds_read offset field) and a lane's 12 fragment addresses per tile (4 row blocks x 3 column taps) are
// computed once per tile. (With PW = W + 2 every fragment read of the 144-MFMA tile loop recomputed its swizzled
// address -- ~5 VALU per read, more vector issue than the MFMAs leave: the MFMA phase ran at 2.45x its issue time.)
constexpr int PATCH_RING = 3;

struct PatchGeom {
  int R, TM, TPI, PW, NP, NS;  // rows per tile, GEMM rows per tile, tiles per image, patch width, pixels, slices
  unsigned long long* stamps;  // profiling (VCG_PATCH_STAMPS=1): s_memtime per phase of workgroup 0, wave 0
};
#define PATCH_STAMP(k)                                                                        \
  do {                                                                                        \
    if (g.stamps && blockIdx.x == 0 && threadIdx.x == 0 && lt < 64) g.stamps[lt * 6 + (k)] = __builtin_amdgcn_s_memtime(); \
  } while (0)

// Patch swizzle: 16-B chunk c of pixel pix sits at slot (c + 2 * (pix / 2)) % 8. A fragment read's 16 lanes of
// one ds_read_b128 bank group take pixels p0..p0+3, p0+12..p0+15 at chunk c and p0+4..p0+11 at chunk c + 1
// (MI355X_MICROARCH: the b128 lane groups); per pixel parity that is 8 consecutive pixels of one parity, offsets
// {0, 2, 5, 7, 9, 11, 12, 14} mod 8 = all 8 slots for any p0, where the XOR swizzle of the [rows][64] tiles
// collides for odd p0 (modelled: 4.5 vs 6.5 LDS cycles per read at W = 56; 4 = conflict-free).
__device__ __forceinline__ int pswz(int pix, int c) { return (c + (pix & ~1)) & 7; }

__device__ __forceinline__ s16x8 patch_frag(const bf16_t* P, int pix, int lane, int s2) {
  return *reinterpret_cast<const s16x8*>(P + pix * 64 + 8 * pswz(pix, 4 * s2 + (lane >> 4)));
}

template <int EPI, bool DG, int PW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void conv3x3_patch_kernel(GemmParams p, PatchGeom g) {
  static_assert(PW == 32 || PW == 64, "patch row pitch");
  constexpr int BM = 128, BN = 64, NW = 4, MT = 4, NT = 2;
  constexpr int PE = PATCH_SLICES * 512;  // elements per patch buffer
  constexpr int YE = 128 * 64;            // elements per y tile (EPI_BWD_AFF)
  constexpr bool BWD = EPI == EPI_BWD_AFF;
  constexpr int NY = BWD ? PATCH_RING : 0;
  constexpr int NIP = 8 + (BWD ? 4 : 0);  // LDS-DMA instructions per wave per tile
  __shared__ __attribute__((aligned(1024))) char smem[(PATCH_RING * PE + NY * YE) * 2];
  bf16_t* Ps = reinterpret_cast<bf16_t*>(smem);
  bf16_t* Ys = Ps + PATCH_RING * PE;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nx = p.N / BN, gy = gridDim.x / nx;
  int bx, by;
  xcd_row_decode(nx, gy, bx, by);
  const int n0 = bx * BN;
  bf16_t* Cout = reinterpret_cast<bf16_t*>(p.C);
  const int mtiles = p.M / g.TM;
  const int my_tiles = by < mtiles ? (mtiles - 1 - by) / gy + 1 : 0;
  const BwdEpi& e = p.bwd;
  if (my_tiles == 0) {
    if (BWD && e.nred > 0 && tid < BN)
      for (int r = 0; r < e.nred; ++r) e.part[((long long)by * e.nred + r) * p.N + n0 + tid] = 0.f;
    return;
  }

  const OpArgs& a = p.a;
  const uint32_t nbytes = (uint32_t)min(a.bytes, (long long)0xFFFFFF00LL);
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.ptr), 0, nbytes, 0x00020000);
  // y of the dgrad epilogue ([M][ldc] bf16; absent: a zero-range descriptor, the DMAs return zeros)
  const uint32_t ybytes = (BWD && e.y) ? (uint32_t)min((long long)p.M * p.ldc * 2, (long long)0xFFFFFF00LL) : 0u;
  const __amdgpu_buffer_rsrc_t yrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(BWD ? e.y : a.ptr), 0, ybytes, 0x00020000);
  const int HW = a.H * a.W;
  // One LDS-DMA piece (1 KiB per wave) of tile lt's loads, q < NIP: q < 8 patch slice wave + 4 q (slices >= NS
  // repeat slice NS - 1: identical bytes to the same place, so the instruction count per wave is fixed; the
  // source chunk is pre-swizzled, the LDS side is lane-linear); q >= 8: y rows 32 wave + 8 (q - 8) .. + 7 of the
  // tile, unswizzled [128][64]. (tg, img, h0: the tile's global index, image, first output row.)
  auto issue_piece = [&](int lt, int tg, int img, int h0, int q) {
    if (q < 8) {
      bf16_t* dst = Ps + (lt % PATCH_RING) * PE;
      const int slice = min(wave + NW * q, g.NS - 1);
      const int pix = 8 * slice + (lane >> 3);
      const int pr = pix / PW, pc = pix % PW;
      const int h = h0 - 1 + pr, w = pc - 1;
      const bool ok = pix < g.NP && (unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W;
      const int csrc = ((lane & 7) - (pix & ~1)) & 7;  // pswz(pix, csrc) == lane & 7
      const uint32_t voff = ok ? (uint32_t)((((img * HW + h * a.W + w) << 6) + 8 * csrc) * 2) : nbytes;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void_t*)(dst + slice * 512), 16, voff, 0, 0, 0);
    } else if constexpr (BWD) {
      bf16_t* ydst = Ys + (lt % PATCH_RING) * YE;
      const int r0 = 32 * wave + 8 * (q - 8), r = r0 + (lane >> 3);
      const uint32_t voff =
          r < g.TM ? (uint32_t)(((long long)(tg * g.TM + r) * p.ldc + n0 + 8 * (lane & 7)) * 2) : ybytes;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(yrsrc, (lds_void_t*)(ydst + r0 * 64), 16, ybytes ? voff : 0u, 0, 0, 0);
    }
  };
  auto issue_tile = [&](int lt) {
    const int tg = by + lt * gy, img = tg / g.TPI, h0 = (tg - img * g.TPI) * g.R;
#pragma unroll
    for (int q = 0; q < NIP; ++q) issue_piece(lt, tg, img, h0, q);
  };
  // register loads first, retired before the first DMA: hipcc's wait tracking then sees them complete inside
  // the loop (otherwise it puts counted vmcnt waits for them between the MFMAs, which also drain the DMAs)
  int rowpix[MT];  // patch pixel of tap (0, 0) for this lane's fragment row (dgrad: of tap (2, 2))
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int ml = wm * 64 + i * 16 + (lane & 15);
    const int r = ml / a.W, w = ml - r * a.W;
    rowpix[i] = ml < g.TM ? r * PW + w : 0;
  }
  // B fragment (tap t, k-step s2, column group j): row n0 + wn*32 + 16j + lane%16, k = 64t + 32 s2 + 8 (lane/16)
  s16x8 breg[9][2][NT];
  {
    const bf16_t* B = reinterpret_cast<const bf16_t*>(p.b.ptr);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const bf16_t* row = B + (long long)(n0 + wn * (BN / 2) + j * 16 + (lane & 15)) * p.b.ld + 8 * (lane >> 4);
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) breg[t][s2][j] = *reinterpret_cast<const s16x8*>(row + 64 * t + 32 * s2);
    }
  }
  // epilogue state: a flush thread always owns the 8-column chunk c = tid % 8
  constexpr int CPR = BN / 8, KC = 128 * BN / 8 / 256;
  const int cc = tid % CPR, ncol = n0 + 8 * cc;
  float mu[8], sc[8], sh[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    mu[i] = (BWD && e.mean) ? e.mean[ncol + i] : 0.f;
    sc[i] = (BWD && e.msc) ? e.msc[ncol + i] : 0.f;
    sh[i] = (BWD && e.msh) ? e.msh[ncol + i] : 0.f;
  }
  __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));  // (once per kernel: no vmcnt waits for them inside the loop)
  issue_tile(0);
  if (my_tiles > 1) issue_tile(1);

  const bool mask = BWD && e.msc != nullptr && e.y != nullptr;
  float b1[8], b2[8], b3[8];  // EPI_STATS: shift, sum (v - shift), sum (v - shift)^2; EPI_BWD_AFF: sum g, sum g (y - mean)
  int scnt = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) b1[i] = b2[i] = b3[i] = 0.f;
  // The epilogue of tile lt is split: its output round is staged and read back into q (and the y chunks into yq)
  // at the end of the tile; the stores and statistics of chunk k run inside tile lt + 1's MFMA stream (unit
  // 2k + 1), and the last tile's after the loop.
  uint4 q[KC], yq[KC];
  int pm0 = 0, pmlim = 0;  // rows of the tile held in q
  auto process = [&](int k) {
    const int m = pm0 + (tid + 256 * k) / CPR;
    if (m >= pmlim) return;
    uint4* dst = reinterpret_cast<uint4*>(Cout + (long long)m * p.ldc + ncol);
    if constexpr (EPI == EPI_STORE) {
      *dst = q[k];
    } else if constexpr (EPI == EPI_STATS) {
      *dst = q[k];
      float v[8];
      unpack8(q[k], v);
      if (scnt == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) b1[i] = v[i];
      }
      ++scnt;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = v[i] - b1[i];
        b2[i] += d;
        b3[i] = fmaf(d, d, b3[i]);
      }
    } else {  // g = mask(dgrad) stored; BN sums of the stored (rounded) g against y
      float v[8], yy[8];
      unpack8(q[k], v);
      unpack8(yq[k], yy);
      if (mask) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = fmaf(yy[i], sc[i], sh[i]) > 0.f ? v[i] : 0.f;
      }
      const uint4 o = pack8(v);
      *dst = o;
      if (e.nred > 0) {
        unpack8(o, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          b1[i] += v[i];
          b2[i] = fmaf(v[i], yy[i] - mu[i], b2[i]);
        }
      }
    }
  };

  for (int lt = 0; lt < my_tiles; ++lt) {
    // tile lt's DMAs have landed for every wave (tile lt + 1's, issued after them, may still be in flight)
    PATCH_STAMP(0);
    if (lt + 1 < my_tiles) __builtin_amdgcn_s_waitcnt(waitcnt_vm(NIP));
    else __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
    __builtin_amdgcn_s_barrier();
    PATCH_STAMP(1);
    // tile lt + 2's DMAs go out one piece per unit, into the ring slot of tile lt - 1 (free: its q / yq reads
    // completed before the barrier above)
    const bool pre = lt + 2 < my_tiles;
    const int tg2 = by + (lt + 2) * gy, img2 = tg2 / g.TPI, h02 = (tg2 - img2 * g.TPI) * g.R;
    const bool prev = lt > 0;
    PATCH_STAMP(2);
    const bf16_t* P = Ps + (lt % PATCH_RING) * PE;
    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // 18 units (tap t = u / 2, k-step u % 2) of 4 fragment reads + 8 MFMAs, reads issued two units ahead (a ring
    // of 3 fragment sets; the scheduler barriers keep hipcc from regrouping them into read-wait-MFMA pairs, whose
    // exposed LDS latency made the first build of this loop 4x slower than its MFMA time)
    // fragment addresses of this tile: column tap c (= kw, dgrad 2 - kw), k-step s2; row taps add kh' PW pixels
    uint32_t fa[MT][3][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int pix = rowpix[i] + c;
        const uint32_t a0 = lds_u32(P + pix * 64 + 8 * pswz(pix, lane >> 4));
        fa[i][c][0] = a0;
        fa[i][c][1] = a0 ^ 64u;  // chunk + 4: slot (c + 4 + x) & 7 = ((c + x) & 7) ^ 4
      }
    auto unit_reads = [&](s16x8 (&f)[MT], int u) {
      const int t = u >> 1, kh = t / 3, kw = t - 3 * (t / 3);
      const int rh = DG ? 2 - kh : kh, cw = DG ? 2 - kw : kw;
#pragma unroll
      for (int i = 0; i < MT; ++i)
        f[i] = *reinterpret_cast<const __attribute__((address_space(3))) s16x8*>(
            (const lds_char*)(uintptr_t)fa[i][cw][u & 1] + rh * PW * 128);
    };
    s16x8 af[3][MT];
    unit_reads(af[0], 0);
    unit_reads(af[1], 1);
#pragma unroll
    for (int u = 0; u < 18; ++u) {
      if (u + 2 < 18) unit_reads(af[(u + 2) % 3], u + 2);
      if (u < NIP && pre) issue_piece(lt + 2, tg2, img2, h02, u);
      // the previous tile's stores / statistics in units after the DMA issues (both are expensive beside the MFMAs:
      // the dgrad epilogue's ~60 VALU per chunk exceeds a unit's MFMA shadow)
      if constexpr (NIP + 2 * KC <= 18) {
        if (u >= NIP && ((u - NIP) & 1) == 0 && ((u - NIP) >> 1) < KC && prev) process((u - NIP) >> 1);
      } else {
        if (u >= 18 - KC && prev) process(u - (18 - KC));
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(breg[u >> 1][u & 1][j], af[u % 3][i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    PATCH_STAMP(3);
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): every wave's fragment reads are back before the staging
    __builtin_amdgcn_s_barrier();
    PATCH_STAMP(4);
    // stage the round in this tile's patch slot, read this thread's chunks (and y chunks) back
    bf16_t* stA = Ps + (lt % PATCH_RING) * PE;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
        stage_put<BN>(stA, stA, wm, wn, lane, i, j, v);
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const bf16_t* Y = Ys + (lt % PATCH_RING) * YE;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const int trow = (tid + 256 * k) / CPR;
      asm volatile("ds_read_b128 %0, %1" : "=v"(q[k]) : "v"(lds_u32(stA + trow * BN + 8 * st_slot<BN>(trow, cc))) : "memory");
      if constexpr (BWD)
        asm volatile("ds_read_b128 %0, %1" : "=v"(yq[k]) : "v"(lds_u32(Y + trow * 64 + 8 * cc)) : "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    pm0 = (by + lt * gy) * g.TM;
    pmlim = pm0 + g.TM;
    PATCH_STAMP(5);
  }
#pragma unroll
  for (int k = 0; k < KC; ++k) process(k);
  __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
  if constexpr (EPI == EPI_STATS)
    stats_finish<BN>(p, reinterpret_cast<float*>(smem), scnt, b1, b2, b3, n0, by, bx, gy, (p.M + 127) / 128);
  if constexpr (BWD) {
    if (e.nred > 0) {
      float* inv = reinterpret_cast<float*>(smem) + 3 * 256 * 8;  // beyond bwd_finish's scratch
      __syncthreads();
      if (tid < BN) inv[tid] = e.invstd ? e.invstd[n0 + tid] : 0.f;
      bwd_finish<256, BN>(p, reinterpret_cast<float*>(smem), inv, b1, b2, b3, n0, by);
    }
  }
}

// ---- the pair-packed stem (7x7 / stride 2 / pad 3 over RGB0 bf16 frames, vcg_conv_fwd's C = 4 layout) --------
// Same scheme as the layer-1 patch kernel: an M-tile is R whole output rows of one image; its input rows
// (2R + KH - 2 rows of OW + KWp - 1 super pixels, 16 B = two RGB0 pixels each) are one LDS-DMA patch, and the
// KH k-units (4 taps each: the super-pixel pairs kwp = 0..3 of filter row kh) read fragments straight from it:
// lane group g = kwp, so a fragment read is 16 consecutive super pixels (contiguous 256 B, conflict-free). The
// im2col engine gathers every input super pixel ~14 times through L2. The filter (64 x 224) stays in registers
// (14 fragments per lane), 2 workgroups per CU, a 3-deep patch ring, the deferred epilogue of the patch kernel.
constexpr int SPATCH_MAXPIX = 1024;  // super pixels per patch buffer (16 KiB)

struct StemGeom {
  int R, TM, TPI, PW, NP, NS, NR;  // rows / GEMM rows per tile, tiles per image, patch width, pixels, slices, rows
  unsigned long long* stamps;
};

template <int EPI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void stem_patch_kernel(GemmParams p, StemGeom g) {
  constexpr int BM = 128, BN = 64, NW = 4, MT = 4, NT = 2, KHMAX = 8, RING = 3, NIP = 4;
  constexpr int PE = SPATCH_MAXPIX * 8;  // elements per patch buffer
  __shared__ __attribute__((aligned(1024))) char smem[RING * PE * 2];
  bf16_t* Ps = reinterpret_cast<bf16_t*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nx = p.N / BN, gy = gridDim.x / nx;
  int bx, by;
  xcd_row_decode(nx, gy, bx, by);
  const int n0 = bx * BN;
  bf16_t* Cout = reinterpret_cast<bf16_t*>(p.C);
  const int mtiles = p.M / g.TM;
  const int my_tiles = by < mtiles ? (mtiles - 1 - by) / gy + 1 : 0;
  if (my_tiles == 0) return;

  const OpArgs& a = p.a;  // a.W: super pixels per image row, a.C = 8, a.KW = 4 super-pixel taps, a.pw their pad
  const int KH = a.KH;
  const uint32_t nbytes = (uint32_t)min(a.bytes, (long long)0xFFFFFF00LL);
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.ptr), 0, nbytes, 0x00020000);
  // piece q < NIP of tile lt: 64 super pixels (slice wave + 4 q, repeated past NS - 1: fixed count per wave)
  auto issue_piece = [&](int lt, int img, int h0, int q) {
    bf16_t* dst = Ps + (lt % RING) * PE;
    const int slice = min(wave + NW * q, g.NS - 1);
    const int pix = 64 * slice + lane;
    const int pr = pix / g.PW, pc = pix - pr * g.PW;
    const int ih = 2 * h0 - a.pad + pr, sx = pc - a.pw;
    const bool ok = pix < g.NP && (unsigned)ih < (unsigned)a.H && (unsigned)sx < (unsigned)a.W;
    const uint32_t voff = ok ? (uint32_t)((((img * a.H + ih) * a.W + sx) << 3) * 2) : nbytes;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void_t*)(dst + slice * 512), 16, voff, 0, 0, 0);
  };
  auto issue_tile = [&](int lt) {
    const int tg = by + lt * gy, img = tg / g.TPI, h0 = (tg - img * g.TPI) * g.R;
#pragma unroll
    for (int q = 0; q < NIP; ++q) issue_piece(lt, img, h0, q);
  };
  int rowpix[MT];  // patch super pixel of tap (kh = 0, kwp = 0) for this lane's fragment row
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int ml = wm * 64 + i * 16 + (lane & 15);
    const int r = ml / a.GW, w = ml - r * a.GW;
    rowpix[i] = ml < g.TM ? 2 * r * g.PW + w : 0;
  }
  // B fragment of filter row kh, column group j: k = 32 kh + 8 (lane / 16) (taps kwp = lane / 16 of row kh)
  s16x8 breg[KHMAX][NT];
  {
    const bf16_t* B = reinterpret_cast<const bf16_t*>(p.b.ptr);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const bf16_t* row = B + (long long)(n0 + wn * (BN / 2) + j * 16 + (lane & 15)) * p.b.ld + 8 * (lane >> 4);
#pragma unroll
      for (int kh = 0; kh < KHMAX; ++kh)
        breg[kh][j] = kh < KH ? *reinterpret_cast<const s16x8*>(row + 32 * kh) : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  constexpr int CPR = BN / 8, KC = 128 * BN / 8 / 256;
  const int cc = tid % CPR, ncol = n0 + 8 * cc;
  __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));  // register loads retired before the first DMA (see the patch kernel)
  issue_tile(0);
  if (my_tiles > 1) issue_tile(1);

  float b1[8], b2[8], b3[8];
  int scnt = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) b1[i] = b2[i] = b3[i] = 0.f;
  uint4 q[KC];
  int pm0 = 0, pmlim = 0;
  auto process = [&](int k) {
    const int m = pm0 + (tid + 256 * k) / CPR;
    if (m >= pmlim) return;
    *reinterpret_cast<uint4*>(Cout + (long long)m * p.ldc + ncol) = q[k];
    if constexpr (EPI == EPI_STATS) {
      float v[8];
      unpack8(q[k], v);
      if (scnt == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) b1[i] = v[i];
      }
      ++scnt;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = v[i] - b1[i];
        b2[i] += d;
        b3[i] = fmaf(d, d, b3[i]);
      }
    }
  };

  for (int lt = 0; lt < my_tiles; ++lt) {
    if (lt + 1 < my_tiles) __builtin_amdgcn_s_waitcnt(waitcnt_vm(NIP));
    else __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
    __builtin_amdgcn_s_barrier();
    const bool pre = lt + 2 < my_tiles;
    const int tg2 = by + (lt + 2) * gy, img2 = tg2 / g.TPI, h02 = (tg2 - img2 * g.TPI) * g.R;
    const bool prev = lt > 0;
    const bf16_t* P = Ps + (lt % RING) * PE;
    // opaque per tile: keeps hipcc from hoisting the loop-invariant fragment addresses (registers)
#pragma unroll
    for (int i = 0; i < MT; ++i) asm volatile("" : "+v"(rowpix[i]));
    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto unit_reads = [&](s16x8 (&f)[MT], int kh) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
        f[i] = *reinterpret_cast<const s16x8*>(P + (rowpix[i] + kh * g.PW + (lane >> 4)) * 8);
    };
    s16x8 af[3][MT];
    unit_reads(af[0], 0);
    unit_reads(af[1], 1);
#pragma unroll
    for (int u = 0; u < KHMAX; ++u) {
      if (u < KH) {
        if (u + 2 < KH) unit_reads(af[(u + 2) % 3], u + 2);
        if (u < NIP && pre) issue_piece(lt + 2, img2, h02, u);
        if (u >= 1 && u - 1 < KC && prev) process(u - 1);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(breg[u][j], af[u % 3][i], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (prev) {  // chunks not yet processed when KH - 1 < KC
#pragma unroll
      for (int k = 0; k < KC; ++k)
        if (k >= KH - 1) process(k);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    bf16_t* stA = Ps + (lt % RING) * PE;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
        stage_put<BN>(stA, stA, wm, wn, lane, i, j, v);
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const int trow = (tid + 256 * k) / CPR;
      asm volatile("ds_read_b128 %0, %1" : "=v"(q[k]) : "v"(lds_u32(stA + trow * BN + 8 * st_slot<BN>(trow, cc))) : "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    pm0 = (by + lt * gy) * g.TM;
    pmlim = pm0 + g.TM;
  }
#pragma unroll
  for (int k = 0; k < KC; ++k) process(k);
  __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
  if constexpr (EPI == EPI_STATS)
    stats_finish<BN>(p, reinterpret_cast<float*>(smem), scnt, b1, b2, b3, n0, by, bx, gy, (p.M + 127) / 128);
}

// Rows per stem tile (0: not the pair-packed 7x7 / 2 stem shape the stem kernel handles)
static int stem_rows(const GemmParams& p) {
  const char* e = getenv("VCG_NO_PATCH");
  const OpArgs& a = p.a;
  if ((e && e[0] == '1') || a.C != 8 || a.sw != 1 || a.KW != 4 || a.stride != 2 || a.KH > 8 || a.KH < 3 ||
      p.K != a.KH * 32 || a.tsm_fold != 0 || p.N % 64 != 0 || p.batch_inner > 0 || p.residual || p.aux || p.bias ||
      p.act != ACT_NONE || a.GW > 128 || a.GW + 3 > SPATCH_MAXPIX)
    return 0;
  for (int R = min(a.GH, 128 / a.GW); R >= 1; --R)
    if (a.GH % R == 0 && (2 * R + a.KH - 2) * (a.GW + 3) <= SPATCH_MAXPIX) return R;
  return 0;
}

static StemGeom stem_geom(const GemmParams& p, int R) {
  StemGeom g{};
  g.R = R;
  g.TM = R * p.a.GW;
  g.TPI = p.a.GH / R;
  g.PW = p.a.GW + p.a.KW - 1;
  g.NR = 2 * R + p.a.KH - 2;
  g.NP = g.NR * g.PW;
  g.NS = (g.NP + 63) / 64;
  return g;
}

// Patch row pitch in pixels (the kernel's PW): 32 or 64 >= W + 2 (the two zero border columns)
static int patch_pitch(int W) { return W + 2 <= 32 ? 32 : 64; }

// Rows per patch tile (0: the patch kernel does not apply). VCG_NO_PATCH=1 keeps these convs on the im2col path.
static int patch_rows(const GemmParams& p, int amode) {
  const char* e = getenv("VCG_NO_PATCH");  // read per call: a test compares both paths in one process
  const bool off = e && e[0] == '1';
  const OpArgs& a = p.a;
  if (off || (amode != OP_IM2COL && amode != OP_DGRAD) || a.C != 64 || a.KH != 3 || a.KW != 3 || a.stride != 1 ||
      a.pad != 1 || a.tsm_fold != 0 || a.tKW != 0 || a.sw != 0 || a.GH != a.H || a.GW != a.W || p.N % 64 != 0 ||
      p.K != 9 * 64 || p.batch_inner > 0 || p.residual || p.aux || p.bias || p.act != ACT_NONE || a.W + 2 > 64 ||
      !bwd_light(p) || p.bwd.nred > 2)
    return 0;
  for (int R = min(a.H, 128 / a.W); R >= 1; --R)
    if (a.H % R == 0 && (R + 2) * patch_pitch(a.W) <= PATCH_MAXPIX) return R;
  return 0;
}

static PatchGeom patch_geom(const GemmParams& p, int R) {
  PatchGeom g{};
  g.R = R;
  g.TM = R * p.a.W;
  g.TPI = p.a.H / R;
  g.PW = patch_pitch(p.a.W);
  g.NP = (R + 2) * g.PW;
  g.NS = (g.NP + 7) / 8;
  return g;
}

// one resident round (1 workgroup per CU); gy <= the 128-row slot count of the EPI_STATS buffer
static int patch_grid_rows(const GemmParams& p, const PatchGeom& g) {
  const int nx = p.N / 64, mtiles = p.M / g.TM;
  int gy = 256 / nx;
  gy = min(gy, min(mtiles, (p.M + 127) / 128));
  if (gy >= 8) gy &= ~7;
  return max(gy, 1);
}

static unsigned long long* g_patch_stamps = nullptr;

template <int EPI, bool DG, int PW>
static int launch_patch(const GemmParams& p, int R, hipStream_t s) {
  const PatchGeom g = patch_geom(p, R);
  const int gy = patch_grid_rows(p, g);
  const int tk = timing_begin(s);
  PatchGeom gs = g;
  const char* st = getenv("VCG_PATCH_STAMPS");
  if (st && st[0] == '1') {
    if (!g_patch_stamps && hipMalloc(&g_patch_stamps, 64 * 6 * 8) != hipSuccess) g_patch_stamps = nullptr;
    gs.stamps = g_patch_stamps;
  }
  hipLaunchKernelGGL((conv3x3_patch_kernel<EPI, DG, PW>), dim3((p.N / 64) * gy), dim3(256), 0, s, p, gs);
  if (census_on()) { char t_[96]; snprintf(t_, sizeof(t_), "conv3x3_patch e%d dg%d pw%d", EPI, (int)DG, PW); census_add(t_, p.M, p.N, p.K); }
  timing_end(tk, s, TIMING_PATCH_CONV, 2.0 * p.M * p.N * (double)p.K, algorithmic_bytes<OP_IM2COL, EPI, false>(p, 1));
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

template <int EPI>
static int launch_stem(const GemmParams& p, int R, hipStream_t s) {
  const StemGeom g = stem_geom(p, R);
  const int nx = p.N / 64, mtiles = p.M / g.TM;
  int gy = min((2 * 256) / nx, min(mtiles, (p.M + 127) / 128));
  if (gy >= 8) gy &= ~7;
  gy = max(gy, 1);
  const int tk = timing_begin(s);
  hipLaunchKernelGGL((stem_patch_kernel<EPI>), dim3(nx * gy), dim3(256), 0, s, p, g);
  if (census_on()) { char t_[96]; snprintf(t_, sizeof(t_), "stem_patch e%d", EPI); census_add(t_, p.M, p.N, p.K); }
  timing_end(tk, s, TIMING_PATCH_CONV, 2.0 * p.M * p.N * (double)p.K, algorithmic_bytes<OP_IM2COL, EPI, false>(p, 1));
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

int patch_bwd_slots(const GemmParams& p) {
  const int R = patch_rows(p, OP_DGRAD);
  return R > 0 ? patch_grid_rows(p, patch_geom(p, R)) : 0;
}

int run_patch_conv(const GemmParams& p, int amode, int epi, hipStream_t s) {
  if (amode == OP_IM2COL_SMALLC && (epi == EPI_STATS || epi == EPI_STORE)) {
    const int R = stem_rows(p);
    if (R > 0) return epi == EPI_STATS ? launch_stem<EPI_STATS>(p, R, s) : launch_stem<EPI_STORE>(p, R, s);
  }
  const int R = patch_rows(p, amode);
  if (R <= 0) return -1;
  const bool w64 = patch_pitch(p.a.W) == 64;
  if (amode == OP_DGRAD) {
    if (epi == EPI_BWD)  // (patch_rows: light epilogues only)
      return w64 ? launch_patch<EPI_BWD_AFF, true, 64>(p, R, s) : launch_patch<EPI_BWD_AFF, true, 32>(p, R, s);
    if (epi == EPI_STATS)
      return w64 ? launch_patch<EPI_STATS, true, 64>(p, R, s) : launch_patch<EPI_STATS, true, 32>(p, R, s);
    if (epi == EPI_STORE)
      return w64 ? launch_patch<EPI_STORE, true, 64>(p, R, s) : launch_patch<EPI_STORE, true, 32>(p, R, s);
  } else {
    if (epi == EPI_STATS)
      return w64 ? launch_patch<EPI_STATS, false, 64>(p, R, s) : launch_patch<EPI_STATS, false, 32>(p, R, s);
    if (epi == EPI_STORE)
      return w64 ? launch_patch<EPI_STORE, false, 64>(p, R, s) : launch_patch<EPI_STORE, false, 32>(p, R, s);
  }
  return -1;
}

}  // namespace vcg

// Profiling aid: the phase stamps (s_memtime) of the last patch-conv launch with VCG_PATCH_STAMPS=1, workgroup 0
// wave 0, 6 per tile (top, after wait+barrier, after DMA issue, after MFMAs, after barrier, after epilogue).
VCG_API int vcg_patch_stamps(unsigned long long* out, int n) {
  if (!vcg::g_patch_stamps) return 1;
  n = n < 64 * 6 ? n : 64 * 6;
  return hipMemcpy(out, vcg::g_patch_stamps, (size_t)n * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
}
