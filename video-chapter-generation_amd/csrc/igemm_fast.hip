// bf16 fast path of the implicit-GEMM engine for K-contiguous operands
// (conv fwd with im2col/TSM gather, conv dgrad gather, dense linear layers / QK^T).
//
// Differences to the generic kernel (igemm.hip):
//   * BK = 64 (two 16x16x32 MFMA k-steps per barrier pair);
//   * operands go global -> LDS directly with buffer_load ... lds (LDS-DMA, 16 B per lane,
//     1 KiB per wave instruction, no VGPR staging); conv zero padding / out-of-range rows come for
//     free from the buffer descriptor's range check (out-of-range offset -> zeros);
//   * LDS tile [rows][64] bf16 with 128-B rows, 16-B chunk c of row r at slot c ^ ((r >> 1) & 7):
//     the global source address is pre-swizzled (LDS stays lane-linear, as LDS-DMA requires) and
//     the fragment ds_read_b64s of a 32-lane half hit 64 distinct banks;
//   * two LDS stages; tile t+1 is in flight while tile t is computed; counted vmcnt + raw
//     s_barrier (never __syncthreads, which would drain the in-flight DMA).
#include "fast_epilogue.h"

// Profiling build (make EXTRA=-DVCG_FAST_STAMPS OUT=... OBJDIR=...): s_memtime per tile phase of workgroup 0,
// wave 0 of every igemm_fast launch (the last launch's survive): tile's first k-step, after its last MFMAs,
// after the output staging, after the epilogue flush. vcg_fast_stamps() copies them out.
// (Defined before bwd_stream.h, whose bodies stamp their phases too.)
#ifdef VCG_FAST_STAMPS
namespace vcg { __device__ unsigned long long g_fast_stamps[64 * 4]; }
#define FAST_STAMP(t, k)                                                                       \
  do {                                                                                         \
    if (blockIdx.x == 0 && threadIdx.x == 0 && (t) < 64) vcg::g_fast_stamps[(t) * 4 + (k)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define FAST_STAMP(t, k) do {} while (0)
#endif

#include "bwd_stream.h"

namespace vcg {

template <int BN, int AM, int EPI, int RES>
__device__ __forceinline__ void igemm_fast_body(const GemmParams& p) {
  // Persistent-style grid: workgroup (bx, by) owns N-tile bx and M-tiles by, by + gy, by + 2gy, ...;
  // the (m-tile, k-tile) steps form one software pipeline, so the next tiles' loads are in flight while
  // a tile finishes its MFMAs and its epilogue. Workgroups are dealt round-robin to the 8 XCDs by
  // linear id, so when gy % 8 == 0 the linear id is decoded such that all N-tiles of an M-tile
  // row run on the same XCD at the same time and the A rows are fetched from HBM once (L2 hits).
  // The bias lives in registers for the whole kernel (loaded before the pipeline starts) and the
  // epilogue (RES = false) loads nothing: a VGPR-destination global load inside the loop, or an LDS
  // object the compiler cannot tell apart from the DMA target, makes hipcc drain the in-flight
  // LDS-DMA prefetch with vmcnt(0) at every tile boundary. Conv (EPI_STATS) GEMMs carry no bias.
  //
  // Shapes: 128-row tiles, 4 waves (2 along M x 2 along N), every wave owns a 64 x BN/2 sub-tile (4 x BN/32
  // fragments of 16x16); 2 LDS stages (1 step in flight), 2 workgroups per CU.
  constexpr int BM = 128, NW = 4;
  constexpr int MT = 4, NT = BN / 32;
  constexpr int AE = BM * FBK, BE = BN * FBK;  // elements per stage
  constexpr int NLD = BM / (8 * NW) + BN / (8 * NW);  // LDS-DMA instructions per thread per step
  constexpr bool BWD = EPI == EPI_BWD || EPI == EPI_BWD_AFF;
  constexpr int CPAR = BWD ? 6 * BN : 0;  // EPI_BWD per-column parameters
  constexpr int RED = 4 * BN + 2 + 4;
  __shared__ __attribute__((aligned(1024))) char smem[2 * (AE + BE) * 2 + (RED + CPAR) * 4];
  bf16_t* As = reinterpret_cast<bf16_t*>(smem);
  bf16_t* Bs = As + 2 * AE;
  float* red = reinterpret_cast<float*>(smem + 2 * (AE + BE) * 2);
  float* cpar = red + RED;  // [mean, msc, msh, mean2, invstd, invstd2][BN]

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nx = (p.N + BN - 1) / BN, gy = gridDim.x / nx;
  int bx, by;
  xcd_row_decode(nx, gy, bx, by);
  const int n0 = bx * BN;
  long long aoff = 0, boff = 0;
  bf16_t* Cout = reinterpret_cast<bf16_t*>(p.C);
  const bf16_t* Res = RES ? reinterpret_cast<const bf16_t*>(p.residual) : nullptr;
  if (p.batch_inner > 0) {
    const int zo = blockIdx.z / p.batch_inner, zi = blockIdx.z - zo * p.batch_inner;
    aoff = zo * p.a_so + zi * p.a_si;
    boff = zo * p.b_so + zi * p.b_si;
    Cout += zo * p.c_so + zi * p.c_si;
    if (Res) Res += zo * p.c_so + zi * p.c_si;
  }
  const int mtiles = (p.M + BM - 1) / BM;
  const int my_tiles = by < mtiles ? (mtiles - 1 - by) / gy + 1 : 0;
  const int ntiles = (p.K + FBK - 1) / FBK;
  const int steps = my_tiles * ntiles;
  if constexpr (BWD) {
    if (steps == 0) {  // no rows: an all-zero partial slot
      if (p.bwd.nred > 0 && tid < BN && n0 + tid < p.N)
        for (int r = 0; r < p.bwd.nred; ++r) p.bwd.part[((long long)by * p.bwd.nred + r) * p.N + n0 + tid] = 0.f;
      return;
    }
    if (tid < BN) {
      const int n = min(n0 + tid, p.N - 1);
      const BwdEpi& e = p.bwd;
      cpar[tid] = e.mean ? e.mean[n] : 0.f;
      cpar[BN + tid] = e.msc ? e.msc[n] : 0.f;
      cpar[2 * BN + tid] = e.msh ? e.msh[n] : 0.f;
      cpar[3 * BN + tid] = e.mean2 ? e.mean2[n] : 0.f;
      cpar[4 * BN + tid] = e.invstd ? e.invstd[n] : 0.f;
      cpar[5 * BN + tid] = e.invstd2 ? e.invstd2[n] : 0.f;
    }
  }
  if (steps == 0) return;

  float bv[NT][4];
  if constexpr (EPI == EPI_STATS) {
#pragma unroll
    for (int j = 0; j < NT; ++j) bv[j][0] = bv[j][1] = bv[j][2] = bv[j][3] = 0.f;
  } else {
    load_bias<BN>(bv, p.bias, n0, wn, lane, p.N);
#pragma unroll
    for (int j = 0; j < NT; ++j) asm volatile("" ::"v"(bv[j][0]), "v"(bv[j][1]), "v"(bv[j][2]), "v"(bv[j][3]));
  }

  FastLoader<BM, AM, NW> la;
  FastLoader<BN, OP_DENSE_K, NW> lb;
  la.init(p.a, aoff, by * BM, wave, lane);
  lb.init(p.b, boff, n0, wave, lane);

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // EPI_STATS: shifted per-column sums over every row this workgroup stores, across all of its M-tiles,
  // merged once at the end -> one (mean, M2) slot per workgroup row `by` (stage_flush_stats, stats_finish).
  float b1[8], b2[8], b3[8];  // EPI_BWD column sums / EPI_STATS shift, s1, s2 of this thread's chunk
  int scnt = 0;               // EPI_STATS rows seen by this thread
#pragma unroll
  for (int i = 0; i < 8; ++i) b1[i] = b2[i] = b3[i] = 0.f;

  // issue side of the pipeline: the next step to load is k-tile ikt of the workgroup's local tile itile
  int ikt = 0, itile = 0;
  auto issue_next = [&](int stage) {
    if (ikt == 0 && itile > 0) la.init(p.a, aoff, (by + itile * gy) * BM, wave, lane);
    la.issue(p.a, ikt * FBK, p.K, As + stage * AE, wave);
    lb.issue(p.b, ikt * FBK, p.K, Bs + stage * BE, wave);
    if (++ikt == ntiles) {
      ikt = 0;
      ++itile;
    }
  };
  issue_next(0);
  int kt = 0, tile = 0, cur = 0;
  for (int s = 0; s < steps; ++s) {
    // step s + 1 goes into the other stage; step s has landed when only that step's loads are outstanding
    if (s + 1 < steps) {
      issue_next(cur ^ 1);
      __builtin_amdgcn_s_waitcnt(waitcnt_vm(NLD));
    } else {
      __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
    }
    __builtin_amdgcn_s_barrier();
    if (kt == 0) FAST_STAMP(tile, 0);
    const bf16_t* Ac = As + cur * AE;
    const bf16_t* Bc = Bs + cur * BE;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      s16x8 af[MT], bfr[NT];
#pragma unroll
      for (int i = 0; i < MT; ++i) af[i] = fast_frag(Ac, wm * 64 + i * 16, lane, s2);
#pragma unroll
      for (int j = 0; j < NT; ++j) bfr[j] = fast_frag(Bc, wn * (BN / 2) + j * 16, lane, s2);
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
    }
    // every wave's ds_reads of this stage have returned before any wave refills it (WAR)
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) only
    __builtin_amdgcn_s_barrier();
    if (++kt == ntiles) {
      FAST_STAMP(tile, 1);
      const int mt = by + tile * gy;
      bf16_t* stA = As + cur * AE;  // the finished stage holds the output tile (see stage_put)
      bf16_t* stB = Bs + cur * BE;
      // every output tile goes through the LDS stage for full-row 16-B stores
      if constexpr (BWD) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int i = 0; i < MT; ++i) {
            float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            if constexpr (AM == OP_DENSE_K2) {  // the folded BN's constant term, before the bf16 rounding
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] += bv[j][r];
            }
            stage_put<BN>(stA, stB, wm, wn, lane, i, j, v);
          }
        FAST_STAMP(tile, 2);
        stage_flush_bwd<BN, EPI == EPI_BWD_AFF>(stA, stB, p, Cout, mt * BM, n0, cpar, b1, b2, b3, p.M);
      } else if constexpr (EPI == EPI_STATS) {  // conv outputs: no bias / activation, alpha = 1
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int i = 0; i < MT; ++i) {
            float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            stage_put<BN>(stA, stB, wm, wn, lane, i, j, v);
          }
        stage_flush_stats<BN>(stA, stB, p, Cout, mt * BM, n0, scnt, b1, b2, b3, p.M);
      } else if constexpr (EPI == EPI_STORE_AUX) {
        epilogue_staged_aux<BN>(acc, p, bv, Cout, stA, stB, mt * BM, n0, wm, wn, lane);
      } else if (!RES && p.aux == nullptr && (p.ldc & 7) == 0 && ((uintptr_t)p.C & 15) == 0) {
        epilogue_staged<BN>(acc, p, bv, Cout, stA, stB, mt * BM, n0, wm, wn, lane, p.M);
      } else if (RES && p.aux == nullptr && (RES >= 2 ? !p.res_sc : (p.res_round && p.act == ACT_RELU)) &&
                 ((p.ldc | p.ldr | p.N) & 7) == 0 && (((uintptr_t)p.residual | (uintptr_t)p.C) & 15) == 0) {
        if constexpr (RES)
          epilogue_staged_res<BN, RES >= 2 ? RES - 1 : 0>(acc, p, bv, Cout, Res, stA, stB, mt * BM, n0, wm, wn, lane, p.M);
      } else {
        gemm_epilogue<bf16_t, BM, BN, EPI>(acc, p, red, bv, Cout, Res, mt * BM, n0, wm, wn, lane, mt, mtiles);
      }
      FAST_STAMP(tile, 3);
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      kt = 0;
      ++tile;
    }
    cur ^= 1;
  }
  if constexpr (EPI == EPI_STATS)  // the stats buffer is laid out for 128-row tiles (vcg_conv_stats_tiles)
    stats_finish<BN>(p, reinterpret_cast<float*>(smem), scnt, b1, b2, b3, n0, by, bx, gy, (p.M + 127) / 128);
  if constexpr (BWD) {
    if (p.bwd.nred > 0) bwd_finish<2 * BM, BN>(p, reinterpret_cast<float*>(smem), cpar + 4 * BN, b1, b2, b3, n0, by);
  }
}

// The kernel: EPI_BWD_STREAM has its own tile schedules (bwd_stream.h; AM = K / 64, XF = its operand flags, BM = 256
// only asks for its 512 threads), every other epilogue runs the persistent 2-stage pipeline above on 128-row tiles.
template <int BM, int BN, int AM, int EPI, int RES, int XF = 0>
__global__ __launch_bounds__(BM * 2) __attribute__((amdgpu_waves_per_eu(EPI == EPI_BWD_AFF && BN == 64 ? 3 : 2)))
void igemm_fast_kernel(GemmParams p) {
  if constexpr (EPI == EPI_BWD_STREAM && BN == 128) {
    bwd_stream128_body<XF>(p);
  } else if constexpr (EPI == EPI_BWD_STREAM) {
    bwd_stream_body<AM, XF>(p);
  } else {
    static_assert(BM == 128, "the persistent engine runs 128-row tiles");
    igemm_fast_body<BN, AM, EPI, RES>(p);
  }
}

// One resident round of workgroups (LDS allows 2 per CU at BN = 128, 3 at BN = 64); each walks
// ceil(mtiles / gy) 128-row M-tiles. gy is a multiple of 8 whenever possible (XCD-aware decode).
// (EPI_BWD's BN = 64 kernel needs > 170 VGPRs: 2 workgroups per CU there too; EPI_BWD_AFF's fits 3)
// (A 256-row 3-stage variant of this engine measured slower than two 4-wave 128-row workgroups per CU on every conv
// shape and was removed; the 256 x 256 8-wave engine is igemm256.hip.)
static int grid_rows(int M, int N, int z, int BN, int epi) {
  const int nx = (N + BN - 1) / BN, mtiles = (M + 127) / 128;
  const int resident = (BN == 128 || epi == EPI_BWD ? 2 : 3) * 256;
  int gy = resident / (nx * z);
  if (gy >= 8) gy &= ~7;
  if (gy > mtiles) gy = mtiles >= 8 ? (mtiles & ~7) : mtiles;
  if (gy < 1) gy = 1;
  return gy;
}

static int fast_bn_cols(int N) { return (N % 128 == 0 || N > 64 * 3) ? 128 : 64; }

int fast_grid_rows(int M, int N, int z, int epi) { return grid_rows(M, N, z, fast_bn_cols(N), epi); }

// EPI_BWD_STREAM applies to a full EPI_BWD (residual; mask bits with y, or neither) of a dense 1x1 dgrad with
// K = 64, 128 or 256 (256: every 64-column tile inside one TSM shift); VCG_BWD_STREAM=0 keeps it on the persistent
// engine (read per call: tests compare both paths)
static bool bwd_stream_ok(const GemmParams& p) {
  const char* v = getenv("VCG_BWD_STREAM");
  if (v && v[0] == '0') return false;
  const BwdEpi& e = p.bwd;
  const bool dense = p.a.KH == 0 && p.a.GH == 0;  // dense_op(): no conv geometry
  if (!dense || (p.K != 64 && p.K != 128 && p.K != 256) || p.N % 64 != 0 || p.batch_inner > 0 || p.ldc != p.N || p.a.ld != p.K ||
      !e.res || e.msc || e.sub || bwd_light(p))
    return false;
  if ((e.y && !e.bits) || (e.y2 && !e.y)) return false;
  if ((e.y || e.bits) && e.nred < 2) return false;
  if (e.tsm_T > 0 && e.tsm_fold % 32 != 0) return false;  // one TSM shift per wave's 32 columns
  // K = 256: one A tile per slot and 3 slots; with y the 64 x 64 form measured slower than the persistent engine
  // (tools/bench_dgrad.py: 400.6 vs 385.1 us at layer 3), so only the mask-bits-only epilogues stream
  if (p.K == 256 && ((e.tsm_T > 0 && e.tsm_fold % 64 != 0) || e.y)) return false;
  if (p.K == 256 && ((uintptr_t)p.b.ptr & 15 || p.b.ld % 8 != 0)) return false;  // 16-B weight fragment loads
  if (((uintptr_t)p.C | (uintptr_t)e.res | (uintptr_t)e.y | (uintptr_t)e.y2 | (uintptr_t)p.a.ptr) & 15) return false;
  if (e.res_s > 1 && (p.M % e.hw) != 0) return false;
  if (e.pj > 0) {  // P = g^T a2 (a2 of 64 columns: layer 1): the mask bits alone, K 64 / 128
    if (e.y || !e.bits || e.pj != 64 || p.K > 128 || ((uintptr_t)e.a2 & 15) || !e.ppart) return false;
    if (((uintptr_t)p.b.ptr & 15) || p.b.ld % 8 != 0) return false;  // weight fragments in registers
  }
  return true;
}

// column tile of the streaming kernel: 128 for K = 256 with the mask bits alone and one TSM shift per 128 columns
// (bwd_stream128_body), else 64; VCG_BWD_STREAM=64 keeps 64 (read per call: tests compare the tilings)
static int bwd_stream_tn(const GemmParams& p) {
  const BwdEpi& e = p.bwd;
  const char* v = getenv("VCG_BWD_STREAM");
  if ((v && v[0] == '6') || p.bwd.pj > 0) return 64;  // (the P product lives in the 64-column kernel)
  return p.K == 256 && p.N % 128 == 0 && !e.y && (e.tsm_T <= 0 || e.tsm_fold % 128 == 0) ? 128 : 64;
}

static int bwd_stream_rows(const GemmParams& p) {
  const int nx = p.N / bwd_stream_tn(p), mtiles = (p.M + 63) / 64;
  int gy = 256 / nx;  // one workgroup per CU (~100-147 KB of LDS)
  if (gy >= 8) gy &= ~7;
  if (gy > mtiles) gy = mtiles >= 8 ? (mtiles & ~7) : mtiles;
  return gy < 1 ? 1 : gy;
}

bool fast_bwd_streams(const GemmParams& p) { return bwd_stream_ok(p); }

int fast_bwd_slots(const GemmParams& p) {
  if (bwd_stream_ok(p)) return bwd_stream_rows(p);
  const int ps = patch_bwd_slots(p);
  if (ps > 0) return ps;
  return fast_grid_rows(p.M, p.N, 1, bwd_light(p) ? EPI_BWD_AFF : EPI_BWD);
}

template <int BN, int AM, int EPI, int RES>
static int launch_fast(const GemmParams& p, int z, hipStream_t s) {
  const int nx = (p.N + BN - 1) / BN;
  const int gy = grid_rows(p.M, p.N, z, BN, EPI);
  dim3 grid(nx * gy, 1, z);
  const int tk = timing_begin(s);
  hipLaunchKernelGGL((igemm_fast_kernel<128, BN, AM, EPI, RES>), grid, dim3(256), 0, s, p);
  if (census_on()) { char t_[96]; snprintf(t_, sizeof(t_), "igemm_fast 128x%d a%d e%d r%d z%d", BN, AM, EPI, RES, z); census_add(t_, p.M, p.N, p.K); }
  timing_end(tk, s, TIMING_FAST_GEMM, 2.0 * p.M * p.N * (double)p.K * z, algorithmic_bytes<AM, EPI, RES>(p, z));
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

// (BM = 256: the streaming bodies' 512 threads)
template <int KC, int XF, int TN = 64>
static int launch_bwd_stream(const GemmParams& p, hipStream_t s) {
  const int nx = p.N / TN, gy = bwd_stream_rows(p);
  const int tk = timing_begin(s);
  hipLaunchKernelGGL((igemm_fast_kernel<256, TN, KC, EPI_BWD_STREAM, false, XF>), dim3(nx * gy), dim3(512), 0, s, p);
  if (census_on()) { char t_[96]; snprintf(t_, sizeof(t_), "igemm_fast_stream tn%d xf%d", TN, XF); census_add(t_, p.M, p.N, p.K); }
  // (with the g^T a2 product: + its flops, the a2 read and the P slabs written and reduced)
  const double pj = bwd_stream_pj(XF);
  timing_end(tk, s, TIMING_FAST_GEMM, 2.0 * p.M * p.N * (double)p.K + 2.0 * p.M * p.N * pj,
             algorithmic_bytes<OP_DENSE_K, EPI_BWD, false>(p, 1) + 2.0 * p.M * pj + 4.0 * p.N * pj);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

template <int KC>
static int run_bwd_stream(const GemmParams& p, hipStream_t s) {
  if constexpr (KC == 4) {  // bwd_stream_ok: K = 256 streams without y and without the P product only
    if (bwd_stream_tn(p) == 128)
      return p.bwd.bits ? launch_bwd_stream<4, XF_BITS, 128>(p, s) : launch_bwd_stream<4, 0, 128>(p, s);
    return p.bwd.bits ? launch_bwd_stream<4, XF_BITS>(p, s) : launch_bwd_stream<4, 0>(p, s);
  } else {
    if (p.bwd.pj == 64) return launch_bwd_stream<KC, XF_BITS | XF_P64>(p, s);
    if (!p.bwd.y) return p.bwd.bits ? launch_bwd_stream<KC, XF_BITS>(p, s) : launch_bwd_stream<KC, 0>(p, s);
    if (!p.bwd.y2) return launch_bwd_stream<KC, XF_HASY>(p, s);
    return launch_bwd_stream<KC, XF_HASY | XF_Y2>(p, s);
  }
}

template <int AM, int EPI, int RES = 0>
static int fast_bn(const GemmParams& p, int z, hipStream_t s) {
  if (fast_bn_cols(p.N) == 128) return launch_fast<128, AM, EPI, RES>(p, z, s);
  return launch_fast<64, AM, EPI, RES>(p, z, s);
}

// Entry from igemm.hip's dispatcher (bf16, K-contiguous A and B, no split-K).
// (Every output tile goes through the LDS stage: measured never slower, tools/bench_gemm.py, round 2.)
int run_fast_gemm(GemmParams& p, int amode, int epi, int z, hipStream_t s) {
  if (p.a.ptr2) {  // a BatchNorm backward folded into this input gradient: A = [g | y] (light epilogue only)
    if (amode != OP_DENSE_K || epi != EPI_BWD || z != 1 || !bwd_light(p) || p.a.split2 % FBK != 0) return -1;
    return fast_bn<OP_DENSE_K2, EPI_BWD_AFF>(p, z, s);
  }
  if (amode == OP_IM2COL && p.a.tsm_fold > 0) amode = OP_IM2COL_TSM;
  if (amode == OP_IM2COL && p.a.C < FBK) amode = OP_IM2COL_SMALLC;
  if (amode == OP_IM2COL_TSM && p.a.C < FBK) return -1;  // (dispatcher keeps these off the fast path)
  if (amode == OP_DGRAD && p.a.C < FBK) return -1;
  if (z == 1) {  // the LDS-patch kernels (conv_patch.hip): the stem, then the layer-1 3x3 convs
    const int r = run_patch_conv(p, amode, epi, s);
    if (r != -1) return r;
  }
  if (amode != OP_IM2COL_SMALLC && gemm256_ok(p, amode, epi, z)) return run_gemm256(p, amode, epi, s);
  if (epi == EPI_BWD && amode == OP_DENSE_K && z == 1 && bwd_stream_ok(p))
    return p.K == 64 ? run_bwd_stream<1>(p, s) : p.K == 128 ? run_bwd_stream<2>(p, s) : run_bwd_stream<4>(p, s);
  if (epi == EPI_BWD && bwd_light(p)) {
    if (amode == OP_DGRAD) return fast_bn<OP_DGRAD, EPI_BWD_AFF>(p, z, s);
    if (amode == OP_DENSE_K) return fast_bn<OP_DENSE_K, EPI_BWD_AFF>(p, z, s);
    return -1;
  }
  if (epi == EPI_BWD) {
    if (amode == OP_DGRAD) return fast_bn<OP_DGRAD, EPI_BWD>(p, z, s);
    if (amode == OP_DENSE_K) return fast_bn<OP_DENSE_K, EPI_BWD>(p, z, s);
    return -1;
  }
  if (epi == EPI_STATS) {
    if (amode == OP_IM2COL_SMALLC) return fast_bn<OP_IM2COL_SMALLC, EPI_STATS>(p, z, s);
    if (amode == OP_IM2COL_TSM) return fast_bn<OP_IM2COL_TSM, EPI_STATS>(p, z, s);
    if (amode == OP_IM2COL) return fast_bn<OP_IM2COL, EPI_STATS>(p, z, s);
    if (amode == OP_DGRAD) return fast_bn<OP_DGRAD, EPI_STATS>(p, z, s);
    return fast_bn<OP_DENSE_K, EPI_STATS>(p, z, s);
  }
  // dense layers only; RES = 2 (erf) / 3 (tanh): the GELU' x residual epilogue (FFN2's input gradient) as its own kernel -- in
  // the ReLU / add instantiation its erf code raised register use and slowed the scoring forward's folded conv3
  // GEMMs by ~10 % (2.72-2.76 K vs 3.06 K windows/s, bisected to that change)
  if (p.residual) return p.act == ACT_GELU_BWD        ? fast_bn<OP_DENSE_K, EPI_STORE, 2>(p, z, s)
                         : p.act == ACT_GELU_TANH_BWD ? fast_bn<OP_DENSE_K, EPI_STORE, 3>(p, z, s)
                                                      : fast_bn<OP_DENSE_K, EPI_STORE, 1>(p, z, s);
  if (p.aux && amode == OP_DENSE_K && (p.ldc & 7) == 0)  // a GELU input kept for the backward
    return fast_bn<OP_DENSE_K, EPI_STORE_AUX>(p, z, s);
  if (amode == OP_IM2COL_SMALLC) return fast_bn<OP_IM2COL_SMALLC, EPI_STORE>(p, z, s);
  if (amode == OP_IM2COL_TSM) return fast_bn<OP_IM2COL_TSM, EPI_STORE>(p, z, s);
  if (amode == OP_IM2COL) return fast_bn<OP_IM2COL, EPI_STORE>(p, z, s);
  if (amode == OP_DGRAD) return fast_bn<OP_DGRAD, EPI_STORE>(p, z, s);
  return fast_bn<OP_DENSE_K, EPI_STORE>(p, z, s);
}

}  // namespace vcg

// Profiling aid: the phase stamps of the last igemm_fast launch of a -DVCG_FAST_STAMPS build (FAST_STAMP above)
VCG_API int vcg_fast_stamps(unsigned long long* out, int n) {
#ifdef VCG_FAST_STAMPS
  n = n < 64 * 4 ? n : 64 * 4;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(vcg::g_fast_stamps), (size_t)n * 8, 0, hipMemcpyDeviceToHost) == hipSuccess
             ? 0 : 2;
#else
  (void)out;
  (void)n;
  return 1;
#endif
}
