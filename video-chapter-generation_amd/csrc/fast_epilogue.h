// Output stage and staged epilogues of the 128-row bf16 fast GEMM kernels (igemm_fast.hip's persistent engine, the
// streaming dgrads of bwd_stream.h, the patch kernels of conv_patch.hip).
#pragma once
#include "fastload.h"

namespace vcg {

// ---- output staging through LDS: full-row 16-B stores instead of 8-B row fragments ----------------
// The output tile (128 rows) lives in the finished stage `cur`: BN = 128 -> rows 0..63 at stA and rows 64..127 at
// stB ([64][128] each); BN = 64 -> the whole [128][64] tile at stA. 16-B chunks are XOR-swizzled per row
// (conflict-free 8-B writes of a 16-row fragment and 16-B reads of a row). LDS accesses are inline asm
// with explicit lgkmcnt waits.
template <int BN> __device__ __forceinline__ int st_slot(int row, int chunk) {
  if constexpr (BN == 128) return chunk ^ (row & 15);
  else return chunk ^ ((row >> 1) & 7);
}

template <int BN>
__device__ __forceinline__ void stage_put(bf16_t* stA, bf16_t* stB, int wm, int wn, int lane, int i, int j,
                                          const float (&v)[4]) {
  const int g = lane >> 4, ci = lane & 15;
  // (wm < 2, but behind readfirstlane the compiler does not know that: without the mask the patch / stem kernels
  // compile to other code than they always had)
  const int trow = (wm & 1) * 64 + i * 16 + ci;     // row in the 128-row tile
  const int tcol = wn * (BN / 2) + j * 16 + 4 * g;  // first of 4 columns
  bf16_t* reg = (BN == 128 && trow >= 64) ? stB : stA;
  const int row = BN == 128 ? (trow & 63) : trow;
  const uint32_t addr = lds_u32(reg + row * BN + 8 * st_slot<BN>(row, tcol >> 3) + (tcol & 7));
  uint2 q;
  q.x = pack2bf(v[0], v[1]);
  q.y = pack2bf(v[2], v[3]);
  asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(q) : "memory");
}

// all waves' stage_put done -> 16-B row chunks to global (rows >= M / cols >= N skipped)
// (m0: first row of the tile)
template <int BN>
__device__ __forceinline__ void stage_flush(const bf16_t* stA, const bf16_t* stB, const GemmParams& p, bf16_t* Cout,
                                            int m0, int n0, int mlim) {
  constexpr int NTH = 256, CPR = BN / 8, NCH = 128 * BN / 8;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  uint4 q[NCH / NTH];
#pragma unroll
  for (int k = 0; k < NCH / NTH; ++k) {
    const int id = threadIdx.x + NTH * k;
    const int trow = id / CPR, c = id - trow * CPR;
    const bf16_t* reg = (BN == 128 && trow >= 64) ? stB : stA;
    const int row = BN == 128 ? (trow & 63) : trow;
    const uint32_t addr = lds_u32(reg + row * BN + 8 * st_slot<BN>(row, c));
    asm volatile("ds_read_b128 %0, %1" : "=v"(q[k]) : "v"(addr) : "memory");
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < NCH / NTH; ++k) {
    const int id = threadIdx.x + NTH * k;
    const int trow = id / CPR, c = id - trow * CPR;
    const int m = m0 + trow, n = n0 + 8 * c;
    if (m < mlim && n < p.N) *reinterpret_cast<uint4*>(Cout + (long long)m * p.ldc + n) = q[k];
  }
  __builtin_amdgcn_s_barrier();  // every wave has read the stage before the next step's DMA refills it
}

// EPI_STORE (no residual / aux) through the stage
template <int BN>
__device__ __forceinline__ void epilogue_staged(f32x4 (&acc)[4][BN / 32], const GemmParams& p,
                                                const float (&bv)[BN / 32][4], bf16_t* Cout, bf16_t* stA,
                                                bf16_t* stB, int m0, int n0, int wm, int wn, int lane, int mlim) {
  constexpr int MT = 4, NT = BN / 32;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float t = acc[i][j][r] * p.alpha + bv[j][r];
        if (p.act != ACT_NONE && !act_is_gelu_bwd(p.act)) t = apply_act(t, p.act, p.fast_act);
        v[r] = t;
      }
      stage_put<BN>(stA, stB, wm, wn, lane, i, j, v);
    }
  stage_flush<BN>(stA, stB, p, Cout, m0, n0, mlim);
}

// EPI_STORE_AUX: the pre-activation values (bias added) to p.aux, then the activated values to Cout, each a
// staged pass of its own
template <int BN>
__device__ __forceinline__ void epilogue_staged_aux(f32x4 (&acc)[4][BN / 32], const GemmParams& p,
                                                    const float (&bv)[BN / 32][4], bf16_t* Cout, bf16_t* stA,
                                                    bf16_t* stB, int m0, int n0, int wm, int wn, int lane) {
  constexpr int MT = 4, NT = BN / 32;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float t = acc[i][j][r] * p.alpha + bv[j][r];
          v[r] = pass == 0 ? t : apply_act(t, p.act, p.fast_act);
        }
        stage_put<BN>(stA, stB, wm, wn, lane, i, j, v);
      }
    stage_flush<BN>(stA, stB, p, pass == 0 ? reinterpret_cast<bf16_t*>(p.aux) : Cout, m0, n0, p.M);
  }
}

// ---- EPI_BWD (igemm.h BwdEpi): conv-dgrad epilogue of the trunk backward ------------------------------
// Per-column parameters live in LDS (cpar[4][BN]: mean, msc, msh, mean2 of the workgroup's BN columns);
// a thread of the flush always owns the same 8-column chunk c = tid % (BN / 8), so its per-column sums stay
// in registers for the whole kernel and are combined across threads once at the end (bwd_finish).
// EPI_STORE + residual + ReLU through the stage (the running-statistics bn3 folded into conv3: relu(x W'^T + b + res),
// trunk.py _conv3_folded): the GEMM value is rounded to bf16 in the stage -- as the unfolded path stores y3 -- and the
// residual is added per 16-B row chunk in the flush, so both the residual loads and the output stores are full rows.
// ACT_GELU_BWD: the residual is the pre-activation and the output dh * GELU'(pre), dh rounded to bf16 first (as
// torch autocast's bf16 matmul output feeding gelu_backward); GELU_BWD 1: the erf form, 2: the tanh form
// (ACT_GELU_TANH_BWD), 0: the residual is an addend
template <int BN, int GELU_BWD>
__device__ __forceinline__ void epilogue_staged_res(f32x4 (&acc)[4][BN / 32], const GemmParams& p,
                                                    const float (&bv)[BN / 32][4], bf16_t* Cout, const bf16_t* Res,
                                                    bf16_t* stA, bf16_t* stB, int m0, int n0, int wm, int wn,
                                                    int lane, int mlim) {
  constexpr int MT = 4, NT = BN / 32, NTH = 256, CPR = BN / 8, KC = 128 * BN / 8 / NTH;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r] * p.alpha + bv[j][r];
      stage_put<BN>(stA, stB, wm, wn, lane, i, j, v);
    }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  uint4 q[KC], rv[KC];
#pragma unroll
  for (int k = 0; k < KC; ++k) {  // residual rows first (clamped to a valid row; discarded below)
    const int id = threadIdx.x + NTH * k;
    const int trow = id / CPR, c = id - trow * CPR;
    const int m = min(m0 + trow, mlim - 1), n = min(n0 + 8 * c, p.N - 8);
    rv[k] = *reinterpret_cast<const uint4*>(Res + (long long)m * p.ldr + n);
  }
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    const int id = threadIdx.x + NTH * k;
    const int trow = id / CPR, c = id - trow * CPR;
    const bf16_t* reg = (BN == 128 && trow >= 64) ? stB : stA;
    const int row = BN == 128 ? (trow & 63) : trow;
    const uint32_t addr = lds_u32(reg + row * BN + 8 * st_slot<BN>(row, c));
    asm volatile("ds_read_b128 %0, %1" : "=v"(q[k]) : "v"(addr) : "memory");
  }
  float rsc[8], rsh[8];  // an affine residual (p.res_sc): this thread's 8 columns are the same for every k
  if (p.res_sc) {
    const int nc = min(n0 + 8 * (int)(threadIdx.x % CPR), p.N - 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      rsc[e] = p.res_sc[nc + e];
      rsh[e] = p.res_sh[nc + e];
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    const int id = threadIdx.x + NTH * k;
    const int trow = id / CPR, c = id - trow * CPR;
    const int m = m0 + trow, n = n0 + 8 * c;
    float a[8], r[8];
    unpack8(q[k], a);
    unpack8(rv[k], r);
    if (p.res_sc) {
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = fmaf(r[e], rsc[e], rsh[e]);
    }
    uint32_t mb = 0;  // ReLU mask of the output (p.obits): bit e = out > 0, as vcg_bn_apply writes it
    if constexpr (GELU_BWD == 1) {  // BERT FFN2's input gradient: dh * GELU'(pre), dh rounded as stored
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] *= p.fast_act ? gelu_erf_grad_fast(r[e]) : gelu_erf_grad(r[e]);
    } else if constexpr (GELU_BWD == 2) {  // GPT's: the tanh form
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] *= p.fast_act ? gelu_tanh_grad_fast(r[e]) : gelu_tanh_grad(r[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a[e] = apply_act(a[e] + r[e], p.act);
        mb |= (a[e] > 0.f ? 1u : 0u) << e;
      }
    }
    const uint4 o = pack8(a);
    if (m < mlim && n < p.N) {
      *reinterpret_cast<uint4*>(Cout + (long long)m * p.ldc + n) = o;
      if (p.obits) p.obits[((long long)m * p.N + n) >> 3] = (uint8_t)mb;
    }
  }
  __builtin_amdgcn_s_barrier();  // every wave has read the stage before the next step's DMA refills it
}

template <int BN, bool LIGHT>
__device__ __forceinline__ void stage_flush_bwd(const bf16_t* stA, const bf16_t* stB, const GemmParams& p,
                                                bf16_t* Cout, int m0, int n0, const float* cpar, float (&s1)[8],
                                                float (&s2)[8], float (&s3)[8], int mlim) {
  constexpr int NTH = 256, CPR = BN / 8, NCH = 128 * BN / 8, KC = NCH / NTH;
#ifdef VCG_EPI_KB
  constexpr int KB = KC < VCG_EPI_KB ? KC : VCG_EPI_KB;
#else
  constexpr int KB = KC < 4 ? KC : 4;
#endif
  const BwdEpi& e = p.bwd;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  uint4 q[KC];
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    const int id = threadIdx.x + NTH * k;
    const int trow = id / CPR, c = id - trow * CPR;
    const bf16_t* reg = (BN == 128 && trow >= 64) ? stB : stA;
    const int row = BN == 128 ? (trow & 63) : trow;
    const uint32_t addr = lds_u32(reg + row * BN + 8 * st_slot<BN>(row, c));
    asm volatile("ds_read_b128 %0, %1" : "=v"(q[k]) : "v"(addr) : "memory");
  }
  const int c = threadIdx.x % CPR;
  const int lc = 8 * c, n = n0 + lc;
  float mu[8], sc[8], sh[8], mu2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    mu[i] = cpar[lc + i];
    sc[i] = cpar[BN + lc + i];
    sh[i] = cpar[2 * BN + lc + i];
    mu2[i] = cpar[3 * BN + lc + i];
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  int shift = 0;  // TSM adjoint: this column group's values move one frame later (+1) / earlier (-1)
  if (!LIGHT && e.tsm_T > 0) shift = n < e.tsm_fold ? 1 : (n < 2 * e.tsm_fold ? -1 : 0);
  const bf16_t* res = LIGHT ? nullptr : reinterpret_cast<const bf16_t*>(e.res);
  const bf16_t* yp = reinterpret_cast<const bf16_t*>(e.y);
  const bf16_t* y2p = LIGHT ? nullptr : reinterpret_cast<const bf16_t*>(e.y2);
  const uint8_t* bitsp = LIGHT ? nullptr : e.bits;
  // (rows beyond mlim / columns beyond N are clamped to a valid address and discarded after the load: a load
  // under a per-element condition makes hipcc branch around it and wait vmcnt(0) per element, i.e. one HBM round
  // trip per chunk; each operand's loads sit under ONE uniform branch per batch instead: l1 / l2 / l3 conv1 fused
  // dgrads 1453 / 760 / 421 -> 1354 / 615 / 355 us, tools/bench_dgrad.py. Rejected: pulling the next tile's
  // residual / y rows into L2 by LDS-DMA pieces into a scratch slot after each flush, +15-20 %.)
  const int nc = min(n, p.N - 8);
#pragma unroll
  for (int k0 = 0; k0 < KC; k0 += KB) {
    long long off[KB], roff[KB];
    bool ok[KB], src[KB], rok[KB];
    uint4 rv[KB], yv[KB], y2v[KB];
    uint32_t bv[KB];
#pragma unroll
    for (int kk = 0; kk < KB; ++kk) {  // addresses of the batch
      const int id = threadIdx.x + NTH * (k0 + kk);
      const int mr = m0 + id / CPR;
      ok[kk] = mr < mlim && n < p.N;
      const int m = min(mr, mlim - 1);
      src[kk] = true;
      int dst = m;
      if (e.sub) {  // sub-pixel class row -> dx row
        const uint32_t f = fdiv((uint32_t)m, e.fd_chw), r = (uint32_t)m - f * e.fd_chw.d;
        const uint32_t i = fdiv(r, e.fd_cw), j = r - i * (uint32_t)e.cW;
        dst = (int)((f * e.fH + 2 * i + e.ry) * e.fW + 2 * j + e.rx);
      }
      if (shift != 0) {
        const int f = (int)fdiv((uint32_t)m, e.fd_hw);
        const int t = f - (int)fdiv((uint32_t)f, e.fd_T) * e.tsm_T;
        const bool edge = shift > 0 ? t == e.tsm_T - 1 : t == 0;
        src[kk] = !edge;
        dst = edge ? m - shift * (e.tsm_T - 1) * e.hw : m + shift * e.hw;
      }
      off[kk] = (long long)dst * p.ldc + n;
      roff[kk] = (long long)dst * p.ldc + nc;
      rok[kk] = true;
      if (!LIGHT && e.res_s > 1) {  // compact residual of a 1x1 / stride-2 conv: only even (h, w) rows carry one
        const uint32_t f = fdiv((uint32_t)dst, e.fd_hw), r = (uint32_t)dst - f * (uint32_t)e.hw;
        const uint32_t h = fdiv(r, e.fd_w), w = r - h * e.fd_w.d;
        rok[kk] = ((h | w) & 1u) == 0;
        roff[kk] = ((long long)(f * e.rH + (h >> 1)) * e.rW + (w >> 1)) * p.ldc + nc;
      }
    }
    const long long* loff = off;  // y / y2 / bits rows (column clamped below)
    if (res) {
#pragma unroll
      for (int kk = 0; kk < KB; ++kk) rv[kk] = *reinterpret_cast<const uint4*>(res + roff[kk]);
    }
    if (bitsp) {
#pragma unroll
      for (int kk = 0; kk < KB; ++kk) bv[kk] = bitsp[(loff[kk] - n + nc) >> 3];
    }
    if (yp) {
#pragma unroll
      for (int kk = 0; kk < KB; ++kk) yv[kk] = *reinterpret_cast<const uint4*>(yp + loff[kk] - n + nc);
    }
    if (y2p) {
#pragma unroll
      for (int kk = 0; kk < KB; ++kk) y2v[kk] = *reinterpret_cast<const uint4*>(y2p + loff[kk] - n + nc);
    }
#pragma unroll
    for (int kk = 0; kk < KB; ++kk) {
      if (!rok[kk]) rv[kk] = make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int kk = 0; kk < KB; ++kk) {
      if (!ok[kk]) continue;
      float v[8];
      unpack8(q[k0 + kk], v);
      if (!src[kk]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0.f;
      }
      if (res) {
        float r[8];
        unpack8(rv[kk], r);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] += r[i];
      }
      if (bitsp) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = ((bv[kk] >> i) & 1u) ? v[i] : 0.f;
      }
      float yy[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (yp) {
        unpack8(yv[kk], yy);
        if (e.msc) {
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] = fmaf(yy[i], sc[i], sh[i]) > 0.f ? v[i] : 0.f;
        }
      }
      const uint4 o = pack8(v);
      *reinterpret_cast<uint4*>(Cout + off[kk]) = o;
      if (e.nred > 0) {
        unpack8(o, v);  // statistics of the stored (rounded) gradient
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          s1[i] += v[i];
          s2[i] = yp ? fmaf(v[i], yy[i] - mu[i], s2[i]) : s2[i];
        }
        if (y2p) {
          float y2[8];
          unpack8(y2v[kk], y2);
#pragma unroll
          for (int i = 0; i < 8; ++i) s3[i] = fmaf(v[i], y2[i] - mu2[i], s3[i]);
        }
      }
    }
  }
  __builtin_amdgcn_s_barrier();  // every wave has read the stage before the next step's DMA refills it
}

// Combine the per-thread column sums of EPI_BWD (threads tid = c (mod BN/8) share columns 8c..8c+7) in a
// fixed order and write this workgroup's partial slot; scratch = the (idle) stage buffers. NTH: threads of the
// workgroup (256; the streaming kernels run 512).
template <int NTH, int BN>
__device__ __forceinline__ void bwd_finish(const GemmParams& p, float* scratch, const float* cpar_invstd,
                                           const float (&s1)[8], const float (&s2)[8], const float (&s3)[8], int n0,
                                           int slot) {
  constexpr int CPR = BN / 8;
  const int nred = p.bwd.nred;
  __syncthreads();
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    scratch[(0 * NTH + tid) * 8 + i] = s1[i];
    scratch[(1 * NTH + tid) * 8 + i] = s2[i];
    scratch[(2 * NTH + tid) * 8 + i] = s3[i];
  }
  __syncthreads();
  if (tid < BN && n0 + tid < p.N) {
    const int c = tid >> 3, i = tid & 7;
    float a[3] = {0.f, 0.f, 0.f};
    for (int t = c; t < NTH; t += CPR)
#pragma unroll
      for (int r = 0; r < 3; ++r) a[r] += scratch[(r * NTH + t) * 8 + i];
    float* out = p.bwd.part + (long long)slot * nred * p.N + n0 + tid;
    out[0] = a[0];
    out[p.N] = a[1] * cpar_invstd[tid];
    if (nred > 2) out[2 * p.N] = a[2] * cpar_invstd[BN + tid];
  }
}

// ---- EPI_STATS: the BatchNorm statistics of the stored (bf16) conv output, from the staged tiles ----------
// A flush thread always owns the same 8-column chunk c = tid % (BN / 8); it keeps shifted sums of the
// values it stores (shift = its first value per column: no cancellation when |mean| >> std) for the whole
// kernel: count, sh[8], s1[8] = sum (v - sh), s2[8] = sum (v - sh)^2.
template <int BN>
__device__ __forceinline__ void stage_flush_stats(const bf16_t* stA, const bf16_t* stB, const GemmParams& p,
                                                  bf16_t* Cout, int m0, int n0, int& cnt, float (&sh)[8],
                                                  float (&s1)[8], float (&s2)[8], int mlim) {
  constexpr int NTH = 256, CPR = BN / 8, NCH = 128 * BN / 8, KC = NCH / NTH;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  uint4 q[KC];
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    const int id = threadIdx.x + NTH * k;
    const int trow = id / CPR, c = id - trow * CPR;
    const bf16_t* reg = (BN == 128 && trow >= 64) ? stB : stA;
    const int row = BN == 128 ? (trow & 63) : trow;
    const uint32_t addr = lds_u32(reg + row * BN + 8 * st_slot<BN>(row, c));
    asm volatile("ds_read_b128 %0, %1" : "=v"(q[k]) : "v"(addr) : "memory");
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  const int c = threadIdx.x % CPR;
  const int n = n0 + 8 * c;
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    const int id = threadIdx.x + NTH * k;
    const int m = m0 + id / CPR;
    if (m < mlim && n < p.N) {
      if (Cout) *reinterpret_cast<uint4*>(Cout + (long long)m * p.ldc + n) = q[k];  // (null: statistics only)
      float v[8];
      unpack8(q[k], v);
      if (cnt == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) sh[i] = v[i];
      }
      ++cnt;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = v[i] - sh[i];
        s1[i] += d;
        s2[i] = fmaf(d, d, s2[i]);
      }
    }
  }
  __builtin_amdgcn_s_barrier();  // every wave has read the stage before the next step's DMA refills it
}

// Per-thread (count, mean, M2) of every column chunk, merged across the threads that share the chunk with
// Chan's formula in thread order (deterministic) -> stats[col][by] = (mean, M2) and the count row
// stats[N][by]; slots by + k*gy (k >= 1) are marked empty. scratch = the idle stage buffers.
template <int BN>
__device__ __forceinline__ void stats_finish(const GemmParams& p, float* scratch, int cnt, const float (&sh)[8],
                                             const float (&s1)[8], const float (&s2)[8], int n0, int by, int bx,
                                             int gy, int mslots) {
  constexpr int NTH = 256, CPR = BN / 8;
  __syncthreads();  // all LDS-DMA retired (the last step waited vmcnt(0)); the stage buffers are free
  const int tid = threadIdx.x;
  const float nf = (float)cnt, inv = cnt > 0 ? 1.f / nf : 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    scratch[(0 * NTH + tid) * 8 + i] = sh[i] + s1[i] * inv;                 // mean
    scratch[(1 * NTH + tid) * 8 + i] = fmaxf(s2[i] - s1[i] * s1[i] * inv, 0.f);  // M2
  }
  scratch[2 * NTH * 8 + tid] = nf;
  __syncthreads();
  if (tid < BN && n0 + tid < p.N) {
    const int c = tid >> 3, i = tid & 7;
    float na = 0.f, mean = 0.f, m2 = 0.f;
    for (int t = c; t < NTH; t += CPR) {
      const float nb = scratch[2 * NTH * 8 + t];
      if (nb > 0.f) {
        const float mb = scratch[t * 8 + i], m2b = scratch[(NTH + t) * 8 + i];
        const float nt = na + nb, d = mb - mean;
        mean += d * (nb / nt);
        m2 += m2b + d * d * (na * nb / nt);
        na = nt;
      }
    }
    reinterpret_cast<float2*>(p.stats)[(long long)(n0 + tid) * mslots + by] = make_float2(mean, m2);
  }
  if (bx == 0 && tid == 0) {
    float rows = 0.f;  // threads 0..CPR-1 cover every row of the workgroup once (one chunk column each)
    for (int t = 0; t < NTH; t += CPR) rows += scratch[2 * NTH * 8 + t];
    float2* cntrow = reinterpret_cast<float2*>(p.stats) + (long long)p.N * mslots;
    cntrow[by] = make_float2(rows, by == 0 ? (float)gy : 0.f);  // slot 0 also tells bn_finalize: gy slots used
    for (int t = by + gy; t < mslots; t += gy) cntrow[t] = make_float2(0.f, 0.f);
  }
}

}  // namespace vcg
