// Row-softmax tile engine: the loss over a wide class axis of Z = X W^T without storing Z. Shared by the masked-LM
// vocabulary head (mlm_head.hip) and the fused InfoNCE (contrast.hip); each includes this file and supplies a policy.
//
//   softmax_tile_kernel<P, TILE_LOSS>    Z in 64 (rows) x 128 (columns) tiles, bf16 MFMA 16x16x32, fp32 accumulators;
//                                        grid = row blocks x column splits, so a few hundred rows still fill the chip.
//                                        Each lane keeps, for its 4 rows, the running maximum, the running sum of
//                                        exponentials (online softmax, as bert_attn_long.hip), the argmax over the
//                                        columns it sees and, for a policy with targets, the target's logit; the 16
//                                        lane states of a row are combined through LDS in a fixed order and written as
//                                        one partial per (split, row). Nothing of rows x columns elements is stored.
//   softmax_tile_kernel<P, TILE_DZ>      recomputes the tiles and writes P::dz once, in bf16, as [R][ldo] (the columns
//                                        V .. kp - 1, kp = V rounded up to 8, are written as zeros).
//   softmax_tile_kernel<P, TILE_LOGITS>  the same main loop with an fp32 store of the logits.
//   merge_splits                         a row's splits, one wave per row, fixed order: the first half of a finalize
//                                        kernel, whose tail (what a row's loss and a correct row are) is the caller's.
//   softmax_mean_kernel                  the mean loss and the count over the rows in one workgroup.
//   softmax_rows_f32_kernel<P>           fp32 logits [R][ldz] (the parity mode forms them with vcg_gemm) -> the same
//                                        partials, one split, for the same finalize kernels.
//   Fixed reduction trees, no atomics: bit-identical run to run.
//
// The MFMA is issued as (W fragment, X fragment), so a lane holds one row (lane % 16) and 4 consecutive columns
// (4 (lane / 16) + r) of each 16 x 16 fragment: the column reduction is mostly in-register, and the dZ / logits stores
// are 8 / 16 bytes per lane.
//
// A policy P is a struct of compile-time choices, nothing is decided at run time:
//   GATHER  bool  output row r reads X[rows[r]] (rows == nullptr: the identity), checked against rows_total
//   SCALED  bool  the logits are the products times TileArgs::zscale
//   TARGET  bool  a row has a target column tgt[r]: its logit is carried in the state and in a fifth partials plane
//   COL0    int   the id of the first column in the argmax (the caller may join columns 0 .. COL0 - 1 in its tail)
//   dz_scale(a)                       the factor of dZ, once per thread
//   dz(z, lse, is_target, scale)      dZ of one logit
#pragma once
#include "common.h"

#include <math.h>

namespace vcg {

namespace {

constexpr int TILE_BR = 64;           // rows per tile
constexpr int TILE_BV = 128;          // columns per tile
constexpr int TILE_BK = 64;           // k per stage
constexpr int TILE_LD = TILE_BK + 8;  // LDS row stride in bf16 (144 B: 16-B aligned, spreads the banks)
constexpr int TILE_MAX_H = 4096;
constexpr int TILE_TARGET_WGS = 512;  // workgroups wanted from row blocks x splits (256 CUs, two per CU)

enum { TILE_LOSS = 0, TILE_DZ = 1, TILE_LOGITS = 2 };

struct TileArgs {
  const bf16_t* X;        // [rows_total][H]
  const long long* rows;  // GATHER: [R] row of X per output row (nullptr: the identity)
  const bf16_t* W;        // [V][H]
  const long long* tgt;   // TARGET: [R]
  int rows_total, R, V, H, splits, tiles_per_split;
  int kp;                 // V rounded up to 8: the columns V .. kp - 1 are written as zeros
  float zscale;           // SCALED
  float* part;            // TILE_LOSS: [planes][splits][R], see RowState
  const float* lse;       // TILE_DZ
  const float* dloss;     // TILE_DZ: a device scalar, or
  float scale;            //          a host one (the policy's dz_scale picks)
  void* out;              // TILE_DZ: bf16 [R][ldo]; TILE_LOGITS: fp32 [R][ldo]
  long long ldo;
};

// Online-softmax state of one row over the columns seen so far: maximum, sum of exp(z - maximum), the target's logit
// (ZT only; 0 until seen) and the argmax as (value, column id). Stored as PLANES floats in this order: m, s, [zt,] av,
// ai.
template <bool ZT>
struct TargetLogit {
  float zt = 0.f;
};
template <>
struct TargetLogit<false> {};

template <bool ZT>
struct RowState : TargetLogit<ZT> {
  static constexpr int PLANES = ZT ? 5 : 4;
  float m = -INFINITY, s = 0.f, av = -INFINITY;
  int ai = -1;
};

// plane j of a state is p[j * stride]
template <bool ZT>
__device__ __forceinline__ RowState<ZT> state_load(const float* p, long long stride) {
  RowState<ZT> t;
  t.m = p[0];
  t.s = p[stride];
  if constexpr (ZT) t.zt = p[2 * stride];
  t.av = p[(2 + ZT) * stride];
  t.ai = __float_as_int(p[(3 + ZT) * stride]);
  return t;
}

template <bool ZT>
__device__ __forceinline__ void state_store(float* p, long long stride, const RowState<ZT>& t) {
  p[0] = t.m;
  p[stride] = t.s;
  if constexpr (ZT) p[2 * stride] = t.zt;
  p[(2 + ZT) * stride] = t.av;
  p[(3 + ZT) * stride] = __int_as_float(t.ai);
}

// a <- a merged with b, over disjoint column sets. Symmetric in (a, b) bit for bit (a maximum, a commutative sum, and
// the argmax tie goes to the lower index), so a butterfly over lanes leaves every lane with the same state.
template <bool ZT>
__device__ __forceinline__ void state_merge(RowState<ZT>& a, const RowState<ZT>& b) {
  const float M = fmaxf(a.m, b.m);
  if (M > -INFINITY) {
    const float sa = a.m > -INFINITY ? a.s * expf(a.m - M) : 0.f;
    const float sb = b.m > -INFINITY ? b.s * expf(b.m - M) : 0.f;
    a.s = sa + sb;
    a.m = M;
  }
  if constexpr (ZT) a.zt += b.zt;
  if (b.ai >= 0 && (a.ai < 0 || b.av > a.av || (b.av == a.av && b.ai < a.ai))) {
    a.av = b.av;
    a.ai = b.ai;
  }
}

template <class P, int MODE>
__global__ __launch_bounds__(256) void softmax_tile_kernel(TileArgs a) {
  using State = RowState<P::TARGET>;
  __shared__ __attribute__((aligned(16))) bf16_t sX[TILE_BR * TILE_LD];
  __shared__ __attribute__((aligned(16))) bf16_t sW[TILE_BV * TILE_LD];
  __shared__ float sred[MODE == TILE_LOSS ? 16 * TILE_BR * State::PLANES : 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int r0 = blockIdx.x * TILE_BR;
  const int ntv = (a.V + TILE_BV - 1) / TILE_BV;
  const int vt0 = blockIdx.y * a.tiles_per_split;
  const int vt1 = min(vt0 + a.tiles_per_split, ntv);
  const int nk = (a.H + TILE_BK - 1) / TILE_BK;

  // this thread's 16-B chunks of the X tile (2) and of the W tile (4): row = chunk / 8, k = 8 (chunk % 8)
  const bf16_t* xp[2];
  int xo[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = tid + j * 256, row = c >> 3;
    xo[j] = row * TILE_LD + (c & 7) * 8;
    const int r = r0 + row;
    if constexpr (P::GATHER) {
      long long idx = -1;
      if (r < a.R) idx = a.rows ? a.rows[r] : (long long)r;
      xp[j] = (idx >= 0 && idx < a.rows_total) ? a.X + idx * a.H + (c & 7) * 8 : nullptr;
    } else {
      xp[j] = r < a.R ? a.X + (long long)r * a.H + (c & 7) * 8 : nullptr;
    }
  }

  // the rows of this lane's fragments: r0 + 16 i + li
  int tg[4];
  float lse[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + i * 16 + li;
    tg[i] = -1;
    lse[i] = 0.f;
    if constexpr (MODE != TILE_LOGITS) {
      if (r < a.R) {
        if constexpr (P::TARGET) tg[i] = (int)a.tgt[r];
        if constexpr (MODE == TILE_DZ) lse[i] = a.lse[r];
      }
    }
  }
  float scale = 0.f;
  if constexpr (MODE == TILE_DZ) scale = P::dz_scale(a);

  State st[4];

  for (int vt = vt0; vt < vt1; ++vt) {
    const int v0 = vt * TILE_BV;
    const bf16_t* wp[4];
    int wo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = tid + j * 256, row = c >> 3;
      wo[j] = row * TILE_LD + (c & 7) * 8;
      const int v = v0 + row;
      wp[j] = v < a.V ? a.W + (long long)v * a.H + (c & 7) * 8 : nullptr;
    }
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int f = 0; f < 2; ++f) acc[i][f] = f32x4{0.f, 0.f, 0.f, 0.f};

    uint4 rx[2], rw[4];
    auto fetch = [&](int k0) {
      const int kc = k0 + (tid & 7) * 8;  // (H % 8 == 0: a chunk is inside the row or past it)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        rx[j] = (xp[j] && kc < a.H) ? *reinterpret_cast<const uint4*>(xp[j] + k0) : make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        rw[j] = (wp[j] && kc < a.H) ? *reinterpret_cast<const uint4*>(wp[j] + k0) : make_uint4(0, 0, 0, 0);
    };
    fetch(0);
    for (int kt = 0; kt < nk; ++kt) {
      __syncthreads();  // the previous stage's fragment reads are done
#pragma unroll
      for (int j = 0; j < 2; ++j) *reinterpret_cast<uint4*>(sX + xo[j]) = rx[j];
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<uint4*>(sW + wo[j]) = rw[j];
      __syncthreads();
      if (kt + 1 < nk) fetch((kt + 1) * TILE_BK);  // in flight during the MFMAs
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        s16x8 xf[4], wf[2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          xf[i] = *reinterpret_cast<const s16x8*>(sX + (i * 16 + li) * TILE_LD + s2 * 32 + g * 8);
#pragma unroll
        for (int f = 0; f < 2; ++f)
          wf[f] = *reinterpret_cast<const s16x8*>(sW + (wave * 32 + f * 16 + li) * TILE_LD + s2 * 32 + g * 8);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int f = 0; f < 2; ++f)
            acc[i][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[f], xf[i], acc[i][f], 0, 0, 0);
      }
    }
    if constexpr (P::SCALED) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int f = 0; f < 2; ++f) acc[i][f] *= a.zscale;
    }

    // acc[i][f][r] = z(row r0 + 16 i + li, column v0 + 32 wave + 16 f + 4 g + r)
    const int vb = v0 + wave * 32 + g * 4;
    if constexpr (MODE == TILE_LOSS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float tmax = -INFINITY;
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int v = vb + f * 16 + r;
            if (v < a.V) {
              const float z = acc[i][f][r];
              tmax = fmaxf(tmax, z);
              if (z > st[i].av || st[i].ai < 0) {  // (columns come in ascending order: the first maximum stays)
                st[i].av = z;
                st[i].ai = P::COL0 + v;
              }
              if constexpr (P::TARGET)
                if (v == tg[i]) st[i].zt = z;
            }
          }
        if (tmax > -INFINITY) {
          const float mn = fmaxf(st[i].m, tmax);
          float s = st[i].m > -INFINITY ? st[i].s * __expf(st[i].m - mn) : 0.f;
#pragma unroll
          for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (vb + f * 16 + r < a.V) s += __expf(acc[i][f][r] - mn);
          st[i].m = mn;
          st[i].s = s;
        }
      }
    } else if constexpr (MODE == TILE_DZ) {
      bf16_t* dz = reinterpret_cast<bf16_t*>(a.out);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = r0 + i * 16 + li;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const int v4 = vb + f * 16;
          if (row < a.R && v4 < a.kp) {  // (kp % 8 == 0, v4 % 4 == 0: the 4 columns are inside the padded row)
            uint32_t w[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              bf16_t b2[2];
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                const int r = 2 * h + e, v = v4 + r;
                b2[e] = f2bf(v < a.V ? P::dz(acc[i][f][r], lse[i], v == tg[i], scale) : 0.f);
              }
              w[h] = (uint32_t)b2[0] | ((uint32_t)b2[1] << 16);
            }
            *reinterpret_cast<uint2*>(dz + (long long)row * a.ldo + v4) = make_uint2(w[0], w[1]);
          }
        }
      }
    } else {
      float* zo = reinterpret_cast<float*>(a.out);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = r0 + i * 16 + li;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const int v4 = vb + f * 16;
          if (row < a.R && v4 < a.kp)  // (columns V .. kp - 1 are zeros: their W rows were zero-filled)
            *reinterpret_cast<float4*>(zo + (long long)row * a.ldo + v4) =
                make_float4(acc[i][f][0], acc[i][f][1], acc[i][f][2], acc[i][f][3]);
        }
      }
    }
  }

  if constexpr (MODE == TILE_LOSS) {
    // the 16 states of a row (4 waves x 4 lane groups), merged in that order by one thread per row
    const int src = wave * 4 + g;
#pragma unroll
    for (int i = 0; i < 4; ++i) state_store(sred + (src * TILE_BR + i * 16 + li) * State::PLANES, 1, st[i]);
    __syncthreads();
    if (tid < TILE_BR && r0 + tid < a.R) {
      State t;
      for (int q = 0; q < 16; ++q) state_merge(t, state_load<P::TARGET>(sred + (q * TILE_BR + tid) * State::PLANES, 1));
      state_store(a.part + (long long)blockIdx.y * a.R + r0 + tid, (long long)a.splits * a.R, t);
    }
  }
}

// Row r's splits merged by one wave: lane l takes splits l, l + 64, ... in order, then a butterfly over the lanes
// (state_merge is symmetric, so the order is fixed and every lane ends with the same state).
template <bool ZT>
__device__ __forceinline__ RowState<ZT> merge_splits(const float* part, int splits, int R, int r, int lane) {
  const long long SR = (long long)splits * R;
  RowState<ZT> t;
  for (int s = lane; s < splits; s += 64) state_merge(t, state_load<ZT>(part + (long long)s * R + r, SR));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    RowState<ZT> u;
    u.m = __shfl_xor(t.m, o, 64);
    u.s = __shfl_xor(t.s, o, 64);
    if constexpr (ZT) u.zt = __shfl_xor(t.zt, o, 64);
    u.av = __shfl_xor(t.av, o, 64);
    u.ai = __shfl_xor(t.ai, o, 64);
    state_merge(t, u);
  }
  return t;
}

// rowres [2][R] (a finalize kernel's output: the row's loss, and 1 where the row is correct) -> the mean and the count
__global__ __launch_bounds__(256) void softmax_mean_kernel(const float* rowres, int R, float* mean_loss,
                                                           long long* n_correct) {
  __shared__ double ssum[256];
  __shared__ int scnt[256];
  const int tid = threadIdx.x;
  double lsum = 0.0;
  int cnt = 0;
  for (int r = tid; r < R; r += 256) {
    lsum += (double)rowres[r];
    cnt += rowres[R + r] != 0.f ? 1 : 0;
  }
  ssum[tid] = lsum;
  scnt[tid] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      ssum[tid] += ssum[tid + o];
      scnt[tid] += scnt[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (mean_loss) mean_loss[0] = (float)(ssum[0] / (double)R);
    if (n_correct) n_correct[0] = scnt[0];
  }
}

// fp32 logits [R][ldz] -> the partials of one split (one workgroup per row; thread t sees columns t, t + 256, ...)
template <class P>
__global__ __launch_bounds__(256) void softmax_rows_f32_kernel(const float* z, long long ldz, const long long* tgt,
                                                               int R, int V, float* part) {
  using State = RowState<P::TARGET>;
  __shared__ float sred[256 * State::PLANES];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* zr = z + (long long)r * ldz;
  int tg = -1;
  if constexpr (P::TARGET) tg = (int)tgt[r];
  State t;
  for (int v = tid; v < V; v += 256) {
    const float x = zr[v];
    if (x > t.av || t.ai < 0) {
      t.av = x;
      t.ai = P::COL0 + v;
    }
    if constexpr (P::TARGET)
      if (v == tg) t.zt = x;
    const float mn = fmaxf(t.m, x);
    t.s = (t.m > -INFINITY ? t.s * expf(t.m - mn) : 0.f) + expf(x - mn);
    t.m = mn;
  }
  state_store(sred + tid * State::PLANES, 1, t);
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {  // fixed tree
    if (tid < o) {
      State x = state_load<P::TARGET>(sred + tid * State::PLANES, 1);
      state_merge(x, state_load<P::TARGET>(sred + (tid + o) * State::PLANES, 1));
      state_store(sred + tid * State::PLANES, 1, x);
    }
    __syncthreads();
  }
  if (tid == 0) state_store(part + r, R, state_load<P::TARGET>(sred, 1));
}

// splits of the column axis for R output rows: a pure function of the shape (the reduction order follows it)
inline void tile_split(int R, int V, int* splits, int* tps) {
  const int ntv = (V + TILE_BV - 1) / TILE_BV, nrb = (R + TILE_BR - 1) / TILE_BR;
  int s = (TILE_TARGET_WGS + nrb - 1) / nrb;
  s = s < 1 ? 1 : (s > ntv ? ntv : s);
  *tps = (ntv + s - 1) / s;
  *splits = (ntv + *tps - 1) / *tps;
}

// workspace: the state's planes per (split, row), then 2 floats per row (a finalize kernel's rowres)
template <class P>
long long tile_ws_floats(int splits, int R) {
  return ((long long)RowState<P::TARGET>::PLANES * splits + 2) * R;
}

inline int tile_shape_ok(const char* who, int R, int V, int H) {
  if (R <= 0 || V <= 0 || H <= 0) {
    set_error(std::string(who) + ": empty shape");
    return VCG_ERR_INVALID;
  }
  if (H % 8 != 0 || H > TILE_MAX_H) {
    set_error(std::string(who) + ": H must be a multiple of 8, at most 4096");
    return VCG_ERR_UNSUPPORTED;
  }
  return VCG_OK;
}

// the arguments every mode shares, with the split of the shape
inline TileArgs tile_args(const void* X, const void* W, int R, int V, int H) {
  TileArgs a{};
  a.X = reinterpret_cast<const bf16_t*>(X);
  a.W = reinterpret_cast<const bf16_t*>(W);
  a.rows_total = R; a.R = R; a.V = V; a.H = H;
  a.kp = (V + 7) / 8 * 8;
  tile_split(R, V, &a.splits, &a.tiles_per_split);
  return a;
}

template <class P, int MODE>
void tile_launch(const TileArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL((softmax_tile_kernel<P, MODE>), dim3((a.R + TILE_BR - 1) / TILE_BR, a.splits), dim3(256), 0,
                     stream, a);
}

}  // namespace

}  // namespace vcg
