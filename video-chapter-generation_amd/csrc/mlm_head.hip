// Masked-LM vocabulary head (reference: model/lang/bert_hugface.py:98-132 projects every position onto the vocabulary,
// softmaxes and only then gathers the masked rows for F.cross_entropy, pretrain_lang_model_hugface.py). Here only the
// R masked rows are projected, and the vocabulary axis is reduced on the fly:
//
//   mlm_tile_kernel<MLM_LOSS>    Z = X[rows] W^T in 64 (rows) x 128 (vocabulary) tiles, bf16 MFMA 16x16x32 with fp32
//                                accumulators; grid = row blocks x vocabulary splits, so R ~ 450 still fills the chip.
//                                Each lane keeps, for its 4 rows, the running maximum, the running sum of exponentials
//                                (online softmax, as bert_attn_long.hip), the target's logit and the argmax over the
//                                columns it sees; the 16 lane states of a row are combined through LDS in a fixed order
//                                and written as one partial per (split, row). Nothing of R x V elements is stored.
//   mlm_finalize_rows_kernel     combines a row's splits (one wave per row, fixed order): lse, lse - z_target and whether
//   mlm_mean_kernel              the argmax (lowest index on equal values) is the target; then the mean loss and the
//                                count over the rows in one workgroup. Fixed reduction trees, no atomics: bit-identical
//                                run to run.
//   mlm_tile_kernel<MLM_DZ>      recomputes the tiles and writes dZ = (exp(z - lse) - onehot(target)) * dloss / R once,
//                                in bf16, as [R][ldz] (ldz = V rounded up to 8; the pad columns are written as zeros).
//   mlm_tile_kernel<MLM_LOGITS>  the same main loop over every row with an fp32 store: the logits of the drop-in forward.
//
// The MFMA is issued as (W fragment, X fragment), so a lane holds one row (lane % 16) and 4 consecutive vocabulary
// columns (4 (lane / 16) + r) of each 16 x 16 fragment: the vocabulary reduction is mostly in-register, and the dZ /
// logits stores are 8 / 16 bytes per lane.
//
// The fp32 parity mode computes the masked rows' logits with vcg_gemm; mlm_rows_f32_kernel reduces them to the same
// partials (one split) for the same finalize kernel, and mlm_dz_f32_kernel turns them into dZ in place.
//
// seq_softmax_kernel: prob[b][l][v] = softmax over l (the reference's F.softmax(logits, dim=1) on [B, L, V],
// bert_hugface.py:114), one thread per (b, v), reads coalesced along v; L <= 64 is held in registers (one read).
#include "common.h"

#include <math.h>

namespace vcg {

namespace {

constexpr int MLM_BR = 64;           // rows per tile
constexpr int MLM_BV = 128;          // vocabulary columns per tile
constexpr int MLM_BK = 64;           // k per stage
constexpr int MLM_LD = MLM_BK + 8;   // LDS row stride in bf16 (144 B: 16-B aligned, spreads the banks)
constexpr int MLM_MAX_H = 4096;
constexpr int MLM_TARGET_WGS = 512;  // workgroups wanted from rows x splits (256 CUs, two per CU)

enum { MLM_LOSS = 0, MLM_DZ = 1, MLM_LOGITS = 2 };

struct MlmArgs {
  const bf16_t* X;        // [rows_total][H]
  const long long* rows;  // [R] row of X per output row (nullptr: the identity)
  const bf16_t* W;        // [V][H]
  const long long* tgt;   // [R]
  int rows_total, R, V, H, splits, tiles_per_split;
  float* part;            // MLM_LOSS: [5][splits][R] (max, sum, target logit, argmax value, argmax index bits)
  const float* lse;       // MLM_DZ
  const float* dloss;     // MLM_DZ: the mean loss' gradient (device scalar)
  void* out;              // MLM_DZ: bf16 [R][ldo]; MLM_LOGITS: fp32 [R][ldo]
  long long ldo;
};

struct RowState {
  float m, s, zt, av;
  int ai;
};

// a <- a merged with b, over disjoint column sets. Symmetric in (a, b) bit for bit (a maximum, a commutative sum, and
// the argmax tie goes to the lower index), so a butterfly over lanes leaves every lane with the same state.
__device__ __forceinline__ void state_merge(RowState& a, const RowState& b) {
  const float M = fmaxf(a.m, b.m);
  if (M > -INFINITY) {
    const float sa = a.m > -INFINITY ? a.s * expf(a.m - M) : 0.f;
    const float sb = b.m > -INFINITY ? b.s * expf(b.m - M) : 0.f;
    a.s = sa + sb;
    a.m = M;
  }
  a.zt += b.zt;
  if (b.ai >= 0 && (a.ai < 0 || b.av > a.av || (b.av == a.av && b.ai < a.ai))) {
    a.av = b.av;
    a.ai = b.ai;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void mlm_tile_kernel(MlmArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t sX[MLM_BR * MLM_LD];
  __shared__ __attribute__((aligned(16))) bf16_t sW[MLM_BV * MLM_LD];
  __shared__ float sred[MODE == MLM_LOSS ? 16 * MLM_BR * 5 : 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int r0 = blockIdx.x * MLM_BR;
  const int ntv = (a.V + MLM_BV - 1) / MLM_BV;
  const int vt0 = blockIdx.y * a.tiles_per_split;
  const int vt1 = min(vt0 + a.tiles_per_split, ntv);
  const int nk = (a.H + MLM_BK - 1) / MLM_BK;

  // this thread's 16-B chunks of the X tile (2) and of the W tile (4): row = chunk / 8, k = 8 (chunk % 8)
  const bf16_t* xp[2];
  int xo[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = tid + j * 256, row = c >> 3;
    xo[j] = row * MLM_LD + (c & 7) * 8;
    const int r = r0 + row;
    long long idx = -1;
    if (r < a.R) idx = a.rows ? a.rows[r] : (long long)r;
    xp[j] = (idx >= 0 && idx < a.rows_total) ? a.X + idx * a.H + (c & 7) * 8 : nullptr;
  }

  // the rows of this lane's fragments: r0 + 16 i + li
  int tg[4];
  float lse[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + i * 16 + li;
    tg[i] = -1;
    lse[i] = 0.f;
    if constexpr (MODE != MLM_LOGITS) {
      if (r < a.R) {
        tg[i] = (int)a.tgt[r];
        if constexpr (MODE == MLM_DZ) lse[i] = a.lse[r];
      }
    }
  }
  float scale = 0.f;
  if constexpr (MODE == MLM_DZ) scale = a.dloss[0] / (float)a.R;

  RowState st[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) st[i] = RowState{-INFINITY, 0.f, 0.f, -INFINITY, -1};

  for (int vt = vt0; vt < vt1; ++vt) {
    const int v0 = vt * MLM_BV;
    const bf16_t* wp[4];
    int wo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = tid + j * 256, row = c >> 3;
      wo[j] = row * MLM_LD + (c & 7) * 8;
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
      if (kt + 1 < nk) fetch((kt + 1) * MLM_BK);  // in flight during the MFMAs
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        s16x8 xf[4], wf[2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          xf[i] = *reinterpret_cast<const s16x8*>(sX + (i * 16 + li) * MLM_LD + s2 * 32 + g * 8);
#pragma unroll
        for (int f = 0; f < 2; ++f)
          wf[f] = *reinterpret_cast<const s16x8*>(sW + (wave * 32 + f * 16 + li) * MLM_LD + s2 * 32 + g * 8);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int f = 0; f < 2; ++f)
            acc[i][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[f], xf[i], acc[i][f], 0, 0, 0);
      }
    }

    // acc[i][f][r] = z(row r0 + 16 i + li, column v0 + 32 wave + 16 f + 4 g + r)
    const int vb = v0 + wave * 32 + g * 4;
    if constexpr (MODE == MLM_LOSS) {
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
                st[i].ai = v;
              }
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
    } else if constexpr (MODE == MLM_DZ) {
      bf16_t* dz = reinterpret_cast<bf16_t*>(a.out);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = r0 + i * 16 + li;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const int v4 = vb + f * 16;
          if (row < a.R && v4 < a.ldo) {  // (ldo % 8 == 0, v4 % 4 == 0: the 4 columns are inside the padded row)
            uint32_t w[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              bf16_t b2[2];
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                const int r = 2 * h + e, v = v4 + r;
                float d = 0.f;
                if (v < a.V) d = (__expf(acc[i][f][r] - lse[i]) - (v == tg[i] ? 1.f : 0.f)) * scale;
                b2[e] = f2bf(d);
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
          if (row < a.R && v4 < a.ldo)  // (columns V .. ldo - 1 are zeros: their W rows were zero-filled)
            *reinterpret_cast<float4*>(zo + (long long)row * a.ldo + v4) =
                make_float4(acc[i][f][0], acc[i][f][1], acc[i][f][2], acc[i][f][3]);
        }
      }
    }
  }

  if constexpr (MODE == MLM_LOSS) {
    // the 16 states of a row (4 waves x 4 lane groups), merged in that order by one thread per row
    const int src = wave * 4 + g;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float* d = sred + (src * MLM_BR + i * 16 + li) * 5;
      d[0] = st[i].m;
      d[1] = st[i].s;
      d[2] = st[i].zt;
      d[3] = st[i].av;
      d[4] = __int_as_float(st[i].ai);
    }
    __syncthreads();
    if (tid < MLM_BR && r0 + tid < a.R) {
      RowState t{-INFINITY, 0.f, 0.f, -INFINITY, -1};
      for (int q = 0; q < 16; ++q) {
        const float* d = sred + (q * MLM_BR + tid) * 5;
        state_merge(t, RowState{d[0], d[1], d[2], d[3], __float_as_int(d[4])});
      }
      const long long SR = (long long)a.splits * a.R, o = (long long)blockIdx.y * a.R + r0 + tid;
      a.part[o] = t.m;
      a.part[SR + o] = t.s;
      a.part[2 * SR + o] = t.zt;
      a.part[3 * SR + o] = t.av;
      a.part[4 * SR + o] = __int_as_float(t.ai);
    }
  }
}

// One wave per row: lane l merges splits l, l + 64, ... in order, then a butterfly over the lanes (state_merge is
// symmetric, so the order is fixed and every lane ends with the same state). rowres [2][R]: the row's loss and
// whether its argmax is the target, for mlm_mean_kernel.
__global__ __launch_bounds__(256) void mlm_finalize_rows_kernel(const float* part, int splits, int R,
                                                                const long long* tgt, float* lse, float* row_loss,
                                                                float* rowres) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const long long SR = (long long)splits * R;
  RowState t{-INFINITY, 0.f, 0.f, -INFINITY, -1};
  for (int s = lane; s < splits; s += 64) {
    const long long o = (long long)s * R + r;
    state_merge(t, RowState{part[o], part[SR + o], part[2 * SR + o], part[3 * SR + o],
                            __float_as_int(part[4 * SR + o])});
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    RowState u{__shfl_xor(t.m, o, 64), __shfl_xor(t.s, o, 64), __shfl_xor(t.zt, o, 64), __shfl_xor(t.av, o, 64),
               __shfl_xor(t.ai, o, 64)};
    state_merge(t, u);
  }
  if (lane == 0) {
    const float l = t.m + logf(t.s), rl = l - t.zt;
    if (lse) lse[r] = l;
    if (row_loss) row_loss[r] = rl;
    rowres[r] = rl;
    rowres[R + r] = (long long)t.ai == tgt[r] ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(256) void mlm_mean_kernel(const float* rowres, int R, float* mean_loss,
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
__global__ __launch_bounds__(256) void mlm_rows_f32_kernel(const float* z, long long ldz, const long long* tgt, int R,
                                                           int V, float* part) {
  __shared__ float sred[256 * 5];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* zr = z + (long long)r * ldz;
  const int tg = (int)tgt[r];
  RowState t{-INFINITY, 0.f, 0.f, -INFINITY, -1};
  for (int v = tid; v < V; v += 256) {
    const float x = zr[v];
    if (x > t.av || t.ai < 0) {
      t.av = x;
      t.ai = v;
    }
    if (v == tg) t.zt = x;
    const float mn = fmaxf(t.m, x);
    t.s = (t.m > -INFINITY ? t.s * expf(t.m - mn) : 0.f) + expf(x - mn);
    t.m = mn;
  }
  float* d = sred + tid * 5;
  d[0] = t.m;
  d[1] = t.s;
  d[2] = t.zt;
  d[3] = t.av;
  d[4] = __int_as_float(t.ai);
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {  // fixed tree
    if (tid < o) {
      float* p = sred + tid * 5;
      const float* q = sred + (tid + o) * 5;
      RowState x{p[0], p[1], p[2], p[3], __float_as_int(p[4])};
      state_merge(x, RowState{q[0], q[1], q[2], q[3], __float_as_int(q[4])});
      p[0] = x.m;
      p[1] = x.s;
      p[2] = x.zt;
      p[3] = x.av;
      p[4] = __int_as_float(x.ai);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const long long SR = R;
    part[r] = sred[0];
    part[SR + r] = sred[1];
    part[2 * SR + r] = sred[2];
    part[3 * SR + r] = sred[3];
    part[4 * SR + r] = sred[4];
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

// splits of the vocabulary for `rows` output rows: a pure function of the shape (the reduction order follows it)
void mlm_split(int rows, int V, int* splits, int* tps) {
  const int ntv = (V + MLM_BV - 1) / MLM_BV, nrb = (rows + MLM_BR - 1) / MLM_BR;
  int s = (MLM_TARGET_WGS + nrb - 1) / nrb;
  s = s < 1 ? 1 : (s > ntv ? ntv : s);
  *tps = (ntv + s - 1) / s;
  *splits = (ntv + *tps - 1) / *tps;
}

// workspace: 5 floats per (split, row), then 2 per row (mlm_finalize_rows_kernel's rowres)
long long mlm_ws_floats(int splits, int R) { return (5LL * splits + 2) * R; }

void mlm_finalize(float* ws, int splits, int R, const long long* tgt, float* lse, float* row_loss, float* mean_loss,
                  long long* n_correct, hipStream_t stream) {
  float* rowres = ws + 5LL * splits * R;
  hipLaunchKernelGGL(mlm_finalize_rows_kernel, dim3((R + 3) / 4), dim3(256), 0, stream, ws, splits, R, tgt, lse,
                     row_loss, rowres);
  hipLaunchKernelGGL(mlm_mean_kernel, dim3(1), dim3(256), 0, stream, rowres, R, mean_loss, n_correct);
}

int mlm_shape_ok(int R, int V, int H) {
  if (R <= 0 || V <= 0 || H <= 0) {
    set_error("mlm: empty shape");
    return VCG_ERR_INVALID;
  }
  if (H % 8 != 0 || H > MLM_MAX_H) {
    set_error("mlm: H must be a multiple of 8, at most 4096");
    return VCG_ERR_UNSUPPORTED;
  }
  return VCG_OK;
}

}  // namespace

}  // namespace vcg

using namespace vcg;

VCG_API long long vcg_mlm_loss_ws_bytes(int R, int V, int H) {
  (void)H;
  if (R <= 0 || V <= 0) return 0;
  int splits, tps;
  mlm_split(R, V, &splits, &tps);
  return mlm_ws_floats(splits, R) * 4;
}

VCG_API int vcg_mlm_loss_fwd(const void* hidden, int rows_total, const long long* rows, const void* W,
                             const long long* targets, int R, int V, int H, float* ws, long long ws_bytes, float* lse,
                             float* row_loss, float* mean_loss, long long* n_correct, hipStream_t stream) {
  if (int rc = mlm_shape_ok(R, V, H)) return rc;
  VCG_REQUIRE(hidden && W && targets && ws, "null argument");
  VCG_REQUIRE(rows_total > 0, "rows_total must be positive");
  VCG_REQUIRE((((uintptr_t)hidden | (uintptr_t)W) & 15) == 0, "hidden and W must be 16-B aligned");
  VCG_REQUIRE(ws_bytes >= vcg_mlm_loss_ws_bytes(R, V, H), "workspace too small");
  MlmArgs a{};
  a.X = reinterpret_cast<const bf16_t*>(hidden);
  a.rows = rows;
  a.W = reinterpret_cast<const bf16_t*>(W);
  a.tgt = targets;
  a.rows_total = rows_total; a.R = R; a.V = V; a.H = H;
  mlm_split(R, V, &a.splits, &a.tiles_per_split);
  a.part = ws;
  hipLaunchKernelGGL(mlm_tile_kernel<MLM_LOSS>, dim3((R + MLM_BR - 1) / MLM_BR, a.splits), dim3(256), 0, stream, a);
  mlm_finalize(ws, a.splits, R, targets, lse, row_loss, mean_loss, n_correct, stream);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_mlm_loss_bwd(const void* hidden, int rows_total, const long long* rows, const void* W,
                             const long long* targets, const float* lse, const float* dloss, int R, int V, int H,
                             void* dZ, long long ldz, hipStream_t stream) {
  if (int rc = mlm_shape_ok(R, V, H)) return rc;
  VCG_REQUIRE(hidden && W && targets && lse && dloss && dZ, "null argument");
  VCG_REQUIRE(rows_total > 0, "rows_total must be positive");
  VCG_REQUIRE((((uintptr_t)hidden | (uintptr_t)W | (uintptr_t)dZ) & 15) == 0, "hidden, W and dZ must be 16-B aligned");
  VCG_REQUIRE(ldz == ((long long)V + 7) / 8 * 8, "ldz must be V rounded up to a multiple of 8");
  MlmArgs a{};
  a.X = reinterpret_cast<const bf16_t*>(hidden);
  a.rows = rows;
  a.W = reinterpret_cast<const bf16_t*>(W);
  a.tgt = targets;
  a.rows_total = rows_total; a.R = R; a.V = V; a.H = H;
  mlm_split(R, V, &a.splits, &a.tiles_per_split);
  a.lse = lse;
  a.dloss = dloss;
  a.out = dZ;
  a.ldo = ldz;
  hipLaunchKernelGGL(mlm_tile_kernel<MLM_DZ>, dim3((R + MLM_BR - 1) / MLM_BR, a.splits), dim3(256), 0, stream, a);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_mlm_logits(const void* hidden, int rows, const void* W, int V, int H, float* logits, long long ldz,
                           hipStream_t stream) {
  if (int rc = mlm_shape_ok(rows, V, H)) return rc;
  VCG_REQUIRE(hidden && W && logits, "null argument");
  VCG_REQUIRE((((uintptr_t)hidden | (uintptr_t)W | (uintptr_t)logits) & 15) == 0, "16-B alignment");
  VCG_REQUIRE(ldz == ((long long)V + 7) / 8 * 8, "ldz must be V rounded up to a multiple of 8");
  MlmArgs a{};
  a.X = reinterpret_cast<const bf16_t*>(hidden);
  a.W = reinterpret_cast<const bf16_t*>(W);
  a.rows_total = rows; a.R = rows; a.V = V; a.H = H;
  mlm_split(rows, V, &a.splits, &a.tiles_per_split);
  a.out = logits;
  a.ldo = ldz;
  hipLaunchKernelGGL(mlm_tile_kernel<MLM_LOGITS>, dim3((rows + MLM_BR - 1) / MLM_BR, a.splits), dim3(256), 0, stream,
                     a);
  VCG_LAUNCH_CHECK();
  return VCG_OK;
}

VCG_API int vcg_mlm_reduce_f32(const float* logits, long long ldz, const long long* targets, int R, int V, float* ws,
                               long long ws_bytes, float* lse, float* row_loss, float* mean_loss,
                               long long* n_correct, hipStream_t stream) {
  VCG_REQUIRE(logits && targets && ws, "null argument");
  VCG_REQUIRE(R > 0 && V > 0 && ldz >= V, "bad shape");
  VCG_REQUIRE(ws_bytes >= mlm_ws_floats(1, R) * 4, "workspace too small");
  hipLaunchKernelGGL(mlm_rows_f32_kernel, dim3(R), dim3(256), 0, stream, logits, ldz, targets, R, V, ws);
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
