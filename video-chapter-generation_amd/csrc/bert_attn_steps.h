// The fused attention kernels' tile constants, MFMA fragment helpers and the steps the kernels are built from, each
// written once: the five self-attention kernels (bert_attn.hip: L <= 128, one workgroup per (sequence, head);
// bert_attn_long.hip: 128 < L <= 512, 128 x 128 tiles with an online softmax) and the three bf16 cross-attention
// kernels of pegasus.hip (Lq != Lk, separate Q and K | V buffers). What the packed and the padded paths, the forwards
// and the backwards, self- and cross-attention must agree on bit for bit -- the masking rule and the no-key convention
// (attn_prob, seq_has_key), the dropout counter (drop_row, dropout_frags), the dK | dV rule of a query tile
// (dkv_query_tile) -- is stated here and nowhere else. Every step is __forceinline__ and takes the lane
// decomposition (g, i) and the tile-skip bounds as arguments; a 256-thread workgroup of 4 waves is assumed throughout.
//
// MFMA: mfma_f32_16x16x32_bf16 (lane l = 16 g + i holds A[row i][k-set g], B[k-set g][col i], D[rows 4g..4g+3]
// [col i]). A k-step's 32 k indices only have to be the same SET on both operands, so a D fragment (4 consecutive
// rows per lane) feeds the next MFMA's operand straight from registers: rows {32s + 4g + r, 32s + 16 + 4g + r} of
// two adjacent D tiles form lane group g's k-set of k-step s (pack8).
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

// the k-set of one k-step from two adjacent D tiles (header comment)
__device__ __forceinline__ s16x8 pack8(const f32x4& a, const f32x4& b) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 u = {pack2(a[0], a[1]), pack2(a[2], a[3]), pack2(b[0], b[1]), pack2(b[2], b[3])};
  return __builtin_bit_cast(s16x8, u);
}

__device__ __forceinline__ uint4 ld16(const bf16_t* p, bool ok) {
  return ok ? *reinterpret_cast<const uint4*>(p) : make_uint4(0u, 0u, 0u, 0u);
}

// ---------------------------------------------------------------------------------------------- coordinates
// the dropout counter of (head z, query q, key 0) in a score space of Lrows queries per head and row pitch Lp: key
// k's is + k -- the unfused kernels' element index (self-attention: Head::drop_row; cross-attention: Lrows = Lq,
// Lp = Lk)
__device__ __forceinline__ uint64_t drop_row(int z, int Lrows, int q, int Lp) {
  return ((uint64_t)z * Lrows + q) * (uint64_t)Lp;
}

// Workgroup blockIdx.x = z * nT + tile of head z = b * nh + h (nT = 1: the L <= 128 kernels). Sequence b is rows
// row0 .. row0 + L - 1 of qkv / ctx (packed: seq[b] .. seq[b + 1] - 1; else b Lmax .. + Lmax - 1); the stats, the D
// vector and the dropout counters keep the padded [B * nh][...] index space.
struct Head {
  int z, tile0, row0, L, H;  // tile0: first query / key row of this workgroup's tile; H = nh * 64
  int tid, w, g, i;          // thread, wave, and the MFMA lane decomposition lane = 16 g + i
  long long ld;              // row pitch of qkv / dqkv (3 H); that of ctx / dctx is H
  long long qo, co, so;      // offsets of (b, h): Q in qkv / dqkv (K at + H, V at + 2 H), ctx / dctx, stats / D rows
  int Lmax, Lp;

  __device__ __forceinline__ Head(int nh, int nT, const int* seq, int Lmax_, int Lp_) : Lmax(Lmax_), Lp(Lp_) {
    z = blockIdx.x / nT;
    tile0 = LT * (blockIdx.x - z * nT);
    const int b = z / nh, h = z - b * nh;
    H = nh * DH;
    ld = 3LL * H;
    tid = threadIdx.x;
    w = tid >> 6;
    g = (tid & 63) >> 4;
    i = tid & 15;
    row0 = seq ? seq[b] : b * Lmax;
    L = seq ? seq[b + 1] - row0 : Lmax;
    qo = (long long)row0 * ld + h * DH;
    co = (long long)row0 * H + h * DH;
    so = (long long)z * (nT * LT);
  }
  // the dropout counter of (z, query q, key 0): key k's is + k -- the unfused kernels' element index
  __device__ __forceinline__ uint64_t drop_row(int q) const { return attn::drop_row(z, Lmax, q, Lp); }
};

// ---------------------------------------------------------------------------------------------- causal rule
// CAUSAL instantiations: key j is visible to query i iff j <= i and the key is valid (its mask entry set). A query
// without any visible key keeps the no-key convention (attn_prob): uniform over all L keys in range, future ones
// included -- which is what HF's OpenAIGPT computes for a fully masked sequence. Such a row exists iff the
// sequence's first key is masked (every query sees key 0 otherwise), so that one block-uniform flag decides
// whether tiles wholly above the diagonal may be skipped: skipping is what the NOSKIP bounds below turn off.
template <bool CAUSAL>
__device__ __forceinline__ bool visible(bool valid_key, int key, int q) {
  return valid_key && (!CAUSAL || key <= q);
}
constexpr int NOSKIP = 1 << 20;  // a first-query / first-key bound under which no tile lies above the diagonal
// may tiles wholly above the diagonal be skipped? (not when some query has no visible key: see above)
__device__ __forceinline__ bool causal_skip(const long long* mask, long long row0, int L) {
  return mask == nullptr || L <= 0 || mask[row0] != 0;
}
// do rows row .. row + L - 1 of the mask, one sequence's keys, hold any valid key? (mask NULL: yes.) Block-uniform;
// every thread must call it (a barrier). Without one the sequence attends uniformly: attn_prob's no-key convention.
// (The cross-attention forwards' scan. bert_attn_long_fwd_kernel keeps its own lines, which differ in the stride -- the
// constant 256 -- and in reaching the barrier with a NULL mask too: through this function its L >= 384 timings moved
// by 0.5 %, profiles/attn_dkv_shared_ab.txt.)
__device__ __forceinline__ bool seq_has_key(const long long* mask, long long row, int L) {
  if (mask == nullptr) return true;
  int any = 0;
  for (int k = threadIdx.x; k < L; k += blockDim.x) any |= mask[row + k] != 0;
  return __syncthreads_or(any) != 0;
}

// the causal cut of dS: no gradient reaches a future key's score -- HF's `w * b + -1e4 (1 - b)` fill multiplies it by
// b = 0. P is zero there anyway, except in a row without a visible key (uniform over all L keys: D still sums over all)
template <bool CAUSAL>
__device__ __forceinline__ float causal_ds(float dS, int key, int q) {
  return (CAUSAL && key > q) ? 0.f : dS;
}

// ---------------------------------------------------------------------------------------------- loads
// rows 0 .. 127 of a [nrows][ld] row-major source (rows >= nrows zero) -> the swizzled row-major tile rm[row][64]
__device__ __forceinline__ void load_rm(const bf16_t* src, long long ld, int nrows, bf16_t* rm, int tid) {
  for (int c = tid; c < LT * 8; c += 256) {
    const int r = c >> 3, ch = c & 7;
    *reinterpret_cast<uint4*>(rm + r * DH + 8 * swz(r, ch)) = ld16(src + (long long)r * ld + 8 * ch, r < nrows);
  }
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

// the flags of a tile's 128 keys: key k < nkeys (rows row + k of the mask) is valid if its mask entry is set (mask NULL:
// every key in range is)
__device__ __forceinline__ void load_key_flags(uint8_t* kval, const long long* mask, long long row, int nkeys, int tid) {
  if (tid < LT) kval[tid] = tid < nkeys && (mask == nullptr || mask[row + tid] != 0);
}

// a wave's 2 x 2 MFMA B operands f[t][s]: rows r0 + 16 t + i, k-set 4 s + g of a [nrows][ld] row-major HBM source
// (rows >= nrows zero). Q, dO (r0: the wave's first query) and K, V (its first key) of all five kernels.
__device__ __forceinline__ void load_frags(s16x8 (&f)[2][2], const bf16_t* src, long long ld, int r0, int nrows, int g,
                                           int i) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int r = r0 + 16 * t + i;
      f[t][s] = __builtin_bit_cast(s16x8, ld16(src + (long long)r * ld + 8 * (4 * s + g), r < nrows));
    }
}

// ---------------------------------------------------------------------------------------------- key-major tiles
// (the forwards and dq: a lane holds [key r0 + 16 kt + 4 g + r][query 16 qt + i of the wave's 32])
// acc[qt][kt] = A B^T over the head dim: A = rows r0 + 16 kt .. + 15 of the swizzled LDS tile a (K for S^T, V for
// dPd^T), B = the wave's Q / dO fragments; tiles whose rows start at or past nrows stay zero. CAUSAL: qlo is the wave's
// first query in the tile's key coordinates (NOSKIP: no skipping); a 16 x 16 tile whose first key lies past its last
// query (16 qt + 15 of the wave) is wholly above the diagonal and stays zero
template <int NT, bool CAUSAL = false>
__device__ __forceinline__ void key_tiles(f32x4 (&acc)[2][NT], const bf16_t* a, int r0, int nrows,
                                          const s16x8 (&bf)[2][2], int g, int i, int qlo = NOSKIP) {
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) acc[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
    if (r0 + 16 * kt < nrows && (!CAUSAL || r0 + 16 * kt <= qlo + 31)) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const s16x8 af = frag_rm(a, r0 + 16 * kt + i, 4 * s + g);
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
          if (!CAUSAL || r0 + 16 * kt <= qlo + 16 * qt + 15)
            acc[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[qt][s], acc[qt][kt], 0, 0, 0);
      }
    }
}

// bit 4 kt + r: key r0 + 16 kt + 4 g + r of the tile is valid (kval: the tile's key flags, 0 past the end)
template <int NT>
__device__ __forceinline__ uint32_t key_bits(const uint8_t* kval, int r0, int g) {
  uint32_t vb = 0;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) vb |= kval[r0 + 16 * kt + 4 * g + r] ? (1u << (4 * kt + r)) : 0u;
  return vb;
}

// the forward's step from a query row's eight probability tiles e[kt] to the four B fragments of Pd = dropout(e * inv):
// counter rowi + key (rowi: Head::drop_row(q) + the tile's first key), a row past the end (!row) all zero. nk: the
// k-steps from key nk on hold only zeros (the causal diagonal tile: keys past the wave's last query) and are not hashed
__device__ __forceinline__ void dropout_frags(s16x8 (&pf)[4], const f32x4 (&e)[8], bool row, uint64_t rowi, float inv,
                                              float rs, float p, uint64_t seed, int g, int nk = NOSKIP) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    f32x4 a, c;
    if (32 * s >= nk) {  // (wave-uniform)
      pf[s] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
      continue;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k0 = 32 * s + 4 * g + r, k1 = k0 + 16;
      const float p0 = e[2 * s][r] * inv, p1 = e[2 * s + 1][r] * inv;
      a[r] = (row && dropout_keep(seed, rowi + k0, p)) ? p0 * rs : 0.f;
      c[r] = (row && dropout_keep(seed, rowi + k1, p)) ? p1 * rs : 0.f;
    }
    pf[s] = pack8(a, c);
  }
}

// O^T += V^T Pd^T over a tile's nkeys keys (A = V^T from LDS, B = Pd from registers; k-steps past the end skipped --
// the causal kernels pass the end of the wave's visible keys when that is sooner)
__device__ __forceinline__ void pv_step(f32x4 (&oacc)[4][2], const bf16_t* Vt, const s16x8 (&pf)[2][4], int nkeys, int g,
                                        int i) {
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (32 * s < nkeys) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const s16x8 vf = frag_split(Vt, 16 * dt + i, 32 * s + 4 * g);
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) oacc[dt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qt][s], oacc[dt][qt], 0, 0, 0);
      }
    }
}

// ---------------------------------------------------------------------------------------------- query-major tiles
// (the L <= 128 backward and dkv: a lane holds [query 16 qt + 4 g + r][key 16 kt + i of the wave's 32])
// acc[qt][kt] = A B^T over the head dim: A = rows r0 + 16 qt .. + 15 of the swizzled LDS tile a (Q for S, dO for dPd),
// B = the wave's K / V fragments; tiles whose rows start at or past nrows stay zero. CAUSAL: klo is the wave's first
// key in the tile's query coordinates (-NOSKIP: no skipping); a 16 x 16 tile whose last query lies before its first
// key (16 kt of the wave) is wholly above the diagonal and stays zero
template <int NT, bool CAUSAL = false>
__device__ __forceinline__ void query_tiles(f32x4 (&acc)[NT][2], const bf16_t* a, int r0, int nrows,
                                            const s16x8 (&bf)[2][2], int g, int i, int klo = -NOSKIP) {
#pragma unroll
  for (int qt = 0; qt < NT; ++qt)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) acc[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int qt = 0; qt < NT; ++qt)
    if (r0 + 16 * qt < nrows && (!CAUSAL || r0 + 16 * qt + 15 >= klo)) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const s16x8 af = frag_rm(a, r0 + 16 * qt + i, 4 * s + g);
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
          if (!CAUSAL || r0 + 16 * qt + 15 >= klo + 16 * kt)
            acc[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[kt][s], acc[qt][kt], 0, 0, 0);
      }
    }
}

// The backward's P from a score and the saved (row max, 1 / row sum): a row without any key is saved with max = -inf
// and 1 / sum = 1 / L and is uniform over the L keys in range, masked or not; otherwise a masked key has P = 0
// (valid_key: the causal kernels pass visible<true>(...), so a future key counts as masked)
__device__ __forceinline__ float attn_prob(float score, float scale, float2 mi, bool valid_key, bool key_in_range,
                                           bool row_in_range) {
  if (!row_in_range) return 0.f;
  if (mi.x == -INFINITY) return key_in_range ? mi.y : 0.f;
  return valid_key ? __expf(score * scale - mi.x) * mi.y : 0.f;
}

// one k-step of dV^T += dO^T Pd and dK^T += Q^T dS: the k-set is queries {col + 4 g + r, col + 16 + 4 g + r}, i.e. the
// adjacent query tiles (p0, p1) of Pd and (s0, s1) of dS, each [kt]; A = dO^T / Q^T from LDS at column col
__device__ __forceinline__ void dvdk_step(f32x4 (&dv)[4][2], f32x4 (&dk)[4][2], const f32x4 (&p0)[2],
                                          const f32x4 (&p1)[2], const f32x4 (&s0)[2], const f32x4 (&s1)[2],
                                          const bf16_t* dOt, const bf16_t* Qt, int col, int g, int i) {
  s16x8 pb[2], sb[2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    pb[kt] = pack8(p0[kt], p1[kt]);
    sb[kt] = pack8(s0[kt], s1[kt]);
  }
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const s16x8 oa = frag_split(dOt, 16 * dt + i, col + 4 * g);
    const s16x8 qa = frag_split(Qt, 16 * dt + i, col + 4 * g);
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      dv[dt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oa, pb[kt], dv[dt][kt], 0, 0, 0);
      dk[dt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa, sb[kt], dk[dt][kt], 0, 0, 0);
    }
  }
}

// One 128-query tile of a dK | dV workgroup (bert_attn_long_dkv_kernel, pegasus.hip's cross_attn_kv_dkv_kernel): the
// workgroup owns a key tile, wave w its keys k0 + 32 w .. + 31 (K / V fragments kf / vf, validity kv, indices keyi),
// and adds this query tile's share to dv / dk. The operands are one head's: query q is row q of Q / dO / stats / D.
struct DkvOperands {
  const bf16_t *q, *dO;   // row 0 of the head's Q and dO
  long long ldq, lddo;    // their row pitches
  const float2* stats;    // the saved row statistics (SUM: (max, sum), cross-attention; else (max, 1 / sum))
  const float* D;         // the dq kernel's D = rowsum(P o dP)
  int nq, nk;             // queries and keys of the sequence
  int z, Lrows, Lp;       // the dropout counter's space (drop_row)
  float scale, p;         // score scale, dropout p
  uint64_t seed;
};
struct DkvLds {
  bf16_t *Qs, *dOs;  // [LT][64] swizzled row-major
  bf16_t *Qt, *dOt;  // [64][TP] transposed
  float2* st;        // [LT], attn_prob's form
  float* Ds;         // [LT]
};
// Stages the tile (queries q0 .. q0 + 127, rows past nq zero), then sweeps it in two halves of 64: S = Q K^T and
// dPd = dO V^T (query_tiles), P from the statistics, Pd = keep P / (1 - p), dS = scale P o (keep dPd / (1 - p) - D),
// dV^T += dO^T Pd and dK^T += Q^T dS (dvdk_step). Two barriers; every thread of the workgroup must call it, a wave
// past the keys' end (!wact) only loads and syncs. MK: the causal rule acts inside this tile -- klo is the wave's
// first key in the tile's query coordinates (-NOSKIP: nothing skipped), and the halves, 16 x 16 tiles and k-steps
// wholly above the diagonal are skipped; !MK is the non-causal body (every key visible to every query, klo unused).
template <bool MK, bool SUM>
__device__ __forceinline__ void dkv_query_tile(f32x4 (&dv)[4][2], f32x4 (&dk)[4][2], const DkvOperands& op,
                                               const DkvLds& lds, int q0, const s16x8 (&kf)[2][2],
                                               const s16x8 (&vf)[2][2], const bool (&kv)[2], const int (&keyi)[2],
                                               bool wact, int klo, int tid, int g, int i) {
  const int Lq = op.nq - q0;  // queries from this tile on (>= 128: a full tile)
  const float rs = op.p > 0.f ? 1.f / (1.f - op.p) : 1.f;
  load_transpose(op.q + (long long)q0 * op.ldq, op.ldq, Lq, lds.Qt, lds.Qs, tid);
  load_transpose(op.dO + (long long)q0 * op.lddo, op.lddo, Lq, lds.dOt, lds.dOs, tid);
  if (tid < LT) {
    float2 m = tid < Lq ? op.stats[q0 + tid] : make_float2(0.f, 0.f);
    if (SUM && tid < Lq) m.y = 1.f / m.y;  // attn_prob's form
    lds.st[tid] = m;
    lds.Ds[tid] = tid < Lq ? op.D[q0 + tid] : 0.f;
  }
  __syncthreads();
#pragma unroll 1
  for (int qh = 0; qh < (wact ? LT : 0) && qh < Lq; qh += 64) {  // the tile's queries in two halves of 64
    if (MK && qh + 63 < klo) continue;  // (the half lies before the wave's first key)
    f32x4 sacc[4][2], pacc[4][2];  // lane holds S / dPd [query q0 + qh + 16 qt + 4 g + r][key k0 + 32 w + 16 kt + i]
    query_tiles<4, MK>(sacc, lds.Qs, qh, Lq, kf, g, i, klo);
    query_tiles<4, MK>(pacc, lds.dOs, qh, Lq, vf, g, i, klo);
#pragma unroll
    for (int qt = 0; qt < 4; ++qt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ql = qh + 16 * qt + 4 * g + r;
        const float2 mi = lds.st[ql];
        const float D = lds.Ds[ql];
        const uint64_t rowi = drop_row(op.z, op.Lrows, q0 + ql, op.Lp);
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          const int key = keyi[kt];
          const float P = attn_prob(sacc[qt][kt][r], op.scale, mi, visible<MK>(kv[kt], key, q0 + ql), key < op.nk,
                                    ql < Lq);
          const bool keep = ql < Lq && key < op.nk && dropout_keep(op.seed, rowi + key, op.p);
          const float dP = keep ? pacc[qt][kt][r] * rs : 0.f;
          sacc[qt][kt][r] = keep ? P * rs : 0.f;                                     // Pd
          pacc[qt][kt][r] = causal_ds<MK>(op.scale * P * (dP - D), key, q0 + ql);  // dS
        }
      }
    // dV^T += dO^T Pd, dK^T += Q^T dS (k-step s: queries {32 s + 4 g + r, 32 s + 16 + 4 g + r} of the half)
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if (qh + 32 * s < Lq && (!MK || qh + 32 * s + 31 >= klo))
        dvdk_step(dv, dk, sacc[2 * s], sacc[2 * s + 1], pacc[2 * s], pacc[2 * s + 1], lds.dOt, lds.Qt, qh + 32 * s, g,
                  i);
  }
  __syncthreads();  // every wave is done with this tile before the next one overwrites it
}

// ---------------------------------------------------------------------------------------------- store
// the lane's 16 values acc[dt][t][r] * mul of a 64-wide bf16 row (d = 16 dt + 4 g + r; dst already at + 4 g)
__device__ __forceinline__ void store_row64(bf16_t* dst, const f32x4 (&acc)[4][2], int t, float mul = 1.f) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    *reinterpret_cast<uint2*>(dst + 16 * dt) = make_uint2(pack2(acc[dt][t][0] * mul, acc[dt][t][1] * mul),
                                                          pack2(acc[dt][t][2] * mul, acc[dt][t][3] * mul));
}

}  // namespace attn
}  // namespace vcg
