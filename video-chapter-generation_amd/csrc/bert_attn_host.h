// Host side of the fused BERT attention shared by bert_attn.hip (the C entry points, which check the arguments and
// launch the L <= 128 kernels) and bert_attn_long.hip (the launchers of the tiled kernels): the stats layout and the
// tiled launchers' prototypes.
#pragma once
#include "bert_attn_steps.h"

namespace vcg {
namespace attn {

// stats: float2 [B * nh][Lr] (row max, 1 / row sum) and, at L > 128, float [B * nh][Lr] behind them (the backward's D),
// Lr = stats_tiles(L) * 128: one tile at L <= 128, above it L rounded up to the tiled kernels' 128-row tiles (their
// grid is B * nh * stats_tiles(L) workgroups). stats_rows: the float2 entries, i.e. where D starts.
inline int stats_tiles(int L) { return L <= LT ? 1 : (L + LT - 1) / LT; }
inline long long stats_rows(int B, int nh, int L) { return (long long)B * nh * stats_tiles(L) * LT; }

}  // namespace attn

// 128 < Lmax <= 512, nT = stats_tiles(Lmax), causal: VCG_ATTN_CAUSAL was given; the other arguments are
// vcg_bert_attn_fwd/bwd_varlen's, already checked
int bert_attn_long_fwd(const void* qkv, const long long* mask, const int* seq, void* ctx, void* stats, int B, int nh,
                       int Lmax, int Lp, int nT, float scale, float dropout_p, unsigned long long seed, bool causal,
                       hipStream_t s);
int bert_attn_long_bwd(const void* qkv, const void* dctx, const long long* mask, const int* seq, void* stats,
                       void* dqkv, int B, int nh, int Lmax, int Lp, int nT, float scale, float dropout_p,
                       unsigned long long seed, bool causal, hipStream_t s);

}  // namespace vcg
