// Wide top-K (65 <= K <= HHFM_TOPK_MAX_K): launchers of topk_wide.hip.
//
// The narrow kernels (topk_common.h) keep a list one entry per lane of a wave,
// which ends at 64.  The wide kernels keep it in LDS, one 256-thread workgroup
// per query; the order is the same strict (score desc, index asc) one, so a
// wide list is the narrow list carried further (include/hhfm.h "Wide K").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/hhfm.h"

namespace hhfm {

// narrow / wide split of every host function: K <= kTopkNarrowMaxK takes the
// wave-list kernels, larger K (up to HHFM_TOPK_MAX_K) the LDS-list kernels
constexpr int kTopkNarrowMaxK = 64;

// Top K of every row of S [B][N] (leading dimension ld; any alignment) into
// os / oi [B][K]; ids are column + base.  N < K is allowed here (the blocked
// catalog route's short last block): the row's N entries, then -inf / kNoIdx.
// Columns >= N are never read.
void launch_topk_wide_dense(const float* S, int64_t B, int32_t N, int64_t ld, int K, int32_t base,
                            float* os, int32_t* oi, hipStream_t st);

// The same over each row's non-listed columns, S only read (the lists of
// hhfm_topk_dense_excl: xptr [B + 1], xrows table rows strictly ascending per
// query, column i being table row item_row_begin + i; xrows NULL: all empty).
void launch_topk_wide_dense_excl(const float* S, int64_t B, int32_t N, int64_t ld, int K,
                                 int32_t base, float* os, int32_t* oi, hipStream_t st,
                                 const int64_t* xptr, const int32_t* xrows,
                                 int64_t item_row_begin);

// R sorted lists per query, list r of query b at in_* + r stride_r + b stride_b
// (K entries, -inf / kNoIdx slots empty), into os / oi [B][K].  The outputs
// must not overlap the inputs.
void launch_topk_wide_merge(const float* in_s, const int32_t* in_i, int R, int64_t B, int K,
                            int64_t stride_r, int64_t stride_b, float* os, int32_t* oi,
                            hipStream_t st);

}  // namespace hhfm
