// Wide top-K: selection and merge for 65 <= K <= HHFM_TOPK_MAX_K
// (include/hhfm.h "Wide K"; DESIGN.md §K2 "Wide K").
//
// The narrow kernels hold a query's list one entry per lane, so they end at
// K = 64, and a register list of 1,024 entries is not possible.  Here one
// 256-thread workgroup owns a query and keeps T 64-bit keys in LDS:
//
//   keys[0, K)   the running list, sorted, best first
//   keys[K, T)   candidates appended since the last sort
//
// A key is (order-preserving score bits | 31 bits of kNoIdx - index | one bit),
// so "larger key" is exactly the strict (score desc, index asc) order of
// tf.nn.top_k.  The narrow kernels compare (score, index) pairs, for which +0
// and -0 are equal scores ordered by index; the key therefore carries the
// score bits of +0 for either zero and remembers a -0 in its lowest bit, below
// the index, where it cannot decide a comparison (indices of one row are
// unique) and from where the original bits are written out again.  Keys of one
// row are unique, hence the top-K set is unique and the order in which
// candidates are appended cannot matter.  Ids lie in [0, 2^31); kNoIdx is the
// empty slot's.
//
// The threshold thr is the list's K-th key (0, below every key, until K
// entries exist).  A batch of candidates is filtered by `key > thr`; every
// wave reserves room for its survivors with one LDS atomic and writes them by
// ballot + prefix count.  A wave whose reservation does not fit writes nothing
// and reports it; the workgroup then sorts all T keys (bitonic, descending),
// which leaves the best K in front and raises thr, and the waves that did not
// fit filter again.  One wave's survivors of one batch are at most T - K_max,
// so after a sort the first wave to reserve always fits: the loop ends after
// at most four sorts per batch whatever the input (all survive: ascending
// scores; all tie: only the K lowest indices ever pass once the list is full).
#include "topk_wide.h"

#include "hhfm_common.h"

#ifndef HHFM_TOPK_NT
#define HHFM_TOPK_NT 1    // non-temporal score loads, as in topk_common.h
#endif

namespace hhfm {

namespace {

// (topk_common.h; that header's launchers would instantiate the narrow
// kernels a second time here)
constexpr float kNegInf = -__builtin_huge_valf();
constexpr int32_t kNoIdx = 0x7fffffff;
HHFM_DEV int lane_id() { return threadIdx.x & (kWave - 1); }

constexpr int kWideThreads = 256;
// T keys of LDS: 1,024 up to K = kWideSmallK, else 2,048; a wave's survivors
// of one batch (64 NE) must fit behind the longest list that T serves
constexpr int kWideSmallK = 256;
constexpr bool wide_batch_fits(int T, int NE) {
  return kWave * NE <= T - (T >= 2 * HHFM_TOPK_MAX_K ? HHFM_TOPK_MAX_K : kWideSmallK);
}

// (the score half is catalog_fused.h's ukey / ukey_inv)
HHFM_DEV uint32_t wide_ukey(float f) {
  const uint32_t b = __float_as_uint(f);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
HHFM_DEV float wide_ukey_inv(uint32_t k) {
  return __uint_as_float(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xffffffffu));
}
HHFM_DEV uint64_t wide_key(float s, int32_t i) {
  const uint32_t b = __float_as_uint(s);
  const bool negzero = b == 0x80000000u;
  const uint32_t lo = ((uint32_t)(kNoIdx - i) << 1) | (negzero ? 1u : 0u);
  return ((uint64_t)wide_ukey(negzero ? 0.f : s) << 32) | lo;
}
HHFM_DEV int32_t wide_key_index(uint64_t key) { return kNoIdx - (int32_t)((uint32_t)key >> 1); }
HHFM_DEV float wide_key_score(uint64_t key) {
  return (key & 1ull) ? -0.f : wide_ukey_inv((uint32_t)(key >> 32));
}

// state[0]: entries reserved in keys[K, T) since the last sort (may pass the
// capacity); state[1]: the smallest reservation that did not fit
HHFM_DEV void wide_reset(uint64_t* keys, int* state, int K) {
  __syncthreads();   // the previous query's list is still being written out
  for (int i = threadIdx.x; i < K; i += kWideThreads) keys[i] = 0ull;
  if (threadIdx.x == 0) {
    state[0] = 0;
    state[1] = 0x7fffffff;
  }
  __syncthreads();
}

// bitonic sort of keys[0, T), descending; ends on a barrier
template <int T>
HHFM_DEV void wide_sort(uint64_t* keys) {
  const int t = threadIdx.x;
#pragma unroll 1
  for (int size = 2; size <= T; size <<= 1) {
#pragma unroll 1
    for (int d = size >> 1; d >= 1; d >>= 1) {
      __syncthreads();
#pragma unroll
      for (int m = 0; m < T / 2 / kWideThreads; ++m) {
        const int p = t + m * kWideThreads;
        const int i = ((p & ~(d - 1)) << 1) | (p & (d - 1));
        const int j = i | d;
        const uint64_t a = keys[i], b = keys[j];
        const bool desc = (i & size) == 0;   // size == T: every pair
        if ((a < b) == desc) {
          keys[i] = b;
          keys[j] = a;
        }
      }
    }
  }
  __syncthreads();
}

// Sort the list with the appended candidates; the new threshold.  Called by
// the whole workgroup behind a barrier that follows the last append.
template <int T>
HHFM_DEV uint64_t wide_flush(uint64_t* keys, int* state, int K) {
  // written slots: every reservation below the first that did not fit
  const int n = state[0] < state[1] ? state[0] : state[1];
  for (int i = K + n + threadIdx.x; i < T; i += kWideThreads) keys[i] = 0ull;
  wide_sort<T>(keys);   // (its first barrier also orders the reads of state)
  if (threadIdx.x == 0) {
    state[0] = 0;
    state[1] = 0x7fffffff;
  }
  const uint64_t thr = keys[K - 1];
  __syncthreads();
  return thr;
}

// Append this thread's NE candidate keys (0 = none) that pass thr.  A wave's
// survivors number at most 64 NE <= T - K (the launcher's choice of T).
template <int T, int NE>
HHFM_DEV void wide_push(const uint64_t (&ck)[NE], uint64_t& thr, uint64_t* keys, int* state,
                        int K) {
  const int cap = T - K;
  bool pending = true;
  for (;;) {
    bool ovf = false;
    if (pending) {
      int wt = 0;
#pragma unroll
      for (int j = 0; j < NE; ++j) wt += __popcll(__ballot(ck[j] > thr));
      if (wt > 0) {
        int base = 0;
        if (lane_id() == 0) base = atomicAdd(&state[0], wt);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base + wt <= cap) {
          int off = K + base;
#pragma unroll
          for (int j = 0; j < NE; ++j) {
            const bool pass = ck[j] > thr;
            const uint64_t m = __ballot(pass);
            if (pass)
              keys[off + (int)__builtin_amdgcn_mbcnt_hi(
                             (uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] =
                  ck[j];
            off += __popcll(m);
          }
        } else {
          ovf = true;
          if (lane_id() == 0) atomicMin(&state[1], base);
        }
      }
      pending = ovf;
    }
    if (!__syncthreads_or(ovf)) break;   // (a barrier: the appends are visible behind it)
    thr = wide_flush<T>(keys, state, K);
  }
}

// final sort, then the K best to out_s / out_i (+ base on real entries)
template <int T>
HHFM_DEV void wide_emit(uint64_t* keys, int* state, int K, int32_t base, float* out_s,
                        int32_t* out_i) {
  wide_flush<T>(keys, state, K);
  for (int i = threadIdx.x; i < K; i += kWideThreads) {
    const uint64_t key = keys[i];
    const float s = key ? wide_key_score(key) : kNegInf;
    const int32_t id = key ? wide_key_index(key) : kNoIdx;
    out_s[i] = s;
    out_i[i] = id == kNoIdx ? kNoIdx : id + base;
  }
}

}  // namespace

// One workgroup per row.  The row is read in batches of U 16-byte loads per
// thread, all issued before the first is used.  The loads are aligned to 16
// bytes in memory, not to the row: a row that starts off a 16-byte boundary
// (the public dense entry takes any ld) begins with a partial vector, and
// partial vectors — the head, and the tail at column N — are read one guarded
// element at a time, so no column outside [0, N) is touched.
//
// EXCL (hhfm_topk_dense_excl, whose matrix is read-only, so it cannot be
// masked): a candidate that passes the threshold is looked up in the query's
// ascending list of table rows (column i is row irb + i) by binary search and
// dropped when listed.  Only survivors are looked up — every column while the
// list fills, few afterwards — and list entries are only compared.
template <int T, int U, bool EXCL>
__global__ __launch_bounds__(kWideThreads) void topk_wide_dense_kernel(
    const float* __restrict__ S, int64_t B, int32_t N, int64_t ld, int K, int32_t base,
    float* __restrict__ out_s, int32_t* __restrict__ out_i,
    const int64_t* __restrict__ excl_ptr, const int32_t* __restrict__ excl_rows, int64_t irb) {
  static_assert(wide_batch_fits(T, 4 * U), "a wave's batch fits behind the longest list");
  __shared__ uint64_t keys[T];
  __shared__ int state[2];
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    wide_reset(keys, state, K);
    uint64_t thr = 0ull;
    const float* row = S + b * ld;
    const int mis = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3);
    const int32_t* xr = excl_rows;   // the query's list: xn entries (a list holds < 2^31)
    int xn = 0;
    if (EXCL && excl_rows) {
      const int64_t x0 = excl_ptr[b];
      xr = excl_rows + x0;
      xn = (int)(excl_ptr[b + 1] - x0);
    }
#pragma unroll 1
    for (int64_t c0 = -mis; c0 < N; c0 += (int64_t)kWideThreads * 4 * U) {
      f32x4_t v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t c = c0 + (int64_t)(u * kWideThreads + (int)threadIdx.x) * 4;
        if (c >= 0 && c + 3 < N) {
          const f32x4_t* p = reinterpret_cast<const f32x4_t*>(row + c);
          v[u] = HHFM_TOPK_NT ? __builtin_nontemporal_load(p) : *p;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[u][e] = (c + e >= 0 && c + e < N) ? row[c + e] : 0.f;
        }
      }
      uint64_t ck[4 * U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t c = c0 + (int64_t)(u * kWideThreads + (int)threadIdx.x) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          ck[u * 4 + e] = (c + e >= 0 && c + e < N) ? wide_key(v[u][e], (int32_t)(c + e)) : 0ull;
      }
      if (EXCL && xn > 0) {
#pragma unroll 1
        for (int j = 0; j < 4 * U; ++j) {
          if (ck[j] > thr) {
            const int64_t want = irb + wide_key_index(ck[j]);
            int a = 0, e = xn;
            while (a < e) {
              const int mid = a + ((e - a) >> 1);
              if ((int64_t)xr[mid] < want) a = mid + 1; else e = mid;
            }
            if (a < xn && (int64_t)xr[a] == want) ck[j] = 0ull;
          }
        }
      }
      wide_push<T, 4 * U>(ck, thr, keys, state, K);
    }
    wide_emit<T>(keys, state, K, base, out_s + b * K, out_i + b * K);
  }
}

// The same list over the R K entries of a query's lists.  An empty slot
// (-inf, kNoIdx) is the smallest key an entry can have, so it ranks behind
// every real entry and comes out as it went in.
template <int T, int U>
__global__ __launch_bounds__(kWideThreads) void topk_wide_merge_kernel(
    const float* __restrict__ in_s, const int32_t* __restrict__ in_i, int R, int64_t B, int K,
    int64_t stride_r, int64_t stride_b, float* __restrict__ out_s, int32_t* __restrict__ out_i) {
  constexpr int NE = 4 * U;
  static_assert(wide_batch_fits(T, NE), "a wave's batch fits behind the longest list");
  __shared__ uint64_t keys[T];
  __shared__ int state[2];
  const uint32_t total = (uint32_t)R * (uint32_t)K;   // < 2^31 (hhfm_topk_merge checks)
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    wide_reset(keys, state, K);
    uint64_t thr = 0ull;
    const float* qs = in_s + b * stride_b;
    const int32_t* qi = in_i + b * stride_b;
#pragma unroll 1
    for (uint32_t e0 = 0; e0 < total; e0 += kWideThreads * NE) {
      float s[NE];
      int32_t id[NE];
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        const uint32_t e = e0 + j * kWideThreads + threadIdx.x;
        const bool ok = e < total;
        const uint32_t r = ok ? e / (uint32_t)K : 0u;
        const int64_t off = (int64_t)r * stride_r + (ok ? e - r * (uint32_t)K : 0u);
        s[j] = ok ? qs[off] : 0.f;
        id[j] = ok ? qi[off] : 0;
      }
      uint64_t ck[NE];
#pragma unroll
      for (int j = 0; j < NE; ++j)
        ck[j] = e0 + j * kWideThreads + threadIdx.x < total ? wide_key(s[j], id[j]) : 0ull;
      wide_push<T, NE>(ck, thr, keys, state, K);
    }
    wide_emit<T>(keys, state, K, 0, out_s + b * K, out_i + b * K);
  }
}

static inline int wide_grid(int64_t B) { return (int)(B < (1 << 20) ? (B < 1 ? 1 : B) : (1 << 20)); }

void launch_topk_wide_dense(const float* S, int64_t B, int32_t N, int64_t ld, int K, int32_t base,
                            float* os, int32_t* oi, hipStream_t st) {
  if (K <= kWideSmallK)
    hipLaunchKernelGGL((topk_wide_dense_kernel<1024, 2, false>), dim3(wide_grid(B)),
                       dim3(kWideThreads), 0, st, S, B, N, ld, K, base, os, oi, nullptr, nullptr,
                       (int64_t)0);
  else
    hipLaunchKernelGGL((topk_wide_dense_kernel<2048, 4, false>), dim3(wide_grid(B)),
                       dim3(kWideThreads), 0, st, S, B, N, ld, K, base, os, oi, nullptr, nullptr,
                       (int64_t)0);
}

void launch_topk_wide_dense_excl(const float* S, int64_t B, int32_t N, int64_t ld, int K,
                                 int32_t base, float* os, int32_t* oi, hipStream_t st,
                                 const int64_t* xptr, const int32_t* xrows,
                                 int64_t item_row_begin) {
  if (K <= kWideSmallK)
    hipLaunchKernelGGL((topk_wide_dense_kernel<1024, 2, true>), dim3(wide_grid(B)),
                       dim3(kWideThreads), 0, st, S, B, N, ld, K, base, os, oi, xptr, xrows,
                       item_row_begin);
  else
    hipLaunchKernelGGL((topk_wide_dense_kernel<2048, 4, true>), dim3(wide_grid(B)),
                       dim3(kWideThreads), 0, st, S, B, N, ld, K, base, os, oi, xptr, xrows,
                       item_row_begin);
}

void launch_topk_wide_merge(const float* in_s, const int32_t* in_i, int R, int64_t B, int K,
                            int64_t stride_r, int64_t stride_b, float* os, int32_t* oi,
                            hipStream_t st) {
  if (K <= kWideSmallK)
    hipLaunchKernelGGL((topk_wide_merge_kernel<1024, 2>), dim3(wide_grid(B)), dim3(kWideThreads),
                       0, st, in_s, in_i, R, B, K, stride_r, stride_b, os, oi);
  else
    hipLaunchKernelGGL((topk_wide_merge_kernel<2048, 4>), dim3(wide_grid(B)), dim3(kWideThreads),
                       0, st, in_s, in_i, R, B, K, stride_r, stride_b, os, oi);
}

}  // namespace hhfm
