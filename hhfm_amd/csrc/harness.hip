// H3 / H5 on the device — the evaluation harness's per-element work
// (SURVEY §8f items 2 and 4).
//
//   hhfm_pf_contains replaces the `neg in self.data.positive_feedback[key]`
//                    rejection test of Train.sample_negative (FM.py:291-293)
//                    and the target test of evaluate_TopK (FM.py:343-355:
//                    `item in positive_feedback[key]`)
//   hhfm_topk_walk   replaces the per-row walk over the 20 predictions of
//                    Train.evaluate_TopK (FM.py:344-357)
//
// positive_feedback (a dict key -> set(item), key = every column but the
// item, NewLoadData.py:49-56) is laid out as two sorted device arrays built
// once on the host: the distinct keys, lexicographically sorted
// [nkeys][key_cols] int32, and the (key rank << 32 | item) codes of every
// (key, item) pair, sorted int64.  A membership test is a binary search for
// the key followed by one for the code: no hashing, no collisions, exact.
// The draws themselves stay on the host (numpy's RNG stream, so the samples
// are the reference's); the walk returns ranks, the host turns them into
// the reference's float64 HR / NDCG / PRE values.
#include "hhfm_common.h"

#include <hipcub/hipcub.hpp>

namespace hhfm {

// row key (every column but item_col, in column order) vs keys[m]
HHFM_DEV int key_cmp(const int32_t* row, int ncols, int item_col, const int32_t* key) {
  int c2 = 0;
  for (int c = 0; c < ncols; ++c) {
    if (c == item_col) continue;
    const int32_t a = row[c], b = key[c2++];
    if (a != b) return a < b ? -1 : 1;
  }
  return 0;
}

// one thread per (row, candidate); cand == nullptr: the row's own item
__global__ __launch_bounds__(256) void pf_contains_kernel(
    const int32_t* __restrict__ keys, int64_t nkeys, int key_cols,
    const int64_t* __restrict__ codes, int64_t ncodes, const int32_t* __restrict__ rows,
    int64_t B, int ncols, int item_col, const int32_t* __restrict__ cand, int num,
    uint8_t* __restrict__ out) {
  const int64_t n = B * num;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n;
       x += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = x / num;
    const int32_t* row = rows + b * ncols;
    const int32_t item = cand ? cand[x] : row[item_col];
    // lower_bound over the sorted keys
    int64_t lo = 0, hi = nkeys;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (key_cmp(row, ncols, item_col, keys + mid * key_cols) > 0) lo = mid + 1;
      else hi = mid;
    }
    uint8_t hit = 0;
    if (lo < nkeys && key_cmp(row, ncols, item_col, keys + lo * key_cols) == 0) {
      const int64_t code = (lo << 32) | (int64_t)(uint32_t)item;
      int64_t a = 0, e = ncodes;
      while (a < e) {
        const int64_t mid = (a + e) >> 1;
        if (codes[mid] < code) a = mid + 1;
        else e = mid;
      }
      hit = a < ncodes && codes[a] == code;
    }
    out[x] = hit;
  }
}

// evaluate_TopK's walk (FM.py:344-357), one thread per row:
//   outcome = n >= 0  the target found at walk position n (< TopK)
//           = -1      walk reached n > TopK-1: the reference appends 0, 0, 0
//           = -2      predictions exhausted: the reference appends nothing
// A target that is itself a train positive of its key makes every non-hit a
// `continue` (n is not advanced), the reference's quirk.
__global__ __launch_bounds__(256) void topk_walk_kernel(
    const int32_t* __restrict__ pred, int64_t B, int P, const int32_t* __restrict__ target,
    const uint8_t* __restrict__ positive, int TopK, int32_t* __restrict__ outcome) {
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B;
       b += (int64_t)gridDim.x * blockDim.x) {
    const int32_t item = target[b];
    const bool pos = positive[b] != 0;
    int n = 0, res = -2;
    for (int p = 0; p < P; ++p) {
      if (n > TopK - 1) { res = -1; break; }
      if (pred[b * P + p] == item) { res = n; break; }
      if (!pos) ++n;
    }
    outcome[b] = res;
  }
}

// Exclusion lists (include/hhfm.h "Exclusion lists"): per row, the run of
// `codes` that carries its key's rank — the key's items, ascending — is the
// row's list.  pf_run finds the run codes[a .. e) of a row (empty for an
// unknown key) and, under keep_own, the place `own` of the row's own item in
// it (-1: not there), which the list leaves out.
struct PfRun {
  int64_t a, e, own;
};

HHFM_DEV PfRun pf_run(const int32_t* __restrict__ keys, int64_t nkeys, int key_cols,
                      const int64_t* __restrict__ codes, int64_t ncodes, const int32_t* row,
                      int ncols, int item_col, int keep_own) {
  PfRun r{0, 0, -1};
  int64_t lo = 0, hi = nkeys;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (key_cmp(row, ncols, item_col, keys + mid * key_cols) > 0) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= nkeys || key_cmp(row, ncols, item_col, keys + lo * key_cols) != 0) return r;
  auto lower = [&](int64_t code) {
    int64_t x = 0, y = ncodes;
    while (x < y) {
      const int64_t mid = (x + y) >> 1;
      if (codes[mid] < code) x = mid + 1;
      else y = mid;
    }
    return x;
  };
  r.a = lower(lo << 32);
  r.e = lower((lo + 1) << 32);
  if (keep_own) {
    const int64_t code = (lo << 32) | (int64_t)(uint32_t)row[item_col];
    const int64_t x = lower(code);
    if (x < r.e && codes[x] == code) r.own = x;
  }
  return r;
}

// sizing: one thread per row, counts[b] = length of row b's list, counts[B] = 0
__global__ __launch_bounds__(256) void pf_excl_count_kernel(
    const int32_t* __restrict__ keys, int64_t nkeys, int key_cols,
    const int64_t* __restrict__ codes, int64_t ncodes, const int32_t* __restrict__ rows,
    int64_t B, int ncols, int item_col, int keep_own, int64_t* __restrict__ counts) {
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b <= B;
       b += (int64_t)gridDim.x * blockDim.x) {
    if (b == B) {
      counts[B] = 0;
      break;
    }
    const PfRun r = pf_run(keys, nkeys, key_cols, codes, ncodes, rows + b * ncols, ncols,
                           item_col, keep_own);
    counts[b] = (r.e - r.a) - (r.own >= 0 ? 1 : 0);
  }
}

// fill: one wave per row (every lane finds the same run, the copy is spread
// over the lanes), out[ptr[b] ..] = the list (ptr = the scanned counts)
__global__ __launch_bounds__(256) void pf_excl_fill_kernel(
    const int32_t* __restrict__ keys, int64_t nkeys, int key_cols,
    const int64_t* __restrict__ codes, int64_t ncodes, const int32_t* __restrict__ rows,
    int64_t B, int ncols, int item_col, int keep_own, const int64_t* __restrict__ ptr,
    int32_t* __restrict__ out) {
  const int l = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t b = wave; b < B; b += nwave) {
    const PfRun r = pf_run(keys, nkeys, key_cols, codes, ncodes, rows + b * ncols, ncols,
                           item_col, keep_own);
    int32_t* dst = out + ptr[b];
    const int64_t room = ptr[b + 1] - ptr[b];   // (a sizing call with other arguments: stay inside)
    for (int64_t x = r.a + l; x < r.e; x += kWave) {
      if (x == r.own) continue;
      const int64_t at = (x - r.a) - (r.own >= 0 && x > r.own ? 1 : 0);
      if (at < room) dst[at] = (int32_t)(uint32_t)codes[x];
    }
  }
}

// exclusive scan of n int64 values by one workgroup, chunk by chunk
__global__ __launch_bounds__(1024) void scan_i64_kernel(const int64_t* __restrict__ in, int64_t n,
                                                        int64_t* __restrict__ out) {
  using Scan = hipcub::BlockScan<int64_t, 1024>;
  __shared__ typename Scan::TempStorage tmp;
  int64_t carry = 0;
  for (int64_t base = 0; base < n; base += 1024) {
    const int64_t x = base + threadIdx.x;
    const int64_t v = x < n ? in[x] : 0;
    int64_t ex, total;
    Scan(tmp).ExclusiveSum(v, ex, total);
    if (x < n) out[x] = carry + ex;
    carry += total;
    __syncthreads();   // tmp is reused by the next chunk
  }
}

static unsigned grid_1d(int64_t n) {
  int64_t g = (n + 255) / 256;
  if (g > 16384) g = 16384;
  return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace hhfm

using namespace hhfm;

extern "C" int hhfm_pf_contains(const int32_t* keys, int64_t nkeys, int32_t key_cols,
                                const int64_t* codes, int64_t ncodes, const int32_t* rows,
                                int64_t B, int32_t ncols, int32_t item_col,
                                const int32_t* cand, int32_t num, uint8_t* out,
                                void* stream) {
  if (B < 0 || nkeys < 0 || ncodes < 0 || ncols < 2 || ncols > 64) return HHFM_EINVAL;
  if (item_col < 0 || item_col >= ncols || key_cols != ncols - 1) return HHFM_EINVAL;
  if (cand ? num < 1 : num != 1) return HHFM_EINVAL;
  if (B == 0) return HHFM_OK;
  if (!rows || !out || (nkeys && !keys) || (ncodes && !codes)) return HHFM_EINVAL;
  hipLaunchKernelGGL(pf_contains_kernel, dim3(grid_1d(B * num)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), keys, nkeys, key_cols, codes,
                     ncodes, rows, B, ncols, item_col, cand, num, out);
  return (int)hipGetLastError();
}

// counts int64 [B + 1] (scanned into excl_ptr by the sizing call)
extern "C" int hhfm_pf_exclusion_lists_workspace(int64_t B, size_t* ws_bytes) {
  if (!ws_bytes || B < 0) return HHFM_EINVAL;
  *ws_bytes = (((size_t)B + 1) * sizeof(int64_t) + 255) & ~size_t(255);
  return HHFM_OK;
}

extern "C" int hhfm_pf_exclusion_lists(const int32_t* keys, int64_t nkeys, int32_t key_cols,
                                       const int64_t* codes, int64_t ncodes,
                                       const int32_t* rows, int64_t B, int32_t ncols,
                                       int32_t item_col, int32_t keep_own, int64_t* excl_ptr,
                                       int32_t* excl_rows, int64_t capacity, void* workspace,
                                       size_t ws_bytes, void* stream) {
  if (B < 0 || nkeys < 0 || ncodes < 0 || ncols < 2 || ncols > 64) return HHFM_EINVAL;
  if (item_col < 0 || item_col >= ncols || key_cols != ncols - 1) return HHFM_EINVAL;
  if (!excl_ptr || (B && !rows) || (nkeys && !keys) || (ncodes && !codes)) return HHFM_EINVAL;
  if (excl_rows && capacity < 0) return HHFM_EINVAL;
  size_t need = 0;
  hhfm_pf_exclusion_lists_workspace(B, &need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!excl_rows) {   // sizing call: per-row counts, then their exclusive scan
    if (!workspace || ws_bytes < need) return HHFM_EWORKSPACE;
    int64_t* counts = reinterpret_cast<int64_t*>(workspace);
    hipLaunchKernelGGL(pf_excl_count_kernel, dim3(grid_1d(B + 1)), dim3(256), 0, st, keys, nkeys,
                       key_cols, codes, ncodes, rows, B, ncols, item_col, keep_own, counts);
    hipLaunchKernelGGL(scan_i64_kernel, dim3(1), dim3(1024), 0, st, counts, B + 1, excl_ptr);
    return (int)hipGetLastError();
  }
  // fill call: excl_ptr is the sizing call's; its total against the capacity
  int64_t total = 0;
  hipError_t e = hipMemcpyAsync(&total, excl_ptr + B, sizeof(total), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  if (total < 0) return HHFM_EINVAL;
  if (capacity < total) return HHFM_EWORKSPACE;
  if (B == 0 || total == 0) return HHFM_OK;
  hipLaunchKernelGGL(pf_excl_fill_kernel, dim3(grid_1d(B * kWave)), dim3(256), 0, st, keys, nkeys,
                     key_cols, codes, ncodes, rows, B, ncols, item_col, keep_own, excl_ptr,
                     excl_rows);
  return (int)hipGetLastError();
}

extern "C" int hhfm_topk_walk(const int32_t* pred, int64_t B, int32_t P, const int32_t* target,
                              const uint8_t* positive, int32_t TopK, int32_t* outcome,
                              void* stream) {
  if (B < 0 || P < 1 || TopK < 1) return HHFM_EINVAL;
  if (B == 0) return HHFM_OK;
  if (!pred || !target || !positive || !outcome) return HHFM_EINVAL;
  hipLaunchKernelGGL(topk_walk_kernel, dim3(grid_1d(B)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), pred, B, P, target, positive, TopK,
                     outcome);
  return (int)hipGetLastError();
}
