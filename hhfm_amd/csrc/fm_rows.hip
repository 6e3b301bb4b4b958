// K1 — per-row FM / HHFM scoring on gfx950 (HBM-bound sparse gather + reduce).
//
//   hhfm_fm_score_rows     replaces the FM.out graph        (Newcode/FM.py:99-120)
//   hhfm_hybrid_score_rows replaces OUR.PositiveFeadback    (Newcode/OurModel7.py:105-171)
//
// Layout / mapping:
//   * one embedding row = RV 16-byte chunks (RV = k*elem_size/16); a row is
//     owned by an aligned group of LPR = RV lanes, each lane issuing ONE
//     16-B load per field (global_load_dwordx4), so a wave-instruction moves
//     64 lanes x 16 B = 1 KiB of whole rows;
//   * every lane keeps U rows x F fields of loads in flight (~20 x 16 B) and
//     the index rows of the NEXT iteration are fetched before this
//     iteration's gathers are consumed (hides the idx->gather dependency);
//   * the ½((Σv)²−Σv²) interaction is reduced first inside the lane (4 or 8
//     elements), then across the LPR lanes by group_sum_dpp (hhfm_common.h):
//     the xor-8/4/2/1 steps are v_add_f32_dpp (row_ror / quad_perm) and only
//     the xor-32/16 steps of LPR 64 / 32 go through ds_bpermute_b32 (LDS
//     hardware, no LDS allocation).  No atomics, one fp32 store per row.
#include <type_traits>

#include "hhfm_common.h"
#include "hhfm_feature.h"

namespace hhfm {

// blocks per CU the grid is capped at (grid-stride beyond): at configs[1]
// 16 / 32 / 64 / 256 / 2048 ran 3.98 / 3.95 / 3.94 / 4.11 / 4.51 ms
// (profiles/r04_k1_grid_cap_ab.txt)
#ifndef HHFM_K1_CAP
#define HHFM_K1_CAP 64
#endif
// diagnostic (timing only, wrong results; default 0): where the `w` gathers
// are served from — 1: every w index folded into a 1 MB window (L2-resident),
// 2: w index x 32 (every gather its own 128-B line of a 2 GB array: no reuse
// in L2 or the Infinity Cache); scripts/diag/k1_wmap.sh
#ifndef HHFM_K1_WMAP
#define HHFM_K1_WMAP 0
#endif
// diagnostic (timing only, wrong results; default 0): 1 — fields 2.. (the
// context columns at configs[1]) keep their ids and `w` gathers but their
// embedding rows are not loaded (zeros); scripts/diag/k1_ctx_ko.sh
#ifndef HHFM_K1_CTXKO
#define HHFM_K1_CTXKO 0
#endif
#if (HHFM_K1_WMAP || HHFM_K1_CTXKO) && !defined(HHFM_DIAG_BUILD)
#error "K1 knock-out macros give wrong results: diagnostic builds only (-DHHFM_DIAG_BUILD)"
#endif
#ifndef HHFM_K1_U5
#define HHFM_K1_U5 5   // rows per lane in flight at F = 5
#endif
// F = 5 (configs[1]): 5 rows in flight per lane 3.98 ms against 4 4.11, 3
// 4.07, 6 5.05 (profiles/r04_k1_rows_in_flight_ab.txt); the HHFM rows and
// the bf16 tables gain or hold too (profiles/r04_k1_u5_microbench.txt)
template <int F>
struct RowsPerLane {
  static constexpr int value =
      F <= 3 ? 6 : (F == 4 ? 4 : (F == 5 ? HHFM_K1_U5 : (F <= 8 ? 3 : 2)));
};

// Raw (unclamped) index rows: nothing may consume them until the gathers
// issued before them are consumed, or the in-order vmcnt would serialise.
template <int F, int U, bool NT = false>
HHFM_DEV void load_ids(int32_t (&id)[U][F], const int32_t* __restrict__ idx,
                       int64_t base, int64_t B, int g, int RPW, int ncols) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    int64_t row = base + (int64_t)u * RPW + g;
    const int32_t* p = idx + (row < B ? row : 0) * (int64_t)ncols;
#pragma unroll
    for (int f = 0; f < F; ++f) id[u][f] = load_i32<NT>(p + f);
  }
}

// ---------------------------------------------------------------------------
// FM row kernel: out = Σ_k ½[(Σ_f e)² − Σ_f e²] + Σ_f w + w0
// ---------------------------------------------------------------------------
// NTM: 0 every load default, 1 every load non-temporal (HHFM_FLAG_STREAM_TABLE),
// 2 only the user and item rows (fields 0, 1) non-temporal — planned for
// tables far beyond the caches, where those rows are read once and the
// default policy lets them evict the re-read `w` lines and context rows from
// the Infinity Cache: 4.21 -> 4.11 ms at configs[1] (ids and output
// non-temporal as well: 4.53 ms; profiles/r04_k1_nt_ab.txt)
// SCALED (hhfm_fm_score_rows_scaled): column c enters the row sum as
// scale[c]·½(s² − q); a lane loads the scale of its C::kElems columns once,
// before the row loop.  Everything else is the same code.
template <int F, int LPR, bool BF16, bool HAS_W, int NTM, bool SCALED = false>
__global__ __launch_bounds__(256) void fm_rows_fast(
    const int32_t* __restrict__ idx, int64_t B, const char* __restrict__ E,
    int64_t M, const float* __restrict__ w, float w0, float* __restrict__ out,
    int32_t* __restrict__ status, const float* __restrict__ scale) {
  constexpr int U = RowsPerLane<F>::value;
  constexpr int RPW = kWave / LPR;  // rows per wave per unroll slot
  constexpr int RPI = RPW * U;      // rows per wave-iteration
  constexpr int64_t ROW_BYTES = (int64_t)LPR * 16;
  constexpr bool NT = NTM == 1;
  using C = Chunk<BF16>;
  const uint32_t M32 = id_limit32(M);

  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (LPR - 1);
  const int g = lane / LPR;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t stride = nwave * RPI;

  [[maybe_unused]] float sc[C::kElems];
  if constexpr (SCALED) {
#pragma unroll
    for (int e = 0; e < C::kElems; ++e) sc[e] = scale[sub * C::kElems + e];
  }

  int64_t base = wave * RPI;
  int32_t raw[U][F];
  bool bad = false;
  if (base < B) load_ids<F, U, NT>(raw, idx, base, B, g, RPW, F);

  for (; base < B; base += stride) {
    C c[U][F];
    int32_t id[U][F];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int f = 0; f < F; ++f) {
        id[u][f] = clamp_id32(raw[u][f], M32);
        bad |= id[u][f] != raw[u][f];
        if (HHFM_K1_CTXKO && f >= 2) {
#pragma unroll
          for (int e = 0; e < C::kElems; ++e) c[u][f].v[e] = 0.f;
        } else if (NTM == 2 && f < 2)
          c[u][f].template load<true>(E + (int64_t)id[u][f] * ROW_BYTES + sub * 16);
        else
          c[u][f].template load<NT>(E + (int64_t)id[u][f] * ROW_BYTES + sub * 16);
      }

    // Σ_f w[x_f]: lane `sub` gathers fields f ≡ sub (mod LPR); loads are
    // unconditional (clamped ids) so the vmcnt counting stays exact
    float wv[U];
    if constexpr (HAS_W) {
      constexpr int WPL = (F + LPR - 1) / LPR;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        wv[u] = 0.f;
#pragma unroll
        for (int r = 0; r < WPL; ++r) {
          const int fsel = r * LPR + sub;
          int32_t my = id[u][0];
#pragma unroll
          for (int f = 1; f < F; ++f) my = (fsel == f) ? id[u][f] : my;
          const float wl = HHFM_K1_WMAP == 1   ? w[my & 0x3ffff]
                           : HHFM_K1_WMAP == 2 ? w[(int64_t)my * 32]
                                               : w[my];
          wv[u] += (fsel < F) ? wl : 0.f;
        }
      }
    }

    // prefetch next iteration's index rows before consuming the gathers
    // (unconditional: rows past B read row 0, which keeps vmcnt counting exact)
    load_ids<F, U, NT>(raw, idx, base + stride, B, g, RPW, F);

#pragma unroll
    for (int u = 0; u < U; ++u) {
      float t = 0.f;
#pragma unroll
      for (int e = 0; e < C::kElems; ++e) {
        float s = c[u][0].v[e];
        float q = c[u][0].v[e] * c[u][0].v[e];
#pragma unroll
        for (int f = 1; f < F; ++f) {
          s += c[u][f].v[e];
          q += c[u][f].v[e] * c[u][f].v[e];
        }
        if constexpr (SCALED) t += sc[e] * (0.5f * (s * s - q));
        else t += 0.5f * (s * s - q);
      }
      t = group_sum_dpp<LPR>(t);
      float fb = 0.f;
      if constexpr (HAS_W) fb = group_sum_dpp<LPR>(wv[u]);
      const int64_t row = base + (int64_t)u * RPW + g;
      if (sub == 0 && row < B) {
        if constexpr (NT) __builtin_nontemporal_store((t + fb) + w0, out + row);
        else out[row] = (t + fb) + w0;
      }
    }
  }
  report_bad_id(status, bad);
}

// ---------------------------------------------------------------------------
// FM row kernel for 3 <= F <= 8 with the table's tail served from LDS
// (DESIGN.md §K1 "hot tail"; the kernel the issue calls fm_rows_hot — the name
// keeps the fm_rows_fast prefix the benchmark's PMC passes select rows by).
//
// The loaders number tokens column-major (users, items, then each context
// column: NewLoadData.py), so the small-vocabulary columns' rows are the last
// rows of the table.  Every workgroup stages the last T = 16 KiB / row_bytes
// rows (and their `w`) in LDS once; a wave-iteration whose field-2.. ids all
// lie in that window keeps only the user and item rows in registers across
// the HBM wait and reads the others from LDS when it consumes them: 2 x U row
// loads per lane in flight in the register budget of 3 waves per SIMD, where
// fm_rows_fast<5> holds F x U = 25 at 2 waves.
//
// The LDS-tail loop runs full wave-iterations only (`base + RPI <= B`, scalar
// work on the wave-uniform `base`) and asks one thing of an iteration's raw
// ids before any row load or LDS read: every user / item id is in [0, M) and
// every field-2.. id lies in the window — two unsigned maxima and two
// compares (HHFM_K1_LEAN_FRONT).  It clamps nothing, raises no `bad` and masks
// no row by `row < B`: on a hit every id is its own clamp and every row exists.
//
// Any input is served: the first wave-iteration that fails the verdict — an
// id outside the window, a bad id anywhere in it — or is a wave's partial last
// one sends its wave to the general loop below — every field from global
// memory, UG row slots, ids clamped, `bad` raised, rows masked — for that
// iteration and the rest of its rows.  Results and the status word do not
// depend on which loop ran; only the speed of such iterations does.  Same
// per-element order, same lane-to-field assignment of `w`, same (t + fb) + w0
// as fm_rows_fast: the same bits on either path.
// ---------------------------------------------------------------------------
#ifndef HHFM_K1_HOT_U
#define HHFM_K1_HOT_U 6   // row slots per lane of the LDS-tail loop
#endif
#ifndef HHFM_K1_HOT_CAP
#define HHFM_K1_HOT_CAP HHFM_K1_CAP   // blocks per CU (each stages 16 KiB)
#endif
#ifndef HHFM_K1_HOT_AUTO
#define HHFM_K1_HOT_AUTO 1   // 0: only HHFM_FLAG_HOT_TAIL selects the kernel
#endif
// Where the LDS-tail loop takes the user's and the item's `w` from:
//   0  one vector load per slot (lanes sub = 0, 1 own fields 0, 1);
//   1  fp32 tables, F <= 5, LPR >= 16: scalar loads.  A row's ids are the
//      same in all LPR lanes of its group, so each (slot, field, group) is one wave-uniform address,
//      fetched through the scalar data cache (counted on lgkmcnt, not on the
//      in-order vmcnt of the row loads, and not a request to TA / vector L1)
//      and put into lanes sub = 0, 1 by v_writelane.  3.483 -> 3.108 ms at
//      configs[1] (profiles/k1_w_scalar_ab.txt).
#ifndef HHFM_K1_W_SCALAR
#define HHFM_K1_W_SCALAR 1
#endif
// The LDS-tail loop's front end (profiles/k1_lean_loop_ab.txt):
//   0  every id clamped and compared per lane, `row < B` per slot;
//   1  validity only: the loop takes full wave-iterations (a wave-uniform,
//      scalar test) and forms one verdict per iteration from the raw ids; the
//      general loop does the clamping, the status word and the partial
//      iteration, so nothing of that is left in this loop.
#ifndef HHFM_K1_LEAN_FRONT
#define HHFM_K1_LEAN_FRONT 1
#endif
// fm_chunk_term on two-element vectors (v_pk_mul / v_pk_add / v_pk_fma_f32):
// the same operations per element in the same order, the same bits
#ifndef HHFM_K1_PK_MATH
#define HHFM_K1_PK_MATH 1
#endif
constexpr int kHotWindowBytes = 16384;
// scalar `w` loads of a wave-iteration at most (more: the vector load), and
// how many results are held in SGPRs at a time
constexpr int kHotWScalarMax = 48;
#ifndef HHFM_K1_W_SCALAR_BATCH
#define HHFM_K1_W_SCALAR_BATCH 24
#endif
constexpr int kHotWScalarBatch = HHFM_K1_W_SCALAR_BATCH;

// Row slots of the two loops, sized so that the kernel stays within the 168
// VGPRs of 3 waves per SIMD (profiles/k1_hot_tail_resources.txt; the bf16
// F = 8 and two bf16 F = 6 variants do not, and run at fm_rows_fast's 2 waves)
template <int F>
struct HotRows {
  static constexpr int U = F <= 6 ? HHFM_K1_HOT_U : 4;  // LDS-tail loop (2 rows per slot)
  static constexpr int UG = F <= 5 ? 3 : 2;             // general loop (F rows per slot)
};

// rows of wave-iteration `base`, slots u0 .. u0+UG-1 (slots >= U and rows
// >= B read row 0: unconditional loads keep the vmcnt counting exact)
template <int F, int U, int UG>
HHFM_DEV void load_ids_slots(int32_t (&id)[UG][F], const int32_t* __restrict__ idx,
                             int64_t base, int u0, int64_t B, int g, int RPW) {
#pragma unroll
  for (int u = 0; u < UG; ++u) {
    int64_t row = base + (int64_t)(u0 + u) * RPW + g;
    const int32_t* p = idx + ((u0 + u < U && row < B) ? row : 0) * (int64_t)F;
#pragma unroll
    for (int f = 0; f < F; ++f) id[u][f] = p[f];
  }
}

// Σ_e ½((Σ_f c_f)² − Σ_f c_f²) of one lane's chunk, fields in index order.
// Per element, what the compiler contracts the plain expression to (here and
// in fm_rows_fast): q = fma(v0, v0, v1·v1) — of the first two squares it is
// the second that is rounded on its own — then q = fma(v_f, v_f, q), s += v_f,
// x = fma(s, s, −q), t += ½·x (exact, so fused or not is the same).  PK: the
// same steps written out on the elements (e, e + 1) together, for the packed
// fp32 instructions; t stays one chain over e, so the bits are the same.
typedef float f32x2_t __attribute__((ext_vector_type(2)));
template <int F, typename C, bool PK = HHFM_K1_PK_MATH == 1>
HHFM_DEV float fm_chunk_term(const C (&c)[F]) {
  static_assert(F >= 2, "the first two fields open the sums");
  float t = 0.f;
  if constexpr (PK) {
#pragma unroll
    for (int e = 0; e < C::kElems; e += 2) {
      const f32x2_t v0 = {c[0].v[e], c[0].v[e + 1]};
      const f32x2_t v1 = {c[1].v[e], c[1].v[e + 1]};
      f32x2_t s = v0 + v1;
      f32x2_t q = __builtin_elementwise_fma(v0, v0, v1 * v1);
#pragma unroll
      for (int f = 2; f < F; ++f) {
        const f32x2_t v = {c[f].v[e], c[f].v[e + 1]};
        s += v;
        q = __builtin_elementwise_fma(v, v, q);
      }
      const f32x2_t x = __builtin_elementwise_fma(s, s, -q);
      t = __builtin_fmaf(0.5f, x[0], t);
      t = __builtin_fmaf(0.5f, x[1], t);
    }
  } else {
#pragma unroll
    for (int e = 0; e < C::kElems; ++e) {
      float s = c[0].v[e];
      float q = c[0].v[e] * c[0].v[e];
#pragma unroll
      for (int f = 1; f < F; ++f) {
        s += c[f].v[e];
        q += c[f].v[e] * c[f].v[e];
      }
      t += 0.5f * (s * s - q);
    }
  }
  return t;
}

template <int F, int LPR, bool BF16, bool HAS_W, bool NT01>
__global__ __launch_bounds__(256) void fm_rows_fast_hot(
    const int32_t* __restrict__ idx, int64_t B, const char* __restrict__ E,
    int64_t M, const float* __restrict__ w, float w0, float* __restrict__ out,
    int32_t* __restrict__ status) {
  static_assert(F >= 3 && F <= 10 && LPR >= 4, "fields 2.. pack into 8-bit local indices");
  constexpr int U = HotRows<F>::U;
  constexpr int UG = HotRows<F>::UG;
  constexpr int RPW = kWave / LPR;
  constexpr int RPI = RPW * U;
  constexpr int64_t ROW_BYTES = (int64_t)LPR * 16;
  constexpr int T = kHotWindowBytes / (int)ROW_BYTES;  // window rows (<= 256)
  constexpr int NC = F - 2;                            // fields read from LDS
  constexpr int PKW = (NC + 3) / 4;                    // 4 local indices per register
  constexpr int WPL = (F + LPR - 1) / LPR;
  // user / item `w` by scalar loads (HHFM_K1_W_SCALAR): fp32 tables, F <= 5,
  // LPR >= 16 (2 * U * RPW <= 48).  F >= 6 spills more SGPRs inside the loop
  // with them (F = 8 bf16 LPR 16: 1.21 -> 1.45 ms) and bf16 F = 5 LPR 16 ran
  // 1.5 % slower (profiles/k1_w_scalar_ab.txt): those keep the vector load.
  constexpr bool WS = HAS_W && HHFM_K1_W_SCALAR == 1 && !BF16 && F <= 5 &&
                      2 * U * RPW <= kHotWScalarMax;
  // Where the lean front end or the packed math would cost the kernel a wave
  // per SIMD by registers, or take it past the 168 VGPRs of 3 waves, it keeps
  // the earlier form (profiles/k1_lean_loop_resources.txt): the front end at
  // F = 3 with LPR <= 8 and at fp32 F = 7 without `w`; the chunk math without
  // `w` at bf16 F = 3, 8 and at fp32 F = 7.  bf16 tables at LPR <= 8 keep both
  // earlier forms: F = 5 k = 64 bf16 ran 1.1 % slower with the two
  // (profiles/k1_lean_loop_ab.txt).
  constexpr bool NARROW_BF16 = BF16 && LPR <= 8;
  constexpr bool LEAN = HHFM_K1_LEAN_FRONT == 1 && !NARROW_BF16 && !(F == 3 && LPR <= 8) &&
                        !(F == 7 && !BF16 && !HAS_W);
  constexpr bool PK = HHFM_K1_PK_MATH == 1 && !NARROW_BF16 &&
                      !(!HAS_W && (BF16 ? (F == 3 || F == 8) : F == 7));
  static_assert(T <= 256, "local index is 8 bits");
  using C = Chunk<BF16>;
  const uint32_t M32 = id_limit32(M);

  __shared__ u32x4_t hot[T * LPR];
  __shared__ float hotw[HAS_W ? T : 1];

  // window [ws, M): the table's last T rows, clipped to the table
  const int64_t ws = M > T ? M - T : 0;
  const int nwin = (int)(M - ws);
  {
    const char* src = E + ws * ROW_BYTES;
    for (int i = threadIdx.x; i < nwin * LPR; i += 256) hot[i] = load16<false>(src + (int64_t)i * 16);
    if constexpr (HAS_W)
      for (int i = threadIdx.x; i < nwin; i += 256) hotw[i] = w[ws + i];
  }
  __syncthreads();
  // ids are int32: a window that starts past them is never hit
  const bool reach = ws <= 0x7fffffff;
  const int32_t ws32 = reach ? (int32_t)ws : 0;
  const uint32_t nhit = reach ? (uint32_t)nwin : 0u;
  [[maybe_unused]] const uint32_t nm1 = (uint32_t)nwin - 1u;

  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (LPR - 1);
  const int g = lane / LPR;
  // LEAN: the wave's number as a scalar, so that `base` and the loop's test
  // `base + RPI <= B` are scalar work
  const int64_t wave =
      LEAN ? (int64_t)blockIdx.x * (blockDim.x / kWave) +
                 __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave))
           : ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t stride = nwave * RPI;

  int64_t base = wave * RPI;
  bool bad = false;
  {
    int32_t raw[U][F];
    if (base < B) load_ids<F, U, false>(raw, idx, base, B, g, RPW, F);

    // LEAN: full wave-iterations only; the partial last one of a wave is the
    // general loop's
    for (; LEAN ? base + RPI <= B : base < B; base += stride) {
      int32_t id01[U][2];
      uint32_t pk[U][PKW];
      bool miss = false;
      if constexpr (LEAN) {
        // one verdict from the raw ids: every user / item id is in [0, M)
        // (unsigned maximum < M32) and every field-2.. id is in the window
        // (maximum of the local indices < nhit).  Nothing is clamped: on a
        // miss nothing below runs, and on a hit every id is its own clamp.
        uint32_t hi = 0u, dm = 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int j = 0; j < PKW; ++j) pk[u][j] = 0u;
#pragma unroll
          for (int f = 0; f < F; ++f) {
            if (f < 2) {
              id01[u][f] = raw[u][f];
              hi = max(hi, (uint32_t)raw[u][f]);
            } else {
              const uint32_t d = (uint32_t)(raw[u][f] - ws32);
              dm = max(dm, d);
              pk[u][(f - 2) >> 2] |= d << (8 * ((f - 2) & 3));
            }
          }
        }
        miss = hi >= M32 || dm >= nhit;
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int j = 0; j < PKW; ++j) pk[u][j] = 0u;
          bool m = false;
#pragma unroll
          for (int f = 0; f < F; ++f) {
            const int32_t id = clamp_id32(raw[u][f], M32);
            bad |= id != raw[u][f];
            if (f < 2) {
              id01[u][f] = id;
            } else {
              const uint32_t d = (uint32_t)(id - ws32);
              m |= d >= nhit;
              pk[u][(f - 2) >> 2] |= (d < nm1 ? d : nm1) << (8 * ((f - 2) & 3));
            }
          }
          miss |= m && (base + (int64_t)u * RPW + g < B);
        }
      }
      // wave-uniform: some row of this wave-iteration needs a row outside the
      // window (LEAN: or holds a bad id) -> the general loop takes over from
      // this iteration on
      if (__ballot(miss) != 0) break;

      C c01[U][2];
      float wg[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          // LEAN: the id is known to be in [0, M): zero-extended
          const int64_t r = LEAN ? (int64_t)(uint32_t)id01[u][f] : (int64_t)id01[u][f];
          c01[u][f].template load<NT01>(E + r * ROW_BYTES + sub * 16);
        }
      }
      // `w` of the user and item from global memory into lanes sub = 0, 1
      // (fields 0, 1) of wg: by scalar loads (HHFM_K1_W_SCALAR), else by one
      // vector load per slot (the other lanes' load is dropped, as in
      // fm_rows_fast).  Rows >= B and clamped ids read w[0] either way.
      if constexpr (WS) {
        // The loop is wave-uniform (the __ballot above): EXEC is full, as
        // v_readlane needs.  The row loads above are already in flight; a
        // batch of scalar loads is issued, waited for on lgkmcnt and moved to
        // lanes sub = 0 (user), 1 (item) of its slots' wg before the next,
        // so no more than kHotWScalarBatch results are held in SGPRs at once
        // and none across the consume phase (all 48 at once spill SGPRs in the
        // loop).  The scheduling barriers keep one load's address arithmetic
        // (64-bit: w + 4 * id for any features_M) from being hoisted over
        // another's, which would hold an address pair per load.
        constexpr int SB = kHotWScalarBatch / (2 * RPW);   // slots per batch
#pragma unroll
        for (int u0 = 0; u0 < U; u0 += SB) {
          float wsc[SB][2][RPW];   // [slot][field][group], SGPRs
#pragma unroll
          for (int u = u0; u < u0 + SB && u < U; ++u)
#pragma unroll
            for (int gg = 0; gg < RPW; ++gg)
#pragma unroll
              for (int f = 0; f < 2; ++f) {
                __builtin_amdgcn_sched_barrier(0);
                wsc[u - u0][f][gg] = w[(int64_t)__builtin_amdgcn_readlane(id01[u][f], gg * LPR)];
              }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = u0; u < u0 + SB && u < U; ++u)
            wg[u] = __int_as_float(write_group_lanes01<LPR, RPW>(0, wsc[u - u0]));
          __builtin_amdgcn_sched_barrier(0);
        }
      } else if constexpr (HAS_W) {
#pragma unroll
        for (int u = 0; u < U; ++u) wg[u] = w[sub == 1 ? id01[u][1] : id01[u][0]];
      }

      // the next iteration's ids (rows past B read row 0; where the next is
      // no full iteration this loop does not use them)
      load_ids<F, U, false>(raw, idx, base + stride, B, g, RPW, F);

#pragma unroll
      for (int u = 0; u < U; ++u) {
        C c[F];
        c[0] = c01[u][0];
        c[1] = c01[u][1];
#pragma unroll
        for (int f = 2; f < F; ++f) {
          const uint32_t li = (pk[u][(f - 2) >> 2] >> (8 * ((f - 2) & 3))) & 0xffu;
          c[f].set(hot[li * LPR + sub]);
        }
        // the row sum is reduced before the `w` terms are formed: stepping
        // the two sums together fills the DPP hazard slots but ran 0.45 %
        // slower and takes F = 6 bf16 past 168 VGPRs (profiles/k1_consume_ab.txt)
        float t = group_sum_dpp<LPR>(fm_chunk_term<F, C, PK>(c));
        float fb = 0.f;
        if constexpr (HAS_W) {
          float wv = 0.f;
#pragma unroll
          for (int r = 0; r < WPL; ++r) {
            const int fsel = r * LPR + sub;
            int j = fsel - 2;
            j = j < 0 ? 0 : (j > NC - 1 ? NC - 1 : j);
            uint32_t word = pk[u][0];
#pragma unroll
            for (int q = 1; q < PKW; ++q) word = (j >> 2) == q ? pk[u][q] : word;
            const float wl = hotw[(word >> (8 * (j & 3))) & 0xffu];
            wv += (fsel < 2) ? wg[u] : ((fsel < F) ? wl : 0.f);
          }
          fb = group_sum_dpp<LPR>(wv);
        }
        const int64_t row = base + (int64_t)u * RPW + g;
        if (sub == 0 && (LEAN || row < B)) out[row] = (t + fb) + w0;
      }
    }
  }

  // general loop: the body of fm_rows_fast at UG row slots, walking the same
  // wave-iterations UG slots at a time
  if (base < B) {
    int u0 = 0;
    int32_t raw[UG][F];
    load_ids_slots<F, U, UG>(raw, idx, base, u0, B, g, RPW);
    while (base < B) {
      C c[UG][F];
      int32_t id[UG][F];
#pragma unroll
      for (int u = 0; u < UG; ++u)
#pragma unroll
        for (int f = 0; f < F; ++f) {
          id[u][f] = clamp_id32(raw[u][f], M32);
          bad |= id[u][f] != raw[u][f];
          if (NT01 && f < 2)
            c[u][f].template load<true>(E + (int64_t)id[u][f] * ROW_BYTES + sub * 16);
          else
            c[u][f].template load<false>(E + (int64_t)id[u][f] * ROW_BYTES + sub * 16);
        }
      float wv[UG];
      if constexpr (HAS_W) {
#pragma unroll
        for (int u = 0; u < UG; ++u) {
          wv[u] = 0.f;
#pragma unroll
          for (int r = 0; r < WPL; ++r) {
            const int fsel = r * LPR + sub;
            int32_t my = id[u][0];
#pragma unroll
            for (int f = 1; f < F; ++f) my = (fsel == f) ? id[u][f] : my;
            const float wl = w[my];
            wv[u] += (fsel < F) ? wl : 0.f;
          }
        }
      }
      int64_t nbase = base;
      int nu0 = u0 + UG;
      if (nu0 >= U) {
        nu0 = 0;
        nbase += stride;
      }
      load_ids_slots<F, U, UG>(raw, idx, nbase, nu0, B, g, RPW);
#pragma unroll
      for (int u = 0; u < UG; ++u) {
        float t = group_sum_dpp<LPR>(fm_chunk_term<F, C, PK>(c[u]));
        float fb = 0.f;
        if constexpr (HAS_W) fb = group_sum_dpp<LPR>(wv[u]);
        const int64_t row = base + (int64_t)(u0 + u) * RPW + g;
        if (sub == 0 && u0 + u < U && row < B) out[row] = (t + fb) + w0;
      }
      base = nbase;
      u0 = nu0;
    }
  }
  report_bad_id(status, bad);
}

// Generic fallback (any k, any F <= 64): one wave per row, lanes stride over k.
template <bool BF16, bool SCALED = false>
__global__ __launch_bounds__(256) void fm_rows_generic(
    const int32_t* __restrict__ idx, int64_t B, int F, const char* __restrict__ E,
    int64_t M, int k, const float* __restrict__ w, float w0,
    float* __restrict__ out, int32_t* __restrict__ status, const float* __restrict__ scale) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int esz = BF16 ? 2 : 4;
  bool bad = false;
  for (int64_t row = wave; row < B; row += nwave) {
    const int32_t* p = idx + row * (int64_t)F;
    for (int f = lane; f < F; f += kWave) bad |= clamp_id(p[f], M) != p[f];
    float t = 0.f;
    for (int e = lane; e < k; e += kWave) {
      float s = 0.f, q = 0.f;
      for (int f = 0; f < F; ++f) {
        const char* r = E + (int64_t)clamp_id(p[f], M) * k * esz;
        float v = BF16 ? bf16_to_f32(reinterpret_cast<const uint16_t*>(r)[e])
                       : reinterpret_cast<const float*>(r)[e];
        s += v;
        q += v * v;
      }
      if constexpr (SCALED) t += scale[e] * (0.5f * (s * s - q));
      else t += 0.5f * (s * s - q);
    }
    t = group_sum<kWave>(t);
    float fb = 0.f;
    if (w != nullptr)
      for (int f = 0; f < F; ++f) fb += w[clamp_id(p[f], M)];
    if (lane == 0) out[row] = (t + fb) + w0;
  }
  report_bad_id(status, bad);
}

// ---------------------------------------------------------------------------
// HHFM row kernel, canonical column layout [user, item, ctx x NC, time x rest]
//   h = (u + Σctx) + Σtime ; out = Σ_k h·item
// ---------------------------------------------------------------------------
template <int F, int LPR, bool BF16>
__global__ __launch_bounds__(256) void hybrid_rows_fast(
    const int32_t* __restrict__ idx, int64_t B, int nctx,
    const char* __restrict__ E, int64_t M, float* __restrict__ out,
    int32_t* __restrict__ status) {
  constexpr int U = RowsPerLane<F>::value;
  constexpr int RPW = kWave / LPR;
  constexpr int RPI = RPW * U;
  constexpr int64_t ROW_BYTES = (int64_t)LPR * 16;
  using C = Chunk<BF16>;
  const uint32_t M32 = id_limit32(M);

  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (LPR - 1);
  const int g = lane / LPR;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t stride = nwave * RPI;
  const int ctx_end = 2 + nctx;

  int64_t base = wave * RPI;
  int32_t raw[U][F];
  bool bad = false;
  if (base < B) load_ids<F, U>(raw, idx, base, B, g, RPW, F);

  for (; base < B; base += stride) {
    C c[U][F];
    int32_t id[U][F];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int f = 0; f < F; ++f) {
        id[u][f] = clamp_id32(raw[u][f], M32);
        bad |= id[u][f] != raw[u][f];
        c[u][f].load(E + (int64_t)id[u][f] * ROW_BYTES + sub * 16);
      }

    // (unconditional: rows past B read row 0, which keeps vmcnt counting exact)
    load_ids<F, U>(raw, idx, base + stride, B, g, RPW, F);

#pragma unroll
    for (int u = 0; u < U; ++u) {
      float t = 0.f;
#pragma unroll
      for (int e = 0; e < C::kElems; ++e) {
        float ctx = 0.f, tim = 0.f;
#pragma unroll
        for (int f = 2; f < F; ++f) {
          if (f < ctx_end) ctx += c[u][f].v[e];
          else tim += c[u][f].v[e];
        }
        float h = c[u][0].v[e];
        if (nctx > 0) h = h + ctx;
        if (ctx_end < F) h = h + tim;
        t += h * c[u][1].v[e];
      }
      t = group_sum_dpp<LPR>(t);
      const int64_t row = base + (int64_t)u * RPW + g;
      if (sub == 0 && row < B) out[row] = t;
    }
  }
  report_bad_id(status, bad);
}

// any layout, any k, with h from the feature policy (hhfm_feature.h: the sum,
// the pooled or the two-way h); each instantiation is a kernel of its own
template <bool BF16, class Feature>
__global__ __launch_bounds__(256) void hybrid_rows_generic(
    const int32_t* __restrict__ idx, int64_t B, int ncols, int ucol, int icol,
    int c0, int c1, int t0, int t1, const char* __restrict__ E, int64_t M,
    int k, float* __restrict__ out, Feature feat, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int esz = BF16 ? 2 : 4;
  auto val = [&](int32_t id, int e) -> float {
    const char* r = E + (int64_t)clamp_id(id, M) * k * esz;
    return BF16 ? bf16_to_f32(reinterpret_cast<const uint16_t*>(r)[e])
                : reinterpret_cast<const float*>(r)[e];
  };
  bool bad = false;
  for (int64_t row = wave; row < B; row += nwave) {
    const int32_t* p = idx + row * (int64_t)ncols;
    // only the columns the score reads (user, item, ctx, time), like
    // check_query_ids_kernel: an unused column never raises
    for (int c = lane; c < ncols; c += kWave)
      if (c == ucol || c == icol || (c >= c0 && c < c1) || (c >= t0 && c < t1))
        bad |= clamp_id(p[c], M) != p[c];
    float t = 0.f;
    for (int e = lane; e < k; e += kWave)
      t += feat.forward(val(p[ucol], e), [&](int c) { return val(p[c], e); }, c0, c1, t0, t1).h *
           val(p[icol], e);
    t = group_sum<kWave>(t);
    if (lane == 0) out[row] = t;
  }
  report_bad_id(status, bad);
}

// ---------------------------------------------------------------------------
// HHFM row kernels with MAX / MEAN pooling (include/hhfm.h "Pooling";
// hhfm_pool.h).  hybrid_rows_pool is hybrid_rows_fast's load phase unchanged —
// the same F x LPR switch, load_ids, unconditional clamped loads, U rows in
// flight, group_sum_dpp — and a consume phase that steps one accumulator per
// pool and element by the modes, which are wave-uniform kernel arguments
// (SGPRs), not template parameters.
// ---------------------------------------------------------------------------
template <int F, int LPR, bool BF16>
__global__ __launch_bounds__(256) void hybrid_rows_pool(
    const int32_t* __restrict__ idx, int64_t B, int nctx,
    const char* __restrict__ E, int64_t M, float* __restrict__ out,
    PoolModes pm, int32_t* __restrict__ status) {
  constexpr int U = RowsPerLane<F>::value;
  constexpr int RPW = kWave / LPR;
  constexpr int RPI = RPW * U;
  constexpr int64_t ROW_BYTES = (int64_t)LPR * 16;
  using C = Chunk<BF16>;
  const uint32_t M32 = id_limit32(M);

  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (LPR - 1);
  const int g = lane / LPR;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t stride = nwave * RPI;
  const int ctx_end = 2 + nctx;
  const int ntime = F - ctx_end;
  const bool cmax = pm.ctx == HHFM_POOL_MAX, tmax = pm.tim == HHFM_POOL_MAX;
  const float cid = pool_identity(pm.ctx), tid = pool_identity(pm.tim);

  int64_t base = wave * RPI;
  int32_t raw[U][F];
  bool bad = false;
  if (base < B) load_ids<F, U>(raw, idx, base, B, g, RPW, F);

  for (; base < B; base += stride) {
    C c[U][F];
    int32_t id[U][F];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int f = 0; f < F; ++f) {
        id[u][f] = clamp_id32(raw[u][f], M32);
        bad |= id[u][f] != raw[u][f];
        c[u][f].load(E + (int64_t)id[u][f] * ROW_BYTES + sub * 16);
      }

    // (unconditional: rows past B read row 0, which keeps vmcnt counting exact)
    load_ids<F, U>(raw, idx, base + stride, B, g, RPW, F);

#pragma unroll
    for (int u = 0; u < U; ++u) {
      float t = 0.f;
      // one accumulator per pool and element; a field outside the pool steps
      // in the identity (wave-uniform select), and the mode is branched on
      // around the whole field x element block, so every block is straight-line
      float cv[C::kElems], tv[C::kElems];
      if (cmax) {
#pragma unroll
        for (int e = 0; e < C::kElems; ++e) cv[e] = cid;
#pragma unroll
        for (int f = 2; f < F; ++f)
#pragma unroll
          for (int e = 0; e < C::kElems; ++e)
            cv[e] = pool_step(HHFM_POOL_MAX, cv[e], f < ctx_end ? c[u][f].v[e] : cid);
      } else {
#pragma unroll
        for (int e = 0; e < C::kElems; ++e) cv[e] = cid;
#pragma unroll
        for (int f = 2; f < F; ++f)
#pragma unroll
          for (int e = 0; e < C::kElems; ++e)
            cv[e] = pool_step(HHFM_POOL_SUM, cv[e], f < ctx_end ? c[u][f].v[e] : cid);
        if (pm.ctx == HHFM_POOL_MEAN) {
#pragma unroll
          for (int e = 0; e < C::kElems; ++e) cv[e] = pool_finish(HHFM_POOL_MEAN, cv[e], nctx);
        }
      }
      if (tmax) {
#pragma unroll
        for (int e = 0; e < C::kElems; ++e) tv[e] = tid;
#pragma unroll
        for (int f = 2; f < F; ++f)
#pragma unroll
          for (int e = 0; e < C::kElems; ++e)
            tv[e] = pool_step(HHFM_POOL_MAX, tv[e], f < ctx_end ? tid : c[u][f].v[e]);
      } else {
#pragma unroll
        for (int e = 0; e < C::kElems; ++e) tv[e] = tid;
#pragma unroll
        for (int f = 2; f < F; ++f)
#pragma unroll
          for (int e = 0; e < C::kElems; ++e)
            tv[e] = pool_step(HHFM_POOL_SUM, tv[e], f < ctx_end ? tid : c[u][f].v[e]);
        if (pm.tim == HHFM_POOL_MEAN) {
#pragma unroll
          for (int e = 0; e < C::kElems; ++e) tv[e] = pool_finish(HHFM_POOL_MEAN, tv[e], ntime);
        }
      }
      if (pm.fin == HHFM_POOL_MAX) {
#pragma unroll
        for (int e = 0; e < C::kElems; ++e)
          t += pool_h(c[u][0].v[e], cv[e], nctx, tv[e], ntime, HHFM_POOL_MAX) * c[u][1].v[e];
      } else if (pm.fin == HHFM_POOL_MEAN) {
#pragma unroll
        for (int e = 0; e < C::kElems; ++e)
          t += pool_h(c[u][0].v[e], cv[e], nctx, tv[e], ntime, HHFM_POOL_MEAN) * c[u][1].v[e];
      } else {
#pragma unroll
        for (int e = 0; e < C::kElems; ++e)
          t += pool_h(c[u][0].v[e], cv[e], nctx, tv[e], ntime, HHFM_POOL_SUM) * c[u][1].v[e];
      }
      t = group_sum_dpp<LPR>(t);
      const int64_t row = base + (int64_t)u * RPW + g;
      if (sub == 0 && row < B) out[row] = t;
    }
  }
  report_bad_id(status, bad);
}

// ---------------------------------------------------------------------------
// Two-way HHFM row kernels (include/hhfm.h "Two-way pooling"; hhfm_pool.h).
// hybrid_rows_two_way is hybrid_rows_pool's load phase unchanged and a consume
// phase that forms each pool's pair products from the rows already in
// registers.  The layout (F, NCTX) is a template parameter — the reference's
// three layouts are instantiated — so every pair is a compile-time register
// pair; the six modes stay wave-uniform kernel arguments, branched on around
// whole straight-line blocks.  The blocks are two_way_mix / two_way_h2 of
// hhfm_pool.h unrolled: the same steps in the same order, the same bits.
// ---------------------------------------------------------------------------
// a[e] = the MODE pool's accumulator over rows c[F0 .. F0 + N)
template <int F0, int N, int MODE, class C>
HHFM_DEV void pool1_regs(const C* c, float* a) {
#pragma unroll
  for (int e = 0; e < C::kElems; ++e) a[e] = pool_identity(MODE);
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int e = 0; e < C::kElems; ++e) a[e] = pool_step(MODE, a[e], c[F0 + i].v[e]);
}

// ... over their pair products, (i, j), i < j, i outer
template <int F0, int N, int MODE, class C>
HHFM_DEV void pool2_regs(const C* c, float* a) {
#pragma unroll
  for (int e = 0; e < C::kElems; ++e) a[e] = pool_identity(MODE);
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = i + 1; j < N; ++j)
#pragma unroll
      for (int e = 0; e < C::kElems; ++e)
        a[e] = pool_step(MODE, a[e], pool_mul(c[F0 + i].v[e], c[F0 + j].v[e]));
}

// mix[e] = P1 + P2 of the rows c[F0 .. F0 + N)
template <int F0, int N, class C>
HHFM_DEV void mix_regs(const C* c, int m1, int m2, float* mix) {
  float a1[C::kElems], a2[C::kElems];
  if (m1 == HHFM_POOL_MAX) {
    pool1_regs<F0, N, HHFM_POOL_MAX>(c, a1);
  } else {
    pool1_regs<F0, N, HHFM_POOL_SUM>(c, a1);
    if (m1 == HHFM_POOL_MEAN) {
#pragma unroll
      for (int e = 0; e < C::kElems; ++e) a1[e] = pool_finish(HHFM_POOL_MEAN, a1[e], N);
    }
  }
  if (m2 == HHFM_POOL_MAX) {
    pool2_regs<F0, N, HHFM_POOL_MAX>(c, a2);
  } else {
    pool2_regs<F0, N, HHFM_POOL_SUM>(c, a2);
    if (m2 == HHFM_POOL_MEAN) {
#pragma unroll
      for (int e = 0; e < C::kElems; ++e)
        a2[e] = pool_finish(HHFM_POOL_MEAN, a2[e], N * (N - 1) / 2);
    }
  }
#pragma unroll
  for (int e = 0; e < C::kElems; ++e) mix[e] = a1[e] + a2[e];
}

template <int F, int NCTX, int LPR, bool BF16>
__global__ __launch_bounds__(256) void hybrid_rows_two_way(
    const int32_t* __restrict__ idx, int64_t B, const char* __restrict__ E, int64_t M,
    float* __restrict__ out, PoolModes2 pm, int32_t* __restrict__ status) {
  constexpr int U = RowsPerLane<F>::value;
  constexpr int RPW = kWave / LPR;
  constexpr int RPI = RPW * U;
  constexpr int64_t ROW_BYTES = (int64_t)LPR * 16;
  constexpr int NT = F - 2 - NCTX;
  static_assert(NCTX != 1 && NT != 1 && NCTX + NT > 0, "a two-way layout");
  using C = Chunk<BF16>;
  const uint32_t M32 = id_limit32(M);

  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (LPR - 1);
  const int g = lane / LPR;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t stride = nwave * RPI;

  int64_t base = wave * RPI;
  int32_t raw[U][F];
  bool bad = false;
  if (base < B) load_ids<F, U>(raw, idx, base, B, g, RPW, F);

  for (; base < B; base += stride) {
    C c[U][F];
    int32_t id[U][F];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int f = 0; f < F; ++f) {
        id[u][f] = clamp_id32(raw[u][f], M32);
        bad |= id[u][f] != raw[u][f];
        c[u][f].load(E + (int64_t)id[u][f] * ROW_BYTES + sub * 16);
      }

    // (unconditional: rows past B read row 0, which keeps vmcnt counting exact)
    load_ids<F, U>(raw, idx, base + stride, B, g, RPW, F);

#pragma unroll
    for (int u = 0; u < U; ++u) {
      float mc[C::kElems], mt[C::kElems], h1[C::kElems], h2[C::kElems];
#pragma unroll
      for (int e = 0; e < C::kElems; ++e) mc[e] = mt[e] = 0.f;
      if constexpr (NCTX > 0) mix_regs<2, NCTX>(c[u], pm.one.ctx, pm.two.ctx, mc);
      if constexpr (NT > 0) mix_regs<2 + NCTX, NT>(c[u], pm.one.tim, pm.two.tim, mt);
      if (pm.one.fin == HHFM_POOL_MAX) {
#pragma unroll
        for (int e = 0; e < C::kElems; ++e)
          h1[e] = pool_h(c[u][0].v[e], mc[e], NCTX, mt[e], NT, HHFM_POOL_MAX);
      } else if (pm.one.fin == HHFM_POOL_MEAN) {
#pragma unroll
        for (int e = 0; e < C::kElems; ++e)
          h1[e] = pool_h(c[u][0].v[e], mc[e], NCTX, mt[e], NT, HHFM_POOL_MEAN);
      } else {
#pragma unroll
        for (int e = 0; e < C::kElems; ++e)
          h1[e] = pool_h(c[u][0].v[e], mc[e], NCTX, mt[e], NT, HHFM_POOL_SUM);
      }
      if (pm.two.fin == HHFM_POOL_MAX) {
#pragma unroll
        for (int e = 0; e < C::kElems; ++e)
          h2[e] = two_way_h2(c[u][0].v[e], mc[e], NCTX, mt[e], NT, HHFM_POOL_MAX);
      } else if (pm.two.fin == HHFM_POOL_MEAN) {
#pragma unroll
        for (int e = 0; e < C::kElems; ++e)
          h2[e] = two_way_h2(c[u][0].v[e], mc[e], NCTX, mt[e], NT, HHFM_POOL_MEAN);
      } else {
#pragma unroll
        for (int e = 0; e < C::kElems; ++e)
          h2[e] = two_way_h2(c[u][0].v[e], mc[e], NCTX, mt[e], NT, HHFM_POOL_SUM);
      }
      float t = 0.f;
#pragma unroll
      for (int e = 0; e < C::kElems; ++e) t += (h1[e] + h2[e]) * c[u][1].v[e];
      t = group_sum_dpp<LPR>(t);
      const int64_t row = base + (int64_t)u * RPW + g;
      if (sub == 0 && row < B) out[row] = t;
    }
  }
  report_bad_id(status, bad);
}

// ---------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------
static int grid_for(int64_t rows, int64_t rows_per_block, hipStream_t s) {
  int64_t g = (rows + rows_per_block - 1) / rows_per_block;
  // CUs x HHFM_K1_CAP blocks; grid-stride the rest
  const int64_t cap = (int64_t)stream_cu_count(s) * HHFM_K1_CAP;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// every row kernel's launch: `grid` blocks of 256 threads on `s`
template <class Kernel, class... Args>
static void launch_rows(Kernel kernel, int grid, hipStream_t s, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, args...);
}

// rows a 256-thread block takes per iteration: 4 waves x 64 / LPR groups x U slots
constexpr int rows_per_block(int lpr, int u) { return 4 * (kWave / lpr) * u; }

// rows far beyond the caches (a table of 1 GiB or more): the user / item rows
// are streamed (fm_rows_fast NTM 2, fm_rows_fast_hot NT01)
static bool big_table(int64_t M, int lpr) { return M * (int64_t)lpr * 16 >= ((int64_t)1 << 30); }

// The fast kernels' template arguments from the run-time shape: fn(F, LPR,
// BF16) is called with std::integral_constants for F in FS..., lpr (16-byte
// chunks per row) in {4, 8, 16, 32, 64} and the dtype, and its result
// returned; false without a call: no kernel for the shape.
template <int... FS>
struct FSet {};
using FastF = FSet<2, 3, 4, 5, 6, 7, 8, 10, 12>;
using HotF = FSet<3, 4, 5, 6, 7, 8>;    // fm_rows_fast_hot
// hybrid_rows_two_way, the reference's layouts: F = 5 with 3 context columns
// (frappe), 10 with 5 + 3 time (jiaju), 12 with 5 + 5 (resturant)
using TwoWayF = FSet<5, 10, 12>;
constexpr int two_way_nctx(int F) { return F == 5 ? 3 : 5; }

template <int V>
using int_c = std::integral_constant<int, V>;

template <int... FS, class Fn>
static bool dispatch_rows(FSet<FS...>, int F, int lpr, bool bf16, Fn fn) {
  auto on_lpr = [&](auto f, auto b) -> bool {
    switch (lpr) {
      case 4: return fn(f, int_c<4>{}, b);
      case 8: return fn(f, int_c<8>{}, b);
      case 16: return fn(f, int_c<16>{}, b);
      case 32: return fn(f, int_c<32>{}, b);
      case 64: return fn(f, int_c<64>{}, b);
      default: return false;
    }
  };
  auto on_f = [&](auto f) -> bool {
    return bf16 ? on_lpr(f, std::true_type{}) : on_lpr(f, std::false_type{});
  };
  bool done = false;
  (void)((F == FS && ((done = on_f(int_c<FS>{})), true)) || ...);
  return done;
}

// fm_rows_fast_hot: launched when `forced` (HHFM_FLAG_HOT_TAIL) or when its
// own grid is at the cap, so that every wave loops and the 16 KiB staging per
// workgroup is amortised; false (nothing launched) otherwise, or where no such
// kernel exists for the shape.  A forced launch below that size takes a
// quarter of the uncapped blocks, so its waves iterate too.
static bool try_fm_hot(const int32_t* idx, int64_t B, int F, const char* E,
                       int64_t M, int lpr, bool bf16, const float* w, float w0,
                       float* out, bool forced, int32_t* status, hipStream_t s) {
  return dispatch_rows(HotF{}, F, lpr, bf16, [&](auto f, auto l, auto b) {
    constexpr int NF = decltype(f)::value, LPR = decltype(l)::value;
    constexpr bool BF16 = decltype(b)::value;
    constexpr int RPB = rows_per_block(LPR, HotRows<NF>::U);
    const int64_t blocks = (B + RPB - 1) / RPB;
    const int64_t cap = (int64_t)stream_cu_count(s) * HHFM_K1_HOT_CAP;
    if (blocks < cap && !forced) return false;
    int64_t g = blocks >= cap ? cap : blocks / 4;
    if (g < 1) g = 1;
    auto kernel = !w                 ? fm_rows_fast_hot<NF, LPR, BF16, false, false>
                  : big_table(M, LPR) ? fm_rows_fast_hot<NF, LPR, BF16, true, true>
                                      : fm_rows_fast_hot<NF, LPR, BF16, true, false>;
    launch_rows(kernel, (int)g, s, idx, B, E, M, w, w0, out, status);
    return true;
  });
}

// fm_rows_fast, SCALED where `scale` is given.  nt: HHFM_FLAG_STREAM_TABLE
// (NTM 1; the scaled entry point has no flags, so no such kernel); else a big
// table streams its user / item rows (NTM 2).  Without `w` neither applies.
static bool try_fm_fast(const int32_t* idx, int64_t B, int F, const char* E,
                        int64_t M, int lpr, bool bf16, const float* w, float w0,
                        const float* scale, float* out, bool nt, int32_t* status,
                        hipStream_t s) {
  return dispatch_rows(FastF{}, F, lpr, bf16, [&](auto f, auto l, auto b) {
    constexpr int NF = decltype(f)::value, LPR = decltype(l)::value;
    constexpr bool BF16 = decltype(b)::value;
    const int grid = grid_for(B, rows_per_block(LPR, RowsPerLane<NF>::value), s);
    const bool big = big_table(M, LPR);
    auto launch = [&](auto scaled) {
      constexpr bool SC = decltype(scaled)::value;
      auto kernel = !w    ? fm_rows_fast<NF, LPR, BF16, false, 0, SC>
                    : big ? fm_rows_fast<NF, LPR, BF16, true, 2, SC>
                          : fm_rows_fast<NF, LPR, BF16, true, 0, SC>;
      if constexpr (!SC) {
        if (w && nt) kernel = fm_rows_fast<NF, LPR, BF16, true, 1>;
      }
      launch_rows(kernel, grid, s, idx, B, E, M, w, w0, out, status, scale);
    };
    if (scale) launch(std::true_type{});
    else launch(std::false_type{});
    return true;
  });
}

// hybrid_rows_fast, or hybrid_rows_pool where `pm` is given
static bool try_hybrid_fast(const int32_t* idx, int64_t B, int F, int nctx,
                            const char* E, int64_t M, int lpr, bool bf16,
                            float* out, const PoolModes* pm, int32_t* status,
                            hipStream_t s) {
  return dispatch_rows(FastF{}, F, lpr, bf16, [&](auto f, auto l, auto b) {
    constexpr int NF = decltype(f)::value, LPR = decltype(l)::value;
    constexpr bool BF16 = decltype(b)::value;
    const int grid = grid_for(B, rows_per_block(LPR, RowsPerLane<NF>::value), s);
    if (pm)
      launch_rows(hybrid_rows_pool<NF, LPR, BF16>, grid, s, idx, B, nctx, E, M, out, *pm, status);
    else
      launch_rows(hybrid_rows_fast<NF, LPR, BF16>, grid, s, idx, B, nctx, E, M, out, status);
    return true;
  });
}

static bool try_two_way(const int32_t* idx, int64_t B, int F, int nctx, const char* E,
                        int64_t M, int lpr, bool bf16, float* out, PoolModes2 pm,
                        int32_t* status, hipStream_t s) {
  return dispatch_rows(TwoWayF{}, F, lpr, bf16, [&](auto f, auto l, auto b) {
    constexpr int NF = decltype(f)::value, LPR = decltype(l)::value;
    constexpr bool BF16 = decltype(b)::value;
    if (nctx != two_way_nctx(NF)) return false;
    launch_rows(hybrid_rows_two_way<NF, two_way_nctx(NF), LPR, BF16>,
                grid_for(B, rows_per_block(LPR, RowsPerLane<NF>::value), s), s, idx, B, E, M, out,
                pm, status);
    return true;
  });
}

// 16-byte chunks per row; 0: no fast kernel reads this table (rows that are
// no whole chunks, or E not 16-byte aligned)
static int lpr_for(const void* E, int64_t k, int dtype) {
  const int64_t row_bytes = k * (dtype == HHFM_BF16 ? 2 : 4);
  if (row_bytes % 16 || (reinterpret_cast<uintptr_t>(E) & 15)) return 0;
  return (int)(row_bytes / 16);
}

// The argument checks of hhfm_fm_score_rows_ex and _scaled in their order:
// shape, dtype, the entry point's own check (`own_ok`: its flags, its scale),
// then — past the empty batch — the pointers.  The caller returns on any code
// but HHFM_OK, and on B == 0.
static int check_fm_args(const int32_t* idx, int64_t B, int F, const void* E, int64_t M, int k,
                         int dtype, const float* out, bool own_ok) {
  if (B < 0 || F < 1 || F > 64 || k < 1 || M < 1) return HHFM_EINVAL;
  if (dtype != HHFM_F32 && dtype != HHFM_BF16) return HHFM_EINVAL;
  if (!own_ok) return HHFM_EINVAL;
  if (B > 0 && (!idx || !E || !out)) return HHFM_EINVAL;
  return HHFM_OK;
}

// fm_rows_fast where it exists for the shape, fm_rows_generic otherwise
static int launch_fm_rows(const int32_t* idx, int64_t B, int F, const char* E, int64_t M, int k,
                          int lpr, bool bf16, const float* w, float w0, const float* scale,
                          float* out, bool nt, int32_t* status, hipStream_t s) {
  if (!(lpr && try_fm_fast(idx, B, F, E, M, lpr, bf16, w, w0, scale, out, nt, status, s))) {
    auto kernel = scale ? (bf16 ? fm_rows_generic<true, true> : fm_rows_generic<false, true>)
                        : (bf16 ? fm_rows_generic<true> : fm_rows_generic<false>);
    launch_rows(kernel, grid_for(B, 4, s), s, idx, B, F, E, M, k, w, w0, out, status, scale);
  }
  return (int)hipGetLastError();
}

// What hhfm_hybrid_score_rows_ex, _pool and _pool2 check, in their order:
// shape, dtype, the columns and ranges, for _pool2 (`two_way`) the two-way
// layout, then — past the empty batch — the pointers.  The caller returns on
// any code but HHFM_OK, and on B == 0; otherwise `sh` is the launch's shape.
struct HybridShape {
  int nctx, ntime;
  bool canonical;   // [user, item, ctx..., time...] spanning every column
  int lpr;          // lpr_for
  bool bf16;
};

static int check_hybrid_args(const int32_t* idx, int64_t B, int ncols, int user_col, int item_col,
                             int ctx_begin, int ctx_end, int time_begin, int time_end,
                             const void* E, int64_t M, int k, int dtype, const float* out,
                             bool two_way, HybridShape& sh) {
  if (B < 0 || ncols < 2 || ncols > 64 || k < 1 || M < 1) return HHFM_EINVAL;
  if (dtype != HHFM_F32 && dtype != HHFM_BF16) return HHFM_EINVAL;
  auto in_range = [&](int c) { return c >= 0 && c < ncols; };
  if (!in_range(user_col) || !in_range(item_col)) return HHFM_EINVAL;
  if (ctx_begin > ctx_end || time_begin > time_end) return HHFM_EINVAL;
  if (ctx_end > ctx_begin && (!in_range(ctx_begin) || ctx_end > ncols)) return HHFM_EINVAL;
  if (time_end > time_begin && (!in_range(time_begin) || time_end > ncols)) return HHFM_EINVAL;
  sh.nctx = ctx_end - ctx_begin;
  sh.ntime = time_end - time_begin;
  if (two_way && !two_way_shape_ok(sh.nctx, sh.ntime)) return HHFM_EINVAL;
  if (B > 0 && (!idx || !E || !out)) return HHFM_EINVAL;
  sh.canonical = user_col == 0 && item_col == 1 && (sh.nctx == 0 || ctx_begin == 2) &&
                 (sh.ntime == 0 || time_begin == 2 + sh.nctx) && 2 + sh.nctx + sh.ntime == ncols;
  sh.lpr = lpr_for(E, k, dtype);
  sh.bf16 = dtype == HHFM_BF16;
  return HHFM_OK;
}

// the generic fall-back of the three hhfm_hybrid_score_rows* entry points
template <class Feature>
static void launch_hybrid_generic(Feature feat, const int32_t* idx, int64_t B, int ncols, int ucol,
                                  int icol, int c0, int c1, int t0, int t1, const char* E,
                                  int64_t M, int k, bool bf16, float* out, int32_t* status,
                                  hipStream_t s) {
  auto kernel = bf16 ? hybrid_rows_generic<true, Feature> : hybrid_rows_generic<false, Feature>;
  launch_rows(kernel, grid_for(B, 4, s), s, idx, B, ncols, ucol, icol, c0, c1, t0, t1, E, M, k,
              out, feat, status);
}

}  // namespace hhfm

using namespace hhfm;

extern "C" int hhfm_fm_score_rows_ex(const int32_t* idx, int64_t B, int32_t F,
                                     const void* E, int64_t features_M, int32_t k,
                                     int32_t dtype, const float* w, float w0,
                                     float* out, int32_t flags, int32_t* status,
                                     void* stream) {
  const bool hot_forced = (flags & HHFM_FLAG_HOT_TAIL) != 0;
  const bool hot_refused = (flags & (HHFM_FLAG_NO_HOT_TAIL | HHFM_FLAG_STREAM_TABLE)) != 0;
  // the LDS-tail kernel has no all-streaming plan, and cannot be both forced and refused
  const bool flags_ok =
      !(flags & ~(HHFM_FLAG_STREAM_TABLE | HHFM_FLAG_HOT_TAIL | HHFM_FLAG_NO_HOT_TAIL)) &&
      !(hot_forced && hot_refused);
  const int rc = check_fm_args(idx, B, F, E, features_M, k, dtype, out, flags_ok);
  if (rc != HHFM_OK || B == 0) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const char* Eb = reinterpret_cast<const char*>(E);
  const bool bf16 = dtype == HHFM_BF16;
  const int lpr = lpr_for(E, k, dtype);
  if (HHFM_K1_HOT_AUTO || hot_forced) {
    if (!hot_refused && lpr &&
        try_fm_hot(idx, B, F, Eb, features_M, lpr, bf16, w, w0, out, hot_forced, status, s))
      return (int)hipGetLastError();
    if (hot_forced) return HHFM_EUNSUPPORTED;   // F outside 3..8, or rows not whole 16-B chunks
  }
  return launch_fm_rows(idx, B, F, Eb, features_M, k, lpr, bf16, w, w0, nullptr, out,
                        (flags & HHFM_FLAG_STREAM_TABLE) != 0, status, s);
}

extern "C" int hhfm_fm_score_rows_scaled(const int32_t* idx, int64_t B, int32_t F,
                                         const void* E, int64_t features_M, int32_t k,
                                         int32_t dtype, const float* w, float w0,
                                         const float* scale, float* out, int32_t* status,
                                         void* stream) {
  const int rc = check_fm_args(idx, B, F, E, features_M, k, dtype, out, scale != nullptr);
  if (rc != HHFM_OK || B == 0) return rc;
  return launch_fm_rows(idx, B, F, reinterpret_cast<const char*>(E), features_M, k,
                        lpr_for(E, k, dtype), dtype == HHFM_BF16, w, w0, scale, out, false, status,
                        reinterpret_cast<hipStream_t>(stream));
}

extern "C" int hhfm_fm_score_rows(const int32_t* idx, int64_t B, int32_t F,
                                  const void* E, int64_t features_M, int32_t k,
                                  int32_t dtype, const float* w, float w0,
                                  float* out, void* stream) {
  return hhfm_fm_score_rows_ex(idx, B, F, E, features_M, k, dtype, w, w0, out,
                               HHFM_FM_ROWS_DEFAULT_FLAGS, nullptr, stream);
}

extern "C" int hhfm_hybrid_score_rows_ex(const int32_t* idx, int64_t B,
                                         int32_t ncols, int32_t user_col,
                                         int32_t item_col, int32_t ctx_begin,
                                         int32_t ctx_end, int32_t time_begin,
                                         int32_t time_end, const void* E,
                                         int64_t features_M, int32_t k,
                                         int32_t dtype, float* out, int32_t* status,
                                         void* stream) {
  HybridShape sh;
  const int rc = check_hybrid_args(idx, B, ncols, user_col, item_col, ctx_begin, ctx_end,
                                   time_begin, time_end, E, features_M, k, dtype, out, false, sh);
  if (rc != HHFM_OK || B == 0) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const char* Eb = reinterpret_cast<const char*>(E);
  if (!(sh.canonical && sh.lpr &&
        try_hybrid_fast(idx, B, ncols, sh.nctx, Eb, features_M, sh.lpr, sh.bf16, out, nullptr,
                        status, s)))
    launch_hybrid_generic(SumFeature{}, idx, B, ncols, user_col, item_col, ctx_begin, ctx_end,
                          time_begin, time_end, Eb, features_M, k, sh.bf16, out, status, s);
  return (int)hipGetLastError();
}

extern "C" int hhfm_hybrid_score_rows(const int32_t* idx, int64_t B,
                                      int32_t ncols, int32_t user_col,
                                      int32_t item_col, int32_t ctx_begin,
                                      int32_t ctx_end, int32_t time_begin,
                                      int32_t time_end, const void* E,
                                      int64_t features_M, int32_t k,
                                      int32_t dtype, float* out, void* stream) {
  return hhfm_hybrid_score_rows_ex(idx, B, ncols, user_col, item_col, ctx_begin, ctx_end,
                                   time_begin, time_end, E, features_M, k, dtype, out,
                                   nullptr, stream);
}

// H1 with pooling: pooling == 0 is hhfm_hybrid_score_rows_ex itself; any other
// legal word runs hybrid_rows_pool (same shapes as hybrid_rows_fast) or
// hybrid_rows_generic over PoolFeature.  Argument checks as in hhfm_hybrid_score_rows_ex.
extern "C" int hhfm_hybrid_score_rows_pool(const int32_t* idx, int64_t B,
                                           int32_t ncols, int32_t user_col,
                                           int32_t item_col, int32_t ctx_begin,
                                           int32_t ctx_end, int32_t time_begin,
                                           int32_t time_end, const void* E,
                                           int64_t features_M, int32_t k,
                                           int32_t dtype, float* out, int32_t pooling,
                                           int32_t* status, void* stream) {
  PoolModes pm;
  if (!pooling_unpack(pooling, pm)) return HHFM_EINVAL;
  if (pooling == 0)
    return hhfm_hybrid_score_rows_ex(idx, B, ncols, user_col, item_col, ctx_begin, ctx_end,
                                     time_begin, time_end, E, features_M, k, dtype, out,
                                     status, stream);
  HybridShape sh;
  const int rc = check_hybrid_args(idx, B, ncols, user_col, item_col, ctx_begin, ctx_end,
                                   time_begin, time_end, E, features_M, k, dtype, out, false, sh);
  if (rc != HHFM_OK || B == 0) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const char* Eb = reinterpret_cast<const char*>(E);
  if (!(sh.canonical && sh.lpr &&
        try_hybrid_fast(idx, B, ncols, sh.nctx, Eb, features_M, sh.lpr, sh.bf16, out, &pm, status,
                        s)))
    launch_hybrid_generic(PoolFeature{pm}, idx, B, ncols, user_col, item_col, ctx_begin, ctx_end,
                          time_begin, time_end, Eb, features_M, k, sh.bf16, out, status, s);
  return (int)hipGetLastError();
}

// H1, two-way: hybrid_rows_two_way on the reference's canonical layouts,
// hybrid_rows_generic over TwoWayFeature everywhere else.  pooling2 == 0 is still the
// two-way model (no routing to the one-way kernels).
extern "C" int hhfm_hybrid_score_rows_pool2(const int32_t* idx, int64_t B,
                                            int32_t ncols, int32_t user_col,
                                            int32_t item_col, int32_t ctx_begin,
                                            int32_t ctx_end, int32_t time_begin,
                                            int32_t time_end, const void* E,
                                            int64_t features_M, int32_t k,
                                            int32_t dtype, float* out, int32_t pooling,
                                            int32_t pooling2, int32_t* status,
                                            void* stream) {
  PoolModes2 pm;
  if (!pooling2_unpack(pooling, pooling2, pm)) return HHFM_EINVAL;
  HybridShape sh;
  const int rc = check_hybrid_args(idx, B, ncols, user_col, item_col, ctx_begin, ctx_end,
                                   time_begin, time_end, E, features_M, k, dtype, out, true, sh);
  if (rc != HHFM_OK || B == 0) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const char* Eb = reinterpret_cast<const char*>(E);
  if (!(sh.canonical && sh.lpr &&
        try_two_way(idx, B, ncols, sh.nctx, Eb, features_M, sh.lpr, sh.bf16, out, pm, status, s)))
    launch_hybrid_generic(TwoWayFeature{pm}, idx, B, ncols, user_col, item_col, ctx_begin, ctx_end,
                          time_begin, time_end, Eb, features_M, k, sh.bf16, out, status, s);
  return (int)hipGetLastError();
}

extern "C" const char* hhfm_error_string(int code) {
  switch (code) {
    case HHFM_OK: return "ok";
    case HHFM_EINVAL: return "invalid argument";
    case HHFM_EUNSUPPORTED: return "unsupported shape";
    case HHFM_EWORKSPACE: return "workspace too small";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
  }
}

extern "C" int hhfm_abi_version(void) { return HHFM_ABI_VERSION; }
