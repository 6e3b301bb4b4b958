/*
 * hhfm.h — C ABI of the MI355X (gfx950) factorization-machine scoring backend.
 *
 * The reference (data-man-34/HHFM, Newcode/{FM,OurModel7,AFM,DFM,CARS2}.py) has no native code and no FFI:
 * its hot path is a chain of TensorFlow-1.x graph ops run through
 * `model.sess.run(...)`.  Each entry point below replaces one such op chain
 * (reference file:line cited per function).  The Python host package
 * `hhfm_amd` binds these through the thin pybind11 module `_hhfm`; the ctypes
 * stub a maintainer would add instead is in INTEGRATION.md.
 *
 * Conventions (every function):
 *   - all array pointers are DEVICE memory owned by the caller; the library
 *     allocates nothing and keeps no global mutable state (reentrant);
 *   - `stream` is a hipStream_t (NULL = default stream); every call is
 *     asynchronous on it;
 *   - index arrays are row-major int32 [rows][ncols] (the reference feeds
 *     int32 placeholders, FM.py:89);
 *   - embedding tables are row-major [features_M][k] in `dtype`
 *     (HHFM_F32 or HHFM_BF16; compute is always fp32);
 *   - return 0 on success, a positive hipError_t on a launch error, or a
 *     negative HHFM_E* code for invalid arguments (see hhfm_error_string).
 */
#ifndef HHFM_H_
#define HHFM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HHFM_ABI_VERSION 6
/* leading workspace bytes of hhfm_catalog_topk(_ex) that must start zero */
#define HHFM_CATALOG_WS_ZERO 16384

enum hhfm_dtype { HHFM_F32 = 0, HHFM_BF16 = 1 };

/* Plan flags (ABI v4).  Which kernel runs is chosen from the shapes and these
 * per-call flags only — the library reads no environment variable.  0 is the
 * default plan.  HHFM_PLAN_EXACT_FP32 is the one NUMERICS choice: the dot
 * products run as k-ordered fp32 fmaf chains on fp32 MFMA instead of on bf16
 * MFMA over an exact three-piece bf16 split of every fp32 operand (both within
 * 1e-5 relative of the reference).  Every other bit forces an
 * alternative kernel that other shapes take anyway (same products; bit-
 * identical, or the same terms summed in another order) so the tests can
 * compare both paths on one shape.  Bits an entry point does not use are
 * ignored; bits outside HHFM_PLAN_ALL are rejected with HHFM_EINVAL. */
#define HHFM_PLAN_DEFAULT 0
#define HHFM_PLAN_EXACT_FP32 (1 << 0) /* catalog, AFM, DeepFM fp32 hidden layers */
#define HHFM_PLAN_NO_SEED (1 << 1)    /* catalog streaming path: no threshold-seed pass */
#define HHFM_PLAN_NO_RING (1 << 2)    /* catalog streaming path: catalog_main, not the ring */
#define HHFM_PLAN_RING_ALT (1 << 3)   /* catalog ring: 8 waves per workgroup for bf16
                                         tables, 4 for fp32 (default: the other way) */
#define HHFM_PLAN_GEMM (1 << 4)       /* small catalog and AFM catalog: the score matrix
                                         from the shared LDS-tiled fp32 GEMM */
#define HHFM_PLAN_ROW_FM (1 << 5)     /* DeepFM fp32 MLP: FM part from the table rows,
                                         not from the pair table C = (E*Wp)E^T */
#define HHFM_PLAN_UNSTAGED (1 << 6)   /* DeepFM fp32 MLP: P rows and table rows read
                                         through the caches, not staged in LDS */
#define HHFM_PLAN_UNGROUPED (1 << 7)  /* DeepFM fp32 MLP: rows not grouped by user */
#define HHFM_PLAN_NARROW (1 << 8)     /* DeepFM bf16 ITEM plan: 128-row kernel, not the 256-row one */
#define HHFM_PLAN_PER_FIELD (1 << 9)  /* AFM catalog: pair product split per query field
                                         (afm_cat_fused), not the folded weights */
#define HHFM_PLAN_ONE_WAVE (1 << 10)  /* dense top-K: one wave per query at every size */
/* DeepFM bf16 ITEM plan, 256-row kernel: its workgroup shape (16-row tiles per
 * wave x waves) — 0 the default 2 x 8; these alternates are instantiated for
 * the k = 64, 3 x 150 test shape only (ABI v5), so every shape the kernel
 * template admits runs in the parity tests (bit-identical by construction) */
#define HHFM_PLAN_WIDE_3X4 (1 << 11)
#define HHFM_PLAN_WIDE_2X4 (2 << 11)
#define HHFM_PLAN_WIDE_1X4 (3 << 11)
#define HHFM_PLAN_WIDE_MASK (3 << 11)
#define HHFM_PLAN_STORE (1 << 13)     /* small catalog: the score matrix materialised by the
                                         catalog kernel + dense top-K, not the fused
                                         score-and-select kernel (ABI v5) */
#define HHFM_PLAN_FUSED (1 << 14)     /* small catalog: the fused kernel at any query count
                                         (default: from 1,024 queries) (ABI v5) */
#define HHFM_PLAN_ALL ((1 << 15) - 1)

/* catalog scoring modes */
enum hhfm_catalog_mode {
  HHFM_MODE_FM = 0,   /* FM.topk:  (u+f)·(i+f) + w_i        FM.py:174-185      */
  HHFM_MODE_HHFM = 1  /* OUR.topk: (u+Σctx[+Σtime])·i        OurModel7.py:232-295 */
};

enum hhfm_status {
  HHFM_OK = 0,
  HHFM_EINVAL = -1,       /* bad size / pointer / column range            */
  HHFM_EUNSUPPORTED = -2, /* shape outside what the kernels implement     */
  HHFM_EWORKSPACE = -3    /* workspace smaller than *_workspace() reports */
};

const char* hhfm_error_string(int code);
int hhfm_abi_version(void);

/* ------------------------------------------------------------------------
 * M1 — FM per-row score (replaces the `FM.out` graph, FM.py:99-120)
 *   out[b] = Σ_k ½[(Σ_f E[x_bf,k])² − Σ_f E[x_bf,k]²] + Σ_f w[x_bf] + w0
 * idx: int32 [B][F]; w may be NULL (then Σw = 0, the DeepFM-interaction use).
 * out: float [B].
 * ---------------------------------------------------------------------- */
int hhfm_fm_score_rows(const int32_t* idx, int64_t B, int32_t F,
                       const void* E, int64_t features_M, int32_t k,
                       int32_t dtype, const float* w, float w0, float* out,
                       void* stream);

/* Same, with tuning flags and an optional id status word:
 *   HHFM_FLAG_STREAM_TABLE — read embedding rows / ids and write `out` with
 *   non-temporal accesses (measured 10 % slower at configs[1]).
 *   HHFM_FLAG_HOT_TAIL / HHFM_FLAG_NO_HOT_TAIL — force / refuse the LDS-tail
 *   kernel: for 3 <= F <= 8 and rows of whole 16-byte chunks
 *   every workgroup stages the table's last 16 KiB of rows (and their `w`) in
 *   LDS and reads columns 2.. from there, which is where the loaders' column-
 *   major token numbering puts the small context vocabularies; rows with an
 *   id of columns 2.. outside that window are computed from global memory by
 *   the same kernel.  The same bits as the default kernel for any input.
 *   Automatic rule (neither bit): taken when the call is large enough that
 *   its grid is at the per-CU block cap (about 1.6 M rows at k = 64 fp32), so
 *   the staging is amortised, and HHFM_FLAG_STREAM_TABLE is not set.
 *   HOT_TAIL forces it at any B (HHFM_EUNSUPPORTED when the shape has no such
 *   kernel); NO_HOT_TAIL keeps the default kernel.  HOT_TAIL together with
 *   NO_HOT_TAIL or STREAM_TABLE is HHFM_EINVAL.
 *   Any other bit is rejected with HHFM_EINVAL.
 *   Without the flag, a table of 1 GiB or more (far beyond the caches) loads
 *   the first two columns' rows — the user and item, read once per launch —
 *   non-temporal and everything else with the default policy (the same
 *   arithmetic and bits; 2.4 % faster at configs[1]).
 * status: NULL, or a device int32 the kernel ORs HHFM_STATUS_BAD_ID into when
 *   it meets an id outside [0, features_M) (such ids are read as row 0 so the
 *   kernel cannot fault).  hhfm_status_read() turns it into HHFM_EINVAL —
 *   the InvalidArgumentError tf.nn.embedding_lookup raises (FM.py:99). */
#define HHFM_FLAG_STREAM_TABLE 1
#define HHFM_FLAG_HOT_TAIL 2
#define HHFM_FLAG_NO_HOT_TAIL 4
#define HHFM_FM_ROWS_DEFAULT_FLAGS 0
#define HHFM_STATUS_BAD_ID 1
int hhfm_fm_score_rows_ex(const int32_t* idx, int64_t B, int32_t F,
                          const void* E, int64_t features_M, int32_t k,
                          int32_t dtype, const float* w, float w0, float* out,
                          int32_t flags, int32_t* status, void* stream);

/* Column-weighted form (the inference score of FM with batch_norm=1, "FM
 * batch norm" below):
 *   out[b] = (Σ_c scale[c]·½[(Σ_f E[x_bf,c])² − Σ_f E[x_bf,c]²] + Σ_f w[x_bf]) + w0
 * scale: device float [k], never NULL.  fp32 and bf16 tables, w == NULL, the
 * status word, bad ids read as row 0 and the generic kernel for rows that are
 * not whole 16-byte chunks are hhfm_fm_score_rows_ex's.  It takes no flags
 * and never runs the LDS-tail kernel.  With scale ≡ 1 the output has the bits
 * of hhfm_fm_score_rows (the same order; a product with 1.0f is exact). */
int hhfm_fm_score_rows_scaled(const int32_t* idx, int64_t B, int32_t F,
                              const void* E, int64_t features_M, int32_t k,
                              int32_t dtype, const float* w, float w0,
                              const float* scale, float* out, int32_t* status,
                              void* stream);

/* ------------------------------------------------------------------------
 * H1 — HHFM per-row score (replaces `OUR.PositiveFeadback`,
 * OurModel7.py:105-171 with sum pooling, :14-19)
 *   h_b = E[x_b,user_col] + Σ_{c∈[ctx_begin,ctx_end)} E[x_bc]
 *                         (+ Σ_{t∈[time_begin,time_end)} E[x_bt])
 *   out[b] = Σ_k h_b,k · E[x_b,item_col],k
 * An empty range (begin == end) disables that term. idx: int32 [B][ncols].
 * ---------------------------------------------------------------------- */
int hhfm_hybrid_score_rows(const int32_t* idx, int64_t B, int32_t ncols,
                           int32_t user_col, int32_t item_col,
                           int32_t ctx_begin, int32_t ctx_end,
                           int32_t time_begin, int32_t time_end,
                           const void* E, int64_t features_M, int32_t k,
                           int32_t dtype, float* out, void* stream);
/* Same, with the optional id status word of hhfm_fm_score_rows_ex. */
int hhfm_hybrid_score_rows_ex(const int32_t* idx, int64_t B, int32_t ncols,
                              int32_t user_col, int32_t item_col,
                              int32_t ctx_begin, int32_t ctx_end,
                              int32_t time_begin, int32_t time_end,
                              const void* E, int64_t features_M, int32_t k,
                              int32_t dtype, float* out, int32_t* status,
                              void* stream);

/* ------------------------------------------------------------------------
 * Pooling — MAX and MEAN beside SUM for the three live pools of the reference
 * (OurModel7.py:14-19: Pooling1C over the context rows :124 / :255, Pooling1T
 * over the time rows :141 / :267, Pooling1F over the stack {user, context
 * pool, time pool} :168 / :292; its Pooling2* results are used by "Two-way
 * pooling" below alone).
 * The *_pool entry points below are pure additions: every earlier entry point
 * keeps its signature and behaviour, so HHFM_ABI_VERSION stays 6.
 *
 * `pooling` packs the three modes, ctx | time << 4 | final << 8
 * (HHFM_POOLING); all 27 triples are legal runtime values, any other bit or
 * mode value is HHFM_EINVAL.  pooling == 0 (sum, sum, sum) runs the very
 * kernels the unpooled entry points run: the same bits.
 * Per element e, in fp32 (nc context rows, nt time rows, in column order):
 *   context pool  sum ((r0 + r1) + ...); max the largest value (the
 *                 accumulator starts from the first row, never from 0); mean
 *                 that sum, then one fp32 division by (float)nc
 *   time pool     the same over the nt time rows
 *   stack         user, then the context pool if nc > 0, then the time pool
 *                 if nt > 0
 *   h             the final pool over the stack in that order: sum
 *                 (u + c) + t, max the largest member, mean the sum form
 *                 divided by the number of members; a single member: h = u
 *   score         Σ_e h_e · item_e, as in H1 / H2
 * (csrc/hhfm_pool.h is the one device implementation; numpy restatement in
 * tests/hhfm_pool_ref.py.)
 * hhfm_hhfm_train_step_det has no pooled form yet.
 * ---------------------------------------------------------------------- */
enum hhfm_pool { HHFM_POOL_SUM = 0, HHFM_POOL_MAX = 1, HHFM_POOL_MEAN = 2 };
#define HHFM_POOLING(ctx, time, final) ((ctx) | (time) << 4 | (final) << 8)

/* H1 with pooling (the arguments of hhfm_hybrid_score_rows_ex, then `pooling`). */
int hhfm_hybrid_score_rows_pool(const int32_t* idx, int64_t B, int32_t ncols,
                                int32_t user_col, int32_t item_col,
                                int32_t ctx_begin, int32_t ctx_end,
                                int32_t time_begin, int32_t time_end,
                                const void* E, int64_t features_M, int32_t k,
                                int32_t dtype, float* out, int32_t pooling,
                                int32_t* status, void* stream);

/* ------------------------------------------------------------------------
 * Two-way pooling — the reference's second level of hybrid feature
 * (OurModel7.py:113-122 mixdouble_features_context, :130-139
 * mixdouble_features_time, :157-166 hybrid_feature2d, pooled by Pooling2C /
 * Pooling2T / Pooling2F) with the three additions its committed text comments
 * out as "#2-way stack hybrid feature" (:124, :141, :168; topk :255, :267,
 * :292) put back.  The entry points above never form these: there the
 * Pooling2* results stay unused.  The *_pool2 entry points are pure
 * additions; HHFM_ABI_VERSION stays 6.
 *
 * Per element e, in fp32.  Each product is one rounded multiply, never
 * contracted into an FMA with the add that follows it (its value is compared
 * by a max pool, selected, and re-formed in the backward pass).
 *   context   rows r_0 .. r_{nc-1} in column order.  P1 = the context pool of
 *             "Pooling" above by `pooling`'s ctx mode.  Pairs (i, j), i < j,
 *             i outer (the reference's loop order), p_ij = r_i · r_j; P2 = the
 *             pool of the nc(nc-1)/2 products in that order by `pooling2`'s
 *             ctx mode, through the same identity / step / finish (mean: the
 *             sum, then one division by the number of products).
 *             mix_c = P1 + P2 (one add).
 *   time      the same over the nt time rows by the two words' time modes.
 *   stack     members s_0 = u, then mix_c if nc > 0, then mix_t if nt > 0.
 *             H1 = the final pool of "Pooling" over them by `pooling`'s final
 *             mode; H2 = the pool by `pooling2`'s final mode of the member
 *             products in the order (0,1), (0,2), (1,2).
 *   h         H1 + H2 (one add);  score = Σ_e h_e · item_e.
 * `pooling2` packs its three modes exactly like `pooling` (HHFM_POOLING); all
 * 27 x 27 combinations are legal, a stray bit or a mode of 3 in either word is
 * HHFM_EINVAL.  pooling2 == 0 (sum, sum, sum) is still the two-way model — a
 * different model from the one-way one — so "off" is not a value of the word:
 * the one-way model is the entry points above.
 * Refused shapes (HHFM_EINVAL, nothing written): a present pool of exactly
 * one row (nc == 1 or nt == 1) and a stack of one member (nc == nt == 0); the
 * reference's graph cannot be built for them either (it stacks an empty list
 * at :119 / :136 / :163).
 * Gradients follow TF's: a product sends d·r_j to r_i and d·r_i to r_j (an id
 * that occurs twice receives both); the pools of both levels use the rules of
 * hhfm_hhfm_train_step_pool — sum d, mean d / n, max d shared among the
 * values bit-equal to the maximum.
 * (csrc/hhfm_pool.h two_way_h is the one device implementation; numpy
 * restatement in tests/hhfm_two_way_ref.py.)
 * Not built: a two-way form of the small-catalog fused kernel,
 * a deterministic two-way step, two-way on bf16 training tables.
 * ---------------------------------------------------------------------- */
/* H1, two-way (the arguments of hhfm_hybrid_score_rows_pool, with `pooling2`
 * after `pooling`). */
int hhfm_hybrid_score_rows_pool2(const int32_t* idx, int64_t B, int32_t ncols,
                                 int32_t user_col, int32_t item_col,
                                 int32_t ctx_begin, int32_t ctx_end,
                                 int32_t time_begin, int32_t time_end,
                                 const void* E, int64_t features_M, int32_t k,
                                 int32_t dtype, float* out, int32_t pooling,
                                 int32_t pooling2, int32_t* status, void* stream);

/* ------------------------------------------------------------------------
 * M2/H2 — full-catalog score + fused top-K (replaces FM.topk, FM.py:172-198,
 * and OUR.topk, OurModel7.py:229-307: broadcast multiply [B,N,k] +
 * reduce_sum + tf.nn.top_k), without materialising the [B,N] score matrix.
 *
 *   query columns (qidx int32 [B][ncols]):
 *     HHFM_MODE_HHFM: h = E[user] + Σ ctx cols (+ Σ time cols); score = h·E[item]
 *     HHFM_MODE_FM:   f = Σ ctx cols, q = E[user]+f;
 *                     score = q·(E[item]+f) + w[item]   (w may be NULL)
 *   catalog: items are rows [item_row_begin, item_row_begin+item_count) of E.
 *   output:  top_score/top_idx [B][K], sorted by (score desc, index asc) —
 *            tf.nn.top_k order; top_idx = global_item_base + offset in range.
 *   K must be in [1, HHFM_TOPK_MAX_K] and <= item_count ("Wide K" below for
 *            K > 64).
 *   arithmetic: the h·item products run on bf16 MFMA with every fp32
 *            operand split exactly into three bf16 pieces (products of
 *            order >= 2^-16 kept, fp32 accumulation: ~1e-7 relative to a
 *            k-ordered fp32 chain); plan HHFM_PLAN_EXACT_FP32 (the _ex form)
 *            selects the fp32-MFMA kernels (the k-ordered fmaf chain).
 *   score range: the streaming path without a threshold seed starts its
 *            per-query threshold hint at about -3.39e38 (the workspace words
 *            are filled with byte 0x80), so catalog scores are assumed finite
 *            and above that value; +-inf or NaN table values are unsupported.
 * Workspace: query `hhfm_catalog_topk_workspace` with the same sizes (it
 * covers every plan).  Its first HHFM_CATALOG_WS_ZERO bytes must be zero
 * before the first call (the small-catalog kernel's per-call arrival
 * counters: every call leaves them zero again); a buffer used by other
 * entry points in between must be re-zeroed there (ABI v6).
 * What the tests pin (tests/test_gpu_workspace_contract.py, region by region
 * in profiles/workspace_contract_map.txt):
 *   - only that prefix must be zero: the rest of the workspace may hold
 *     anything when a call starts (every region is written by the call before
 *     it is read; the results are bit-identical over zero, 0xFF and 0x7F
 *     bytes), and the same holds for the whole workspace of every other
 *     scoring / top-K entry point, the exclusion-list builder and the sampler;
 *   - every call, on every path and plan and of every form that shares this
 *     layout (_pool, _pool2, _excl, CARS2, AFM without attention), leaves the
 *     prefix zero: only the small-catalog kernel writes there, and it re-arms
 *     its counters; no region of any plan lies below HHFM_CATALOG_WS_ZERO;
 *   - one workspace serves any sequence of calls it is large enough for,
 *     whatever their B, item_count, K, dtype, mode and plan.
 * A prefix that is NOT zero is a caller error the library cannot see: the
 * partial lists are then merged by the wrong workgroup or by none (wrong or
 * unwritten output, HHFM_OK returned).
 * ---------------------------------------------------------------------- */
int hhfm_catalog_topk_workspace(int64_t B, int32_t item_count, int32_t k,
                                int32_t K, size_t* ws_bytes);

/* ------------------------------------------------------------------------
 * Wide K: 65 <= K <= HHFM_TOPK_MAX_K ("narrow" is K <= 64) — ABI v6, additions
 * only.  Every catalog entry point of this header (hhfm_catalog_topk and its
 * _ex, _pool, _pool2 and _excl forms, the CARS2 and AFM-without-attention
 * forms, hhfm_afm_catalog_topk*, hhfm_dfm_catalog_topk*), hhfm_topk_dense,
 * _dense_ex, _dense_excl and hhfm_topk_merge take a wide K with the signature
 * and the meaning of the narrow call:
 *   order:   score descending, index ascending on equal scores; a wide list is
 *            that order carried further, so for K' < K the top-K' list is the
 *            first K' entries of the top-K list, scores bit for bit (+0 and
 *            -0 are equal scores ordered by index, as in the narrow kernels,
 *            and each comes out with its own sign bit).
 *   scores:  those of the narrow call under the same HHFM_PLAN_EXACT_FP32 /
 *            HHFM_PLAN_GEMM bits (the same products in the same k order).  Plan
 *            bits that choose among narrow selection kernels (_NO_SEED,
 *            _NO_RING, _RING_ALT, _FUSED, _STORE, _ONE_WAVE) are accepted and
 *            have no effect.
 *   unchanged: the score range, the id status word, global_item_base, the
 *            exclusion lists and their K + max_excl <= item_count rule.
 *   errors:  K > item_count is HHFM_EINVAL (checked first),
 *            K > HHFM_TOPK_MAX_K HHFM_EUNSUPPORTED.
 * Route (hhfm_catalog_topk family): the score matrix of a small catalog, or
 * of one block of at most 16,384 items after another of a large one, is
 * written by the narrow call's own score kernels, masked at listed columns,
 * and selected by one workgroup per query that keeps its list in LDS; the
 * blocks' lists are merged into a running list.
 * Workspace of that family: hhfm_catalog_topk_wide_workspace, a host-only
 * query valid for 1 <= K <= HHFM_TOPK_MAX_K (hhfm_catalog_topk_workspace keeps
 * refusing K > 64).  For K <= 64 it is the narrow query.  For K > 64 it covers
 * one score block plus the running lists and does not grow with item_count
 * beyond 16,384.  A wide call on a smaller buffer returns HHFM_EWORKSPACE
 * before anything is launched.  The rules above hold unchanged: the first
 * HHFM_CATALOG_WS_ZERO bytes zero before the first call and left zero by every
 * call (the wide route never writes there), the rest may hold anything, one
 * buffer serves any mix of narrow and wide calls it is large enough for.  The
 * AFM and DeepFM catalogs select from the score block they already own: their
 * workspace queries are unchanged.
 * ---------------------------------------------------------------------- */
#define HHFM_TOPK_MAX_K 1024
int hhfm_catalog_topk_wide_workspace(int64_t B, int32_t item_count, int32_t k,
                                     int32_t K, size_t* ws_bytes);

int hhfm_catalog_topk(const int32_t* qidx, int64_t B, int32_t ncols,
                      int32_t mode, int32_t user_col, int32_t ctx_begin,
                      int32_t ctx_end, int32_t time_begin, int32_t time_end,
                      const void* E, int64_t features_M, int32_t k,
                      int32_t dtype, const float* w, int32_t item_row_begin,
                      int32_t item_count, int32_t global_item_base, int32_t K,
                      float* top_score, int32_t* top_idx, void* workspace,
                      size_t ws_bytes, void* stream);
/* Same, with plan flags (HHFM_PLAN_EXACT_FP32, _NO_SEED, _NO_RING,
 * _RING_ALT, _GEMM, _ONE_WAVE) and the optional id status word (query ids
 * are checked on the stream before scoring; the item range on the host). */
int hhfm_catalog_topk_ex(const int32_t* qidx, int64_t B, int32_t ncols,
                         int32_t mode, int32_t user_col, int32_t ctx_begin,
                         int32_t ctx_end, int32_t time_begin, int32_t time_end,
                         const void* E, int64_t features_M, int32_t k,
                         int32_t dtype, const float* w, int32_t item_row_begin,
                         int32_t item_count, int32_t global_item_base, int32_t K,
                         float* top_score, int32_t* top_idx, void* workspace,
                         size_t ws_bytes, int32_t plan, int32_t* status, void* stream);
/* Same, with `pooling` ("Pooling" above) for HHFM_MODE_HHFM: the query vector
 * h is the pooled one, everything after it (the MFMA kernels, the seed, the
 * ring, the merges) is unchanged.  HHFM_MODE_FM with pooling != 0 is
 * HHFM_EINVAL.  The workspace query and the plan rules are unchanged: a
 * small catalog takes the fused kernel (its POOL form: the same h in its
 * step 0) where the sum form takes it, and HHFM_PLAN_STORE / _FUSED / _GEMM
 * mean what they mean there. */
int hhfm_catalog_topk_pool(const int32_t* qidx, int64_t B, int32_t ncols,
                           int32_t mode, int32_t user_col, int32_t ctx_begin,
                           int32_t ctx_end, int32_t time_begin, int32_t time_end,
                           const void* E, int64_t features_M, int32_t k,
                           int32_t dtype, const float* w, int32_t item_row_begin,
                           int32_t item_count, int32_t global_item_base, int32_t K,
                           float* top_score, int32_t* top_idx, void* workspace,
                           size_t ws_bytes, int32_t plan, int32_t pooling,
                           int32_t* status, void* stream);
/* Same, two-way ("Two-way pooling" above; `pooling2` after `pooling`):
 * HHFM_MODE_HHFM only (HHFM_MODE_FM is HHFM_EINVAL).  The workspace query is
 * unchanged.  The query vector h is always formed by its own query kernel and
 * the main kernels (score matrix, seed, ring, merges) then run unchanged; the
 * small-catalog fused kernel is never taken — a two-way form of it is not
 * built — so HHFM_PLAN_FUSED has no effect here. */
int hhfm_catalog_topk_pool2(const int32_t* qidx, int64_t B, int32_t ncols,
                            int32_t mode, int32_t user_col, int32_t ctx_begin,
                            int32_t ctx_end, int32_t time_begin, int32_t time_end,
                            const void* E, int64_t features_M, int32_t k,
                            int32_t dtype, const float* w, int32_t item_row_begin,
                            int32_t item_count, int32_t global_item_base, int32_t K,
                            float* top_score, int32_t* top_idx, void* workspace,
                            size_t ws_bytes, int32_t plan, int32_t pooling,
                            int32_t pooling2, int32_t* status, void* stream);

/* ------------------------------------------------------------------------
 * Exclusion lists — catalog top-K over the items a query has not seen yet
 * (what evaluate_TopK's walk tries at FM.py:354-355, where it tests the target
 * instead of the prediction: SURVEY §8a-H3).  Pure additions: every earlier
 * entry point keeps its signature and behaviour, HHFM_ABI_VERSION stays 6.
 *
 * Lists (CSR over the B queries of one call, device memory):
 *   excl_ptr   int64 [B + 1], excl_ptr[0] = 0, non-decreasing;
 *   excl_rows  int32 [excl_ptr[B]]: TABLE ROW ids (rows of E: the ids the
 *              loader assigns and `codes` below stores in its low word),
 *              strictly ascending within a query.
 * The ids do not depend on the item shard: a row outside [item_row_begin,
 * item_row_begin + item_count) is ignored, and so is a negative or
 * >= features_M id — ids are compared, never used as an index.
 *
 * hhfm_catalog_topk_excl takes hhfm_catalog_topk_pool's arguments, then
 * excl_ptr, excl_rows, max_excl.  HHFM_MODE_FM with pooling 0 and
 * HHFM_MODE_HHFM with any pooling word.  The result is the top K of the
 * range's non-excluded items in the same (score desc, index asc) order, every
 * score bit for bit the plain call's score of that item; with every list empty
 * the output equals the plain call's.  max_excl is the caller's promise of the
 * longest list: K + max_excl > item_count (or max_excl < 0) is HHFM_EINVAL
 * before anything is launched, so no list can leave a range short of K items.
 * A list longer than max_excl may leave that query's output unspecified; the
 * kernels size and index nothing by max_excl.  excl_ptr NULL with B > 0 is
 * HHFM_EINVAL; excl_rows NULL means every list is empty.  The workspace is
 * hhfm_catalog_topk_workspace's, unchanged.
 * Routes: the score matrix (HHFM_PLAN_GEMM: from the GEMM)
 * with the excluded entries set to -FLT_MAX before the dense top-K, or the
 * streaming kernel's exclusion form behind a threshold seed without the tiles
 * that hold an excluded row.  The fused small-catalog kernel and the ring are
 * never taken: HHFM_PLAN_FUSED, _STORE, _NO_RING and _RING_ALT are accepted
 * without effect; _EXACT_FP32, _GEMM, _NO_SEED and _ONE_WAVE keep their meaning.
 *
 * The other models' catalogs take the same three arguments after their plain
 * call's, under the same rules (argument checks before anything is launched,
 * outputs untouched on an error; scores the plain call's bit for bit; empty
 * lists give the plain call's output; the plain call's workspace and its
 * contract: nothing read before the call writes it, the zero prefix left
 * zero).  The lists are indexed by the call's query number whatever the
 * call's query chunks (max_cols / chunk_rows):
 *   hhfm_cars2_catalog_topk_excl      hhfm_cars2_catalog_topk's arguments;
 *                                     the ids are rows of UI
 *   hhfm_afm_noatt_catalog_topk_excl  hhfm_afm_noatt_catalog_topk's
 *     — both on hhfm_catalog_topk_excl's routes behind their own query kernel;
 *   hhfm_afm_catalog_topk_excl        hhfm_afm_catalog_topk_ex's, on each of
 *                                     its three scoring routes
 *   hhfm_dfm_catalog_topk_excl        hhfm_dfm_catalog_topk_head's: the full,
 *                                     deep-only and FM-only heads
 *     — both write each query chunk's score block as the plain call does, set
 *     its listed entries to -FLT_MAX and run the plain dense top-K (the route
 *     of hhfm_catalog_topk_excl's score matrix; measured faster than the
 *     select below, DESIGN.md §K2 "Exclusion lists").
 * hhfm_topk_dense_excl is the dense top-K's own exclusion form on a caller's
 * matrix, which it reads and never writes: hhfm_topk_dense_ex's
 * arguments, then item_row_begin (column i is table row item_row_begin + i),
 * excl_ptr, excl_rows, max_excl.  The top K of each row's non-listed columns
 * in (score desc, index asc) order, every score the matrix element's own
 * bits; HHFM_PLAN_ONE_WAVE and the default four waves per query give the same
 * output bit for bit; max_excl < 0 or K + max_excl > N, and excl_ptr NULL
 * with B > 0, are HHFM_EINVAL.
 *
 * Not built: an exclusion form of the two-way catalog (hhfm_catalog_topk_pool2),
 * of the ring and of the fused kernel, and lists that run a range short of K
 * (DESIGN.md §7).
 *
 * hhfm_pf_exclusion_lists builds the lists of `rows` from positive_feedback's
 * device arrays (keys / codes as for hhfm_pf_contains below; in `codes` the
 * items of one key are one contiguous ascending run): row b's list is its
 * key's run, empty for an unknown key; keep_own != 0 leaves the row's own
 * item (column item_col) out, as a filtered evaluation must for its target.
 * Two calls:
 *   excl_rows == NULL  writes excl_ptr [B + 1] alone (per-row counts and their
 *                      exclusive scan, on the stream; needs the workspace of
 *                      hhfm_pf_exclusion_lists_workspace(B), a host-only query);
 *   excl_rows != NULL  fills the lists for the excl_ptr of the first call (same
 *                      arguments).  It reads excl_ptr[B] back (the stream is
 *                      synchronised): capacity < excl_ptr[B] is
 *                      HHFM_EWORKSPACE and nothing is written.
 * ---------------------------------------------------------------------- */
int hhfm_catalog_topk_excl(const int32_t* qidx, int64_t B, int32_t ncols,
                           int32_t mode, int32_t user_col, int32_t ctx_begin,
                           int32_t ctx_end, int32_t time_begin, int32_t time_end,
                           const void* E, int64_t features_M, int32_t k,
                           int32_t dtype, const float* w, int32_t item_row_begin,
                           int32_t item_count, int32_t global_item_base, int32_t K,
                           float* top_score, int32_t* top_idx, void* workspace,
                           size_t ws_bytes, int32_t plan, int32_t pooling,
                           int32_t* status, void* stream, const int64_t* excl_ptr,
                           const int32_t* excl_rows, int64_t max_excl);
int hhfm_cars2_catalog_topk_excl(const int32_t* q, int64_t B, const void* UI, int64_t n_ui,
                                 int32_t D, int32_t dtype, const void* prepared, int64_t Mc,
                                 int32_t item_row_begin, int32_t item_count,
                                 int32_t global_item_base, int32_t K, float* top_score,
                                 int32_t* top_idx, void* workspace, size_t ws_bytes,
                                 int32_t plan, int32_t* status, void* stream,
                                 const int64_t* excl_ptr, const int32_t* excl_rows,
                                 int64_t max_excl);
int hhfm_afm_noatt_catalog_topk_excl(const int32_t* qidx, int64_t B, int32_t F, const void* E,
                                     int64_t features_M, int32_t k, int32_t dtype,
                                     const float* w, float w0, const float* P,
                                     int32_t item_row_begin, int32_t item_count,
                                     int32_t global_item_base, int32_t K, float* top_score,
                                     int32_t* top_idx, void* workspace, size_t ws_bytes,
                                     int32_t plan, int32_t* status, void* stream,
                                     const int64_t* excl_ptr, const int32_t* excl_rows,
                                     int64_t max_excl);
int hhfm_afm_catalog_topk_excl(const int32_t* qidx, int64_t B, int32_t F, const void* E,
                               int64_t features_M, int32_t k, int32_t dtype, const float* w,
                               const float* Wt, const float* att_b, const float* att_p,
                               int32_t A, const float* P, int32_t item_row_begin,
                               int32_t item_count, int32_t global_item_base, int32_t K,
                               int64_t max_cols, float* top_score, int32_t* top_idx,
                               int32_t plan, void* workspace, size_t ws_bytes, void* stream,
                               const int64_t* excl_ptr, const int32_t* excl_rows,
                               int64_t max_excl);
int hhfm_dfm_catalog_topk_excl(const int32_t* qidx, int64_t B, int32_t F, int32_t item_col,
                               const void* E, int64_t features_M, int32_t k, int32_t dtype,
                               const float* w, int32_t nlayers, const int32_t* layer_dims,
                               const void* const* Wt, const float* const* bias,
                               int32_t mlp_dtype, const float* Wp, float bp,
                               int32_t item_row_begin, int32_t item_count,
                               int32_t global_item_base, int32_t K, int64_t chunk_rows,
                               float* top_score, int32_t* top_idx, int32_t proj_mode,
                               int32_t plan, void* workspace, size_t ws_bytes, void* stream,
                               int32_t head, const int64_t* excl_ptr, const int32_t* excl_rows,
                               int64_t max_excl);
int hhfm_topk_dense_excl(const float* scores, int64_t B, int32_t N, int64_t ld, int32_t K,
                         int32_t global_item_base, float* top_score, int32_t* top_idx,
                         int32_t plan, void* stream, int32_t item_row_begin,
                         const int64_t* excl_ptr, const int32_t* excl_rows, int64_t max_excl);
int hhfm_pf_exclusion_lists_workspace(int64_t B, size_t* ws_bytes);
int hhfm_pf_exclusion_lists(const int32_t* keys, int64_t nkeys, int32_t key_cols,
                            const int64_t* codes, int64_t ncodes, const int32_t* rows,
                            int64_t B, int32_t ncols, int32_t item_col, int32_t keep_own,
                            int64_t* excl_ptr, int32_t* excl_rows, int64_t capacity,
                            void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Top-K merge of R sorted partial lists per query (the item-sharded
 * multi-GPU path: RCCL all-gather output, rank-major).  Replaces the single
 * tf.nn.top_k over the full catalog (FM.py:185, OurModel7.py:295).
 *   in_score/in_idx: [R][B][K]; out_*: [B][K]; same (score desc, idx asc) order.
 *   K <= HHFM_TOPK_MAX_K ("Wide K": K > 64 merges in LDS, one workgroup per query).
 * hhfm_topk_merge_host is the same merge on host memory (no GPU needed).
 * ---------------------------------------------------------------------- */
int hhfm_topk_merge(const float* in_score, const int32_t* in_idx, int32_t R,
                    int64_t B, int32_t K, float* out_score, int32_t* out_idx,
                    void* stream);
int hhfm_topk_merge_host(const float* in_score, const int32_t* in_idx,
                         int32_t R, int64_t B, int32_t K, float* out_score,
                         int32_t* out_idx);

/* ------------------------------------------------------------------------
 * D1 — DeepFM per-row score (replaces `DeepFM.out`, DFM.py:104-137)
 *   y1 = w[x] (F), y2 = ½((Σe)² − Σe²) (k), h_0 = concat_f E[x_f] (F·k),
 *   h_{i+1} = relu(h_i · W_i + b_i) for every layer (ReLU after the last one
 *   too, DFM.py:128), out = [y1, y2, h_L] · Wp + bp.
 * Wt[i] are DEVICE pointers to the layer weights TRANSPOSED, [dims[i]][K_i]
 * with K_0 = F·k and K_i = dims[i-1] rounded up to a multiple of 8 (pad
 * columns zero), in mlp_dtype; bias[i] device float [dims[i]];
 * the Wt/bias/layer_dims arrays themselves are host arrays.  mlp_dtype
 * HHFM_F32 runs exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), HHFM_BF16 runs
 * bf16 MFMA with fp32 accumulation (activations rounded to bf16).
 * Wp: device float [F + k + dims[L-1]].  k must be a multiple of 4 (f32) /
 * 8 (bf16); layer widths are arbitrary.
 * ---------------------------------------------------------------------- */
int hhfm_dfm_forward_workspace(int64_t B, int32_t nlayers, const int32_t* layer_dims,
                               int32_t mlp_dtype, size_t* ws_bytes);

/* Projected layer 0 (ABI v3).  Layer 0 is linear before its ReLU, so
 * h_0 = Σ_f P_f[x_f] with P_f[id] = W0[:, f·k:(f+1)·k] · E[id]: the forward
 * computes P for every table row of the projected fields once per call (MFMA
 * GEMMs, the direct kernel's operand rounding, fp32 results) and the fused
 * kernel gathers it instead of streaming those fields' layer-0 weights — a
 * saving when rows >= 2·features_M (DFM.py:125-128 computed by the same
 * products, summed per field first).
 * The *_ex entry points take proj_mode explicitly; hhfm_dfm_forward /
 * hhfm_dfm_catalog_topk follow HHFM_DFM_PROJ_AUTO when ws_bytes covers that
 * plan (the *_workspace_ex size with HHFM_DFM_PROJ_AUTO) and run direct
 * otherwise.  The plan (direct, projected, which fields) changes the
 * summation order of layer 0, so scores may differ between plans within the
 * tested tolerances (fp32 MLP 2e-5, bf16 MLP 5e-3 of the output magnitude).
 * Projection needs the fused envelope (k % 16 == 0, k <= 512, F <= 16,
 * <= 4 layers of <= 416 units) and 16-B aligned Wt[i]; otherwise every mode
 * runs direct.
 * P needs (F - first projected field)·features_M·32·⌈max width/32⌉ floats
 * (at most 1 GiB planned). */
enum hhfm_dfm_proj {
  HHFM_DFM_PROJ_OFF = 0,  /* plan the direct path only                       */
  HHFM_DFM_PROJ_ON = 1,   /* project every field                             */
  HHFM_DFM_PROJ_AUTO = 2, /* below rows (B, or B·item_count) = 2·M: OFF;
                             fp32 MLP: ON; bf16 MLP: ITEM in the catalog,
                             ITEM in the forward from rows >= 64·M, CTX
                             below that                                      */
  HHFM_DFM_PROJ_CTX = 3,  /* bf16 MLP, F >= 3: project the context fields
                             2..F-1 (LoadData's layout: user, item,
                             contexts), fields 0 and 1 stay on MFMA; other
                             shapes run direct                               */
  HHFM_DFM_PROJ_ITEM = 4  /* bf16 MLP, F >= 2: project every field but the
                             item (field 1 of a forward row, item_col of a
                             catalog row), which stays on MFMA; the forward
                             processes its rows grouped by field 0 (a device
                             radix sort; scores land at the caller's row
                             positions); other shapes run direct             */
};
int hhfm_dfm_forward_workspace_ex(int64_t B, int32_t F, int32_t k, int64_t features_M,
                                  int32_t nlayers, const int32_t* layer_dims,
                                  int32_t mlp_dtype, int32_t proj_mode, size_t* ws_bytes);
int hhfm_dfm_forward(const int32_t* idx, int64_t B, int32_t F, const void* E,
                     int64_t features_M, int32_t k, int32_t dtype, const float* w,
                     int32_t nlayers, const int32_t* layer_dims, const void* const* Wt,
                     const float* const* bias, int32_t mlp_dtype, const float* Wp,
                     float bp, float* out, void* workspace, size_t ws_bytes,
                     void* stream);
/* Same, with the projection mode and the plan flags explicit (fp32 MLP:
 * HHFM_PLAN_EXACT_FP32 keeps the hidden layers on exact-fp32 MFMA, _ROW_FM,
 * _UNSTAGED, _UNGROUPED; bf16 MLP: _NARROW; the catalog also _ONE_WAVE);
 * ws_bytes must cover hhfm_dfm_forward_workspace_ex(..., proj_mode). */
int hhfm_dfm_forward_ex(const int32_t* idx, int64_t B, int32_t F, const void* E,
                        int64_t features_M, int32_t k, int32_t dtype, const float* w,
                        int32_t nlayers, const int32_t* layer_dims, const void* const* Wt,
                        const float* const* bias, int32_t mlp_dtype, const float* Wp,
                        float bp, float* out, int32_t proj_mode, int32_t plan,
                        void* workspace, size_t ws_bytes, void* stream);

/* D2 — DeepFM.topk (DFM.py:219-231): every query row is tiled over the
 * catalog with column item_col replaced by each item id, scored by D1 and
 * top-K selected; at most chunk_rows (query x item) rows per pass. */
int hhfm_dfm_catalog_topk_workspace(int64_t B, int32_t F, int32_t item_count,
                                    int32_t nlayers, const int32_t* layer_dims,
                                    int32_t mlp_dtype, int64_t chunk_rows,
                                    size_t* ws_bytes);
int hhfm_dfm_catalog_topk_workspace_ex(int64_t B, int32_t F, int32_t k,
                                       int64_t features_M, int32_t item_count,
                                       int32_t nlayers, const int32_t* layer_dims,
                                       int32_t mlp_dtype, int64_t chunk_rows,
                                       int32_t proj_mode, size_t* ws_bytes);
int hhfm_dfm_catalog_topk(const int32_t* qidx, int64_t B, int32_t F, int32_t item_col,
                          const void* E, int64_t features_M, int32_t k, int32_t dtype,
                          const float* w, int32_t nlayers, const int32_t* layer_dims,
                          const void* const* Wt, const float* const* bias,
                          int32_t mlp_dtype, const float* Wp, float bp,
                          int32_t item_row_begin, int32_t item_count,
                          int32_t global_item_base, int32_t K, int64_t chunk_rows,
                          float* top_score, int32_t* top_idx, void* workspace,
                          size_t ws_bytes, void* stream);
/* Same, with the projection mode and plan flags explicit (see
 * hhfm_dfm_forward_ex). */
int hhfm_dfm_catalog_topk_ex(const int32_t* qidx, int64_t B, int32_t F, int32_t item_col,
                             const void* E, int64_t features_M, int32_t k, int32_t dtype,
                             const float* w, int32_t nlayers, const int32_t* layer_dims,
                             const void* const* Wt, const float* const* bias,
                             int32_t mlp_dtype, const float* Wp, float bp,
                             int32_t item_row_begin, int32_t item_count,
                             int32_t global_item_base, int32_t K, int64_t chunk_rows,
                             float* top_score, int32_t* top_idx, int32_t proj_mode,
                             int32_t plan, void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * A1 — AFM per-row score (replaces `AFM.out`, AFM.py:103-142), attention on,
 * keep = [1,1]: pairs i<j of the F fields, logit = Σ_a p_a·relu(((e_i⊙e_j)·W)_a
 * + b_a), att = softmax over pairs, out = (Σ att·(e_i⊙e_j))·P + Σ w + w0.
 * Wt: device float [A][k] = attention_W TRANSPOSED; att_b [A], att_p [A],
 * P [k] (the prediction vector).  F <= 16, k % 4 == 0.
 * ---------------------------------------------------------------------- */
int hhfm_afm_forward_workspace(int64_t B, int32_t F, int32_t A, size_t* ws_bytes);
int hhfm_afm_forward(const int32_t* idx, int64_t B, int32_t F, const void* E,
                     int64_t features_M, int32_t k, int32_t dtype, const float* w, float w0,
                     const float* Wt, const float* att_b, const float* att_p, int32_t A,
                     const float* P, float* out, void* workspace, size_t ws_bytes,
                     void* stream);
/* Same, with plan flags: HHFM_PLAN_EXACT_FP32 runs the attention contraction
 * on exact-fp32 MFMA instead of split-bf16 (k % 16 == 0 shapes). */
int hhfm_afm_forward_ex(const int32_t* idx, int64_t B, int32_t F, const void* E,
                        int64_t features_M, int32_t k, int32_t dtype, const float* w,
                        float w0, const float* Wt, const float* att_b, const float* att_p,
                        int32_t A, const float* P, float* out, int32_t plan,
                        void* workspace, size_t ws_bytes, void* stream);

/* A2 — AFM.topk (AFM.py:209-246): uf = [E[col 0], E[cols 2..F-1]], exp-weighted
 * pair attention over uf pairs and uf x item pairs (raw exp, as the
 * reference), score = (Σ_c P_c·score1_c) / weight + w_item, then top-K.
 * At most max_cols = (queries per pass)·(F-1)·A GEMM columns per pass.
 * k <= 256, k % 4 == 0, A % 16 == 0 (or inside the fused envelope), F <= 16. */
int hhfm_afm_catalog_topk_workspace(int64_t B, int32_t F, int32_t k, int32_t A,
                                    int32_t item_count, int64_t max_cols,
                                    size_t* ws_bytes);
int hhfm_afm_catalog_topk(const int32_t* qidx, int64_t B, int32_t F, const void* E,
                          int64_t features_M, int32_t k, int32_t dtype, const float* w,
                          const float* Wt, const float* att_b, const float* att_p,
                          int32_t A, const float* P, int32_t item_row_begin,
                          int32_t item_count, int32_t global_item_base, int32_t K,
                          int64_t max_cols, float* top_score, int32_t* top_idx,
                          void* workspace, size_t ws_bytes, void* stream);
/* Same, with plan flags: HHFM_PLAN_EXACT_FP32, _PER_FIELD, _GEMM (the
 * workspace for _GEMM is hhfm_afm_catalog_topk_workspace_ex's). */
int hhfm_afm_catalog_topk_workspace_ex(int64_t B, int32_t F, int32_t k, int32_t A,
                                       int32_t item_count, int64_t max_cols, int32_t plan,
                                       size_t* ws_bytes);
int hhfm_afm_catalog_topk_ex(const int32_t* qidx, int64_t B, int32_t F, const void* E,
                             int64_t features_M, int32_t k, int32_t dtype, const float* w,
                             const float* Wt, const float* att_b, const float* att_p,
                             int32_t A, const float* P, int32_t item_row_begin,
                             int32_t item_count, int32_t global_item_base, int32_t K,
                             int64_t max_cols, float* top_score, int32_t* top_idx,
                             int32_t plan, void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * AFM without attention — the reference's `--attention 0` (AFM.py:103-148
 * with self.attention false; the AFM paper's ablation).  The model has four
 * variables: the table E, w, w0 and the prediction vector P [k].  For a row
 * of F ids x_0..x_{F-1}, e_f = E[x_f]:
 *   x_c  = Σ_{i<j} e_i,c·e_j,c = ½[(Σ_f e_f,c)² − Σ_f e_f,c²]
 *   d_c  = x_c / keep_afm · bin_c        tf.nn.dropout on the k-vector (AFM.py:134)
 *   out  = Σ_c d_c·P_c + Σ_f w[x_f] + w0
 *   loss = Σ_b (y_b − out_b)²/2          no regulariser, whatever lamda_attention
 *                                        is (AFM.py:148)
 * keep[0] (the attention's) has no site in this model.
 *
 * Row scores need no entry point of their own: hhfm_fm_score_rows_scaled with
 * scale = P is `out` at keep = 1, for fp32 and bf16 tables.
 *
 * Catalog score.  The reference's topk raises KeyError('attention_W') here,
 * so this is THIS LIBRARY'S definition: the score of item i for query row b
 * is `out` (keep = 1) of the row with column 1 replaced by the item's table
 * row — as with attention on, where the reference's topk ranks by `out`.
 * Column 1 of the query is ignored, as in AFM.topk.
 *   q_b   = Σ_{f≠1} E[x_bf]
 *   score = (P ⊙ q_b)·E[i] + w[i] + cst_b
 *   cst_b = Σ_c P_c·½(q_bc² − Σ_{f≠1} e_bf,c²) + Σ_{f≠1} w[x_bf] + w0
 * top_score is that full value (not up to a per-query constant): it can be
 * compared with the row score of the same row.  hhfm_afm_noatt_catalog_topk
 * forms H = P ⊙ q and cst in a query kernel of its own and runs
 * hhfm_catalog_topk_ex's plans on them (HHFM_MODE_FM's form: H·E[i] + w[i] +
 * cst): the same workspace (hhfm_catalog_topk_workspace), item range
 * arguments, K in [1, 64], plan flags, zero-prefix contract and status word
 * (the ids of every query column but column 1), and the same k limits (fp32
 * k in {8, .., 128}, bf16 k in {16, .., 256}, powers of two).  The
 * small-catalog fused kernel is never taken (HHFM_PLAN_FUSED is accepted and
 * falls through to the score-matrix path).  F >= 2; w may be NULL.
 *
 * Training.  hhfm_afm_noatt_train_step is one TF step on E, w, w0 and P; acc
 * = slots of {E, w, w0, P} in that order (NULL under SGD).  No variable
 * carries an l2 term, so E and w follow the IndexedSlices rules of "optimizer"
 * below (sparse Momentum touches the batch's rows only, sparse Adam decays
 * every row), w0 and P are dense.  With g_b = out_b − y_b, m_bc = bin_bc /
 * keep_afm and s_bc = Σ_f e_bf,c:
 *   dP_c = Σ_b g_b·x_bc·m_bc      dE[x_bf][c] += g_b·P_c·m_bc·(s_bc − e_bf,c)
 *   dw[x_bf] += g_b               dw0 = Σ_b g_b
 * The mask is "Training dropout"'s site 2 (n = k, r = the batch row) under the
 * step's seed — AFM's own site, so keep_afm = 1 draws nothing.  dP is summed
 * in fp32 inside a workgroup and in double across workgroups; the loss in
 * double.  B = 0 is a step like any other: no row is touched, Adam's moments
 * and powers advance, the loss is 0, idx / y may be NULL.
 * Envelope: F >= 1, 1 <= k <= 256.  k > 256 is HHFM_EUNSUPPORTED, as is an
 * unknown optimizer; F < 1, k < 1, B < 0, features_M < 1, a keep_afm that is
 * NaN or outside (0, 1], a NULL parameter / loss / workspace, missing slots
 * and a workspace not 8-byte aligned are HHFM_EINVAL, a short workspace
 * HHFM_EWORKSPACE — all before any launch.  The workspace
 * (hhfm_afm_noatt_train_workspace bytes: hhfm_train_workspace's layout, then
 * dP [k] and its double sums) is zero-filled once and left zeroed but Adam's
 * β powers; it does not depend on B.
 *
 * hhfm_afm_noatt_train_step_det: the same step under the promise of
 * "Deterministic training steps" below, no float atomic:
 *   dE[id][c], dw[id]   an occurrence is o = b·F + f (FM's order); its
 *       contribution is gc·(S_b[c] − e) with gc = g_b·P_c (· bin / keep), to
 *       dw[id] it is g_b; a dropped column adds nothing.  Each element is the
 *       fp32 sum of the id's contributions in ascending o, started from the
 *       first one.
 *   dP[c]   the rows' values v_bc = g_b·(x_bc / keep · bin_bc) in the scalar
 *       order: 256 partials, partial t = rows t, t + 256, ... ascending from
 *       0, then the partials in ascending t from 0, all in fp32.
 *   dw0, the loss   the scalar order on g_b (float) and g_b²/2 formed in
 *       double, rounded to float once.  There is no Σ var².
 * Every product above is rounded on its own (no fused multiply-add).
 * `scratch` (hhfm_afm_noatt_train_det_scratch bytes, for that B or any smaller
 * one) carries no state and need not be zeroed; the query runs on the host.
 * The default step's checks come first, in their order; then a NULL scratch is
 * HHFM_EINVAL and a too small one HHFM_EWORKSPACE (also at B = 0), and
 * hipCUB's real temporary-storage figure is checked, before anything is
 * launched: a refusal leaves every parameter, slot and the workspace
 * untouched.  (numpy restatement: tests/train_det_noatt_ref.py.)
 * ---------------------------------------------------------------------- */
int hhfm_afm_noatt_catalog_topk(const int32_t* qidx, int64_t B, int32_t F, const void* E,
                                int64_t features_M, int32_t k, int32_t dtype, const float* w,
                                float w0, const float* P, int32_t item_row_begin,
                                int32_t item_count, int32_t global_item_base, int32_t K,
                                float* top_score, int32_t* top_idx, void* workspace,
                                size_t ws_bytes, int32_t plan, int32_t* status, void* stream);
int hhfm_afm_noatt_train_workspace(int64_t features_M, int32_t k, size_t* ws_bytes);
int hhfm_afm_noatt_train_step(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                              float* w, float* w0, float* P, int64_t features_M, int32_t k,
                              float lr, int32_t optimizer, float keep_afm, uint64_t seed,
                              float* const* acc, void* workspace, size_t ws_bytes, float* loss,
                              void* stream);
int hhfm_afm_noatt_train_det_scratch(int64_t B, int32_t F, int32_t k, int64_t features_M,
                                     size_t* bytes);
int hhfm_afm_noatt_train_step_det(const int32_t* idx, const float* y, int64_t B, int32_t F,
                                  float* E, float* w, float* w0, float* P, int64_t features_M,
                                  int32_t k, float lr, int32_t optimizer, float keep_afm,
                                  uint64_t seed, float* const* acc, void* workspace,
                                  size_t ws_bytes, void* scratch, size_t scratch_bytes,
                                  float* loss, void* stream);

/* ------------------------------------------------------------------------
 * H6 — one training step (`partial_fit`, sess.run((loss, optimizer))).
 *   FM   (FM.py:123-136):        loss = Σ (y − out)²/2 + λ·Σ E²/2
 *   HHFM (OurModel7.py:172-193): loss = −Σ log σ(pos − max_j neg_j) + λ·Σ E²/2
 * optimizer (enum hhfm_optimizer below; TF-1.x semantics, FM.py:129-136; `acc`
 * slots per variable):
 *   HHFM_OPT_ADAGRAD   AdagradOptimizer  accum += g², var -= lr·g·rsqrt(accum);
 *       n floats initialised to 0.1 (TF's initial_accumulator_value);
 *   HHFM_OPT_SGD       GradientDescentOptimizer (no slots);
 *   HHFM_OPT_MOMENTUM  MomentumOptimizer(momentum = 0.95)  accum = accum·0.95 + g,
 *       var -= accum·lr; n floats initialised to 0;
 *   HHFM_OPT_ADAM      AdamOptimizer(β1 0.9, β2 0.999, ε 1e-8)  2n floats (m,
 *       then v) initialised to 0; β1^t, β2^t and a started flag live in the
 *       workspace (zero-filled once = step 1; a power that underflows to 0
 *       stays 0, as TF's does).
 * Variables whose TF gradient is an IndexedSlices (an embedding_lookup with
 * no dense l2 term on the same variable: w of FM; the table of FM / HHFM at
 * λ = 0, of DeepFM and of AFM; w of DeepFM and AFM) follow TF's sparse
 * rules: Momentum updates only the rows the batch touched, Adam decays m
 * and v of every row (AdamOptimizer._apply_sparse_shared).
 * E, w are fp32 and updated in place; *loss (device float) receives the loss
 * of the pre-update parameters.  The workspace (hhfm_train_workspace bytes:
 * gradient buffers, 16 scalars, the touched-row mask; the layout is
 * fm_train_plan's in train.hip) must be zero-filled once; the step leaves it
 * zeroed except Adam's β powers.  HHFM: X [B][ncols] full rows [user, item,
 * ctx..., time...], Neg [B][NG] negative item ids, NG <= 16.
 * B = 0 is a step like any other in all four train entry points (the l2
 * term still decays its variable, Adam's moments and powers still advance);
 * the row pointers (idx / X, y / Neg) may then be NULL.
 * ---------------------------------------------------------------------- */
enum hhfm_optimizer {
  HHFM_OPT_ADAGRAD = 0,
  HHFM_OPT_SGD = 1,
  HHFM_OPT_MOMENTUM = 2,
  HHFM_OPT_ADAM = 3
};

size_t hhfm_train_workspace(int64_t features_M, int32_t k);
int hhfm_fm_train_step(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                       float* w, float* w0, int64_t features_M, int32_t k, float lr,
                       float lambda_l2, int32_t optimizer, float* accE, float* accw,
                       float* accw0, void* workspace, size_t ws_bytes, float* loss,
                       void* stream);
int hhfm_hhfm_train_step(const int32_t* X, const int32_t* Neg, int64_t B, int32_t ncols,
                         int32_t ctx_begin, int32_t ctx_end, int32_t time_begin,
                         int32_t time_end, int32_t NG, float* E, int64_t features_M,
                         int32_t k, float lr, float lambda_l2, int32_t optimizer, float* accE,
                         void* workspace, size_t ws_bytes, float* loss, void* stream);
/* hhfm_hhfm_train_step with `pooling` ("Pooling" above): the forward's h is
 * the pooled one and the backward follows TF's gradients — reduce_max sends
 * dh_e, divided by the number of values equal to the maximum at element e, to
 * each of those values (context rows, time rows and stack members alike),
 * reduce_mean divides by the count.  The BPR part, the optimizer, the l2 term,
 * the loss and the workspace (hhfm_train_workspace) are hhfm_hhfm_train_step's;
 * pooling == 0 is that step itself. */
int hhfm_hhfm_train_step_pool(const int32_t* X, const int32_t* Neg, int64_t B, int32_t ncols,
                              int32_t ctx_begin, int32_t ctx_end, int32_t time_begin,
                              int32_t time_end, int32_t NG, float* E, int64_t features_M,
                              int32_t k, float lr, float lambda_l2, int32_t optimizer,
                              float* accE, void* workspace, size_t ws_bytes, int32_t pooling,
                              float* loss, void* stream);
/* The two-way step ("Two-way pooling" above; `pooling2` after `pooling`): the
 * forward's h is the two-way one, the backward sends dh_e through H1 and H2
 * to the stack members and each mix's gradient through P1 and every pair
 * product to the rows.  Same workspace, BPR part, optimizer tail and loss;
 * fp32 tables, not deterministic. */
int hhfm_hhfm_train_step_pool2(const int32_t* X, const int32_t* Neg, int64_t B, int32_t ncols,
                               int32_t ctx_begin, int32_t ctx_end, int32_t time_begin,
                               int32_t time_end, int32_t NG, float* E, int64_t features_M,
                               int32_t k, float lr, float lambda_l2, int32_t optimizer,
                               float* accE, void* workspace, size_t ws_bytes, int32_t pooling,
                               int32_t pooling2, float* loss, void* stream);

/* Training dropout (`--keep` < 1 of FM.py:42-43, AFM.py:43-44).  The
 * arithmetic and the gradient are tf.nn.dropout's (TF 1.x):
 *   binary = floor(keep + uniform[0,1)),  y = x / keep · binary
 * one mask per step, shared by its forward and backward pass; *loss is the
 * loss of the dropped forward.  The mask is NOT TensorFlow's (its Philox
 * stream is keyed by the graph seed and an op counter) but this library's,
 * specified bit for bit: Philox4x32-10 keyed by the caller's 64-bit per-step
 * `seed` (low word, high word); element e of row r at site s reads word
 * (e >> 6) & 3 of the block with counter
 *   ((e & 63) | ((e >> 8) << 6),  r & 0xffffffff,  r >> 32,  s)
 * as u = float(x >> 9) · 2^-23 and binary = floorf(keep + u) in fp32.  Sites:
 * 0 FM's k-vector FM_OUT (FM.py:114, n = k); 1 AFM's softmaxed attention
 * (AFM.py:126, n = F(F−1)/2 pairs in i < j order); 2 AFM's k-vector
 * (AFM.py:134, n = k).  r is the batch row.  (csrc/dropout.h; numpy
 * restatement in tests/dropout_ref.py.)
 * hhfm_fm_train_step_ex / hhfm_afm_train_step_ex are the steps above with
 * that dropout; keep = 1 is exactly the plain step (hhfm_fm_train_step and
 * hhfm_afm_train_step forward here with keep 1), and a keep that is NaN or
 * outside (0, 1] is HHFM_EINVAL before anything is launched.  Workspaces are
 * the plain steps'.  hhfm_dropout_mask writes the decisions themselves,
 * binary [rows][n] floats 0 / 1 (rows = 0 is a no-op). */
int hhfm_fm_train_step_ex(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                          float* w, float* w0, int64_t features_M, int32_t k, float lr,
                          float lambda_l2, int32_t optimizer, float keep, uint64_t seed,
                          float* accE, float* accw, float* accw0, void* workspace,
                          size_t ws_bytes, float* loss, void* stream);
int hhfm_dropout_mask(uint64_t seed, int32_t site, int64_t rows, int32_t n, float keep,
                      float* binary, void* stream);

/* FM batch norm (`--batch_norm 1` of FM.py:50, :111-112, :160-166).  A
 * restatement — TensorFlow is not available, TF-level parity is unpinned —
 * of tf.contrib.layers.batch_norm(x, decay=0.9, center=True, scale=True,
 * updates_collections=None) on x = FM of shape [B, 1, k], which takes the
 * non-fused path (rank 3): tf.nn.moments over axes [0, 1],
 * tf.nn.batch_normalization, assign_moving_average with zero_debias=False.
 * Variables, all float [k]: gamma (initial 1), beta (0), moving_mean (0),
 * moving_var (1).  eps is the contrib default 0.001 and bn_update =
 * float(1.0 − decay), the complement formed in double by the caller as TF
 * forms it in Python; both are arguments.
 *
 * Training forward, per column c over the rows b = 0..B−1:
 *   x_bc  = ½(s_bc² − q_bc)                   s, q as in hhfm_fm_train_step
 *   μ_c   = (Σ_b x_bc) / B
 *   v_c   = (Σ_b (x_bc − μ_c)²) / B           biased, two-pass; never Σx² − Bμ²
 *   inv_c = 1 / sqrtf(v_c + eps)              IEEE sqrt, one correctly rounded division
 *   a_c   = inv_c · γ_c
 *   y_bc  = x_bc · a_c + (β_c − μ_c · a_c)    tf.nn.batch_normalization's form
 *   FM_OUT_bc = y_bc / keep · bin_bc          dropout site 0, after the layer
 *   out_b = Σ_c FM_OUT_bc + Σ_f w[x_bf] + w0
 *   loss  = Σ_b (y_b − out_b)²/2 + λ·Σ E²/2
 * Backward, g_b = out_b − y_b, dy_bc = g_b · bin_bc / keep, x̂_bc = (x_bc − μ_c)·inv_c:
 *   dβ_c = Σ_b dy_bc        dγ_c = Σ_b dy_bc · x̂_bc
 *   dx_bc = (a_c / B) · (B·dy_bc − dβ_c − x̂_bc · dγ_c)
 *   dE[x_bf][c] += dx_bc · (s_bc − e_bfc)     dw, dw0 as in hhfm_fm_train_step
 * After the forward, whatever the optimizer:
 *   mm_c −= (mm_c − μ_c)·bn_update            mv_c −= (mv_c − v_c)·bn_update
 * The optimizer acts on E (λ; dense when λ > 0, IndexedSlices when λ = 0), w
 * (sparse), w0, and on γ and β: dense, no l2 term, the usual slots.  The
 * moving statistics are not optimizer variables.
 * Every batch sum (Σx, Σ(x−μ)², dβ, dγ, Σg, the loss at every keep) is added in
 * fp32 inside a workgroup and in double across workgroups, and rounded once.
 *
 * Inference (hhfm_fm_score_rows_scaled): the same y with mm, mv in place of
 * μ, v and no dropout,
 *   out_b = (Σ_c a_c·x_bc + Σ_f w) + w0',  a_c = γ_c / sqrtf(mv_c + eps),
 *   w0' = w0 + Σ_c (β_c − mm_c·a_c)
 * with a and w0' formed by the caller.  Scoring never writes a weight.
 *
 * hhfm_fm_train_step_bn is hhfm_fm_train_step_ex with the layer.  Checks: the
 * plain step's first, in their order; then B = 0 (TF's moments of an empty
 * batch are NaN), eps not > 0 or NaN, bn_update outside [0, 1], a NULL gamma /
 * beta / moving_mean / moving_var, a NULL acc_gamma / acc_beta unless SGD, a
 * workspace that is not 8-byte aligned: HHFM_EINVAL, nothing launched.
 * Workspace: hhfm_fm_train_bn_workspace(B, ...) bytes, zero-filled once.  Its
 * first hhfm_fm_train_bn_state_bytes() bytes are the persistent part
 * (hhfm_train_workspace's layout, then the gradients of γ and β), left zeroed
 * by the step but for Adam's β powers; the rest is per-batch scratch that
 * carries no state, so a workspace grown for a larger batch keeps its state
 * by copying that prefix.  hhfm_fm_train_bn_workspace is HHFM_EINVAL for
 * B < 0, features_M < 1, k < 1 or a NULL ws_bytes and runs on the host;
 * hhfm_fm_train_bn_state_bytes is 0 for such sizes. */
int hhfm_fm_train_bn_workspace(int64_t B, int64_t features_M, int32_t k, size_t* ws_bytes);
size_t hhfm_fm_train_bn_state_bytes(int64_t features_M, int32_t k);
int hhfm_fm_train_step_bn(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                          float* w, float* w0, int64_t features_M, int32_t k, float lr,
                          float lambda_l2, int32_t optimizer, float keep, uint64_t seed,
                          float* accE, float* accw, float* accw0, void* workspace,
                          size_t ws_bytes, float* gamma, float* beta, float* moving_mean,
                          float* moving_var, float eps, float bn_update, float* acc_gamma,
                          float* acc_beta, float* loss, void* stream);

/* Deterministic training steps (opt-in; FM and HHFM here, AFM and DeepFM
 * after their default steps below).  The steps above add
 * their gradients with float atomics, whose order changes from run to run.
 * hhfm_fm_train_step_det / hhfm_hhfm_train_step_det are hhfm_fm_train_step_ex /
 * hhfm_hhfm_train_step with no float atomic: the order of every sum is a
 * function of the batch alone.
 *
 * The contribution of one occurrence of an id in the batch is the value the
 * default step adds atomically, formed from the same expressions in the same
 * order (s = Σ_f E[x_f][c] in field order, g·(s − e), g·h, −gt·h,
 * dh = g·it − gt·nsum); only the order in which contributions meet differs:
 *   dE[id][c], dw[id]   the fp32 sum of the id's contributions in ascending
 *       occurrence index o = b·S + slot, started from the first one.
 *       FM: S = F, slot = the field.  HHFM: S = 2 + NG + ctx columns + time
 *       columns, slots in the order item, negatives 0..NG-1, user, context
 *       columns ascending, time columns ascending.  Only tied maxima
 *       contribute (an untied negative adds nothing); a column that FM's
 *       dropout drops adds nothing; ids are clamped to row 0 as always.
 *   w0's gradient, the data loss   per-row values g_b (float) and loss_b
 *       (double; FM r²/2 formed in double, HHFM −logf(σ) widened): 256
 *       partials, partial t = rows t, t + 256, ... added in ascending order
 *       from 0, then the 256 partials in ascending t from 0; the loss is
 *       rounded to float once.
 *   Σ var² of the l2 term   the optimizer's grid is a function of the
 *       variable's size alone; every wave's partial is stored at its global
 *       wave index and the partials are added in ascending index in double,
 *       rounded to float once.
 * Promised: with the same build, the same device model, the same inputs, the
 * same initial parameters and slots and the same seed, the parameters, slots
 * and *loss are the same bits — in the same process or a fresh one, on any
 * stream.  NOT promised: equal bits to the default steps, to TensorFlow, or
 * across builds.  (numpy restatement of the orders: tests/train_det_ref.py.)
 *
 * `scratch` holds hhfm_train_det_scratch(B, occ_per_row, k, features_M) bytes
 * for batches of exactly that shape or any smaller B (occ_per_row = F for FM,
 * the S above for HHFM): sort keys and values, hipCUB's temporary storage,
 * the run starts, the per-row vectors and scalars, the Σvar² partials.  It
 * carries no state between steps and need not be zeroed; the size query runs
 * on the host and needs no device, and is HHFM_EINVAL when B·occ_per_row does
 * not fit an int.  The workspace is the default steps' (hhfm_train_workspace),
 * same layout, still left zeroed.  The default steps' argument checks come
 * first, in their order; then a NULL or too small scratch is HHFM_EINVAL
 * before anything is launched (also at B = 0, whose Σvar² partials live
 * there). */
int hhfm_train_det_scratch(int64_t B, int32_t occ_per_row, int32_t k, int64_t features_M,
                           size_t* bytes);
int hhfm_fm_train_step_det(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                           float* w, float* w0, int64_t features_M, int32_t k, float lr,
                           float lambda_l2, int32_t optimizer, float keep, uint64_t seed,
                           float* accE, float* accw, float* accw0, void* workspace,
                           size_t ws_bytes, void* scratch, size_t scratch_bytes, float* loss,
                           void* stream);
int hhfm_hhfm_train_step_det(const int32_t* X, const int32_t* Neg, int64_t B, int32_t ncols,
                             int32_t ctx_begin, int32_t ctx_end, int32_t time_begin,
                             int32_t time_end, int32_t NG, float* E, int64_t features_M,
                             int32_t k, float lr, float lambda_l2, int32_t optimizer,
                             float* accE, void* workspace, size_t ws_bytes, void* scratch,
                             size_t scratch_bytes, float* loss, void* stream);

/* DeepFM (DFM.py:139-155, 214-217; use_fm = use_deep = True, loss "mse"):
 *   loss = Σ (y − out)²/2 + λ·(‖Wp‖² + Σ_l ‖W_l‖²)/2
 * one step of the optimizer (codes as above) on every variable, in place.
 * W[l] is layer l row-major [d_{l-1}][d_l] (d_{-1} = F·k), bias[l] [d_l], Wp
 * the concat projection [F + k + d_{L-1}], bp a device float.  acc (every
 * optimizer but HHFM_OPT_SGD): 2L+4 device slot arrays in the order E, w, W_0..W_{L-1},
 * b_0..b_{L-1}, Wp, bp, sized and initialised as above.
 * The workspace (hhfm_dfm_train_workspace bytes for batches of at most B rows)
 * must be zero-filled once; the step keeps its gradient regions zeroed.  Its
 * persistent part (every gradient the step accumulates into, Adam's β
 * powers, the touched-row mask; the layout is TrainWs's in train.hip) leads at
 * offsets independent of B, so a later smaller batch finds it where the last
 * step left it, and a workspace grown for a larger batch keeps the state when
 * that prefix (hhfm_dfm_train_state_bytes) is copied into the new zero-filled
 * one.
 * Requires k % 4 == 0, L <= 4, F + k + d_{L-1} <= 1024. */
int hhfm_dfm_train_workspace(int64_t B, int32_t F, int32_t k, int64_t features_M,
                             int32_t nlayers, const int32_t* layer_dims, size_t* ws_bytes);
/* The size of that persistent prefix (ABI v5): copy exactly these bytes of an
 * old workspace into a new zero-filled one; everything after it is per-batch
 * scratch. */
int hhfm_dfm_train_state_bytes(int32_t F, int32_t k, int64_t features_M, int32_t nlayers,
                               const int32_t* layer_dims, size_t* state_bytes);
int hhfm_dfm_train_step(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                        float* w, int64_t features_M, int32_t k, int32_t nlayers,
                        const int32_t* layer_dims, float* const* W, float* const* bias,
                        float* Wp, float* bp, float lr, float lambda_l2, int32_t optimizer,
                        float* const* acc, void* workspace, size_t ws_bytes, float* loss,
                        void* stream);

/* AFM (AFM.py:103-156, 205-207; attention = 1; keep = [1, 1], or
 * [keep_att, keep_afm] through hhfm_afm_train_step_ex — "Training dropout"
 * above: keep_att on the softmaxed attention, keep_afm on the k-vector):
 *   loss = Σ (y − out)²/2 + λ·‖attention_W‖²/2
 * one step of the optimizer (codes as above) on every variable, in place:
 * E [M][k], w [M], w0 (device float), W = attention_W [k][A] row-major,
 * b = attention_b [A], pvec = attention_p [A], P = prediction [k].  acc
 * (every optimizer but HHFM_OPT_SGD): 7 device slot arrays in the order E, w, w0, W, b,
 * pvec, P, sized and initialised as above.  The workspace
 * (hhfm_afm_train_workspace bytes for batches of at most B rows) must be
 * zero-filled once; the step keeps its gradient regions zeroed; grown as for
 * DeepFM (the hhfm_afm_train_state_bytes prefix copied into the new one).
 * Requires 2 <= F <= 16, k and A multiples of 4 and <= 256.  Replaces
 * sess.run((loss, optimizer)) of AFM.partial_fit (AFM.py:205-207). */
int hhfm_afm_train_workspace(int64_t B, int32_t F, int32_t k, int32_t A,
                             int64_t features_M, size_t* ws_bytes);
int hhfm_afm_train_state_bytes(int32_t F, int32_t k, int32_t A, int64_t features_M,
                               size_t* state_bytes);
int hhfm_afm_train_step(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                        float* w, float* w0, int64_t features_M, int32_t k, int32_t A,
                        float* W, float* b, float* pvec, float* P, float lr,
                        float lambda_att, int32_t optimizer, float* const* acc,
                        void* workspace, size_t ws_bytes, float* loss, void* stream);
int hhfm_afm_train_step_ex(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                           float* w, float* w0, int64_t features_M, int32_t k, int32_t A,
                           float* W, float* b, float* pvec, float* P, float lr,
                           float lambda_att, int32_t optimizer, float keep_att, float keep_afm,
                           uint64_t seed, float* const* acc, void* workspace, size_t ws_bytes,
                           float* loss, void* stream);

/* Deterministic AFM and DeepFM steps (opt-in), under the promise of
 * "Deterministic training steps" above: hhfm_afm_train_step_det is
 * hhfm_afm_train_step_ex (dropout included: the masks are a function of
 * (seed, row, element)) and hhfm_dfm_train_step_det is hhfm_dfm_train_step,
 * with no float atomic.  The GEMMs, AFM's split-order dW and DeepFM's db were
 * order-fixed already; what changes is where contributions meet:
 *   dE[id][c], dw[id]   an occurrence is o = b·F + f (FM's order).  Its
 *       contribution to dE[id][c] is the value the default step hands to its
 *       atomic add, from the same expressions in the same order — AFM:
 *       de[f] = Σ_{pairs ∋ f} fma(fma(ã_p, g·P_c(·m2_c), DP[p][c]), e_other, ·)
 *       in pair order i < j; DeepFM: dX0[b][f·k+c] + (g·Wp[F+c])·(s − e) — and
 *       to dw[id] it is g_b (AFM) or g_b·Wp[f] (DeepFM).  Each is the fp32 sum
 *       of the id's contributions in ascending o, started from the first one.
 *       A dropped AFM column still contributes its DP term.
 *   AFM dP[k], dp[A], db[A]; DeepFM dWp[F+k+d_L]   a row's value for an element
 *       is what the default kernel's accumulator holds after that row alone,
 *       from zero (the same fmaf chain over the row's pairs / columns).  The
 *       element is the sum of the rows' values in the scalar order above: 256
 *       partials, partial t = rows t, t + 256, ... ascending from 0, then the
 *       partials in ascending t from 0, all in fp32.  The head kernel's grid
 *       does not enter.
 *   w0's / bp's gradient, the data loss   the scalar order above on g_b
 *       (float) and g_b²/2 formed in double, rounded to float once.
 *   Σ var²   as above, over attention_W (AFM) or every layer weight and the
 *       concat projection in the optimizer's variable order W_0.., Wp (DeepFM).
 * (numpy restatement: tests/train_det_heads_ref.py.)
 *
 * `scratch` holds hhfm_afm_train_det_scratch / hhfm_dfm_train_det_scratch
 * bytes for batches of that shape or any smaller B: the grouping's regions as
 * for FM, the stored contributions [B·F][k], the per-row head values, the
 * row losses and the Σvar² partials.  It carries no state and need not be
 * zeroed.  The size queries run on the host, need no device, and are
 * HHFM_EINVAL wherever the matching workspace query is, or when B·F does not
 * fit an int.  hipCUB's temporary storage is reserved by an upper bound; the
 * step checks the real figure before it launches anything.  Workspaces are
 * the default steps', same layout, still left zeroed.  The default steps'
 * argument checks come first, in their order; then a NULL scratch is
 * HHFM_EINVAL and a too small one HHFM_EWORKSPACE (also at B = 0), before
 * anything is launched: a refusal leaves every parameter, slot and the
 * workspace untouched. */
int hhfm_afm_train_det_scratch(int64_t B, int32_t F, int32_t k, int32_t A, int64_t features_M,
                               size_t* bytes);
int hhfm_dfm_train_det_scratch(int64_t B, int32_t F, int32_t k, int64_t features_M,
                               int32_t nlayers, const int32_t* layer_dims, size_t* bytes);
int hhfm_afm_train_step_det(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                            float* w, float* w0, int64_t features_M, int32_t k, int32_t A,
                            float* W, float* b, float* pvec, float* P, float lr,
                            float lambda_att, int32_t optimizer, float keep_att, float keep_afm,
                            uint64_t seed, float* const* acc, void* workspace, size_t ws_bytes,
                            void* scratch, size_t scratch_bytes, float* loss, void* stream);
int hhfm_dfm_train_step_det(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                            float* w, int64_t features_M, int32_t k, int32_t nlayers,
                            const int32_t* layer_dims, float* const* W, float* const* bias,
                            float* Wp, float* bp, float lr, float lambda_l2, int32_t optimizer,
                            float* const* acc, void* workspace, size_t ws_bytes, void* scratch,
                            size_t scratch_bytes, float* loss, void* stream);

/* ------------------------------------------------------------------------
 * DeepFM heads — the reference constructor's use_fm / use_deep / loss_type
 * (DFM.py:131-152, 199-204) as a run-time word of four entry points, whose
 * argument lists are those of hhfm_dfm_forward_ex, hhfm_dfm_catalog_topk_ex,
 * hhfm_dfm_train_step and hhfm_dfm_train_step_det plus `head`:
 *   head = HHFM_DFM_HEAD_FM | HHFM_DFM_HEAD_DEEP | HHFM_DFM_HEAD_SIGMOID
 * Neither FM nor DEEP set, or any other bit, is HHFM_EINVAL.  FM | DEEP (3)
 * is the model of the entry points above and runs their code: the same bits.
 *
 * Layouts.  Wp is the reference's concat_projection of that head — [F + k]
 * (FM), [d_L] (DEEP), [F + k + d_L] (both): the present parts in the order
 * y1, y2, h_L.  Without DEEP nlayers may be 0 and layer_dims / Wt / W / bias
 * NULL: nothing reads them.  w is a valid [features_M] array for every head.
 *
 * Forward.  z = [present parts]·Wp + bp; out = z, or 1/(1 + expf(−z)) with
 * SIGMOID (one elementwise pass over out after the forward).
 *   FM head: the FM part's own row kernels (the ones the fp32 split forward
 *     takes its `base` from; any k % 4 == 0, fp32 or bf16 table); proj_mode,
 *     plan and mlp_dtype are accepted and unused, the workspace is not touched
 *     and may be NULL.
 *   DEEP head: the full forward on a copy of Wp with F + k exact zeros in
 *     front, built on the stream in the workspace: ws_bytes must cover the
 *     *_workspace_ex size of the call plus HHFM_DFM_HEAD_WS_EXTRA(F, k, d_L)
 *     (the copy lies after the plan; the other heads need no extra).  Adding exact
 *     zeros changes no bit of h_L·Wp + bp — given finite w and table values:
 *     an Inf or NaN there would reach the score through 0·Inf.
 * Bad ids are read as row 0, as everywhere (flag them with hhfm_check_ids).
 *
 * Catalog top-K ranks by z and returns z, for every head: the sigmoid is
 * monotone, so the id lists are the reference's, and merges of item shards
 * stay exact because they merge z.  One difference: where two items' fp32
 * sigmoid values are equal although their z differ, the reference's top_k
 * orders them by index and this code by z.
 *
 * Loss and step.  Without SIGMOID  Σ_b (y_b − z_b)²/2, as hhfm_dfm_train_step.
 * With SIGMOID TF-1.x tf.losses.log_loss at its defaults:
 *   loss = (Σ_b l_b)/B,  l_b = −y·logf(p + ε) − (1 − y)·logf(1 − p + ε),
 *   ε = 1e-7f, p = 1/(1 + expf(−z)), one division by B, 0 at B = 0, y any
 *   real (the reference's epoch loop feeds −1; the formula stays finite);
 *   g_b = ∂loss/∂z_b = ((1 − y)/(1 − p + ε) − y/(p + ε))·p·(1 − p)/B.
 * Everything downstream of g_b is hhfm_dfm_train_step's expressions (dWp, dbp,
 * dw, the last layer's delta, the table scatter) over the present parts; the
 * l2 term is λ·‖Wp‖²/2, plus Σ_l λ·‖W_l‖²/2 only with DEEP (DFM.py:146-152).
 * A variable without a gradient does not move (TF's minimize skips it), nor
 * does its slot: without DEEP no W_l / b_l, without FM not w — the table then
 * receives the deep gradient only.  acc keeps the 2L+4 order; the entries of
 * variables that do not move are ignored (they may be NULL).  Without DEEP
 * the step launches no transpose and no GEMM.
 * hhfm_dfm_train_workspace / _state_bytes / _det_scratch serve every head
 * (upper bounds; the dWp region keeps its full-concat size and a head uses its
 * first entries), so heads of one layer list can share a workspace.  The
 * deterministic step keeps its promise for every head (the row loss l_b is
 * formed in float and summed in double in the scalar order, then divided by
 * B once).
 * ---------------------------------------------------------------------- */
#define HHFM_DFM_HEAD_FM 1
#define HHFM_DFM_HEAD_DEEP 2
#define HHFM_DFM_HEAD_SIGMOID 4
#define HHFM_DFM_HEAD_WS_EXTRA(F, k, dL) \
  ((((size_t)(F) + (size_t)(k) + (size_t)(dL)) * 4 + 255) & ~(size_t)255)
int hhfm_dfm_forward_head(const int32_t* idx, int64_t B, int32_t F, const void* E,
                          int64_t features_M, int32_t k, int32_t dtype, const float* w,
                          int32_t nlayers, const int32_t* layer_dims, const void* const* Wt,
                          const float* const* bias, int32_t mlp_dtype, const float* Wp,
                          float bp, float* out, int32_t proj_mode, int32_t plan,
                          void* workspace, size_t ws_bytes, void* stream, int32_t head);
int hhfm_dfm_catalog_topk_head(const int32_t* qidx, int64_t B, int32_t F, int32_t item_col,
                               const void* E, int64_t features_M, int32_t k, int32_t dtype,
                               const float* w, int32_t nlayers, const int32_t* layer_dims,
                               const void* const* Wt, const float* const* bias,
                               int32_t mlp_dtype, const float* Wp, float bp,
                               int32_t item_row_begin, int32_t item_count,
                               int32_t global_item_base, int32_t K, int64_t chunk_rows,
                               float* top_score, int32_t* top_idx, int32_t proj_mode,
                               int32_t plan, void* workspace, size_t ws_bytes, void* stream,
                               int32_t head);
int hhfm_dfm_train_step_head(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                             float* w, int64_t features_M, int32_t k, int32_t nlayers,
                             const int32_t* layer_dims, float* const* W, float* const* bias,
                             float* Wp, float* bp, float lr, float lambda_l2,
                             int32_t optimizer, float* const* acc, void* workspace,
                             size_t ws_bytes, float* loss, void* stream, int32_t head);
int hhfm_dfm_train_step_head_det(const int32_t* idx, const float* y, int64_t B, int32_t F,
                                 float* E, float* w, int64_t features_M, int32_t k,
                                 int32_t nlayers, const int32_t* layer_dims, float* const* W,
                                 float* const* bias, float* Wp, float* bp, float lr,
                                 float lambda_l2, int32_t optimizer, float* const* acc,
                                 void* workspace, size_t ws_bytes, void* scratch,
                                 size_t scratch_bytes, float* loss, void* stream, int32_t head);

/* ------------------------------------------------------------------------
 * CARS2 — the context-aware baseline the reference's driver runs beside the
 * four FM-family models (Newcode/CARS2.py; main.py:63).  Pure additions:
 * HHFM_ABI_VERSION stays 6.
 *
 * Sizes (CARS2.py:53-56): D = hidden_factor, Dc = int(D/2.5), Dp = int(D/5),
 * Dq = int(D/2.5); the entry points take them as arguments, each >= 1.
 * Variables (:150-164), all row-major: UI [n_ui][D] (n_ui = n_user + n_item;
 * fp32, or bf16 for scoring: upcast exactly), and always fp32 Context [Mc][Dc],
 * W [D][Dp][Dc], Z [D][Dq][Dc], A [Dp], B [Dq].  Mc is the number of distinct
 * context tuples (Train.__init__, :212-216); a row is (user id, item id,
 * context id m), ids of UI rows in [0, n_ui), m in [0, Mc).
 *
 * The reference's graph (:85-105), u = UI[user], i = UI[item], c = Context[m]:
 *   pik_p = Σ_c (Σ_d u_d W[d,p,c]) c_c      qjk_q = Σ_c (Σ_d i_d Z[d,q,c]) c_c
 *   s     = u·i + Σ_p pik_p A_p + Σ_q qjk_q B_q
 * The device arithmetic is the folded form — the same elementary products in
 * another association, every sum an fp32 fmaf chain:
 *   WA[d,c] = Σ_p W[d,p,c]·A[p]      ZB[d,c] = Σ_q Z[d,q,c]·B[q]      (D x Dc)
 *   GA[m,:] = WA · Context[m]        GB[m,:] = ZB · Context[m]        (Mc x D)
 *   row      s = u·i + u·GA[m] + i·GB[m]
 *   catalog  h = u + GB[m], cst = u·GA[m], score[b,n] = h_b·UI[item n] + cst_b
 *            (CARS2.topk, :171-187)
 *
 * hhfm_cars2_prepare writes GA | GB | WA | ZB, in that order and unpadded,
 * into `prepared` (hhfm_cars2_prepared_bytes(Mc, D, Dc) bytes; 16-byte aligned
 * for the fast row kernel).  It must be called again whenever Context, W, Z, A
 * or B change; UI does not enter it.
 *
 * hhfm_cars2_score_rows: idx int32 [B][3] -> out [B].  A user or item id
 * outside [0, n_ui) or a context id outside [0, Mc) reads row 0 and ORs
 * HHFM_STATUS_BAD_ID into *status (status may be NULL).  UI rows that are a
 * power-of-two number (<= 64) of 16-byte chunks take the chunked kernel, any
 * other D (e.g. 20) a generic one-wave-per-row kernel.
 *
 * hhfm_cars2_catalog_topk: q int32 [B][2] = (user id, context id); items are
 * rows [item_row_begin, item_row_begin + item_count) of UI.  A query kernel
 * writes h and cst into the hhfm_catalog_topk_workspace layout, then the
 * dense / streaming / ring / merge paths of hhfm_catalog_topk_ex run
 * unchanged, on their HHFM_MODE_FM form with w = NULL.  Workspace
 * (hhfm_catalog_topk_workspace(B, item_count, D, K)), plan flags, shape limits
 * (D/8 fp32 or D/16 bf16 a power of two <= 16, K <= 64, K <= item_count), the
 * (score desc, index asc) order and the error codes are that entry point's.
 * The small-catalog fused kernel is never taken.  Bad ids as above.
 *
 * hhfm_cars2_train_step (partial_fit, :87, :103-136, :167-170): X int32 [B][2]
 * (user, item), Fea int32 [B] context ids, Neg int32 [B][NG], 1 <= NG <= 16.
 *   n_b = Σ_j UI[Neg[b,j]]  (a SUM; the reference trains with NG = 1)
 *   δ = i − n,  x_b = u·δ + δ·GB[m]   (pik·A is in both feedbacks and cancels)
 *   loss = −Σ_b logf σ(x_b)  (+ λ·Σ var²/2 over all six variables when λ > 0)
 * With g_b = σ(x_b) − 1:
 *   dUI[user] += g·δ;  dUI[item] += g·(u + GB[m]);  dUI[Neg[b,j]] −= g·(u + GB[m])
 *   for every j (a repeated id receives every contribution);
 *   dContext[m][c] += g·Σ_d δ_d ZB[d,c];   T[d,c] = Σ_b g_b δ_bd c_bc;
 *   dZ[d,q,c] = B_q·T[d,c];   dB[q] = Σ_{d,c} Z[d,q,c]·T[d,c];
 *   W and A: the data gradient is identically zero, only λ acts on them.
 * Optimizer rules as in H6 (enum hhfm_optimizer).  λ > 0: every variable is
 * dense.  λ <= 0 is λ = 0 (:115): UI and Context follow the IndexedSlices
 * rules, Z and B are dense, W and A receive a dense zero gradient.  acc: 6
 * slot arrays in the order UI, Context, W, Z, A, B (ignored under SGD).
 * *loss is the loss of the pre-update parameters.  Float atomics: not
 * deterministic.  fp32 only.  B = 0 is a step like any other.
 * Workspace: hhfm_cars2_train_workspace(B, ...) bytes for batches of at most B
 * rows, zero-filled once; its first hhfm_cars2_train_state_bytes bytes are the
 * persistent part (gradient buffers, Adam's β powers, the touched masks), left
 * zeroed but for the powers; the rest is per-batch scratch, so a workspace
 * grown for a larger batch keeps its state by copying that prefix.
 * Checks, in order: sizes (HHFM_EINVAL), NG > 16 or D > 512
 * (HHFM_EUNSUPPORTED), the optimizer code (HHFM_EUNSUPPORTED), NULL variables /
 * loss / workspace, NULL rows at B > 0, NULL slots (HHFM_EINVAL), a short
 * workspace (HHFM_EWORKSPACE) — all before anything is launched.
 * Not built: a deterministic CARS2 step, bf16 training tables, a CARS2 form of
 * the small-catalog fused kernel.
 * (numpy restatement in the reference's op order: tests/cars2_ref.py.)
 * ---------------------------------------------------------------------- */
int hhfm_cars2_prepared_bytes(int64_t Mc, int32_t D, int32_t Dc, size_t* bytes);
int hhfm_cars2_prepare(const float* Context, int64_t Mc, const float* W, const float* A,
                       const float* Z, const float* B, int32_t D, int32_t Dc, int32_t Dp,
                       int32_t Dq, void* prepared, size_t prepared_bytes, void* stream);
int hhfm_cars2_score_rows(const int32_t* idx, int64_t B, const void* UI, int64_t n_ui,
                          int32_t D, int32_t dtype, const void* prepared, int64_t Mc,
                          float* out, int32_t* status, void* stream);
int hhfm_cars2_catalog_topk(const int32_t* q, int64_t B, const void* UI, int64_t n_ui,
                            int32_t D, int32_t dtype, const void* prepared, int64_t Mc,
                            int32_t item_row_begin, int32_t item_count,
                            int32_t global_item_base, int32_t K, float* top_score,
                            int32_t* top_idx, void* workspace, size_t ws_bytes, int32_t plan,
                            int32_t* status, void* stream);
int hhfm_cars2_train_workspace(int64_t B, int64_t n_ui, int64_t Mc, int32_t D, int32_t Dc,
                               int32_t Dp, int32_t Dq, size_t* ws_bytes);
int hhfm_cars2_train_state_bytes(int64_t n_ui, int64_t Mc, int32_t D, int32_t Dc, int32_t Dp,
                                 int32_t Dq, size_t* state_bytes);
int hhfm_cars2_train_step(const int32_t* X, const int32_t* Fea, const int32_t* Neg, int64_t B,
                          int32_t NG, float* UI, int64_t n_ui, float* Context, int64_t Mc,
                          float* W, float* Z, float* A, float* Bv, int32_t D, int32_t Dc,
                          int32_t Dp, int32_t Dq, float lr, float lambda_l2, int32_t optimizer,
                          float* const* acc, void* workspace, size_t ws_bytes, float* loss,
                          void* stream);

/* tf.nn.top_k(scores, K) over a materialised score matrix [B][ld] (first N
 * columns), K <= 64; ids reported as global_item_base + column. */
int hhfm_topk_dense(const float* scores, int64_t B, int32_t N, int64_t ld, int32_t K,
                    int32_t global_item_base, float* top_score, int32_t* top_idx,
                    void* stream);
/* Same, with plan flags: HHFM_PLAN_ONE_WAVE keeps one wave per query where
 * the default splits a query over 4 waves (B <= 1,024, N >= 1,024). */
int hhfm_topk_dense_ex(const float* scores, int64_t B, int32_t N, int64_t ld, int32_t K,
                       int32_t global_item_base, float* top_score, int32_t* top_idx,
                       int32_t plan, void* stream);

/* ------------------------------------------------------------------------
 * H5 / H3 — harness membership test and metric walk
 *
 * positive_feedback (NewLoadData.py:49-56: key = every column but the item
 * -> set of items) as two sorted device arrays: keys [nkeys][key_cols]
 * int32, distinct, lexicographically sorted (key_cols = ncols - 1); codes
 * [ncodes] int64 = (rank of the key in `keys`) << 32 | item, sorted.
 *
 * hhfm_pf_contains: out[b][j] = 1 iff cand[b][j] is in positive_feedback
 * of row b's key — the rejection test of Train.sample_negative
 * (FM.py:291-293).  cand == NULL (num = 1): the row's own item (column
 * item_col) — evaluate_TopK's `item in positive_feedback[key]`
 * (FM.py:343-355).  rows: int32 [B][ncols]; out: uint8 [B][num].
 *
 * hhfm_topk_walk: evaluate_TopK's walk over P predictions (FM.py:344-357)
 * per row: outcome = n >= 0 (target at walk position n < TopK), -1 (walk
 * passed TopK-1: the reference appends 0, 0, 0), -2 (predictions
 * exhausted: it appends nothing).  pred: int32 [B][P] global item ids,
 * target int32 [B], positive uint8 [B] (from hhfm_pf_contains).
 * ---------------------------------------------------------------------- */
int hhfm_pf_contains(const int32_t* keys, int64_t nkeys, int32_t key_cols,
                     const int64_t* codes, int64_t ncodes, const int32_t* rows,
                     int64_t B, int32_t ncols, int32_t item_col,
                     const int32_t* cand, int32_t num, uint8_t* out, void* stream);
int hhfm_topk_walk(const int32_t* pred, int64_t B, int32_t P, const int32_t* target,
                   const uint8_t* positive, int32_t TopK, int32_t* outcome, void* stream);

/* hhfm_sample_negative (ABI v5) — all of Train.sample_negative
 * (FM.py:284-294) on the device, on numpy's own random stream:
 *   samples = np.random.randint(lo, hi, size=(B, num)), then in row-major
 *   order each sample that is in positive_feedback[key of its row] re-drawn
 *   with np.random.randint(lo, hi) until it is not.
 * mt_state: device uint32 [625] = the legacy RandomState's MT19937 key[624]
 * followed by pos (np.random.get_state()[1:3]); on return it holds the state
 * after the last word the call read, for np.random.set_state — the samples
 * and the state equal the reference's bit for bit (numpy's masked bounded
 * draw: 32-bit outputs AND the smallest covering mask, rejected while > hi -
 * 1 - lo).  rows int32 [B][ncols] (key = every column but item_col), keys /
 * codes as for hhfm_pf_contains; samples: device int64 [B][num].  Requires
 * 0 <= lo < hi <= 2^31, B·num < 2^30.  A row whose positives cover all of
 * [lo, hi) (where the reference loops forever) returns HHFM_EINVAL.  Unlike
 * the other entry points this call synchronises `stream` (a few small
 * device-to-host reads steer the generation rounds); the workspace is
 * hhfm_sample_negative_workspace(B, num) bytes, no initialisation needed.
 * Replaces FM.py:284-294 (and OurModel7.py, AFM.py, DFM.py's copies). */
int hhfm_sample_negative_workspace(int64_t B, int32_t num, size_t* ws_bytes);
/* The same, sized for the faster re-draw test: per-key bitmaps of the
 * positives over [lo, hi) (nkeys x ceil((hi - lo) / 32) words, used when at
 * most 256 MB); hhfm_sample_negative takes the bitmap path whenever ws_bytes
 * covers it.  Results are identical either way. */
int hhfm_sample_negative_workspace_ex(int64_t B, int32_t num, int64_t lo, int64_t hi,
                                      int64_t nkeys, size_t* ws_bytes);
int hhfm_sample_negative(uint32_t* mt_state, int64_t lo, int64_t hi, const int32_t* rows,
                         int64_t B, int32_t ncols, int32_t item_col, int32_t num,
                         const int32_t* keys, int64_t nkeys, const int64_t* codes,
                         int64_t ncodes, int64_t* samples, void* workspace, size_t ws_bytes,
                         void* stream);

/* ------------------------------------------------------------------------
 * L1 — the libfm loader's per-cell work (NewLoadData.py:16-58), HOST code:
 * every pointer below is host memory, nothing touches the GPU.
 *
 * hhfm_libfm_encode: parse `len` bytes of "label tok ... tok" lines
 * (ncols fields separated by single spaces, blank lines skipped, at most
 * max_rows rows) into labels [rows] (double) and ids [rows][ncols-1]
 * (int64): the column-major first-occurrence token -> id map over columns
 * 1.. (NewLoadData.py:29-34; identical tokens share an id across columns).
 * distinct[ncols-1] = distinct tokens per column (n_user, n_item, ...:
 * NewLoadData.py:22-23); *features_M = distinct tokens overall.
 *
 * hhfm_loader_split: over the shuffled rows data [rows][ncols] (label,
 * user, item, ctx...), is_test[r] = 1 iff row r's key (every column but 0
 * and item_col) is unseen and fewer than test_size rows went to Test so
 * far (NewLoadData.py:46-58).
 * ---------------------------------------------------------------------- */
int hhfm_libfm_encode(const char* buf, int64_t len, int32_t ncols, int64_t max_rows,
                      double* labels, int64_t* ids, int64_t* rows_out, int64_t* features_M,
                      int64_t* distinct);
int hhfm_loader_split(const int64_t* data, int64_t rows, int32_t ncols, int32_t item_col,
                      int64_t test_size, uint8_t* is_test);

/* ------------------------------------------------------------------------
 * Id validation (tf.nn.embedding_lookup raises InvalidArgumentError on an id
 * outside [0, features_M): FM.py:99, OurModel7.py:105, AFM.py:104, DFM.py:105).
 * Every kernel reads such an id as row 0 so it can never fault; callers that
 * want TF's error pass a device status word:
 *   hhfm_check_ids   — async: ORs HHFM_STATUS_BAD_ID into *status (device
 *                      int32) if any of idx[0..n) is outside [0, features_M);
 *                      covers every entry point without an _ex status form
 *                      (AFM, DeepFM, training, harness).
 *   hhfm_status_read — synchronises `stream`, reads and clears *status;
 *                      returns HHFM_EINVAL if a bad id was seen, else HHFM_OK.
 * ---------------------------------------------------------------------- */
int hhfm_check_ids(const int32_t* idx, int64_t n, int64_t features_M, int32_t* status,
                   void* stream);
int hhfm_status_read(int32_t* status, void* stream);

/* ------------------------------------------------------------------------
 * Measurement probe (not a scoring entry point): streams `bytes` (a multiple
 * of 16, 16-B aligned) of device memory once with 16-B loads, so bench.py
 * can report K1's HBM fraction against the box's measured read ceiling as
 * well as the 8 TB/s spec.  mode 0: grid-stride; 1: one contiguous chunk per
 * workgroup, 8 loads in flight per lane; 2: as 1 with non-temporal loads.
 * `sink`: one device float (written only on an impossible data value, so the
 * loads cannot be elided).
 * ---------------------------------------------------------------------- */
int hhfm_probe_stream_read(const void* buf, int64_t bytes, int32_t mode, float* sink,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HHFM_H_ */
