// CARS2 (Newcode/CARS2.py) — what cars2.hip offers the other translation
// units: its query kernel to catalog_topk.hip (hhfm_cars2_catalog_topk runs
// catalog_topk_impl's main kernels on it) and its training kernels to
// train.hip (hhfm_cars2_train_step ends in optimizer_tail).  include/hhfm.h
// "CARS2" states the model, the fold and the layouts.
#pragma once
#include "hhfm_common.h"

namespace hhfm {

// The query side of hhfm_cars2_catalog_topk: q [B][2] = (user id, context id).
struct Cars2Query {
  const float* GA;   // [Mc][D] fp32 (hhfm_cars2_prepare)
  const float* GB;   // [Mc][D]
  int64_t Mc;
};

// H[b] = UI[user] + GB[m], cst[b] = UI[user]·GA[m] for b < B, zeros up to
// Bpad; a user id outside [0, n_ui) or a context id outside [0, Mc) reads row
// 0 and ORs HHFM_STATUS_BAD_ID into *status (when given).
void cars2_launch_queries(const int32_t* q, int64_t B, int64_t Bpad, const char* UI, bool bf16,
                          int64_t n_ui, int D, const Cars2Query& cq, float* H, float* cst,
                          int32_t* status, hipStream_t st);

// out[d][c] = Σ_p T3[d][p][c]·vec[p]   (WA from W, A; ZB from Z, B)
void cars2_launch_fold(const float* T3, const float* vec, int D, int P, int Dc, float* out,
                       hipStream_t st);
// G[m][d] = Σ_c fold[d][c]·Context[m][c]   (GA from WA; GB from ZB)
void cars2_launch_table(const float* fold, const float* Context, int64_t Mc, int D, int Dc,
                        float* G, hipStream_t st);

constexpr int kCars2TrainMaxD = 512;   // one row's δ staged per wave in LDS

// The row pass of the step (B > 0): loss and g per row, the scatter into dUI
// and dContext, and gδ [B][D] for cars2_launch_t.
void cars2_launch_train_rows(const int32_t* X, const int32_t* Fea, const int32_t* Neg, int64_t B,
                             int NG, const float* UI, int64_t n_ui, int D, int Dc,
                             const float* GB, const float* ZB, int64_t Mc, float* dUI,
                             float* dCtx, float* gdelta, float* data_loss, hipStream_t st);
// T[d][c] += Σ_b gδ[b][d]·Context[m_b][c]   (T zeroed by the caller)
void cars2_launch_t(const float* gdelta, const int32_t* Fea, const float* Context, int64_t B,
                    int64_t Mc, int D, int Dc, float* T, hipStream_t st);
// dZ[d][q][c] = B[q]·T[d][c];  dB[q] = Σ_{d,c} Z[d][q][c]·T[d][c]
void cars2_launch_dz_db(const float* Z, const float* Bv, const float* T, int D, int Dq, int Dc,
                        float* dZ, float* dB, hipStream_t st);

}  // namespace hhfm
