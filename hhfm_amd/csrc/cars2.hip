// CARS2 — the context-aware baseline of the reference's driver
// (Newcode/CARS2.py; main.py:63) on gfx950.
//
//   hhfm_cars2_prepare        folds W·A and Z·B and forms the per-context
//                             tables GA, GB (CARS2.py:90-97 restated, below)
//   hhfm_cars2_score_rows     replaces sess.run(PositiveFeadback)  (CARS2.py:85-105)
//   cars2_queries             the query kernel of hhfm_cars2_catalog_topk
//                             (catalog_topk.hip; CARS2.topk, CARS2.py:171-187)
//   cars2_train_rows, cars2_t, cars2_dz, cars2_db
//                             the kernels of hhfm_cars2_train_step (train.hip;
//                             CARS2.partial_fit, CARS2.py:87, :103-136, :167-170)
//
// The reference's graph, with u = UI[user], i = UI[item], c = Context[m]:
//   pik_p = Σ_c (Σ_d u_d W[d,p,c]) c_c      qjk_q = Σ_c (Σ_d i_d Z[d,q,c]) c_c
//   s     = u·i + Σ_p pik_p A_p + Σ_q qjk_q B_q
// The device arithmetic is the same elementary products folded per context id:
//   WA[d,c] = Σ_p W[d,p,c]·A[p]     ZB[d,c] = Σ_q Z[d,q,c]·B[q]
//   GA[m,:] = WA · Context[m]       GB[m,:] = ZB · Context[m]       (fp32)
//   s = u·i + u·GA[m] + i·GB[m]
// so a row is four gathered rows — two of UI, two of the small tables — and
// three dot products in registers, and a catalog query is h = u + GB[m],
// cst = u·GA[m], score = h·item + cst: the form catalog_topk.hip consumes.
#include "cars2.h"

namespace hhfm {

// ---------------------------------------------------------------------------
// prepare
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cars2_fold(const float* __restrict__ T3,
                                                  const float* __restrict__ vec, int D, int P,
                                                  int Dc, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D * Dc) return;
  const int d = i / Dc, c = i - d * Dc;
  float s = 0.f;
  for (int p = 0; p < P; ++p) s = fmaf(T3[((int64_t)d * P + p) * Dc + c], vec[p], s);
  out[i] = s;
}

__global__ __launch_bounds__(256) void cars2_table(const float* __restrict__ fold,
                                                   const float* __restrict__ Context, int64_t Mc,
                                                   int D, int Dc, float* __restrict__ G) {
  const int64_t n = Mc * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / D;
    const int d = (int)(i - m * D);
    float s = 0.f;
    for (int c = 0; c < Dc; ++c) s = fmaf(fold[d * Dc + c], Context[m * Dc + c], s);
    G[i] = s;
  }
}

static int blocks_for(int64_t n, int cap) {
  int64_t g = (n + 255) / 256;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

void cars2_launch_fold(const float* T3, const float* vec, int D, int P, int Dc, float* out,
                       hipStream_t st) {
  hipLaunchKernelGGL(cars2_fold, dim3(blocks_for((int64_t)D * Dc, 1 << 20)), dim3(256), 0, st, T3,
                     vec, D, P, Dc, out);
}

void cars2_launch_table(const float* fold, const float* Context, int64_t Mc, int D, int Dc,
                        float* G, hipStream_t st) {
  hipLaunchKernelGGL(cars2_table, dim3(blocks_for(Mc * D, 8192)), dim3(256), 0, st, fold, Context,
                     Mc, D, Dc, G);
}

// ---------------------------------------------------------------------------
// row scores
// ---------------------------------------------------------------------------
// LPR lanes per row, one 16-byte chunk of the UI rows each (fm_rows.hip's
// layout); the lane's E elements of GA[m] / GB[m] are E/4 further 16-byte
// loads.  Rows past B read row 0 so that every lane stays active for the DPP
// reduction.
template <int LPR, bool BF16>
__global__ __launch_bounds__(256) void cars2_rows_fast(
    const int32_t* __restrict__ idx, int64_t B, const char* __restrict__ UI, int64_t n_ui,
    const float* __restrict__ GA, const float* __restrict__ GB, int64_t Mc,
    float* __restrict__ out, int32_t* __restrict__ status) {
  using C = Chunk<BF16>;
  constexpr int E = C::kElems;
  constexpr int RPW = kWave / LPR;
  constexpr int64_t ROW_BYTES = (int64_t)LPR * 16;
  constexpr int D = LPR * E;
  const uint32_t N32 = id_limit32(n_ui), M32 = id_limit32(Mc);
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (LPR - 1);
  const int g = lane / LPR;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  bool bad = false;
  for (int64_t base = wave * RPW; base < B; base += nwave * RPW) {
    const int64_t row = base + g;
    const bool live = row < B;
    int32_t ru = 0, ri = 0, rm = 0;
    if (live) {
      const int32_t* p = idx + row * 3;
      ru = p[0];
      ri = p[1];
      rm = p[2];
    }
    const int32_t iu = clamp_id32(ru, N32), ii = clamp_id32(ri, N32), im = clamp_id32(rm, M32);
    bad |= iu != ru || ii != ri || im != rm;
    C u, it;
    u.load(UI + (int64_t)iu * ROW_BYTES + sub * 16);
    it.load(UI + (int64_t)ii * ROW_BYTES + sub * 16);
    const float* ga = GA + (int64_t)im * D + sub * E;
    const float* gb = GB + (int64_t)im * D + sub * E;
    float a[E], b[E];
#pragma unroll
    for (int j = 0; j < E / 4; ++j) {
      const f32x4_t va = *reinterpret_cast<const f32x4_t*>(ga + 4 * j);
      const f32x4_t vb = *reinterpret_cast<const f32x4_t*>(gb + 4 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[4 * j + e] = va[e];
        b[4 * j + e] = vb[e];
      }
    }
    float t = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      t = fmaf(u.v[e], it.v[e], t);   // u·i       CARS2.py:103
      t = fmaf(u.v[e], a[e], t);      // pik·A     :104, folded
      t = fmaf(it.v[e], b[e], t);     // qjk·B     :105, folded
    }
    t = group_sum_dpp<LPR>(t);
    if (sub == 0 && live) out[row] = t;
  }
  report_bad_id(status, bad);
}

// any D: one wave per row
template <bool BF16>
__global__ __launch_bounds__(256) void cars2_rows_generic(
    const int32_t* __restrict__ idx, int64_t B, const char* __restrict__ UI, int64_t n_ui, int D,
    const float* __restrict__ GA, const float* __restrict__ GB, int64_t Mc,
    float* __restrict__ out, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int esz = BF16 ? 2 : 4;
  auto val = [&](int32_t id, int e) -> float {
    const char* r = UI + (int64_t)id * D * esz;
    return BF16 ? bf16_to_f32(reinterpret_cast<const uint16_t*>(r)[e])
                : reinterpret_cast<const float*>(r)[e];
  };
  bool bad = false;
  for (int64_t row = wave; row < B; row += nwave) {
    const int32_t* p = idx + row * 3;
    const int32_t iu = clamp_id(p[0], n_ui), ii = clamp_id(p[1], n_ui), im = clamp_id(p[2], Mc);
    bad |= iu != p[0] || ii != p[1] || im != p[2];
    float t = 0.f;
    for (int e = lane; e < D; e += kWave) {
      const float u = val(iu, e), it = val(ii, e);
      t = fmaf(u, it, t);
      t = fmaf(u, GA[(int64_t)im * D + e], t);
      t = fmaf(it, GB[(int64_t)im * D + e], t);
    }
    t = group_sum<kWave>(t);
    if (lane == 0) out[row] = t;
  }
  report_bad_id(status, bad);
}

// ---------------------------------------------------------------------------
// catalog query vectors (CARS2.topk, CARS2.py:171-187): one wave per query
// ---------------------------------------------------------------------------
template <bool BF16>
__global__ __launch_bounds__(256) void cars2_queries(
    const int32_t* __restrict__ q, int64_t B, int64_t Bpad, const char* __restrict__ UI,
    int64_t n_ui, int D, const float* __restrict__ GA, const float* __restrict__ GB, int64_t Mc,
    float* __restrict__ H, float* __restrict__ cst, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int esz = BF16 ? 2 : 4;
  bool bad = false;
  for (int64_t b = wave; b < Bpad; b += nwave) {
    float part = 0.f;
    if (b < B) {
      const int32_t ru = q[b * 2], rm = q[b * 2 + 1];
      const int32_t iu = clamp_id(ru, n_ui), im = clamp_id(rm, Mc);
      bad |= iu != ru || im != rm;
      const char* r = UI + (int64_t)iu * D * esz;
      for (int e = lane; e < D; e += kWave) {
        const float u = BF16 ? bf16_to_f32(reinterpret_cast<const uint16_t*>(r)[e])
                             : reinterpret_cast<const float*>(r)[e];
        H[b * D + e] = u + GB[(int64_t)im * D + e];        // the item's factor  :181-185
        part = fmaf(u, GA[(int64_t)im * D + e], part);     // item-independent   :178-184
      }
    } else {
      for (int e = lane; e < D; e += kWave) H[b * D + e] = 0.f;
    }
    part = group_sum<kWave>(part);
    if (lane == 0) cst[b] = part;
  }
  report_bad_id(status, bad);
}

void cars2_launch_queries(const int32_t* q, int64_t B, int64_t Bpad, const char* UI, bool bf16,
                          int64_t n_ui, int D, const Cars2Query& cq, float* H, float* cst,
                          int32_t* status, hipStream_t st) {
  int64_t blocks = (Bpad + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  if (bf16)
    hipLaunchKernelGGL(cars2_queries<true>, dim3((int)blocks), dim3(256), 0, st, q, B, Bpad, UI,
                       n_ui, D, cq.GA, cq.GB, cq.Mc, H, cst, status);
  else
    hipLaunchKernelGGL(cars2_queries<false>, dim3((int)blocks), dim3(256), 0, st, q, B, Bpad, UI,
                       n_ui, D, cq.GA, cq.GB, cq.Mc, H, cst, status);
}

// ---------------------------------------------------------------------------
// training (include/hhfm.h "CARS2": loss, gradients)
// ---------------------------------------------------------------------------
// One wave per batch row:
//   n = Σ_j UI[Neg_j], δ = i − n, x = u·δ + δ·GB[m], g = σ(x) − 1
//   dUI[user] += g·δ; dUI[item] += g·(u + GB[m]); dUI[Neg_j] −= g·(u + GB[m])
//   dContext[m][c] += g·Σ_d δ_d ZB[d][c]      (δ staged in LDS, lane = c)
//   gδ[b][:] for the T reduction
__global__ __launch_bounds__(256) void cars2_train_rows(
    const int32_t* __restrict__ X, const int32_t* __restrict__ Fea,
    const int32_t* __restrict__ Neg, int64_t B, int NG, const float* __restrict__ UI,
    int64_t n_ui, int D, int Dc, const float* __restrict__ GB, const float* __restrict__ ZB,
    int64_t Mc, float* __restrict__ dUI, float* __restrict__ dCtx, float* __restrict__ gdelta,
    float* __restrict__ data_loss) {
  __shared__ float sdelta[4][kCars2TrainMaxD];
  const int l = threadIdx.x & 63;
  float* sd = sdelta[threadIdx.x >> 6];
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t b = wave; b < B; b += nwave) {
    const int64_t iu = clamp_id(X[b * 2], n_ui), ii = clamp_id(X[b * 2 + 1], n_ui);
    const int64_t im = clamp_id(Fea[b], Mc);
    const int32_t* ng = Neg + b * NG;
    int32_t nid[kMaxNeg];
#pragma unroll
    for (int j = 0; j < kMaxNeg; ++j) nid[j] = j < NG ? clamp_id(ng[j], n_ui) : 0;
    float x = 0.f;
    for (int e = l; e < D; e += kWave) {
      float n = 0.f;
#pragma unroll
      for (int j = 0; j < kMaxNeg; ++j)
        if (j < NG) n += UI[(int64_t)nid[j] * D + e];      // Negitems: a sum   :87
      const float dl = UI[ii * D + e] - n;
      sd[e] = dl;
      x = fmaf(UI[iu * D + e], dl, x);
      x = fmaf(dl, GB[im * D + e], x);
    }
    x = group_sum<kWave>(x);                               // Positive − Negative  :112
    const float sg = 1.f / (1.f + expf(-x));
    const float g = sg - 1.f;                              // d(−log σ(x))/dx
    for (int e = l; e < D; e += kWave) {
      const float dl = sd[e];
      const float hv = UI[iu * D + e] + GB[im * D + e];
      gdelta[b * D + e] = g * dl;
      atomicAdd(dUI + iu * D + e, g * dl);
      atomicAdd(dUI + ii * D + e, g * hv);
#pragma unroll
      for (int j = 0; j < kMaxNeg; ++j)
        if (j < NG) atomicAdd(dUI + (int64_t)nid[j] * D + e, -g * hv);
    }
    __builtin_amdgcn_wave_barrier();   // the wave's LDS accesses are in order
    for (int c = l; c < Dc; c += kWave) {
      float s = 0.f;
      for (int d = 0; d < D; ++d) s = fmaf(sd[d], ZB[d * Dc + c], s);
      atomicAdd(dCtx + im * Dc + c, g * s);
    }
    __builtin_amdgcn_wave_barrier();
    if (l == 0) atomicAdd(data_loss, -logf(sg));
  }
}

// T[d][c] += Σ_b gδ[b][d]·Context[m_b][c]: thread = (d, c), the rows split
// over gridDim.y
__global__ __launch_bounds__(256) void cars2_t(const float* __restrict__ gdelta,
                                               const int32_t* __restrict__ Fea,
                                               const float* __restrict__ Context, int64_t B,
                                               int64_t Mc, int D, int Dc, float* __restrict__ T) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D * Dc) return;
  const int d = i / Dc, c = i - d * Dc;
  float s = 0.f;
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y)
    s = fmaf(gdelta[b * D + d], Context[(int64_t)clamp_id(Fea[b], Mc) * Dc + c], s);
  atomicAdd(T + i, s);
}

__global__ __launch_bounds__(256) void cars2_dz(const float* __restrict__ Bv,
                                                const float* __restrict__ T, int D, int Dq,
                                                int Dc, float* __restrict__ dZ) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D * Dq * Dc) return;
  const int c = i % Dc, q = (i / Dc) % Dq, d = i / (Dc * Dq);
  dZ[i] = Bv[q] * T[d * Dc + c];
}

// one workgroup per q
__global__ __launch_bounds__(256) void cars2_db(const float* __restrict__ Z,
                                                const float* __restrict__ T, int D, int Dq,
                                                int Dc, float* __restrict__ dB) {
  __shared__ float part[4];
  const int q = blockIdx.x;
  float s = 0.f;
  for (int j = threadIdx.x; j < D * Dc; j += blockDim.x) {
    const int d = j / Dc, c = j - d * Dc;
    s = fmaf(Z[((int64_t)d * Dq + q) * Dc + c], T[j], s);
  }
  s = group_sum<kWave>(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) dB[q] = (part[0] + part[1]) + (part[2] + part[3]);
}

void cars2_launch_train_rows(const int32_t* X, const int32_t* Fea, const int32_t* Neg, int64_t B,
                             int NG, const float* UI, int64_t n_ui, int D, int Dc,
                             const float* GB, const float* ZB, int64_t Mc, float* dUI,
                             float* dCtx, float* gdelta, float* data_loss, hipStream_t st) {
  hipLaunchKernelGGL(cars2_train_rows, dim3(blocks_for(B * 64, 8192)), dim3(256), 0, st, X, Fea,
                     Neg, B, NG, UI, n_ui, D, Dc, GB, ZB, Mc, dUI, dCtx, gdelta, data_loss);
}

void cars2_launch_t(const float* gdelta, const int32_t* Fea, const float* Context, int64_t B,
                    int64_t Mc, int D, int Dc, float* T, hipStream_t st) {
  const int split = (int)(B < 64 ? B : 64);
  hipLaunchKernelGGL(cars2_t, dim3(blocks_for((int64_t)D * Dc, 1 << 20), split), dim3(256), 0, st,
                     gdelta, Fea, Context, B, Mc, D, Dc, T);
}

void cars2_launch_dz_db(const float* Z, const float* Bv, const float* T, int D, int Dq, int Dc,
                        float* dZ, float* dB, hipStream_t st) {
  hipLaunchKernelGGL(cars2_dz, dim3(blocks_for((int64_t)D * Dq * Dc, 1 << 20)), dim3(256), 0, st,
                     Bv, T, D, Dq, Dc, dZ);
  hipLaunchKernelGGL(cars2_db, dim3(Dq), dim3(256), 0, st, Z, T, D, Dq, Dc, dB);
}

// fp32 rows of LPR 16-byte chunks, LPR a power of two <= 64; 0: the generic kernel
static int cars2_lpr(int D, bool bf16) {
  const int64_t row_bytes = (int64_t)D * (bf16 ? 2 : 4);
  if (row_bytes % 16) return 0;
  const int64_t lpr = row_bytes / 16;
  if (lpr > 64 || (lpr & (lpr - 1))) return 0;
  return (int)lpr;
}

template <int LPR, bool BF16>
static void launch_rows_fast(const int32_t* idx, int64_t B, const char* UI, int64_t n_ui,
                             const float* GA, const float* GB, int64_t Mc, float* out,
                             int32_t* status, hipStream_t st) {
  const int64_t rpb = 4 * (kWave / LPR);
  int64_t grid = (B + rpb - 1) / rpb;
  const int64_t cap = (int64_t)stream_cu_count(st) * 8;
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL((cars2_rows_fast<LPR, BF16>), dim3((int)grid), dim3(256), 0, st, idx, B, UI,
                     n_ui, GA, GB, Mc, out, status);
}

template <bool BF16>
static void dispatch_rows_fast(int lpr, const int32_t* idx, int64_t B, const char* UI,
                               int64_t n_ui, const float* GA, const float* GB, int64_t Mc,
                               float* out, int32_t* status, hipStream_t st) {
  switch (lpr) {
#define HHFM_CARS2_LPR(L) \
  case L: launch_rows_fast<L, BF16>(idx, B, UI, n_ui, GA, GB, Mc, out, status, st); break;
    HHFM_CARS2_LPR(1) HHFM_CARS2_LPR(2) HHFM_CARS2_LPR(4) HHFM_CARS2_LPR(8)
    HHFM_CARS2_LPR(16) HHFM_CARS2_LPR(32) HHFM_CARS2_LPR(64)
#undef HHFM_CARS2_LPR
  }
}

static bool cars2_sizes_ok(int64_t Mc, int D, int Dc) {
  return Mc >= 1 && D >= 1 && Dc >= 1 && Mc <= (int64_t)1 << 31 &&
         Mc * (int64_t)D <= (int64_t)1 << 40;
}

}  // namespace hhfm

using namespace hhfm;

extern "C" int hhfm_cars2_prepared_bytes(int64_t Mc, int32_t D, int32_t Dc, size_t* bytes) {
  if (!bytes || !cars2_sizes_ok(Mc, D, Dc)) return HHFM_EINVAL;
  *bytes = (size_t)(2 * Mc * D + 2 * (int64_t)D * Dc) * sizeof(float);
  return HHFM_OK;
}

extern "C" int hhfm_cars2_prepare(const float* Context, int64_t Mc, const float* W,
                                  const float* A, const float* Z, const float* Bv, int32_t D,
                                  int32_t Dc, int32_t Dp, int32_t Dq, void* prepared,
                                  size_t prepared_bytes, void* stream) {
  size_t need = 0;
  if (hhfm_cars2_prepared_bytes(Mc, D, Dc, &need) != HHFM_OK || Dp < 1 || Dq < 1)
    return HHFM_EINVAL;
  if (!Context || !W || !A || !Z || !Bv) return HHFM_EINVAL;
  if (!prepared || prepared_bytes < need) return HHFM_EWORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* GA = reinterpret_cast<float*>(prepared);
  float* GB = GA + Mc * D;
  float* WA = GB + Mc * D;
  float* ZB = WA + (int64_t)D * Dc;
  cars2_launch_fold(W, A, D, Dp, Dc, WA, st);
  cars2_launch_fold(Z, Bv, D, Dq, Dc, ZB, st);
  cars2_launch_table(WA, Context, Mc, D, Dc, GA, st);
  cars2_launch_table(ZB, Context, Mc, D, Dc, GB, st);
  return (int)hipGetLastError();
}

extern "C" int hhfm_cars2_score_rows(const int32_t* idx, int64_t B, const void* UI, int64_t n_ui,
                                     int32_t D, int32_t dtype, const void* prepared, int64_t Mc,
                                     float* out, int32_t* status, void* stream) {
  if (B < 0 || D < 1 || n_ui < 1 || Mc < 1) return HHFM_EINVAL;
  if (dtype != HHFM_F32 && dtype != HHFM_BF16) return HHFM_EINVAL;
  if (B == 0) return HHFM_OK;
  if (!idx || !UI || !prepared || !out) return HHFM_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool bf16 = dtype == HHFM_BF16;
  const float* GA = reinterpret_cast<const float*>(prepared);
  const float* GB = GA + Mc * D;
  const char* U = reinterpret_cast<const char*>(UI);
  const int lpr = cars2_lpr(D, bf16);
  // the fast kernel's 16-byte loads: UI, GA and GB rows on 16-byte boundaries
  const bool aligned = ((reinterpret_cast<uintptr_t>(UI) | reinterpret_cast<uintptr_t>(prepared)) & 15) == 0 &&
                       D % 4 == 0;
  if (lpr && aligned) {
    if (bf16) dispatch_rows_fast<true>(lpr, idx, B, U, n_ui, GA, GB, Mc, out, status, st);
    else dispatch_rows_fast<false>(lpr, idx, B, U, n_ui, GA, GB, Mc, out, status, st);
  } else {
    int64_t grid = (B + 3) / 4;
    const int64_t cap = (int64_t)stream_cu_count(st) * 8;
    if (grid > cap) grid = cap;
    if (bf16)
      hipLaunchKernelGGL(cars2_rows_generic<true>, dim3((int)grid), dim3(256), 0, st, idx, B, U,
                         n_ui, D, GA, GB, Mc, out, status);
    else
      hipLaunchKernelGGL(cars2_rows_generic<false>, dim3((int)grid), dim3(256), 0, st, idx, B, U,
                         n_ui, D, GA, GB, Mc, out, status);
  }
  return (int)hipGetLastError();
}
