// H6 — training step (`partial_fit`) for FM, HHFM, DeepFM and AFM on gfx950.
//
//   hhfm_fm_train_step    replaces sess.run((loss, optimizer)) of FM
//                         (Newcode/FM.py:123-136, 168-171)
//   hhfm_hhfm_train_step  replaces the same for OUR
//                         (Newcode/OurModel7.py:172-193, 219-228)
//   hhfm_dfm_train_step   replaces the same for DeepFM
//                         (Newcode/DFM.py:139-155, 214-217)
//   hhfm_afm_train_step   replaces the same for AFM
//                         (Newcode/AFM.py:144-156, 205-207)
//   hhfm_fm_train_step_ex / hhfm_afm_train_step_ex  the same with `--keep` < 1
//                         (tf.nn.dropout, FM.py:114, AFM.py:126 / :134) on the
//                         mask of dropout.h; hhfm_dropout_mask writes that mask
//   hhfm_fm_train_step_bn  the FM step with `--batch_norm 1` (FM.py:111-112,
//                         :160-166): batch statistics between the k-vector and
//                         its row sum ("FM with batch_norm=1" below)
//   hhfm_*_train_step_det the four steps without float atomics, every sum in a
//                         fixed order ("Deterministic ... steps" below; AFM's and
//                         DeepFM's reuse their default kernels under a DET flag)
//   hhfm_dfm_train_step_head / _head_det  DeepFM's FM-only, deep-only and logloss
//                         heads (DFM.py:131-152): the DeepFM step under a head word
//   hhfm_cars2_train_step replaces the same for CARS2 (Newcode/CARS2.py:87,
//                         :103-136, :167-170); its kernels are in cars2.hip
//   hhfm_afm_noatt_train_step / _det  AFM with `--attention 0` (AFM.py:103-148
//                         with self.attention false): FM's k-vector weighted by
//                         the prediction vector ("AFM without attention" below)
//
// One wave per batch row computes the forward score(s) and scatters the
// gradient of the row's loss into dense fp32 gradient buffers with float
// atomics (the embedding gradient is a scatter by nature; rows repeat).  The
// L2 term λ·Σ E²/2 (tf.contrib.layers.l2_regularizer) makes the embedding
// gradient dense, so — exactly like TF — the optimizer then updates the whole
// table: `optimizer_apply` applies TF's Adagrad (accumulators initialised to
// 0.1 by the caller), GradientDescent, Momentum or Adam (slots initialised to
// 0) with the sparse-gradient rules TF uses for IndexedSlices variables, and
// accumulates Σ var² of the pre-update table for the reported loss (TF
// evaluates `loss` and the update in the same run).
// Gradients of reduce_max split equally between tied maxima (TF _MaxGrad).
//
// Workspaces.  Every step keeps a block of kScalFloats scalars (`scal`, slots
// below), dense gradient buffers that the optimizer leaves zeroed, and a byte
// mask of the rows a batch touched.  The byte layouts are stated once each, in
// the plan functions: fm_train_plan (FM and HHFM), dfm_train_plan and
// afm_train_plan (their shared persistent prefix in TrainWs).  The optimizer
// tail every step ends with is optimizer_tail.
#include <hipcub/hipcub.hpp>

#include <cfloat>
#include <initializer_list>
#include <iterator>
#include <type_traits>

#include "cars2.h"
#include "dropout.h"
#include "gemm_mfma.h"
#include "hhfm_feature.h"

namespace hhfm {

// The scalar block's slots.  kScalAdam: Adam's β1^t, β2^t (kept between steps)
// and a flag that is != 0 once Adam has taken a step (a separate flag: β1^t
// underflows to exactly 0 after 828 steps (TF's flush-to-zero), and TF then
// keeps using 0, so 0 cannot also mean "not started").  finish_loss zeroes
// floats 0..3 (3 is unused) and the double of kScalLoss64.
constexpr int kScalBiasGrad = 0;   // Σ dL/d(out): the gradient of w0 / bp
constexpr int kScalDataLoss = 1;   // the batch's loss without the l2 term
constexpr int kScalSumSq = 2;      // Σ var² (pre-update) of the l2-regularised variables
constexpr int kScalLoss64 = 4;     // floats 4..6 hold one 8-byte-aligned double (scal_loss64)
constexpr int kScalAdam = 8;       // [β1^t, β2^t, started]
constexpr int kScalFloats = 16;

// The data loss of FM's dropout step, summed in double.  One wave per row adds
// its r²/2 into one scalar: 32,773 float atomics leave the sum ~6e-6 (rms) off
// in relative terms — the loss is then checked to 1e-5 — because every add
// rounds to the running sum's ulp; with the dropped forward's larger
// residuals that showed (measured up to 1.1e-5).  A double takes the same adds
// exactly enough.  It lives in the scalar block's unused floats, at whichever
// of floats 4 / 5 is 8-byte aligned (the block itself is only 4-byte aligned
// in fm_train_plan), is 0 between steps like the rest, and finish_loss adds
// it to the float slot (0 in every step that does not use it).
__host__ __device__ inline double* scal_loss64(float* scal) {
  return reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(scal + kScalLoss64) + 7) &
                                   ~uintptr_t(7));
}

// DROP: tf.nn.dropout on the k-vector FM_OUT (FM.py:114; dropout.h, site 0, the
// row index the batch row b): column c enters out as t_c / keep · bin_c and
// its gradient carries the same factor; a dropped column scatters nothing.
template <bool DROP>
__global__ __launch_bounds__(256) void fm_train_rows(
    const int32_t* __restrict__ idx, const float* __restrict__ y, int64_t B, int F,
    const float* __restrict__ E, const float* __restrict__ w, const float* __restrict__ w0,
    int64_t M, int k, float* __restrict__ dE, float* __restrict__ dw, float* __restrict__ scal,
    DropoutArgs dr) {
  const int l = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t b = wave; b < B; b += nwave) {
    const int32_t* x = idx + b * F;
    float t = 0.f;
    [[maybe_unused]] LaneDropout ld;
    for (int c = l; c < k; c += kWave) {
      float s = 0.f, q = 0.f;
      for (int f = 0; f < F; ++f) {
        const float v = E[(int64_t)clamp_id(x[f], M) * k + c];
        s += v;
        q += v * v;
      }
      if constexpr (DROP)
        t += 0.5f * (s * s - q) / dr.keep0 * ld.binary(dr, dr.keep0, kDropSiteFm, b, c);
      else
        t += 0.5f * (s * s - q);
    }
    t = group_sum<kWave>(t);
    float fb = 0.f;
    for (int f = 0; f < F; ++f) fb += w[clamp_id(x[f], M)];
    const float out = (t + fb) + w0[0];
    const float r = y[b] - out;        // l2_loss(y - out) = r²/2   FM.py:124
    const float g = -r;                // d/d out
    for (int c = l; c < k; c += kWave) {
      float gc = g;
      if constexpr (DROP) {
        const float bin = ld.binary(dr, dr.keep0, kDropSiteFm, b, c);
        if (bin == 0.f) continue;
        gc = g * bin / dr.keep0;
      }
      float s = 0.f;
      for (int f = 0; f < F; ++f) s += E[(int64_t)clamp_id(x[f], M) * k + c];
      for (int f = 0; f < F; ++f) {
        const int64_t id = clamp_id(x[f], M);
        atomicAdd(dE + id * k + c, gc * (s - E[id * k + c]));   // ∂out/∂e_f = Σe − e_f
      }
    }
    for (int f = l; f < F; f += kWave) atomicAdd(dw + clamp_id(x[f], M), g);
    if (l == 0) {
      atomicAdd(scal + kScalBiasGrad, g);
      if constexpr (DROP)
        atomicAdd(scal_loss64(scal), 0.5 * ((double)r * (double)r));
      else
        atomicAdd(scal + kScalDataLoss, 0.5f * r * r);
    }
  }
}

// HHFM: loss_b = -log σ(pos - max_j neg_j) with h from the feature policy
// (hhfm_feature.h: SumFeature h = u + Σctx (+ Σtime) or TwoWayFeature — the
// scoring kernels' h bit for bit; the pooled step is hhfm_train_rows_pool
// below).  The BPR part — reduce_max over the negatives with ties split, g,
// gt, dh — is stated here for the default, the deterministic and the two-way
// step; each instantiation is a kernel of its own and keeps its code and
// registers.
// DET = false: the item and negative scatters, Feature::back's per-row values
// and the loss are float atomics into dE / scal (gb .. HV are null and unused).
// DET = true (hhfm_hhfm_train_step_det): no atomics, dE / scal unused — per
// row g (gb), gt = g / ties (gtb), bit j of the mask = negative j is a tied
// maximum (maskb), h[c] and dh[c] = g·it − gt·nsum (HV [B][2k]: h, then dh)
// and the loss −log σ(z) in double (lossb) are stored for det_scatter; back is
// never called.
template <class Feature, bool DET>
__global__ __launch_bounds__(256) void hhfm_train_rows(
    const int32_t* __restrict__ X, const int32_t* __restrict__ Neg, int64_t B, int ncols,
    int c0, int c1, int t0, int t1, int NG, const float* __restrict__ E, int64_t M, int k,
    Feature feat, float* __restrict__ dE, float* __restrict__ scal, float* __restrict__ gb,
    float* __restrict__ gtb, uint32_t* __restrict__ maskb, double* __restrict__ lossb,
    float* __restrict__ HV) {
  const int l = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t b = wave; b < B; b += nwave) {
    const int32_t* x = X + b * ncols;
    const int32_t* ng = Neg + b * NG;
    const int64_t iu = clamp_id(x[kUserCol], M), ii = clamp_id(x[kItemCol], M);
    auto fwd = [&](int c) {
      return feat.forward(
          E[iu * k + c], [&](int j) { return E[(int64_t)clamp_id(x[j], M) * k + c]; }, c0, c1, t0,
          t1);
    };
    float pos = 0.f;
    for (int c = l; c < k; c += kWave) pos += fwd(c).h * E[ii * k + c];
    pos = group_sum<kWave>(pos);                        // PositiveFeadback  :171
    // NegativeFeadback (:172) for up to kMaxNeg negatives, kept in registers
    float negv[kMaxNeg];
    float mx = -__builtin_huge_valf();
#pragma unroll
    for (int j = 0; j < kMaxNeg; ++j) {
      negv[j] = -__builtin_huge_valf();
      if (j < NG) {
        float v = 0.f;
        const int64_t in = clamp_id(ng[j], M);
        for (int c = l; c < k; c += kWave) v += fwd(c).h * E[in * k + c];
        v = group_sum<kWave>(v);
        negv[j] = v;
        mx = fmaxf(mx, v);
      }
    }
    // ties of the max share its gradient (reduce_max, :174)
    int nt = 0;
    [[maybe_unused]] uint32_t tied = 0;
#pragma unroll
    for (int j = 0; j < kMaxNeg; ++j) {
      nt += (j < NG && negv[j] == mx);
      if constexpr (DET) tied |= (uint32_t)(j < NG && negv[j] == mx) << j;
    }
    const float z = pos - mx;
    const float sg = 1.f / (1.f + expf(-z));
    const float g = sg - 1.f;                           // d(-log σ(z))/dz      :178
    const float gt = g / (float)nt;
    for (int c = l; c < k; c += kWave) {
      const auto f = fwd(c);
      const float it = E[ii * k + c];
      float nsum = 0.f;
#pragma unroll
      for (int j = 0; j < kMaxNeg; ++j)
        if (j < NG && negv[j] == mx) nsum += E[(int64_t)clamp_id(ng[j], M) * k + c];
      const float dh = g * it - gt * nsum;
      if constexpr (DET) {
        HV[b * 2 * k + c] = f.h;
        HV[b * 2 * k + k + c] = dh;
      } else {
        atomicAdd(dE + ii * k + c, g * f.h);
#pragma unroll
        for (int j = 0; j < kMaxNeg; ++j)
          if (j < NG && negv[j] == mx)
            atomicAdd(dE + (int64_t)clamp_id(ng[j], M) * k + c, -gt * f.h);
        feat.back(
            f, dh, E[iu * k + c], [&](int j) { return E[(int64_t)clamp_id(x[j], M) * k + c]; }, c0,
            c1, t0, t1,
            [&](int j, float v) { atomicAdd(dE + (int64_t)clamp_id(x[j], M) * k + c, v); });
      }
    }
    if constexpr (DET) {
      if (l == 0) {
        gb[b] = g;
        gtb[b] = gt;
        maskb[b] = tied;
        lossb[b] = (double)-logf(sg);
      }
    } else {
      if (l == 0) atomicAdd(scal + kScalDataLoss, -logf(sg));
    }
  }
}

// HHFM with MAX / MEAN pooling (include/hhfm.h "Pooling"): the same step with
// PoolFeature's forward (the scoring kernels' h bit for bit) and TF's pool
// gradients on the way back: dh_e reaches the stack members through the final
// pool and the context / time rows through theirs (pool_grad: max shares
// between the values equal to the maximum at that element, mean divides by
// the count).  Kept as a kernel of its own, with its own copy of the BPR part
// (reduce_max over the negatives with ties split, g, gt, the loss — a change
// to hhfm_train_rows's is made here too): as an instantiation of the skeleton
// above its (max, max, max) step measured 0.5 % slower than this kernel
// (profiles/hybrid_feature_time.txt).
__global__ __launch_bounds__(256) void hhfm_train_rows_pool(
    const int32_t* __restrict__ X, const int32_t* __restrict__ Neg, int64_t B, int ncols,
    int c0, int c1, int t0, int t1, int NG, const float* __restrict__ E, int64_t M, int k,
    PoolModes pm, float* __restrict__ dE, float* __restrict__ scal) {
  const int l = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int nc = c1 > c0 ? c1 - c0 : 0, ntm = t1 > t0 ? t1 - t0 : 0;
  const int members = 1 + (nc > 0) + (ntm > 0);
  for (int64_t b = wave; b < B; b += nwave) {
    const int32_t* x = X + b * ncols;
    const int32_t* ng = Neg + b * NG;
    const int64_t iu = clamp_id(x[0], M), ii = clamp_id(x[1], M);
    auto row = [&](int j, int c) { return E[(int64_t)clamp_id(x[j], M) * k + c]; };
    // h at element c; cv / tv: the pools' values (a max pool's value is its maximum)
    auto hval = [&](int c, float& cv, float& tv) {
      cv = pool_identity(pm.ctx);
      tv = pool_identity(pm.tim);
      for (int j = c0; j < c1; ++j) cv = pool_step(pm.ctx, cv, row(j, c));
      for (int j = t0; j < t1; ++j) tv = pool_step(pm.tim, tv, row(j, c));
      cv = pool_finish(pm.ctx, cv, nc);
      tv = pool_finish(pm.tim, tv, ntm);
      return pool_h(E[iu * k + c], cv, nc, tv, ntm, pm.fin);
    };
    auto h_only = [&](int c) {
      float cv, tv;
      return hval(c, cv, tv);
    };
    float pos = 0.f;
    for (int c = l; c < k; c += kWave) pos += h_only(c) * E[ii * k + c];
    pos = group_sum<kWave>(pos);                        // PositiveFeadback  :171
    float negv[kMaxNeg];
    float mx = -__builtin_huge_valf();
#pragma unroll
    for (int j = 0; j < kMaxNeg; ++j) {
      negv[j] = -__builtin_huge_valf();
      if (j < NG) {
        float v = 0.f;
        const int64_t in = clamp_id(ng[j], M);
        for (int c = l; c < k; c += kWave) v += h_only(c) * E[in * k + c];
        v = group_sum<kWave>(v);
        negv[j] = v;
        mx = fmaxf(mx, v);
      }
    }
    int nt = 0;
#pragma unroll
    for (int j = 0; j < kMaxNeg; ++j) nt += (j < NG && negv[j] == mx);
    const float z = pos - mx;
    const float sg = 1.f / (1.f + expf(-z));
    const float g = sg - 1.f;                           // d(-log σ(z))/dz      :178
    const float gt = g / (float)nt;
    for (int c = l; c < k; c += kWave) {
      float cv, tv;
      const float h = hval(c, cv, tv);
      const float u = E[iu * k + c];
      const float it = E[ii * k + c];
      float nsum = 0.f;
#pragma unroll
      for (int j = 0; j < kMaxNeg; ++j)
        if (j < NG && negv[j] == mx) nsum += E[(int64_t)clamp_id(ng[j], M) * k + c];
      const float dh = g * it - gt * nsum;
      atomicAdd(dE + ii * k + c, g * h);
#pragma unroll
      for (int j = 0; j < kMaxNeg; ++j)
        if (j < NG && negv[j] == mx) atomicAdd(dE + (int64_t)clamp_id(ng[j], M) * k + c, -gt * h);
      if (members == 1) {                               // h = u under every mode
        atomicAdd(dE + iu * k + c, dh);
        continue;
      }
      // the final pool: with max, h is the largest member (bit-equal to it)
      const int feq = (u == h) + (nc > 0 && cv == h) + (ntm > 0 && tv == h);
      atomicAdd(dE + iu * k + c, pool_grad(pm.fin, dh, u, h, feq, members));
      if (nc > 0) {
        const float dc = pool_grad(pm.fin, dh, cv, h, feq, members);
        int eq = 0;
        for (int j = c0; j < c1; ++j) eq += row(j, c) == cv;
        for (int j = c0; j < c1; ++j)
          atomicAdd(dE + (int64_t)clamp_id(x[j], M) * k + c,
                    pool_grad(pm.ctx, dc, row(j, c), cv, eq, nc));
      }
      if (ntm > 0) {
        const float dt = pool_grad(pm.fin, dh, tv, h, feq, members);
        int eq = 0;
        for (int j = t0; j < t1; ++j) eq += row(j, c) == tv;
        for (int j = t0; j < t1; ++j)
          atomicAdd(dE + (int64_t)clamp_id(x[j], M) * k + c,
                    pool_grad(pm.tim, dt, row(j, c), tv, eq, ntm));
      }
    }
    if (l == 0) atomicAdd(scal + kScalDataLoss, -logf(sg));
  }
}

// One TF-1.x optimizer step on a variable (training_ops.cc semantics, fp32):
//   Adagrad   accum += g²; var -= lr·g·rsqrt(accum)           (ApplyAdagrad)
//   SGD       var -= lr·g                                      (ApplyGradientDescent)
//   Momentum  accum = accum·0.95 + g; var -= accum·lr           (ApplyMomentum,
//             momentum 0.95 as FM.py:136); a SPARSE variable (its gradient an
//             IndexedSlices: embedding_lookup without a dense l2 term) updates
//             only the rows the batch touched (SparseApplyMomentum)
//   Adam      β1 0.9, β2 0.999, ε 1e-8 (FM.py:130), α = lr·√(1−β2^t)/(1−β1^t):
//             dense  m += (g−m)(1−β1); v += (g²−v)(1−β2); var -= m·α/(√v+ε)
//             (ApplyAdam); sparse (AdamOptimizer._apply_sparse_shared)
//             m = m·β1 + g(1−β1); v = v·β2 + g²(1−β2) on every row, the same
//             var update — the two differ only in rounding
// g = grad + λ·var; Σ var² (pre-update) accumulated into *sumsq when given.
// state: Adagrad / Momentum n floats, Adam 2n (m, then v).  pw: the step's
// β1^t, β2^t (TF's beta1_power / beta2_power) and the started flag pw[2]
// (0 = the first step, whose powers are β1, β2).
constexpr float kMomentum = 0.95f, kBeta1 = 0.9f, kBeta2 = 0.999f, kAdamEps = 1e-8f;

struct OptStep {
  int opt;
  float lr;
  const float* pw;         // Adam: [β1^t, β2^t, started] (device)
  const uint8_t* touched;  // sparse Momentum: rows the batch touched (else null)
  int rowlen;              // elements per row of the variable (touched index = i / rowlen)
  int sparse;              // the variable's TF gradient is an IndexedSlices
};

// ORDERED (the deterministic steps): `sumsq` is an array and every wave stores
// its partial at its global wave index — the grid is a function of n alone —
// for det_sumsq to add in ascending index; else one float atomic per wave.
template <bool ORDERED>
__global__ __launch_bounds__(256) void optimizer_apply(float* __restrict__ var,
                                                       float* __restrict__ grad,
                                                       float* __restrict__ state, int64_t n,
                                                       float lam, OptStep o,
                                                       float* __restrict__ sumsq) {
  float alpha = 0.f;
  if (o.opt == HHFM_OPT_ADAM) {
    const bool started = o.pw[2] != 0.f;
    const float b1p = started ? o.pw[0] : kBeta1;
    const float b2p = started ? o.pw[1] : kBeta2;
    alpha = o.lr * sqrtf(1.f - b2p) / (1.f - b1p);
  }
  float ss = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float v = var[i];
    ss += v * v;
    const float g = grad[i] + lam * v;
    if (o.opt == HHFM_OPT_ADAGRAD) {
      const float a = state[i] + g * g;
      state[i] = a;
      var[i] = v - o.lr * g * rsqrtf(a);
    } else if (o.opt == HHFM_OPT_SGD) {
      var[i] = v - o.lr * g;
    } else if (o.opt == HHFM_OPT_MOMENTUM) {
      if (!o.sparse || o.touched[i / o.rowlen]) {
        const float a = state[i] * kMomentum + g;
        state[i] = a;
        var[i] = v - a * o.lr;
      }
    } else {
      float m = state[i], vv = state[n + i];
      if (o.sparse) {
        m = m * kBeta1 + g * (1.f - kBeta1);
        vv = vv * kBeta2 + (g * g) * (1.f - kBeta2);
      } else {
        m += (g - m) * (1.f - kBeta1);
        vv += (g * g - vv) * (1.f - kBeta2);
      }
      state[i] = m;
      state[n + i] = vv;
      var[i] = v - (m * alpha) / (sqrtf(vv) + kAdamEps);
    }
    grad[i] = 0.f;   // leave the gradient buffer zeroed for the next step
  }
  if (sumsq) {
    ss = group_sum<kWave>(ss);
    if ((threadIdx.x & 63) == 0) {
      if constexpr (ORDERED)
        sumsq[((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave] = ss;
      else
        atomicAdd(sumsq, ss);
    }
  }
}

// Σvar² of a deterministic step: the waves' partials added in ascending index
// in double by one thread (the others stage them through LDS), rounded once.
constexpr int kDetStage = 4096;

__global__ __launch_bounds__(256) void det_sumsq(const float* __restrict__ part, int64_t n,
                                                 float* __restrict__ out) {
  __shared__ float buf[kDetStage];
  double s = 0.0;
  for (int64_t base = 0; base < n; base += kDetStage) {
    const int m = (int)(n - base < kDetStage ? n - base : kDetStage);
    for (int j = threadIdx.x; j < m; j += blockDim.x) buf[j] = part[base + j];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int j = 0; j < m; ++j) s += (double)buf[j];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)s;
}

// after every variable's update: β1^t, β2^t -> β1^(t+1), β2^(t+1) (AdamOptimizer._finish).
// TF runs the product with flush-to-zero set (its CPU thread pools set FTZ/DAZ,
// core/lib/core/threadpool.cc), so β1^t reaches exactly 0 at t = 829 and stays
// there; the flush is explicit here, whatever the kernel's denormal mode.
__device__ __forceinline__ float ftz(float x) { return fabsf(x) < FLT_MIN ? 0.f : x; }

__global__ void adam_advance(float* pw) {
  const bool started = pw[2] != 0.f;
  pw[0] = ftz((started ? pw[0] : kBeta1) * kBeta1);
  pw[1] = ftz((started ? pw[1] : kBeta2) * kBeta2);
  pw[2] = 1.f;
}

// touched[x] = val for every id of the batch (rows of a sparse variable the
// step updates under Momentum); plain byte stores, equal values
__global__ __launch_bounds__(256) void mark_rows(const int32_t* __restrict__ idx, int64_t n,
                                                 int64_t M, uint8_t* __restrict__ touched,
                                                 uint8_t val) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    touched[clamp_id(idx[i], M)] = val;
}

__global__ void finish_loss(float* scal, float lam, float* loss) {
  double* l64 = scal_loss64(scal);
  const float data = (float)((double)scal[kScalDataLoss] + *l64);
  loss[0] = data + lam * 0.5f * scal[kScalSumSq];   // + l2_regularizer(λ)(var)
  scal[0] = scal[1] = scal[2] = scal[3] = 0.f;
  *l64 = 0.0;
}

static int grid_for_n(int64_t n) {
  int64_t g = (n + 255) / 256;
  return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

// waves of optimizer_apply's grid over n elements = Σvar² partials it stores when ORDERED
static int64_t det_sumsq_floats(int64_t n) { return (int64_t)grid_for_n(n) * (256 / kWave); }

static bool opt_ok(int opt) {
  return opt == HHFM_OPT_ADAGRAD || opt == HHFM_OPT_SGD || opt == HHFM_OPT_MOMENTUM ||
         opt == HHFM_OPT_ADAM;
}

// the optimizer's slot arrays: `acc` holds n non-null entries, unless SGD (which keeps none)
static bool slots_ok(int opt, float* const* acc, int n) {
  if (opt == HHFM_OPT_SGD) return true;
  if (!acc) return false;
  for (int i = 0; i < n; ++i)
    if (!acc[i]) return false;
  return true;
}

static float* slot_of(int opt, float* const* acc, int i) {
  return opt != HHFM_OPT_SGD ? acc[i] : nullptr;
}

// One variable of a step, as the optimizer tail sees it.
struct OptVar {
  float* var;
  float* grad;    // dense gradient buffer, n floats; left zeroed
  float* slot;    // the optimizer's slot array (null under SGD)
  int64_t n;
  float lam;      // g = grad + lam·var
  int rowlen;     // elements per table row (the touched mask's index is i / rowlen)
  bool sparse;    // the variable's TF gradient is an IndexedSlices
  bool sumsq;     // Σ var² (pre-update) goes into the loss's l2 term
  // a sparse variable indexed by ids other than the tail's `ids` (CARS2's
  // Context): its own touched mask, marked and cleared by the caller
  const uint8_t* own_touched = nullptr;
};

struct IdList {
  const int32_t* ids;
  int64_t n;
};

// What every step ends with: under Momentum the rows of `ids` are marked in
// `touched` for the sparse variables (and unmarked afterwards: the mask is
// left zeroed), one optimizer_apply per variable in list order, Adam's powers
// advance, and finish_loss writes loss = data loss + loss_lam·Σvar²/2 and
// clears the scalars.  With `ss_part` (the deterministic steps; one float per
// wave of every sumsq variable's grid, det_sumsq_floats) Σvar² is the ordered
// sum of det_sumsq instead of float atomics.  Returns hipGetLastError().
static int optimizer_tail(const OptVar* vars, int nvars, std::initializer_list<IdList> ids,
                          int64_t M, int opt, float lr, float* scal, uint8_t* touched,
                          float loss_lam, float* loss, hipStream_t st,
                          float* ss_part = nullptr) {
  bool mark = false;
  for (int i = 0; i < nvars; ++i) mark |= opt == HHFM_OPT_MOMENTUM && vars[i].sparse;
  auto set_mask = [&](uint8_t val) {
    for (const IdList& l : ids)
      if (mark && l.n > 0)   // an empty batch touches no row
        hipLaunchKernelGGL(mark_rows, dim3(grid_for_n(l.n)), dim3(256), 0, st, l.ids, l.n, M,
                           touched, val);
  };
  set_mask(1);
  int64_t nss = 0;   // partials written so far
  for (int i = 0; i < nvars; ++i) {
    const OptVar& v = vars[i];
    const uint8_t* mask = v.own_touched ? v.own_touched : touched;
    OptStep o{opt, lr, scal + kScalAdam, v.sparse ? mask : nullptr, v.rowlen, v.sparse ? 1 : 0};
    if (ss_part) {
      hipLaunchKernelGGL(optimizer_apply<true>, dim3(grid_for_n(v.n)), dim3(256), 0, st, v.var,
                         v.grad, v.slot, v.n, v.lam, o, v.sumsq ? ss_part + nss : nullptr);
      if (v.sumsq) nss += det_sumsq_floats(v.n);
    } else {
      hipLaunchKernelGGL(optimizer_apply<false>, dim3(grid_for_n(v.n)), dim3(256), 0, st, v.var,
                         v.grad, v.slot, v.n, v.lam, o, v.sumsq ? scal + kScalSumSq : nullptr);
    }
  }
  if (nss > 0)
    hipLaunchKernelGGL(det_sumsq, dim3(1), dim3(256), 0, st, ss_part, nss, scal + kScalSumSq);
  set_mask(0);
  if (opt == HHFM_OPT_ADAM)
    hipLaunchKernelGGL(adam_advance, dim3(1), dim3(1), 0, st, scal + kScalAdam);
  hipLaunchKernelGGL(finish_loss, dim3(1), dim3(1), 0, st, scal, loss_lam, loss);
  return (int)hipGetLastError();
}

// The FM / HHFM workspace: dE [M·k] | dw [M] | scal [kScalFloats] floats, then
// the touched mask, M bytes rounded up to 256.  Zero-filled once by the caller.
struct FmTrainPlan {
  int64_t off_dE, off_dw, off_scal, off_touch;   // floats
  size_t bytes;
};

static FmTrainPlan fm_train_plan(int64_t M, int k) {
  FmTrainPlan p;
  p.off_dE = 0;
  p.off_dw = M * k;
  p.off_scal = p.off_dw + M;
  p.off_touch = p.off_scal + kScalFloats;
  p.bytes = (size_t)p.off_touch * 4 + (((size_t)M + 255) & ~size_t(255));
  return p;
}

// ---------------------------------------------------------------------------
// Deterministic FM / HHFM steps (hhfm_fm_train_step_det, hhfm_hhfm_train_step_det):
// no float atomics, every sum's order a function of the batch alone
// (include/hhfm.h "Deterministic training steps" states the orders).
//   row pass      *_train_rows_det: the forward of the row kernels above, one
//                 wave per row, which STORES per row what the scatter needs
//                 (FM: g, S[c] = Σ_f E[x_f][c]; HHFM: g, gt, the tie mask,
//                 h[c], dh[c]) and the row's loss
//   grouping      det_keys -> a stable radix sort of (clamped id, occurrence
//                 o = b·S + slot) -> det_runs: the first position of every
//                 distinct id (compacted with an integer atomic: the order of
//                 the run list decides nothing)
//   segment pass  det_segments<C>: one wave per distinct id walks the id's
//                 occurrences in ascending o and adds their contributions in
//                 fp32, lane = column; one plain store per element of dE / dw
//   scalars       det_scalars (g and the loss), det_sumsq (Σvar²)
// The contribution of an occurrence is a functor C (FmContrib, HhfmContrib;
// StoredContrib for AFM and DeepFM, whose scatter kernels' DET instantiations
// are the row pass of their table gradient and whose head kernels' DET
// instantiations store per-row values that det_columns adds in the scalar
// order).
// ---------------------------------------------------------------------------
static size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

static int det_key_bits(int64_t M) {
  int b = 1;
  while (b < 31 && (int64_t(1) << b) < M) ++b;
  return b;
}

// Byte offsets of the per-batch scratch (nothing in it outlives a step).
struct DetPlan {
  int n, bits;   // occurrences B·S, key bits of the sort
  size_t keys_in, keys_out, vals_in, vals_out, runs, nruns, rowvec, g, gt, mask, loss, sspart,
      tmp, tmp_bytes, bias, heads, bytes;
};

// rowvec_f / ss_f: floats of the per-row (or per-occurrence) vectors and of
// the Σvar² partials; bias_f / heads_f: the AFM / DeepFM steps' per-occurrence
// dw values and per-row head values (0 for FM / HHFM).
static bool det_plan_regions(int64_t B, int S, int64_t M, int64_t rowvec_f, int64_t ss_f,
                             int64_t bias_f, int64_t heads_f, DetPlan& p) {
  if (B < 0 || S < 1 || M < 1) return false;
  if (B > 0x7fffffff || B * S > 0x7fffffff) return false;   // the sort counts in int
  p = DetPlan{};
  p.n = (int)(B * S);
  p.bits = det_key_bits(M);
  // The sort's temporary storage.  hipCUB's own size query needs a device (it
  // picks a tuning by architecture) and this plan must not, so an upper bound
  // is reserved instead: a second copy of the n keys and of the n values
  // (8n bytes), one 4-byte look-back state per digit and block of >= 256
  // items (<= 4n + 1 KiB) and at most 32 histograms of 256 8-byte bins
  // (64 KiB), with slack.  det_scatter asks hipCUB for the real figure and
  // refuses the step should it ever be larger.
  p.tmp_bytes = p.n > 0 ? 16 * (size_t)p.n + (size_t(256) << 10) : 0;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t r = off;
    off += al256(bytes);
    return r;
  };
  p.keys_in = take((size_t)p.n * 4);
  p.keys_out = take((size_t)p.n * 4);
  p.vals_in = take((size_t)p.n * 4);
  p.vals_out = take((size_t)p.n * 4);
  p.runs = take((size_t)p.n * 4);
  p.nruns = take(4);
  p.rowvec = take((size_t)rowvec_f * 4);
  p.g = take((size_t)B * 4);
  p.gt = take((size_t)B * 4);
  p.mask = take((size_t)B * 4);
  p.loss = take((size_t)B * 8);
  p.sspart = take((size_t)ss_f * 4);
  p.tmp = take(p.tmp_bytes);
  p.bias = take((size_t)bias_f * 4);
  p.heads = take((size_t)heads_f * 4);
  p.bytes = off;
  return true;
}

// FM / HHFM: the row vectors are FM's [B][k] or HHFM's [B][2k]; Σvar² over the table
static bool det_plan(int64_t B, int S, int k, int64_t M, DetPlan& p) {
  if (k < 1 || B < 0 || M < 1) return false;
  return det_plan_regions(B, S, M, B * 2 * k, det_sumsq_floats(M * k), 0, 0, p);
}

// FM's row pass: fm_train_rows's forward (the same expressions in the same
// order), then S_b[c] = Σ_f E[x_f][c] (Sb [B][k]; under dropout the mask's
// bin_b[c] follows it, [B][k] more), g_b and the row's loss r²/2 stored.
template <bool DROP>
__global__ __launch_bounds__(256) void fm_train_rows_det(
    const int32_t* __restrict__ idx, const float* __restrict__ y, int64_t B, int F,
    const float* __restrict__ E, const float* __restrict__ w, const float* __restrict__ w0,
    int64_t M, int k, float* __restrict__ gb, double* __restrict__ lossb,
    float* __restrict__ Sb, DropoutArgs dr) {
  const int l = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t b = wave; b < B; b += nwave) {
    const int32_t* x = idx + b * F;
    float t = 0.f;
    [[maybe_unused]] LaneDropout ld;
    for (int c = l; c < k; c += kWave) {
      float s = 0.f, q = 0.f;
      for (int f = 0; f < F; ++f) {
        const float v = E[(int64_t)clamp_id(x[f], M) * k + c];
        s += v;
        q += v * v;
      }
      if constexpr (DROP) {
        const float bin = ld.binary(dr, dr.keep0, kDropSiteFm, b, c);
        t += 0.5f * (s * s - q) / dr.keep0 * bin;
        Sb[(B + b) * k + c] = bin;
      } else {
        t += 0.5f * (s * s - q);
      }
      Sb[b * k + c] = s;
    }
    t = group_sum<kWave>(t);
    float fb = 0.f;
    for (int f = 0; f < F; ++f) fb += w[clamp_id(x[f], M)];
    const float out = (t + fb) + w0[0];
    const float r = y[b] - out;
    if (l == 0) {
      gb[b] = -r;
      lossb[b] = 0.5 * ((double)r * (double)r);
    }
  }
}

// Where the id of occurrence (b, slot) comes from.  FM (Neg null): slot = the
// field, S = ncols.  HHFM: item, negatives 0..NG-1, user, context columns,
// time columns — the order hhfm_train_rows scatters in.
struct OccSource {
  const int32_t* X;
  const int32_t* Neg;
  int ncols, NG, c0, c1, t0, t1;
};

HHFM_DEV int32_t occ_id(const OccSource& s, int64_t b, int slot) {
  const int32_t* x = s.X + b * s.ncols;
  if (!s.Neg) return x[slot];
  if (slot == 0) return x[1];
  if (slot <= s.NG) return s.Neg[b * s.NG + slot - 1];
  if (slot == s.NG + 1) return x[0];
  const int j = slot - s.NG - 2, nc = s.c1 - s.c0;
  return x[j < nc ? s.c0 + j : s.t0 + (j - nc)];
}

// keys[o] = the clamped id of occurrence o, vals[o] = o; clears the run counter
__global__ __launch_bounds__(256) void det_keys(OccSource s, int S, int n, int64_t M,
                                                uint32_t* __restrict__ keys,
                                                int32_t* __restrict__ vals,
                                                int32_t* __restrict__ nruns) {
  if (blockIdx.x == 0 && threadIdx.x == 0) nruns[0] = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / S);
    keys[i] = (uint32_t)clamp_id(occ_id(s, b, (int)(i - (int64_t)b * S)), M);
    vals[i] = (int32_t)i;
  }
}

// runs[...] = every position of the sorted keys at which a new id starts
__global__ __launch_bounds__(256) void det_runs(const uint32_t* __restrict__ keys, int n,
                                                int32_t* __restrict__ runs,
                                                int32_t* __restrict__ nruns) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    if (i == 0 || keys[i] != keys[i - 1]) runs[atomicAdd(nruns, 1)] = (int32_t)i;
}

// the value lane `lane` (wave-uniform) holds
HHFM_DEV int lane_i(int x, int lane) { return __builtin_amdgcn_readlane(x, lane); }
HHFM_DEV float lane_f(float x, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}

// A contribution functor C tells det_segments what an occurrence adds:
//   Occ load(o)            the occurrence's row data (each lane loads another o)
//   Occ lane(occ, u)       lane u's Occ in every lane
//   bool value(occ, c, e, out)   the contribution to column c of the id's row
//                          (e = E[id][c]); false = it adds nothing.  No
//                          branch: det_segments issues a group's loads together
//   kBias, bias(occ)       the contribution to dw[id], where the model has one
//
// FM's, o = b·F + f: gc·(S_b[c] − e), gc = g_b (· bin / keep under dropout, the
// row pass's mask read back; a dropped column adds nothing); dw: g_b.
template <bool DROP>
struct FmContrib {
  static constexpr bool kBias = true;
  const float* g;
  const float* S;   // S [B][k], then (DROP) bin [B][k]
  int64_t B;
  int F, k;
  float keep;
  struct Occ {
    int b;
    float g;
  };
  HHFM_DEV Occ load(int o) const {
    const int b = o / F;
    return Occ{b, g[b]};
  }
  HHFM_DEV Occ lane(const Occ& oc, int u) const { return Occ{lane_i(oc.b, u), lane_f(oc.g, u)}; }
  HHFM_DEV float bias(const Occ& oc) const { return oc.g; }
  HHFM_DEV bool value(const Occ& oc, int c, float e, float& out) const {
#pragma clang fp contract(off)
    float gc = oc.g;
    bool kept = true;
    if constexpr (DROP) {
      const float bin = S[((int64_t)B + oc.b) * k + c];
      kept = bin != 0.f;
      gc = oc.g * bin / keep;
    }
    out = gc * (S[(int64_t)oc.b * k + c] - e);
    return kept;
  }
};

// HHFM's, o = b·S + slot: slot 0 (item) g·h; slots 1..NG (negative j) −gt·h
// when j is a tied maximum, else nothing; the other slots dh.
struct HhfmContrib {
  static constexpr bool kBias = false;
  const float* g;
  const float* gt;
  const uint32_t* mask;
  const float* HV;
  int S, NG, k;
  enum { kNothing = 0, kTimesH = 1, kDh = 2 };
  struct Occ {
    int b, kind;
    float coef;   // what multiplies h
  };
  HHFM_DEV Occ load(int o) const {
    const int b = o / S, slot = o - b * S;
    if (slot == 0) return Occ{b, kTimesH, g[b]};
    if (slot <= NG) return Occ{b, (int)((mask[b] >> (slot - 1)) & 1u), -gt[b]};
    return Occ{b, kDh, 0.f};
  }
  HHFM_DEV Occ lane(const Occ& oc, int u) const {
    return Occ{lane_i(oc.b, u), lane_i(oc.kind, u), lane_f(oc.coef, u)};
  }
  HHFM_DEV float bias(const Occ&) const { return 0.f; }
  HHFM_DEV bool value(const Occ& oc, int c, float, float& out) const {
#pragma clang fp contract(off)
    const float v = HV[(int64_t)oc.b * 2 * k + (oc.kind == kDh ? k : 0) + c];
    out = oc.kind == kDh ? v : oc.coef * v;
    return oc.kind != kNothing;
  }
};

// AFM's and DeepFM's, o = b·F + f: the det instantiation of the model's
// scatter kernel stored what the default one hands to atomicAdd — V[o][c] for
// dE and wb[o] for dw (AFM g_b, DeepFM g_b·Wp[f]) — so an occurrence's
// contribution is one load, whatever the model.
struct StoredContrib {
  static constexpr bool kBias = true;
  const float* V;    // [B·F][k]
  const float* wb;   // [B·F]
  int k;
  struct Occ {
    int o;
    float wb;
  };
  HHFM_DEV Occ load(int o) const { return Occ{o, wb[o]}; }
  HHFM_DEV Occ lane(const Occ& oc, int u) const { return Occ{lane_i(oc.o, u), lane_f(oc.wb, u)}; }
  HHFM_DEV float bias(const Occ& oc) const { return oc.wb; }
  HHFM_DEV bool value(const Occ& oc, int c, float, float& out) const {
    out = V[(int64_t)oc.o * k + c];
    return true;
  }
};

// One wave per distinct id (grid-stride over the run list), lane = column
// (strided for k > 64).  The id's occurrences lie consecutively in `vals`, in
// ascending o.  The wave takes 64 at a time: lane u loads occurrence u's row
// data (the next 64 are requested before these are consumed), then the
// occurrences are visited in order, kDetAhead at a time: their row vectors
// are loaded together — the addresses come from the sorted list — and only
// the chain of fp32 adds acc = acc + contribution is serial, the first
// contribution starting the sum.  An id whose occurrences all add nothing
// stores 0.
constexpr int kDetAhead = 32;

template <class C>
__global__ __launch_bounds__(256) void det_segments(
    const uint32_t* __restrict__ keys, const int32_t* __restrict__ vals, int n,
    const int32_t* __restrict__ runs, const int32_t* __restrict__ nruns,
    const float* __restrict__ E, int k, float* __restrict__ dE, float* __restrict__ dw,
    C contrib) {
  using Occ = typename C::Occ;
  const int l = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) / kWave);
  const int nwave = (int)((gridDim.x * blockDim.x) / kWave);
  const int nr = nruns[0];
  for (int r = wave; r < nr; r += nwave) {
    const int start = __builtin_amdgcn_readfirstlane(runs[r]);
    const uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane((int)keys[start]);
    // lane l's occurrence of the 64 from `base`; -> how many of them are the id's
    auto fetch = [&](int64_t base, Occ& mine) {
      const int64_t j = base + l;
      const bool ok = j < n && keys[j] == id;
      mine = contrib.load(ok ? vals[j] : 0);
      return (int)__popcll(__ballot(ok));   // the id's occurrences are a prefix
    };
    for (int cb = 0; cb < k; cb += kWave) {
      const int c = cb + l;
      const bool live = c < k;
      const float e = live ? E[(int64_t)id * k + c] : 0.f;
      float acc = 0.f, accw = 0.f;
      bool have = false, havew = false;
      Occ mine, next;
      int cnt = fetch(start, mine);
      for (int64_t base = start;; base += kWave) {
        const int cntn = cnt == kWave ? fetch(base + kWave, next) : 0;
        for (int u0 = 0; u0 < cnt; u0 += kDetAhead) {
          // straight-line: every load of the group is issued before the first
          // add (a slot past the id's last occurrence re-reads that one, a
          // lane past column k reads column 0; both are masked out below)
          float cv[kDetAhead];
          bool hv[kDetAhead];
#pragma unroll
          for (int u = 0; u < kDetAhead; ++u) {
            const bool in = u0 + u < cnt;
            const Occ oc = contrib.lane(mine, in ? u0 + u : cnt - 1);
            const bool adds = contrib.value(oc, live ? c : 0, e, cv[u]);
            hv[u] = in & live & adds;
          }
#pragma unroll
          for (int u = 0; u < kDetAhead; ++u) {
#pragma clang fp contract(off)
            const float sum = acc + cv[u];
            acc = hv[u] ? (have ? sum : cv[u]) : acc;
            have |= hv[u];
          }
          if (C::kBias && cb == 0) {
#pragma unroll
            for (int u = 0; u < kDetAhead; ++u) {
#pragma clang fp contract(off)
              const bool in = u0 + u < cnt;
              const float gb = contrib.bias(contrib.lane(mine, in ? u0 + u : cnt - 1));
              const float sum = accw + gb;
              accw = in ? (havew ? sum : gb) : accw;
              havew |= in;
            }
          }
        }
        if (cntn == 0) break;
        mine = next;
        cnt = cntn;
      }
      if (live) dE[(int64_t)id * k + c] = have ? acc : 0.f;
      if (C::kBias && cb == 0 && l == 0) dw[id] = accw;
    }
  }
}

// The step's scalars in a fixed order: thread t of one 256-thread workgroup
// adds rows t, t + 256, ... ascending (g in float — null for HHFM, which has
// no bias — the loss in double), thread 0 the 256 partials in ascending t.
__global__ __launch_bounds__(256) void det_scalars(const float* __restrict__ gb,
                                                   const double* __restrict__ lossb, int64_t B,
                                                   float* __restrict__ scal) {
  __shared__ float sg[256];
  __shared__ double sl[256];
  float a = 0.f;
  double d = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += 256) {
    if (gb) a += gb[b];
    d += lossb[b];
  }
  sg[threadIdx.x] = a;
  sl[threadIdx.x] = d;
  __syncthreads();
  if (threadIdx.x == 0) {
    float A = 0.f;
    double D = 0.0;
    for (int t = 0; t < 256; ++t) {
      A += sg[t];
      D += sl[t];
    }
    if (gb) scal[kScalBiasGrad] = A;
    scal[kScalDataLoss] = (float)D;
  }
}

// A dense head gradient in the scalar order: workgroup c adds column c of the
// per-row values V [B][ld] as det_scalars adds g — thread t rows t, t + 256,
// ... ascending from 0, thread 0 the 256 partials in ascending t from 0 —
// and stores out[c] (plain store; the buffer was zero).
__global__ __launch_bounds__(256) void det_columns(const float* __restrict__ V, int64_t B,
                                                   int64_t ld, float* __restrict__ out) {
  __shared__ float sv[256];
  const int c = blockIdx.x;
  float a = 0.f;
  for (int64_t b = threadIdx.x; b < B; b += 256) a += V[b * ld + c];
  sv[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    float A = 0.f;
    for (int t = 0; t < 256; ++t) A += sv[t];
    out[c] = A;
  }
}

// hipCUB's real temporary-storage figure against the plan's upper bound, before
// a step launches anything (a refusal must leave the workspace untouched)
static int det_sort_fits(const DetPlan& p, hipStream_t st) {
  if (p.n == 0) return 0;
  size_t tmp = 0;
  uint32_t* kk = nullptr;
  int32_t* vv = nullptr;
  const hipError_t e =
      hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, kk, kk, vv, vv, p.n, 0, p.bits, st);
  if (e != hipSuccess) return (int)e;
  return tmp > p.tmp_bytes ? HHFM_EWORKSPACE : 0;
}

// grouping + segment pass + scalars of one deterministic step (n > 0); the
// row pass has run (it wrote only scratch: a refusal here leaves every parameter
// untouched).  Returns 0, a hipError_t or HHFM_EWORKSPACE.
template <class C>
static int det_scatter(const DetPlan& p, char* sc, const OccSource& src, int S, int64_t B,
                       int64_t M, const float* E, int k, float* dE, float* dw, const float* gb,
                       float* scal, const C& contrib, hipStream_t st) {
  uint32_t* kin = reinterpret_cast<uint32_t*>(sc + p.keys_in);
  uint32_t* kout = reinterpret_cast<uint32_t*>(sc + p.keys_out);
  int32_t* vin = reinterpret_cast<int32_t*>(sc + p.vals_in);
  int32_t* vout = reinterpret_cast<int32_t*>(sc + p.vals_out);
  int32_t* runs = reinterpret_cast<int32_t*>(sc + p.runs);
  int32_t* nruns = reinterpret_cast<int32_t*>(sc + p.nruns);
  const int gn = grid_for_n(p.n);
  size_t tmp = 0;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, kin, kout, vin, vout, p.n, 0,
                                                    p.bits, st);
  if (e != hipSuccess) return (int)e;
  if (tmp > p.tmp_bytes) return HHFM_EWORKSPACE;
  hipLaunchKernelGGL(det_keys, dim3(gn), dim3(256), 0, st, src, S, p.n, M, kin, vin, nruns);
  e = hipcub::DeviceRadixSort::SortPairs(sc + p.tmp, tmp, kin, kout, vin, vout, p.n, 0, p.bits,
                                         st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(det_runs, dim3(gn), dim3(256), 0, st, kout, p.n, runs, nruns);
  const int64_t ids = M < p.n ? M : p.n;   // at most this many distinct ids
  hipLaunchKernelGGL(det_segments<C>, dim3(grid_for_n(ids * kWave)), dim3(256), 0, st, kout, vout,
                     p.n, runs, nruns, E, k, dE, dw, contrib);
  hipLaunchKernelGGL(det_scalars, dim3(1), dim3(256), 0, st, gb,
                     reinterpret_cast<const double*>(sc + p.loss), B, scal);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// DeepFM training (fp32, the reference numerics).  Forward: the MLP as
// exact-fp32 MFMA GEMMs (gemm_mfma.h, layer 0 gathering its A rows from the
// table), activations kept for the backward pass.  Backward: a row kernel for
// the concat projection (out, d = out − y, dWp, dbp, dw, the last layer's
// delta), per layer dW = Hᵀ·G and G_prev = (G·Wᵀ) ⊙ relu' as GEMMs on
// transposed / zero-padded copies, and a scatter of the embedding gradient
// (deep part + FM part ∂y2/∂e_f = Σe − e_f).  Every activation row is padded
// to a multiple of 8 floats and every transposed copy to Bp = pad8(B) columns,
// zero-filled, so the GEMM's 16-byte K chunks never read past a row.
// ---------------------------------------------------------------------------
constexpr int kDfmTrainMaxLayers = 4;
constexpr int kDfmHeadMaxCols = 1024;   // F + k + d_L per concat row

static int64_t pad8(int64_t x) { return (x + 7) & ~int64_t(7); }

// dst[c][r] = src[r][c] (r < R, c < C; zero for R <= r < Rp) and, with a mask
// H, both the masked src (written back in place) and its transpose use
// src ⊙ (H > 0).  32x32 tiles through LDS.
__global__ __launch_bounds__(256) void tr_pad(float* __restrict__ src, int64_t R, int C,
                                              int64_t lds, const float* __restrict__ H,
                                              int64_t ldh, float* __restrict__ dst,
                                              int64_t ldd, int64_t Rp) {
  __shared__ float t[32][33];
  const int64_t r0 = (int64_t)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int64_t r = r0 + i;
    const int c = c0 + tx;
    float v = 0.f;
    if (r < R && c < C) {
      v = src[r * lds + c];
      if (H) {
        v = H[r * ldh + c] > 0.f ? v : 0.f;
        src[r * lds + c] = v;
      }
    }
    t[i][tx] = v;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i;
    const int64_t r = r0 + tx;
    if (c < C && r < Rp) dst[c * ldd + r] = t[tx][i];
  }
}

// dst[r][c] = src[r][c] for c < C, 0 for C <= c < ldd (row-major zero pad)
__global__ __launch_bounds__(256) void copy_pad(const float* __restrict__ src, int64_t R, int C,
                                                float* __restrict__ dst, int ldd) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < R * ldd;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / ldd;
    const int c = (int)(i - r * ldd);
    dst[i] = c < C ? src[r * C + c] : 0.f;
  }
}

// X0ᵀ[c][m] = E[x_m, c/k][c%k] (m < B), 0 for B <= m < Bp
__global__ __launch_bounds__(256) void gather_tr(const int32_t* __restrict__ idx, int64_t B,
                                                 int F, const float* __restrict__ E, int64_t M,
                                                 int k, float* __restrict__ dst, int64_t Bp) {
  __shared__ float t[32][33];
  const int64_t m0 = (int64_t)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32;
  const int D = F * k;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int64_t m = m0 + i;
    const int c = c0 + tx;
    float v = 0.f;
    if (m < B && c < D) {
      const int f = c / k;
      v = E[(int64_t)clamp_id(idx[m * F + f], M) * k + (c - f * k)];
    }
    t[i][tx] = v;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i;
    const int64_t m = m0 + tx;
    if (c < D && m < Bp) dst[c * Bp + m] = t[tx][i];
  }
}

// db[n] = Σ_m G_T[n][m]  (wave per output)
__global__ __launch_bounds__(256) void row_sums(const float* __restrict__ GT, int N, int64_t ld,
                                                int64_t cols, float* __restrict__ out) {
  const int l = threadIdx.x & 63;
  const int64_t n = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  if (n >= N) return;
  float s = 0.f;
  for (int64_t m = l; m < cols; m += kWave) s += GT[n * ld + m];
  s = group_sum<kWave>(s);
  if (l == 0) out[n] = s;
}

// Concat projection, forward and backward (DFM.py:109-137, l2_loss), wave
// per row; each lane keeps its columns' dWp partials over the block's rows.
// scal[kScalBiasGrad] += dbp  scal[kScalDataLoss] += (out − y)²/2
// DET (hhfm_dfm_train_step_det): no atomics — the partials restart from zero at
// every row and are stored per row (rowv [B][F+k+dL], for det_columns), the
// row's loss goes to lossb in double, dw is left to the scatter pass.
// `head` (include/hhfm.h "DeepFM heads", wave-uniform): the concat columns are
// the present parts only — [y1 | y2] without DEEP (HL, GL unused), [h_L]
// without FM (w unread, no dw) — and with SIGMOID z = the projection, p =
// 1/(1 + expf(−z)), the row's loss is log_loss's l_b (the step divides the sum
// by B) and g = ((1 − y)/(1 − p + ε) − y/(p + ε))·p·(1 − p)/B.
constexpr float kLogLossEps = 1e-7f;   // tf.losses.log_loss's default epsilon

template <bool DET>
__global__ __launch_bounds__(256) void dfm_train_head(
    const int32_t* __restrict__ idx, const float* __restrict__ y, int64_t B, int F,
    const float* __restrict__ E, const float* __restrict__ w, int64_t M, int k,
    const float* __restrict__ HL, int dL, int64_t ldh, const float* __restrict__ Wp,
    const float* __restrict__ bp, float* __restrict__ GL, float* __restrict__ gvec,
    float* __restrict__ dWp, float* __restrict__ dw, float* __restrict__ scal,
    float* __restrict__ rowv, double* __restrict__ lossb, int head) {
  constexpr int NJ = kDfmHeadMaxCols / kWave;
  const int l = threadIdx.x & 63;
  const bool sig = head & HHFM_DFM_HEAD_SIGMOID;
  const int F1 = head & HHFM_DFM_HEAD_FM ? F : 0;        // y1 columns
  const int FK = head & HHFM_DFM_HEAD_FM ? F + k : 0;    // y1 and y2 columns
  const int D = FK + (head & HHFM_DFM_HEAD_DEEP ? dL : 0);
  float part[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) part[j] = 0.f;
  float sb = 0.f, sl = 0.f;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t m = wave; m < B; m += nwave) {
    const int32_t* x = idx + m * F;
    // this lane's concat columns c = l + 64 j: [y1 (F) | y2 (k) | h_L (dL)]
    float cv[NJ];
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = l + kWave * j;
      float v = 0.f;
      if (c < F1) {
        v = w[clamp_id(x[c], M)];
      } else if (c < FK) {
        const int cc = c - F1;
        float s = 0.f, q = 0.f;
        for (int f = 0; f < F; ++f) {
          const float e = E[(int64_t)clamp_id(x[f], M) * k + cc];
          s += e;
          q += e * e;
        }
        v = 0.5f * (s * s - q);
      } else if (c < D) {
        v = HL[m * ldh + (c - FK)];
      }
      cv[j] = v;
      if (c < D) dot = fmaf(v, Wp[c], dot);
    }
    const float out = group_sum<kWave>(dot) + bp[0];
    float g = out - y[m];                          // d l2_loss(y − out) / d out
    float ll = 0.f;                                // log_loss's l_b
    if (sig) {
      const float yy = y[m];
      const float pr = 1.f / (1.f + expf(-out));
      ll = -yy * logf(pr + kLogLossEps) - (1.f - yy) * logf(1.f - pr + kLogLossEps);
      g = ((1.f - yy) / (1.f - pr + kLogLossEps) - yy / (pr + kLogLossEps)) * pr * (1.f - pr) /
          (float)B;
    }
    if constexpr (DET) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) part[j] = 0.f;
      if (l == 0) lossb[m] = sig ? (double)ll : 0.5 * ((double)g * (double)g);
    } else {
      sb += g;
      sl += sig ? ll : 0.5f * g * g;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = l + kWave * j;
      if (c < D) part[j] = fmaf(g, cv[j], part[j]);
      if constexpr (DET) {
        if (c < D) rowv[m * D + c] = part[j];
      } else {
        if (c < F1) atomicAdd(&dw[clamp_id(x[c], M)], g * Wp[c]);
      }
      if (c >= FK && c < D) {
        const int n = c - FK;
        GL[m * ldh + n] = cv[j] > 0.f ? g * Wp[c] : 0.f;   // relu' of the last layer
      }
    }
    if (l == 0) gvec[m] = g;
  }
  if constexpr (DET) return;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = l + kWave * j;
    if (c < D && part[j] != 0.f) atomicAdd(&dWp[c], part[j]);
  }
  if (l == 0) {   // (g is wave-uniform: every lane holds the same sums)
    atomicAdd(&scal[kScalBiasGrad], sb);
    atomicAdd(&scal[kScalDataLoss], sl);
  }
}

// dE[x_f][c] += dX0[m][f·k + c] + g_m·Wp[F+c]·(Σ_f' e_f'c − e_fc)   (wave per row)
// DET: the same value is stored at its occurrence instead, dE [B·F][k], and the
// occurrence's dw value g_m·Wp[f] (the head's expression) in wb [B·F], for the
// segment pass (StoredContrib).
// `head`: without DEEP there is no dX0 term (dX0 unread); without FM no
// g·Wp[F+c]·(s − e) term and wb = 0 (Wp then holds h_L's entries only).
template <bool DET>
__global__ __launch_bounds__(256) void dfm_train_scatter(
    const int32_t* __restrict__ idx, int64_t B, int F, const float* __restrict__ E, int64_t M,
    int k, const float* __restrict__ dX0, const float* __restrict__ gvec,
    const float* __restrict__ Wp, float* __restrict__ dE, float* __restrict__ wb, int head) {
  const int l = threadIdx.x & 63;
  const bool fm = head & HHFM_DFM_HEAD_FM, deep = head & HHFM_DFM_HEAD_DEEP;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t m = wave; m < B; m += nwave) {
    const int32_t* x = idx + m * F;
    const float g = gvec[m];
    if constexpr (DET)
      for (int f = l; f < F; f += kWave) wb[m * F + f] = fm ? g * Wp[f] : 0.f;
    for (int c = l; c < k; c += kWave) {
      float s = 0.f, gy2 = 0.f;
      if (fm) {
        for (int f = 0; f < F; ++f) s += E[(int64_t)clamp_id(x[f], M) * k + c];
        gy2 = g * Wp[F + c];
      }
      for (int f = 0; f < F; ++f) {
        const int64_t id = clamp_id(x[f], M);
        float v;
        if (fm) {
          const float e = E[id * k + c];
          if (deep)
            v = dX0[m * (int64_t)(F * k) + f * k + c] + gy2 * (s - e);
          else
            v = gy2 * (s - e);
        } else {
          v = dX0[m * (int64_t)(F * k) + f * k + c];
        }
        if constexpr (DET)
          dE[(m * F + f) * k + c] = v;
        else
          atomicAdd(&dE[id * k + c], v);
      }
    }
  }
}

// log_loss's one division by B, on the summed row losses (default step: after
// the head's atomics; deterministic: after det_scalars stored the ordered sum)
__global__ void dfm_mean_loss(float* scal, float Bf) { scal[kScalDataLoss] /= Bf; }

// The DeepFM / AFM workspace allocator and the part of the layout the two
// plans share.  Offsets are in floats, every region rounded up to 64 floats.
// The persistent prefix comes first, at offsets independent of B:
//   scal | dE [M·k] | dw [M] | the model's own dense gradients | touched [M bytes]
// all zero-initialised and kept zeroed by the step (but Adam's β powers in
// scal), so a workspace grown for a larger batch keeps its state by copying the
// old one's first `state` floats, and a smaller batch finds every buffer the
// step accumulates into where the last step left it zeroed.  What follows is
// per-batch scratch that a step writes before it reads it, so it may move
// with B.
struct TrainWs {
  int64_t off_scal, off_dE, off_dw, off_touch;
  int64_t state;   // floats of the persistent prefix
  int64_t total;   // floats allocated so far
  int64_t take(int64_t n) {
    const int64_t r = total;
    total += (n + 63) & ~int64_t(63);
    return r;
  }
  void take_state_head(int64_t M, int k) {
    off_scal = take(kScalFloats);
    off_dE = take(M * k);
    off_dw = take(M);
  }
  void take_state_tail(int64_t M) {
    off_touch = take((M + 3) / 4);
    state = total;
  }
};

struct DfmTrainPlan : TrainWs {
  int64_t Bp;
  int L, D0, dL;                     // dL: the last layer's width (0 without layers)
  int d[kDfmTrainMaxLayers + 1];     // d[0] = F·k, d[l+1] = layer l width
  int64_t off_WtP[kDfmTrainMaxLayers], off_WP[kDfmTrainMaxLayers];
  int64_t off_dW[kDfmTrainMaxLayers], off_db[kDfmTrainMaxLayers];
  int64_t off_H[kDfmTrainMaxLayers + 1], off_HT[kDfmTrainMaxLayers];
  int64_t off_G[kDfmTrainMaxLayers + 1], off_GT[kDfmTrainMaxLayers + 1];
  int64_t off_dX0, off_g, off_dWp;
};

// `min_layers` 0: a step without the deep part may come with no layer list
// (d_L = 0: the dWp region is [F + k], no per-layer scratch).
static bool dfm_train_plan(int64_t B, int F, int k, int64_t M, int L, const int32_t* dims,
                           DfmTrainPlan& p, int min_layers = 1) {
  if (L < min_layers || L > kDfmTrainMaxLayers || F < 1 || k < 4 || k % 4) return false;
  if (L > 0 && !dims) return false;
  p = DfmTrainPlan{};
  p.L = L;
  p.D0 = F * k;
  p.d[0] = p.D0;
  for (int i = 0; i < L; ++i) {
    if (dims[i] < 1) return false;
    p.d[i + 1] = dims[i];
  }
  p.dL = L > 0 ? p.d[L] : 0;
  if (F + k + p.dL > kDfmHeadMaxCols) return false;
  p.Bp = pad8(B > 0 ? B : 1);
  p.take_state_head(M, k);
  p.off_dWp = p.take(F + k + p.dL);
  p.take_state_tail(M);
  // per-batch scratch (dW / db are written by the step before the optimizer reads them)
  for (int i = 0; i < L; ++i) {
    p.off_WtP[i] = p.take((int64_t)p.d[i + 1] * pad8(p.d[i]));
    p.off_WP[i] = p.take((int64_t)p.d[i] * pad8(p.d[i + 1]));
    p.off_dW[i] = p.take((int64_t)p.d[i] * p.d[i + 1]);
    p.off_db[i] = p.take(p.d[i + 1]);
    p.off_HT[i] = p.take((int64_t)p.d[i] * p.Bp);
  }
  for (int i = 1; i <= L; ++i) {
    p.off_H[i] = p.take(p.Bp * pad8(p.d[i]));
    p.off_G[i] = p.take(p.Bp * pad8(p.d[i]));
    p.off_GT[i] = p.take((int64_t)p.d[i] * p.Bp);
  }
  p.off_dX0 = p.take(p.Bp * p.D0);
  p.off_g = p.take(p.Bp);
  return true;
}


// ---------------------------------------------------------------------------
// AFM training (fp32, AFM.py:103-156): the two pair-shaped products run as
// exact-fp32 MFMA GEMMs (gemm_mfma.h) over the B·np (row, pair) "combos":
//   R   = relu(pairs · W + b)           pair-mode A operand (e_i ⊙ e_j formed
//                                        in the loader), [B·np][A]
//   DP  = dZ · Wᵀ                       ∂L/∂pairs through the attention MLP
//   dW  = pairsᵀ · dZ                   split-K over the B·np combos, then a
//                                        fixed-order sum of the splits
// and two wave-per-row kernels do the rest: `afm_train_head` (logits,
// softmax over the row's pairs, out, d = out − y, the softmax backward
// dlogit = a ⊙ (da − Σ a·da), dZ = dlogit·p ⊙ relu', db, dp, dP, dw; writes
// dZ and the pair products transposed for the dW GEMM) and `afm_train_scatter`
// (∂L/∂e_i += dpair ⊙ e_j, ∂L/∂e_j += dpair ⊙ e_i, float atomics into dE).
// ---------------------------------------------------------------------------
constexpr int kAfmTrainMaxF = 16;                          // np <= 120
constexpr int kAfmTrainMaxNp = kAfmTrainMaxF * (kAfmTrainMaxF - 1) / 2;
constexpr int kAfmTrainMaxKA = 256;                        // k, A <= 256
constexpr int kAfmSplitK = 512;                            // combos per dW split

// DROP: tf.nn.dropout on the softmaxed attention (AFM.py:126; dropout.h site 1,
// keep0) and on the k-vector AFM (AFM.py:134; site 2, keep1), row index m.
// With m1_p = bin1_p / keep0, m2_c = bin2_c / keep1 and ã = a ⊙ m1:
//   out  = Σ_c m2_c P_c Σ_p ã_p pr_pc + Σw + w0      s_p = Σ_c P_c m2_c pr_pc
//   da_p = m1_p·g·s_p, dlogit = a ⊙ (da − Σ a·da) on the undropped softmax a
//   dP_c = g·m2_c·Σ_p ã_p pr_pc
// `att` receives ã for the scatter.  k <= 256 and np <= 120: one Philox block
// per lane and site serves the lane's columns l + 64·kc and pairs l + 64·j.
// DET (hhfm_afm_train_step_det): no atomics — accP / accV / accB restart from
// zero at every row and are stored per row (rowv [B][k + 2A]: dP, dp, db, for
// det_columns), the row's loss goes to lossb in double, dw is left to the
// scatter pass.
template <bool DROP, bool DET = false>
__global__ __launch_bounds__(256) void afm_train_head(
    const int32_t* __restrict__ idx, const float* __restrict__ y, int64_t B, int F,
    const float* __restrict__ E, const float* __restrict__ w, const float* __restrict__ w0,
    int64_t M, int k, int A, const float* __restrict__ R, const float* __restrict__ pvec,
    const float* __restrict__ P, float* __restrict__ Gz, float* __restrict__ PT,
    float* __restrict__ GzT, int64_t Kp, float* __restrict__ att, float* __restrict__ gvec,
    float* __restrict__ dP, float* __restrict__ dpv, float* __restrict__ db,
    float* __restrict__ dw, float* __restrict__ scal, DropoutArgs dr,
    float* __restrict__ rowv, double* __restrict__ lossb) {
  constexpr int NC = kAfmTrainMaxKA / kWave;
  __shared__ float sp_all[4][kAfmTrainMaxNp], lg_all[4][kAfmTrainMaxNp];
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* sp = sp_all[wv];
  float* lg = lg_all[wv];
  const int np = F * (F - 1) / 2;
  float accP[NC], accV[NC], accB[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) accP[j] = accV[j] = accB[j] = 0.f;
  float sg = 0.f, sl = 0.f;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t m = wave; m < B; m += nwave) {
    const int32_t* x = idx + m * F;
    const int64_t c0 = m * np;   // first combo of this row
    // this lane's m2 of columns l + 64·kc and m1 of pairs l, l + 64
    [[maybe_unused]] float m2[NC], m1a = 1.f, m1b = 1.f;
    if constexpr (DROP) {
      const Philox4 b2 = dropout_block(dr.key0, dr.key1, kDropSiteAfmVec, m, l);
#pragma unroll
      for (int kc = 0; kc < NC; ++kc) m2[kc] = dropout_binary(dr.keep1, b2.v[kc]) / dr.keep1;
      const Philox4 b1 = dropout_block(dr.key0, dr.key1, kDropSiteAfmAtt, m, l);
      m1a = dropout_binary(dr.keep0, b1.v[0]) / dr.keep0;
      m1b = dropout_binary(dr.keep0, b1.v[1]) / dr.keep0;
    }
    // s_p = P·(e_i ⊙ e_j)   (lanes over k; one wave sum per pair and chunk)
    for (int p = l; p < np; p += kWave) sp[p] = 0.f;
#pragma unroll
    for (int kc = 0; kc < NC; ++kc) {
      const int c = l + kWave * kc;
      if (kc * kWave >= k) break;
      float ev[kAfmTrainMaxF];
#pragma unroll
      for (int f = 0; f < kAfmTrainMaxF; ++f)
        ev[f] = (f < F && c < k) ? E[(int64_t)clamp_id(x[f], M) * k + c] : 0.f;
      float pc = c < k ? P[c] : 0.f;
      if constexpr (DROP) pc *= m2[kc];
      int p = 0;
#pragma unroll
      for (int i = 0; i < kAfmTrainMaxF; ++i)
#pragma unroll
        for (int j = i + 1; j < kAfmTrainMaxF; ++j)
          if (j < F) {
            const float s = group_sum<kWave>(ev[i] * ev[j] * pc);
            if (l == 0) sp[p] += s;
            ++p;
          }
    }
    __builtin_amdgcn_wave_barrier();
    // logit_p = Σ_a pvec_a · R[p][a]   (lanes over A)
    for (int p = 0; p < np; ++p) {
      float t = 0.f;
      for (int a = l; a < A; a += kWave) t = fmaf(pvec[a], R[(c0 + p) * A + a], t);
      t = group_sum<kWave>(t);
      if (l == 0) lg[p] = t;
    }
    __builtin_amdgcn_wave_barrier();
    // softmax over the row's pairs (AFM.py:125, max subtracted), out, d
    float mx = -__builtin_huge_valf();
    for (int p = l; p < np; p += kWave) mx = fmaxf(mx, lg[p]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, kWave));
    float se = 0.f;
    for (int p = l; p < np; p += kWave) se += expf(lg[p] - mx);
    se = group_sum<kWave>(se);
    float os = 0.f;
    for (int p = l; p < np; p += kWave) {
      if constexpr (DROP)
        os += expf(lg[p] - mx) / se * (p < kWave ? m1a : m1b) * sp[p];
      else
        os += expf(lg[p] - mx) / se * sp[p];
    }
    os = group_sum<kWave>(os);
    float fb = 0.f;
    for (int f = l; f < F; f += kWave) fb += w[clamp_id(x[f], M)];
    fb = group_sum<kWave>(fb);
    const float out = (os + fb) + w0[0];
    const float g = out - y[m];                      // d l2_loss(y − out) / d out
    if constexpr (DET) {
#pragma unroll
      for (int j = 0; j < NC; ++j) accP[j] = accV[j] = accB[j] = 0.f;
      if (l == 0) lossb[m] = 0.5 * ((double)g * (double)g);
    } else {
      sg += g;
      sl += 0.5f * g * g;
    }
    // da_p = g·s_p, dlogit_p = a_p (da_p − Σ a·da)
    float t = 0.f;
    for (int p = l; p < np; p += kWave) {
      if constexpr (DROP)
        t += expf(lg[p] - mx) / se * ((p < kWave ? m1a : m1b) * (g * sp[p]));
      else
        t += expf(lg[p] - mx) / se * (g * sp[p]);
    }
    t = group_sum<kWave>(t);
    for (int p = l; p < np; p += kWave) {
      const float a = expf(lg[p] - mx) / se;
      if constexpr (DROP) {
        const float m1 = p < kWave ? m1a : m1b;
        att[c0 + p] = a * m1;                        // ã for the scatter
        lg[p] = a * (m1 * (g * sp[p]) - t);
        sp[p] = a * m1;
      } else {
        att[c0 + p] = a;
        lg[p] = a * (g * sp[p] - t);                 // lg now holds dlogit
        sp[p] = a;                                   // sp now holds att
      }
    }
    if (l == 0) gvec[m] = g;
    __builtin_amdgcn_wave_barrier();
    // dZ = dlogit·p ⊙ relu'(z)  (lanes over A), written row-major and transposed
#pragma unroll
    for (int ac = 0; ac < NC; ++ac) {
      const int a = l + kWave * ac;
      if (ac * kWave >= A) break;
      if (a < A) {
        const float pa = pvec[a];
        for (int p = 0; p < np; ++p) {
          const float r = R[(c0 + p) * A + a];
          const float dl = lg[p];
          accV[ac] = fmaf(dl, r, accV[ac]);
          const float dz = r > 0.f ? dl * pa : 0.f;
          accB[ac] += dz;
          Gz[(c0 + p) * A + a] = dz;
          GzT[a * Kp + c0 + p] = dz;
        }
      }
    }
    // afm = Σ a_p (e_i ⊙ e_j) -> dP; pair products transposed for the dW GEMM
#pragma unroll
    for (int kc = 0; kc < NC; ++kc) {
      const int c = l + kWave * kc;
      if (kc * kWave >= k) break;
      if (c < k) {
        float ev[kAfmTrainMaxF];
#pragma unroll
        for (int f = 0; f < kAfmTrainMaxF; ++f)
          ev[f] = f < F ? E[(int64_t)clamp_id(x[f], M) * k + c] : 0.f;
        float afm = 0.f;
        int p = 0;
#pragma unroll
        for (int i = 0; i < kAfmTrainMaxF; ++i)
#pragma unroll
          for (int j = i + 1; j < kAfmTrainMaxF; ++j)
            if (j < F) {
              const float pr = ev[i] * ev[j];
              afm = fmaf(sp[p], pr, afm);
              PT[c * Kp + c0 + p] = pr;
              ++p;
            }
        if constexpr (DROP)
          accP[kc] = fmaf(g * m2[kc], afm, accP[kc]);
        else
          accP[kc] = fmaf(g, afm, accP[kc]);
      }
    }
    if constexpr (DET) {
      float* rv = rowv + m * (k + 2 * A);
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int c = l + kWave * j;
        if (c < k) rv[c] = accP[j];
        if (c < A) rv[k + c] = accV[j];
        if (c < A) rv[k + A + c] = accB[j];
      }
    } else {
      for (int f = l; f < F; f += kWave) atomicAdd(&dw[clamp_id(x[f], M)], g);
    }
    __builtin_amdgcn_wave_barrier();   // sp / lg are rewritten by the next row
  }
  if constexpr (DET) return;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int c = l + kWave * j;
    if (c < k && accP[j] != 0.f) atomicAdd(&dP[c], accP[j]);
    if (c < A && accV[j] != 0.f) atomicAdd(&dpv[c], accV[j]);
    if (c < A && accB[j] != 0.f) atomicAdd(&db[c], accB[j]);
  }
  if (l == 0) {   // g is wave-uniform
    atomicAdd(&scal[kScalBiasGrad], sg);
    atomicAdd(&scal[kScalDataLoss], sl);
  }
}

// dE[x_f][c] += Σ_{pairs ∋ f} (DP + a_p·d·P_c) ⊙ e_other   (wave per row, lanes over k)
// DROP: `att` holds ã and the AFM-path term is ã_p·d·P_c·m2_c, m2 regenerated
// from the counter (site 2); the DP term is unchanged.
// DET: de[f] is stored at its occurrence instead, dE [B·F][k], and the
// occurrence's dw value g_m in wb [B·F], for the segment pass (StoredContrib).
template <bool DROP, bool DET = false>
__global__ __launch_bounds__(256) void afm_train_scatter(
    const int32_t* __restrict__ idx, int64_t B, int F, const float* __restrict__ E, int64_t M,
    int k, const float* __restrict__ DP, const float* __restrict__ att,
    const float* __restrict__ gvec, const float* __restrict__ P, float* __restrict__ dE,
    DropoutArgs dr, float* __restrict__ wb) {
  const int l = threadIdx.x & 63;
  const int np = F * (F - 1) / 2;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t m = wave; m < B; m += nwave) {
    const int32_t* x = idx + m * F;
    const int64_t c0 = m * np;
    const float g = gvec[m];
    if constexpr (DET)
      for (int f = l; f < F; f += kWave) wb[m * F + f] = g;
    [[maybe_unused]] LaneDropout ld;
    for (int c = l; c < k; c += kWave) {
      float ev[kAfmTrainMaxF], de[kAfmTrainMaxF];
#pragma unroll
      for (int f = 0; f < kAfmTrainMaxF; ++f) {
        ev[f] = f < F ? E[(int64_t)clamp_id(x[f], M) * k + c] : 0.f;
        de[f] = 0.f;
      }
      float gp = g * P[c];
      if constexpr (DROP) gp *= ld.binary(dr, dr.keep1, kDropSiteAfmVec, m, c) / dr.keep1;
      int p = 0;
#pragma unroll
      for (int i = 0; i < kAfmTrainMaxF; ++i)
#pragma unroll
        for (int j = i + 1; j < kAfmTrainMaxF; ++j)
          if (j < F) {
            const float d = fmaf(att[c0 + p], gp, DP[(c0 + p) * k + c]);
            de[i] = fmaf(d, ev[j], de[i]);
            de[j] = fmaf(d, ev[i], de[j]);
            ++p;
          }
#pragma unroll
      for (int f = 0; f < kAfmTrainMaxF; ++f)
        if (f < F) {
          if constexpr (DET)
            dE[(m * F + f) * k + c] = de[f];
          else
            atomicAdd(&dE[(int64_t)clamp_id(x[f], M) * k + c], de[f]);
        }
    }
  }
}

// zero the K padding [n, Kp) of `rows` transposed rows of stride Kp
__global__ __launch_bounds__(256) void zero_cols(float* __restrict__ T, int rows, int64_t Kp,
                                                 int64_t n) {
  const int pad = (int)(Kp - n);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)rows * pad;
       i += (int64_t)gridDim.x * blockDim.x)
    T[(i / pad) * Kp + n + i % pad] = 0.f;
}

// dW[i] = Σ_s part[s][i] in split order (deterministic)
__global__ __launch_bounds__(256) void sum_splits(const float* __restrict__ part, int S,
                                                  int64_t n, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int z = 0; z < S; ++z) s += part[z * n + i];
    out[i] = s;
  }
}

struct AfmTrainPlan : TrainWs {
  int np;
  int64_t n, Kp;
  int S;
  int64_t off_Wt, off_R, off_Gz, off_T, off_DP, off_att, off_g, off_part;
  int64_t off_dW, off_db, off_dpv, off_dP;
};

static bool afm_train_plan(int64_t B, int F, int k, int A, int64_t M, AfmTrainPlan& p) {
  if (F < 2 || F > kAfmTrainMaxF || k < 4 || k % 4 || k > kAfmTrainMaxKA || A < 4 || A % 4 ||
      A > kAfmTrainMaxKA || B < 0 || M < 1)
    return false;
  p = AfmTrainPlan{};
  p.np = F * (F - 1) / 2;
  p.n = B * p.np;
  if (p.n > (int64_t)1 << 30) return false;
  p.Kp = pad8(p.n > 0 ? p.n : 1);
  p.S = (int)((p.Kp + kAfmSplitK - 1) / kAfmSplitK);
  p.take_state_head(M, k);
  p.off_dW = p.take((int64_t)k * A);
  p.off_db = p.take(A);
  p.off_dpv = p.take(A);
  p.off_dP = p.take(k);
  p.take_state_tail(M);
  // per-batch scratch
  p.off_Wt = p.take((int64_t)A * k);
  p.off_R = p.take(p.n * A);
  p.off_Gz = p.take(p.n * A);
  p.off_T = p.take((int64_t)(k + A) * p.Kp);   // PT [k][Kp] then GzT [A][Kp]
  p.off_DP = p.take(p.n * k);
  p.off_att = p.take(p.n);
  p.off_g = p.take(B);
  p.off_part = p.take((int64_t)p.S * k * A);
  return true;
}

// The scratch of the deterministic DeepFM / AFM steps: the grouping's regions
// as for FM (S = F), the stored contributions [B·F][k] in `rowvec`, the
// occurrences' dw values [B·F] in `bias`, the per-row head values in `heads`
// (DeepFM [B][F+k+d_L]; AFM [B][k+2A]), the row losses, and one Σvar² partial
// per wave of every λ-carrying variable's optimizer grid.
static bool dfm_det_plan(int64_t B, int F, int k, int64_t M, const DfmTrainPlan& p, DetPlan& d) {
  if (B > 0x7fffffff) return false;
  const int D = F + k + p.dL;
  int64_t ss = det_sumsq_floats(D);
  for (int i = 0; i < p.L; ++i) ss += det_sumsq_floats((int64_t)p.d[i] * p.d[i + 1]);
  return det_plan_regions(B, F, M, B * F * k, ss, B * F, B * D, d);
}

static bool afm_det_plan(int64_t B, int F, int k, int A, int64_t M, DetPlan& d) {
  if (B > 0x7fffffff) return false;
  return det_plan_regions(B, F, M, B * F * k, det_sumsq_floats((int64_t)k * A), B * F,
                          B * (k + 2 * A), d);
}

// tr_pad over src [R][C] (row stride lds): dst [C][ldd], rows R..Rp zero
static void launch_tr_pad(float* src, int64_t R, int C, int64_t lds, const float* H, int64_t ldh,
                          float* dst, int64_t ldd, int64_t Rp, hipStream_t st) {
  hipLaunchKernelGGL(tr_pad, dim3((unsigned)((Rp + 31) / 32), (unsigned)((C + 31) / 32)),
                     dim3(256), 0, st, src, R, C, lds, H, ldh, dst, ldd, Rp);
}

// C [M][ldc] = A [M][lda] · Btᵀ, Bt [N][ldb]; the callers add what else they need
static GemmArgs gemm_plain(int64_t M, int N, int64_t K, const void* A, int64_t lda,
                           const void* Bt, int64_t ldb, void* C, int64_t ldc) {
  GemmArgs g{};
  g.M = M;
  g.N = N;
  g.K = (int)K;
  g.A = A;
  g.lda = lda;
  g.Bt = Bt;
  g.ldb = ldb;
  g.C = C;
  g.ldc = ldc;
  return g;
}

// ---------------------------------------------------------------------------
// FM with batch_norm=1 (hhfm_fm_train_step_bn; include/hhfm.h "FM batch norm").
// The layer sits between the k-vector x_bc = ½(s² − q) and its row sum, and its
// statistics are sums over the whole batch, so the step is a chain of kernels
// with column sums between them.  Two mappings:
//   row kernels     one wave per row, lane = column (c = l + 64·j), as
//                   fm_train_rows: fm_bn_out (out_b, g_b, the loss) and
//                   fm_bn_scatter (dx_bc and the scatter into dE, dw)
//   column kernels  the same waves, but the column slab j is the outer loop
//                   and the wave's rows the inner one, so a lane adds its
//                   column's terms over its rows in a register (fp32), the
//                   workgroup's four waves are added through LDS (fp32) and
//                   ONE double atomicAdd per workgroup and column goes to
//                   memory (bn_block_add): fm_bn_x (x_bc stored [B][k], Σx),
//                   fm_bn_m2 (Σ(x − μ)², two-pass), fm_bn_colgrad (dβ, dγ)
// fm_bn_stats finishes μ, v, inv, a, β − μ·a and moves the moving averages;
// fm_bn_grads rounds the double sums into the fp32 gradient buffers of γ, β
// and w0 the optimizer tail reads.  The grid of every kernel but the scatter
// is capped at kBnMaxBlocks workgroups, so a column receives at most that many
// double adds and a lane's fp32 partial spans B / (4·kBnMaxBlocks) rows.
// ---------------------------------------------------------------------------
constexpr int kBnMaxBlocks = 2048;
constexpr int kBnSums = 4;   // per column, in double: Σx | Σ(x−μ)² | Σdy | Σdy·x̂ ; then Σg [1]
constexpr int kBnStats = 4;  // per column, fp32: μ | inv | a | β − μ·a

static int bn_grid(int64_t B) {
  const int64_t g = (B + 3) / 4;
  return (int)(g > kBnMaxBlocks ? kBnMaxBlocks : (g < 1 ? 1 : g));
}

// The FM-BN workspace, in bytes.  Persistent prefix (`state`): fm_train_plan's
// layout, then dγ [k] | dβ [k] floats — zero-filled once, left zeroed by the
// step (but Adam's β powers).  Per-batch scratch after it, written before it
// is read: the double sums (zeroed by the step itself), the fp32 statistics,
// g [B] and x [B][k].
struct FmBnPlan {
  FmTrainPlan fm;
  size_t off_dgamma, off_dbeta, state, off_sums, off_stats, off_g, off_x, bytes;
};

static bool fm_bn_plan(int64_t B, int64_t M, int k, FmBnPlan& p) {
  if (B < 0 || M < 1 || k < 1) return false;
  p.fm = fm_train_plan(M, k);
  p.off_dgamma = al256(p.fm.bytes);
  p.off_dbeta = p.off_dgamma + (size_t)k * 4;
  p.state = al256(p.off_dbeta + (size_t)k * 4);
  p.off_sums = p.state;
  p.off_stats = al256(p.off_sums + ((size_t)kBnSums * k + 1) * 8);
  p.off_g = al256(p.off_stats + (size_t)kBnStats * k * 4);
  p.off_x = al256(p.off_g + (size_t)B * 4);
  p.bytes = al256(p.off_x + (size_t)B * k * 4);
  return true;
}

// μ_c as every kernel forms it: the double column sum over B, rounded once
__device__ __forceinline__ float bn_mean(const double* __restrict__ sum, int c, int64_t B) {
  return (float)(sum[c] / (double)B);
}

// dst[c] += the four waves' partials of column c (lane l of every wave holds
// one), added in fp32 in wave order.  Every thread of the workgroup calls it.
__device__ __forceinline__ void bn_block_add(float (&red)[4][kWave], float acc, int c, int k,
                                             double* __restrict__ dst) {
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
  red[wv][l] = acc;
  __syncthreads();
  if (wv == 0 && c < k)
    atomicAdd(dst + c, (double)(((red[0][l] + red[1][l]) + red[2][l]) + red[3][l]));
  __syncthreads();
}

__global__ __launch_bounds__(256) void fm_bn_x(const int32_t* __restrict__ idx, int64_t B, int F,
                                               const float* __restrict__ E, int64_t M, int k,
                                               float* __restrict__ xs, double* __restrict__ sum) {
  __shared__ float red[4][kWave];
  const int l = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int c0 = 0; c0 < k; c0 += kWave) {
    const int c = c0 + l;
    float acc = 0.f;
    if (c < k)
      for (int64_t b = wave; b < B; b += nwave) {
        const int32_t* x = idx + b * F;
        float s = 0.f, q = 0.f;
        for (int f = 0; f < F; ++f) {
          const float v = E[(int64_t)clamp_id(x[f], M) * k + c];
          s += v;
          q += v * v;
        }
        const float xv = 0.5f * (s * s - q);
        xs[b * k + c] = xv;
        acc += xv;
      }
    bn_block_add(red, acc, c, k, sum);
  }
}

__global__ __launch_bounds__(256) void fm_bn_m2(int64_t B, int k, const float* __restrict__ xs,
                                                const double* __restrict__ sum,
                                                double* __restrict__ m2) {
  __shared__ float red[4][kWave];
  const int l = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int c0 = 0; c0 < k; c0 += kWave) {
    const int c = c0 + l;
    float acc = 0.f;
    if (c < k) {
      const float mu = bn_mean(sum, c, B);
      for (int64_t b = wave; b < B; b += nwave) {
        const float d = xs[b * k + c] - mu;
        acc += d * d;
      }
    }
    bn_block_add(red, acc, c, k, m2);
  }
}

// v = Σ(x−μ)²/B (biased), inv = 1/√(v + eps) with IEEE sqrt and division,
// a = inv·γ, shift = β − μ·a (tf.nn.batch_normalization); then
// assign_moving_average (zero_debias=False): mm −= (mm − μ)·u, mv −= (mv − v)·u
__global__ __launch_bounds__(256) void fm_bn_stats(int64_t B, int k,
                                                   const double* __restrict__ sums,
                                                   const float* __restrict__ gamma,
                                                   const float* __restrict__ beta,
                                                   float* __restrict__ mm, float* __restrict__ mv,
                                                   float eps, float bn_update,
                                                   float* __restrict__ stats) {
  for (int c = threadIdx.x; c < k; c += blockDim.x) {
    const float mu = bn_mean(sums, c, B);
    const float v = (float)(sums[k + c] / (double)B);
    const float inv = __fdiv_rn(1.f, __fsqrt_rn(v + eps));
    const float a = inv * gamma[c];
    stats[c] = mu;
    stats[k + c] = inv;
    stats[2 * k + c] = a;
    stats[3 * k + c] = beta[c] - mu * a;
    mm[c] -= (mm[c] - mu) * bn_update;
    mv[c] -= (mv[c] - v) * bn_update;
  }
}

// out_b = Σ_c y_bc (/ keep · bin_bc) + Σ_f w + w0, y = x·a + (β − μ·a); g_b
// stored; a wave adds its rows' r²/2 and g in double / fp32 registers and
// sends one double atomic each when it is done.
template <bool DROP>
__global__ __launch_bounds__(256) void fm_bn_out(
    const int32_t* __restrict__ idx, const float* __restrict__ y, int64_t B, int F,
    const float* __restrict__ w, const float* __restrict__ w0, int64_t M, int k,
    const float* __restrict__ xs, const float* __restrict__ stats, float* __restrict__ gb,
    float* __restrict__ scal, double* __restrict__ gsum, DropoutArgs dr) {
  const int l = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const float* a = stats + 2 * (int64_t)k;
  const float* shift = stats + 3 * (int64_t)k;
  double loss = 0.0, gs = 0.0;
  for (int64_t b = wave; b < B; b += nwave) {
    const int32_t* x = idx + b * F;
    float t = 0.f;
    [[maybe_unused]] LaneDropout ld;
    for (int c = l; c < k; c += kWave) {
      const float yv = xs[b * k + c] * a[c] + shift[c];
      if constexpr (DROP)
        t += yv / dr.keep0 * ld.binary(dr, dr.keep0, kDropSiteFm, b, c);
      else
        t += yv;
    }
    t = group_sum<kWave>(t);
    float fb = 0.f;
    for (int f = 0; f < F; ++f) fb += w[clamp_id(x[f], M)];
    const float out = (t + fb) + w0[0];
    const float r = y[b] - out;
    if (l == 0) gb[b] = -r;
    loss += 0.5 * ((double)r * (double)r);
    gs += (double)(-r);
  }
  if (l == 0 && wave < B) {
    atomicAdd(scal_loss64(scal), loss);
    atomicAdd(gsum, gs);
  }
}

// dβ_c = Σ_b dy_bc, dγ_c = Σ_b dy_bc·x̂_bc; dy = g·bin/keep, x̂ = (x − μ)·inv.
// The slab-outer loop does not walk a row's columns in order, so the mask is
// dropout_element's (a block per element), not LaneDropout's.
template <bool DROP>
__global__ __launch_bounds__(256) void fm_bn_colgrad(
    int64_t B, int k, const float* __restrict__ xs, const float* __restrict__ gb,
    const float* __restrict__ stats, double* __restrict__ dbeta, double* __restrict__ dgamma,
    DropoutArgs dr) {
  __shared__ float red[4][kWave];
  const int l = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int c0 = 0; c0 < k; c0 += kWave) {
    const int c = c0 + l;
    float sb = 0.f, sg = 0.f;
    if (c < k) {
      const float mu = stats[c], inv = stats[k + c];
      for (int64_t b = wave; b < B; b += nwave) {
        float dy = gb[b];
        if constexpr (DROP)
          dy = dy * dropout_element(dr.key0, dr.key1, kDropSiteFm, b, c, dr.keep0) / dr.keep0;
        sb += dy;
        sg += dy * ((xs[b * k + c] - mu) * inv);
      }
    }
    bn_block_add(red, sb, c, k, dbeta);
    bn_block_add(red, sg, c, k, dgamma);
  }
}

// the double sums rounded once into the optimizer's fp32 gradient buffers
__global__ __launch_bounds__(256) void fm_bn_grads(int k, const double* __restrict__ sums,
                                                   float* __restrict__ dgamma,
                                                   float* __restrict__ dbeta,
                                                   float* __restrict__ scal) {
  for (int c = threadIdx.x; c < k; c += blockDim.x) {
    dbeta[c] = (float)sums[2 * (int64_t)k + c];
    dgamma[c] = (float)sums[3 * (int64_t)k + c];
  }
  if (threadIdx.x == 0) scal[kScalBiasGrad] = (float)sums[(int64_t)kBnSums * k];
}

// dx_bc = (a_c / B)·(B·dy_bc − dβ_c − x̂_bc·dγ_c), scattered as fm_train_rows
// scatters g: dE[x_f][c] += dx_bc·(s_bc − e_fc), dw[x_f] += g_b.  A dropped
// column still carries the −dβ − x̂·dγ part, so no column is skipped.
template <bool DROP>
__global__ __launch_bounds__(256) void fm_bn_scatter(
    const int32_t* __restrict__ idx, int64_t B, int F, const float* __restrict__ E, int64_t M,
    int k, const float* __restrict__ xs, const float* __restrict__ gb,
    const float* __restrict__ stats, const float* __restrict__ dgamma,
    const float* __restrict__ dbeta, float* __restrict__ dE, float* __restrict__ dw,
    DropoutArgs dr) {
  const int l = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const float Bf = (float)B;
  for (int64_t b = wave; b < B; b += nwave) {
    const int32_t* x = idx + b * F;
    const float g = gb[b];
    [[maybe_unused]] LaneDropout ld;
    for (int c = l; c < k; c += kWave) {
      float dy = g;
      if constexpr (DROP) dy = g * ld.binary(dr, dr.keep0, kDropSiteFm, b, c) / dr.keep0;
      const float xh = (xs[b * k + c] - stats[c]) * stats[k + c];
      const float dx = (stats[2 * (int64_t)k + c] / Bf) * (Bf * dy - dbeta[c] - xh * dgamma[c]);
      float s = 0.f;
      for (int f = 0; f < F; ++f) s += E[(int64_t)clamp_id(x[f], M) * k + c];
      for (int f = 0; f < F; ++f) {
        const int64_t id = clamp_id(x[f], M);
        atomicAdd(dE + id * k + c, dx * (s - E[id * k + c]));
      }
    }
    for (int f = l; f < F; f += kWave) atomicAdd(dw + clamp_id(x[f], M), g);
  }
}

// ---------------------------------------------------------------------------
// AFM without attention (hhfm_afm_noatt_train_step; include/hhfm.h "AFM without
// attention", AFM.py:103-148 with self.attention false): FM's k-vector
// x_c = ½(s² − q) weighted by the prediction vector P,
//   out = Σ_c d_c·P_c + Σ_f w + w0     d_c = x_c (/ keep · bin_c)
// with tf.nn.dropout on the k-vector (dropout.h site 2, keep1, the row index
// the batch row) and no regulariser.  One wave per row, lane l the columns
// l + 64·j (k <= 256: one Philox block per lane serves them), the forward with
// fm_train_rows's expressions for s and q in field order.
// DET false: dE / dw by float atomics; a lane adds g·d_c of its rows in a
// register (fp32), the workgroup's waves meet through LDS and ONE double
// atomicAdd per workgroup and column goes to dP64 (bn_block_add, as FM-BN's
// dγ); a wave adds its rows' r²/2 in double and g in fp32 and sends one atomic
// each when it is done.
// DET true (hhfm_afm_noatt_train_step_det): no atomics — S_b[c] (Sb [B][k];
// under dropout bin_b[c] follows, [B][k] more), v_bc = g_b·d_bc (Vb [B][k], for
// det_columns), g_b and the row's loss in double are stored.
// ---------------------------------------------------------------------------
constexpr int kNoAttMaxK = 256;

template <bool DROP, bool DET>
__global__ __launch_bounds__(256) void afm_noatt_train_rows(
    const int32_t* __restrict__ idx, const float* __restrict__ y, int64_t B, int F,
    const float* __restrict__ E, const float* __restrict__ w, const float* __restrict__ w0,
    const float* __restrict__ P, int64_t M, int k, float* __restrict__ dE,
    float* __restrict__ dw, float* __restrict__ scal, double* __restrict__ dP64, DropoutArgs dr,
    float* __restrict__ gb, double* __restrict__ lossb, float* __restrict__ Sb,
    float* __restrict__ Vb) {
#pragma clang fp contract(off)
  constexpr int NC = kNoAttMaxK / kWave;
  __shared__ float red[4][kWave];
  const int l = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) / kWave;
  float accP[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) accP[j] = 0.f;
  double lossw = 0.0;
  float gw = 0.f;
  for (int64_t b = wave; b < B; b += nwave) {
    const int32_t* x = idx + b * F;
    float sv[NC], dv[NC], mb[NC];
    [[maybe_unused]] Philox4 blk;
    if constexpr (DROP) blk = dropout_block(dr.key0, dr.key1, kDropSiteAfmVec, b, l);
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int c = l + kWave * j;
      sv[j] = dv[j] = 0.f;
      mb[j] = 1.f;
      if (c < k) {
        float s = 0.f, q = 0.f;
        for (int f = 0; f < F; ++f) {
          const float v = E[(int64_t)clamp_id(x[f], M) * k + c];
          s += v;
          q += v * v;
        }
        float xv = 0.5f * (s * s - q);
        if constexpr (DROP) {
          mb[j] = dropout_binary(dr.keep1, blk.v[j]);
          xv = xv / dr.keep1 * mb[j];
        }
        sv[j] = s;
        dv[j] = xv;
        t += xv * P[c];
      }
    }
    t = group_sum<kWave>(t);
    float fb = 0.f;
    for (int f = 0; f < F; ++f) fb += w[clamp_id(x[f], M)];
    const float out = (t + fb) + w0[0];
    const float r = y[b] - out;        // l2_loss(y - out) = r²/2   AFM.py:148
    const float g = -r;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int c = l + kWave * j;
      if (c < k) {
        const float v = g * dv[j];     // the row's term of dP_c
        if constexpr (DET) {
          Sb[b * k + c] = sv[j];
          if constexpr (DROP) Sb[(B + b) * k + c] = mb[j];
          Vb[b * k + c] = v;
        } else {
          accP[j] += v;
          if (!DROP || mb[j] != 0.f) {   // a dropped column scatters nothing
            float gc = g * P[c];
            if constexpr (DROP) gc = gc * mb[j] / dr.keep1;
            for (int f = 0; f < F; ++f) {
              const int64_t id = clamp_id(x[f], M);
              atomicAdd(dE + id * k + c, gc * (sv[j] - E[id * k + c]));
            }
          }
        }
      }
    }
    if constexpr (DET) {
      if (l == 0) {
        gb[b] = g;
        lossb[b] = 0.5 * ((double)r * (double)r);
      }
    } else {
      for (int f = l; f < F; f += kWave) atomicAdd(dw + clamp_id(x[f], M), g);
      gw += g;
      lossw += 0.5 * ((double)r * (double)r);
    }
  }
  if constexpr (DET) return;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    if (j * kWave >= k) break;
    bn_block_add(red, accP[j], l + kWave * j, k, dP64);
  }
  if (l == 0 && wave < B) {   // g and the loss are wave-uniform
    atomicAdd(scal + kScalBiasGrad, gw);
    atomicAdd(scal_loss64(scal), lossw);
  }
}

// dP[c] = the double column sum rounded once; the sums are left zeroed
__global__ __launch_bounds__(256) void afm_noatt_dp(int k, double* __restrict__ dP64,
                                                    float* __restrict__ dP) {
  for (int c = threadIdx.x; c < k; c += blockDim.x) {
    dP[c] = (float)dP64[c];
    dP64[c] = 0.0;
  }
}

// The occurrence o = b·F + f of the deterministic step: FmContrib with the
// column weight, gc = g_b·P_c (· bin / keep under dropout), contribution
// gc·(S_b[c] − e); a dropped column adds nothing; dw: g_b.
template <bool DROP>
struct NoAttContrib {
  static constexpr bool kBias = true;
  const float* g;
  const float* S;   // S [B][k], then (DROP) bin [B][k]
  const float* P;
  int64_t B;
  int F, k;
  float keep;
  struct Occ {
    int b;
    float g;
  };
  HHFM_DEV Occ load(int o) const {
    const int b = o / F;
    return Occ{b, g[b]};
  }
  HHFM_DEV Occ lane(const Occ& oc, int u) const { return Occ{lane_i(oc.b, u), lane_f(oc.g, u)}; }
  HHFM_DEV float bias(const Occ& oc) const { return oc.g; }
  HHFM_DEV bool value(const Occ& oc, int c, float e, float& out) const {
#pragma clang fp contract(off)
    float gc = oc.g * P[c];
    bool kept = true;
    if constexpr (DROP) {
      const float bin = S[((int64_t)B + oc.b) * k + c];
      kept = bin != 0.f;
      gc = gc * bin / keep;
    }
    out = gc * (S[(int64_t)oc.b * k + c] - e);
    return kept;
  }
};

// The workspace: fm_train_plan's layout, then dP [k] floats and the column
// sums dP64 [k] doubles — all zero-filled once by the caller and left zeroed.
struct NoAttPlan {
  FmTrainPlan fm;
  size_t off_dP, off_dP64, bytes;
};

static NoAttPlan afm_noatt_plan(int64_t M, int k) {
  NoAttPlan p;
  p.fm = fm_train_plan(M, k);
  p.off_dP = al256(p.fm.bytes);
  p.off_dP64 = al256(p.off_dP + (size_t)k * 4);
  p.bytes = al256(p.off_dP64 + (size_t)k * 8);
  return p;
}

// S and bin [2][B][k] in `rowvec`, v [B][k] in `heads`; there is no Σvar²
static bool afm_noatt_det_plan(int64_t B, int F, int k, int64_t M, DetPlan& d) {
  if (k < 1 || B < 0 || M < 1 || B > 0x7fffffff) return false;
  return det_plan_regions(B, F, M, B * 2 * k, 0, 0, B * k, d);
}

// binary[r][e] = the train kernels' dropout decision (dropout.h) as 0.f / 1.f
__global__ __launch_bounds__(256) void dropout_mask(DropoutArgs dr, int site, int64_t rows, int n,
                                                    float* __restrict__ binary) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / n;
    binary[i] = dropout_element(dr.key0, dr.key1, site, r, (int)(i - r * n), dr.keep0);
  }
}

}  // namespace hhfm

using namespace hhfm;

extern "C" size_t hhfm_train_workspace(int64_t features_M, int32_t k) {
  return fm_train_plan(features_M, k).bytes;
}

extern "C" int hhfm_dropout_mask(uint64_t seed, int32_t site, int64_t rows, int32_t n,
                                 float keep, float* binary, void* stream) {
  if (site < 0 || rows < 0 || n < 1 || !keep_ok(keep)) return HHFM_EINVAL;
  if (rows == 0) return HHFM_OK;
  if (!binary) return HHFM_EINVAL;
  hipLaunchKernelGGL(dropout_mask, dim3(grid_for_n(rows * n)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), dropout_args(keep, keep, seed), site,
                     rows, n, binary);
  return (int)hipGetLastError();
}

extern "C" int hhfm_fm_train_step(const int32_t* idx, const float* y, int64_t B, int32_t F,
                                  float* E, float* w, float* w0, int64_t features_M, int32_t k,
                                  float lr, float lam, int32_t optimizer, float* accE,
                                  float* accw, float* accw0, void* workspace, size_t ws_bytes,
                                  float* loss, void* stream) {
  return hhfm_fm_train_step_ex(idx, y, B, F, E, w, w0, features_M, k, lr, lam, optimizer, 1.f, 0,
                               accE, accw, accw0, workspace, ws_bytes, loss, stream);
}

// The FM step: the default path (det false; scratch unused), or the
// deterministic one on `scratch` (hhfm_train_det_scratch bytes).
static int fm_train_step_impl(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                              float* w, float* w0, int64_t features_M, int32_t k, float lr,
                              float lam, int32_t optimizer, float keep, uint64_t seed,
                              float* accE, float* accw, float* accw0, void* workspace,
                              size_t ws_bytes, bool det, void* scratch, size_t scratch_bytes,
                              float* loss, void* stream) {
  if (B < 0 || F < 1 || k < 1 || features_M < 1 || !keep_ok(keep)) return HHFM_EINVAL;
  if (!opt_ok(optimizer)) return HHFM_EUNSUPPORTED;
  if (!E || !w || !w0 || !loss || !workspace) return HHFM_EINVAL;
  if (B > 0 && (!idx || !y)) return HHFM_EINVAL;   // an empty batch reads no rows
  float* const acc[] = {accE, accw, accw0};
  if (!slots_ok(optimizer, acc, 3)) return HHFM_EINVAL;
  const FmTrainPlan p = fm_train_plan(features_M, k);
  if (ws_bytes < p.bytes) return HHFM_EWORKSPACE;
  DetPlan d{};
  if (det && (!det_plan(B, F, k, features_M, d) || !scratch || scratch_bytes < d.bytes))
    return HHFM_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* ws = reinterpret_cast<float*>(workspace);
  float* scal = ws + p.off_scal;
  char* sc = reinterpret_cast<char*>(scratch);
  const DropoutArgs dr = dropout_args(keep, 1.f, seed);
  if (B > 0 && !det) {
    auto rows = keep < 1.f ? fm_train_rows<true> : fm_train_rows<false>;
    hipLaunchKernelGGL(rows, dim3(grid_for_n(B * 64)), dim3(256), 0, st, idx, y, B, F, E, w, w0,
                       features_M, k, ws + p.off_dE, ws + p.off_dw, scal, dr);
  } else if (B > 0) {
    float* gb = reinterpret_cast<float*>(sc + d.g);
    float* Sb = reinterpret_cast<float*>(sc + d.rowvec);
    auto rows = keep < 1.f ? fm_train_rows_det<true> : fm_train_rows_det<false>;
    hipLaunchKernelGGL(rows, dim3(grid_for_n(B * 64)), dim3(256), 0, st, idx, y, B, F, E, w, w0,
                       features_M, k, gb, reinterpret_cast<double*>(sc + d.loss), Sb, dr);
    const OccSource src{idx, nullptr, F, 0, 0, 0, 0, 0};
    const int rc = keep < 1.f
                       ? det_scatter(d, sc, src, F, B, features_M, E, k, ws + p.off_dE,
                                     ws + p.off_dw, gb, scal, FmContrib<true>{gb, Sb, B, F, k, keep}, st)
                       : det_scatter(d, sc, src, F, B, features_M, E, k, ws + p.off_dE,
                                     ws + p.off_dw, gb, scal, FmContrib<false>{gb, Sb, B, F, k, keep},
                                     st);
    if (rc != 0) return rc;
  }
  // sparse gradients (FM.py:123-126): w's always (embedding_lookup only), E's
  // when λ = 0 (no dense l2 term); w0 and the λ > 0 table are dense
  const OptVar vars[] = {
      {E, ws + p.off_dE, accE, features_M * k, lam, k, lam == 0.f, true},
      {w, ws + p.off_dw, accw, features_M, 0.f, 1, true, false},
      {w0, scal + kScalBiasGrad, accw0, 1, 0.f, 1, false, false}};
  uint8_t* touched = reinterpret_cast<uint8_t*>(ws + p.off_touch);
  return optimizer_tail(vars, (int)std::size(vars), {{idx, B * F}}, features_M, optimizer, lr,
                        scal, touched, lam, loss, st,
                        det ? reinterpret_cast<float*>(sc + d.sspart) : nullptr);
}

extern "C" int hhfm_fm_train_step_ex(const int32_t* idx, const float* y, int64_t B, int32_t F,
                                     float* E, float* w, float* w0, int64_t features_M,
                                     int32_t k, float lr, float lam, int32_t optimizer,
                                     float keep, uint64_t seed, float* accE, float* accw,
                                     float* accw0, void* workspace, size_t ws_bytes, float* loss,
                                     void* stream) {
  return fm_train_step_impl(idx, y, B, F, E, w, w0, features_M, k, lr, lam, optimizer, keep, seed,
                            accE, accw, accw0, workspace, ws_bytes, false, nullptr, 0, loss,
                            stream);
}

extern "C" int hhfm_fm_train_step_det(const int32_t* idx, const float* y, int64_t B, int32_t F,
                                      float* E, float* w, float* w0, int64_t features_M,
                                      int32_t k, float lr, float lam, int32_t optimizer,
                                      float keep, uint64_t seed, float* accE, float* accw,
                                      float* accw0, void* workspace, size_t ws_bytes,
                                      void* scratch, size_t scratch_bytes, float* loss,
                                      void* stream) {
  return fm_train_step_impl(idx, y, B, F, E, w, w0, features_M, k, lr, lam, optimizer, keep, seed,
                            accE, accw, accw0, workspace, ws_bytes, true, scratch, scratch_bytes,
                            loss, stream);
}

extern "C" int hhfm_fm_train_bn_workspace(int64_t B, int64_t features_M, int32_t k,
                                          size_t* ws_bytes) {
  FmBnPlan p;
  if (!ws_bytes || !fm_bn_plan(B, features_M, k, p)) return HHFM_EINVAL;
  *ws_bytes = p.bytes;
  return HHFM_OK;
}

// the FM-BN workspace's persistent prefix (0: invalid sizes)
extern "C" size_t hhfm_fm_train_bn_state_bytes(int64_t features_M, int32_t k) {
  FmBnPlan p;
  return fm_bn_plan(0, features_M, k, p) ? p.state : 0;
}

extern "C" int hhfm_fm_train_step_bn(const int32_t* idx, const float* y, int64_t B, int32_t F,
                                     float* E, float* w, float* w0, int64_t features_M,
                                     int32_t k, float lr, float lam, int32_t optimizer,
                                     float keep, uint64_t seed, float* accE, float* accw,
                                     float* accw0, void* workspace, size_t ws_bytes,
                                     float* gamma, float* beta, float* moving_mean,
                                     float* moving_var, float eps, float bn_update,
                                     float* acc_gamma, float* acc_beta, float* loss,
                                     void* stream) {
  // the plain step's checks, in its order ...
  if (B < 0 || F < 1 || k < 1 || features_M < 1 || !keep_ok(keep)) return HHFM_EINVAL;
  if (!opt_ok(optimizer)) return HHFM_EUNSUPPORTED;
  if (!E || !w || !w0 || !loss || !workspace) return HHFM_EINVAL;
  if (B > 0 && (!idx || !y)) return HHFM_EINVAL;
  float* const acc[] = {accE, accw, accw0, acc_gamma, acc_beta};
  if (!slots_ok(optimizer, acc, 3)) return HHFM_EINVAL;
  FmBnPlan p;
  if (!fm_bn_plan(B, features_M, k, p)) return HHFM_EINVAL;
  if (ws_bytes < p.bytes) return HHFM_EWORKSPACE;
  // ... then the layer's: the moments of an empty batch are NaN in TF
  if (B == 0 || !(eps > 0.f) || !(bn_update >= 0.f && bn_update <= 1.f)) return HHFM_EINVAL;
  if (!gamma || !beta || !moving_mean || !moving_var) return HHFM_EINVAL;
  if (!slots_ok(optimizer, acc + 3, 2)) return HHFM_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return HHFM_EINVAL;   // the double sums
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = reinterpret_cast<char*>(workspace);
  float* ws = reinterpret_cast<float*>(workspace);
  float* scal = ws + p.fm.off_scal;
  float* dgamma = reinterpret_cast<float*>(base + p.off_dgamma);
  float* dbeta = reinterpret_cast<float*>(base + p.off_dbeta);
  double* sums = reinterpret_cast<double*>(base + p.off_sums);
  float* stats = reinterpret_cast<float*>(base + p.off_stats);
  float* gb = reinterpret_cast<float*>(base + p.off_g);
  float* xs = reinterpret_cast<float*>(base + p.off_x);
  const DropoutArgs dr = dropout_args(keep, 1.f, seed);
  const bool drop = keep < 1.f;
  const dim3 grid(bn_grid(B)), blk(256);
  auto k_out = drop ? fm_bn_out<true> : fm_bn_out<false>;
  auto k_col = drop ? fm_bn_colgrad<true> : fm_bn_colgrad<false>;
  auto k_scat = drop ? fm_bn_scatter<true> : fm_bn_scatter<false>;
  if (hipMemsetAsync(sums, 0, ((size_t)kBnSums * k + 1) * 8, st) != hipSuccess)
    return (int)hipGetLastError();
  hipLaunchKernelGGL(fm_bn_x, grid, blk, 0, st, idx, B, F, E, features_M, k, xs, sums);
  hipLaunchKernelGGL(fm_bn_m2, grid, blk, 0, st, B, k, xs, sums, sums + k);
  hipLaunchKernelGGL(fm_bn_stats, dim3(1), blk, 0, st, B, k, sums, gamma, beta, moving_mean,
                     moving_var, eps, bn_update, stats);
  hipLaunchKernelGGL(k_out, grid, blk, 0, st, idx, y, B, F, w,
                     w0, features_M, k, xs, stats, gb, scal, sums + (int64_t)kBnSums * k, dr);
  hipLaunchKernelGGL(k_col, grid, blk, 0, st, B, k,
                     xs, gb, stats, sums + 2 * (int64_t)k, sums + 3 * (int64_t)k, dr);
  hipLaunchKernelGGL(fm_bn_grads, dim3(1), blk, 0, st, k, sums, dgamma, dbeta, scal);
  hipLaunchKernelGGL(k_scat, dim3(grid_for_n(B * 64)),
                     blk, 0, st, idx, B, F, E, features_M, k, xs, gb, stats, dgamma, dbeta,
                     ws + p.fm.off_dE, ws + p.fm.off_dw, dr);
  // γ and β are dense variables without an l2 term; the moving statistics are
  // no optimizer variables (fm_bn_stats has moved them)
  const OptVar vars[] = {
      {E, ws + p.fm.off_dE, accE, features_M * k, lam, k, lam == 0.f, true},
      {w, ws + p.fm.off_dw, accw, features_M, 0.f, 1, true, false},
      {w0, scal + kScalBiasGrad, accw0, 1, 0.f, 1, false, false},
      {gamma, dgamma, slot_of(optimizer, acc, 3), k, 0.f, 1, false, false},
      {beta, dbeta, slot_of(optimizer, acc, 4), k, 0.f, 1, false, false}};
  uint8_t* touched = reinterpret_cast<uint8_t*>(ws + p.fm.off_touch);
  return optimizer_tail(vars, (int)std::size(vars), {{idx, B * F}}, features_M, optimizer, lr,
                        scal, touched, lam, loss, st);
}

extern "C" int hhfm_train_det_scratch(int64_t B, int32_t occ_per_row, int32_t k,
                                      int64_t features_M, size_t* bytes) {
  DetPlan d;
  if (!bytes || !det_plan(B, occ_per_row, k, features_M, d)) return HHFM_EINVAL;
  *bytes = d.bytes;
  return HHFM_OK;
}

static int hhfm_train_step_impl(const int32_t* X, const int32_t* Neg, int64_t B, int32_t ncols,
                                int32_t ctx_begin, int32_t ctx_end, int32_t time_begin,
                                int32_t time_end, int32_t NG, float* E, int64_t features_M,
                                int32_t k, float lr, float lam, int32_t optimizer, float* accE,
                                void* workspace, size_t ws_bytes, bool det, void* scratch,
                                size_t scratch_bytes, float* loss, void* stream,
                                int32_t pooling = 0, bool two_way = false,
                                int32_t pooling2 = 0) {
  PoolModes pm;
  PoolModes2 pm2{};
  if (!pooling_unpack(pooling, pm) || (pooling != 0 && det)) return HHFM_EINVAL;
  if (two_way) {   // no deterministic two-way step; the layouts of two_way_shape_ok only
    if (det || !pooling2_unpack(pooling, pooling2, pm2)) return HHFM_EINVAL;
    if (ctx_begin > ctx_end || time_begin > time_end || ctx_begin < 0 || time_begin < 0 ||
        ctx_end > ncols || time_end > ncols ||
        !two_way_shape_ok(ctx_end - ctx_begin, time_end - time_begin))
      return HHFM_EINVAL;
  }
  if (B < 0 || ncols < 2 || NG < 1 || k < 1 || features_M < 1) return HHFM_EINVAL;
  if (NG > kMaxNeg) return HHFM_EUNSUPPORTED;
  if (!opt_ok(optimizer)) return HHFM_EUNSUPPORTED;
  if (!E || !loss || !workspace) return HHFM_EINVAL;
  if (B > 0 && (!X || !Neg)) return HHFM_EINVAL;
  if (!slots_ok(optimizer, &accE, 1)) return HHFM_EINVAL;
  const FmTrainPlan p = fm_train_plan(features_M, k);   // dw stays unused
  if (ws_bytes < p.bytes) return HHFM_EWORKSPACE;
  // occurrences per row: item, negatives, user, context and time columns
  const int nc = ctx_end > ctx_begin ? ctx_end - ctx_begin : 0;
  const int nt = time_end > time_begin ? time_end - time_begin : 0;
  const int S = 2 + NG + nc + nt;
  DetPlan d{};
  if (det && (!det_plan(B, S, k, features_M, d) || !scratch || scratch_bytes < d.bytes))
    return HHFM_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* ws = reinterpret_cast<float*>(workspace);
  float* scal = ws + p.off_scal;
  char* sc = reinterpret_cast<char*>(scratch);
  // the row pass over the feature policy; the deterministic one stores per-row values
  float *gb = nullptr, *gtb = nullptr, *HV = nullptr;
  uint32_t* maskb = nullptr;
  double* lossb = nullptr;
  auto rows = [&](auto feat, auto is_det) {
    hipLaunchKernelGGL((hhfm_train_rows<decltype(feat), decltype(is_det)::value>),
                       dim3(grid_for_n(B * 64)), dim3(256), 0, st, X, Neg, B, ncols, ctx_begin,
                       ctx_end, time_begin, time_end, NG, E, features_M, k, feat, ws + p.off_dE,
                       scal, gb, gtb, maskb, lossb, HV);
  };
  if (B > 0 && two_way) {
    rows(TwoWayFeature{pm2}, std::false_type{});
  } else if (B > 0 && pooling != 0) {
    hipLaunchKernelGGL(hhfm_train_rows_pool, dim3(grid_for_n(B * 64)), dim3(256), 0, st, X, Neg,
                       B, ncols, ctx_begin, ctx_end, time_begin, time_end, NG, E, features_M, k,
                       pm, ws + p.off_dE, scal);
  } else if (B > 0 && !det) {
    rows(SumFeature{}, std::false_type{});
  } else if (B > 0) {
    gb = reinterpret_cast<float*>(sc + d.g);
    gtb = reinterpret_cast<float*>(sc + d.gt);
    maskb = reinterpret_cast<uint32_t*>(sc + d.mask);
    lossb = reinterpret_cast<double*>(sc + d.loss);
    HV = reinterpret_cast<float*>(sc + d.rowvec);
    rows(SumFeature{}, std::true_type{});
    const OccSource src{X, Neg, ncols, NG, ctx_begin, ctx_begin + nc, time_begin, time_begin + nt};
    const int rc = det_scatter(d, sc, src, S, B, features_M, E, k, ws + p.off_dE, nullptr, nullptr,
                               scal, HhfmContrib{gb, gtb, maskb, HV, S, NG, k}, st);
    if (rc != 0) return rc;
  }
  // E's gradient is dense through λ·l2(E) (OurModel7.py:180-184), sparse at λ = 0
  const OptVar vars[] = {{E, ws + p.off_dE, accE, features_M * k, lam, k, lam == 0.f, true}};
  uint8_t* touched = reinterpret_cast<uint8_t*>(ws + p.off_touch);
  return optimizer_tail(vars, (int)std::size(vars), {{X, B * ncols}, {Neg, B * NG}}, features_M,
                        optimizer, lr, scal, touched, lam, loss, st,
                        det ? reinterpret_cast<float*>(sc + d.sspart) : nullptr);
}

extern "C" int hhfm_hhfm_train_step(const int32_t* X, const int32_t* Neg, int64_t B,
                                    int32_t ncols, int32_t ctx_begin, int32_t ctx_end,
                                    int32_t time_begin, int32_t time_end, int32_t NG, float* E,
                                    int64_t features_M, int32_t k, float lr, float lam,
                                    int32_t optimizer, float* accE, void* workspace,
                                    size_t ws_bytes, float* loss, void* stream) {
  return hhfm_train_step_impl(X, Neg, B, ncols, ctx_begin, ctx_end, time_begin, time_end, NG, E,
                              features_M, k, lr, lam, optimizer, accE, workspace, ws_bytes, false,
                              nullptr, 0, loss, stream);
}

extern "C" int hhfm_hhfm_train_step_pool(const int32_t* X, const int32_t* Neg, int64_t B,
                                         int32_t ncols, int32_t ctx_begin, int32_t ctx_end,
                                         int32_t time_begin, int32_t time_end, int32_t NG,
                                         float* E, int64_t features_M, int32_t k, float lr,
                                         float lam, int32_t optimizer, float* accE,
                                         void* workspace, size_t ws_bytes, int32_t pooling,
                                         float* loss, void* stream) {
  return hhfm_train_step_impl(X, Neg, B, ncols, ctx_begin, ctx_end, time_begin, time_end, NG, E,
                              features_M, k, lr, lam, optimizer, accE, workspace, ws_bytes, false,
                              nullptr, 0, loss, stream, pooling);
}

extern "C" int hhfm_hhfm_train_step_pool2(const int32_t* X, const int32_t* Neg, int64_t B,
                                          int32_t ncols, int32_t ctx_begin, int32_t ctx_end,
                                          int32_t time_begin, int32_t time_end, int32_t NG,
                                          float* E, int64_t features_M, int32_t k, float lr,
                                          float lam, int32_t optimizer, float* accE,
                                          void* workspace, size_t ws_bytes, int32_t pooling,
                                          int32_t pooling2, float* loss, void* stream) {
  return hhfm_train_step_impl(X, Neg, B, ncols, ctx_begin, ctx_end, time_begin, time_end, NG, E,
                              features_M, k, lr, lam, optimizer, accE, workspace, ws_bytes, false,
                              nullptr, 0, loss, stream, pooling, true, pooling2);
}

extern "C" int hhfm_hhfm_train_step_det(const int32_t* X, const int32_t* Neg, int64_t B,
                                        int32_t ncols, int32_t ctx_begin, int32_t ctx_end,
                                        int32_t time_begin, int32_t time_end, int32_t NG,
                                        float* E, int64_t features_M, int32_t k, float lr,
                                        float lam, int32_t optimizer, float* accE,
                                        void* workspace, size_t ws_bytes, void* scratch,
                                        size_t scratch_bytes, float* loss, void* stream) {
  return hhfm_train_step_impl(X, Neg, B, ncols, ctx_begin, ctx_end, time_begin, time_end, NG, E,
                              features_M, k, lr, lam, optimizer, accE, workspace, ws_bytes, true,
                              scratch, scratch_bytes, loss, stream);
}

// ---------------------------------------------------------------------------
// CARS2 (Newcode/CARS2.py:87, :103-136, :167-170; include/hhfm.h "CARS2").
// The workspace, in floats, every region on a 256-byte boundary:
//   dUI [n_ui·D] | dContext [Mc·Dc] | dW [D·Dp·Dc] | dZ [D·Dq·Dc] | dA [Dp] |
//   dB [Dq] | scal [kScalFloats] | touched mask of UI (n_ui bytes) | touched
//   mask of Context (Mc bytes)                      <- the persistent prefix
//   ZB [D·Dc] | GB [Mc·D] | T [D·Dc] | gδ [B·D]     <- per-batch scratch
// dW and dA stay zero: the data gradient of W and A is identically zero.
// ---------------------------------------------------------------------------
struct Cars2TrainPlan {
  int64_t dUI, dCtx, dW, dZ, dA, dB, scal, touchUI, touchCtx, state;
  int64_t ZB, GB, T, gd, total;   // floats
};

static bool cars2_train_plan(int64_t B, int64_t n_ui, int64_t Mc, int D, int Dc, int Dp, int Dq,
                             Cars2TrainPlan& p) {
  if (B < 0 || n_ui < 1 || Mc < 1 || D < 1 || Dc < 1 || Dp < 1 || Dq < 1) return false;
  if (n_ui > ((int64_t)1 << 31) || Mc > ((int64_t)1 << 31) || B > ((int64_t)1 << 31)) return false;
  if ((int64_t)D * Dc * (Dp > Dq ? Dp : Dq) > ((int64_t)1 << 30)) return false;
  int64_t o = 0;
  auto take = [&](int64_t n) {
    const int64_t at = o;
    o += (n + 63) & ~int64_t(63);
    return at;
  };
  p.dUI = take(n_ui * D);
  p.dCtx = take(Mc * Dc);
  p.dW = take((int64_t)D * Dp * Dc);
  p.dZ = take((int64_t)D * Dq * Dc);
  p.dA = take(Dp);
  p.dB = take(Dq);
  p.scal = take(kScalFloats);
  p.touchUI = take((n_ui + 3) / 4);
  p.touchCtx = take((Mc + 3) / 4);
  p.state = o;
  p.ZB = take((int64_t)D * Dc);
  p.GB = take(Mc * D);
  p.T = take((int64_t)D * Dc);
  p.gd = take(B * D);
  p.total = o;
  return true;
}

extern "C" int hhfm_cars2_train_workspace(int64_t B, int64_t n_ui, int64_t Mc, int32_t D,
                                          int32_t Dc, int32_t Dp, int32_t Dq, size_t* ws_bytes) {
  Cars2TrainPlan p;
  if (!ws_bytes || !cars2_train_plan(B, n_ui, Mc, D, Dc, Dp, Dq, p)) return HHFM_EINVAL;
  *ws_bytes = (size_t)p.total * 4;
  return HHFM_OK;
}

extern "C" int hhfm_cars2_train_state_bytes(int64_t n_ui, int64_t Mc, int32_t D, int32_t Dc,
                                            int32_t Dp, int32_t Dq, size_t* state_bytes) {
  Cars2TrainPlan p;
  if (!state_bytes || !cars2_train_plan(1, n_ui, Mc, D, Dc, Dp, Dq, p)) return HHFM_EINVAL;
  *state_bytes = (size_t)p.state * 4;
  return HHFM_OK;
}

extern "C" int hhfm_cars2_train_step(const int32_t* X, const int32_t* Fea, const int32_t* Neg,
                                     int64_t B, int32_t NG, float* UI, int64_t n_ui,
                                     float* Context, int64_t Mc, float* W, float* Z, float* A,
                                     float* Bv, int32_t D, int32_t Dc, int32_t Dp, int32_t Dq,
                                     float lr, float lambda_l2, int32_t optimizer,
                                     float* const* acc, void* workspace, size_t ws_bytes,
                                     float* loss, void* stream) {
  Cars2TrainPlan p;
  if (NG < 1 || !cars2_train_plan(B, n_ui, Mc, D, Dc, Dp, Dq, p)) return HHFM_EINVAL;
  if (NG > kMaxNeg || D > kCars2TrainMaxD) return HHFM_EUNSUPPORTED;
  if (!opt_ok(optimizer)) return HHFM_EUNSUPPORTED;
  if (!UI || !Context || !W || !Z || !A || !Bv || !loss || !workspace) return HHFM_EINVAL;
  if (B > 0 && (!X || !Fea || !Neg)) return HHFM_EINVAL;
  if (!slots_ok(optimizer, acc, 6)) return HHFM_EINVAL;   // acc: UI, Context, W, Z, A, B
  if (ws_bytes < (size_t)p.total * 4) return HHFM_EWORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* ws = reinterpret_cast<float*>(workspace);
  float* scal = ws + p.scal;
  const float lam = lambda_l2 > 0.f ? lambda_l2 : 0.f;   // CARS2.py:115
  if (B > 0) {
    const hipError_t me = hipMemsetAsync(ws + p.T, 0, (size_t)D * Dc * 4, st);
    if (me != hipSuccess) return (int)me;
    cars2_launch_fold(Z, Bv, D, Dq, Dc, ws + p.ZB, st);
    cars2_launch_table(ws + p.ZB, Context, Mc, D, Dc, ws + p.GB, st);
    cars2_launch_train_rows(X, Fea, Neg, B, NG, UI, n_ui, D, Dc, ws + p.GB, ws + p.ZB, Mc,
                            ws + p.dUI, ws + p.dCtx, ws + p.gd, scal + kScalDataLoss, st);
    cars2_launch_t(ws + p.gd, Fea, Context, B, Mc, D, Dc, ws + p.T, st);
    cars2_launch_dz_db(Z, Bv, ws + p.T, D, Dq, Dc, ws + p.dZ, ws + p.dB, st);
  }
  // with λ > 0 the l2 terms make every gradient dense (CARS2.py:115-121); at
  // λ = 0 UI and Context are IndexedSlices, Z and B dense, W and A dense zeros
  const bool sp = lam == 0.f;
  uint8_t* touchedUI = reinterpret_cast<uint8_t*>(ws + p.touchUI);
  uint8_t* touchedCtx = reinterpret_cast<uint8_t*>(ws + p.touchCtx);
  const bool mark = sp && optimizer == HHFM_OPT_MOMENTUM && B > 0;
  if (mark)
    hipLaunchKernelGGL(mark_rows, dim3(grid_for_n(B)), dim3(256), 0, st, Fea, B, Mc, touchedCtx,
                       (uint8_t)1);
  const OptVar vars[] = {
      {UI, ws + p.dUI, slot_of(optimizer, acc, 0), n_ui * D, lam, D, sp, true},
      {Context, ws + p.dCtx, slot_of(optimizer, acc, 1), Mc * Dc, lam, Dc, sp, true, touchedCtx},
      {W, ws + p.dW, slot_of(optimizer, acc, 2), (int64_t)D * Dp * Dc, lam, 1, false, true},
      {Z, ws + p.dZ, slot_of(optimizer, acc, 3), (int64_t)D * Dq * Dc, lam, 1, false, true},
      {A, ws + p.dA, slot_of(optimizer, acc, 4), Dp, lam, 1, false, true},
      {Bv, ws + p.dB, slot_of(optimizer, acc, 5), Dq, lam, 1, false, true}};
  const int rc = optimizer_tail(vars, (int)std::size(vars), {{X, B * 2}, {Neg, B * NG}}, n_ui,
                                optimizer, lr, scal, touchedUI, lam, loss, st);
  if (mark)
    hipLaunchKernelGGL(mark_rows, dim3(grid_for_n(B)), dim3(256), 0, st, Fea, B, Mc, touchedCtx,
                       (uint8_t)0);
  return rc != 0 ? rc : (int)hipGetLastError();
}

extern "C" int hhfm_dfm_train_workspace(int64_t B, int32_t F, int32_t k, int64_t features_M,
                                        int32_t nlayers, const int32_t* layer_dims,
                                        size_t* ws_bytes) {
  DfmTrainPlan p;
  if (!ws_bytes || !layer_dims || B < 0 || features_M < 1 ||
      !dfm_train_plan(B, F, k, features_M, nlayers, layer_dims, p))
    return HHFM_EINVAL;
  *ws_bytes = (size_t)p.total * 4;
  return HHFM_OK;
}

// bytes at the front of the DeepFM workspace that carry state between steps
// (TrainWs's persistent prefix); B-independent
extern "C" int hhfm_dfm_train_state_bytes(int32_t F, int32_t k, int64_t features_M,
                                          int32_t nlayers, const int32_t* layer_dims,
                                          size_t* state_bytes) {
  DfmTrainPlan p;
  if (!state_bytes || !layer_dims || features_M < 1 ||
      !dfm_train_plan(1, F, k, features_M, nlayers, layer_dims, p))
    return HHFM_EINVAL;
  *state_bytes = (size_t)p.state * 4;
  return HHFM_OK;
}

// The DeepFM step: the default path (det false; scratch unused), or the
// deterministic one on `scratch` (hhfm_dfm_train_det_scratch bytes).  `head`
// (include/hhfm.h "DeepFM heads"; FM | DEEP is the reference default): without
// DEEP no layer is read and no transpose or GEMM runs; a variable the head
// gives no gradient is left out of the optimizer's list.
static int dfm_train_step_impl(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                               float* w, int64_t features_M, int32_t k, int32_t nlayers,
                               const int32_t* layer_dims, float* const* W, float* const* bias,
                               float* Wp, float* bp, float lr, float lambda_l2,
                               int32_t optimizer, float* const* acc, void* workspace,
                               size_t ws_bytes, bool det, void* scratch, size_t scratch_bytes,
                               float* loss, void* stream,
                               int32_t head = HHFM_DFM_HEAD_FM | HHFM_DFM_HEAD_DEEP) {
  DfmTrainPlan p;
  DetPlan d{};
  if (head & ~(HHFM_DFM_HEAD_FM | HHFM_DFM_HEAD_DEEP | HHFM_DFM_HEAD_SIGMOID)) return HHFM_EINVAL;
  const bool fm = head & HHFM_DFM_HEAD_FM, deep = head & HHFM_DFM_HEAD_DEEP;
  const bool sig = head & HHFM_DFM_HEAD_SIGMOID;
  if (!fm && !deep) return HHFM_EINVAL;
  if (B < 0 || features_M < 1 || (deep && !layer_dims) ||
      !dfm_train_plan(B, F, k, features_M, nlayers, layer_dims, p, deep ? 1 : 0) ||
      (det && !dfm_det_plan(B, F, k, features_M, p, d)))
    return HHFM_EINVAL;
  if (!opt_ok(optimizer)) return HHFM_EUNSUPPORTED;
  if (!E || !w || (deep && (!W || !bias)) || !Wp || !bp || !loss || !workspace)
    return HHFM_EINVAL;
  if (B > 0 && (!idx || !y)) return HHFM_EINVAL;
  const int L = p.L;
  for (int i = 0; deep && i < L; ++i)
    if (!W[i] || !bias[i]) return HHFM_EINVAL;
  // acc: E, w, W_0..W_{L-1}, b_0..b_{L-1}, Wp, bp; a head looks only at the
  // slots of the variables it moves
  if (fm && deep) {
    if (!slots_ok(optimizer, acc, 2 * L + 4)) return HHFM_EINVAL;
  } else if (optimizer != HHFM_OPT_SGD) {
    if (!acc || !acc[0] || (fm && !acc[1]) || !acc[2 + 2 * L] || !acc[3 + 2 * L])
      return HHFM_EINVAL;
    for (int i = 0; deep && i < 2 * L; ++i)
      if (!acc[2 + i]) return HHFM_EINVAL;
  }
  // the head's concat columns: the present parts of [y1 (F) | y2 (k) | h_L (d_L)]
  const int D = (fm ? F + k : 0) + (deep ? p.dL : 0);
  if (ws_bytes < (size_t)p.total * 4) return HHFM_EWORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (det) {
    if (!scratch) return HHFM_EINVAL;
    if (scratch_bytes < d.bytes) return HHFM_EWORKSPACE;
    if (const int rc = det_sort_fits(d, st)) return rc;
  }
  float* ws = reinterpret_cast<float*>(workspace);
  auto at = [&](int64_t off) { return ws + off; };
  float* scal = at(p.off_scal);
  const int64_t Bp = p.Bp;
  char* sc = reinterpret_cast<char*>(scratch);
  auto sf = [&](size_t off) { return reinterpret_cast<float*>(sc + off); };

  if (B > 0 && !deep) {
    // the FM head: head, scatter (or the det row pass and segment pass); no GEMM chain
    hipLaunchKernelGGL(det ? dfm_train_head<true> : dfm_train_head<false>,
                       dim3(grid_for_n(B * 64 / 8)), dim3(256), 0, st, idx, y, B, F, E, w,
                       features_M, k, nullptr, 0, (int64_t)0, Wp, bp, nullptr, at(p.off_g),
                       at(p.off_dWp), at(p.off_dw), scal, det ? sf(d.heads) : nullptr,
                       det ? reinterpret_cast<double*>(sc + d.loss) : nullptr, head);
    if (!det) {
      if (sig) hipLaunchKernelGGL(dfm_mean_loss, dim3(1), dim3(1), 0, st, scal, (float)B);
      hipLaunchKernelGGL(dfm_train_scatter<false>, dim3(grid_for_n(B * 64)), dim3(256), 0, st,
                         idx, B, F, E, features_M, k, nullptr, at(p.off_g), Wp, at(p.off_dE),
                         nullptr, head);
    } else {
      hipLaunchKernelGGL(det_columns, dim3(D), dim3(256), 0, st, sf(d.heads), B, (int64_t)D,
                         at(p.off_dWp));
      hipLaunchKernelGGL(dfm_train_scatter<true>, dim3(grid_for_n(B * 64)), dim3(256), 0, st, idx,
                         B, F, E, features_M, k, nullptr, at(p.off_g), Wp, sf(d.rowvec),
                         sf(d.bias), head);
      const OccSource src{idx, nullptr, F, 0, 0, 0, 0, 0};
      const int rc = det_scatter(d, sc, src, F, B, features_M, E, k, at(p.off_dE), at(p.off_dw),
                                 at(p.off_g), scal, StoredContrib{sf(d.rowvec), sf(d.bias), k}, st);
      if (rc != 0) return rc;
      if (sig) hipLaunchKernelGGL(dfm_mean_loss, dim3(1), dim3(1), 0, st, scal, (float)B);
    }
  } else if (B > 0) {
    // weights: Wᵀ zero-padded (forward Bt) and W zero-padded (backward Bt)
    for (int i = 0; i < L; ++i) {
      const int din = p.d[i], dout = p.d[i + 1];
      launch_tr_pad(W[i], din, dout, dout, nullptr, 0, at(p.off_WtP[i]), pad8(din), pad8(din), st);
      hipLaunchKernelGGL(copy_pad, dim3(grid_for_n((int64_t)din * pad8(dout))), dim3(256), 0, st,
                         W[i], (int64_t)din, dout, at(p.off_WP[i]), (int)pad8(dout));
    }
    // forward: H_{i+1} = relu(H_i · W_i + b_i), H_0 gathered from the table
    for (int i = 0; i < L; ++i) {
      GemmArgs g = gemm_plain(B, p.d[i + 1], p.d[i], i ? at(p.off_H[i]) : nullptr,
                              i ? pad8(p.d[i]) : 0, at(p.off_WtP[i]), pad8(p.d[i]),
                              at(p.off_H[i + 1]), pad8(p.d[i + 1]));
      if (i == 0) {
        g.gidx = idx;
        g.T = E;
        g.Mtab = features_M;
        g.F = F;
        g.kf = k;
      }
      g.bias = bias[i];
      g.relu = 1;
      launch_gemm(g, false, 0, st);
    }
    // head: out, d = out − y, dWp, dbp, dw, last layer's delta
    const int64_t ldL = pad8(p.d[L]);
    (void)hipMemsetAsync(at(p.off_G[L]), 0, (size_t)(B * ldL) * 4, st);
    hipLaunchKernelGGL(det ? dfm_train_head<true> : dfm_train_head<false>,
                       dim3(grid_for_n(B * 64 / 8)), dim3(256), 0, st, idx, y, B, F, E, w,
                       features_M, k, at(p.off_H[L]), p.d[L], ldL, Wp, bp, at(p.off_G[L]),
                       at(p.off_g), at(p.off_dWp), at(p.off_dw), scal,
                       det ? sf(d.heads) : nullptr,
                       det ? reinterpret_cast<double*>(sc + d.loss) : nullptr, head);
    if (sig && !det) hipLaunchKernelGGL(dfm_mean_loss, dim3(1), dim3(1), 0, st, scal, (float)B);
    if (det) {
      hipLaunchKernelGGL(det_columns, dim3(D), dim3(256), 0, st, sf(d.heads), B, (int64_t)D,
                         at(p.off_dWp));
    }
    launch_tr_pad(at(p.off_G[L]), B, p.d[L], ldL, nullptr, 0, at(p.off_GT[L]), Bp, Bp, st);
    // backward through the layers
    for (int i = L - 1; i >= 0; --i) {
      const int din = p.d[i], dout = p.d[i + 1];
      // H_iᵀ (transposed activations; the gathered table rows for i = 0)
      if (i == 0)
        hipLaunchKernelGGL(gather_tr, dim3((unsigned)((Bp + 31) / 32), (unsigned)((din + 31) / 32)),
                           dim3(256), 0, st, idx, B, F, E, features_M, k, at(p.off_HT[0]), Bp);
      else
        launch_tr_pad(at(p.off_H[i]), B, din, pad8(din), nullptr, 0, at(p.off_HT[i]), Bp, Bp, st);
      // dW_i = H_iᵀ · G_{i+1}
      launch_gemm(gemm_plain(din, dout, Bp, at(p.off_HT[i]), Bp, at(p.off_GT[i + 1]), Bp,
                             at(p.off_dW[i]), dout),
                  false, 0, st);
      hipLaunchKernelGGL(row_sums, dim3((unsigned)((dout + 3) / 4)), dim3(256), 0, st,
                         at(p.off_GT[i + 1]), dout, Bp, Bp, at(p.off_db[i]));
      // G_i = (G_{i+1} · W_iᵀ) ⊙ relu'(H_i), or dX0 = G_1 · W_0ᵀ
      launch_gemm(gemm_plain(B, din, dout, at(p.off_G[i + 1]), pad8(dout), at(p.off_WP[i]),
                             pad8(dout), i == 0 ? at(p.off_dX0) : at(p.off_G[i]),
                             i == 0 ? p.D0 : pad8(din)),
                  false, 0, st);
      if (i > 0)
        launch_tr_pad(at(p.off_G[i]), B, din, pad8(din), at(p.off_H[i]), pad8(din),
                      at(p.off_GT[i]), Bp, Bp, st);
    }
    if (!det) {
      hipLaunchKernelGGL(dfm_train_scatter<false>, dim3(grid_for_n(B * 64)), dim3(256), 0, st,
                         idx, B, F, E, features_M, k, at(p.off_dX0), at(p.off_g), Wp,
                         at(p.off_dE), nullptr, head);
    } else {
      hipLaunchKernelGGL(dfm_train_scatter<true>, dim3(grid_for_n(B * 64)), dim3(256), 0, st, idx,
                         B, F, E, features_M, k, at(p.off_dX0), at(p.off_g), Wp, sf(d.rowvec),
                         sf(d.bias), head);
      const OccSource src{idx, nullptr, F, 0, 0, 0, 0, 0};
      const int rc = det_scatter(d, sc, src, F, B, features_M, E, k, at(p.off_dE), at(p.off_dw),
                                 at(p.off_g), scal, StoredContrib{sf(d.rowvec), sf(d.bias), k}, st);
      if (rc != 0) return rc;
      if (sig) hipLaunchKernelGGL(dfm_mean_loss, dim3(1), dim3(1), 0, st, scal, (float)B);
    }
  }
  // optimizer: λ only on the layer weights and the concat projection
  // (DFM.py:146-152); the table and w have IndexedSlices gradients (sparse)
  OptVar vars[2 * kDfmTrainMaxLayers + 4];
  int nv = 0;
  vars[nv++] = {E, at(p.off_dE), slot_of(optimizer, acc, 0), features_M * k, 0.f, k, true, false};
  if (fm)   // (without FM dw stays zero: the head adds nothing, the segment pass stores 0)
    vars[nv++] = {w, at(p.off_dw), slot_of(optimizer, acc, 1), features_M, 0.f, 1, true, false};
  for (int i = 0; deep && i < L; ++i) {
    const int64_t n = (int64_t)p.d[i] * p.d[i + 1];
    if (B == 0) {   // no backward pass wrote this batch's dW / db
      (void)hipMemsetAsync(at(p.off_dW[i]), 0, n * 4, st);
      (void)hipMemsetAsync(at(p.off_db[i]), 0, p.d[i + 1] * 4, st);
    }
    vars[nv++] = {W[i], at(p.off_dW[i]), slot_of(optimizer, acc, 2 + i), n, lambda_l2, 1, false,
                  true};
    vars[nv++] = {bias[i], at(p.off_db[i]), slot_of(optimizer, acc, 2 + L + i), p.d[i + 1], 0.f,
                  1, false, false};
  }
  vars[nv++] = {Wp, at(p.off_dWp), slot_of(optimizer, acc, 2 + 2 * L), D, lambda_l2, 1, false,
                true};
  vars[nv++] = {bp, scal + kScalBiasGrad, slot_of(optimizer, acc, 3 + 2 * L), 1, 0.f, 1, false,
                false};
  uint8_t* touched = reinterpret_cast<uint8_t*>(at(p.off_touch));
  return optimizer_tail(vars, nv, {{idx, B * F}}, features_M, optimizer, lr, scal, touched,
                        lambda_l2, loss, st, det ? sf(d.sspart) : nullptr);
}

extern "C" int hhfm_dfm_train_step(const int32_t* idx, const float* y, int64_t B, int32_t F,
                                   float* E, float* w, int64_t features_M, int32_t k,
                                   int32_t nlayers, const int32_t* layer_dims, float* const* W,
                                   float* const* bias, float* Wp, float* bp, float lr,
                                   float lambda_l2, int32_t optimizer, float* const* acc,
                                   void* workspace, size_t ws_bytes, float* loss,
                                   void* stream) {
  return dfm_train_step_impl(idx, y, B, F, E, w, features_M, k, nlayers, layer_dims, W, bias, Wp,
                             bp, lr, lambda_l2, optimizer, acc, workspace, ws_bytes, false,
                             nullptr, 0, loss, stream);
}

extern "C" int hhfm_dfm_train_step_det(const int32_t* idx, const float* y, int64_t B, int32_t F,
                                       float* E, float* w, int64_t features_M, int32_t k,
                                       int32_t nlayers, const int32_t* layer_dims,
                                       float* const* W, float* const* bias, float* Wp, float* bp,
                                       float lr, float lambda_l2, int32_t optimizer,
                                       float* const* acc, void* workspace, size_t ws_bytes,
                                       void* scratch, size_t scratch_bytes, float* loss,
                                       void* stream) {
  return dfm_train_step_impl(idx, y, B, F, E, w, features_M, k, nlayers, layer_dims, W, bias, Wp,
                             bp, lr, lambda_l2, optimizer, acc, workspace, ws_bytes, true, scratch,
                             scratch_bytes, loss, stream);
}

extern "C" int hhfm_dfm_train_step_head(const int32_t* idx, const float* y, int64_t B, int32_t F,
                                        float* E, float* w, int64_t features_M, int32_t k,
                                        int32_t nlayers, const int32_t* layer_dims,
                                        float* const* W, float* const* bias, float* Wp,
                                        float* bp, float lr, float lambda_l2, int32_t optimizer,
                                        float* const* acc, void* workspace, size_t ws_bytes,
                                        float* loss, void* stream, int32_t head) {
  return dfm_train_step_impl(idx, y, B, F, E, w, features_M, k, nlayers, layer_dims, W, bias, Wp,
                             bp, lr, lambda_l2, optimizer, acc, workspace, ws_bytes, false,
                             nullptr, 0, loss, stream, head);
}

extern "C" int hhfm_dfm_train_step_head_det(const int32_t* idx, const float* y, int64_t B,
                                            int32_t F, float* E, float* w, int64_t features_M,
                                            int32_t k, int32_t nlayers,
                                            const int32_t* layer_dims, float* const* W,
                                            float* const* bias, float* Wp, float* bp, float lr,
                                            float lambda_l2, int32_t optimizer,
                                            float* const* acc, void* workspace, size_t ws_bytes,
                                            void* scratch, size_t scratch_bytes, float* loss,
                                            void* stream, int32_t head) {
  return dfm_train_step_impl(idx, y, B, F, E, w, features_M, k, nlayers, layer_dims, W, bias, Wp,
                             bp, lr, lambda_l2, optimizer, acc, workspace, ws_bytes, true, scratch,
                             scratch_bytes, loss, stream, head);
}

extern "C" int hhfm_dfm_train_det_scratch(int64_t B, int32_t F, int32_t k, int64_t features_M,
                                          int32_t nlayers, const int32_t* layer_dims,
                                          size_t* bytes) {
  DfmTrainPlan p;
  DetPlan d;
  if (!bytes || !layer_dims || B < 0 || features_M < 1 ||
      !dfm_train_plan(B, F, k, features_M, nlayers, layer_dims, p) ||
      !dfm_det_plan(B, F, k, features_M, p, d))
    return HHFM_EINVAL;
  *bytes = d.bytes;
  return HHFM_OK;
}

extern "C" int hhfm_afm_train_workspace(int64_t B, int32_t F, int32_t k, int32_t A,
                                        int64_t features_M, size_t* ws_bytes) {
  AfmTrainPlan p;
  if (!ws_bytes || !afm_train_plan(B, F, k, A, features_M, p)) return HHFM_EINVAL;
  *ws_bytes = (size_t)p.total * 4;
  return HHFM_OK;
}

// the AFM workspace's persistent prefix (as hhfm_dfm_train_state_bytes)
extern "C" int hhfm_afm_train_state_bytes(int32_t F, int32_t k, int32_t A, int64_t features_M,
                                          size_t* state_bytes) {
  AfmTrainPlan p;
  if (!state_bytes || !afm_train_plan(1, F, k, A, features_M, p)) return HHFM_EINVAL;
  *state_bytes = (size_t)p.state * 4;
  return HHFM_OK;
}

extern "C" int hhfm_afm_train_step(const int32_t* idx, const float* y, int64_t B, int32_t F,
                                   float* E, float* w, float* w0, int64_t features_M, int32_t k,
                                   int32_t A, float* W, float* b, float* pvec, float* P,
                                   float lr, float lambda_att, int32_t optimizer,
                                   float* const* acc, void* workspace, size_t ws_bytes,
                                   float* loss, void* stream) {
  return hhfm_afm_train_step_ex(idx, y, B, F, E, w, w0, features_M, k, A, W, b, pvec, P, lr,
                                lambda_att, optimizer, 1.f, 1.f, 0, acc, workspace, ws_bytes,
                                loss, stream);
}

// The AFM step: the default path (det false; scratch unused), or the
// deterministic one on `scratch` (hhfm_afm_train_det_scratch bytes).
static int afm_train_step_impl(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                               float* w, float* w0, int64_t features_M, int32_t k, int32_t A,
                               float* W, float* b, float* pvec, float* P, float lr,
                               float lambda_att, int32_t optimizer, float keep_att,
                               float keep_afm, uint64_t seed, float* const* acc, void* workspace,
                               size_t ws_bytes, bool det, void* scratch, size_t scratch_bytes,
                               float* loss, void* stream) {
  AfmTrainPlan p;
  DetPlan d{};
  if (!afm_train_plan(B, F, k, A, features_M, p) || !keep_ok(keep_att) || !keep_ok(keep_afm) ||
      (det && !afm_det_plan(B, F, k, A, features_M, d)))
    return HHFM_EINVAL;
  const bool drop = keep_att < 1.f || keep_afm < 1.f;
  const DropoutArgs dr = dropout_args(keep_att, keep_afm, seed);
  if (!opt_ok(optimizer)) return HHFM_EUNSUPPORTED;
  if (!E || !w || !w0 || !W || !b || !pvec || !P || !loss || !workspace) return HHFM_EINVAL;
  if (B > 0 && (!idx || !y)) return HHFM_EINVAL;
  if (!slots_ok(optimizer, acc, 7)) return HHFM_EINVAL;   // acc: E, w, w0, W, b, pvec, P
  if (ws_bytes < (size_t)p.total * 4) return HHFM_EWORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (det) {
    if (!scratch) return HHFM_EINVAL;
    if (scratch_bytes < d.bytes) return HHFM_EWORKSPACE;
    if (const int rc = det_sort_fits(d, st)) return rc;
  }
  char* sc = reinterpret_cast<char*>(scratch);
  auto sf = [&](size_t off) { return reinterpret_cast<float*>(sc + off); };
  float* ws = reinterpret_cast<float*>(workspace);
  auto at = [&](int64_t off) { return ws + off; };
  float* scal = at(p.off_scal);
  float* PT = at(p.off_T);
  float* GzT = PT + (int64_t)k * p.Kp;

  if (B > 0) {
    // Wᵀ [A][k] for the forward GEMM
    launch_tr_pad(W, k, A, A, nullptr, 0, at(p.off_Wt), k, k, st);
    {   // R = relu(pairs · W + b)   (AFM.py:117-121)
      GemmArgs g = gemm_plain(p.n, A, k, nullptr, 0, at(p.off_Wt), k, at(p.off_R), A);
      g.pair_mode = 1;
      g.P = p.np;
      g.gidx = idx;
      g.T = E;
      g.Mtab = features_M;
      g.F = F;
      g.kf = k;
      g.bias = b;
      g.relu = 1;
      launch_gemm(g, false, 0, st);
    }
    // a few rows per wave: the per-wave dP / dp / db flush is k + 2A same-address atomics
    const unsigned hb = (unsigned)std::min<int64_t>(256, (B + 3) / 4);
    auto head = det ? (drop ? afm_train_head<true, true> : afm_train_head<false, true>)
                    : (drop ? afm_train_head<true> : afm_train_head<false>);
    hipLaunchKernelGGL(head, dim3(hb), dim3(256), 0, st, idx, y, B, F, E, w, w0, features_M, k, A,
                       at(p.off_R), pvec, P, at(p.off_Gz), PT, GzT, p.Kp, at(p.off_att),
                       at(p.off_g), at(p.off_dP), at(p.off_dpv), at(p.off_db), at(p.off_dw), scal,
                       dr, det ? sf(d.heads) : nullptr,
                       det ? reinterpret_cast<double*>(sc + d.loss) : nullptr);
    if (det) {   // row values [B][k + 2A]: dP, then dp, then db
      const int64_t ld = k + 2 * A;
      hipLaunchKernelGGL(det_columns, dim3(k), dim3(256), 0, st, sf(d.heads), B, ld,
                         at(p.off_dP));
      hipLaunchKernelGGL(det_columns, dim3(A), dim3(256), 0, st, sf(d.heads) + k, B, ld,
                         at(p.off_dpv));
      hipLaunchKernelGGL(det_columns, dim3(A), dim3(256), 0, st, sf(d.heads) + k + A, B, ld,
                         at(p.off_db));
    }
    if (p.Kp > p.n)
      hipLaunchKernelGGL(zero_cols, dim3(grid_for_n((int64_t)(k + A) * (p.Kp - p.n))),
                         dim3(256), 0, st, PT, k + A, p.Kp, p.n);
    // DP = dZ · Wᵀ   (Bt = W [k][A])
    launch_gemm(gemm_plain(p.n, k, A, at(p.off_Gz), A, W, A, at(p.off_DP), k), false, 0, st);
    {   // dW = pairsᵀ · dZ, split over the combos
      GemmArgs g = gemm_plain(k, A, p.Kp, PT, p.Kp, GzT, p.Kp, at(p.off_part), A);
      g.ksplit = kAfmSplitK;
      g.cz_stride = (int64_t)k * A;
      launch_gemm(g, false, 0, st);
      hipLaunchKernelGGL(sum_splits, dim3(grid_for_n((int64_t)k * A)), dim3(256), 0, st,
                         (const float*)at(p.off_part), p.S, (int64_t)k * A, at(p.off_dW));
    }
    if (!det) {
      hipLaunchKernelGGL(drop ? afm_train_scatter<true> : afm_train_scatter<false>,
                         dim3(grid_for_n(B * 64)), dim3(256), 0, st, idx, B, F, E, features_M, k,
                         at(p.off_DP), at(p.off_att), at(p.off_g), P, at(p.off_dE), dr, nullptr);
    } else {
      auto scat = drop ? afm_train_scatter<true, true> : afm_train_scatter<false, true>;
      hipLaunchKernelGGL(scat, dim3(grid_for_n(B * 64)), dim3(256), 0, st, idx, B, F, E, features_M, k,
                         at(p.off_DP), at(p.off_att), at(p.off_g), P, sf(d.rowvec), dr,
                         sf(d.bias));
      const OccSource src{idx, nullptr, F, 0, 0, 0, 0, 0};
      const int rc = det_scatter(d, sc, src, F, B, features_M, E, k, at(p.off_dE), at(p.off_dw),
                                 at(p.off_g), scal, StoredContrib{sf(d.rowvec), sf(d.bias), k}, st);
      if (rc != 0) return rc;
    }
  }
  // the table and w have IndexedSlices gradients (sparse); l2_regularizer(λ)
  // on attention_W only (AFM.py:146)
  auto slot = [&](int i) { return slot_of(optimizer, acc, i); };
  const OptVar vars[] = {
      {E, at(p.off_dE), slot(0), features_M * k, 0.f, k, true, false},
      {w, at(p.off_dw), slot(1), features_M, 0.f, 1, true, false},
      {w0, scal + kScalBiasGrad, slot(2), 1, 0.f, 1, false, false},
      {W, at(p.off_dW), slot(3), (int64_t)k * A, lambda_att, 1, false, true},
      {b, at(p.off_db), slot(4), A, 0.f, 1, false, false},
      {pvec, at(p.off_dpv), slot(5), A, 0.f, 1, false, false},
      {P, at(p.off_dP), slot(6), k, 0.f, 1, false, false}};
  uint8_t* touched = reinterpret_cast<uint8_t*>(at(p.off_touch));
  return optimizer_tail(vars, (int)std::size(vars), {{idx, B * F}}, features_M, optimizer, lr,
                        scal, touched, lambda_att, loss, st, det ? sf(d.sspart) : nullptr);
}

extern "C" int hhfm_afm_train_step_ex(const int32_t* idx, const float* y, int64_t B, int32_t F,
                                      float* E, float* w, float* w0, int64_t features_M,
                                      int32_t k, int32_t A, float* W, float* b, float* pvec,
                                      float* P, float lr, float lambda_att, int32_t optimizer,
                                      float keep_att, float keep_afm, uint64_t seed,
                                      float* const* acc, void* workspace, size_t ws_bytes,
                                      float* loss, void* stream) {
  return afm_train_step_impl(idx, y, B, F, E, w, w0, features_M, k, A, W, b, pvec, P, lr,
                             lambda_att, optimizer, keep_att, keep_afm, seed, acc, workspace,
                             ws_bytes, false, nullptr, 0, loss, stream);
}

extern "C" int hhfm_afm_train_step_det(const int32_t* idx, const float* y, int64_t B, int32_t F,
                                       float* E, float* w, float* w0, int64_t features_M,
                                       int32_t k, int32_t A, float* W, float* b, float* pvec,
                                       float* P, float lr, float lambda_att, int32_t optimizer,
                                       float keep_att, float keep_afm, uint64_t seed,
                                       float* const* acc, void* workspace, size_t ws_bytes,
                                       void* scratch, size_t scratch_bytes, float* loss,
                                       void* stream) {
  return afm_train_step_impl(idx, y, B, F, E, w, w0, features_M, k, A, W, b, pvec, P, lr,
                             lambda_att, optimizer, keep_att, keep_afm, seed, acc, workspace,
                             ws_bytes, true, scratch, scratch_bytes, loss, stream);
}

extern "C" int hhfm_afm_train_det_scratch(int64_t B, int32_t F, int32_t k, int32_t A,
                                          int64_t features_M, size_t* bytes) {
  AfmTrainPlan p;
  DetPlan d;
  if (!bytes || !afm_train_plan(B, F, k, A, features_M, p) ||
      !afm_det_plan(B, F, k, A, features_M, d))
    return HHFM_EINVAL;
  *bytes = d.bytes;
  return HHFM_OK;
}


extern "C" int hhfm_afm_noatt_train_workspace(int64_t features_M, int32_t k, size_t* ws_bytes) {
  if (!ws_bytes || features_M < 1 || k < 1) return HHFM_EINVAL;
  if (k > kNoAttMaxK) return HHFM_EUNSUPPORTED;
  *ws_bytes = afm_noatt_plan(features_M, k).bytes;
  return HHFM_OK;
}

// The attention=0 step: the default path (det false; scratch unused), or the
// deterministic one on `scratch` (hhfm_afm_noatt_train_det_scratch bytes).
static int afm_noatt_step_impl(const int32_t* idx, const float* y, int64_t B, int32_t F, float* E,
                               float* w, float* w0, float* P, int64_t features_M, int32_t k,
                               float lr, int32_t optimizer, float keep_afm, uint64_t seed,
                               float* const* acc, void* workspace, size_t ws_bytes, bool det,
                               void* scratch, size_t scratch_bytes, float* loss, void* stream) {
  if (B < 0 || F < 1 || k < 1 || features_M < 1 || !keep_ok(keep_afm)) return HHFM_EINVAL;
  if (k > kNoAttMaxK) return HHFM_EUNSUPPORTED;
  if (!opt_ok(optimizer)) return HHFM_EUNSUPPORTED;
  if (!E || !w || !w0 || !P || !loss || !workspace) return HHFM_EINVAL;
  if (B > 0 && (!idx || !y)) return HHFM_EINVAL;   // an empty batch reads no rows
  if (!slots_ok(optimizer, acc, 4)) return HHFM_EINVAL;   // acc: E, w, w0, P
  const NoAttPlan p = afm_noatt_plan(features_M, k);
  if (ws_bytes < p.bytes) return HHFM_EWORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return HHFM_EINVAL;   // the double sums
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  DetPlan d{};
  if (det) {
    if (!afm_noatt_det_plan(B, F, k, features_M, d) || !scratch) return HHFM_EINVAL;
    if (scratch_bytes < d.bytes) return HHFM_EWORKSPACE;
    if (const int rc = det_sort_fits(d, st)) return rc;
  }
  char* base = reinterpret_cast<char*>(workspace);
  float* ws = reinterpret_cast<float*>(workspace);
  float* scal = ws + p.fm.off_scal;
  float* dP = reinterpret_cast<float*>(base + p.off_dP);
  double* dP64 = reinterpret_cast<double*>(base + p.off_dP64);
  char* sc = reinterpret_cast<char*>(scratch);
  const bool drop = keep_afm < 1.f;
  const DropoutArgs dr = dropout_args(1.f, keep_afm, seed);
  if (B > 0 && !det) {
    auto rows = drop ? afm_noatt_train_rows<true, false> : afm_noatt_train_rows<false, false>;
    hipLaunchKernelGGL(rows, dim3(bn_grid(B)), dim3(256), 0, st, idx, y, B, F, E, w, w0, P,
                       features_M, k, ws + p.fm.off_dE, ws + p.fm.off_dw, scal, dP64, dr, nullptr,
                       nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(afm_noatt_dp, dim3(1), dim3(256), 0, st, k, dP64, dP);
  } else if (B > 0) {
    float* gb = reinterpret_cast<float*>(sc + d.g);
    float* Sb = reinterpret_cast<float*>(sc + d.rowvec);
    float* Vb = reinterpret_cast<float*>(sc + d.heads);
    auto rows = drop ? afm_noatt_train_rows<true, true> : afm_noatt_train_rows<false, true>;
    hipLaunchKernelGGL(rows, dim3(grid_for_n(B * 64)), dim3(256), 0, st, idx, y, B, F, E, w, w0, P,
                       features_M, k, nullptr, nullptr, nullptr, nullptr, dr, gb,
                       reinterpret_cast<double*>(sc + d.loss), Sb, Vb);
    hipLaunchKernelGGL(det_columns, dim3(k), dim3(256), 0, st, Vb, B, (int64_t)k, dP);
    const OccSource src{idx, nullptr, F, 0, 0, 0, 0, 0};
    const int rc =
        drop ? det_scatter(d, sc, src, F, B, features_M, E, k, ws + p.fm.off_dE, ws + p.fm.off_dw,
                           gb, scal, NoAttContrib<true>{gb, Sb, P, B, F, k, keep_afm}, st)
             : det_scatter(d, sc, src, F, B, features_M, E, k, ws + p.fm.off_dE, ws + p.fm.off_dw,
                           gb, scal, NoAttContrib<false>{gb, Sb, P, B, F, k, keep_afm}, st);
    if (rc != 0) return rc;
  }
  // E and w have IndexedSlices gradients (sparse), w0 and P dense; no variable
  // carries an l2 term (AFM.py:148) and the loss none
  auto slot = [&](int i) { return slot_of(optimizer, acc, i); };
  const OptVar vars[] = {{E, ws + p.fm.off_dE, slot(0), features_M * k, 0.f, k, true, false},
                         {w, ws + p.fm.off_dw, slot(1), features_M, 0.f, 1, true, false},
                         {w0, scal + kScalBiasGrad, slot(2), 1, 0.f, 1, false, false},
                         {P, dP, slot(3), k, 0.f, 1, false, false}};
  uint8_t* touched = reinterpret_cast<uint8_t*>(ws + p.fm.off_touch);
  return optimizer_tail(vars, (int)std::size(vars), {{idx, B * F}}, features_M, optimizer, lr,
                        scal, touched, 0.f, loss, st);
}

extern "C" int hhfm_afm_noatt_train_step(const int32_t* idx, const float* y, int64_t B, int32_t F,
                                         float* E, float* w, float* w0, float* P,
                                         int64_t features_M, int32_t k, float lr,
                                         int32_t optimizer, float keep_afm, uint64_t seed,
                                         float* const* acc, void* workspace, size_t ws_bytes,
                                         float* loss, void* stream) {
  return afm_noatt_step_impl(idx, y, B, F, E, w, w0, P, features_M, k, lr, optimizer, keep_afm,
                             seed, acc, workspace, ws_bytes, false, nullptr, 0, loss, stream);
}

extern "C" int hhfm_afm_noatt_train_step_det(const int32_t* idx, const float* y, int64_t B,
                                             int32_t F, float* E, float* w, float* w0, float* P,
                                             int64_t features_M, int32_t k, float lr,
                                             int32_t optimizer, float keep_afm, uint64_t seed,
                                             float* const* acc, void* workspace, size_t ws_bytes,
                                             void* scratch, size_t scratch_bytes, float* loss,
                                             void* stream) {
  return afm_noatt_step_impl(idx, y, B, F, E, w, w0, P, features_M, k, lr, optimizer, keep_afm,
                             seed, acc, workspace, ws_bytes, true, scratch, scratch_bytes, loss,
                             stream);
}

extern "C" int hhfm_afm_noatt_train_det_scratch(int64_t B, int32_t F, int32_t k,
                                                int64_t features_M, size_t* bytes) {
  DetPlan d;
  if (!bytes || F < 1 || !afm_noatt_det_plan(B, F, k, features_M, d)) return HHFM_EINVAL;
  if (k > kNoAttMaxK) return HHFM_EUNSUPPORTED;
  *bytes = d.bytes;
  return HHFM_OK;
}
