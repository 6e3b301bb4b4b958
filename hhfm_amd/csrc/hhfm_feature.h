// The three forms of the HHFM query vector h as feature policies: what the
// runtime-shaped, one-wave-per-row kernels — hybrid_rows_generic (fm_rows.hip),
// catalog_queries (catalog_topk.hip) and hhfm_train_rows (train.hip) — are
// instantiated over.  A policy is a kernel argument (its modes stay
// wave-uniform SGPRs) with two operations at one element of the k-vector:
//
//   forward(u, row, c0, c1, t0, t1)
//       u: the user row's value; row(j): the value of column j's embedding
//       row; [c0, c1) / [t0, t1): the context / time columns.  Returns a
//       struct with .h and whatever back() needs again.
//   back(fwd, dh, u, row, c0, c1, t0, t1, emit)
//       the gradient dh of h sent to the rows: emit(j, value) exactly once
//       per row occurrence, in the order user (column kUserCol of a training
//       row), context columns, time columns.  (SumFeature and TwoWayFeature: the
//       policies hhfm_train_rows is instantiated over.)
//
// The expressions are the ones the kernels carried before they were merged,
// in the same order, so every instantiation keeps its bits.
#ifndef HHFM_FEATURE_H_
#define HHFM_FEATURE_H_

#include "hhfm_pool.h"

namespace hhfm {

constexpr int kUserCol = 0, kItemCol = 1;   // a training row: [user, item, ...]

// h = u + Σctx (+ Σtime): each present pool summed from 0 in column order,
// then added to h.  Not pool_step's sum (that one starts from -0).
struct SumFeature {
  struct Fwd {
    float h;
  };
  template <class Row>
  HHFM_DEV Fwd forward(float u, Row row, int c0, int c1, int t0, int t1) const {
    float h = u;
    if (c1 > c0) {
      float s = 0.f;
      for (int j = c0; j < c1; ++j) s += row(j);
      h = h + s;
    }
    if (t1 > t0) {
      float s = 0.f;
      for (int j = t0; j < t1; ++j) s += row(j);
      h = h + s;
    }
    return Fwd{h};
  }
  template <class Row, class Emit>
  HHFM_DEV void back(const Fwd&, float dh, float, Row, int c0, int c1, int t0, int t1,
                     Emit emit) const {
    emit(kUserCol, dh);
    for (int j = c0; j < c1; ++j) emit(j, dh);
    for (int j = t0; j < t1; ++j) emit(j, dh);
  }
};

// MAX / MEAN pooling (include/hhfm.h "Pooling"): h through pool_step /
// pool_finish / pool_h.  A pool is present when its count is > 0; an empty (or
// reversed) range is never read or divided by.  Forward only: the pooled
// training step keeps a kernel of its own (hhfm_train_rows_pool, train.hip),
// which carries the same forward and the pool gradients.
struct PoolFeature {
  PoolModes pm;
  struct Fwd {
    float h, cv, tv;   // cv / tv: the pools' values (a max pool's value is its maximum)
  };
  template <class Row>
  HHFM_DEV Fwd forward(float u, Row row, int c0, int c1, int t0, int t1) const {
    const int nc = c1 - c0, ntm = t1 - t0;
    float cv = pool_identity(pm.ctx), tv = pool_identity(pm.tim);
    for (int j = c0; j < c1; ++j) cv = pool_step(pm.ctx, cv, row(j));
    for (int j = t0; j < t1; ++j) tv = pool_step(pm.tim, tv, row(j));
    cv = pool_finish(pm.ctx, cv, nc);
    tv = pool_finish(pm.tim, tv, ntm);
    return Fwd{pool_h(u, cv, nc, tv, ntm, pm.fin), cv, tv};
  }
};

// Two-way pooling (include/hhfm.h "Two-way pooling"): h from two_way_h.  On
// the way back dh reaches the stack members through H1 (pool_grad) and through
// every member product of H2 (a product sends d·s_n to s_m and d·s_m to s_n);
// each mix's gradient reaches its rows through P1 and through every pair
// product of P2 the same way.  A max pool's ties are found by re-forming the
// fp32 values with the forward's own expressions (pool_mul), so the equality
// tests see the forward's bits.  One emit per row occurrence carries that
// occurrence's summed contribution.  Layouts of two_way_shape_ok only.
struct TwoWayFeature {
  PoolModes2 pm;
  using Fwd = TwoWay;
  template <class Row>
  HHFM_DEV Fwd forward(float u, Row row, int c0, int c1, int t0, int t1) const {
    return two_way_h(
        u, [&](int i) { return row(c0 + i); }, c1 > c0 ? c1 - c0 : 0,
        [&](int i) { return row(t0 + i); }, t1 > t0 ? t1 - t0 : 0, pm);
  }
  // the gradient of one mix (value w, gradient d) towards its n rows [j0, j0 + n)
  template <class Row, class Emit>
  HHFM_DEV static void mix_back(Row row, Emit emit, const Mix2& w, float d, int j0, int n, int m1,
                                int m2) {
    const int np = n * (n - 1) / 2;
    int eq1 = 0, eq2 = 0;
    for (int i = 0; i < n; ++i) {
      const float ri = row(j0 + i);
      eq1 += ri == w.p1;
      for (int j = i + 1; j < n; ++j) eq2 += pool_mul(ri, row(j0 + j)) == w.p2;
    }
    for (int i = 0; i < n; ++i) {
      const float ri = row(j0 + i);
      float acc = pool_grad(m1, d, ri, w.p1, eq1, n);
      for (int j = 0; j < n; ++j) {
        if (j == i) continue;
        const float rj = row(j0 + j);
        acc += pool_grad(m2, d, pool_mul(ri, rj), w.p2, eq2, np) * rj;
      }
      emit(j0 + i, acc);
    }
  }
  template <class Row, class Emit>
  HHFM_DEV void back(const Fwd& w, float dh, float u, Row row, int c0, int c1, int t0, int t1,
                     Emit emit) const {
    const int nc = c1 > c0 ? c1 - c0 : 0, ntm = t1 > t0 ? t1 - t0 : 0;
    const int members = 1 + (nc > 0) + (ntm > 0);       // 2 or 3 (two_way_shape_ok)
    // the stack: s0 = u, then mix_c, then mix_t; h = H1 + H2 sends dh to both
    const float sc = w.c.mix, st = w.t.mix;
    const int feq = (u == w.h1) + (nc > 0 && sc == w.h1) + (ntm > 0 && st == w.h1);
    float du = pool_grad(pm.one.fin, dh, u, w.h1, feq, members);
    float dc = nc > 0 ? pool_grad(pm.one.fin, dh, sc, w.h1, feq, members) : 0.f;
    float dt = ntm > 0 ? pool_grad(pm.one.fin, dh, st, w.h1, feq, members) : 0.f;
    if (members == 3) {
      const float p01 = pool_mul(u, sc), p02 = pool_mul(u, st), p12 = pool_mul(sc, st);
      const int e2 = (p01 == w.h2) + (p02 == w.h2) + (p12 == w.h2);
      const float g01 = pool_grad(pm.two.fin, dh, p01, w.h2, e2, 3);
      const float g02 = pool_grad(pm.two.fin, dh, p02, w.h2, e2, 3);
      const float g12 = pool_grad(pm.two.fin, dh, p12, w.h2, e2, 3);
      du += g01 * sc + g02 * st;
      dc += g01 * u + g12 * st;
      dt += g02 * u + g12 * sc;
    } else {                                          // one product: H2 = u · s under every mode
      const float s = nc > 0 ? sc : st;
      du += dh * s;
      if (nc > 0) dc += dh * u; else dt += dh * u;
    }
    emit(kUserCol, du);
    if (nc > 0) mix_back(row, emit, w.c, dc, c0, nc, pm.one.ctx, pm.two.ctx);
    if (ntm > 0) mix_back(row, emit, w.t, dt, t0, ntm, pm.one.tim, pm.two.tim);
  }
};

}  // namespace hhfm
#endif  // HHFM_FEATURE_H_
