// HHFM pooling (Pooling1C / Pooling1T / Pooling1F of OurModel7.py:14-19, used
// at :124, :141, :168 and :255, :267, :292): how the context rows, the time
// rows and the stack {user, context pool, time pool} are reduced to the query
// vector h.  The contract is include/hhfm.h "Pooling"; this header is its one
// implementation: the row kernel (fm_rows.hip), the catalog query kernel
// (catalog_topk.hip, catalog_fused.h) and the training forward (train.hip) all
// form h_e through pool_step / pool_finish / pool_h, so they agree on it bit
// for bit.  hhfm_feature.h wraps these helpers, and the original sum's own
// expressions (which start from +0, not from pool_identity), as the feature
// policies the runtime-shaped kernels are instantiated over.
#ifndef HHFM_POOL_H_
#define HHFM_POOL_H_

#include "hhfm_common.h"

namespace hhfm {

struct PoolModes {
  int ctx, tim, fin;
};

// the packed word's fields; false: a mode outside {sum, max, mean} or a stray bit
inline bool pooling_unpack(int32_t pooling, PoolModes& m) {
  if (pooling & ~0xfff) return false;
  m.ctx = pooling & 15;
  m.tim = (pooling >> 4) & 15;
  m.fin = (pooling >> 8) & 15;
  return m.ctx <= HHFM_POOL_MEAN && m.tim <= HHFM_POOL_MEAN && m.fin <= HHFM_POOL_MEAN;
}

// One pool at one element is a single accumulator.  It starts from the mode's
// identity — -0.0f for a sum ((-0) + x and x + (-0) are x for every x, signed
// zeros included), -inf for a maximum — so stepping it through the pool's
// values in column order gives ((r0 + r1) + ...) or the largest value to the
// bit, as if it had started from the first row, and a value outside the pool
// can be stepped in as the identity without a branch.
HHFM_DEV float pool_identity(int mode) {
  return mode == HHFM_POOL_MAX ? -__builtin_huge_valf() : -0.f;
}
// max(a, b) as v_med3_f32(a, b, +inf): no canonicalising copies of the operands
HHFM_DEV float pool_max(float a, float b) {
  return __builtin_amdgcn_fmed3f(a, b, __builtin_huge_valf());
}
HHFM_DEV float pool_step(int mode, float acc, float v) {
  return mode == HHFM_POOL_MAX ? pool_max(acc, v) : acc + v;
}
// the pool's value from its accumulator over n values: the mean is the sum,
// then one correctly rounded fp32 division by (float)n
HHFM_DEV float pool_finish(int mode, float acc, int n) {
  return mode == HHFM_POOL_MEAN ? acc / (float)n : acc;
}

// h_e from the user value and the two pools' values cv, tv (of nc / nt rows;
// 0 rows: that stack member is absent and its value is ignored).  Members in
// the order user, context pool, time pool: sum (u + c) + t, max the largest,
// mean the sum form / count; a single member: h = u.
HHFM_DEV float pool_h(float u, float cv, int nc, float tv, int nt, int fin) {
  const float id = pool_identity(fin);
  float h = pool_step(fin, u, nc > 0 ? cv : id);
  h = pool_step(fin, h, nt > 0 ? tv : id);
  const int members = 1 + (nc > 0) + (nt > 0);
  return members == 1 ? u : pool_finish(fin, h, members);
}

// TF's gradient of one pool towards one of its n values v (math_grad.py
// _SumGrad / _MeanGrad / _MinOrMaxGrad): sum d; mean d / n; max d / (number of
// values equal to the maximum mx) for those values, 0 for the others.
HHFM_DEV float pool_grad(int mode, float d, float v, float mx, int n_equal, int n) {
  if (mode == HHFM_POOL_MAX) return v == mx ? d / (float)n_equal : 0.f;
  return mode == HHFM_POOL_MEAN ? d / (float)n : d;
}

// ---------------------------------------------------------------------------
// Two-way pooling (include/hhfm.h "Two-way pooling"): the reference's
// commented-out additions of OurModel7.py:124 / :141 / :168 put back.  Each
// pool of rows gains P2, the pool (by pooling2's mode) of its pair products
// r_i · r_j, i < j, i outer, and the stack gains H2 over its member products.
// two_way_h below is the one implementation the generic row kernel, the
// catalog query kernel and the training forward call (through TwoWayFeature
// of hhfm_feature.h), so they agree on h bit for bit; hybrid_rows_two_way
// (fm_rows.hip) unrolls the same expressions over its registers.
// ---------------------------------------------------------------------------
struct PoolModes2 {
  PoolModes one, two;   // pooling (P1, H1) and pooling2 (P2, H2)
};

inline bool pooling2_unpack(int32_t pooling, int32_t pooling2, PoolModes2& m) {
  return pooling_unpack(pooling, m.one) && pooling_unpack(pooling2, m.two);
}

// the layouts the two-way graph exists for: a present pool has two rows or
// more and the stack two members or more (the reference stacks an empty list
// otherwise, OurModel7.py:119 / :136 / :163)
inline bool two_way_shape_ok(int nc, int nt) {
  return nc != 1 && nt != 1 && nc + nt > 0;
}

// One rounded fp32 multiply, never contracted into an FMA with a later add:
// the product's value is compared (max ties), selected and re-formed in the
// backward pass.
HHFM_DEV float pool_mul(float a, float b) {
#pragma clang fp contract(off)
  const float p = a * b;
  return p;
}

struct Mix2 {
  float p1, p2, mix;    // P1, P2, P1 + P2
};

// one pool of n >= 2 rows at one element; row(i): the i-th row's value
template <class Row>
HHFM_DEV Mix2 two_way_mix(Row row, int n, int m1, int m2) {
  float a1 = pool_identity(m1), a2 = pool_identity(m2);
  for (int i = 0; i < n; ++i) {
    const float ri = row(i);
    a1 = pool_step(m1, a1, ri);
    for (int j = i + 1; j < n; ++j) a2 = pool_step(m2, a2, pool_mul(ri, row(j)));
  }
  Mix2 r;
  r.p1 = pool_finish(m1, a1, n);
  r.p2 = pool_finish(m2, a2, n * (n - 1) / 2);
  r.mix = r.p1 + r.p2;
  return r;
}

// H2 from the members u, mix_c (nc > 0), mix_t (nt > 0): the pool of their
// products in the order (0,1), (0,2), (1,2)
HHFM_DEV float two_way_h2(float u, float mc, int nc, float mt, int nt, int fin2) {
  float a = pool_identity(fin2);
  if (nc > 0 && nt > 0) {
    a = pool_step(fin2, a, pool_mul(u, mc));
    a = pool_step(fin2, a, pool_mul(u, mt));
    a = pool_step(fin2, a, pool_mul(mc, mt));
    return pool_finish(fin2, a, 3);
  }
  a = pool_step(fin2, a, pool_mul(u, nc > 0 ? mc : mt));
  return pool_finish(fin2, a, 1);
}

struct TwoWay {
  Mix2 c, t;            // the context and the time pool (unset when absent)
  float h1, h2, h;      // H1, H2, H1 + H2
};

// h at one element, with the intermediate values the backward needs
template <class Ctx, class Tim>
HHFM_DEV TwoWay two_way_h(float u, Ctx ctx, int nc, Tim tim, int nt, const PoolModes2& pm) {
  TwoWay r;
  r.c = r.t = Mix2{0.f, 0.f, 0.f};
  if (nc > 0) r.c = two_way_mix(ctx, nc, pm.one.ctx, pm.two.ctx);
  if (nt > 0) r.t = two_way_mix(tim, nt, pm.one.tim, pm.two.tim);
  r.h1 = pool_h(u, r.c.mix, nc, r.t.mix, nt, pm.one.fin);
  r.h2 = two_way_h2(u, r.c.mix, nc, r.t.mix, nt, pm.two.fin);
  r.h = r.h1 + r.h2;
  return r;
}

}  // namespace hhfm
#endif  // HHFM_POOL_H_
