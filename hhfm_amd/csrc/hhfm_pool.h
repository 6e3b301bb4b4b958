// HHFM pooling (Pooling1C / Pooling1T / Pooling1F of OurModel7.py:14-19, used
// at :124, :141, :168 and :255, :267, :292): how the context rows, the time
// rows and the stack {user, context pool, time pool} are reduced to the query
// vector h.  The contract is include/hhfm.h "Pooling"; this header is its one
// implementation: the row kernel (fm_rows.hip), the catalog query kernel
// (catalog_topk.hip, catalog_fused.h) and the training forward (train.hip) all
// form h_e through pool_step / pool_finish / pool_h, so they agree on it bit
// for bit.  The sum-only kernels keep their own (older) expressions and are
// not routed through here.
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

}  // namespace hhfm
#endif  // HHFM_POOL_H_
