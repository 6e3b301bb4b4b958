// Training dropout (tf.nn.dropout, TF 1.x: y = x / keep · floor(keep + u)) on a
// mask this project specifies bit for bit — TF's own random stream cannot be
// reproduced here.  Plain C++, host and device.
//
// Generator: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl
// constants 0x9E3779B9, 0xBB67AE85).  Key = the step's 64-bit seed (low word,
// high word).  Element e of row r at site s reads word (e >> 6) & 3 of the
// block whose counter is
//   c0 = (e & 63) | ((e >> 8) << 6)   c1 = r & 0xffffffff   c2 = r >> 32   c3 = s
// so a lane l of a wave that holds elements l + 64·j finds four consecutive
// j in one block (dropout_lane_block): nothing is generated and thrown away.
// Sites: 0 FM's FM_OUT (n = k), 1 AFM's attention (n = F(F−1)/2 pairs, i < j
// order), 2 AFM's k-vector (n = k).
//   u = float(x >> 9) · 2^-23 (exact)      binary = floorf(keep + u)
// one fp32 add and one floor (tests/dropout_ref.py restates all of it in numpy).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HHFM_HD __host__ __device__ __forceinline__
#else
#define HHFM_HD inline
#endif

namespace hhfm {

constexpr int kDropSiteFm = 0, kDropSiteAfmAtt = 1, kDropSiteAfmVec = 2;

struct Philox4 {
  uint32_t v[4];
};

HHFM_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                              uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// what a step's kernels need of the dropout arguments: keep per site pair
// (FM: keep0; AFM: keep0 attention, keep1 k-vector) and the key
struct DropoutArgs {
  float keep0, keep1;
  uint32_t key0, key1;
};

static inline DropoutArgs dropout_args(float keep0, float keep1, uint64_t seed) {
  return DropoutArgs{keep0, keep1, (uint32_t)seed, (uint32_t)(seed >> 32)};
}

// NaN fails both comparisons
static inline bool keep_ok(float keep) { return keep > 0.f && keep <= 1.f; }

HHFM_HD float dropout_binary(float keep, uint32_t x) {
  return __builtin_floorf(keep + (float)(x >> 9) * 0x1p-23f);
}

// the block of element e (any e >= 0) of row `row` at `site`
HHFM_HD Philox4 dropout_block(uint32_t key0, uint32_t key1, int site, int64_t row, int e) {
  const uint32_t c0 = ((uint32_t)e & 63u) | (((uint32_t)e >> 8) << 6);
  return philox4x32_10(c0, (uint32_t)row, (uint32_t)((uint64_t)row >> 32), (uint32_t)site, key0,
                       key1);
}

// word j of a block without a dynamically indexed array (no scratch)
HHFM_HD uint32_t philox_word(const Philox4& b, int j) {
  return j == 0 ? b.v[0] : j == 1 ? b.v[1] : j == 2 ? b.v[2] : b.v[3];
}

HHFM_HD float dropout_element(uint32_t key0, uint32_t key1, int site, int64_t row, int e,
                              float keep) {
  return dropout_binary(keep, philox_word(dropout_block(key0, key1, site, row, e), (e >> 6) & 3));
}

// A lane walking its elements c = l + 64·j in ascending j: binary of element
// c, generating a block only when c enters a new one (every fourth step).
struct LaneDropout {
  Philox4 blk;
  HHFM_HD float binary(const DropoutArgs& d, float keep, int site, int64_t row, int c) {
    const int j = (c >> 6) & 3;
    if (j == 0) blk = dropout_block(d.key0, d.key1, site, row, c);
    return dropout_binary(keep, philox_word(blk, j));
  }
};

}  // namespace hhfm
