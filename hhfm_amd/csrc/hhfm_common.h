// Shared device helpers for the gfx950 FM-family kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/hhfm.h"

#define HHFM_DEV __device__ __forceinline__

namespace hhfm {

constexpr int kWave = 64;  // CDNA wavefront

// negatives per row of a BPR training step, kept in registers (HHFM and CARS2;
// the reference samples 10, OurModel7.py:371)
constexpr int kMaxNeg = 16;

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// 16-byte load; NT = non-temporal (streamed once: does not displace the
// hot, re-read data — e.g. the FM bias table — from L2 / Infinity Cache)
template <bool NT>
HHFM_DEV u32x4_t load16(const void* p) {
  const u32x4_t* q = reinterpret_cast<const u32x4_t*>(p);
  if constexpr (NT) return __builtin_nontemporal_load(q);
  else return *q;
}

template <bool NT>
HHFM_DEV int32_t load_i32(const int32_t* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

// 16-byte chunk of an embedding row, widened to fp32.
// fp32 rows: 4 elements per chunk; bf16 rows: 8 elements per chunk.
template <bool BF16>
struct Chunk;

template <>
struct Chunk<false> {
  static constexpr int kElems = 4;
  float v[4];
  // from the 16 bytes as loaded (any address space)
  HHFM_DEV void set(const u32x4_t x) {
    v[0] = __uint_as_float(x[0]); v[1] = __uint_as_float(x[1]);
    v[2] = __uint_as_float(x[2]); v[3] = __uint_as_float(x[3]);
  }
  template <bool NT = false>
  HHFM_DEV void load(const void* p) { set(load16<NT>(p)); }
};

template <>
struct Chunk<true> {
  static constexpr int kElems = 8;
  float v[8];
  HHFM_DEV void set(const u32x4_t x) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(x[i] << 16);             // low bf16
      v[2 * i + 1] = __uint_as_float(x[i] & 0xffff0000u);  // high bf16
    }
  }
  template <bool NT = false>
  HHFM_DEV void load(const void* p) { set(load16<NT>(p)); }
};

HHFM_DEV float bf16_to_f32(uint16_t b) { return __uint_as_float(uint32_t(b) << 16); }

// Out-of-range ids are clamped to row 0 so a bad index can never fault the
// device; the Python layer validates ids and raises (TF embedding_lookup
// raises InvalidArgumentError on them).
HHFM_DEV int32_t clamp_id(int32_t id, int64_t M) {
  return (uint64_t)(uint32_t)id < (uint64_t)M ? id : 0;
}

// Record that this wave met an id outside [0, M) in the caller's status word
// (include/hhfm.h, HHFM_STATUS_BAD_ID): one vector atomic per wave that saw
// one, none otherwise; NULL = the caller did not ask.  Every lane of the wave
// must call it (kernel epilogue).
HHFM_DEV void report_bad_id(int32_t* status, bool bad) {
  if (status == nullptr) return;
  const uint64_t m = __ballot(bad);
  if (m != 0 && (threadIdx.x & (kWave - 1)) == (unsigned)(__ffsll((long long)m) - 1))
    atomicOr(status, HHFM_STATUS_BAD_ID);
}

// Query-column id check of hhfm_catalog_topk_ex (status.hip).
int launch_check_query_ids(const int32_t* q, int64_t B, int ncols, int ucol, int c0, int c1,
                           int t0, int t1, int64_t M, int32_t* status, hipStream_t s);

// Butterfly sum over aligned groups of G lanes (G a power of two <= 64).
template <int G>
HHFM_DEV float group_sum(float x) {
#pragma unroll
  for (int m = G / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, kWave);
  return x;
}

// In-register form of group_sum for the row kernels: the same partner (lane
// xor m) and the same order of steps m = G/2 .. 1, so the same bits, with the
// steps m <= 8 done by DPP inside a row of 16 lanes instead of a round trip
// through LDS (__shfl_xor is ds_bpermute_b32 + lgkmcnt wait).  Every lane of
// the wave must be active.
//   m = 8        row_ror:8
//   m = 4, G>=16 row_ror:4 — lane i reads lane (i - 4) mod 16, which is lane
//                i ^ 4 or i ^ 4 ^ 8; after the m = 8 step the two hold the
//                same value
//   m = 4, G = 8 row_shl:4 into banks 0, 2 and row_shr:4 into banks 1, 3
//   m = 2, 1     quad_perm [2,3,0,1], [1,0,3,2]
// The compiler folds each move into v_add_f32_dpp.
constexpr int kDppQuadXor1 = 0xB1;  // quad_perm [1,0,3,2]
constexpr int kDppQuadXor2 = 0x4E;  // quad_perm [2,3,0,1]
constexpr int kDppRowShl4 = 0x104;
constexpr int kDppRowShr4 = 0x114;
constexpr int kDppRowRor4 = 0x124;
constexpr int kDppRowRor8 = 0x128;

template <int CTRL>
HHFM_DEV float dpp_read(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}

// the value of lane xor M (M <= 8 within a row of 16 lanes, else by LDS);
// PERIODIC8: x is known to be equal in lanes i and i ^ 8
template <int M, bool PERIODIC8>
HHFM_DEV float xor_partner(float x) {
  if constexpr (M == 1) return dpp_read<kDppQuadXor1>(x);
  else if constexpr (M == 2) return dpp_read<kDppQuadXor2>(x);
  else if constexpr (M == 4 && PERIODIC8) return dpp_read<kDppRowRor4>(x);
  else if constexpr (M == 4) {
    const int xi = __float_as_int(x);
    int r = __builtin_amdgcn_update_dpp(xi, xi, kDppRowShl4, 0xf, 0x5, false);
    r = __builtin_amdgcn_update_dpp(r, xi, kDppRowShr4, 0xf, 0xa, false);
    return __int_as_float(r);
  } else if constexpr (M == 8) return dpp_read<kDppRowRor8>(x);
  else return __shfl_xor(x, M, kWave);
}

template <int G>
HHFM_DEV float group_sum_dpp(float x) {
  static_assert(G >= 1 && G <= kWave && (G & (G - 1)) == 0, "aligned power-of-two groups");
  if constexpr (G >= 64) x += xor_partner<32, false>(x);
  if constexpr (G >= 32) x += xor_partner<16, false>(x);
  if constexpr (G >= 16) x += xor_partner<8, false>(x);
  if constexpr (G >= 8) x += xor_partner<4, (G >= 16)>(x);
  if constexpr (G >= 4) x += xor_partner<2, false>(x);
  if constexpr (G >= 2) x += xor_partner<1, false>(x);
  return x;
}

// `v` with lane LANE replaced by the wave-uniform `s` (v_writelane_b32; this
// compiler has the readlane builtin but none for writelane)
template <int LANE>
HHFM_DEV int write_lane(int v, int s) {
  static_assert(LANE >= 0 && LANE < kWave, "lane of the wave");
  asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(s), "n"(LANE));
  return v;
}
// lanes 0, 1 of every group of LPR lanes: lane gg * LPR + f <- s[f][gg]
template <int LPR, int RPW, int I = 0>
HHFM_DEV int write_group_lanes01(int v, const float (&s)[2][RPW]) {
  if constexpr (I < 2 * RPW) {
    v = write_lane<(I >> 1) * LPR + (I & 1)>(v, __float_as_int(s[I & 1][I >> 1]));
    return write_group_lanes01<LPR, RPW, I + 1>(v, s);
  } else {
    return v;
  }
}

// 32-bit form of clamp_id for kernels that clamp many ids per iteration:
// M32 = id_limit32(M) once per kernel; an int32 id is in [0, M) iff
// (uint32_t)id < M32 (a negative id is >= 2^31 as unsigned).
HHFM_DEV uint32_t id_limit32(int64_t M) {
  return M < ((int64_t)1 << 31) ? (uint32_t)M : 0x80000000u;
}
HHFM_DEV int32_t clamp_id32(int32_t id, uint32_t M32) { return (uint32_t)id < M32 ? id : 0; }

// CUs of the device that owns `st` (the stream's device, not the calling
// thread's current one), cached per device: the persistent grids ask per call
inline int stream_cu_count(hipStream_t st) {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipStreamGetDevice(st, &dev) != hipSuccess && hipGetDevice(&dev) != hipSuccess) return 256;
  if (dev < 0 || dev >= 64) return 256;
  int c = cache[dev].load(std::memory_order_relaxed);
  if (c <= 0) {
    c = 256;
    (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev);
    cache[dev].store(c, std::memory_order_relaxed);
  }
  return c;
}

}  // namespace hhfm
