// pb_fixed.hpp -- the fixed-point kit of the analyses that accumulate exact integers on the device (pb_moments.hip,
// pb_timecorr.hip, pb_vanhove.hip, pb_field.hip, pb_dynamics.hip, pb_correlate.hip; the wave helpers serve pb_cluster.hip,
// pb_contacts.hip and pb_structure.hip too): the quantiser and its range, the split of a 64-bit product into two
// accumulators, the sums over a wave and over a workgroup's four waves, and the host's way back to a pbMoment128.
// The arithmetic part compiles as plain C++ (tests/pb_fixed_check.cpp); the device part needs hipcc.
//
// THE BOUND, stated here once.  A value is MEASURED iff |v| < 2048 (pbFixedInRange; a NaN or an infinity fails the
// comparison).  Then v * 2^20 is exact in fp32 (a scaling by a power of two, no overflow), the largest magnitude is
// (2048 - 2^-13) 2^20 = 2^31 - 128, and rounding to nearest even (v_rndne_f32) gives an integer q with
// |q| <= 2^31 - 128: it fits an int.  A product of two such values is below 2^62 in magnitude and a sum of two products
// below 2^63: it fits a long long.  pbFixedSplitAdd adds such a p as its low 32 bits, 0 <= . < 2^32, and the rest,
// p >> 32 with |.| <= 2^31, to two 64-bit accumulators; over fewer than 2^31 samples both stay below 2^63 in magnitude,
// so nothing wraps, integer adds commute, and lo + hi * 2^32 (pbFixedCompose) is the exact sum whatever order the
// device added in.  Hence the cap every analysis states: fewer than 2^31 samples per pair of words.
#pragma once

#include <stdint.h>

#include "particlebot_hip.h"

#ifdef __HIP__
#define PB_FIXED_HD __host__ __device__ __forceinline__
#else
#define PB_FIXED_HD inline
#endif

constexpr float PB_FIXED_SCALE = 1048576.0f;  // 2^20: a quantised value is in units of 2^-20
constexpr float PB_FIXED_LIMIT = 2048.0f;     // measured iff the magnitude is below this

PB_FIXED_HD bool pbFixedInRange(float v) { return __builtin_fabsf(v) < PB_FIXED_LIMIT; }

// (long long)rint(v * 2^20) of a value in range
PB_FIXED_HD long long pbFixedQuantise(float v) { return (long long)(int)__builtin_rintf(v * PB_FIXED_SCALE); }

// The two's-complement split of a 64-bit p, so that a signed p needs no special case: its low 32 bits and the rest.
// The shift of a signed p is arithmetic, and a sum of rests wraps like the signed sum it stands for; an unsigned p is
// below 2^63 and splits the same way.
template <typename P>
PB_FIXED_HD unsigned long long pbFixedLow(P p) {
  return (unsigned long long)(uint32_t)p;
}
template <typename P>
PB_FIXED_HD unsigned long long pbFixedRest(P p) {
  return (unsigned long long)(p >> 32);
}
// p into its two accumulators
template <typename P>
PB_FIXED_HD void pbFixedSplitAdd(P p, unsigned long long &lo, unsigned long long &hi) {
  lo += pbFixedLow(p);
  hi += pbFixedRest(p);
}

// low part (a sum of 32-bit values) plus signed rest times 2^32: what the two accumulators of a split stand for
inline __int128 pbFixedCompose(unsigned long long low, unsigned long long rest) {
  return (__int128)low + (__int128)(long long)rest * ((__int128)1 << 32);
}

// value = hi * 2^32 + lo with 0 <= lo < 2^32 and hi the floor quotient: the same form however the device split its adds
inline pbMoment128 pbFixedNormalised(__int128 v) {
  pbMoment128 m;
  m.lo = (unsigned long long)(v & (__int128)0xFFFFFFFFull);
  m.hi = (long long)(v >> 32);  // (arithmetic: the floor)
  return m;
}

#ifdef __HIP__
#include "pb_device.hpp"

// ---- wave helpers (wave64) ---------------------------------------------------------------------------------------------
PB_DEV uint32_t waveMaxU32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, m);
    v = o > v ? o : v;
  }
  return v;
}
PB_DEV uint32_t waveSumU32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
  return v;
}
PB_DEV unsigned long long shflXor64(unsigned long long v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
  return ((unsigned long long)hi << 32) | lo;
}
PB_DEV unsigned long long shflUp64(unsigned long long v, int d) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d);
  const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
  return ((unsigned long long)hi << 32) | lo;
}
PB_DEV unsigned long long waveMaxU64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = shflXor64(v, m);
    v = o > v ? o : v;
  }
  return v;
}
PB_DEV unsigned long long waveSumU64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += shflXor64(v, m);
  return v;
}

// The sums of N accumulators over the wave, left in every lane: one butterfly stage in the code, run six
// times (unrolled, the stages' temporaries cost registers that a pass once per workgroup does not earn back).  stage(m)
// is the caller's own work in the stage with partner lane ^ m: a minimum or a maximum that rides along.
template <int N, typename Stage>
PB_DEV void waveSumRolled(unsigned long long (&a)[N], const Stage &stage) {
#pragma unroll 1
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int c = 0; c < N; c++) a[c] += shflXor64(a[c], m);
    stage(m);
  }
}

// The four waves of a 256-lane workgroup through LDS: lane 0 of each wave stores the wave's COLS words, a barrier, and
// thread c < COLS gets true and, in s, column c folded over the waves under opOf(c); the other threads get false.
// Every lane of the workgroup must call it; a caller that comes back for more puts a barrier in between (sRed is
// written again).
enum PbFoldOp { PB_FOLD_SUM, PB_FOLD_MIN_SIGNED, PB_FOLD_MAX_SIGNED, PB_FOLD_MAX_UNSIGNED };
template <int COLS, typename OpOf>
PB_DEV bool blockFold(unsigned long long (&sRed)[4][COLS], const unsigned long long (&mine)[COLS], const OpOf &opOf,
                      unsigned long long &s) {
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (lane == 0u) {
#pragma unroll
    for (int c = 0; c < COLS; c++) sRed[w][c] = mine[c];
  }
  __syncthreads();
  s = 0ull;
  if (threadIdx.x >= (uint32_t)COLS) return false;
  const uint32_t c = threadIdx.x;
  const PbFoldOp op = opOf(c);
  s = sRed[0][c];
  for (int k = 1; k < 4; k++) {
    const unsigned long long u = sRed[k][c];
    if (op == PB_FOLD_SUM) s += u;
    else if (op == PB_FOLD_MIN_SIGNED) s = (long long)u < (long long)s ? u : s;
    else if (op == PB_FOLD_MAX_SIGNED) s = (long long)u > (long long)s ? u : s;
    else s = u > s ? u : s;
  }
  return true;
}
#endif  // __HIP__
