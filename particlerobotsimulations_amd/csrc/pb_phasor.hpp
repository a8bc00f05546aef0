// pb_phasor.hpp -- the phasor kit of the reciprocal-space analyses (pb_sfactor.hip, pb_scatter.hip): exp(i k.r) as one entry of
// an integer cosine/sine table, so that sums of phasors are integers like every other sum of the analysis layer.
// The arithmetic part compiles as plain C++ (tests/pb_phasor_check.cpp); nothing here needs hipcc.
//
// THE TURN.  Positions are quantised as pb_fixed.hpp quantises them (units of 2^-20) and the box is L = 2^e, so
// k.r / 2 pi = (nx qx + ny qy) 2^-20 2^-e is a binary fraction, known exactly mod 1: as a 32-bit fraction it is
// t = u << (12 - e) with u = (uint32)nx * (uint32)qx + (uint32)ny * (uint32)qy, everything mod 2^32.  With
// -8 <= e <= 12 the shift is 0 ... 20.  Huge |n| alias, as they must.
// THE INDEX.  idx = ((t + 0x80000) >> 20) & 4095: the turn rounded to the nearest of 4096 table steps (a tie rounds up;
// the step just below a whole turn wraps to 0).
// THE TABLE.  C[j] = rint(cos(2 pi j / 4096) 2^30) and S[j] = C[(j - 1024) & 4095], both int.  Every entry is at least
// 7e-4 away from a rounding tie and a double near 2^30 has an ulp of 2e-7, so any faithfully rounded cos gives the same
// integers; tests/test_sfactor_ref.py pins them with a CRC.  The host builds the table once, in double.
#pragma once

#include <math.h>
#include <stdint.h>

#include "particlebot_hip.h"  // PB_PHASOR_BITS, PB_SK_MAX_LOG2

#ifdef __HIP__
#define PB_PHASOR_HD __host__ __device__ __forceinline__
#else
#define PB_PHASOR_HD inline
#endif

constexpr uint32_t PB_PHASOR_STEPS = 1u << PB_PHASOR_BITS;  // 4096 steps per turn
constexpr int PB_PHASOR_UNIT_LOG2 = 30;                     // a table entry is in units of 2^-30
static_assert(PB_PHASOR_BITS == 12, "the index function below is written for 4096 steps");

// what the host derives from the box once: t = u << pbPhasorShift(e), PB_SK_MIN_LOG2 <= e <= PB_SK_MAX_LOG2
PB_PHASOR_HD int pbPhasorShift(int boxLog2) { return PB_SK_MAX_LOG2 - boxLog2; }

// k.r / 2 pi mod 1 as a 32-bit binary fraction, of a bot at (qx, qy) 2^-20 and the wavevector (2 pi / 2^e)(nx, ny)
PB_PHASOR_HD uint32_t pbPhasorTurn(uint32_t nx, uint32_t ny, uint32_t qx, uint32_t qy, int shift) {
  return (nx * qx + ny * qy) << shift;
}

// the table step nearest to the turn t
PB_PHASOR_HD uint32_t pbPhasorIndex(uint32_t t) { return ((t + 0x80000u) >> 20) & (PB_PHASOR_STEPS - 1u); }

// the table, interleaved: cosSin[2 j] = C[j], cosSin[2 j + 1] = S[j] (host, double)
inline void pbPhasorBuild(int *cosSin) {
  const double step = 6.283185307179586476925286766559 / (double)PB_PHASOR_STEPS;
  const double unit = (double)(1u << PB_PHASOR_UNIT_LOG2);
  for (uint32_t j = 0; j < PB_PHASOR_STEPS; j++) cosSin[2u * j] = (int)rint(cos((double)j * step) * unit);
  for (uint32_t j = 0; j < PB_PHASOR_STEPS; j++)
    cosSin[2u * j + 1u] = cosSin[2u * ((j - PB_PHASOR_STEPS / 4u) & (PB_PHASOR_STEPS - 1u))];
}
