// pb_fourpoint.hpp -- the arithmetic of the four-point recorder that has no device in it (pb_fourpoint.hip holds the
// kernels and the entry points; include/particlebot_hip.h has the definitions): the overlap rule, the words of a
// per-record mode and of a table cell, the signed 128-bit add on two limbs, and what one origin adds to a cell.  The
// product, the sum of two products and the 192-bit add are pb_coherent.hpp's and are not restated.  Compiles as plain C++
// (tests/pb_fourpoint_check.cpp); the kernels, the host's row writer and the check program all use what is here, so
// there is one statement of each rule.
//
// All of it is integer arithmetic.  Per origin pair, member and wavevector the masked mode is (A, B) = (sum w C[idx],
// sum w S[idx]) over the bots, w being the overlap of the pair: two signed 64-bit words with |A|, |B| <= Q 2^30 < 2^58,
// Q = sum w < 2^28.  Over fewer than 2^31 origins: sum Q < 2^59 (one word), sum Q^2 < 2^87 (two limbs), sum A and
// sum B below 2^89 in magnitude (signed 128-bit, two limbs), sum (A^2 + B^2) < 2^148 (three limbs).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "pb_coherent.hpp"
#include "pb_fixed.hpp"

// the words of an origin's mode and of its two counts in the per-record scratch, ...
enum { PB_FP_A, PB_FP_B, PB_FP_MODE_WORDS };
enum { PB_FP_M, PB_FP_Q, PB_FP_COUNT_WORDS };
// ... of a (member, lag, vector) cell: re and im as two limbs each, power as three, one word to spare, ...
enum { PB_FP_RE, PB_FP_IM = 2, PB_FP_POWER = 4, PB_FP_SPARE = 7, PB_FP_WORDS };
// ... and of a (member, lag) cell: the measured pairs, the overlapping ones, and the two limbs of the sum of Q^2
enum { PB_FP_SAMPLES, PB_FP_OVERLAP, PB_FP_OVERLAP2, PB_FP_LAG_WORDS = 4 };
static_assert(PB_FP_MODE_WORDS == 2 && PB_FP_COUNT_WORDS == 2 && PB_FP_WORDS == 8 && PB_FP_LAG_WORDS == 4,
              "16 bytes per mode and per pair of counts; 8 words per vector, 4 per (member, lag)");

// qa = rint(overlapRadius 2^20), formed once on the host in fp32 (the scaling is exact): below 2^31 for a radius below 2048
inline long long pbFpRadiusQuanta(float overlapRadius) { return (long long)__builtin_rintf(overlapRadius * 1048576.0f); }

// THE OVERLAP of a measured pair: the squared length of the difference of the QUANTISED positions, as 64-bit integers,
// is below a2 = qa qa (equality does not overlap; qa == 0 overlaps nothing).  |dqx| < qa and |dqy| < qa are tested
// first: the sum of squares implies both, and they keep each square below 2^62 (qa < 2^31) whatever the difference,
// which is below 2^32 in magnitude.
PB_FIXED_HD bool pbFpOverlaps(int qxNow, int qyNow, int qxThen, int qyThen, long long qa, unsigned long long a2) {
  const long long dx = (long long)qxNow - (long long)qxThen, dy = (long long)qyNow - (long long)qyThen;
  const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  if (ax >= qa || ay >= qa) return false;
  return (unsigned long long)(ax * ax) + (unsigned long long)(ay * ay) < a2;
}

// w += v on two little-endian limbs, v sign-extended to 128 bits
PB_FIXED_HD void pbFpAdd128(unsigned long long *w, long long v) {
  const unsigned long long lo = (unsigned long long)v, sign = (unsigned long long)(v >> 63);  // 0 or all ones
  const unsigned long long s0 = w[0] + lo;
  w[1] += sign + (s0 < lo ? 1ull : 0ull);
  w[0] = s0;
}

// What one origin adds to a (member, lag, vector) cell:  re += A,  im += B,  power += A^2 + B^2.
PB_FIXED_HD void pbFpMode(unsigned long long *cell, long long a, long long b) {
  pbFpAdd128(cell + PB_FP_RE, a);
  pbFpAdd128(cell + PB_FP_IM, b);
  pbCohAdd(cell + PB_FP_POWER, pbCohSum(pbCohMul(a, a), pbCohMul(b, b)));
}

// ... and to the (member, lag) cell:  samples += m,  overlap += Q,  overlap2 += Q^2  (Q < 2^28: the square is one word)
PB_FIXED_HD void pbFpCounts(unsigned long long *cell, unsigned long long m, unsigned long long q) {
  cell[PB_FP_SAMPLES] += m;
  cell[PB_FP_OVERLAP] += q;
  const unsigned long long q2 = q * q, s0 = cell[PB_FP_OVERLAP2] + q2;
  cell[PB_FP_OVERLAP2 + 1] += s0 < q2 ? 1ull : 0ull;
  cell[PB_FP_OVERLAP2] = s0;
}
