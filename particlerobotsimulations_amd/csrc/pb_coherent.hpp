// pb_coherent.hpp -- the arithmetic of the coherent intermediate scattering function that has no device in it
// (pb_coherent.hip holds the kernels and the entry points; include/particlebot_hip.h has the definitions): the words of a
// mode and of a table cell, the signed 64 x 64 -> 128-bit product as (lo, hi), the 192-bit add with carry, and what one
// origin adds to a cell.  Compiles as plain C++ (tests/pb_coherent_check.cpp); the kernel, the host's row writer and the
// check program all use what is here, so there is one statement of each rule.
//
// All of it is integer arithmetic.  A mode is (C, S) = (sum C[idx], sum S[idx]) over the measured bots of a member, two
// signed 64-bit words with |C|, |S| <= measured 2^30 < 2^58.  A product of two such words is below 2^116 in magnitude, the
// sum or the difference of two products below 2^117, and a sum over fewer than 2^31 origins below 2^148: a signed 192-bit
// two's-complement word in three little-endian 64-bit limbs holds it with room to spare, whatever the state.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "pb_fixed.hpp"

// the words of a mode in the ring, and of a table cell: re and im as three limbs each, then the two summed counts
enum { PB_COH_C, PB_COH_S, PB_COH_MODE_WORDS };
enum { PB_COH_RE, PB_COH_IM = 3, PB_COH_BOTS_NOW = 6, PB_COH_BOTS_THEN, PB_COH_WORDS };
static_assert(PB_COH_MODE_WORDS == 2 && PB_COH_WORDS == 8, "16 bytes per mode; 6 words of sums and 2 of counts per cell");

// a signed 128-bit value, two's complement: hi * 2^64 + lo
struct PbCohProduct {
  unsigned long long lo;
  long long hi;
};

// a * b of any two signed 64-bit words.  The unsigned product's halves come from the four 32 x 32 -> 64-bit pieces; the
// signed high half is the unsigned one minus b where a is negative and minus a where b is (mod 2^64): a two's-complement
// word read as unsigned is 2^64 too large exactly when it is negative.
PB_FIXED_HD PbCohProduct pbCohMul(long long a, long long b) {
  const unsigned long long ua = (unsigned long long)a, ub = (unsigned long long)b;
  const unsigned long long a0 = (uint32_t)ua, a1 = ua >> 32, b0 = (uint32_t)ub, b1 = ub >> 32;
  const unsigned long long p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const unsigned long long mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;  // below 3 * 2^32
  unsigned long long hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);       // the unsigned high half: no wrap
  hi -= (a < 0 ? ub : 0ull) + (b < 0 ? ua : 0ull);
  return {ua * ub, (long long)hi};
}

// p + q of two products of modes: below 2^117 in magnitude, so the signed 128-bit sum does not wrap
PB_FIXED_HD PbCohProduct pbCohSum(PbCohProduct p, PbCohProduct q) {
  const unsigned long long lo = p.lo + q.lo;
  return {lo, (long long)((unsigned long long)p.hi + (unsigned long long)q.hi + (lo < q.lo ? 1ull : 0ull))};
}

// w += p on three little-endian limbs, p sign-extended to 192 bits; the carries ripple through both limb boundaries
PB_FIXED_HD void pbCohAdd(unsigned long long *w, PbCohProduct p) {
  const unsigned long long hi = (unsigned long long)p.hi, sign = (unsigned long long)(p.hi >> 63);  // 0 or all ones
  const unsigned long long s0 = w[0] + p.lo, c0 = s0 < p.lo ? 1ull : 0ull;
  const unsigned long long t1 = w[1] + hi, s1 = t1 + c0;
  const unsigned long long c1 = (t1 < hi ? 1ull : 0ull) + (s1 < t1 ? 1ull : 0ull);  // at most one of the two
  w[0] = s0, w[1] = s1, w[2] += sign + c1;
}

// What one origin adds to a cell: rho_now * conj(rho_then) with rho = C + i S, and the two measured counts.
//     re += C_now C_then + S_now S_then        im += S_now C_then - C_now S_then
// |C_now| < 2^58, so -C_now is a signed 64-bit word and the difference is the sum with the product of -C_now.
PB_FIXED_HD void pbCohPair(unsigned long long *cell, long long cNow, long long sNow, long long cThen, long long sThen,
                           unsigned long long botsNow, unsigned long long botsThen) {
  pbCohAdd(cell + PB_COH_RE, pbCohSum(pbCohMul(cNow, cThen), pbCohMul(sNow, sThen)));
  pbCohAdd(cell + PB_COH_IM, pbCohSum(pbCohMul(sNow, cThen), pbCohMul(-cNow, sThen)));
  cell[PB_COH_BOTS_NOW] += botsNow;
  cell[PB_COH_BOTS_THEN] += botsThen;
}
