// pb_bonds.hpp -- the arithmetic of the bond recorder that has no device in it (pb_bonds.hip holds the kernels and the
// entry points; include/particlebot_hip.h has the definitions): the presence rule, the network that sorts a bot's eight
// list entries, the intersection count of two lists, the cage vector with its range test, the overlap comparison, the
// split of the plain squares, and the words of a table cell.  Compiles as plain C++ (tests/pb_bonds_check.cpp); the
// kernels, the host's row writer and the check program all use what is here, so there is one statement of each rule.
//
// All of it is integer arithmetic behind the presence rule.  A quantised coordinate has |q| <= 2^31 - 128 (pb_fixed.hpp),
// so a difference dq of two of them has |dq| <= 2^32 - 256 < 2^32 and needs 64 bits; a bot has at most k <= 8 listed
// neighbours, so k dq and a sum of k differences are below 2^35 in magnitude and their difference below 2^36: the cage
// vector never wraps a long long.  It is accepted iff |cx|, |cy| < 2^31; then s = cx^2 + cy^2 < 2^63.
#pragma once

#include <stdint.h>

#include "pb_fixed.hpp"

constexpr uint32_t PB_BOND_NONE = 0xFFFFFFFFu;  // the padding of a list: no index (indices are below 2^28), sorts last
constexpr int PB_BOND_ABSENT = INT32_MIN;       // head.x of an absent bot (|q| <= 2^31 - 128: the value is free)

// a bot's list at a record: PB_BOND_WIDTH member-local original indices, ascending, padded with PB_BOND_NONE (two 16-byte
// words in memory); named members, so that a kernel holds it in registers and never indexes it
struct alignas(16) PbBondList {
  uint32_t e0, e1, e2, e3, e4, e5, e6, e7;
};
static_assert(sizeof(PbBondList) == sizeof(uint32_t) * PB_BOND_WIDTH, "a list is PB_BOND_WIDTH words");

// The words of a (member, lag) cell: eight counts, the two partial sums of the plain squares, and per k = 1 ... 8 the
// caged samples, those that overlap and the two partial sums of s (pbFixedLow / pbFixedRest).
enum {
  PB_BOND_SAMPLES, PB_BOND_CROWDED, PB_BOND_THEN, PB_BOND_NOW, PB_BOND_KEPT, PB_BOND_UNCHANGED, PB_BOND_LOST,
  PB_BOND_GAINED, PB_BOND_PLAIN_LO, PB_BOND_PLAIN_HI, PB_BOND_SCALARS,
  PB_BOND_CAGE_SAMPLES = PB_BOND_SCALARS, PB_BOND_CAGE_OVERLAP = PB_BOND_CAGE_SAMPLES + PB_BOND_WIDTH,
  PB_BOND_CAGE_LO = PB_BOND_CAGE_OVERLAP + PB_BOND_WIDTH, PB_BOND_CAGE_HI = PB_BOND_CAGE_LO + PB_BOND_WIDTH,
  PB_BOND_WORDS = PB_BOND_CAGE_HI + PB_BOND_WIDTH
};
static_assert(PB_BOND_WORDS == 42, "42 words per (member, lag): 336 bytes of LDS per workgroup");

// qa = rint(overlapRadius 2^20), formed once on the host in fp32 (the scaling is exact): at most 2^28 - 16 for a radius
// below 256, so that 8 qa < 2^31 and (k qa)^2 < 2^62
inline long long pbBondRadiusQuanta(float overlapRadius) { return (long long)__builtin_rintf(overlapRadius * 1048576.0f); }

// PRESENT: the position passes the scattering's rule on both axes and the radius is finite and <= maxRadius (a NaN fails
// every comparison)
PB_FIXED_HD bool pbBondPresent(float x, float y, float r, float maxRadius) {
  return pbFixedInRange(x) && pbFixedInRange(y) && __builtin_fabsf(r) < __builtin_inff() && r <= maxRadius;
}

PB_FIXED_HD void pbBondExchange(uint32_t &a, uint32_t &b) {
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo, b = hi;
}
// The eight entries ascending: a fixed network of 19 compare-exchanges in six layers (the padding is the largest
// unsigned value and sorts last by itself).
PB_FIXED_HD void pbBondSort(PbBondList &l) {
  pbBondExchange(l.e0, l.e2), pbBondExchange(l.e1, l.e3), pbBondExchange(l.e4, l.e6), pbBondExchange(l.e5, l.e7);
  pbBondExchange(l.e0, l.e4), pbBondExchange(l.e1, l.e5), pbBondExchange(l.e2, l.e6), pbBondExchange(l.e3, l.e7);
  pbBondExchange(l.e0, l.e1), pbBondExchange(l.e2, l.e3), pbBondExchange(l.e4, l.e5), pbBondExchange(l.e6, l.e7);
  pbBondExchange(l.e2, l.e4), pbBondExchange(l.e3, l.e5);
  pbBondExchange(l.e1, l.e4), pbBondExchange(l.e3, l.e6);
  pbBondExchange(l.e1, l.e2), pbBondExchange(l.e3, l.e4), pbBondExchange(l.e5, l.e6);
}

// 1 iff index j, which is not the padding, is an entry of b
PB_FIXED_HD uint32_t pbBondHas(const PbBondList &b, uint32_t j) {
  const bool hit = (j == b.e0) | (j == b.e1) | (j == b.e2) | (j == b.e3) | (j == b.e4) | (j == b.e5) | (j == b.e6) |
                   (j == b.e7);
  return hit && j != PB_BOND_NONE ? 1u : 0u;
}
// |a n b| of two lists whose entries other than the padding are distinct: 64 comparisons, no index
PB_FIXED_HD uint32_t pbBondKept(const PbBondList &a, const PbBondList &b) {
  return pbBondHas(b, a.e0) + pbBondHas(b, a.e1) + pbBondHas(b, a.e2) + pbBondHas(b, a.e3) + pbBondHas(b, a.e4) +
         pbBondHas(b, a.e5) + pbBondHas(b, a.e6) + pbBondHas(b, a.e7);
}

// THE CAGE VECTOR of a bot with k earlier neighbours: c = k dq_i - sum_j dq_j per axis, k times the cage-relative
// displacement in units of 2^-20.  True, with s = cx^2 + cy^2 < 2^63, iff |cx| < 2^31 and |cy| < 2^31.
PB_FIXED_HD bool pbBondCage(uint32_t k, long long dqx, long long dqy, long long sumX, long long sumY,
                            unsigned long long &s) {
  const long long cx = (long long)k * dqx - sumX, cy = (long long)k * dqy - sumY;  // below 2^36 in magnitude
  const long long ax = cx < 0 ? -cx : cx, ay = cy < 0 ? -cy : cy;
  s = 0ull;
  if (ax >= (1ll << 31) || ay >= (1ll << 31)) return false;
  s = (unsigned long long)(ax * ax) + (unsigned long long)(ay * ay);
  return true;
}

// THE OVERLAP of a caged bot: s < (k qa)^2, that is the cage-relative displacement is shorter than the radius; equality
// does not overlap and qa == 0 overlaps nothing.  k qa < 2^31.
PB_FIXED_HD bool pbBondOverlaps(unsigned long long s, uint32_t k, long long qa) {
  const unsigned long long kq = (unsigned long long)k * (unsigned long long)qa;
  return s < kq * kq;
}

// THE PLAIN SQUARES of a caged bot: dqx^2 and dqy^2 are below 2^64 each (|dq| < 2^32) and their sum may pass 2^64, so
// each is split on its own: lo gets the two low halves, below 2^33 together, hi the two high halves, below 2^33 too.
// Over fewer than 2^31 samples both words stay below 2^64 and lo + hi 2^32 (pbBondPlain) is the exact sum.
PB_FIXED_HD void pbBondPlainSplit(long long dqx, long long dqy, unsigned long long &lo, unsigned long long &hi) {
  const unsigned long long ax = (unsigned long long)(dqx < 0 ? -dqx : dqx), ay = (unsigned long long)(dqy < 0 ? -dqy : dqy);
  const unsigned long long x2 = ax * ax, y2 = ay * ay;
  lo = (x2 & 0xFFFFFFFFull) + (y2 & 0xFFFFFFFFull);
  hi = (x2 >> 32) + (y2 >> 32);
}
// what the two UNSIGNED words of the plain sum stand for (pbFixedCompose reads its rest as signed; this one may not)
inline __int128 pbBondPlain(unsigned long long lo, unsigned long long hi) {
  return (__int128)(((unsigned __int128)hi << 32) + (unsigned __int128)lo);
}
