// pb_vanhove.hpp -- the arithmetic of the self van Hove function that has no device in it (pb_vanhove.hip holds the
// kernels and the entry points; include/particlebot_hip.h has the definitions): the words of a table cell, the table of
// radial edges, the two bin rules and the 192-bit sum of fourth powers, and behind them the cell and the radial rules of
// the distinct part (pb_vanhove_distinct.hip).  Compiles as plain C++ (tests/pb_vanhove_check.cpp,
// tests/pb_vanhove_distinct_check.cpp); the kernel and the host's row writer both use what is here, so there is one statement of
// each rule.
//
// All of it is integer arithmetic on pb_fixed.hpp's quantities: |qx|, |qy| <= 2^31 - 128, s = qx^2 + qy^2 < 2^63, the bin
// width qw = pbFixedQuantise(binWidth) in 1 ... 2^31 - 128 and bins in 1 ... PB_VANHOVE_MAX_BINS.  The self part guesses
// nowhere in floating point: the radial bin is a binary search in the exact edges and the axis bin an integer division.
// The distinct part's two further radial rules (at the end) start from a floating-point guess and end in exact integer
// comparisons that hold whatever the guess was, so there is no correction step whose reach would have to be proven.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "pb_fixed.hpp"

// the words of a table cell: ten moments, then bins radial counters, 2 bins of x and 2 bins of y
enum {
  PB_VH_SAMPLES, PB_VH_BEYOND_R, PB_VH_BEYOND_X, PB_VH_BEYOND_Y, PB_VH_MSD_LO, PB_VH_MSD_HI,
  PB_VH_Q4_0, PB_VH_Q4_1, PB_VH_Q4_2, PB_VH_Q4_3, PB_VH_MOMENTS
};
static_assert(PB_VH_MOMENTS == 10, "ten accumulators per lane and ten words in front of a cell's histograms");
constexpr uint32_t PB_VH_HIST_PER_BIN = 5u;  // counters per bin: one radial, two of x, two of y
PB_FIXED_HD uint32_t pbVhRadialAt(uint32_t) { return 0u; }                   // where each histogram starts, in counters
PB_FIXED_HD uint32_t pbVhXAt(uint32_t bins) { return bins; }
PB_FIXED_HD uint32_t pbVhYAt(uint32_t bins) { return 3u * bins; }
PB_FIXED_HD size_t pbVhCellWords(uint32_t bins) { return (size_t)PB_VH_MOMENTS + (size_t)PB_VH_HIST_PER_BIN * bins; }

constexpr unsigned long long PB_VH_EDGE_CAP = 1ull << 63;  // every s is below it

// E_k = min((k qw)^2, 2^63) for k = 0 ... bins, bins + 1 entries: k qw < 2^41, so the square needs 128 bits
inline void pbVhEdges(uint32_t qw, uint32_t bins, unsigned long long *edges) {
  for (uint32_t k = 0; k <= bins; k++) {
    const unsigned __int128 e = (unsigned __int128)k * qw, e2 = e * e;
    edges[k] = e2 < (unsigned __int128)PB_VH_EDGE_CAP ? (unsigned long long)e2 : PB_VH_EDGE_CAP;
  }
}

// The radial rule: max{k : E_k <= s} of an s < 2^63, where edgeAt(k) gives E_k for k = 1 ... bins (E_0 = 0 <= s is never
// read).  The result is in 0 ... bins, and bins itself says "beyond": s >= E_bins.  The edges do not decrease, a
// saturated edge is above every s, so the prefix {k : E_k <= s} is found by a binary search whose trip count depends on
// bins alone: the highest power of two not above bins, halved down to 1 (at most 11 trips, the same in every lane).
template <typename EdgeAt>
PB_FIXED_HD uint32_t pbVhRadialBin(const EdgeAt &edgeAt, uint32_t bins, unsigned long long s) {
  uint32_t step = 1u;
  while (step <= bins >> 1) step <<= 1;
  uint32_t k = 0u;
  for (; step; step >>= 1) {
    const uint32_t c = k + step;
    if (c <= bins && edgeAt(c) <= s) k = c;
  }
  return k;
}

// The axis rule: floor(q / qw) towards minus infinity of |q| <= 2^31 - 128 and 1 <= qw: one unsigned 32-bit division.
// For q < 0, floor(q / qw) = -((-q - 1) / qw) - 1 with -q - 1 >= 0; the magnitude of the result is at most 2^31 - 128.
PB_FIXED_HD int pbVhAxisFloor(int q, uint32_t qw) {
  return q >= 0 ? (int)((uint32_t)q / qw) : -(int)(((uint32_t)(-q) - 1u) / qw) - 1;
}
// ... and its counter: index b + bins of the axis' 2 bins counters iff -bins <= b < bins; else 2 bins, which says "beyond"
PB_FIXED_HD uint32_t pbVhAxisIndex(int q, uint32_t qw, uint32_t bins) {
  const uint32_t at = (uint32_t)pbVhAxisFloor(q, qw) + bins;  // (mod 2^32: a b below -bins becomes a huge index)
  return at < 2u * bins ? at : 2u * bins;
}

// s^2 < 2^126 given as the two halves of the 128-bit product, added as its four 32-bit pieces: each accumulator gains less
// than 2^32 per sample, so with fewer than 2^31 samples none reaches 2^63
PB_FIXED_HD void pbVhQ4Add(unsigned long long lo, unsigned long long hi, unsigned long long &a0, unsigned long long &a1,
                           unsigned long long &a2, unsigned long long &a3) {
  a0 += (unsigned long long)(uint32_t)lo, a1 += lo >> 32;
  a2 += (unsigned long long)(uint32_t)hi, a3 += hi >> 32;
}
// a0 + a1 2^32 + a2 2^64 + a3 2^96 of four accumulators below 2^63 each, as three little-endian 64-bit limbs (the sum is
// below 2^160)
inline void pbVhQ4Compose(unsigned long long a0, unsigned long long a1, unsigned long long a2, unsigned long long a3,
                          unsigned long long (&limbs)[3]) {
  const unsigned __int128 low = (unsigned __int128)a0 + ((unsigned __int128)a1 << 32);                   // below 2^96
  const unsigned __int128 high = (low >> 64) + (unsigned __int128)a2 + ((unsigned __int128)a3 << 32);  // below 2^96
  limbs[0] = (unsigned long long)low, limbs[1] = (unsigned long long)high, limbs[2] = (unsigned long long)(high >> 64);
}

// ---- the distinct part (pb_vanhove_distinct.hip) -------------------------------------------------------------------------
// The words of a table cell: the bots present at the earlier record, the bots present at the later one, both summed over
// the origins, then bins radial counters of ordered pairs.
enum { PB_VHD_CENTRES, PB_VHD_PARTNERS, PB_VHD_HEAD };
PB_FIXED_HD size_t pbVhdCellWords(uint32_t bins) { return (size_t)PB_VHD_HEAD + bins; }

// The distinct part asks qw bins < 2^31 on top of the self part's bounds: rMax = bins binWidth < 2048, no edge
// saturates, E_bins = (qw bins)^2 < 2^62, and a pair is counted iff s < E_bins.  For such an s there are two more ways
// to the radial bin max{k : (k qw)^2 <= s}; both end in exact integer comparisons, so neither needs a proof of how good
// its first guess is: the guess only decides how many comparisons are made.
//
// (b) from a guess (the kernel's is (uint32_t)(sqrtf(d2) / binWidth) in fp32): clamped into 0 ... bins - 1, then moved
// down while E_g > s and up while E_(g + 1) <= s.  E_0 = 0 <= s ends the first loop and E_bins > s the second, and
// between them E_g <= s < E_(g + 1) holds: that is the rule.  edgeAt(k) gives E_k for k = 1 ... bins, as above.
template <typename EdgeAt>
PB_FIXED_HD uint32_t pbVhRadialBinFrom(const EdgeAt &edgeAt, uint32_t bins, unsigned long long s, uint32_t guess) {
  uint32_t g = guess < bins ? guess : bins - 1u;
  while (g > 0u && edgeAt(g) > s) g--;
  while (g + 1u < bins && edgeAt(g + 1u) <= s) g++;  // (E_bins > s is the caller's: the edge is not read)
  return g;
}

// (c) by the integer square root: k qw <= sqrt(s) iff k qw <= floor(sqrt(s)) for integers, so the bin is
// floor(sqrt(s)) / qw, one 32-bit division.  The root of s < 2^62 starts from the fp64 root (within one of the truth:
// the conversion and the root each err by 2^-53 relative, the root is below 2^31) and is corrected by comparing squares,
// which do not overflow: (r + 1)^2 <= 2^62.
PB_FIXED_HD uint32_t pbVhIsqrt(unsigned long long s) {
  unsigned long long r = (unsigned long long)__builtin_sqrt((double)s);
  while (r * r > s) r--;
  while ((r + 1ull) * (r + 1ull) <= s) r++;
  return (uint32_t)r;
}
PB_FIXED_HD uint32_t pbVhRadialBinRoot(uint32_t qw, unsigned long long s) { return pbVhIsqrt(s) / qw; }
