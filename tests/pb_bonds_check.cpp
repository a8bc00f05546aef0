// Stand-alone check of the arithmetic of the bond recorder (csrc/pb_bonds.hpp) on the CPU against __int128 and
// brute-force sets: the sort network on all 8! orders of a list and with every amount of padding; the intersection count
// on every pair of subset sizes; the cage vector at |c| = 2^31 - 1 and 2^31 and at the largest differences there are;
// the overlap rule at k qa - 1, k qa and k qa + 1; the split of the plain squares at |dq| = 2^32 - 1 over 2^31 - 1
// samples; the presence rule.  Built plainly and with -fsanitize=address,undefined and run as a program by
// tests/test_bonds_ref.py.  The kernels and the host's row writer use the same functions.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <set>

#include "pb_bonds.hpp"

namespace {

typedef __int128 i128;
typedef unsigned __int128 u128;

int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      failures++;                                                \
    }                                                            \
  } while (0)

const long long Q_TOP = (1ll << 31) - 128;  // the largest quantised coordinate
const long long DQ_TOP = 2 * Q_TOP;         // the largest difference of two: 2^32 - 256

PbBondList listOf(const uint32_t *e) { return {e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7]}; }
void wordsOf(const PbBondList &l, uint32_t *e) {
  e[0] = l.e0, e[1] = l.e1, e[2] = l.e2, e[3] = l.e3, e[4] = l.e4, e[5] = l.e5, e[6] = l.e6, e[7] = l.e7;
}

void checkSort() {
  // all 8! orders of eight distinct indices, and of 8 - p indices with p paddings
  for (int pad = 0; pad <= 8; pad++) {
    uint32_t base[8];
    for (int k = 0; k < 8; k++) base[k] = k < 8 - pad ? 3u + 5u * (uint32_t)k : PB_BOND_NONE;
    uint32_t perm[8];
    std::copy(base, base + 8, perm);
    std::sort(perm, perm + 8);
    long orders = 0;
    do {
      PbBondList l = listOf(perm);
      pbBondSort(l);
      uint32_t got[8];
      wordsOf(l, got);
      bool same = true;
      for (int k = 0; k < 8; k++) same = same && got[k] == base[k];
      if (!same) {
        CHECK(same);
        return;
      }
      orders++;
    } while (std::next_permutation(perm, perm + 8));
    if (pad == 0) CHECK(orders == 40320);
  }
  // indices near the top of their range stay below the padding
  uint32_t top[8] = {PB_BOND_NONE, (1u << 28) - 1u, 0u, PB_BOND_NONE, 0xFFFFFFFEu, 7u, PB_BOND_NONE, 1u};
  PbBondList l = listOf(top);
  pbBondSort(l);
  CHECK(l.e0 == 0u && l.e1 == 1u && l.e2 == 7u && l.e3 == (1u << 28) - 1u && l.e4 == 0xFFFFFFFEu && l.e5 == PB_BOND_NONE &&
        l.e7 == PB_BOND_NONE);
}

void checkKept() {
  // every pair of subsets of a universe of ten indices with at most eight members each, by size: 1013^2 pairs
  long pairs = 0;
  bool seen[9][9] = {};
  for (uint32_t a = 0; a < 1024u; a++) {
    if (__builtin_popcount(a) > 8) continue;
    for (uint32_t b = 0; b < 1024u; b++) {
      if (__builtin_popcount(b) > 8) continue;
      uint32_t ea[8], eb[8];
      int na = 0, nb = 0;
      for (uint32_t k = 0; k < 10u; k++) {
        if (a >> k & 1u) ea[na++] = k * 1000003u;
        if (b >> k & 1u) eb[nb++] = k * 1000003u;
      }
      seen[na][nb] = true;
      for (int k = na; k < 8; k++) ea[k] = PB_BOND_NONE;
      for (int k = nb; k < 8; k++) eb[k] = PB_BOND_NONE;
      if (pbBondKept(listOf(ea), listOf(eb)) != (uint32_t)__builtin_popcount(a & b)) {
        CHECK(pbBondKept(listOf(ea), listOf(eb)) == (uint32_t)__builtin_popcount(a & b));
        return;
      }
      pairs++;
    }
  }
  CHECK(pairs == 1013l * 1013l);
  for (int x = 0; x <= 8; x++)
    for (int y = 0; y <= 8; y++) CHECK(seen[x][y]);
  // two empty lists share nothing: the padding is not an index
  const uint32_t none[8] = {PB_BOND_NONE, PB_BOND_NONE, PB_BOND_NONE, PB_BOND_NONE,
                            PB_BOND_NONE, PB_BOND_NONE, PB_BOND_NONE, PB_BOND_NONE};
  CHECK(pbBondKept(listOf(none), listOf(none)) == 0u);
}

// the cage vector on 128-bit integers: nothing can wrap
void checkCageOne(uint32_t k, long long dqx, long long dqy, long long sumX, long long sumY) {
  const i128 cx = (i128)k * dqx - sumX, cy = (i128)k * dqy - sumY;
  const i128 top = (i128)1 << 31;
  const bool want = cx > -top && cx < top && cy > -top && cy < top;
  unsigned long long s = 77ull;
  const bool got = pbBondCage(k, dqx, dqy, sumX, sumY, s);
  CHECK(got == want);
  if (want) CHECK((i128)s == cx * cx + cy * cy && s < (1ull << 63));
  else CHECK(s == 0ull);
}

void checkCage() {
  const long long edge = (1ll << 31);
  for (uint32_t k = 1; k <= 8; k++) {
    for (long long c : {edge - 1, edge, edge + 1, -(edge - 1), -edge, -(edge + 1), 0ll, 1ll, -1ll}) {
      // c = k dq - sum with dq at several places, the largest included
      for (long long dq : {0ll, 1ll, -1ll, DQ_TOP, -DQ_TOP, 12345678ll}) {
        checkCageOne(k, dq, 0, (long long)k * dq - c, 0);
        checkCageOne(k, 0, dq, 0, (long long)k * dq - c);
        checkCageOne(k, dq, dq, (long long)k * dq - c, (long long)k * dq - (edge - 1));
        checkCageOne(k, dq, dq, (long long)k * dq - (edge - 1), (long long)k * dq - c);
      }
    }
    // the largest magnitudes there are: the bot at one end of the range, its k neighbours at the other
    checkCageOne(k, DQ_TOP, -DQ_TOP, -(long long)k * DQ_TOP, (long long)k * DQ_TOP);
    checkCageOne(k, -DQ_TOP, DQ_TOP, (long long)k * DQ_TOP, -(long long)k * DQ_TOP);
  }
  unsigned long long s;
  CHECK(pbBondCage(8, 0, 0, edge - 1, edge - 1, s) && s == 2ull * (unsigned long long)((edge - 1) * (edge - 1)));
  CHECK(!pbBondCage(8, 300ll << 20, 0, 0, 0, s));  // 8 x 300 world units is past 2^31 quanta
  CHECK(pbBondCage(1, 0, 0, 300ll << 20, 0, s) && s == (unsigned long long)(300ll << 20) * (unsigned long long)(300ll << 20));
}

void checkOverlap() {
  const long long qaTop = pbBondRadiusQuanta(std::nextafterf(256.0f, 0.0f));
  CHECK(qaTop == (1ll << 28) - 16 && 8 * qaTop < (1ll << 31));
  CHECK(pbBondRadiusQuanta(0.0f) == 0 && pbBondRadiusQuanta(0.0078125f) == 8192 && pbBondRadiusQuanta(1.5e-6f) == 2);
  for (uint32_t k = 1; k <= 8; k++) {
    for (long long qa : {1ll, 2ll, 8192ll, 1048576ll, qaTop}) {
      const u128 edge = (u128)k * (u128)qa;
      for (long long off : {-1ll, 0ll, 1ll}) {
        const long long c = (long long)edge + off;  // s = c^2 + 0: at k qa - 1, k qa and k qa + 1
        const unsigned long long s = (unsigned long long)c * (unsigned long long)c;
        CHECK(pbBondOverlaps(s, k, qa) == ((u128)s < edge * edge));
        CHECK(pbBondOverlaps(s, k, qa) == (off < 0));
      }
      CHECK(pbBondOverlaps(edge * edge - 1ull, k, qa) && !pbBondOverlaps((unsigned long long)(edge * edge), k, qa));
      CHECK(pbBondOverlaps(0ull, k, qa));
    }
    CHECK(!pbBondOverlaps(0ull, k, 0));  // a radius of 0 overlaps nothing, a bot that has not moved included
    CHECK(!pbBondOverlaps((1ull << 63) - 1ull, k, 0));
  }
}

void checkPlain() {
  // one sample at the largest differences
  for (long long dx : {0ll, 1ll, -1ll, 65536ll, (1ll << 32) - 1, -((1ll << 32) - 1), DQ_TOP, -DQ_TOP}) {
    for (long long dy : {0ll, -3ll, (1ll << 32) - 1, -((1ll << 32) - 1), DQ_TOP}) {
      unsigned long long lo, hi;
      pbBondPlainSplit(dx, dy, lo, hi);
      CHECK(lo < (1ull << 33) && hi < (1ull << 33));
      CHECK(pbBondPlain(lo, hi) == (i128)dx * dx + (i128)dy * dy);
    }
  }
  // 2^31 - 1 samples of the largest square there could be: neither word wraps, and the composed sum is exact
  unsigned long long lo, hi;
  pbBondPlainSplit((1ll << 32) - 1, -((1ll << 32) - 1), lo, hi);
  const u128 count = ((u128)1 << 31) - 1;
  const u128 sumLo = (u128)lo * count, sumHi = (u128)hi * count;
  CHECK(sumLo < ((u128)1 << 64) && sumHi < ((u128)1 << 64));
  const i128 each = (i128)((1ll << 32) - 1) * ((1ll << 32) - 1) * 2;
  CHECK(pbBondPlain((unsigned long long)sumLo, (unsigned long long)sumHi) == each * (i128)count);
  CHECK(pbBondPlain((unsigned long long)sumLo, (unsigned long long)sumHi) < ((i128)1 << 96));
  // the way back to a pbMoment128 keeps the value: hi 2^32 + lo with 0 <= lo < 2^32
  const i128 v = pbBondPlain(0xFFFFFFFFFFFFFFFFull, 1ull << 40);
  const pbMoment128 m = pbFixedNormalised(v);
  CHECK(m.lo < (1ull << 32) && ((i128)m.hi << 32) + (i128)m.lo == v);
  // a cage sum, signed rest included: the time correlation's split and its way back
  unsigned long long a = 0ull, b = 0ull;
  const unsigned long long s = (1ull << 63) - 5ull;
  for (int n = 0; n < 1000; n++) pbFixedSplitAdd(s, a, b);
  CHECK(pbFixedCompose(a, b) == (i128)s * 1000);
}

void checkPresent() {
  const float inf = __builtin_inff(), nan = __builtin_nanf("");
  const float below = std::nextafterf(2048.0f, 0.0f), above = std::nextafterf(0.3f, 1.0f);
  CHECK(pbBondPresent(0.0f, 0.0f, 0.3f, 0.3f) && pbBondPresent(below, -below, 0.3f, 0.3f));
  CHECK(!pbBondPresent(2048.0f, 0.0f, 0.1f, 0.3f) && !pbBondPresent(0.0f, -2048.0f, 0.1f, 0.3f));
  CHECK(!pbBondPresent(nan, 0.0f, 0.1f, 0.3f) && !pbBondPresent(0.0f, inf, 0.1f, 0.3f) && !pbBondPresent(-inf, 0.0f, 0.1f, 0.3f));
  CHECK(!pbBondPresent(0.0f, 0.0f, above, 0.3f) && !pbBondPresent(0.0f, 0.0f, nan, 0.3f));
  CHECK(!pbBondPresent(0.0f, 0.0f, inf, 0.3f) && !pbBondPresent(0.0f, 0.0f, -inf, 0.3f));
  CHECK(pbBondPresent(0.0f, 0.0f, 0.0f, 0.3f) && pbBondPresent(0.0f, 0.0f, -1.0f, 0.3f));  // finite and <= maxRadius
  CHECK(pbFixedQuantise(below) == Q_TOP && pbFixedQuantise(-below) == -Q_TOP);
}

}  // namespace

int main() {
  checkSort();
  checkKept();
  checkCage();
  checkOverlap();
  checkPlain();
  checkPresent();
  if (failures) {
    printf("pb_bonds_check: %d FAILED\n", failures);
    return 1;
  }
  printf("pb_bonds_check ok\n");
  return 0;
}
