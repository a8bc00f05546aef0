// Stand-alone check of the arithmetic of the four-point recorder (csrc/pb_fourpoint.hpp) on the CPU: the overlap rule at
// and around the radius, at differences near 2^32 and at a radius of 0; the signed 128-bit add on two limbs; and what one
// origin adds to a cell against __int128 arithmetic, through negative sums and the third limb of power.  Built plainly
// and with -fsanitize=address,undefined and run as a program by tests/test_fourpoint_ref.py.  The kernels and the host's
// row writer use the same functions.  No state of a few seconds' size reaches the third limb, so this program is where
// that limb is held.
#include <climits>
#include <cstdint>
#include <cstdio>

#include "pb_fourpoint.hpp"

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

const long long MODE_TOP = (1ll << 58) - 1;  // |A|, |B| < 2^58
const int Q_TOP = INT_MAX - 127;             // the largest quantised position: 2^31 - 128

// the rule as the header states it, on 128-bit integers: nothing can wrap
bool plain(int xn, int yn, int xt, int yt, long long qa) {
  const i128 dx = (i128)xn - xt, dy = (i128)yn - yt;
  return dx * dx + dy * dy < (i128)qa * qa;
}

void checkOverlap(int xn, int yn, int xt, int yt, long long qa) {
  CHECK(pbFpOverlaps(xn, yn, xt, yt, qa, (unsigned long long)(qa * qa)) == plain(xn, yn, xt, yt, qa));
}

bool same128(const unsigned long long *w, i128 v) {
  return w[0] == (unsigned long long)v && w[1] == (unsigned long long)(v >> 64);
}

// a 192-bit value as a low unsigned 128 bits and a top limb: the independent restatement
struct Wide {
  u128 low = 0;
  unsigned long long top = 0;
  void add(u128 p) {
    const u128 before = low;
    low += p;
    top += low < before ? 1 : 0;
  }
};

bool same192(const unsigned long long *w, const Wide &v) {
  return w[0] == (unsigned long long)v.low && w[1] == (unsigned long long)(v.low >> 64) && w[2] == v.top;
}

}  // namespace

int main() {
  CHECK(PB_FP_WORDS == 8 && PB_FP_LAG_WORDS == 4 && PB_FP_RE == 0 && PB_FP_IM == 2 && PB_FP_POWER == 4 &&
        PB_FP_SAMPLES == 0 && PB_FP_OVERLAP == 1 && PB_FP_OVERLAP2 == 2 && PB_FP_MODE_WORDS == 2);
  // the radius: rint in fp32, ties to even, below 2^31
  CHECK(pbFpRadiusQuanta(0.0f) == 0 && pbFpRadiusQuanta(0.25f) == 262144 && pbFpRadiusQuanta(1.0f) == 1048576);
  CHECK(pbFpRadiusQuanta(1.5f / 1048576.0f) == 2 && pbFpRadiusQuanta(2.5f / 1048576.0f) == 2);
  CHECK(pbFpRadiusQuanta(__builtin_nextafterf(2048.0f, 0.0f)) == (1ll << 31) - 128);
  // the overlap at qa - 1, qa, qa + 1 along an axis and on the diagonal, both signs, for small and the largest radii
  const long long radii[] = {1, 2, 5, 262144, 1048576, (1ll << 31) - 128};
  for (long long qa : radii) {
    for (long long d = qa - 1; d <= qa + 1; d++) {
      const int e = (int)d;  // qa + 1 <= 2^31 - 127
      CHECK(pbFpOverlaps(e, 0, 0, 0, qa, (unsigned long long)(qa * qa)) == (d < qa));
      CHECK(pbFpOverlaps(0, 0, 0, e, qa, (unsigned long long)(qa * qa)) == (d < qa));
      CHECK(pbFpOverlaps(0, -e, 0, 0, qa, (unsigned long long)(qa * qa)) == (d < qa));
      checkOverlap(e, 1, 0, 0, qa), checkOverlap(e, (int)(qa - 1), 0, 0, qa), checkOverlap(-e, 7, 3, -2, qa);
    }
    CHECK(pbFpOverlaps(5, 5, 5, 5, qa, (unsigned long long)(qa * qa)));  // no displacement overlaps for qa >= 1
  }
  // exact ties s == a2 do not overlap: the Pythagorean triples scaled to the grid of 2^-6 (16384 quanta)
  CHECK(!pbFpOverlaps(3, 4, 0, 0, 5, 25) && pbFpOverlaps(3, 3, 0, 0, 5, 25) && !pbFpOverlaps(0, 5, 0, 0, 5, 25));
  {
    const long long qa = 5 * 16384 * 4;  // a radius of 0.3125
    CHECK(!pbFpOverlaps(3 * 65536, -4 * 65536, 0, 0, qa, (unsigned long long)(qa * qa)));
    CHECK(pbFpOverlaps(3 * 65536 - 1, -4 * 65536, 0, 0, qa, (unsigned long long)(qa * qa)));
  }
  // a radius of 0 overlaps nothing, not even a bot that stayed
  CHECK(!pbFpOverlaps(0, 0, 0, 0, 0, 0) && !pbFpOverlaps(7, -7, 7, -7, 0, 0) && !pbFpOverlaps(1, 0, 0, 0, 0, 0));
  // differences near 2^32: the near test keeps every square from wrapping, whatever the radius
  for (long long qa : radii)
    for (int a : {Q_TOP, Q_TOP - 1, -Q_TOP, -Q_TOP + 1, 0, 1})
      for (int b : {Q_TOP, -Q_TOP, -Q_TOP + 1, 0, -1}) {
        checkOverlap(a, b, b, a, qa), checkOverlap(a, 0, b, 0, qa), checkOverlap(0, a, 0, b, qa);
        checkOverlap(a, a, b, b, qa);
      }
  CHECK(!pbFpOverlaps(Q_TOP, 0, -Q_TOP, 0, (1ll << 31) - 128, (unsigned long long)(((1ll << 31) - 128) * ((1ll << 31) - 128))));
  unsigned long long x = 0x9E3779B97F4A7C15ull;
  const auto next = [&] {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return x;
  };
  for (int k = 0; k < 200000; k++) {  // any positions in range, radii of every size
    const long long qa = (long long)(next() >> (33 + (k % 31)));
    const unsigned long long span = 2ull * (Q_TOP - 2000) + 1ull;  // (room for the small offsets below)
    const int xn = (int)((long long)(next() % span) - (Q_TOP - 2000)), xt = (int)((long long)(next() % span) - (Q_TOP - 2000));
    const int yn = (int)((long long)(next() % span) - (Q_TOP - 2000));
    const int near1 = (int)((long long)(next() % 2001ull) - 1000), near2 = (int)((long long)(next() % 2001ull) - 1000);
    checkOverlap(xn, yn, xt, yn + near1, qa);
    checkOverlap(xn, yn, xn + near1, yn + near2, qa & 2047);  // a close pair against a small radius
  }
  // the 128-bit add: carries and borrows through the limb boundary, in both signs
  {
    unsigned long long w[2] = {0, 0};
    i128 v = 0;
    const auto add = [&](long long p) {
      pbFpAdd128(w, p);
      v += p;
      CHECK(same128(w, v));
    };
    add(-1);
    CHECK(w[0] == ~0ull && w[1] == ~0ull);
    add(1);
    CHECK(w[0] == 0 && w[1] == 0);
    add(LLONG_MAX), add(LLONG_MAX), add(2);  // a carry into the second limb
    CHECK(w[0] == 0 && w[1] == 1);
    add(-1);  // a borrow out of it
    CHECK(w[0] == ~0ull && w[1] == 0);
    add(LLONG_MIN), add(LLONG_MIN), add(-1);  // down through zero
    CHECK(w[0] == ~1ull && w[1] == ~0ull);
    for (int k = 0; k < 5000; k++) add(MODE_TOP);  // past 2^64 upwards ...
    CHECK((long long)w[1] > 0);
    for (int k = 0; k < 10000; k++) add(-MODE_TOP);  // ... and below -2^64
    CHECK((long long)w[1] < -1);
    for (int k = 0; k < 100000; k++) add((long long)next() >> 6);  // any sequence of modes
  }
  // a cell: one origin after another against the definition, every sign pattern of the mode, the third limb of power
  {
    unsigned long long cell[PB_FP_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    i128 re = 0, im = 0;
    Wide power;
    const long long m[] = {MODE_TOP, -MODE_TOP, 0, 1, -1, 1ll << 30, -(1ll << 57), 0x2AAAAAAAAAAAAAAll};
    for (int round = 0; round < 400; round++)
      for (long long a : m)
        for (long long b : m) {
          pbFpMode(cell, a, b);
          re += a, im += b;
          power.add((u128)((i128)a * a)), power.add((u128)((i128)b * b));
          CHECK(same128(cell + PB_FP_RE, re) && same128(cell + PB_FP_IM, im) && same192(cell + PB_FP_POWER, power));
          CHECK(cell[PB_FP_SPARE] == 0);
        }
    CHECK(cell[PB_FP_POWER + 2] >= 1ull);  // 400 rounds of 32 squares of 2^116: past 2^128
    for (int k = 0; k < 100000; k++) {
      const long long a = (long long)next() >> 6, b = (long long)next() >> 6;
      pbFpMode(cell, a, b);
      re += a, im += b;
      power.add((u128)((i128)a * a)), power.add((u128)((i128)b * b));
    }
    CHECK(same128(cell + PB_FP_RE, re) && same128(cell + PB_FP_IM, im) && same192(cell + PB_FP_POWER, power));
    // negative sums: the upper limb of re is all ones
    unsigned long long neg[PB_FP_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    pbFpMode(neg, -3, 0), pbFpMode(neg, -MODE_TOP, 5);
    CHECK(neg[PB_FP_RE + 1] == ~0ull && neg[PB_FP_RE] == (unsigned long long)(-3 - MODE_TOP) && neg[PB_FP_IM] == 5 &&
          neg[PB_FP_IM + 1] == 0);
  }
  // the (member, lag) words: the largest counts, 2^31 - 1 origins' worth through the second limb of overlap2
  {
    unsigned long long cell[PB_FP_LAG_WORDS] = {0, 0, 0, 0};
    const unsigned long long top = (1ull << 28) - 1;
    u128 q2 = 0;
    unsigned long long samples = 0, overlap = 0;
    for (int k = 0; k < 3000; k++) {
      const unsigned long long q = k % 3 ? top : next() % (top + 1);
      pbFpCounts(cell, top, q);
      samples += top, overlap += q, q2 += (u128)q * q;
      CHECK(cell[PB_FP_SAMPLES] == samples && cell[PB_FP_OVERLAP] == overlap);
      CHECK(cell[PB_FP_OVERLAP2] == (unsigned long long)q2 && cell[PB_FP_OVERLAP2 + 1] == (unsigned long long)(q2 >> 64));
    }
    CHECK(cell[PB_FP_OVERLAP2 + 1] >= 1ull);  // 2000 x (2^28 - 1)^2 > 2^64
  }
  if (failures) return printf("pb_fourpoint_check: %d FAILED\n", failures), 1;
  printf("pb_fourpoint_check ok\n");
  return 0;
}
