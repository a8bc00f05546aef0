// Stand-alone check of the arithmetic of the coherent intermediate scattering function (csrc/pb_coherent.hpp) against
// __int128 arithmetic on the CPU: the signed 64 x 64 -> 128-bit product, the 192-bit add with its carries and borrows
// through both limb boundaries in both signs, and what one origin adds to a cell.  Built plainly and with
// -fsanitize=address,undefined and run as a program by tests/test_coherent_ref.py.  The kernel and the host's row writer
// use the same functions.  No state of a few seconds' size reaches the third limb with a positive value, so this program
// is where that limb is held.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pb_coherent.hpp"

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

const long long MODE_TOP = (1ll << 58) - 1;  // |C|, |S| < 2^58

// a signed 192-bit value as a low unsigned 128 bits and a signed top limb: the independent restatement
struct Wide {
  u128 low = 0;
  long long top = 0;
  void add(i128 p) {
    const u128 before = low;
    low += (u128)p;
    const long long carry = low < before ? 1 : 0;
    top += (p < 0 ? -1 : 0) + carry;  // the sign extension of p, and the carry out of the low 128 bits
  }
};

bool same(const unsigned long long *w, const Wide &v) {
  return w[0] == (unsigned long long)v.low && w[1] == (unsigned long long)(v.low >> 64) && w[2] == (unsigned long long)v.top;
}

void checkMul(long long a, long long b) {
  const PbCohProduct p = pbCohMul(a, b);
  const i128 want = (i128)a * (i128)b;
  CHECK(p.lo == (unsigned long long)want);
  CHECK(p.hi == (long long)(want >> 64));
}

}  // namespace

int main() {
  CHECK(PB_COH_WORDS == 8 && PB_COH_MODE_WORDS == 2 && PB_COH_RE == 0 && PB_COH_IM == 3 && PB_COH_BOTS_NOW == 6 &&
        PB_COH_BOTS_THEN == 7);
  // the product: every pairing of values at and around the 32-bit pieces' edges, the modes' bound and the words' ends
  const long long edge[] = {0, 1, -1, 2, -2, 0xFFFFFFFFll, 0x100000000ll, -0xFFFFFFFFll, -0x100000000ll, 0x100000001ll,
                            1ll << 30, -(1ll << 30), MODE_TOP, -MODE_TOP, MODE_TOP - 1, 1ll << 58, -(1ll << 58),
                            0x7FFFFFFFFFFFFFFFll, -0x7FFFFFFFFFFFFFFFll - 1, 0x7FFFFFFF00000001ll, -0x7FFFFFFF00000001ll,
                            0x123456789ABCDEFll, -0x0FEDCBA987654321ll};
  for (long long a : edge)
    for (long long b : edge) checkMul(a, b);
  unsigned long long x = 0x9E3779B97F4A7C15ull;
  for (int k = 0; k < 200000; k++) {  // (a xorshift: any two words)
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    const long long a = (long long)x;
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    checkMul(a, (long long)x);
    checkMul(a >> 6, (long long)x >> 6);  // inside the modes' bound
  }
  {  // +-(2^58 - 1)^2, the largest products there are
    const i128 top2 = (i128)MODE_TOP * MODE_TOP;
    const PbCohProduct p = pbCohMul(MODE_TOP, MODE_TOP), q = pbCohMul(-MODE_TOP, MODE_TOP), r = pbCohMul(-MODE_TOP, -MODE_TOP);
    CHECK(p.lo == (unsigned long long)top2 && p.hi == (long long)(top2 >> 64) && p.hi > 0 && p.hi < (1ll << 52));
    CHECK(q.lo == (unsigned long long)-top2 && q.hi == (long long)((-top2) >> 64) && q.hi < 0);
    CHECK(r.lo == p.lo && r.hi == p.hi);
  }
  // the add: carries and borrows through both limb boundaries, in both signs
  {
    unsigned long long w[3] = {0, 0, 0};
    Wide v;
    const auto add = [&](i128 p) {
      pbCohAdd(w, PbCohProduct{(unsigned long long)p, (long long)(p >> 64)});
      v.add(p);
      CHECK(same(w, v));
    };
    add(-1);  // a small negative: all-ones upper limbs
    CHECK(w[0] == ~0ull && w[1] == ~0ull && w[2] == ~0ull);
    add(1);  // back through both boundaries
    CHECK(w[0] == 0 && w[1] == 0 && w[2] == 0);
    add((i128)~0ull);  // the first limb full
    add(1);            // a carry into the second
    CHECK(w[0] == 0 && w[1] == 1 && w[2] == 0);
    add(-1);  // a borrow out of it
    CHECK(w[0] == ~0ull && w[1] == 0 && w[2] == 0);
    add(-(i128)~0ull - 1);  // down through zero: -1
    CHECK(w[0] == ~0ull && w[1] == ~0ull && w[2] == ~0ull);
    add(1);
    // sums driven past 2^128: the largest increment, 2 (2^58 - 1)^2 < 2^117, 4200 times, then back down below -2^128
    const i128 step = (i128)2 * MODE_TOP * MODE_TOP;
    for (int k = 0; k < 4200; k++) add(step);
    CHECK(w[2] >= 1ull && (long long)w[2] > 0);  // the third limb holds a positive value
    const unsigned long long top = w[2];
    add(1), add(-1), add(-step), add(step);
    CHECK(w[2] == top);
    for (int k = 0; k < 8400; k++) add(-step);
    CHECK((long long)w[2] < -1);  // and a negative one, below -2^128
    for (int k = 0; k < 4200; k++) add(step);
    CHECK(w[0] == 0 && w[1] == 0 && w[2] == 0);
    // the low two limbs full, then one more: a carry that ripples through both boundaries at once
    add((i128)(((u128)1 << 127) - 1)), add((i128)(((u128)1 << 127) - 1)), add(1);
    CHECK(w[0] == ~0ull && w[1] == ~0ull && w[2] == 0);
    add(1);
    CHECK(w[0] == 0 && w[1] == 0 && w[2] == 1);
    add(-1);
    CHECK(w[0] == ~0ull && w[1] == ~0ull && w[2] == 0);
    // any sequence of products of modes
    for (int k = 0; k < 100000; k++) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      const long long a = (long long)x >> 6;
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      add((i128)a * (i128)((long long)x >> 6));
    }
  }
  // a cell: one origin after another against the definition, both counts, every sign pattern of the modes
  {
    unsigned long long cell[PB_COH_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    Wide re, im;
    unsigned long long botsNow = 0, botsThen = 0;
    const long long m[] = {MODE_TOP, -MODE_TOP, 0, 1, -1, 1ll << 30, -(1ll << 57), 0x2AAAAAAAAAAAAAAll};
    for (long long cn : m)
      for (long long sn : m)
        for (long long ct : m)
          for (long long st : m) {
            pbCohPair(cell, cn, sn, ct, st, 268435455ull, 3ull);
            re.add((i128)cn * ct), re.add((i128)sn * st);
            im.add((i128)sn * ct), im.add(-((i128)cn * st));
            botsNow += 268435455ull, botsThen += 3ull;
            CHECK(same(cell + PB_COH_RE, re) && same(cell + PB_COH_IM, im));
            CHECK(cell[PB_COH_BOTS_NOW] == botsNow && cell[PB_COH_BOTS_THEN] == botsThen);
          }
    // lag 0: a record with itself has no imaginary part
    unsigned long long self[PB_COH_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long c : m)
      for (long long s : m) pbCohPair(self, c, s, c, s, 1ull, 1ull);
    CHECK(self[PB_COH_IM] == 0 && self[PB_COH_IM + 1] == 0 && self[PB_COH_IM + 2] == 0);
    CHECK((long long)self[PB_COH_RE + 2] >= 0 && self[PB_COH_BOTS_NOW] == 64 && self[PB_COH_BOTS_THEN] == 64);
  }
  if (failures) return printf("pb_coherent_check: %d FAILED\n", failures), 1;
  printf("pb_coherent_check ok\n");
  return 0;
}
