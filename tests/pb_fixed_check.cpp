// Stand-alone check of the host-callable part of the fixed-point kit (csrc/pb_fixed.hpp) against plain __int128
// arithmetic on the CPU: the quantiser and its range, the split of a 64-bit value into two accumulators, the composer
// and the normaliser.  Built plainly and with -fsanitize=address,undefined and run as a program by
// tests/test_fixed_point.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "pb_fixed.hpp"

namespace {

int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      failures++;                                                \
    }                                                            \
  } while (0)

// xorshift64*: the same values on every run
uint64_t rngState = 0x9E3779B97F4A7C15ull;
uint64_t nextRandom() {
  rngState ^= rngState >> 12, rngState ^= rngState << 25, rngState ^= rngState >> 27;
  return rngState * 0x2545F4914F6CDD1Dull;
}

// p through the split into two fresh accumulators and back
__int128 roundTrip(long long p) {
  unsigned long long lo = 0, hi = 0;
  pbFixedSplitAdd(p, lo, hi);
  return pbFixedCompose(lo, hi);
}

void checkNormalised(__int128 v) {
  const pbMoment128 m = pbFixedNormalised(v);
  CHECK(m.lo < (1ull << 32));
  CHECK((__int128)m.hi * ((__int128)1 << 32) + (__int128)m.lo == v);  // with 0 <= lo < 2^32, hi is the floor quotient
}

}  // namespace

int main() {
  const float step = 1.0f / PB_FIXED_SCALE;  // 2^-20
  const float inf = std::numeric_limits<float>::infinity();
  const float below = std::nextafterf(PB_FIXED_LIMIT, 0.0f);  // the largest measured magnitude
  CHECK(PB_FIXED_SCALE == 1048576.0f && PB_FIXED_LIMIT == 2048.0f);

  // the quantiser: zeros, ties to even, the ends of the range
  CHECK(pbFixedQuantise(0.0f) == 0 && pbFixedQuantise(-0.0f) == 0);
  CHECK(pbFixedQuantise(0.5f * step) == 0 && pbFixedQuantise(1.5f * step) == 2 && pbFixedQuantise(2.5f * step) == 2);
  CHECK(pbFixedQuantise(-0.5f * step) == 0 && pbFixedQuantise(-1.5f * step) == -2);
  CHECK(pbFixedQuantise(-2.5f * step) == -2);
  CHECK(pbFixedQuantise(1.0f) == 1048576 && pbFixedQuantise(-3.0f * step) == -3);
  CHECK(pbFixedQuantise(below) == 2147483648ll - 128 && pbFixedQuantise(-below) == -(2147483648ll - 128));

  // the range: open at 2048, closed to everything that is no number
  CHECK(pbFixedInRange(0.0f) && pbFixedInRange(-0.0f) && pbFixedInRange(below) && pbFixedInRange(-below));
  CHECK(!pbFixedInRange(2048.0f) && !pbFixedInRange(-2048.0f) && !pbFixedInRange(inf) && !pbFixedInRange(-inf));
  CHECK(!pbFixedInRange(std::numeric_limits<float>::quiet_NaN()));

  // split-add, then compose: p again
  const long long two32 = 1ll << 32, two62 = 1ll << 62, max63 = std::numeric_limits<long long>::max();
  const long long fixedCases[] = {0, 1, -1, two32 - 1, two32, -two32, two62, -two62, max63, -max63};
  for (const long long p : fixedCases) {
    CHECK(roundTrip(p) == (__int128)p);
    const long long rest = (long long)pbFixedRest(p);
    CHECK(pbFixedLow(p) < (1ull << 32) && rest >= -(1ll << 31) && rest < (1ll << 31));
  }
  for (int k = 0; k < 4096; k++) {
    const long long p = (long long)nextRandom();
    CHECK(roundTrip(p) == (__int128)p);
    if (p >= 0) {  // an unsigned value below 2^63 splits the same way
      unsigned long long lo = 0, hi = 0, lo2 = 0, hi2 = 0;
      pbFixedSplitAdd((unsigned long long)p, lo, hi), pbFixedSplitAdd(p, lo2, hi2);
      CHECK(lo == lo2 && hi == hi2);
    }
  }

  // 2^16 splits into one pair of accumulators: the __int128 sum, whatever the signs
  {
    unsigned long long lo = 0, hi = 0;
    __int128 sum = 0;
    for (int k = 0; k < (1 << 16); k++) {
      const long long p = k < 8 ? (k & 1 ? -max63 : max63) : (long long)nextRandom();
      pbFixedSplitAdd(p, lo, hi);
      sum += p;
    }
    CHECK(pbFixedCompose(lo, hi) == sum);
    checkNormalised(sum);
  }
  {  // all at the negative end: the sum is far below -2^64, the high accumulator has wrapped as a signed sum does
    unsigned long long lo = 0, hi = 0;
    for (int k = 0; k < (1 << 16); k++) pbFixedSplitAdd(-max63, lo, hi);
    CHECK(pbFixedCompose(lo, hi) == (__int128)(-max63) * (1 << 16));
  }

  // the normaliser: 0 <= lo < 2^32 and hi the floor quotient, for negative values too
  const pbMoment128 minusOne = pbFixedNormalised(-1);
  CHECK(minusOne.lo == (1ull << 32) - 1 && minusOne.hi == -1);
  const pbMoment128 zero = pbFixedNormalised(0);
  CHECK(zero.lo == 0 && zero.hi == 0);
  const __int128 big = (__int128)max63 * (1 << 16);
  const __int128 normalCases[] = {0, 1, -1, two32 - 1, two32, two32 + 1, -two32 + 1, -two32, -two32 - 1, max63, -max63,
                                  big, -big, big + 12345, -big - 12345};
  for (const __int128 v : normalCases) checkNormalised(v);
  for (int k = 0; k < 4096; k++) checkNormalised((__int128)(long long)nextRandom() * (long long)(nextRandom() >> 34));

  if (failures) return 1;
  printf("pb_fixed_check ok\n");
  return 0;
}
