// Stand-alone check of the arithmetic of the self van Hove function (csrc/pb_vanhove.hpp) against plain 128-bit loops on
// the CPU: the edge table, the radial rule at and around every edge, the axis rule at and around every multiple of the
// width for both signs, the four accumulators of the fourth power and their 192-bit composition.  Built plainly and
// with -fsanitize=address,undefined and run as a program by tests/test_vanhove_ref.py.  The kernel calls the same
// functions; it has no floating point guess, so there is no guess function to sweep.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pb_vanhove.hpp"

namespace {

typedef unsigned __int128 u128;

int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      failures++;                                                \
    }                                                            \
  } while (0)

const uint32_t TOP = 2147483520u;  // 2^31 - 128, the largest quantised magnitude
const unsigned long long S_MAX = (1ull << 63) - 1ull;

// the definition, as a plain loop in 128 bits: max{k : min((k qw)^2, 2^63) <= s} for k = 0 ... bins
uint32_t plainRadial(uint32_t qw, uint32_t bins, unsigned long long s) {
  uint32_t best = 0;
  for (uint32_t k = 0; k <= bins; k++) {
    u128 e = (u128)k * qw;
    e *= e;
    if (e > (u128)1 << 63) e = (u128)1 << 63;
    if (e <= (u128)s) best = k;
  }
  return best;
}

// floor(q / qw) towards minus infinity in 64 bits
long long plainFloor(long long q, long long qw) {
  long long b = q / qw;
  if (q % qw != 0 && q < 0) b--;
  return b;
}

void checkRadial(const std::vector<unsigned long long> &edges, uint32_t qw, uint32_t bins, unsigned long long s) {
  if (s > S_MAX) return;  // (an s is below 2^63: a saturated edge and what is above it are no inputs)
  const auto edgeAt = [&](uint32_t k) { return edges[k]; };
  const uint32_t got = pbVhRadialBin(edgeAt, bins, s), want = plainRadial(qw, bins, s);
  CHECK(got == want);
  CHECK(got <= bins);
  CHECK((got == bins) == (s >= edges[bins]));  // bins says "beyond"
}

void checkAxis(uint32_t qw, uint32_t bins, long long q) {
  if (q > (long long)TOP || q < -(long long)TOP) return;
  const long long want = plainFloor(q, (long long)qw);
  CHECK((long long)pbVhAxisFloor((int)q, qw) == want);
  const uint32_t at = pbVhAxisIndex((int)q, qw, bins);
  if (want >= -(long long)bins && want < (long long)bins) CHECK((long long)at == want + (long long)bins);
  else CHECK(at == 2u * bins);
}

void checkQ4(unsigned long long s, unsigned long long times) {
  // `times` samples of s: the accumulators as the device would hold them, without the loop
  const u128 sq = (u128)s * s;
  unsigned long long a[4] = {0, 0, 0, 0}, one[4] = {0, 0, 0, 0};
  pbVhQ4Add((unsigned long long)sq, (unsigned long long)(sq >> 64), one[0], one[1], one[2], one[3]);
  for (int k = 0; k < 4; k++) {
    CHECK(one[k] < (1ull << 32));
    a[k] = one[k] * times;  // below 2^63 for fewer than 2^31 samples
    CHECK(a[k] < (1ull << 63) && (!times || a[k] / times == one[k]));
  }
  CHECK(((u128)one[3] << 96) + ((u128)one[2] << 64) + ((u128)one[1] << 32) + (u128)one[0] == sq);
  unsigned long long limbs[3];
  pbVhQ4Compose(a[0], a[1], a[2], a[3], limbs);
  // sq * times in 192 bits: the low 128 bits and the carry out of them
  const u128 lowHalf = (u128)(unsigned long long)sq * times, highHalf = (u128)(unsigned long long)(sq >> 64) * times;
  const u128 mid = (lowHalf >> 64) + (u128)(unsigned long long)highHalf;
  const unsigned long long w0 = (unsigned long long)lowHalf, w1 = (unsigned long long)mid;
  const unsigned long long w2 = (unsigned long long)((mid >> 64) + (highHalf >> 64));
  CHECK(limbs[0] == w0 && limbs[1] == w1 && limbs[2] == w2);
}

}  // namespace

int main() {
  CHECK(PB_VH_MOMENTS == 10 && pbVhCellWords(1024u) == 10u + 5u * 1024u);
  CHECK(pbVhXAt(7u) == 7u && pbVhYAt(7u) == 21u && pbVhRadialAt(7u) == 0u);
  const uint32_t widths[] = {1u, 2u, 3u, 314573u, 1u << 20, (1u << 30) + 1u, TOP};
  const uint32_t counts[] = {1u, 2u, 1024u};
  for (uint32_t qw : widths)
    for (uint32_t bins : counts) {
      std::vector<unsigned long long> edges(bins + 1u);
      pbVhEdges(qw, bins, edges.data());
      CHECK(edges[0] == 0ull);
      for (uint32_t k = 0; k <= bins; k++) {
        u128 e = (u128)k * qw;
        e *= e;
        CHECK(edges[k] == (e < (u128)1 << 63 ? (unsigned long long)e : 1ull << 63));
        if (k) CHECK(edges[k] >= edges[k - 1u]);
        // every edge and its two neighbours, the saturated ones included (those above 2^63 - 1 are skipped as inputs)
        checkRadial(edges, qw, bins, edges[k]);
        checkRadial(edges, qw, bins, edges[k] + 1ull);
        if (edges[k]) checkRadial(edges, qw, bins, edges[k] - 1ull);
      }
      checkRadial(edges, qw, bins, 0ull);
      checkRadial(edges, qw, bins, S_MAX);
      checkRadial(edges, qw, bins, 2ull * TOP * TOP);  // the largest s there is
      const auto edgeAt = [&](uint32_t k) { return edges[k]; };
      CHECK(pbVhRadialBin(edgeAt, bins, 0ull) == 0u);  // a displacement of zero lands in bin 0
      if ((u128)bins * qw * ((u128)bins * qw) > (u128)S_MAX) CHECK(pbVhRadialBin(edgeAt, bins, S_MAX) < bins);
      // the axis rule: k qw and its neighbours for both signs, across the histogram's ends and at the range's ends
      for (long long k = -(long long)bins - 2; k <= (long long)bins + 2; k++)
        for (long long d = -1; d <= 1; d++) checkAxis(qw, bins, k * (long long)qw + d);
      for (long long q : {0ll, 1ll, -1ll, (long long)TOP, -(long long)TOP, (long long)TOP - 1, -(long long)TOP + 1})
        checkAxis(qw, bins, q);
      CHECK(pbVhAxisIndex(0, qw, bins) == bins);  // zero is the first counter of the upper half
      CHECK(pbVhAxisIndex(-1, qw, bins) == bins - 1u);
      if ((long long)bins * qw <= (long long)TOP) {
        CHECK(pbVhAxisIndex((int)((long long)bins * qw), qw, bins) == 2u * bins);        // exactly bins widths: beyond
        CHECK(pbVhAxisIndex((int)((long long)bins * qw) - 1, qw, bins) == 2u * bins - 1u);
        CHECK(pbVhAxisIndex(-(int)((long long)bins * qw), qw, bins) == 0u);              // the lowest edge is inside
        if ((long long)bins * qw < (long long)TOP) CHECK(pbVhAxisIndex(-(int)((long long)bins * qw) - 1, qw, bins) == 2u * bins);
      }
    }
  // the fourth power at the accumulators' bounds: the largest s, 2^31 - 1 samples
  const unsigned long long most = (1ull << 31) - 1ull;
  for (unsigned long long s : {0ull, 1ull, 0xFFFFFFFFull, 0x100000000ull, 2ull * TOP * TOP, S_MAX, 0x7FFFFFFF00000001ull,
                               0x00000001FFFFFFFFull})
    for (unsigned long long times : {0ull, 1ull, 2ull, 65537ull, most}) checkQ4(s, times);
  // every accumulator at its largest: 2^63 - 2^31 - ... each below 2^63; the composition is their weighted sum
  {
    const unsigned long long a = 0xFFFFFFFFull * most;
    unsigned long long limbs[3];
    pbVhQ4Compose(a, a, a, a, limbs);
    const u128 low = (u128)a + ((u128)a << 32), high = (low >> 64) + (u128)a + ((u128)a << 32);
    CHECK(limbs[0] == (unsigned long long)low && limbs[1] == (unsigned long long)high &&
          limbs[2] == (unsigned long long)(high >> 64));
    CHECK(limbs[2] >= (a >> 32) && limbs[2] <= (a >> 32) + 1ull);  // a3's upper half, plus at most one carry
  }
  if (failures) return printf("pb_vanhove_check: %d FAILED\n", failures), 1;
  printf("pb_vanhove_check ok\n");
  return 0;
}
