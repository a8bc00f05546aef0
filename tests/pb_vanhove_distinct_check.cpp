// Stand-alone check of the radial bin rules the distinct van Hove kernel can be built with (csrc/pb_vanhove.hpp, behind
// PB_VHD_BIN_RULE in csrc/pb_vanhove_distinct.hip): the self part's binary search, the guess corrected against the edges
// (pbVhRadialBinFrom) and the integer square root with one division (pbVhRadialBinRoot).  For every s the kernel can
// hand them, s < (bins qw)^2 with bins qw < 2^31, all three must give max{k : (k qw)^2 <= s}.  Swept here: every edge and
// its two neighbours, for qw in {1, 3, 2^17, 2^31 / bins - 1} and bins in {1, 2, 64, 1024}, and 200000 random s per
// shape; the corrected guess from the best guess there is (the fp32 one the kernel forms), from the two ends of the
// histogram and from a guess out of range.  Built plainly and with -fsanitize=address,undefined and run as a program by
// tests/test_vanhove_distinct_api.py.
#include <cmath>
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
      if (failures < 20) printf("FAILED line %d: %s\n", __LINE__, #cond); \
      failures++;                                                \
    }                                                            \
  } while (0)

// xorshift64*: the random s need no quality, only to be the same in every run
unsigned long long state = 0x9E3779B97F4A7C15ull;
unsigned long long nextRandom() {
  state ^= state >> 12, state ^= state << 25, state ^= state >> 27;
  return state * 0x2545F4914F6CDD1Dull;
}

// the definition as a plain loop in 128 bits
uint32_t plainRadial(uint32_t qw, uint32_t bins, unsigned long long s) {
  uint32_t best = 0;
  for (uint32_t k = 0; k < bins; k++) {
    const u128 e = (u128)k * qw;
    if (e * e <= (u128)s) best = k;
  }
  return best;
}

struct Shape {
  uint32_t qw, bins;
  std::vector<unsigned long long> edges;
  float invWidth;
};

// the guess the kernel forms: the fp32 root of the fp32 squared distance times the reciprocal of the width
uint32_t kernelGuess(const Shape &S, unsigned long long s) {
  const float d2 = (float)((double)s / 1099511627776.0);  // s 2^-40, rounded once more than the walk's d2: a guess
  return (uint32_t)(int)(sqrtf(d2) * S.invWidth);
}

void checkOne(const Shape &S, unsigned long long s, bool slow) {
  if (s >= S.edges[S.bins]) return;  // not counted: the kernel asks none of the rules
  const auto edgeAt = [&](uint32_t k) { return S.edges[k]; };
  const uint32_t want = pbVhRadialBin(edgeAt, S.bins, s);
  CHECK(want < S.bins);
  if (slow) CHECK(want == plainRadial(S.qw, S.bins, s));
  CHECK(S.edges[want] <= s && s < S.edges[want + 1u]);
  CHECK(pbVhRadialBinRoot(S.qw, s) == want);
  for (uint32_t guess : {kernelGuess(S, s), 0u, S.bins - 1u, S.bins, S.bins + 5u, 0xFFFFFFFFu, want, want + 1u})
    CHECK(pbVhRadialBinFrom(edgeAt, S.bins, s, guess) == want);
  if (want) CHECK(pbVhRadialBinFrom(edgeAt, S.bins, s, want - 1u) == want);
  const uint32_t root = pbVhIsqrt(s);
  CHECK((unsigned long long)root * root <= s && ((unsigned long long)root + 1ull) * ((unsigned long long)root + 1ull) > s);
}

}  // namespace

int main() {
  CHECK(PB_VHD_HEAD == 2 && pbVhdCellWords(1024u) == 1026u && PB_VHD_CENTRES == 0 && PB_VHD_PARTNERS == 1);
  // the integer root at squares and next to them, up to the largest s < 2^62
  for (unsigned long long r : {0ull, 1ull, 2ull, 3ull, 65535ull, 65536ull, 94906265ull, 94906266ull, 94906267ull,
                               (1ull << 26) + 5ull, (1ull << 31) - 2ull, (1ull << 31) - 1ull}) {
    CHECK(pbVhIsqrt(r * r) == r);
    if (r) CHECK(pbVhIsqrt(r * r - 1ull) == r - 1ull);
    if (r < (1ull << 31) - 1ull) CHECK(pbVhIsqrt(r * r + 2ull * r) == r && pbVhIsqrt((r + 1ull) * (r + 1ull)) == r + 1ull);
  }
  CHECK(pbVhIsqrt((1ull << 62) - 1ull) == (1u << 31) - 1u);
  const uint32_t counts[] = {1u, 2u, 64u, 1024u};
  for (uint32_t bins : counts) {
    const uint32_t widths[] = {1u, 3u, 1u << 17, (uint32_t)((1ull << 31) / bins) - 1u};
    for (uint32_t qw : widths) {
      if ((unsigned long long)qw * bins >= (1ull << 31)) continue;  // (2^17 x 1024 ... is no shape the setter admits)
      Shape S;
      S.qw = qw, S.bins = bins, S.edges.resize(bins + 1u), S.invWidth = 1.0f / ((float)qw / 1048576.0f);
      pbVhEdges(qw, bins, S.edges.data());
      CHECK(S.edges[bins] == (unsigned long long)qw * bins * ((unsigned long long)qw * bins) && S.edges[bins] < (1ull << 62));
      for (uint32_t k = 0; k <= bins; k++) {
        checkOne(S, S.edges[k], true);
        checkOne(S, S.edges[k] + 1ull, true);
        if (S.edges[k]) checkOne(S, S.edges[k] - 1ull, true);
      }
      for (int k = 0; k < 200000; k++) checkOne(S, nextRandom() % S.edges[bins], k < 2000);
      // uniform in the root as well: uniform s crowds the outer bins
      for (int k = 0; k < 200000; k++) {
        const unsigned long long r = nextRandom() % ((unsigned long long)qw * bins);
        checkOne(S, r * r + nextRandom() % (2ull * r + 1ull), false);
      }
    }
  }
  if (failures) return printf("pb_vanhove_distinct_check: %d FAILED\n", failures), 1;
  printf("pb_vanhove_distinct_check ok\n");
  return 0;
}
