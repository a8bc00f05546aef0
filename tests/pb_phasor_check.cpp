// Stand-alone check of the phasor kit's host-callable part (csrc/pb_phasor.hpp): the index function at its edges, the
// turn of a bot at every box length, and the table.  tests/test_sfactor_ref.py builds it under AddressSanitizer and
// UBSan and runs it; it needs no GPU.
#include <stdio.h>

#include <vector>

#include "pb_phasor.hpp"

static int failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAILED line %d: %s\n", __LINE__, #cond);            \
      failures++;                                                 \
    }                                                             \
  } while (0)

// CRC-32 as zlib computes it (reflected, polynomial 0xEDB88320)
static uint32_t crc32(const unsigned char *p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int b = 0; b < 8; b++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

int main() {
  // the index: the nearest of 4096 steps, a tie up, the last half step wraps to 0
  CHECK(pbPhasorIndex(0u) == 0u);
  CHECK(pbPhasorIndex(0x7FFFFu) == 0u);
  CHECK(pbPhasorIndex(0x80000u) == 1u);
  CHECK(pbPhasorIndex(0xFFF7FFFFu) == 4095u);
  CHECK(pbPhasorIndex(0xFFF80000u) == 0u);
  CHECK(pbPhasorIndex(0xFFFFFFFFu) == 0u);
  CHECK(pbPhasorIndex(0x40000000u) == 1024u);
  CHECK(pbPhasorIndex(0x80000000u) == 2048u);
  for (uint32_t j = 0; j < PB_PHASOR_STEPS; j++) {
    CHECK(pbPhasorIndex(j << 20) == j);
    CHECK(pbPhasorIndex((j << 20) + 0x7FFFFu) == j);
    CHECK(pbPhasorIndex((j << 20) - 0x80000u) == j);
  }
  // the turn at every box length L = 2^e: a bot a quarter of the box along x (L / 4 = 2^(e - 2), in units of 2^-20)
  for (int e = PB_SK_MIN_LOG2; e <= PB_SK_MAX_LOG2; e++) {
    const int shift = pbPhasorShift(e);
    CHECK(shift >= 0 && shift <= 20);
    const uint32_t quarter = 1u << (20 + e - 2), zero = 0u;
    CHECK(pbPhasorTurn(1u, 0u, quarter, zero, shift) == 0x40000000u);
    CHECK(pbPhasorIndex(pbPhasorTurn(1u, 0u, quarter, zero, shift)) == 1024u);
    CHECK(pbPhasorIndex(pbPhasorTurn(0u, 1u, zero, quarter, shift)) == 1024u);
    CHECK(pbPhasorIndex(pbPhasorTurn(3u, 0u, quarter, zero, shift)) == 3072u);
    CHECK(pbPhasorIndex(pbPhasorTurn(1u, 1u, quarter, quarter, shift)) == 2048u);
    CHECK(pbPhasorIndex(pbPhasorTurn(4u, 0u, quarter, zero, shift)) == 0u);  // a whole turn
    // negative integers and negative positions as their 32-bit words
    CHECK(pbPhasorIndex(pbPhasorTurn((uint32_t)-1, 0u, quarter, zero, shift)) == 3072u);
    CHECK(pbPhasorIndex(pbPhasorTurn(1u, 0u, (uint32_t)(-(int)quarter), zero, shift)) == 3072u);
    CHECK(pbPhasorIndex(pbPhasorTurn((uint32_t)-1, (uint32_t)-1, (uint32_t)(-(int)quarter), zero, shift)) == 1024u);
    // aliasing: (2^31 - 1, -2^31) is (-1, 0) wherever the shift is at least 1, so at every e below 12
    if (shift >= 1)
      CHECK(pbPhasorTurn(0x7FFFFFFFu, 0x80000000u, quarter, 12345u, shift) == pbPhasorTurn((uint32_t)-1, 0u, quarter, zero, shift));
  }
  // the table
  std::vector<int> t(2u * PB_PHASOR_STEPS);
  pbPhasorBuild(t.data());
  const int one = 1 << PB_PHASOR_UNIT_LOG2;
  CHECK(t[0] == one && t[1] == 0);
  CHECK(t[2 * 1024] == 0 && t[2 * 1024 + 1] == one);
  CHECK(t[2 * 2048] == -one && t[2 * 2048 + 1] == 0);
  CHECK(t[2 * 3072] == 0 && t[2 * 3072 + 1] == -one);
  for (uint32_t j = 1; j < PB_PHASOR_STEPS; j++) {
    CHECK(t[2 * j] == t[2 * (PB_PHASOR_STEPS - j)]);
    CHECK(t[2 * j + 1] == -t[2 * (PB_PHASOR_STEPS - j) + 1]);
  }
  for (uint32_t j = 0; j < PB_PHASOR_STEPS; j++) {
    CHECK(t[2 * j + 1] == t[2 * ((j - 1024u) & 4095u)]);
    const long long c = t[2 * j], s = t[2 * j + 1], norm = c * c + s * s - (long long)one * one;
    CHECK(norm > -2ll * one && norm < 2ll * one);  // on the circle to within the entries' rounding
  }
  unsigned char bytes[8u * PB_PHASOR_STEPS];
  for (uint32_t k = 0; k < 2u * PB_PHASOR_STEPS; k++)
    for (int b = 0; b < 4; b++) bytes[4u * k + b] = (unsigned char)((uint32_t)t[k] >> (8 * b));  // little-endian
  CHECK(crc32(bytes, sizeof bytes) == 3228437924u);
  if (failures) {
    printf("pb_phasor_check: %d FAILED\n", failures);
    return 1;
  }
  printf("pb_phasor_check ok\n");
  return 0;
}
