// pb_strain_check.cpp -- the strain analysis' fit (csrc/pb_strain.hpp) as plain C++, for tests/test_strain_api.py: reads
// rows of nine integer moments (k Yxx Yxy Yyy Xxx Xxy Xyx Xyy W) from standard input and prints, per row, whether the bot
// is fitted, the bit patterns of Jxx Jxy Jyx Jyy and d2 as 16 hex digits each, and e = pbStrainUnits(d2).  The test
// evaluates the same table with tests/strain_ref.py and compares the lines.  Also checks the bond rule's reach here.
#include <stdio.h>
#include <string.h>

#include <cmath>

#include "pb_strain.hpp"

static unsigned long long bitsOf(double v) {
  unsigned long long u;
  static_assert(sizeof u == sizeof v, "binary64");
  memcpy(&u, &v, sizeof u);
  return u;
}

int main() {
  int bad = 0;
  const float below = std::nextafterf(PB_STRAIN_REACH, 0.0f);
  bad += !pbStrainInReach(below) || !pbStrainInReach(-below) || pbStrainInReach(PB_STRAIN_REACH);
  bad += pbStrainInReach(-PB_STRAIN_REACH) || pbStrainInReach(NAN) || pbStrainInReach(INFINITY) || !pbStrainInReach(0.0f);
  bad += pbFixedQuantise(below) != (1ll << 23) || pbFixedQuantise(-below) != -(1ll << 23);  // the largest q, a tie to even
  bad += pbStrainUnits(0.5) != 0ull || pbStrainUnits(1.5) != 2ull || pbStrainUnits(9223372036854775808.0) != 1ull << 63;
  bad += pbStrainUnits(1e300) != 1ull << 63 || pbStrainUnits(9223372036854774784.0) != 9223372036854774784ull;
  if (bad) {
    printf("pb_strain_check FAILED: the bond rule or the units\n");
    return 1;
  }
  long long m[PB_STRAIN_MOMENTS];
  size_t rows = 0;
  for (;;) {
    int got = 0;
    for (int c = 0; c < PB_STRAIN_MOMENTS; c++) got += scanf("%lld", &m[c]) == 1;
    if (got == 0) break;
    if (got != PB_STRAIN_MOMENTS) {
      printf("pb_strain_check FAILED: a row of %d words\n", got);
      return 1;
    }
    const PbStrainFit f = pbStrainFit(m);
    printf("%d %016llx %016llx %016llx %016llx %016llx %llu\n", f.fitted ? 1 : 0, bitsOf(f.jxx), bitsOf(f.jxy),
           bitsOf(f.jyx), bitsOf(f.jyy), bitsOf(f.d2), f.fitted ? pbStrainUnits(f.d2) : 0ull);
    rows++;
  }
  printf("pb_strain_check ok: %zu rows\n", rows);
  return 0;
}
