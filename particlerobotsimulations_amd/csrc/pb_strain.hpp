// pb_strain.hpp -- the arithmetic of the strain analysis that has no device in it (pb_strain.hip holds the kernel and the
// entry points; include/particlebot_hip.h has the definitions): which bond is used, and the Falk-Langer fit of a bot's
// nine integer moments.  Compiles as plain C++ (tests/pb_strain_check.cpp); the kernel and the host's gradient writer
// both call pbStrainFit, so there is one statement of the fit and the device's d2 is the host's, bit for bit.
//
// The fit is binary64 with every operation rounded once and in the order written below.  On the device the operations
// are the explicitly rounded intrinsics (__dmul_rn, __dadd_rn, __ddiv_rn); on the host they are plain operators in
// functions that switch contraction off.  The build passes -ffp-contract=off to both sides as well.  The moments are
// below 2^63 in magnitude (pb_strain.hip states why) and are converted with round-to-nearest.
#pragma once

#include <stdint.h>

#include "pb_fixed.hpp"

constexpr uint32_t PB_STRAIN_MAX_LIST = 1u << 16;  // a bot with this many marked entries or more is unfitted

// the bond rule's test of one of the four values: a NaN or an infinity fails the comparison
PB_FIXED_HD bool pbStrainInReach(float v) { return __builtin_fabsf(v) < PB_STRAIN_REACH; }

namespace pb_strain_ops {
#if defined(__HIP_DEVICE_COMPILE__)
PB_FIXED_HD double mul(double x, double y) { return __dmul_rn(x, y); }
PB_FIXED_HD double sub(double x, double y) { return __dadd_rn(x, -y); }  // (x - y is x + (-y): the negation is exact)
PB_FIXED_HD double add(double x, double y) { return __dadd_rn(x, y); }
PB_FIXED_HD double div(double x, double y) { return __ddiv_rn(x, y); }
PB_FIXED_HD double real(long long v) { return __ll2double_rn(v); }
#else
#if defined(__clang__)
#define PB_STRAIN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PB_STRAIN_NO_CONTRACT
#endif
PB_FIXED_HD double mul(double x, double y) { PB_STRAIN_NO_CONTRACT return x * y; }
PB_FIXED_HD double sub(double x, double y) { PB_STRAIN_NO_CONTRACT return x - y; }
PB_FIXED_HD double add(double x, double y) { PB_STRAIN_NO_CONTRACT return x + y; }
PB_FIXED_HD double div(double x, double y) { PB_STRAIN_NO_CONTRACT return x / y; }
PB_FIXED_HD double real(long long v) { return (double)v; }
#endif
}  // namespace pb_strain_ops

struct PbStrainFit {
  double jxx, jxy, jyx, jyy;  // the local deformation gradient: d ~ J d0
  double d2;                  // D2min, units of 2^-40
  bool fitted;
};

// m: the nine moments in the header's order (PB_STRAIN_K ... PB_STRAIN_W)
template <typename Moments>
PB_FIXED_HD PbStrainFit pbStrainFit(const Moments &m) {
  using namespace pb_strain_ops;
  PbStrainFit f;
  f.jxx = f.jxy = f.jyx = f.jyy = f.d2 = 0.0;
  const double a = real(m[PB_STRAIN_YXX]), b = real(m[PB_STRAIN_YXY]), c = real(m[PB_STRAIN_YYY]);
  const double det = sub(mul(a, c), mul(b, b));
  f.fitted = m[PB_STRAIN_K] >= 3 && det > 0.0;
  if (!f.fitted) return f;
  const double xxx = real(m[PB_STRAIN_XXX]), xxy = real(m[PB_STRAIN_XXY]);
  const double xyx = real(m[PB_STRAIN_XYX]), xyy = real(m[PB_STRAIN_XYY]);
  f.jxx = div(sub(mul(xxx, c), mul(xxy, b)), det);
  f.jxy = div(sub(mul(xxy, a), mul(xxx, b)), det);
  f.jyx = div(sub(mul(xyx, c), mul(xyy, b)), det);
  f.jyy = div(sub(mul(xyy, a), mul(xyx, b)), det);
  const double fit = add(add(mul(f.jxx, xxx), mul(f.jxy, xxy)), add(mul(f.jyx, xyx), mul(f.jyy, xyy)));
  const double d2 = sub(real(m[PB_STRAIN_W]), fit);
  f.d2 = d2 > 0.0 ? d2 : 0.0;
  return f;
}

// e = (unsigned long long)rint(d2) of a d2 >= 0; 2^63 for a d2 of 2^63 or more (only the rounding of an ill-conditioned
// fit gets there: W itself is below 2^63)
PB_FIXED_HD unsigned long long pbStrainUnits(double d2) {
  return d2 < 9223372036854775808.0 ? (unsigned long long)__builtin_rint(d2) : 1ull << 63;
}
