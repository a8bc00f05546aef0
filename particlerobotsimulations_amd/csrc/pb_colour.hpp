// pb_colour.hpp -- the reference's bot colour (updateCol_k, particlebot_kernel_impl.cuh:351-443) as device code shared
// by the display kernels (pb_display.hip) and the frame rasteriser (pb_render.hip).
#pragma once

#include "pb_device.hpp"

namespace {

// ---- colour (impl.cuh:351-443) -------------------------------------------------------------------------------
// The HSL round trip is written with C's usual arithmetic conversions made explicit: every double literal promotes
// its expression to double, and the result narrows back to float where the reference assigns, passes or returns a
// float.  Device double arithmetic is IEEE (no contraction under -ffp-contract=off), so the bits are the reference's.

__device__ float pbHue2Rgb(float p, float q, float t) {  // impl.cuh:351-358
  if (t < 0) t = t + 1.0f;
  if (t > 1) t = t - 1.0f;
  if ((double)t < 1.0 / 6.0) return (float)((double)p + (double)(q - p) * 6.0 * (double)t);
  if ((double)t < 1.0 / 2.0) return q;
  if ((double)t < 2.0 / 3.0) return (float)((double)p + (double)(q - p) * (2.0 / 3.0 - (double)t) * 6.0);
  return p;
}

__device__ void pbHslToRgb(float h, float s, float l, float &r, float &g, float &b) {  // impl.cuh:359-374
  if (s == 0) {
    r = l;
    g = l;
    b = l;
  } else {
    const float q = (double)l < 0.5 ? (float)((double)l * (1.0 + (double)s)) : l + s - l * s;
    const float p = (float)(2.0 * (double)l - (double)q);
    r = pbHue2Rgb(p, q, (float)((double)h + 1.0 / 3.0));
    g = pbHue2Rgb(p, q, h);
    b = pbHue2Rgb(p, q, (float)((double)h - 1.0 / 3.0));
  }
}

__device__ void pbRgbToHsl(float r, float g, float b, float &h, float &s, float &l) {  // impl.cuh:376-398
  const float mx = fmaxf(fmaxf(r, g), b);
  const float mn = fminf(fminf(r, g), b);
  h = (mx + mn) / 2;
  s = (mx + mn) / 2;
  l = (mx + mn) / 2;
  if (mx == mn) {
    h = s = 0;
  } else {
    const float d = mx - mn;
    s = (double)l > 0.5 ? (float)((double)d / (2.0 - (double)mx - (double)mn)) : d / (mx + mn);
    if (mx == r)
      h = (float)((double)((g - b) / d) + (g < b ? 6.0 : 0.0));
    else if (mx == g)
      h = (float)((double)((b - r) / d) + 2.0);
    else
      h = (float)((double)((r - g) / d) + 4.0);
    h = (float)((double)h / 6.0);
  }
}

// one bot's colour; `c` carries the alpha through (impl.cuh:401-443).  powf(x, 2) -> x*x and powf(x, 0.5f) -> sqrtf
// as everywhere else (pb_device.hpp), the reference's operation order kept: (200-20)*A / B, then +20, then /255.
__device__ float4 pbBotColour(const PbDevParams &P, uint32_t displayShadow, float px, float py, float rad, int dead,
                              float4 c) {
  if (dead) {
    c.x = 0.0f;
    c.y = 0.0f;
    c.z = 0.0f;
    return c;
  }
  const float a = P.max_radius - rad, s = P.max_radius - P.min_radius;
  c.x = 30.0f / 255.0f;
  c.y = (20.0f + (200.0f - 20.0f) * (a * a) / (s * s)) / 255.0f;
  c.z = (30.0f + (210.0f - 30.0f) * sqrtf(rad - P.min_radius) / sqrtf(s)) / 255.0f;
  if (displayShadow && pbInShadow(P, px, py)) {
    float h = 137, sat = 36, l = 42;
    pbRgbToHsl(c.x, c.y, c.z, h, sat, l);
    pbHslToRgb(h, sat, (float)((double)l / 2.0), c.x, c.y, c.z);
  }
  return c;
}

}  // namespace
