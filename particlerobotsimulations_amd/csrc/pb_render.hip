// pb_render.hip -- the headless frame (Particlebot::writeFrame, particlebot.cpp) rasterised on gfx950 from the engine's
// resident state: byte for byte the host writer's picture, with 3 W H bytes leaving the device instead of the state.
//
// The host paints items in order (background, rectangles, circle obstacles, light, bots by original index, trail) and a
// pixel keeps the last item that covers it.  Here every pixel holds one uint32 key, the maximum over the items that
// cover it:  0 nothing, orig + 1 a bot (nCells <= 2^32 - 32, pbSimCreateBatch, so no index bit is taken),
// 0xFFFFFFFF a trail disc.  Maxima do not depend on the order of the atomics, so a frame is deterministic.
//   k_render_bots<LANES>   one bot per LANES lanes, slot order (coalesced); culls, scatters the key over the disc's
//                          clamped box, and leaves the bot's RGB8 at rgb8[orig]
//   k_render_trail<LANES>  the same for the recorded slots of the member's centroid ring (reference style, trail on)
//   k_render_resolve       four pixels per lane: the analytic items under the key, 12 bytes of packed RGB out
// The coverage test is the host's, operation for operation, in fp32 without contraction.
#include "pb_colour.hpp"
#include "pb_device.hpp"
#include "pb_internal.hpp"

namespace {

constexpr uint32_t KEY_TRAIL = 0xFFFFFFFFu;

PB_DEV float viewX(const PbRenderParams &V, float x) { return V.halfW - (x - V.centerX) * V.scale; }
PB_DEV float viewY(const PbRenderParams &V, float y) { return V.halfH - (y - V.centerY) * V.scale; }

// A disc in pixel space with the host's clamped floorf / ceilf box.  The clamps are applied before the conversion to
// int (same integers as the host's max / min after it for everything an int holds); a disc whose centre or radius is
// not finite has no box.
struct PixDisc {
  float cx, cy, r2;
  int x0, x1, y0, y1;  // inclusive; x0 > x1: draws nothing
};

PB_DEV PixDisc pixDisc(const PbRenderParams &V, float x, float y, float r) {
  PixDisc d;
  d.cx = viewX(V, x);
  d.cy = viewY(V, y);
  const float pr = r * V.scale;
  d.r2 = pr * pr;
  d.x0 = 1, d.x1 = 0, d.y0 = 1, d.y1 = 0;
  const float xlo = floorf(d.cx - pr), xhi = ceilf(d.cx + pr), ylo = floorf(d.cy - pr), yhi = ceilf(d.cy + pr);
  const float wm = (float)(V.width - 1), hm = (float)(V.height - 1);
  const float inf = __builtin_inff();
  if (!(fabsf(d.cx) < inf) || !(fabsf(d.cy) < inf) || !(fabsf(pr) < inf)) return d;
  if (!(xhi >= 0.0f) || !(xlo <= wm) || !(yhi >= 0.0f) || !(ylo <= hm)) return d;  // box misses the frame
  d.x0 = (int)fmaxf(xlo, 0.0f);
  d.x1 = (int)fminf(xhi, wm);
  d.y0 = (int)fmaxf(ylo, 0.0f);
  d.y1 = (int)fminf(yhi, hm);
  return d;
}

PB_DEV bool discCovers(const PixDisc &d, int xx, int yy) {
  if (xx < d.x0 || xx > d.x1 || yy < d.y0 || yy > d.y1) return false;
  const float dx = (float)xx + 0.5f - d.cx, dy = (float)yy + 0.5f - d.cy;
  return dx * dx + dy * dy <= d.r2;
}

// lane `sub` of the LANES that share the disc: columns sub, sub + LANES, ... of every row of the box
template <int LANES>
PB_DEV void scatterDisc(uint32_t *__restrict__ ids, int width, const PixDisc &d, uint32_t key, int sub) {
  for (int yy = d.y0; yy <= d.y1; yy++) {
    const float dy = (float)yy + 0.5f - d.cy;
    const float dy2 = dy * dy;
    uint32_t *row = ids + (size_t)yy * (size_t)width;
    for (int xx = d.x0 + sub; xx <= d.x1; xx += LANES) {
      const float dx = (float)xx + 0.5f - d.cx;
      if (dx * dx + dy2 <= d.r2) atomicMax(row + xx, key);
    }
  }
}

PB_DEV uint32_t packRgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

// min(255, max(0, lrintf(c * 255.0f))): round to nearest even.  A NaN or an infinity (max_radius == min_radius) gives
// 0, as the host's lrintf does for them on x86-64 (LONG_MIN).
PB_DEV uint32_t channel8(float c) {
  float v = rintf(c * 255.0f);
  v = v > 0.0f && v < __builtin_inff() ? v : 0.0f;
  v = v < 255.0f ? v : 255.0f;
  return (uint32_t)v;
}

// (unsigned char)std::min(255.0f, std::max(0.0f, v)): std::max / std::min keep their first argument on a NaN
PB_DEV uint32_t trunc8(float v) {
  float m = 0.0f < v ? v : 0.0f;
  m = m < 255.0f ? m : 255.0f;
  return (uint32_t)m;
}

PB_DEV uint32_t botRgb8(const PbDevParams &P, const PbRenderParams &V, float x, float y, float r, int dead) {
  if (V.style) {  // the device colours (updateCol_k)
    const float4 c = pbBotColour(P, V.displayShadow, x, y, r, dead, make_float4(0, 0, 0, 1.0f));
    return packRgb(channel8(c.x), channel8(c.y), channel8(c.z));
  }
  if (dead) return 0u;
  const float span = P.max_radius - P.min_radius;
  const float g = span > 0 ? (P.max_radius - r) / span : 0.0f;
  const float b = span > 0 ? (r - P.min_radius) / span : 0.0f;
  const float b0 = 0.0f < b ? b : 0.0f;
  return packRgb(30u, trunc8(20.0f + 180.0f * g * g), trunc8(30.0f + 180.0f * sqrtf(b0)));
}

template <int LANES>
__global__ __launch_bounds__(256) void k_render_bots(const PbDevParams *__restrict__ params, uint32_t member,
                                                     PbRenderParams V, const float4 *__restrict__ pr,
                                                     const int *__restrict__ dead, const uint32_t *__restrict__ orig,
                                                     uint32_t n, uint32_t *__restrict__ ids,
                                                     uint32_t *__restrict__ rgb8) {
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t l = g / LANES;
  const int sub = (int)(g % LANES);
  if (l >= n) return;
  const size_t s = (size_t)member * n + l;
  const float4 q = pr[s];
  const PixDisc d = pixDisc(V, q.x, q.y, q.z);
  if (d.x0 > d.x1 || d.y0 > d.y1) return;
  const uint32_t o = orig[s];
  if (sub == 0) rgb8[o] = botRgb8(params[member], V, q.x, q.y, q.z, dead[s]);
  scatterDisc<LANES>(ids, V.width, d, o + 1u, sub);
}

template <int LANES>
__global__ __launch_bounds__(256) void k_render_trail(PbRenderParams V, const float2 *__restrict__ ring, uint32_t slots,
                                                      float radius, uint32_t *__restrict__ ids) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  const uint32_t k = g / LANES;
  const int sub = (int)(g % LANES);
  if (k >= slots) return;
  const float2 v = ring[k];
  if (!(v.x != -5000.0f)) return;  // never written (particlebot.cpp:776-779)
  const PixDisc d = pixDisc(V, v.x, v.y - 2000.0f, radius);
  if (d.x0 > d.x1 || d.y0 > d.y1) return;
  scatterDisc<LANES>(ids, V.width, d, KEY_TRAIL, sub);
}

// the host's inclusive floorf / ceilf bounds of a rectangle side, clamped to [-1, limit] before the conversion
PB_DEV int sideLo(float v, int limit) { return (int)fminf(fmaxf(floorf(v), -1.0f), (float)limit); }
PB_DEV int sideHi(float v, int limit) { return (int)fminf(fmaxf(ceilf(v), -1.0f), (float)limit); }

struct Rgb3 {
  uint32_t a, b, c;
};

__global__ __launch_bounds__(256) void k_render_resolve(const PbDevParams *__restrict__ params, uint32_t member,
                                                        PbRenderParams V, const uint32_t *__restrict__ ids,
                                                        const uint32_t *__restrict__ rgb8, uint32_t pixels,
                                                        Rgb3 *__restrict__ out) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  const uint32_t p0 = t * 4u;
  if (p0 >= pixels) return;
  const PbDevParams &P = params[member];
  const uint32_t W = (uint32_t)V.width;
  int yy = (int)(p0 / W), xx = (int)(p0 - (uint32_t)yy * W);
  uint32_t px[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    uint32_t c = packRgb(245u, 245u, 245u);
    const uint32_t p = p0 + (uint32_t)j;
    const uint32_t id = p < pixels ? ids[p] : 0u;
    if (id == KEY_TRAIL) {
      c = packRgb(255u, 0u, 0u);
    } else if (id) {
      c = rgb8[id - 1u];
    } else if (p < pixels) {
      for (int k = 0; k < P.nobstacles; k++) {  // rectangles, x mirrored: x2 is the left edge
        const int xa = sideLo(viewX(V, P.x2obs[k]), V.width), xb = sideHi(viewX(V, P.x1obs[k]), V.width);
        const int ya = sideLo(viewY(V, P.y2obs[k]), V.height), yb = sideHi(viewY(V, P.y1obs[k]), V.height);
        if (xx >= xa && xx <= xb && yy >= ya && yy <= yb) c = packRgb(110u, 110u, 110u);
      }
      for (int k = 0; k < P.n_cir; k++)
        if (discCovers(pixDisc(V, P.xc[k], P.yc[k], P.rc[k]), xx, yy)) c = packRgb(110u, 110u, 110u);
      if (discCovers(pixDisc(V, P.light_x, P.light_y, V.lightRadius), xx, yy)) c = packRgb(250u, 210u, 40u);
    }
    px[j] = c;
    if (++xx == V.width) xx = 0, yy++;
  }
  // four RGB pixels in three dwords (the buffer is padded to whole groups of four)
  Rgb3 o;
  o.a = px[0] | (px[1] << 24);
  o.b = (px[1] >> 8) | (px[2] << 16);
  o.c = (px[2] >> 16) | (px[3] << 8);
  out[t] = o;
}

inline uint32_t blocksFor(uint64_t threads) { return (uint32_t)((threads + 255u) / 256u); }

// lanes per disc from its radius in pixels: a few pixels are one lane's work, a large disc is a wave's
inline int lanesFor(float radiusPixels) {
  if (!(radiusPixels > 2.0f)) return 1;
  return radiusPixels > 16.0f ? 64 : 8;
}

}  // namespace

void pbLaunchRenderBots(const PbDevParams *params, uint32_t member, const PbRenderParams &V, float maxRadius,
                        const float4 *pr, const int *dead, const uint32_t *orig, uint32_t n, uint32_t *ids,
                        uint32_t *rgb8, hipStream_t stream) {
  const int lanes = lanesFor(maxRadius * V.scale);
  const dim3 grid(blocksFor((uint64_t)n * (uint64_t)lanes)), block(256);
  if (lanes == 1)
    hipLaunchKernelGGL(k_render_bots<1>, grid, block, 0, stream, params, member, V, pr, dead, orig, n, ids, rgb8);
  else if (lanes == 8)
    hipLaunchKernelGGL(k_render_bots<8>, grid, block, 0, stream, params, member, V, pr, dead, orig, n, ids, rgb8);
  else
    hipLaunchKernelGGL(k_render_bots<64>, grid, block, 0, stream, params, member, V, pr, dead, orig, n, ids, rgb8);
}

void pbLaunchRenderTrail(const PbRenderParams &V, const float2 *ring, uint32_t slots, float radius, uint32_t *ids,
                         hipStream_t stream) {
  const int lanes = lanesFor(radius * V.scale);
  const dim3 grid(blocksFor((uint64_t)slots * (uint64_t)lanes)), block(256);
  if (lanes == 1)
    hipLaunchKernelGGL(k_render_trail<1>, grid, block, 0, stream, V, ring, slots, radius, ids);
  else if (lanes == 8)
    hipLaunchKernelGGL(k_render_trail<8>, grid, block, 0, stream, V, ring, slots, radius, ids);
  else
    hipLaunchKernelGGL(k_render_trail<64>, grid, block, 0, stream, V, ring, slots, radius, ids);
}

void pbLaunchRenderResolve(const PbDevParams *params, uint32_t member, const PbRenderParams &V, const uint32_t *ids,
                           const uint32_t *rgb8, uint32_t pixels, uint32_t *out, hipStream_t stream) {
  hipLaunchKernelGGL(k_render_resolve, dim3(blocksFor(((uint64_t)pixels + 3u) / 4u)), dim3(256), 0, stream, params, member,
                     V, ids, rgb8, pixels, (Rgb3 *)out);
}
