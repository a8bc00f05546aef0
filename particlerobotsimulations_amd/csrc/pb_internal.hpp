// pb_internal.hpp -- host-side declarations shared between the translation units of
// libparticlebot_hip.so (not part of the public C-ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- stable LSD radix sort of (key,value) pairs, 8 bits per pass (pb_sort.hip) ----------------
// Tile geometry of one sort workgroup.
constexpr int PB_SORT_THREADS = 256;
constexpr int PB_SORT_ITEMS = 8;
constexpr int PB_SORT_TILE = PB_SORT_THREADS * PB_SORT_ITEMS;

static inline uint32_t pbSortBlocks(uint32_t n) { return (n + PB_SORT_TILE - 1) / PB_SORT_TILE; }
// number of uint32 entries the histogram workspace needs for n pairs
// (the 256 x nblocks digit table, plus one sum per 2048-entry chunk of it for the scan)
static inline size_t pbSortHistEntries(uint32_t n) {
  const size_t table = (size_t)256 * (pbSortBlocks(n) ? pbSortBlocks(n) : 1);
  return table + (table + 2047) / 2048 + 1;
}

// Sorts n pairs by the low `bits` bits of the key; equal keys keep their input order (this is what
// thrust::sort_by_key gives the reference, particlebot_cuda.cu:377-382).  Buffers ping-pong; the
// return value is 0 when the result is in (keys, vals) and 1 when it is in (keys_tmp, vals_tmp).
// Returns -1 after recording a HIP error.
int pbRadixSortPairs(uint32_t *keys, uint32_t *vals, uint32_t *keys_tmp, uint32_t *vals_tmp,
                     uint32_t *hist, uint32_t n, int bits, hipStream_t stream, hipError_t *err);

static inline int pbKeyBits(uint32_t numKeys) {
  int b = 0;
  while (b < 32 && (numKeys > (1u << b))) b++;
  return b < 1 ? 1 : b;
}

// ---- XORWOW jump table (pb_xorwow.hpp) on the CURRENT device: built on the host once per process,
// uploaded once per device; returns nullptr and sets *err after a HIP error (pb_legacy.hip)
const uint32_t *pbXorwowDeviceTable(hipError_t *err);

// ---- the reference's display kernels (pb_display.hip); strides count float2 / float4 elements, n >= 1 ---------
struct PbDevParams;
// updateCol_k over caller arrays in original order: rgb of col[i] for i < n, alpha untouched
void pbLaunchUpdateCol(const PbDevParams &P, uint32_t displayShadow, const float *rad, float *col, const float *pos,
                       const int *dead, uint32_t n, hipStream_t stream);
// one member's colours from the engine's cell-sorted slots, written to out[orig] with alpha 1
void pbLaunchEngineColors(const PbDevParams *params, uint32_t member, uint32_t displayShadow, const float4 *pr,
                          const int *dead, const uint32_t *orig, uint32_t n, float4 *out, hipStream_t stream);
// calcCOG's tree for `members` inputs of n float2 each (member k at pos + 2 k posStride): the centroid, y + 2000, to
// dst + 2 k dstStride.  tmp0 / tmp1: scratch of ceil(n / 64) float2 per member (member k at + 2 k tmpStride)
void pbLaunchCentroid(const float *pos, size_t posStride, uint32_t n, float *tmp0, float *tmp1, size_t tmpStride,
                      float *dst, size_t dstStride, uint32_t members, hipStream_t stream);

// ---- the frame rasteriser (pb_render.hip) --------------------------------------------------------------------------
// One view, flattened on the host with the host writer's fp32 operations (Particlebot::writeFrame):
// scale = 0.5f * height / halfExtent, halfW = 0.5f * width, halfH = 0.5f * height.
struct PbRenderParams {
  int width, height;
  float centerX, centerY, scale, halfW, halfH;
  float lightRadius;
  int style;                // 0 plain, 1 reference (updateCol_k's colours)
  uint32_t displayShadow;   // the member's display_shadow (style 1)
};
// ids: one key per pixel, cleared by the caller; rgb8: n packed colours, written at [orig] for every bot that is drawn.
// maxRadius (world units) picks the lanes per bot.
void pbLaunchRenderBots(const PbDevParams *params, uint32_t member, const PbRenderParams &V, float maxRadius,
                        const float4 *pr, const int *dead, const uint32_t *orig, uint32_t n, uint32_t *ids,
                        uint32_t *rgb8, hipStream_t stream);
// the recorded slots of one member's centroid ring as discs of `radius` at (x, y - 2000), above every bot
void pbLaunchRenderTrail(const PbRenderParams &V, const float2 *ring, uint32_t slots, float radius, uint32_t *ids,
                         hipStream_t stream);
// keys -> packed RGB8 (3 * pixels bytes, `out` padded to a multiple of 12), the analytic items where no key is set
void pbLaunchRenderResolve(const PbDevParams *params, uint32_t member, const PbRenderParams &V, const uint32_t *ids,
                           const uint32_t *rgb8, uint32_t pixels, uint32_t *out, hipStream_t stream);
