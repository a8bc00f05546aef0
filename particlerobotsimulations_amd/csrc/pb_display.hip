// pb_display.hip -- the reference's two display kernels on gfx950: the bot colours (updateCol_k,
// particlebot_kernel_impl.cuh:351-443) and the centroid trail (calcCOG / calcCOG1, impl.cuh:295-349, driven by
// particlebot_cuda.cu:241-281).  Neither changes the dynamics; both are bit-identical to the reference's text.
//
// Used by the `extern "C"` seam (updateCol / calcCOG, pb_legacy.hip) and by the resident engine
// (pbSimGetColorsOf, pbSimSetCentroidTrail / pbSimGetCentroidTrailOf, the trail record of stepMany).
#include "pb_colour.hpp"
#include "pb_device.hpp"
#include "pb_internal.hpp"

namespace {

inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// the reference's kernel: caller's arrays in original order, alpha left as it is
__global__ __launch_bounds__(256) void k_update_col(PbDevParams P, uint32_t displayShadow, const float *__restrict__ rad,
                                                    float4 *__restrict__ col, const float2 *__restrict__ pos,
                                                    const int *__restrict__ dead, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float2 p = pos[i];
  col[i] = pbBotColour(P, displayShadow, p.x, p.y, rad[i], dead[i], col[i]);
}

// the engine's: one member's cell-sorted slots, colours written in original order with the reference's alpha fill
__global__ __launch_bounds__(256) void k_engine_col(const PbDevParams *__restrict__ params, uint32_t member,
                                                     uint32_t displayShadow, const float4 *__restrict__ pr,
                                                     const int *__restrict__ dead, const uint32_t *__restrict__ orig,
                                                     uint32_t n, float4 *__restrict__ out) {
  const uint32_t l = blockIdx.x * 256u + threadIdx.x;
  if (l >= n) return;
  const size_t s = (size_t)member * n + l;
  const float4 q = pr[s];
  out[orig[s]] = pbBotColour(params[member], displayShadow, q.x, q.y, q.z, dead[s], make_float4(0, 0, 0, 1.0f));
}

// ---- centroid (impl.cuh:295-349) ----------------------------------------------------------------------------
// One level of the reference's tree: each 64-value block b of a member's m inputs becomes one sum.  Lane t starts from
// 0.0f + v[64b + t] (0.0f past the end: the add turns -0.0f into +0.0f) and the lanes combine as s[t] += s[t + k] for
// k = 32 ... 1; lane 0 holds the reference's sdata[0].  A 64-wide wave is one reference block, four per workgroup.
// LAST: the level whose one block is the whole input (calcCOG1): times mul = 1/n, plus the shader's 2000 on y, into
// dst[member * dstStride].
template <bool LAST>
__global__ __launch_bounds__(256) void k_cog_level(const float2 *__restrict__ in, size_t inStride, uint32_t m,
                                                   float2 *__restrict__ out, size_t outStride, float mul) {
  const uint32_t t = threadIdx.x & 63u;
  const uint32_t blk = blockIdx.x * 4u + (threadIdx.x >> 6);
  const uint32_t i = blk * 64u + t;  // < 2^32: m <= 2^32 - 32 bots per member (pbSimCreateBatch)
  const float2 *src = in + (size_t)blockIdx.y * inStride;
  float sx = 0.0f, sy = 0.0f;
  if (i < m) {
    const float2 v = src[i];
    sx = sx + v.x;
    sy = sy + v.y;
  }
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) {
    const float ox = __shfl_down(sx, k, 64), oy = __shfl_down(sy, k, 64);
    sx = sx + ox;
    sy = sy + oy;
  }
  if (t != 0u || blk * 64u >= m) return;
  float2 r;
  if (LAST) {
    r.x = sx * mul;
    r.y = sy * mul;
    r.y = r.y + 2000.0f;
  } else {
    r = make_float2(sx, sy);
  }
  out[(size_t)blockIdx.y * outStride + (LAST ? 0u : blk)] = r;
}

}  // namespace

// ---- launchers (declared in pb_internal.hpp) --------------------------------------------------------------

void pbLaunchUpdateCol(const PbDevParams &P, uint32_t displayShadow, const float *rad, float *col, const float *pos,
                       const int *dead, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_update_col, dim3(cdiv(n, 256)), dim3(256), 0, stream, P, displayShadow, rad, (float4 *)col,
                     (const float2 *)pos, dead, n);
}

void pbLaunchCentroid(const float *pos, size_t posStride, uint32_t n, float *tmp0, float *tmp1, size_t tmpStride,
                      float *dst, size_t dstStride, uint32_t members, hipStream_t stream) {
  // the host driver of particlebot_cuda.cu:241-281: levels on the block sums until one block remains, without a copy
  // back between levels (the two temporaries alternate) and without a host synchronisation
  const float mul = 1.0f / (float)n;
  const float2 *src = (const float2 *)pos;
  size_t srcStride = posStride;
  float2 *buf[2] = {(float2 *)tmp0, (float2 *)tmp1};
  int w = 0;
  uint32_t m = n;
  for (;;) {
    const uint32_t blocks = cdiv(m, 64);
    const dim3 grid(cdiv(blocks, 4), members);
    if (blocks == 1) {
      hipLaunchKernelGGL(k_cog_level<true>, grid, dim3(256), 0, stream, src, srcStride, m, (float2 *)dst, dstStride,
                         mul);
      return;
    }
    hipLaunchKernelGGL(k_cog_level<false>, grid, dim3(256), 0, stream, src, srcStride, m, buf[w], tmpStride, mul);
    src = buf[w];
    srcStride = tmpStride;
    m = blocks;
    w ^= 1;
  }
}

void pbLaunchEngineColors(const PbDevParams *params, uint32_t member, uint32_t displayShadow, const float4 *pr,
                          const int *dead, const uint32_t *orig, uint32_t n, float4 *out, hipStream_t stream) {
  hipLaunchKernelGGL(k_engine_col, dim3(cdiv(n, 256)), dim3(256), 0, stream, params, member, displayShadow, pr, dead, orig, n,
                     out);
}
