// pb_structure.hip -- structure analysis on gfx950: radial pair counts and the hexatic order psi6 of every member, from
// the engine's resident state (pbSimRadialCounts / pbSimStructureStats / pbSimHexaticOf, include/particlebot_hip.h has
// the definitions).
//
// The front end is the cluster analysis' (pbClusterFile, pb_cluster.hip): the bots filed afresh on a wrapped
// power-of-two grid, the sorted posrad array, dense cell starts.  Every entry point re-files with the edge it needs.
// On top of it, for the whole batch at once:
//   k_struct_rdf      the hot path.  Grid edge rMax (1 + 2^-10): a counted pair is never further apart than one cell.
//                     One bot per lane over the nine cells (pbWalkNine, pb_cluster.hpp).  Every unordered pair is met
//                     from both ends; it is counted by the end with the smaller sorted slot, as 2: the walk is the one
//                     that starts each range behind the own slot.  Bins go into the workgroup's LDS histogram (32-bit
//                     counters, LDS atomics), which is flushed once into the member's 64-bit counters with vector
//                     atomics, zeros skipped.  blockIdx.y is the member, so a workgroup's histogram belongs to one
//                     member.
//   k_struct_psi6     on the cluster analysis' grid, the same walk and the link rule (pbWhenLinked) without the
//                     union-find:
//                     per bot the neighbour count and the two fixed-point sums in registers, written in ORIGINAL order;
//                     the member's row reduced with wave shuffles and ballots, LDS, one set of integer atomics per
//                     workgroup (as k_cluster_reduce)
//   k_struct_hexatic  one member's sums into doubles
// Everything that is added is an integer: nothing depends on the order of the adds.  No float atomics, no scratch
// memory.
#include <string.h>

#include <cmath>

#include "pb_cluster.hpp"

static_assert(sizeof(pbStructureStats) == 56, "a member's row is 56 bytes");
static_assert(PB_RADIAL_MAX_BINS * sizeof(uint32_t) == 16384, "the LDS histogram is 16 KB");

namespace {

// A lane sends at most this many adds of 2 into the LDS histogram and adds the rest straight to the global counters:
// 256 lanes x 2^22 x 2 = 2^31, so no 32-bit LDS counter can wrap whatever the member holds -- the all-coincident pile
// folded into one cell (up to 2^28 - 1 partners per bot) included.
constexpr uint32_t LDS_ADDS_PER_LANE = 1u << 22;

__global__ __launch_bounds__(CT) void k_struct_rdf(const float4 *__restrict__ cpr, const uint32_t *__restrict__ start,
                                                   uint32_t n, ClusterGrid G, float scale, float d2max, uint32_t bins,
                                                   unsigned long long *__restrict__ counts) {
  __shared__ uint32_t hist[PB_RADIAL_MAX_BINS];
  for (uint32_t b = threadIdx.x; b < bins; b += CT) hist[b] = 0u;
  __syncthreads();
  unsigned long long *__restrict__ mine = counts + (size_t)blockIdx.y * bins;
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  const uint32_t t = blockIdx.y * n + (l < n ? l : 0u);
  float4 me = cpr[t];
  if (l >= n) me.x = __builtin_nanf("");  // (no early return: every lane meets the barriers)
  if (me.x == me.x) {  // a bot with a non-finite position or radius is in no pair
    const float fbins = (float)bins;
    uint32_t ldsAdds = 0u;
    // Cheap rejection in front of the correctly rounded root.  A counted pair has fl(dist * scale) < bins, hence
    // dist * scale < bins exactly (rounding is monotone, bins is a float), dist < bins / scale <= rMax (1 + 2^-23) for a
    // normal scale = fl(bins / rMax), sqrt(d2) <= dist (1 + 2^-23) and d2 < fl(rMax * rMax) (1 + 2^-20): d2max =
    // rMax * rMax * 1.0001f + 1e-30f (host, fp32) admits every such pair -- the absolute term where rMax * rMax is
    // subnormal, infinity where it overflows or scale is subnormal; with an infinite scale nothing is counted at all.
    // Whatever else it admits the exact rule decides.
    pbWalkNine<true>(cpr, start, blockIdx.y, G, t, me, [&](uint32_t, const float4 &, float, float, float d2) {
      if (d2 <= d2max) {  // (false for a non-finite partner: its position is NaN)
        const float fb = sqrtf(d2) * scale;
        if (fb < fbins) {
          const uint32_t b = (uint32_t)(int)fb;
          if (ldsAdds < LDS_ADDS_PER_LANE) {
            ldsAdds++;
            __hip_atomic_fetch_add(hist + b, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          } else {
            __hip_atomic_fetch_add(mine + b, 2ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
    });
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < bins; b += CT) {
    const uint32_t v = hist[b];
    if (v) __hip_atomic_fetch_add(mine + b, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// rint(v * 2^30) as an integer: |v| is a product of unit-vector components, at most a few ulps above 1, so the value
// fits 32 bits; v_rndne_f32 rounds to nearest even
PB_DEV long long fixed30(float v) { return (long long)(int)__builtin_rintf(v * 1073741824.0f); }

__global__ __launch_bounds__(CT) void k_struct_psi6(const float4 *__restrict__ cpr, const uint32_t *__restrict__ start,
                                                    uint32_t n, ClusterGrid G, float gap, long long *__restrict__ sRe,
                                                    long long *__restrict__ sIm, uint32_t *__restrict__ sNb,
                                                    pbStructureStats *__restrict__ rows) {
  __shared__ unsigned long long sBonds[CT / 64], sSumRe[CT / 64], sSumIm[CT / 64];
  __shared__ uint32_t sCoord[CT / 64][8];
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  const bool live = l < n;
  const uint32_t t = blockIdx.y * n + (live ? l : 0u);
  const float4 me = cpr[t];
  uint32_t deg = 0u;
  long long re = 0ll, im = 0ll;
  if (live && me.x == me.x) {  // a bot with a non-finite position or radius has no bonds
    pbWalkNine<false>(cpr, start, blockIdx.y, G, t, me, [&](uint32_t j, const float4 &q, float rx, float ry, float d2) {
      pbWhenLinked(t, me, j, q, d2, gap, [&](float dist, float) {
        deg++;
        if (dist > 0.0f) {
          const float ux = rx / dist, uy = ry / dist;
          const float c2 = ux * ux - uy * uy, s2 = (ux * uy) + (ux * uy);
          const float c4 = c2 * c2 - s2 * s2, s4 = (c2 * s2) + (c2 * s2);
          const float c6 = c4 * c2 - s4 * s2, s6 = s4 * c2 + c4 * s2;
          re += fixed30(c6);
          im += fixed30(s6);
        }
      });
    });
  }
  if (live) {
    const uint32_t o = __float_as_uint(me.w);
    sRe[o] = re, sIm[o] = im, sNb[o] = deg;
  }
  // the member's row: sums over the wave, the four waves through LDS, one set of atomics per workgroup
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const unsigned long long bonds = waveSumU64(deg);
  const unsigned long long sumRe = waveSumU64((unsigned long long)re), sumIm = waveSumU64((unsigned long long)im);
  const uint32_t cls = live ? (deg < 7u ? deg : 7u) : 8u;
#pragma unroll
  for (uint32_t k = 0; k < 8u; k++) {
    const uint32_t cnt = (uint32_t)__popcll(__ballot(cls == k));
    if (lane == 0u) sCoord[w][k] = cnt;
  }
  if (lane == 0u) sBonds[w] = bonds, sSumRe[w] = sumRe, sSumIm[w] = sumIm;
  __syncthreads();
  pbStructureStats *row = rows + blockIdx.y;
  if (threadIdx.x < 8u) {
    uint32_t c = 0u;
    for (int k = 0; k < CT / 64; k++) c += sCoord[k][threadIdx.x];
    if (c) atomicAdd(&row->coordination[threadIdx.x], c);
  } else if (threadIdx.x == 64u) {
    unsigned long long b = 0ull, r = 0ull, i = 0ull;
    for (int k = 0; k < CT / 64; k++) b += sBonds[k], r += sSumRe[k], i += sSumIm[k];
    if (b) {  // (no bonds: both sums are zero)
      atomicAdd(&row->bonds, b);
      atomicAdd((unsigned long long *)&row->psi6_re, r);  // two's complement: the signed sum modulo 2^64
      atomicAdd((unsigned long long *)&row->psi6_im, i);
    }
  }
}

__global__ __launch_bounds__(CT) void k_struct_hexatic(const long long *__restrict__ sRe, const long long *__restrict__ sIm,
                                                       const uint32_t *__restrict__ sNb, uint32_t base, uint32_t n,
                                                       double *__restrict__ psi) {
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  if (l >= n) return;
  const uint32_t nb = sNb[base + l];
  double re = 0.0, im = 0.0;
  if (nb) {
    re = ((double)sRe[base + l] / 1073741824.0) / (double)nb;
    im = ((double)sIm[base + l] / 1073741824.0) / (double)nb;
  }
  psi[2u * l] = re;
  psi[2u * l + 1u] = im;
}

int endOfAnalysis(pbSim *S) { return pbClockStop(S, S->cluster->structureClock); }

// files the bots on the cluster analysis' grid and leaves every bot's sums and every member's row on the device
int hexaticSweep(pbSim *S, float gap) {
  const int rc = pbClusterFile(S, (double)gap, 2.0);
  if (rc != PB_OK) return rc;
  PbClusterScratch *C = S->cluster;
  const ClusterGrid G = gridOf(C);
  const size_t total = S->total;  // (each on its own: a failed allocation leaves the rest to the next call)
  PB_TRY(C->sRe.ensure(total));
  PB_TRY(C->sIm.ensure(total));
  PB_TRY(C->sNb.ensure(total));
  PB_TRY(C->sRows.ensure(S->nsims));
  PB_TRY(C->sPsi.ensure(2 * (size_t)S->n));
  PB_TRY(hipMemsetAsync(C->sRows, 0, sizeof(pbStructureStats) * S->nsims, S->stream));
  hipLaunchKernelGGL(k_struct_psi6, dim3(cdiv(S->n, CT), S->nsims), dim3(CT), 0, S->stream, C->cpr, C->start, S->n, G,
                     gap, C->sRe, C->sIm, C->sNb, C->sRows);
  PB_TRY(hipGetLastError());
  return PB_OK;
}

}  // namespace

int pbSimRadialCounts(pbSim *S, float rMax, unsigned bins, unsigned long long *counts) {
  if (!S || !counts) return pbFail("pbSimRadialCounts", ": null handle or counts");
  if (!(rMax > 0.0f) || !(rMax < __builtin_inff())) return pbFail("pbSimRadialCounts", ": rMax must be finite and > 0");
  if (bins < 1u || bins > PB_RADIAL_MAX_BINS) return pbFail("pbSimRadialCounts", ": bins must be 1 ... 4096");
  int rc = pbClusterCheckArgs("pbSimRadialCounts", S, nullptr, nullptr);
  if (rc != PB_OK) return rc;
  rc = pbClusterFile(S, (double)rMax, 0.0);
  if (rc != PB_OK) return rc;
  PbClusterScratch *C = S->cluster;
  const ClusterGrid G = gridOf(C);
  PB_TRY(C->sCounts.ensure((size_t)S->nsims * bins));  // (grows with bins: the members of a batch are fixed)
  const size_t bytes = sizeof(unsigned long long) * (size_t)S->nsims * bins;
  const float scale = (float)bins / rMax;
  const float d2max = rMax * rMax * 1.0001f + 1e-30f;
  PB_TRY(hipMemsetAsync(C->sCounts, 0, bytes, S->stream));
  hipLaunchKernelGGL(k_struct_rdf, dim3(cdiv(S->n, CT), S->nsims), dim3(CT), 0, S->stream, C->cpr, C->start, S->n, G,
                     scale, d2max, bins, C->sCounts);
  PB_TRY(hipGetLastError());
  rc = endOfAnalysis(S);
  if (rc != PB_OK) return rc;
  PB_TRY(hipMemcpy(counts, C->sCounts, bytes, hipMemcpyDeviceToHost));
  return PB_OK;
}

int pbSimStructureStats(pbSim *S, float linkGap, pbStructureStats *rows) {
  if (!S || !rows) return pbFail("pbSimStructureStats", ": null handle or rows");
  int rc = pbClusterCheckArgs("pbSimStructureStats", S, &linkGap, nullptr);
  if (rc != PB_OK) return rc;
  rc = hexaticSweep(S, linkGap);
  if (rc == PB_OK) rc = endOfAnalysis(S);
  if (rc != PB_OK) return rc;
  PB_TRY(hipMemcpy(rows, S->cluster->sRows, sizeof(pbStructureStats) * S->nsims, hipMemcpyDeviceToHost));
  return PB_OK;
}

int pbSimHexaticOf(pbSim *S, unsigned member, float linkGap, double *psi6, unsigned *neighbours) {
  if (!S) return pbFail("pbSimHexaticOf", ": null handle");
  if (!psi6 && !neighbours) return pbFail("pbSimHexaticOf", ": psi6 and neighbours are both null");
  int rc = pbClusterCheckArgs("pbSimHexaticOf", S, &linkGap, &member);
  if (rc != PB_OK) return rc;
  rc = hexaticSweep(S, linkGap);
  if (rc != PB_OK) return rc;
  PbClusterScratch *C = S->cluster;
  const uint32_t n = S->n, base = member * n;
  if (psi6) {
    hipLaunchKernelGGL(k_struct_hexatic, dim3(cdiv(n, CT)), dim3(CT), 0, S->stream, C->sRe, C->sIm, C->sNb, base, n,
                       C->sPsi);
    PB_TRY(hipGetLastError());
  }
  rc = endOfAnalysis(S);
  if (rc != PB_OK) return rc;
  if (psi6) PB_TRY(hipMemcpyAsync(psi6, C->sPsi, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, S->stream));
  if (neighbours)
    PB_TRY(hipMemcpyAsync(neighbours, C->sNb + base, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, S->stream));
  PB_TRY(hipStreamSynchronize(S->stream));
  return PB_OK;
}

int pbSimGetStructureTimes(pbSim *S, unsigned long long *analyses, float *last_device_ms) {
  return pbClockGet("pbSimGetStructureTimes", S, &PbClusterScratch::structureClock, analyses, last_device_ms);
}
