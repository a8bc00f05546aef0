// pb_correlate.hip -- pair correlations on gfx950: every member's pairs binned by distance, with the sum of the dot
// products a_i . a_j of a per-bot integer vector per bin (pbSimPairCorrelation, include/particlebot_hip.h has the
// definitions).
//
// The front end is the cluster analysis' (pbClusterFile, pb_cluster.hip): the bots filed afresh on a wrapped
// power-of-two grid of edge rMax (1 + 2^-10), the sorted posrad array, dense cell starts.  On top of it, for the whole
// batch at once (blockIdx.y is the member):
//   k_corr_gather  per sorted slot the vector a as one int2, x = INT_MIN for a bot that is not measured (a measured
//                  component has |.| <= 2^31 - 128).  Velocities come through the sorted slots from the state arrays, as
//                  k_contact_gather_vel reads them; displacements from the marked positions through the original index
//                  in cpr.w; the radius from cpr.z.  The member's totals row is reduced with wave shuffles, the four waves
//                  through LDS, one set of integer atomics per workgroup.
//   k_corr_sweep   the hot path: the radial sweep's walk, bin rule and cheap rejection (k_struct_rdf, pb_structure.hip),
//                  one bot per lane over the nine cells, a pair met once from the lower sorted slot and entered for both
//                  of its orders.  Per counted pair five 64-bit LDS atomics into the workgroup's table (5 words x bins,
//                  at most 40 KB, sized by bins at the launch): pairs += 2, 2 lo32(d), 2 (d >> 32), ax_i + ax_j,
//                  ay_i + ay_j with d = ax_i ax_j + ay_i ay_j.  One flush per workgroup into the member's global words,
//                  zeros skipped, every partial but the count split into its low 32 bits and the rest.
// The host composes the words into 128-bit integers and normalises them (0 <= lo < 2^32, hi the floor quotient).
//
// EXACTNESS.  Everything that is added is an integer modulo 2^64, so nothing depends on the order of the adds; what is
// left to show is that no word wraps.  pairs: a member holds fewer than 2^28 bots, hence fewer than 2^56 ordered pairs:
// the LDS word and the global word hold the count whatever the state is.  The other words, for a bin that holds P < 2^31
// ordered pairs of its member (any workgroup's share is at most that): by pb_fixed.hpp's bound |d| < 2^63,
// 0 <= lo32(d) < 2^32 and |d >> 32| <= 2^31.  The LDS word of the low halves stays below P 2^32 < 2^63; the signed words
// (high halves, ax, ay) stay within P 2^31 <= 2^62 in magnitude, which two's complement holds.  A flush adds a low part
// below 2^32 and a rest within 2^31 in magnitude; a member has at most 2^20 workgroups, so the global words stay within
// 2^52.  The call reads the counts it is about to return and refuses the answer when a bin holds 2^31 ordered pairs or
// more.  No float atomics, no 128-bit atomics, no scratch memory.
#include <limits.h>

#include <vector>

#include "pb_cluster.hpp"

static_assert(sizeof(pbCorrelationBin) == 56, "a bin's row is 56 bytes");
static_assert(sizeof(pbCorrelationTotals) == 48, "a member's totals row is 48 bytes");
static_assert(PB_CORR_MAX_BINS * 5 * sizeof(unsigned long long) == 40960, "the LDS table is at most 40 KB");

namespace {

// the words of the workgroup's table and of a member's totals
enum { T_PAIRS, T_DLO, T_DHI, T_AX, T_AY, T_WORDS };
enum { S_MEASURED, S_AX, S_AY, S_A2LO, S_A2HI, S_WORDS };
// the global words of one bin: the count, then low 32 bits and rest of each of the table's other four words
constexpr uint32_t G_WORDS = 9;

__global__ __launch_bounds__(CT) void k_corr_gather(const float4 *__restrict__ cpr,
                                                    const uint32_t *__restrict__ sortedSlots,
                                                    const float2 *__restrict__ vel, const float2 *__restrict__ pos0,
                                                    uint32_t n, int kind, int2 *__restrict__ a,
                                                    unsigned long long *__restrict__ totals) {
  __shared__ unsigned long long sRed[CT / 64][S_WORDS];
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  const bool live = l < n;
  const uint32_t t = blockIdx.y * n + (live ? l : 0u);
  const float4 me = cpr[t];
  float fx = __builtin_nanf(""), fy = 0.0f;
  if (live && me.x == me.x) {  // a bot with a non-finite position or radius is no node
    if (kind == PB_CORR_VELOCITY) {
      const float2 v = vel[sortedSlots[t]];  // keys carry the member: the slot is one of this member's
      fx = v.x, fy = v.y;
    } else if (kind == PB_CORR_DISPLACEMENT) {
      const float2 p0 = pos0[__float_as_uint(me.w)];
      fx = me.x - p0.x, fy = me.y - p0.y;
    } else {
      fx = me.z;
    }
  }
  // an f in range is finite, and for a displacement both of its coordinates are
  const bool measured = pbFixedInRange(fx) && pbFixedInRange(fy);
  long long qx = 0ll, qy = 0ll;
  unsigned long long s = 0ull;
  if (measured) {
    qx = pbFixedQuantise(fx), qy = pbFixedQuantise(fy);
    s = (unsigned long long)(qx * qx) + (unsigned long long)(qy * qy);
  }
  if (live) a[t] = make_int2(measured ? (int)qx : INT_MIN, (int)qy);
  // the member's totals: sums over the wave, the four waves through LDS, one set of atomics per workgroup
  unsigned long long r[S_WORDS], v;
  r[S_MEASURED] = __popcll(__ballot(measured));
  r[S_AX] = waveSumU64((unsigned long long)qx), r[S_AY] = waveSumU64((unsigned long long)qy);
  r[S_A2LO] = waveSumU64(pbFixedLow(s)), r[S_A2HI] = waveSumU64(pbFixedRest(s));
  if (blockFold(sRed, r, [](uint32_t) { return PB_FOLD_SUM; }, v)) {
    // (two's complement: a signed sum modulo 2^64; one that is zero adds nothing either)
    if (v) atomicAdd(totals + (size_t)blockIdx.y * S_WORDS + threadIdx.x, v);
  }
}

__global__ __launch_bounds__(CT) void k_corr_sweep(const float4 *__restrict__ cpr, const uint32_t *__restrict__ start,
                                                   const int2 *__restrict__ a, uint32_t n, ClusterGrid G, float scale,
                                                   float d2max, uint32_t bins, unsigned long long *__restrict__ acc) {
  extern __shared__ unsigned long long tab[];  // T_WORDS x bins, word-major
  const uint32_t words = (uint32_t)T_WORDS * bins;
  for (uint32_t k = threadIdx.x; k < words; k += CT) tab[k] = 0ull;
  __syncthreads();
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  const uint32_t t = blockIdx.y * n + (l < n ? l : 0u);
  float4 me = cpr[t];
  const int2 mine = a[t];
  if (l >= n) me.x = __builtin_nanf("");  // (no early return: every lane meets the barriers)
  if (me.x == me.x && mine.x != INT_MIN) {  // an unmeasured bot is in no pair
    const float fbins = (float)bins;
    // the radial sweep's rejection in front of the correctly rounded root and its bin rule (k_struct_rdf has the
    // argument for d2max); the partner's vector is requested ahead of both
    pbWalkNine<true>(cpr, start, blockIdx.y, G, t, me, [&](uint32_t j, const float4 &, float, float, float d2) {
      const int2 other = a[j];
      if (d2 <= d2max) {  // (false for a non-finite partner: its position is NaN)
        const float fb = sqrtf(d2) * scale;
        if (fb < fbins && other.x != INT_MIN) {
          const uint32_t b = (uint32_t)(int)fb;
          const long long d = (long long)mine.x * (long long)other.x + (long long)mine.y * (long long)other.y;
          const unsigned long long dlo = ((unsigned long long)d & 0xFFFFFFFFull) << 1;
          const unsigned long long dhi = (unsigned long long)((d >> 32) * 2ll);
          const unsigned long long sx = (unsigned long long)((long long)mine.x + (long long)other.x);
          const unsigned long long sy = (unsigned long long)((long long)mine.y + (long long)other.y);
          __hip_atomic_fetch_add(tab + T_PAIRS * bins + b, 2ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(tab + T_DLO * bins + b, dlo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(tab + T_DHI * bins + b, dhi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(tab + T_AX * bins + b, sx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(tab + T_AY * bins + b, sy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    });
  }
  __syncthreads();
  unsigned long long *__restrict__ mineAcc = acc + (size_t)blockIdx.y * bins * G_WORDS;
  for (uint32_t k = threadIdx.x; k < words; k += CT) {
    const unsigned long long v = tab[k];
    if (!v) continue;
    const uint32_t word = k / bins, b = k - word * bins;
    unsigned long long *dst = mineAcc + (size_t)b * G_WORDS;
    if (word == (uint32_t)T_PAIRS) {
      __hip_atomic_fetch_add(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      // v = rest * 2^32 + low; the rest of a signed word is its arithmetic shift
      const unsigned long long low = v & 0xFFFFFFFFull;
      const unsigned long long rest = word == (uint32_t)T_DLO ? v >> 32 : (unsigned long long)((long long)v >> 32);
      dst += 2u * word - 1u;
      if (low) __hip_atomic_fetch_add(dst, low, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (rest) __hip_atomic_fetch_add(dst + 1, rest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace

int pbSimPairCorrelation(pbSim *S, int kind, float rMax, unsigned bins, pbCorrelationBin *rows,
                         pbCorrelationTotals *totals) {
  if (!S || !rows) return pbFail("pbSimPairCorrelation", ": null handle or rows");
  if (kind != PB_CORR_VELOCITY && kind != PB_CORR_DISPLACEMENT && kind != PB_CORR_RADIUS)
    return pbFail("pbSimPairCorrelation", ": unknown kind");
  if (!(rMax > 0.0f) || !(rMax < __builtin_inff()))
    return pbFail("pbSimPairCorrelation", ": rMax must be finite and > 0");
  if (bins < 1u || bins > PB_CORR_MAX_BINS) return pbFail("pbSimPairCorrelation", ": bins must be 1 ... 1024");
  int rc = pbClusterCheckArgs("pbSimPairCorrelation", S, nullptr, nullptr);
  if (rc != PB_OK) return rc;
  if (kind == PB_CORR_DISPLACEMENT && !(S->cluster && S->cluster->dMarked))  // known without the device
    return pbFail("pbSimPairCorrelation", ": no reference marked");
  rc = pbClusterFile(S, (double)rMax, 0.0);
  if (rc != PB_OK) return rc;
  PbClusterScratch *C = S->cluster;
  const ClusterGrid G = gridOf(C);
  const size_t nsims = S->nsims;
  PB_TRY(C->kA.ensure((size_t)S->total));
  PB_TRY(C->kTotals.ensure(nsims * S_WORDS));
  PB_TRY(C->kAcc.ensure(nsims * bins * G_WORDS));  // (grows with bins: the members of a batch are fixed)
  const size_t accWords = nsims * bins * G_WORDS, totWords = nsims * S_WORDS;
  const float scale = (float)bins / rMax;
  const float d2max = rMax * rMax * 1.0001f + 1e-30f;
  const dim3 b(CT), g(cdiv(S->n, CT), S->nsims);
  PB_TRY(hipMemsetAsync(C->kAcc, 0, sizeof(unsigned long long) * accWords, S->stream));
  PB_TRY(hipMemsetAsync(C->kTotals, 0, sizeof(unsigned long long) * totWords, S->stream));
  hipLaunchKernelGGL(k_corr_gather, g, b, 0, S->stream, C->cpr, C->vals[C->sortedIn], S->vel[S->cur],
                     kind == PB_CORR_DISPLACEMENT ? C->dPos0 : (const float2 *)nullptr, S->n, kind, C->kA, C->kTotals);
  hipLaunchKernelGGL(k_corr_sweep, g, b, sizeof(unsigned long long) * T_WORDS * bins, S->stream, C->cpr, C->start, C->kA,
                     S->n, G, scale, d2max, bins, C->kAcc);
  PB_TRY(hipGetLastError());
  rc = pbClockStop(S, C->correlateClock);
  if (rc != PB_OK) return rc;
  std::vector<unsigned long long> acc(accWords), tot(totWords);
  PB_TRY(hipMemcpy(acc.data(), C->kAcc, sizeof(unsigned long long) * accWords, hipMemcpyDeviceToHost));
  PB_TRY(hipMemcpy(tot.data(), C->kTotals, sizeof(unsigned long long) * totWords, hipMemcpyDeviceToHost));
  for (size_t k = 0; k < nsims * bins; k++)
    if (acc[k * G_WORDS] >= (1ull << 31))  // the counts are exact whatever the state: the other sums may not be
      return pbFail("pbSimPairCorrelation", ": a bin holds 2^31 pairs or more: raise bins or lower rMax");
  for (size_t m = 0; m < nsims; m++) {
    unsigned long long pairs = 0ull;
    for (size_t k = m * bins; k < (m + 1) * bins; k++) {
      const unsigned long long *w = &acc[k * G_WORDS];
      pbCorrelationBin &row = rows[k];
      row.pairs = w[0];
      row.dot = pbFixedNormalised(pbFixedCompose(w[1], w[2]) + pbFixedCompose(w[3], w[4]) * ((__int128)1 << 32));
      row.ax = pbFixedNormalised(pbFixedCompose(w[5], w[6]));
      row.ay = pbFixedNormalised(pbFixedCompose(w[7], w[8]));
      pairs += w[0];
    }
    if (totals) {
      const unsigned long long *w = &tot[m * S_WORDS];
      pbCorrelationTotals &out = totals[m];
      out.measured = (unsigned)w[S_MEASURED], out.reserved = 0u;
      out.sum_ax = (long long)w[S_AX], out.sum_ay = (long long)w[S_AY];
      out.sum_a2 = pbFixedNormalised(pbFixedCompose(w[S_A2LO], w[S_A2HI]));
      out.pairs = pairs;
    }
  }
  return PB_OK;
}

int pbSimGetCorrelationTimes(pbSim *S, unsigned long long *analyses, float *last_device_ms) {
  return pbClockGet("pbSimGetCorrelationTimes", S, &PbClusterScratch::correlateClock, analyses, last_device_ms);
}
