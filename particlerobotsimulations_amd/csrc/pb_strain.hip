// pb_strain.hip -- local strain and non-affine displacement D2min on gfx950: the Falk-Langer fit of every bot's marked
// bond vectors onto its present ones (pbSimStrainStats / pbSimStrainOf, include/particlebot_hip.h has the definitions;
// pb_strain.hpp the fit).  The mark is the rearrangement analysis' (pb_dynamics.hip): its CSR in ORIGINAL order and its
// positions are on the device already, so nothing is filed and no grid is built.
//   k_dyn_scatter   (pb_dynamics.hip, pbDynamicsScatter) the present positions into ORIGINAL order, raw from the state
//                   arrays
//   k_strain_fit    one bot per lane.  The lane loads its share of the CSR and its own two positions, walks its list
//                   (the next entry's index is in flight while an entry's two positions are gathered), quantises the
//                   four bond components and accumulates the nine moments in registers, evaluates the fit and stores
//                   the moments and d2 in ORIGINAL order.  The members' rows are reduced as k_dyn_compare reduces its
//                   own: wave sums, the four waves through LDS, then one set of integer atomics per workgroup and member
//                   (a workgroup may straddle members).
// Lanes are dealt to bots in ORIGINAL order: the CSR share, the own positions and the stores are coalesced, the
// neighbours' positions are gathered.  PB_STRAIN_SORTED_LANES builds the other dealing, in the current sorted order (the
// gathers of a wave are closer together, everything else scatters), for a measurement of the two against each other.
// THE BOUND.  |q| <= 2^23 (pb_strain.hpp: a used component is below 8 in magnitude), a product of two is at most 2^46,
// W's term at most 2^47, and a list has fewer than 2^16 entries: every per-bot moment stays below 2^63.  A member's sums
// are added as the low 32 bits and the rest of every per-bot moment (pb_fixed.hpp's split): with fewer than 2^28 bots
// neither accumulator wraps.
// Everything that is added is an integer: nothing depends on the order of the adds.  No float atomics, no scratch
// memory, no private array.
#include <vector>

#include "pb_cluster.hpp"
#include "pb_strain.hpp"

static_assert(sizeof(pbStrainStats) == 184, "a member's row is 184 bytes");
static_assert(PB_STRAIN_MOMENTS == 9, "nine words per bot");

namespace {

// the columns of the row reduction: first the sums that ride one rolled butterfly (from T_SUMS on the nine pbMoment128 of
// the row, yxx ... w and sum_d2, low word and rest), then the ballots and the maximum
enum { T_USED, T_DROPPED, T_SUMS, T_COUNTS = T_SUMS + 18, T_FITTED = T_COUNTS, T_UNFITTED, T_ABOVE, T_MAX, T_COLS };

__global__ __launch_bounds__(CT) void k_strain_fit(const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ other,
                                                   const float2 *__restrict__ pos0, const float2 *__restrict__ pos1,
                                                   const uint32_t *__restrict__ orig, uint32_t n, uint32_t total,
                                                   double threshold, long long *__restrict__ moments,
                                                   double *__restrict__ d2min, pbStrainStats *__restrict__ rows) {
  __shared__ unsigned long long sRed[CT / 64][T_COLS];
  const uint32_t t0 = blockIdx.x * CT;
  const bool live = t0 + threadIdx.x < total;
  const uint32_t t = live ? t0 + threadIdx.x : total - 1u;
  const uint32_t member = t / n, base = member * n;  // a member's slots and its original indices are the same block
#ifdef PB_STRAIN_SORTED_LANES
  const uint32_t o = base + orig[t];
#else
  const uint32_t o = t;
#endif
  const uint32_t first = offsets[o], end = offsets[o + 1u];
  const float2 a0 = pos0[o], a1 = pos1[o];
  const uint32_t len = end - first;
  long long m[PB_STRAIN_MOMENTS];
#pragma unroll
  for (int c = 0; c < PB_STRAIN_MOMENTS; c++) m[c] = 0ll;
  uint32_t dropped = 0u;
  if (live && len < PB_STRAIN_MAX_LIST) {
    uint32_t jn = first < end ? other[first] : 0u;
#pragma unroll 1
    for (uint32_t e = first; e < end; e++) {
      const uint32_t j = base + jn;
      jn = e + 1u < end ? other[e + 1u] : 0u;  // (never past this bot's share of the entries)
      const float2 b0 = pos0[j], b1 = pos1[j];
      const float d0x = b0.x - a0.x, d0y = b0.y - a0.y, dx = b1.x - a1.x, dy = b1.y - a1.y;
      if (pbStrainInReach(d0x) && pbStrainInReach(d0y) && pbStrainInReach(dx) && pbStrainInReach(dy)) {
        const long long q0x = pbFixedQuantise(d0x), q0y = pbFixedQuantise(d0y);
        const long long qx = pbFixedQuantise(dx), qy = pbFixedQuantise(dy);
        m[PB_STRAIN_K] += 1ll;
        m[PB_STRAIN_YXX] += q0x * q0x, m[PB_STRAIN_YXY] += q0x * q0y, m[PB_STRAIN_YYY] += q0y * q0y;
        m[PB_STRAIN_XXX] += qx * q0x, m[PB_STRAIN_XXY] += qx * q0y;
        m[PB_STRAIN_XYX] += qy * q0x, m[PB_STRAIN_XYY] += qy * q0y;
        m[PB_STRAIN_W] += qx * qx + qy * qy;
      } else {
        dropped++;
      }
    }
  } else if (live) {
    dropped = len;
  }
  const PbStrainFit f = pbStrainFit(m);
  const unsigned long long e2 = f.fitted ? pbStrainUnits(f.d2) : 0ull;
  if (live) {
    long long *mine = moments + (size_t)o * PB_STRAIN_MOMENTS;
#pragma unroll
    for (int c = 0; c < PB_STRAIN_MOMENTS; c++) mine[c] = m[c];
    d2min[o] = f.d2;
  }
  // the members' rows: per member the sums over each wave, the four waves through LDS, one set of atomics
  const uint32_t tLast = (total - t0 < (uint32_t)CT ? total : t0 + CT) - 1u;
  const uint32_t mFirst = t0 / n, mLast = tLast / n;
#pragma unroll 1
  for (uint32_t mb = mFirst; mb <= mLast; mb++) {
    const bool mine = live && member == mb;
    const bool fit = mine && f.fitted;
    unsigned long long r[T_COLS], sums[T_COUNTS], v;
    sums[T_USED] = mine ? (unsigned long long)m[PB_STRAIN_K] : 0ull;
    sums[T_DROPPED] = mine ? dropped : 0u;
#pragma unroll
    for (int c = 0; c < 8; c++) {  // (an unused bot's moments are zero)
      sums[T_SUMS + 2 * c] = mine ? pbFixedLow(m[PB_STRAIN_YXX + c]) : 0ull;
      sums[T_SUMS + 2 * c + 1] = mine ? pbFixedRest(m[PB_STRAIN_YXX + c]) : 0ull;
    }
    sums[T_SUMS + 16] = fit ? pbFixedLow(e2) : 0ull;
    sums[T_SUMS + 17] = fit ? pbFixedRest(e2) : 0ull;
    unsigned long long mx = fit ? e2 : 0ull;
    waveSumRolled(sums, [&](int stage) {  // one butterfly stage in the code: twenty sums and the maximum
      const unsigned long long u = shflXor64(mx, stage);
      mx = u > mx ? u : mx;
    });
#pragma unroll
    for (int c = 0; c < T_COUNTS; c++) r[c] = sums[c];
    r[T_FITTED] = __popcll(__ballot(fit));
    r[T_UNFITTED] = __popcll(__ballot(mine && !f.fitted));
    r[T_ABOVE] = __popcll(__ballot(fit && f.d2 > threshold));
    r[T_MAX] = mx;
    const auto opOf = [](uint32_t c) { return c == (uint32_t)T_MAX ? PB_FOLD_MAX_UNSIGNED : PB_FOLD_SUM; };
    if (blockFold(sRed, r, opOf, v)) {
      const uint32_t c = threadIdx.x;
      pbStrainStats *row = rows + mb;
      if (v) {  // (a signed sum that is zero adds nothing either)
        if (c == T_FITTED) atomicAdd(&row->fitted, (unsigned)v);
        else if (c == T_UNFITTED) atomicAdd(&row->unfitted, (unsigned)v);
        else if (c == T_ABOVE) atomicAdd(&row->above, (unsigned)v);
        else if (c == T_USED) atomicAdd(&row->bonds_used, v);
        else if (c == T_DROPPED) atomicAdd(&row->bonds_dropped, v);
        else if (c == T_MAX) atomicMax(&row->max_d2, v);
        else atomicAdd((unsigned long long *)&row->yxx + (c - T_SUMS), v);  // the two partial sums: the host composes them
      }
    }
    __syncthreads();  // sRed is written again for the next member
  }
}

// leaves the moments, d2 and the rows (partial sums in every pbMoment128) on the device and the stream drained
int strainSweep(pbSim *S, float d2Threshold) {
  useDevice(S);
  PbClusterScratch *C = S->cluster;
  const size_t total = S->total;  // (each on its own: a failed allocation leaves the rest to the next call)
  PB_TRY(C->tPos1.ensure(total));
  PB_TRY(C->tMoments.ensure(total * PB_STRAIN_MOMENTS));
  PB_TRY(C->tD2.ensure(total));
  PB_TRY(C->tRows.ensure(S->nsims));
  PB_TRY(C->strainSpan.start(S->stream));
  PB_TRY(hipMemsetAsync(C->tRows, 0, sizeof(pbStrainStats) * S->nsims, S->stream));
  const int rc = pbDynamicsScatter(S, C->tPos1);
  if (rc != PB_OK) return rc;
  const double threshold = (double)d2Threshold * 1099511627776.0;  // 2^40: exact
  hipLaunchKernelGGL(k_strain_fit, dim3(cdiv(S->total, CT)), dim3(CT), 0, S->stream, C->dOffsets, C->dOther, C->dPos0,
                     C->tPos1, S->orig[S->cur], S->n, S->total, threshold, C->tMoments, C->tD2, C->tRows);
  PB_TRY(hipGetLastError());
  PB_TRY(C->strainSpan.stop(S->stream));
  PB_TRY(C->strainSpan.ms(&C->strainMs));
  PB_TRY(hipStreamSynchronize(S->stream));
  C->strainRuns++;
  return PB_OK;
}

}  // namespace

int pbSimStrainStats(pbSim *S, float d2Threshold, pbStrainStats *rows) {
  if (!S || !rows) return pbFail("pbSimStrainStats", ": null handle or rows");
  if (!(d2Threshold >= 0.0f) || !(d2Threshold < __builtin_inff()))
    return pbFail("pbSimStrainStats", ": d2Threshold must be finite and >= 0");
  int rc = pbClusterCheckArgs("pbSimStrainStats", S, nullptr, nullptr);
  if (rc == PB_OK) rc = pbNeedMark("pbSimStrainStats", S);
  if (rc == PB_OK) rc = strainSweep(S, d2Threshold);
  if (rc != PB_OK) return rc;
  PB_TRY(hipMemcpy(rows, S->cluster->tRows, sizeof(pbStrainStats) * S->nsims, hipMemcpyDeviceToHost));
  for (uint32_t mb = 0; mb < S->nsims; mb++) {  // every pair of partial sums as one normalised 128-bit integer
    pbMoment128 *sums = &rows[mb].yxx;          // yxx ... w and sum_d2 follow one another
    for (int c = 0; c < 9; c++) sums[c] = pbFixedNormalised(pbFixedCompose(sums[c].lo, (unsigned long long)sums[c].hi));
  }
  return PB_OK;
}

int pbSimStrainOf(pbSim *S, unsigned member, long long *moments, double *gradient, double *d2min) {
  if (!S) return pbFail("pbSimStrainOf", ": null handle");
  if (!moments && !gradient && !d2min) return pbFail("pbSimStrainOf", ": moments, gradient and d2min are all null");
  int rc = pbClusterCheckArgs("pbSimStrainOf", S, nullptr, &member);
  if (rc == PB_OK) rc = pbNeedMark("pbSimStrainOf", S);
  if (rc == PB_OK) rc = strainSweep(S, 0.0f);
  if (rc != PB_OK) return rc;
  PbClusterScratch *C = S->cluster;
  const size_t n = S->n, base = (size_t)member * n;
  std::vector<long long> own;
  if (gradient && !moments) own.resize(n * PB_STRAIN_MOMENTS), moments = own.data();
  if (moments)
    PB_TRY(hipMemcpyAsync(moments, C->tMoments + base * PB_STRAIN_MOMENTS, sizeof(long long) * n * PB_STRAIN_MOMENTS,
                          hipMemcpyDeviceToHost, S->stream));
  if (d2min) PB_TRY(hipMemcpyAsync(d2min, C->tD2 + base, sizeof(double) * n, hipMemcpyDeviceToHost, S->stream));
  PB_TRY(hipStreamSynchronize(S->stream));
  if (gradient)
    for (size_t i = 0; i < n; i++) {
      const PbStrainFit f = pbStrainFit(moments + i * PB_STRAIN_MOMENTS);
      gradient[4 * i] = f.jxx, gradient[4 * i + 1] = f.jxy, gradient[4 * i + 2] = f.jyx, gradient[4 * i + 3] = f.jyy;
    }
  return PB_OK;
}

int pbSimGetStrainTimes(pbSim *S, unsigned long long *analyses, float *last_device_ms) {
  if (!S) return pbFail("pbSimGetStrainTimes", ": null handle");
  if (analyses) *analyses = S->cluster ? S->cluster->strainRuns : 0ull;
  if (last_device_ms) *last_device_ms = S->cluster ? S->cluster->strainMs : 0.0f;
  return PB_OK;
}
