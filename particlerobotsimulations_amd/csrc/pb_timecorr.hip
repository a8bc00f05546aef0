// pb_timecorr.hip -- time correlations on gfx950: the mean squared displacement, the velocity autocorrelation and the
// overlap function per lag, averaged over time origins while pbSimStep runs (pbSimSetTimeCorrelation /
// pbSimTimeCorrelationRecord / pbSimGetTimeCorrelation; include/particlebot_hip.h has the definitions).
//
// The ring of snapshots, its pairing lag by lag, its book and the shells of the entry points are the lag ring's
// (pb_engine.hpp, PbLagBook ... pbLagTimes); here are what the ring stores, what a pair adds and how a row is written.
// The table is nine 64-bit words per (member, lag).
//
//   k_tc_snapshot    one pass over pr[cur], vel[cur] and orig[cur] in SLOT order (coalesced reads); each lane writes one
//                    float4 (x, y, vx, vy) to ring[slot][member * n + orig]: the scattered 16-byte store is the only
//                    uncoalesced access
//   k_tc_accumulate  entirely in ORIGINAL order: one workgroup of 256 lanes per (member, lag, block), at most
//                    PB_TCORR_BLOCKS blocks per member and lag; each lane a grid-stride loop over two snapshots read as
//                    coalesced 16-byte loads, nine 64-bit accumulators in registers; then a wave butterfly, the four
//                    waves through 288 bytes of LDS, and one set of 64-bit integer atomics per workgroup into the cell
//                    (atomicMax for max_q2).  All lags of a record go in one launch; the current snapshot is re-read
//                    per lag, which L2 and the Infinity Cache serve.
// Everything that is added is an integer, so nothing depends on the slot order, on the kernel form that stepped or on the
// order of the adds.  No float atomics, no 128-bit atomics, no scratch memory.  A record is these launches on the batch's
// stream between two events; the host never waits for them.
// The bounds are pb_fixed.hpp's: the cap is 2^31 samples in a cell.
#include <math.h>

#include "pb_engine.hpp"
#include "pb_fixed.hpp"

static_assert(sizeof(pbTimeCorrelationRow) == 96, "a lag's row is 96 bytes");

namespace {

constexpr int TT = PB_LAG_LANES;
// the words of a table cell
enum { T_SAMPLES, T_QX, T_QY, T_MSD_LO, T_MSD_HI, T_VACF_LO, T_VACF_HI, T_OVERLAP, T_SUMS, T_MAX_Q2 = T_SUMS, T_COLS };
static_assert(T_COLS == 9, "nine accumulators per lane and per cell");

__global__ __launch_bounds__(TT) void k_tc_snapshot(const float4 *__restrict__ pr, const float2 *__restrict__ vel,
                                                    const uint32_t *__restrict__ orig, uint32_t n,
                                                    float4 *__restrict__ snap) {
  const uint32_t l = blockIdx.x * TT + threadIdx.x;
  if (l >= n) return;
  const uint32_t s = blockIdx.y * n + l;  // the batch is below 2^28 bots
  const uint32_t o = orig[s];
  // A layout is a permutation of 0 .. n - 1.  Were it not, nothing is written outside the member's block: the slot is
  // skipped, and the bot it should have named keeps the entry of the record that used this ring slot before.
  if (o >= n) return;
  const float4 q = pr[s];
  const float2 v = vel[s];
  snap[blockIdx.y * n + o] = make_float4(q.x, q.y, v.x, v.y);
}

__global__ __launch_bounds__(TT) void k_tc_accumulate(const float4 *__restrict__ ring, uint32_t n, uint32_t total,
                                                      uint32_t lags, uint32_t slotNow, uint32_t nLags,
                                                      uint32_t blocksPerLag, unsigned long long a2,
                                                      unsigned long long *__restrict__ table) {
  __shared__ unsigned long long sRed[TT / 64][T_COLS];
  const auto [member, lag, b, now, then] = pbLagPair(ring, n, total, lags, slotNow, nLags, blocksPerLag);
  unsigned long long a[T_SUMS];
#pragma unroll
  for (int c = 0; c < T_SUMS; c++) a[c] = 0ull;
  unsigned long long maxQ2 = 0ull;
#pragma unroll 1
  for (uint32_t i = b * TT + threadIdx.x; i < n; i += blocksPerLag * TT) {
    const float4 u = now[i], z = then[i];
    const float dx = u.x - z.x, dy = u.y - z.y;
    // (a NaN or an infinity in any of the eight inputs is out of range: inf - inf and inf - x are not below 2048)
    if (pbFixedInRange(dx) && pbFixedInRange(dy) && pbFixedInRange(u.z) && pbFixedInRange(u.w) &&
        pbFixedInRange(z.z) && pbFixedInRange(z.w)) {
      const long long qx = pbFixedQuantise(dx), qy = pbFixedQuantise(dy);
      const unsigned long long s = (unsigned long long)(qx * qx + qy * qy);  // below 2^63
      const long long p = pbFixedQuantise(u.z) * pbFixedQuantise(z.z) + pbFixedQuantise(u.w) * pbFixedQuantise(z.w);
      a[T_SAMPLES] += 1ull;
      a[T_QX] += (unsigned long long)qx, a[T_QY] += (unsigned long long)qy;
      pbFixedSplitAdd(s, a[T_MSD_LO], a[T_MSD_HI]);
      pbFixedSplitAdd(p, a[T_VACF_LO], a[T_VACF_HI]);
      a[T_OVERLAP] += s < a2 ? 1ull : 0ull;
      maxQ2 = s > maxQ2 ? s : maxQ2;
    }
  }
  // the wave's sums with a butterfly of 64-bit shuffles, the four waves through LDS, one set of atomics
  waveSumRolled(a, [&](int m) {
    const unsigned long long other = shflXor64(maxQ2, m);
    maxQ2 = other > maxQ2 ? other : maxQ2;
  });
  unsigned long long cols[T_COLS];  // (an array of their own, as k_mom_accumulate's)
#pragma unroll
  for (int c = 0; c < T_SUMS; c++) cols[c] = a[c];
  cols[T_MAX_Q2] = maxQ2;
  unsigned long long v;
  const auto opOf = [](uint32_t c) { return c == (uint32_t)T_MAX_Q2 ? PB_FOLD_MAX_UNSIGNED : PB_FOLD_SUM; };
  if (!blockFold(sRed, cols, opOf, v)) return;
  const uint32_t c = threadIdx.x;
  if (!v) return;  // (a sum that is zero adds nothing, and 0 is the maximum's identity)
  unsigned long long *cell = table + ((size_t)member * lags + lag) * T_COLS;
  if (c == (uint32_t)T_MAX_Q2) atomicMax(cell + c, v);
  else atomicAdd(cell + c, v);  // two's complement: a signed word takes its sum modulo 2^64
}

}  // namespace

int pbTimeCorrRecord(pbSim *S) {
  PbTimeCorr &T = S->tc;
  const int c = S->cur;
  return pbLagRecord(S, T.lag, [&](dim3 grid, float4 *snap) {
    hipLaunchKernelGGL(k_tc_snapshot, grid, dim3(TT), 0, S->stream, S->pr[c], S->vel[c], S->orig[c], S->n, snap);
  }, [&](dim3 grid, uint32_t slot, uint32_t nLags, uint32_t bpl) {
    hipLaunchKernelGGL(k_tc_accumulate, grid, dim3(TT), 0, S->stream, T.lag.ring, S->n, S->total, T.lag.book.lags,
                       slot, nLags, bpl, T.a2, T.lag.table);
  });
}

extern "C" {

int pbSimSetTimeCorrelation(pbSim *S, float interval, unsigned lags, float overlapRadius) {
  const char *fn = "pbSimSetTimeCorrelation";
  if (!S) return pbFail(fn, ": null handle");
  if (const int rc = pbLagCheckArgs(fn, interval, lags)) return rc;
  if (!(overlapRadius >= 0.0f) || !pbFixedInRange(overlapRadius))
    return pbFail(fn, ": overlapRadius must be in [0, 2048)");
  if (const int rc = pbLagCheckBatch<float4>(fn, S, lags)) return rc;
  return pbLagSwitch(S, S->tc, interval, lags, T_COLS, [&](PbTimeCorr &T) {
    const long long qa = pbFixedQuantise(overlapRadius);
    T.radius = overlapRadius, T.a2 = (unsigned long long)(qa * qa);
    return PB_OK;
  });
}

int pbSimTimeCorrelationRecord(pbSim *S) {
  return pbLagManualRecord("pbSimTimeCorrelationRecord", S, &pbSim::tc, "correlation", pbTimeCorrRecord);
}

int pbSimGetTimeCorrelationInfo(pbSim *S, float *interval, unsigned *lags, float *overlapRadius,
                                unsigned long long *records) {
  if (!S) return pbFail("pbSimGetTimeCorrelationInfo", ": null handle");
  if (!interval && !lags && !overlapRadius && !records)
    return pbFail("pbSimGetTimeCorrelationInfo", ": interval, lags, overlapRadius and records are all null");
  if (interval) *interval = S->tc.lag.interval;
  if (lags) *lags = S->tc.lag.book.lags;
  if (overlapRadius) *overlapRadius = S->tc.radius;
  if (records) *records = S->tc.lag.book.records;
  return PB_OK;
}

int pbSimGetTimeCorrelation(pbSim *S, pbTimeCorrelationRow *rows) {
  if (!S || !rows) return pbFail("pbSimGetTimeCorrelation", ": null handle or rows");
  const PbLagBook &book = S->tc.lag.book;
  std::vector<unsigned long long> acc;
  if (const int rc = pbLagFetch("pbSimGetTimeCorrelation", S, S->tc.lag, "correlation", acc, T_SAMPLES, T_COLS))
    return rc;
  for (size_t k = 0; k < (size_t)S->nsims * book.lags; k++) {
    const unsigned long long *w = &acc[k * T_COLS];
    pbTimeCorrelationRow &r = rows[k];
    book.columns((unsigned)(k % book.lags), r);
    r.reserved = 0u, r.samples = w[T_SAMPLES];
    r.sum_qx = (long long)w[T_QX], r.sum_qy = (long long)w[T_QY];
    r.msd = pbFixedNormalised(pbFixedCompose(w[T_MSD_LO], w[T_MSD_HI]));
    r.vacf = pbFixedNormalised(pbFixedCompose(w[T_VACF_LO], w[T_VACF_HI]));
    r.overlap = w[T_OVERLAP], r.max_q2 = w[T_MAX_Q2];
  }
  return PB_OK;
}

int pbSimGetTimeCorrelationTimes(pbSim *S, unsigned long long *records, float *last_device_ms) {
  return pbLagTimes("pbSimGetTimeCorrelationTimes", S, &pbSim::tc, records, last_device_ms);
}

}  // extern "C"
