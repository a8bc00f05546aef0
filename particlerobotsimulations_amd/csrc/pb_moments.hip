// pb_moments.hip -- time series on gfx950: one row of integer moments of positions, velocities and radii per member
// (pbMomentsRow), taken now (pbSimMoments) or recorded into a device ring in front of chosen steps while pbSimStep runs
// (pbSimSetSeries / pbSimGetSeriesOf; include/particlebot_hip.h has the definitions).
//
//   k_mom_init        the target row of every member: zeros, the box at its identities (INT_MAX / INT_MIN)
//   k_mom_accumulate  one pass over pr[cur] and vel[cur] of the whole batch in SLOT order (16 + 8 bytes per bot, coalesced;
//                     orig is never read).  Up to PB_MOMENTS_BLOCKS workgroups per member, each lane a grid-stride loop
//                     over its member's slots with twenty accumulators in registers; then shuffles inside the wave, the
//                     four waves through 640 bytes of LDS, and one set of 64-bit integer atomics (32-bit min / max for
//                     the box) per workgroup into the member's row.
// Everything that is added is an integer, so nothing depends on the slot order, on the kernel form that stepped or on the
// order of the adds.  No float atomics, no 128-bit atomics, no scratch memory.  A record is two launches on the batch's
// stream between two events; the host never waits for them.
#include <limits.h>
#include <math.h>

#include "pb_engine.hpp"
#include "pb_fixed.hpp"

static_assert(sizeof(pbMoment128) == 16, "a 128-bit sum is two 64-bit accumulators");
static_assert(sizeof(pbMomentsRow) == 152, "a member's row is 152 bytes");

namespace {

constexpr int MT = 256;
// the columns of the row reduction: sixteen sums, then the box
enum {
  M_MEASURED, M_QX, M_QY, M_QR, M_WX, M_WY,
  M_XX_LO, M_XX_HI, M_YY_LO, M_YY_HI, M_XY_LO, M_XY_HI, M_RR_LO, M_RR_HI, M_VV_LO, M_VV_HI,
  M_SUMS,
  M_MIN_X = M_SUMS, M_MAX_X, M_MIN_Y, M_MAX_Y,
  M_COLS
};

__global__ __launch_bounds__(MT) void k_mom_init(pbMomentsRow *__restrict__ rows, uint32_t stride, uint32_t nsims) {
  const uint32_t m = blockIdx.x * MT + threadIdx.x;
  if (m >= nsims) return;
  pbMomentsRow *r = rows + (size_t)m * stride;
  r->step = 0ull, r->time = 0.0f, r->measured = 0u;
  r->sum_qx = r->sum_qy = r->sum_qr = r->sum_wx = r->sum_wy = 0ll;
  r->min_qx = r->min_qy = INT_MAX;
  r->max_qx = r->max_qy = INT_MIN;
  r->xx.lo = r->yy.lo = r->xy.lo = r->rr.lo = r->vv.lo = 0ull;
  r->xx.hi = r->yy.hi = r->xy.hi = r->rr.hi = r->vv.hi = 0ll;
}

__global__ __launch_bounds__(MT) void k_mom_accumulate(const float4 *__restrict__ pr, const float2 *__restrict__ vel,
                                                       uint32_t n, uint32_t blocksPerMember,
                                                       pbMomentsRow *__restrict__ rows, uint32_t stride) {
  __shared__ unsigned long long sRed[MT / 64][M_COLS];
  const uint32_t member = blockIdx.x / blocksPerMember, b = blockIdx.x - member * blocksPerMember;
  const uint32_t base = member * n;  // a member's slots are its own block of the arrays; the batch is below 2^28 bots
  unsigned long long a[M_SUMS];
#pragma unroll
  for (int c = 0; c < M_SUMS; c++) a[c] = 0ull;
  int minX = INT_MAX, maxX = INT_MIN, minY = INT_MAX, maxY = INT_MIN;
#pragma unroll 1
  for (uint32_t i = b * MT + threadIdx.x; i < n; i += blocksPerMember * MT) {
    const float4 q = pr[base + i];
    const float2 v = vel[base + i];
    if (pbFixedInRange(q.x) && pbFixedInRange(q.y) && pbFixedInRange(v.x) && pbFixedInRange(v.y) &&
        pbFixedInRange(q.z)) {
      const long long qx = pbFixedQuantise(q.x), qy = pbFixedQuantise(q.y), qr = pbFixedQuantise(q.z);
      const long long wx = pbFixedQuantise(v.x), wy = pbFixedQuantise(v.y);
      a[M_MEASURED] += 1ull;
      a[M_QX] += (unsigned long long)qx, a[M_QY] += (unsigned long long)qy, a[M_QR] += (unsigned long long)qr;
      a[M_WX] += (unsigned long long)wx, a[M_WY] += (unsigned long long)wy;
      pbFixedSplitAdd(qx * qx, a[M_XX_LO], a[M_XX_HI]);
      pbFixedSplitAdd(qy * qy, a[M_YY_LO], a[M_YY_HI]);
      pbFixedSplitAdd(qx * qy, a[M_XY_LO], a[M_XY_HI]);
      pbFixedSplitAdd(qr * qr, a[M_RR_LO], a[M_RR_HI]);
      pbFixedSplitAdd(wx * wx + wy * wy, a[M_VV_LO], a[M_VV_HI]);  // below 2^63
      minX = min(minX, (int)qx), maxX = max(maxX, (int)qx);
      minY = min(minY, (int)qy), maxY = max(maxY, (int)qy);
    }
  }
  // the wave's sums with shuffles, the four waves through LDS, one set of atomics
  // (the butterfly stays rolled: waveSumRolled, pb_fixed.hpp, has the reason)
  waveSumRolled(a, [&](int m) {
    minX = min(minX, __shfl_xor(minX, m)), maxX = max(maxX, __shfl_xor(maxX, m));
    minY = min(minY, __shfl_xor(minY, m)), maxY = max(maxY, __shfl_xor(maxY, m));
  });
  // the fold's columns (an array of their own: the sums keep the shape the loop and the butterfly compile best with);
  // the box as sign-extended 64-bit values, so that one signed compare serves all four
  unsigned long long cols[M_COLS];
#pragma unroll
  for (int c = 0; c < M_SUMS; c++) cols[c] = a[c];
  cols[M_MIN_X] = (unsigned long long)(long long)minX, cols[M_MAX_X] = (unsigned long long)(long long)maxX;
  cols[M_MIN_Y] = (unsigned long long)(long long)minY, cols[M_MAX_Y] = (unsigned long long)(long long)maxY;
  unsigned long long s;
  const auto opOf = [](uint32_t c) {
    return c < (uint32_t)M_SUMS ? PB_FOLD_SUM
           : c == (uint32_t)M_MIN_X || c == (uint32_t)M_MIN_Y ? PB_FOLD_MIN_SIGNED : PB_FOLD_MAX_SIGNED;
  };
  if (!blockFold(sRed, cols, opOf, s)) return;
  const uint32_t c = threadIdx.x;
  const bool isMin = c == (uint32_t)M_MIN_X || c == (uint32_t)M_MIN_Y;
  pbMomentsRow *row = rows + (size_t)member * stride;
  if (c >= (uint32_t)M_SUMS) {  // (a workgroup without a measured bot holds the identities: they change nothing)
    int *f = c == (uint32_t)M_MIN_X ? &row->min_qx : c == (uint32_t)M_MAX_X ? &row->max_qx
             : c == (uint32_t)M_MIN_Y ? &row->min_qy : &row->max_qy;
    if (isMin) atomicMin(f, (int)(long long)s);
    else atomicMax(f, (int)(long long)s);
    return;
  }
  if (!s) return;  // (a signed sum that is zero adds nothing either)
  if (c == (uint32_t)M_MEASURED) {
    atomicAdd(&row->measured, (unsigned)s);
    return;
  }
  unsigned long long *f;  // two's complement: a signed field takes its sum modulo 2^64
  switch (c) {
    case M_QX: f = (unsigned long long *)&row->sum_qx; break;
    case M_QY: f = (unsigned long long *)&row->sum_qy; break;
    case M_QR: f = (unsigned long long *)&row->sum_qr; break;
    case M_WX: f = (unsigned long long *)&row->sum_wx; break;
    case M_WY: f = (unsigned long long *)&row->sum_wy; break;
    case M_XX_LO: f = &row->xx.lo; break;
    case M_XX_HI: f = (unsigned long long *)&row->xx.hi; break;
    case M_YY_LO: f = &row->yy.lo; break;
    case M_YY_HI: f = (unsigned long long *)&row->yy.hi; break;
    case M_XY_LO: f = &row->xy.lo; break;
    case M_XY_HI: f = (unsigned long long *)&row->xy.hi; break;
    case M_RR_LO: f = &row->rr.lo; break;
    case M_RR_HI: f = (unsigned long long *)&row->rr.hi; break;
    case M_VV_LO: f = &row->vv.lo; break;
    default: f = (unsigned long long *)&row->vv.hi; break;
  }
  atomicAdd(f, s);
}

// the rows of every member, rows[m * stride], from the state as it is: queued on the batch's stream, not waited for
int momentsPass(pbSim *S, pbMomentsRow *rows, uint32_t stride) {
  const uint32_t perMember = cdiv(S->n, MT);
  const uint32_t bpm = perMember < PB_MOMENTS_BLOCKS ? perMember : PB_MOMENTS_BLOCKS;
  PB_TRY(S->momClock.start(S->stream));
  hipLaunchKernelGGL(k_mom_init, dim3(cdiv(S->nsims, MT)), dim3(MT), 0, S->stream, rows, stride, S->nsims);
  hipLaunchKernelGGL(k_mom_accumulate, dim3(S->nsims * bpm), dim3(MT), 0, S->stream, S->pr[S->cur], S->vel[S->cur],
                     S->n, bpm, rows, stride);
  PB_TRY(hipGetLastError());
  PB_TRY(S->momClock.stop(S->stream));
  return PB_OK;
}

// what the device leaves to the host: the clock, and a box of zeros for a row without a measured bot
void finishRow(pbMomentsRow &r, float time, unsigned long long step) {
  r.time = time, r.step = step;
  if (!r.measured) r.min_qx = r.max_qx = r.min_qy = r.max_qy = 0;
}

}  // namespace

int pbSeriesRecord(pbSim *S, float t) {
  const uint32_t slot = (uint32_t)(S->series.records % S->series.cap);
  const int rc = momentsPass(S, S->series.ring + slot, S->series.cap);
  if (rc != PB_OK) return rc;
  S->series.times[slot] = t, S->series.steps[slot] = S->stats.steps;
  S->series.records++;
  return PB_OK;
}

extern "C" {

int pbSimMoments(pbSim *S, pbMomentsRow *rows) {
  if (!S || !rows) return pbFail("pbSimMoments", ": null handle or rows");
  int rc = pbCheckBatch("pbSimMoments", S);
  if (rc != PB_OK) return rc;
  useDevice(S);
  PB_TRY(S->momRows.ensure(S->nsims));
  rc = momentsPass(S, S->momRows, 1u);
  if (rc != PB_OK) return rc;
  PB_TRY(hipMemcpyAsync(rows, S->momRows, sizeof(pbMomentsRow) * S->nsims, hipMemcpyDeviceToHost, S->stream));
  PB_TRY(hipStreamSynchronize(S->stream));
  for (uint32_t m = 0; m < S->nsims; m++) finishRow(rows[m], S->time, S->stats.steps);
  return PB_OK;
}

int pbSimSetSeries(pbSim *S, float interval, unsigned capacity) {
  if (!S) return pbFail("pbSimSetSeries", ": null handle");
  if (const int rc = pbCheckInterval("pbSimSetSeries", interval, false)) return rc;  // (the series has no manual records)
  if ((unsigned long long)capacity * S->nsims * sizeof(pbMomentsRow) > (1ull << 31))
    return pbFail("pbSimSetSeries", ": capacity x members x 152 bytes must not exceed 2^31 bytes");
  const int rc = pbCheckBatch("pbSimSetSeries", S);
  if (rc != PB_OK) return rc;
  useDevice(S);
  PB_TRY(hipStreamSynchronize(S->stream));  // a record of the old ring may still be in flight
  S->series = PbSeries();
  if (!capacity) return PB_OK;
  PB_TRY(S->series.ring.alloc((size_t)capacity * S->nsims));
  S->series.interval = interval, S->series.cap = capacity;
  S->series.times.assign(capacity, 0.0f);
  S->series.steps.assign(capacity, 0ull);
  return PB_OK;
}

int pbSimGetSeriesInfo(pbSim *S, float *interval, unsigned *capacity, unsigned long long *records) {
  if (!S) return pbFail("pbSimGetSeriesInfo", ": null handle");
  if (!interval && !capacity && !records)
    return pbFail("pbSimGetSeriesInfo", ": interval, capacity and records are all null");
  if (interval) *interval = S->series.interval;
  if (capacity) *capacity = S->series.cap;
  if (records) *records = S->series.records;
  return PB_OK;
}

int pbSimGetSeriesOf(pbSim *S, unsigned member, unsigned long long first, unsigned count, pbMomentsRow *rows) {
  if (!S || !rows) return pbFail("pbSimGetSeriesOf", ": null handle or rows");
  if (member >= S->nsims) return pbFail("pbSimGetSeriesOf", ": member out of range");
  if (!S->series.ring) return pbFail("pbSimGetSeriesOf", ": the series is off");
  const unsigned long long have = S->series.records, cap = S->series.cap;
  const unsigned long long oldest = have - (have < cap ? have : cap);
  if (first < oldest || first > have || count > have - first)
    return pbFail("pbSimGetSeriesOf", ": records outside the ring's window");
  if (!count) return PB_OK;
  useDevice(S);
  // the ring wraps at most once inside the range
  const pbMomentsRow *ring = S->series.ring + (size_t)member * cap;
  const unsigned long long s0 = first % cap;
  const unsigned long long head = count < cap - s0 ? count : cap - s0;
  PB_TRY(hipMemcpyAsync(rows, ring + s0, sizeof(pbMomentsRow) * head, hipMemcpyDeviceToHost, S->stream));
  if (head < count)
    PB_TRY(hipMemcpyAsync(rows + head, ring, sizeof(pbMomentsRow) * (count - head), hipMemcpyDeviceToHost, S->stream));
  PB_TRY(hipStreamSynchronize(S->stream));
  for (unsigned k = 0; k < count; k++) {
    const size_t slot = (size_t)((first + k) % cap);
    finishRow(rows[k], S->series.times[slot], S->series.steps[slot]);
  }
  return PB_OK;
}

int pbSimGetSeriesTimes(pbSim *S, unsigned long long *records, float *last_device_ms) {
  if (!S) return pbFail("pbSimGetSeriesTimes", ": null handle");
  return pbSpanGet(S, S->momClock, S->series.records, records, last_device_ms);
}

}  // extern "C"
