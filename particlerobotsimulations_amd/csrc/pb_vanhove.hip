// pb_vanhove.hip -- the self part of the van Hove function on gfx950: per member and lag, the histogram of the
// displacement's length, the histograms of its signed x and y components, and the sums of its second and fourth powers,
// over the measured (bot, origin) pairs, averaged over time origins while pbSimStep runs (pbSimSetVanHove /
// pbSimVanHoveRecord / pbSimGetVanHove; include/particlebot_hip.h has the definitions).  The ring of snapshots, its
// pairing lag by lag, its book and the shells of the entry points are the lag ring's (pb_engine.hpp, PbLagBook ...
// pbLagTimes); the cell's words, the edges and both bin rules are pb_vanhove.hpp's; neither is restated here.
//
//   k_vh_snapshot    one pass over pr[cur] and orig[cur] in SLOT order (coalesced reads); each lane writes one float2
//                    (x, y) to ring[slot][member * n + orig]: the scattered 8-byte store is the only uncoalesced access
//   k_vh_accumulate  entirely in ORIGINAL order: one workgroup of 256 lanes per (member, lag, block), at most
//                    PB_VANHOVE_BLOCKS blocks per member and lag, all lags of a record in one launch.  A workgroup copies
//                    the edges E_1 ... E_bins into LDS (8 KiB at most; E_0 = 0 is not stored) and zeroes a histogram of
//                    5 bins 32-bit counters in LDS (20 KiB at most).  Each lane runs a grid-stride loop over two
//                    snapshots read as coalesced 8-byte loads; per measured pair it finds the radial bin by a binary
//                    search in the LDS edges and the two axis bins by one unsigned 32-bit division each, adds 1 to three
//                    LDS counters (vhCount: equal counters of a wave combined once by ballot, then LDS atomics; a
//                    beyond count goes to a register instead), and keeps ten
//                    64-bit moments in registers.  At the end every non-zero LDS counter becomes one 64-bit atomicAdd
//                    into the cell, and the moments go through a wave butterfly, the four waves through 320 bytes of
//                    LDS, and one set of 64-bit integer atomics per workgroup, as k_tc_accumulate's.
// WHY 32 BITS SUFFICE IN LDS.  pbLagRecord gives a member and lag bpl = min(ceil(n / 256), 256) workgroups, and workgroup
// b takes the bots b * 256 + t + j * bpl * 256.  With bpl < 256 that is one trip: at most 256 pairs.  With bpl == 256 a
// lane makes at most ceil(n / 65536) trips, and n < 2^28 (pbLagCheckBatch), so a workgroup sees at most
// 256 * ceil(n / 65536) <= 256 * 2^12 = 2^20 pairs per launch, and a pair adds 1 to at most one counter of each
// histogram (combined or not): no LDS counter passes 2^20.
// Everything that is added is an integer, so nothing depends on the slot order, on the kernel form that stepped or on the
// order of the adds.  No float atomics, no 128-bit atomics, no scratch memory.  A record is these launches on the batch's
// stream between two events; the host never waits for them.
// The bounds are pb_fixed.hpp's: the cap is 2^31 samples in a cell.
#include <math.h>

#include <algorithm>

#include "pb_engine.hpp"
#include "pb_fixed.hpp"
#include "pb_vanhove.hpp"

static_assert(sizeof(pbVanHoveRow) == 96, "a lag's row is 96 bytes");

namespace {

constexpr int VT = PB_LAG_LANES;
constexpr uint32_t VH_LDS_EDGES = PB_VANHOVE_MAX_BINS, VH_LDS_COUNTERS = PB_VH_HIST_PER_BIN * PB_VANHOVE_MAX_BINS;

__global__ __launch_bounds__(VT) void k_vh_snapshot(const float4 *__restrict__ pr, const uint32_t *__restrict__ orig,
                                                    uint32_t n, float2 *__restrict__ snap) {
  const uint32_t l = blockIdx.x * VT + threadIdx.x;
  if (l >= n) return;
  const uint32_t s = blockIdx.y * n + l;  // the batch is below 2^28 bots
  const uint32_t o = orig[s];
  // (a layout is a permutation of 0 .. n - 1; were it not, nothing is written outside the member's block: k_tc_snapshot)
  if (o >= n) return;
  const float4 q = pr[s];
  snap[blockIdx.y * n + o] = make_float2(q.x, q.y);
}

// How a wave adds its lanes' counts to the LDS histogram.  For PB_VH_COMBINE_ROUNDS rounds the first lane that still has
// a count to add is the leader, the lanes with its counter are found by a ballot and the leader adds their number with
// one LDS atomic, as the field map's PB_FIELD_ROUNDS; what is left after the rounds is one plain LDS atomic per lane.
// Displacements at short lags are narrow: most lanes of a wave hit one or two counters, and plain atomics on one
// address serialise.  One round ships.  Measured on the 10^6-bot arena at 16 lags (profiles/van_hove.txt, `form` rows):
// against 0 rounds it takes 0.13 ms instead of 0.22 ms per record where every pair hits one counter, and 0.14 ms instead
// of 0.13 ms on displacements spread over 34 bins; two rounds are slower than one on both.  `at` is the counter's index
// or VH_NONE; every lane of the wave calls it.
#ifndef PB_VH_COMBINE_ROUNDS
#define PB_VH_COMBINE_ROUNDS 1  // (0: plain atomics only, for the A/B of tools/vanhove_cost.py)
#endif
constexpr uint32_t VH_NONE = 0xFFFFFFFFu;
PB_DEV void vhCount(uint32_t *sHist, uint32_t at) {
#if PB_VH_COMBINE_ROUNDS > 0
  unsigned long long pending = __ballot(at != VH_NONE);
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll 1
  for (int k = 0; k < PB_VH_COMBINE_ROUNDS && pending; k++) {  // (wave-uniform)
    const uint32_t leader = (uint32_t)__ffsll((long long)pending) - 1u;
    const uint32_t key = (uint32_t)__shfl((int)at, (int)leader);
    const unsigned long long same = __ballot(at == key);
    if (lane == leader) atomicAdd(&sHist[key], (uint32_t)__popcll(same));
    if (at == key) at = VH_NONE;
    pending &= ~same;
  }
#endif
  if (at != VH_NONE) atomicAdd(&sHist[at], 1u);
}

__global__ __launch_bounds__(VT) void k_vh_accumulate(const float2 *__restrict__ ring, uint32_t n, uint32_t total,
                                                      uint32_t lags, uint32_t slotNow, uint32_t nLags,
                                                      uint32_t blocksPerLag, uint32_t qw, uint32_t bins,
                                                      const unsigned long long *__restrict__ edges,
                                                      unsigned long long *__restrict__ table) {
  __shared__ unsigned long long sEdge[VH_LDS_EDGES];  // sEdge[k - 1] = E_k, k = 1 ... bins
  __shared__ uint32_t sHist[VH_LDS_COUNTERS];         // radial | x | y, as the cell behind its moments
  __shared__ unsigned long long sRed[VT / 64][PB_VH_MOMENTS];
  const auto [member, lag, b, now, then] = pbLagPair(ring, n, total, lags, slotNow, nLags, blocksPerLag);
  const uint32_t counters = PB_VH_HIST_PER_BIN * bins;  // bins <= PB_VANHOVE_MAX_BINS: the setter's check
  for (uint32_t j = threadIdx.x; j < bins; j += VT) sEdge[j] = edges[j + 1u];
  for (uint32_t j = threadIdx.x; j < counters; j += VT) sHist[j] = 0u;
  __syncthreads();
  const auto edgeAt = [&](uint32_t k) { return sEdge[k - 1u]; };
  unsigned long long a[PB_VH_MOMENTS];
#pragma unroll
  for (int c = 0; c < PB_VH_MOMENTS; c++) a[c] = 0ull;
#pragma unroll 1
  for (uint32_t t0 = b * VT; t0 < n; t0 += blocksPerLag * VT) {  // (workgroup-uniform: vhCount needs whole waves)
    const uint32_t i = t0 + threadIdx.x;
    uint32_t r = VH_NONE, x = VH_NONE, y = VH_NONE;  // the counters this lane adds to
    if (i < n) {
      const float2 u = now[i], z = then[i];
      const float dx = u.x - z.x, dy = u.y - z.y;
      // (a NaN or an infinity in any of the four inputs is out of range: inf - inf and inf - x are not below 2048)
      if (pbFixedInRange(dx) && pbFixedInRange(dy)) {
        const long long qx = pbFixedQuantise(dx), qy = pbFixedQuantise(dy);
        const unsigned long long s = (unsigned long long)(qx * qx + qy * qy);  // below 2^63: k_tc_accumulate's s
        a[PB_VH_SAMPLES] += 1ull;
        pbFixedSplitAdd(s, a[PB_VH_MSD_LO], a[PB_VH_MSD_HI]);
        pbVhQ4Add(s * s, __umul64hi(s, s), a[PB_VH_Q4_0], a[PB_VH_Q4_1], a[PB_VH_Q4_2], a[PB_VH_Q4_3]);
        const uint32_t rb = pbVhRadialBin(edgeAt, bins, s);
        const uint32_t xb = pbVhAxisIndex((int)qx, qw, bins), yb = pbVhAxisIndex((int)qy, qw, bins);
        if (rb < bins) r = pbVhRadialAt(bins) + rb;
        else a[PB_VH_BEYOND_R] += 1ull;
        if (xb < 2u * bins) x = pbVhXAt(bins) + xb;
        else a[PB_VH_BEYOND_X] += 1ull;
        if (yb < 2u * bins) y = pbVhYAt(bins) + yb;
        else a[PB_VH_BEYOND_Y] += 1ull;
      }
    }
    vhCount(sHist, r);
    vhCount(sHist, x);
    vhCount(sHist, y);
  }
  unsigned long long *cell = table + ((size_t)member * lags + lag) * pbVhCellWords(bins);
  __syncthreads();  // the workgroup's histogram is complete
  for (uint32_t j = threadIdx.x; j < counters; j += VT) {
    const uint32_t c = sHist[j];
    if (c) (void)__hip_atomic_fetch_add(cell + PB_VH_MOMENTS + j, (unsigned long long)c, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);  // no-return
  }
  // the wave's sums with a butterfly of 64-bit shuffles, the four waves through LDS, one set of atomics
  waveSumRolled(a, [](int) {});
  unsigned long long v;
  if (!blockFold(sRed, a, [](uint32_t) { return PB_FOLD_SUM; }, v)) return;
  if (v) atomicAdd(cell + threadIdx.x, v);
}

}  // namespace

int pbVanHoveRecord(pbSim *S) {
  PbVanHove &V = S->vh;
  const int c = S->cur;
  return pbLagRecord(S, V.lag, [&](dim3 grid, float2 *snap) {
    hipLaunchKernelGGL(k_vh_snapshot, grid, dim3(VT), 0, S->stream, S->pr[c], S->orig[c], S->n, snap);
  }, [&](dim3 grid, uint32_t slot, uint32_t nLags, uint32_t bpl) {
    hipLaunchKernelGGL(k_vh_accumulate, grid, dim3(VT), 0, S->stream, V.lag.ring, S->n, S->total, V.lag.book.lags, slot,
                       nLags, bpl, V.qw, V.bins, V.edges, V.lag.table);
  });
}

extern "C" {

int pbSimSetVanHove(pbSim *S, float interval, unsigned lags, float binWidth, unsigned bins) {
  const char *fn = "pbSimSetVanHove";
  if (!S) return pbFail(fn, ": null handle");
  if (const int rc = pbLagCheckArgs(fn, interval, lags)) return rc;
  uint32_t qw = 0u;
  if (lags) {  // (lags == 0 switches off: the width and the bins are not read)
    if (bins < 1u || bins > PB_VANHOVE_MAX_BINS) return pbFail(fn, ": bins must be 1 ... 1024");
    if (!(binWidth > 0.0f) || !pbFixedInRange(binWidth)) return pbFail(fn, ": binWidth must be in (0, 2048)");
    qw = (uint32_t)pbFixedQuantise(binWidth);
    if (qw < 1u) return pbFail(fn, ": binWidth must be at least one quantum of 2^-20");
  }
  if (const int rc = pbLagCheckBatch<float2>(fn, S, lags)) return rc;
  if (lags && (unsigned long long)S->nsims * lags * pbVhCellWords(bins) * sizeof(unsigned long long) > (1ull << 31))
    return pbFail(fn, ": the table (members x lags x (10 + 5 bins) x 8 bytes) must not exceed 2^31 bytes");
  return pbLagSwitch(S, S->vh, interval, lags, pbVhCellWords(bins), [&](PbVanHove &V) -> int {
    V.width = binWidth, V.qw = qw, V.bins = bins;
    std::vector<unsigned long long> host((size_t)bins + 1u);
    pbVhEdges(qw, bins, host.data());
    PB_TRY(V.edges.alloc(host.size()));
    PB_TRY(hipMemcpyAsync(V.edges, host.data(), sizeof(unsigned long long) * host.size(), hipMemcpyHostToDevice,
                          S->stream));
    PB_TRY(hipStreamSynchronize(S->stream));  // (the copy reads host memory that goes with this call)
    return PB_OK;
  });
}

int pbSimVanHoveRecord(pbSim *S) {
  return pbLagManualRecord("pbSimVanHoveRecord", S, &pbSim::vh, "van Hove function", pbVanHoveRecord);
}

int pbSimGetVanHoveInfo(pbSim *S, float *interval, unsigned *lags, float *binWidth, unsigned *bins,
                        unsigned long long *records) {
  if (!S) return pbFail("pbSimGetVanHoveInfo", ": null handle");
  if (!interval && !lags && !binWidth && !bins && !records)
    return pbFail("pbSimGetVanHoveInfo", ": interval, lags, binWidth, bins and records are all null");
  if (interval) *interval = S->vh.lag.interval;
  if (lags) *lags = S->vh.lag.book.lags;
  if (binWidth) *binWidth = S->vh.width;
  if (bins) *bins = S->vh.bins;
  if (records) *records = S->vh.lag.book.records;
  return PB_OK;
}

int pbSimGetVanHove(pbSim *S, pbVanHoveRow *rows, unsigned long long *counts) {
  if (!S || (!rows && !counts)) return pbFail("pbSimGetVanHove", ": null handle, or rows and counts both null");
  const PbVanHove &V = S->vh;
  const PbLagBook &book = V.lag.book;
  const size_t words = pbVhCellWords(V.bins), hist = words - PB_VH_MOMENTS;
  std::vector<unsigned long long> acc;
  if (const int rc = pbLagFetch("pbSimGetVanHove", S, V.lag, "van Hove function", acc, PB_VH_SAMPLES, words)) return rc;
  for (size_t k = 0; k < (size_t)S->nsims * book.lags; k++) {
    const unsigned long long *w = &acc[k * words];
    if (counts) std::copy(w + PB_VH_MOMENTS, w + words, counts + k * hist);
    if (!rows) continue;
    pbVanHoveRow &r = rows[k];
    book.columns((unsigned)(k % book.lags), r);
    r.reserved = 0u, r.samples = w[PB_VH_SAMPLES];
    r.beyond_r = w[PB_VH_BEYOND_R], r.beyond_x = w[PB_VH_BEYOND_X], r.beyond_y = w[PB_VH_BEYOND_Y];
    r.msd = pbFixedNormalised(pbFixedCompose(w[PB_VH_MSD_LO], w[PB_VH_MSD_HI]));
    pbVhQ4Compose(w[PB_VH_Q4_0], w[PB_VH_Q4_1], w[PB_VH_Q4_2], w[PB_VH_Q4_3], r.q4);
  }
  return PB_OK;
}

int pbSimGetVanHoveTimes(pbSim *S, unsigned long long *records, float *last_device_ms) {
  return pbLagTimes("pbSimGetVanHoveTimes", S, &pbSim::vh, records, last_device_ms);
}

}  // extern "C"
