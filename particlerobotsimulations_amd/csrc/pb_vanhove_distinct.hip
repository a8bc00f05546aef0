// pb_vanhove_distinct.hip -- the distinct part of the van Hove function on gfx950: per member and lag, the radial
// histogram of the distances between where a bot was and where every OTHER bot is `lag` records later, over all ordered
// pairs and all time origins while pbSimStep runs (pbSimSetVanHoveDistinct / pbSimVanHoveDistinctRecord /
// pbSimGetVanHoveDistinct; include/particlebot_hip.h has the definitions).  The ring, its pairing and its book are the
// lag ring's (pb_engine.hpp); the filing, the walk over nine cells and the scratch are the analysis layer's
// (pb_cluster.hpp); the cell's words, the edges and the bin rules are pb_vanhove.hpp's.  None is restated here.
//
// A record is, on the batch's stream and without a wait:
//   pbClusterFile     the bots as they are now, filed on a wrapped grid of edge rMax (1 + 2^-10), rMax = bins qw 2^-20
//   k_vhd_snapshot    one pass over the filed cpr in SORTED order (coalesced 16-byte reads): (x, y) to
//                     ring[slot][original index], the NaNs of an absent bot already in place
//   k_vhd_accumulate  the hot path, one launch for all paired lags: grid (blocks of 256 sorted slots, member, lag).  The
//                     lane of sorted slot t stands for the bot o = bits(cpr[t].w) as it WAS: its centre is then[o] (an
//                     8-byte gather, the only uncoalesced read).  If the bot was present, the lane walks the nine cells
//                     around the cell of that earlier position over the current filing (pbWalkNine), so a bot that has
//                     moved by many cells still meets the bots that are now around its old place.  Every partner
//                     but the bot itself goes through an fp32 prefilter and then the exact integer rule; its bin gets 1
//                     in the workgroup's LDS histogram of 32-bit counters (4 KiB at most), which is flushed once into
//                     the cell's 64-bit counters with vector atomics, zeros skipped.  Bots present then and bots present
//                     now are counted once per bot and lag: wave sum, workgroup fold, one atomic each.
// WHY 32 BITS SUFFICE IN LDS.  As k_struct_rdf: a lane sends at most 2^23 adds of 1 into LDS and the rest straight to
// the global counter; 256 lanes x 2^23 = 2^31, so no LDS counter wraps whatever pile a member holds.
// Everything that is added is an integer: nothing depends on the slot order, on the kernel form that stepped or on the
// order of the adds.  No float atomics, no 128-bit atomics, no scratch memory.
#include <math.h>

#include <algorithm>

#include "pb_cluster.hpp"
#include "pb_fixed.hpp"
#include "pb_vanhove.hpp"

static_assert(sizeof(pbVanHoveDistinctRow) == 48, "a lag's row is 48 bytes");
static_assert(PB_VANHOVE_MAX_BINS * sizeof(uint32_t) == 4096, "the LDS histogram is 4 KiB");

// How the radial bin of a counted pair is found (pb_vanhove.hpp has all three; each is exact): 0 the self part's binary
// search in the LDS edges, 1 an fp32 first guess, sqrtf(d2) over the quantised width, corrected against the LDS edges
// until E_b <= s < E_(b + 1), 2 the integer square root and one division, which needs no edges in LDS.  The guess
// ships.  Measured on one MI355X, the 10^6-bot arena, 16 lags, 64 bins, rMax 5 / 10 radii, medians of 20 records into a
// full ring (tools/vanhove_distinct_cost.py; profiles/van_hove_distinct.txt, `form` rows): 1.37 / 4.39 ms per record
// against 2.03 / 6.74 ms for the search (six dependent LDS reads per pair) and 1.82 / 6.27 ms for the root (the fp64 root
// and two 64-bit products per pair).
#ifndef PB_VHD_BIN_RULE
#define PB_VHD_BIN_RULE 1
#endif
// 1: the active lanes of a wave that hit the first active lane's counter add once, by ballot, in front of the LDS atomic
// (one round of the self part's vhCount); 0: plain LDS atomics, which ship.  The self part's answer does not carry over:
// this histogram is broad (counts grow with r) and the lanes of a wave are in different trips of different ranges, so
// there is little to combine.  Same measurement: 1.59 / 5.23 ms with the ballot against 1.37 / 4.39 ms without.
#ifndef PB_VHD_COMBINE
#define PB_VHD_COMBINE 0
#endif

namespace {

constexpr uint32_t VHD_LDS_ADDS_PER_LANE = 1u << 23;
constexpr uint32_t VHD_LDS_EDGES = PB_VHD_BIN_RULE == 2 ? 1u : PB_VANHOVE_MAX_BINS;

PB_DEV uint32_t bitsOf(float w) { return __float_as_uint(w); }

__global__ __launch_bounds__(CT) void k_vhd_snapshot(const float4 *__restrict__ cpr, uint32_t n, uint32_t total,
                                                     float2 *__restrict__ snap) {
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  if (l >= n) return;
  const float4 q = cpr[blockIdx.y * n + l];  // the batch is below 2^28 bots
  const uint32_t o = bitsOf(q.w);
  // (the filing writes every global original index once; were it not so, nothing is written outside the slot)
  if (o >= total) return;
  snap[o] = make_float2(q.x, q.y);  // an absent bot's (NaN, NaN), as k_cluster_gather left it
}

// one count into LDS counter `at`; with PB_VHD_COMBINE the active lanes that hit the first active lane's counter add once
PB_DEV void vhdCount(uint32_t *sHist, uint32_t at) {
#if PB_VHD_COMBINE
  const unsigned long long active = __ballot(1);
  const uint32_t leader = (uint32_t)__ffsll((long long)active) - 1u;
  const uint32_t key = (uint32_t)__shfl((int)at, (int)leader);
  const unsigned long long same = __ballot(at == key);
  if (at == key) {
    if ((threadIdx.x & 63u) == leader)
      __hip_atomic_fetch_add(sHist + key, (uint32_t)__popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return;
  }
#endif
  __hip_atomic_fetch_add(sHist + at, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(CT) void k_vhd_accumulate(const float4 *__restrict__ cpr, const uint32_t *__restrict__ start,
                                                       const float2 *__restrict__ ring, uint32_t n, uint32_t total,
                                                       uint32_t lags, uint32_t slotNow, ClusterGrid G, float d2max,
                                                       float invWidth, uint32_t qw, uint32_t bins,
                                                       const unsigned long long *__restrict__ edges,
                                                       unsigned long long *__restrict__ table) {
  __shared__ unsigned long long sEdge[VHD_LDS_EDGES];  // sEdge[k - 1] = E_k, k = 1 ... bins (rules 0 and 1)
  __shared__ uint32_t sHist[PB_VANHOVE_MAX_BINS];
  __shared__ unsigned long long sRed[CT / 64][PB_VHD_HEAD];
  const uint32_t member = blockIdx.y, lag = blockIdx.z;  // lag < the lags this record is paired with <= lags
  const uint32_t slotThen = slotNow >= lag ? slotNow - lag : slotNow + lags - lag;
  const float2 *__restrict__ then = ring + (size_t)slotThen * total;  // indexed by the GLOBAL original index
  unsigned long long *__restrict__ cell = table + ((size_t)member * lags + lag) * pbVhdCellWords(bins);
  unsigned long long *__restrict__ mine = cell + PB_VHD_HEAD;
  const unsigned long long eBins = edges[bins];  // (bins qw)^2 < 2^62: a pair is counted iff s is below it
#if PB_VHD_BIN_RULE != 2
  for (uint32_t j = threadIdx.x; j < bins; j += CT) sEdge[j] = edges[j + 1u];
#endif
  for (uint32_t j = threadIdx.x; j < bins; j += CT) sHist[j] = 0u;  // bins <= PB_VANHOVE_MAX_BINS: the setter's check
  __syncthreads();
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  const bool live = l < n;  // (no early return: every lane meets the barriers)
  const uint32_t t = member * n + (live ? l : 0u);
  const float4 here = cpr[t];
  const uint32_t o = bitsOf(here.w);
  unsigned long long a[PB_VHD_HEAD] = {0ull, 0ull};
  if (live && o < total) {
    a[PB_VHD_PARTNERS] = here.x == here.x ? 1ull : 0ull;  // present now: the filing's rule (k_cluster_gather)
    const float2 p = then[o];
    if (p.x == p.x) {  // present then: the snapshot holds the filing's NaNs
      a[PB_VHD_CENTRES] = 1ull;
      uint32_t ldsAdds = 0u;
      [[maybe_unused]] const auto edgeAt = [&](uint32_t k) { return sEdge[k - 1u]; };
      // Cheap rejection in front of the exact rule.  The walk's rx, ry are the rule's dx, dy bit for bit (fp32
      // differences without contraction) and d2 = fl(fl(rx rx) + fl(ry ry)).  A counted pair has s = qx^2 + qy^2 < R^2
      // with R = bins qw, so sqrt(s) < R.  rx 2^20 is exact and |rx 2^20 - qx| <= 1/2, likewise y, hence
      //   (rx^2 + ry^2) 2^40 <= (|qx| + 1/2)^2 + (|qy| + 1/2)^2 = s + |qx| + |qy| + 1/2 <= s + sqrt(2 s) + 1/2
      //                      < (sqrt(s) + 1)^2 < (R + 1)^2,
      // and three fp32 roundings raise d2 by at most (1 + 2^-24)^2 (an underflow only lowers it):
      // d2 < ((R + 1) 2^-20)^2 (1 + 2^-22).  The host's d2max = r1 r1 1.0001f + 1e-30f with r1 = fl((R + 1) 2^-20) is
      // above that: its own three roundings lose less than 2^-22 relative against the 2^-14 that 1.0001 adds, and
      // r1 >= 2^-19 squares to a normal number.  So every counted pair is admitted; whatever else is admitted the exact
      // rule decides.  A partner that is absent now has a NaN position and a NaN d2, which fails the comparison.
      pbWalkNine<false>(cpr, start, member, G, t, make_float4(p.x, p.y, 0.0f, 0.0f),
                        [&](uint32_t, const float4 &q, float rx, float ry, float d2) {
        if (d2 <= d2max && bitsOf(q.w) != o) {  // the self pair is excluded by the index, wherever the others are
          if (pbFixedInRange(rx) && pbFixedInRange(ry)) {
            const long long qx = pbFixedQuantise(rx), qy = pbFixedQuantise(ry);
            const unsigned long long s = (unsigned long long)(qx * qx + qy * qy);  // below 2^63
            if (s < eBins) {
#if PB_VHD_BIN_RULE == 0
              const uint32_t b = pbVhRadialBin(edgeAt, bins, s);
#elif PB_VHD_BIN_RULE == 1
              const uint32_t b = pbVhRadialBinFrom(edgeAt, bins, s, (uint32_t)(int)(sqrtf(d2) * invWidth));
#else
              const uint32_t b = pbVhRadialBinRoot(qw, s);
#endif
              if (ldsAdds < VHD_LDS_ADDS_PER_LANE) {
                ldsAdds++;
                vhdCount(sHist, b);
              } else {
                __hip_atomic_fetch_add(mine + b, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              }
            }
          }
        }
      });
    }
  }
  (void)invWidth, (void)qw;
  __syncthreads();  // the workgroup's histogram is complete
  for (uint32_t j = threadIdx.x; j < bins; j += CT) {
    const uint32_t c = sHist[j];
    if (c) (void)__hip_atomic_fetch_add(mine + j, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // bots present then and bots present now: the wave's sums, the four waves through LDS, one atomic each
  waveSumRolled(a, [](int) {});
  unsigned long long v;
  if (!blockFold(sRed, a, [](uint32_t) { return PB_FOLD_SUM; }, v)) return;
  if (v) atomicAdd(cell + threadIdx.x, v);
}

}  // namespace

int pbVanHoveDistinctRecord(pbSim *S) {
  PbVanHoveDistinct &V = S->vd;
  // R = bins qw < 2^31 is exact in a double and so is rMax = R 2^-20, the reach the bots are filed with: a counted pair
  // has |dx|, |dy| < rMax and is never more than one cell apart (k_struct_rdf's grid).  No read-back: nothing waits.
  const double R = (double)((unsigned long long)V.qw * V.bins);
  int filed = PB_OK;
  const int rc = pbLagRecord(S, V.lag, [&](dim3 grid, float2 *snap) {
    filed = pbClusterFile(S, R / 1048576.0, 0.0);
    if (filed != PB_OK) return;
    hipLaunchKernelGGL(k_vhd_snapshot, grid, dim3(CT), 0, S->stream, S->cluster->cpr, S->n, S->total, snap);
  }, [&](dim3, uint32_t slot, uint32_t nLags, uint32_t) {
    if (filed != PB_OK) return;
    const PbClusterScratch *C = S->cluster;
    const float r1 = (float)((R + 1.0) / 1048576.0);
    hipLaunchKernelGGL(k_vhd_accumulate, dim3(cdiv(S->n, CT), S->nsims, nLags), dim3(CT), 0, S->stream, C->cpr, C->start,
                       V.lag.ring, S->n, S->total, V.lag.book.lags, slot, gridOf(C), r1 * r1 * 1.0001f + 1e-30f,
                       1048576.0f / (float)V.qw, V.qw, V.bins, V.edges, V.lag.table);  // (1 / the QUANTISED width)
  });
  return filed != PB_OK ? filed : rc;
}

extern "C" {

int pbSimSetVanHoveDistinct(pbSim *S, float interval, unsigned lags, float binWidth, unsigned bins) {
  const char *fn = "pbSimSetVanHoveDistinct";
  if (!S) return pbFail(fn, ": null handle");
  if (const int rc = pbLagCheckArgs(fn, interval, lags)) return rc;
  uint32_t qw = 0u;
  if (lags) {  // (lags == 0 switches off: the width and the bins are not read)
    if (bins < 1u || bins > PB_VANHOVE_MAX_BINS) return pbFail(fn, ": bins must be 1 ... 1024");
    if (!(binWidth > 0.0f) || !pbFixedInRange(binWidth)) return pbFail(fn, ": binWidth must be in (0, 2048)");
    qw = (uint32_t)pbFixedQuantise(binWidth);
    if (qw < 1u) return pbFail(fn, ": binWidth must be at least one quantum of 2^-20");
    if ((unsigned long long)qw * bins >= (1ull << 31))
      return pbFail(fn, ": bins x binWidth must be below 2048 (rint(binWidth 2^20) x bins < 2^31)");
  }
  if (const int rc = pbLagCheckBatch<float2>(fn, S, lags)) return rc;
  if (lags && (unsigned long long)S->nsims * lags * pbVhdCellWords(bins) * sizeof(unsigned long long) > (1ull << 31))
    return pbFail(fn, ": the table (members x lags x (2 + bins) x 8 bytes) must not exceed 2^31 bytes");
  return pbLagSwitch(S, S->vd, interval, lags, pbVhdCellWords(bins), [&](PbVanHoveDistinct &V) -> int {
    V.width = binWidth, V.qw = qw, V.bins = bins;
    std::vector<unsigned long long> host((size_t)bins + 1u);
    pbVhEdges(qw, bins, host.data());
    PB_TRY(V.edges.alloc(host.size()));
    PB_TRY(hipMemcpyAsync(V.edges, host.data(), sizeof(unsigned long long) * host.size(), hipMemcpyHostToDevice,
                          S->stream));
    PB_TRY(hipStreamSynchronize(S->stream));  // (the copy reads host memory that goes with this call)
    return pbClusterEnsureScratch(S);         // a record files the bots: it finds the shared scratch made
  });
}

int pbSimVanHoveDistinctRecord(pbSim *S) {
  return pbLagManualRecord("pbSimVanHoveDistinctRecord", S, &pbSim::vd, "distinct van Hove function",
                           pbVanHoveDistinctRecord);
}

int pbSimGetVanHoveDistinctInfo(pbSim *S, float *interval, unsigned *lags, float *binWidth, unsigned *bins,
                                unsigned long long *records) {
  if (!S) return pbFail("pbSimGetVanHoveDistinctInfo", ": null handle");
  if (!interval && !lags && !binWidth && !bins && !records)
    return pbFail("pbSimGetVanHoveDistinctInfo", ": interval, lags, binWidth, bins and records are all null");
  if (interval) *interval = S->vd.lag.interval;
  if (lags) *lags = S->vd.lag.book.lags;
  if (binWidth) *binWidth = S->vd.width;
  if (bins) *bins = S->vd.bins;
  if (records) *records = S->vd.lag.book.records;
  return PB_OK;
}

int pbSimGetVanHoveDistinct(pbSim *S, pbVanHoveDistinctRow *rows, unsigned long long *counts) {
  const char *fn = "pbSimGetVanHoveDistinct";
  if (!S || (!rows && !counts)) return pbFail(fn, ": null handle, or rows and counts both null");
  const PbVanHoveDistinct &V = S->vd;
  const PbLagBook &book = V.lag.book;
  const size_t words = pbVhdCellWords(V.bins);
  std::vector<unsigned long long> acc;
  if (const int rc = pbLagFetch(fn, S, V.lag, "distinct van Hove function", acc, PB_VHD_CENTRES, words)) return rc;
  for (size_t k = 0; k < (size_t)S->nsims * book.lags; k++) {
    const unsigned long long *w = &acc[k * words];
    if (counts) std::copy(w + PB_VHD_HEAD, w + words, counts + k * V.bins);
    if (!rows) continue;
    pbVanHoveDistinctRow &r = rows[k];
    book.columns((unsigned)(k % book.lags), r);
    r.reserved = 0u, r.centres = w[PB_VHD_CENTRES], r.partners = w[PB_VHD_PARTNERS], r.pairs = 0ull;
    for (size_t j = PB_VHD_HEAD; j < words; j++) r.pairs += w[j];
  }
  return PB_OK;
}

int pbSimGetVanHoveDistinctTimes(pbSim *S, unsigned long long *records, float *last_device_ms) {
  return pbLagTimes("pbSimGetVanHoveDistinctTimes", S, &pbSim::vd, records, last_device_ms);
}

}  // extern "C"
