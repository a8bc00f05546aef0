// pb_cluster.hpp -- what pb_cluster.hip shares with pb_contacts.hip, pb_structure.hip, pb_dynamics.hip, pb_strain.hip and
// pb_correlate.hip and pb_vanhove_distinct.hip: the scratch object with its five clocks, the fresh grid, the workgroup
// scan (the wave helpers are pb_fixed.hpp's), the walk over a bot's nine cells (pbWalkNine) and the link rule (pbWhenLinked) that every neighbour
// sweep of the analysis layer is built on, the front end that files the bots (rmax, hash, sort, gather, cell starts) and
// the argument checks of the entry points.
#pragma once

#include "pb_engine.hpp"
#include "pb_fixed.hpp"

// One analysis' clock: it starts at the front end's ev0 and ends at an event of its own (pbClockStop).
struct PbAnalysisClock {
  PbEvent end;  // behind the analysis' last launch; created by the first stop
  unsigned long long runs = 0;
  float lastMs = 0.0f;
};

// Every buffer is an owner: the scratch goes with `delete` (pbClusterFree).
struct PbClusterScratch {
  PbDevBuf<uint32_t> keys[2], vals[2], hist;
  PbDevBuf<float4> cpr;        // total + 2: sorted posrad, .w = global original index
  PbDevBuf<uint32_t> start;    // nsims * cells + 1
  PbDevBuf<uint32_t> parent, degree, size;  // total each, ORIGINAL order
  PbDevBuf<uint32_t> labels;   // n: one member's labels
  PbDevBuf<unsigned long long> acc;  // 4 words per member
  PbDevBuf<pbClusterStats> rows;     // nsims
  PbDevBuf<uint32_t> flag;           // [0] changed, [1] rmax bits
  PbEvent ev0;                       // the front end's first launch: where every clock starts
  PbAnalysisClock clusterClock, contactClock, structureClock, dynamicsClock;
  uint32_t gxLog2 = 2, gyLog2 = 2;
  unsigned rounds = 0;
  // what the last analysis left behind for the contact export (pb_contacts.hip)
  double invCell = 0.0;  // the grid's 1 / edge
  int sortedIn = 0;      // vals[sortedIn] holds the slots in sorted order
  // contact export (pb_contacts.hip): allocated by the first export, links grown when a call needs more
  PbDevBuf<uint32_t> cOffsets;            // n + 1, ORIGINAL order
  PbDevBuf<unsigned long long> cParts;    // ceil(n / 256) + 2: block sums, then [blocks] the total, [blocks + 1] the flag
  PbDevBuf<float2> cVel;                  // n: the member's velocities in sorted order
  PbDevBuf<float2> cPos;                  // n: the member's positions in ORIGINAL order
  PbDevBuf<double> cVirial;               // 4 n, ORIGINAL order
  PbDevBuf<uint4> cLinks;                 // entries of 16 bytes (pbContactLink)
  // structure analysis (pb_structure.hip): allocated by the first call that needs each, counts grown with bins
  PbDevBuf<unsigned long long> sCounts;   // nsims * the most bins asked for so far: the radial histograms
  PbDevBuf<long long> sRe, sIm;           // total each, ORIGINAL order: per-bot sums of qre, qim
  PbDevBuf<uint32_t> sNb;                 // total, ORIGINAL order: neighbours
  PbDevBuf<pbStructureStats> sRows;       // nsims
  PbDevBuf<double> sPsi;                  // 2 n: one member's psi6
  // rearrangement analysis (pb_dynamics.hip).  The mark: allocated by the first pbSimMarkReference, entries grown when a
  // mark needs more, kept until pbSimClearReference
  bool dMarked = false;                   // a mark is held: everything below describes it
  float dGap = 0.0f, dTime = 0.0f;        // its linkGap and the batch's fp32 time when it was taken
  unsigned long long dEntries = 0;        // directed entries of the whole batch
  PbDevBuf<float2> dPos0;                 // total, ORIGINAL order: the marked positions, bit for bit
  PbDevBuf<uint32_t> dOffsets;            // total + 1, ORIGINAL order: the marked network's CSR over the whole batch
  PbDevBuf<uint32_t> dOther;              // `other`, member-local original index
  PbDevBuf<unsigned long long> dParts;    // ceil(total / 256) + 2: block sums, then the total, then the flag
  // the compare: allocated by the first one, kept
  PbDevBuf<uint32_t> dNow, dKept;         // total each, ORIGINAL order
  PbDevBuf<float2> dDisp;                 // total, ORIGINAL order: dx, dy
  PbDevBuf<pbRearrangementStats> dRows;   // nsims; sum_q2_lo / sum_q2_hi hold the two partial sums until the host
                                          // composes them
  // pair correlations (pb_correlate.hip): allocated by the first call, the bins' words grown with bins
  PbDevBuf<int2> kA;                      // total, SORTED order: the vector a, x = INT_MIN for an unmeasured bot
  PbDevBuf<unsigned long long> kAcc;      // nsims * the most bins so far * 9: per bin the count and eight partial sums
  PbDevBuf<unsigned long long> kTotals;   // nsims * 5: measured, sum ax, sum ay, the two partial sums of a^2
  PbAnalysisClock correlateClock;
  // strain analysis (pb_strain.hip): allocated by the first call, kept
  PbDevBuf<float2> tPos1;                 // total, ORIGINAL order: the present positions, raw from the state arrays
  PbDevBuf<long long> tMoments;           // 9 per bot, ORIGINAL order
  PbDevBuf<double> tD2;                   // total, ORIGINAL order: D2min
  PbDevBuf<pbStrainStats> tRows;          // nsims; every pbMoment128 holds the two partial sums until the host composes them
  PbSpanClock strainSpan;                 // no filing, so no ev0: the span is the analysis' own
  unsigned long long strainRuns = 0;
  float strainMs = 0.0f;
};

namespace {

constexpr int CT = 256;

struct ClusterGrid {
  double invCell;
  uint32_t gxLog2, gyLog2;
};

// the grid the last pbClusterFile left in the scratch object
inline ClusterGrid gridOf(const PbClusterScratch *C) {
  ClusterGrid G;
  G.invCell = C->invCell;
  G.gxLog2 = C->gxLog2, G.gyLog2 = C->gyLog2;
  return G;
}

PB_DEV bool finitePosRad(const float4 &q) {
  const float inf = __builtin_inff();
  return fabsf(q.x) < inf && fabsf(q.y) < inf && fabsf(q.z) < inf;
}

// floor(v) as an int, clamped so that positions outside the guaranteed range convert without overflow
PB_DEV int cellCoord(double v) {
  const double f = floor(v);
  return (int)fmin(fmax(f, -1073741824.0), 1073741824.0);
}

PB_DEV uint32_t cellX(const ClusterGrid &G, float x) {
  return (uint32_t)cellCoord((double)x * G.invCell) & ((1u << G.gxLog2) - 1u);
}
PB_DEV uint32_t cellY(const ClusterGrid &G, float y) {
  return (uint32_t)cellCoord((double)y * G.invCell) & ((1u << G.gyLog2) - 1u);
}

// exclusive prefix of v over the workgroup and the workgroup's total: an inclusive scan inside each wave with
// shuffles, the four wave totals through LDS.  Every lane of the workgroup must call it.
PB_DEV unsigned long long blockScanExclusive(unsigned long long v, unsigned long long *sWave,
                                             unsigned long long &blockTotal) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long up = shflUp64(incl, d);
    if (lane >= (uint32_t)d) incl += up;
  }
  if (lane == 63u) sWave[w] = incl;
  __syncthreads();
  unsigned long long before = 0ull, tot = 0ull;
#pragma unroll
  for (uint32_t k = 0; k < CT / 64; k++) {
    const unsigned long long s = sWave[k];
    before += k < w ? s : 0ull;
    tot += s;
  }
  __syncthreads();  // sWave may be written again
  blockTotal = tot;
  return before + incl - v;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------
// The neighbour sweep of one bot (sorted slot t, posrad me with a finite position, member `member` of the batch) over the
// nine cells around its own: three slot ranges of three cells each, and at the x-wrap (the own cell in the first or last
// column) nine ranges of one.  The wrapped dimensions are >= 4, so the nine cells are distinct and a pair is met once
// from each end however the grid folds.  The bounds of the range after the next and the first posrad of the next range
// are in flight while a range is walked, and so is the next slot's posrad inside a range (one slot past a range is
// inside the array: cpr has spare elements).  For every slot j of every range, the own one included,
// body(j, q, rx, ry, d2) gets the slot's posrad and rx = q.x - me.x, ry = q.y - me.y, d2 = rx*rx + ry*ry in fp32 without
// contraction.  BEHIND: only the slots behind the own one are walked (j > t), for a sweep that counts a pair at one end.
template <bool BEHIND, typename Body>
PB_DEV void pbWalkNine(const float4 *__restrict__ cpr, const uint32_t *__restrict__ start, uint32_t member,
                       const ClusterGrid &G, uint32_t t, const float4 &me, const Body &body) {
  const uint32_t GX = 1u << G.gxLog2;
  const uint32_t cx = cellX(G, me.x), cy = cellY(G, me.y);
  const uint32_t *__restrict__ cells = start + ((size_t)member << (G.gxLog2 + G.gyLog2));
  const bool wrap = cx == 0u || cx == GX - 1u;
  const uint32_t step = wrap ? 1u : 3u;
  auto bounds = [&](uint32_t si, uint32_t &lo, uint32_t &hi) __attribute__((always_inline)) {
    lo = hi = t;
    if (si < 9u) {
      const uint32_t rowI = si / 3u, col = si - 3u * rowI;
      const uint32_t row = ((cy + rowI - 1u) & ((1u << G.gyLog2) - 1u)) << G.gxLog2;
      const uint32_t c0 = (cx + col - 1u) & (GX - 1u);
      lo = cells[row + c0];
      hi = cells[row + c0 + step];
      if constexpr (BEHIND) {
        lo = lo > t ? lo : t + 1u;
        lo = lo < hi ? lo : hi;
      }
    }
  };
  uint32_t loA, hiA, loB, hiB;
  bounds(0u, loA, hiA);
  bounds(step, loB, hiB);
  float4 qA = cpr[loA];
#pragma unroll 1
  for (uint32_t si = 0u; si < 9u; si += step) {
    const uint32_t lo = loA, hi = hiA;
    float4 q = qA;
    loA = loB, hiA = hiB;
    qA = cpr[loA];                      // first posrad of the next range
    bounds(si + 2u * step, loB, hiB);   // bounds of the range after the next
    for (uint32_t j = lo; j < hi; j++) {
      const float4 qn = cpr[(size_t)j + 1u];  // (widened before the add: the address needs no 32-bit wrap)
      const float rx = q.x - me.x, ry = q.y - me.y;
      const float d2 = rx * rx + ry * ry;
      body(j, q, rx, ry, d2);
      q = qn;
    }
  }
}

// ---- the link rule -------------------------------------------------------------------------------------------------------
// then(dist, R) when the bots in sorted slots t (posrad me) and j (posrad q), d2 apart squared as the walk computes it,
// are linked at `gap`: two different slots with fl(dist - R) < gap, R = ri + rj and dist = sqrtf(d2), the pair law's
// geometry in fp32 without contraction (the stored gap is dist - R).  A bot is not linked to itself: j != t is part of
// the rule.  A continuation and not a bool, so that the root stays behind the rejection in the machine code: the
// compiler folds a returned `near && exact` into one test and takes the root for every pair.
// The cheap rejection in front of the correctly rounded root: a linked pair has fl(dist - R) < gap, hence
// dist - R <= gap exactly (rounding is monotone), dist <= fl(R + gap) (1 + 2^-23) and
// fl(rx*rx + ry*ry) <= fl(R + gap)^2 (1 + 2^-20): the bound below (1e-4 relative, 1e-30 absolute for the subnormal cases)
// admits every such pair; whatever else it admits the exact predicate decides.  A non-finite partner's position is NaN,
// which passes neither.
template <typename Then>
PB_DEV void pbWhenLinked(uint32_t t, const float4 &me, uint32_t j, const float4 &q, float d2, float gap,
                         const Then &then) {
  const float R = me.z + q.z;
  const float s = R + gap;
  if (j != t && d2 <= s * s * 1.0001f + 1e-30f) {
    const float dist = sqrtf(d2);
    if ((dist - R) < gap) then(dist, R);
  }
}

// ---- the clocks ----------------------------------------------------------------------------------------------------------
// The end of a run of the analysis K times, in two steps for a caller that queues something of its own in between:
// pbClockMark records K's end event (created here the first time) behind what the stream holds; pbClockRead drains the
// stream, takes the device time since the front end's ev0 and counts the run.  pbClockStop is both.
inline int pbClockMark(pbSim *S, PbAnalysisClock &K) {
  if (!K.end) PB_TRY(K.end.create());
  PB_TRY(hipEventRecord(K.end, S->stream));
  return PB_OK;
}
inline int pbClockRead(pbSim *S, PbAnalysisClock &K) {
  PB_TRY(hipStreamSynchronize(S->stream));
  PB_TRY(hipEventElapsedTime(&K.lastMs, S->cluster->ev0, K.end));
  K.runs++;
  return PB_OK;
}
inline int pbClockStop(pbSim *S, PbAnalysisClock &K) {
  const int rc = pbClockMark(S, K);
  return rc != PB_OK ? rc : pbClockRead(S, K);
}
// "no reference marked" is known without the device (pb_dynamics.hip holds the mark)
inline int pbNeedMark(const char *fn, const pbSim *S) {
  return S->cluster && S->cluster->dMarked ? PB_OK : pbFail(fn, ": no reference marked");
}
// the body of pbSimGet{Cluster,Contact,Structure,Rearrangement}Times; K points into S's scratch object
inline int pbClockGet(const char *fn, const pbSim *S, PbAnalysisClock PbClusterScratch::*K, unsigned long long *runs,
                      float *last_device_ms) {
  if (!S) return pbFail(fn, ": null handle");
  if (runs) *runs = S->cluster ? (S->cluster->*K).runs : 0ull;
  if (last_device_ms) *last_device_ms = S->cluster ? (S->cluster->*K).lastMs : 0.0f;
  return PB_OK;
}

}  // namespace

// The filing front end: records ev0, files every bot of the batch on a wrapped power-of-two grid of edge
// (perRmax * rmax + reach) (1 + 2^-10), never below 2^-8 (rmax: the largest finite radius, reduced on the device and
// read back only when perRmax != 0), and leaves cpr (sorted posrad, .w = global original index), the cell starts,
// vals[sortedIn], parent[o] = o and size[o] = 0 on the device, the grid (invCell, gxLog2, gyLog2) in the scratch object.
// Allocates the scratch on first use.  Launches are queued on the batch's stream, not waited for.       pb_cluster.hip
int pbClusterFile(pbSim *S, double reach, double perRmax);
// Makes the scratch pbClusterFile would make on first use, and nothing else: for a recorder that files inside the
// schedule, where nothing may allocate (pb_vanhove_distinct.hip).                                       pb_cluster.hip
int pbClusterEnsureScratch(pbSim *S);
// The whole cluster pipeline (the front end with reach = gap, perRmax = 2); leaves cpr, the cell starts, parent (roots),
// degree and the rows on the device and the stream drained.                                             pb_cluster.hip
int pbClusterAnalyse(pbSim *S, float gap);
// The argument checks the entry points of the analysis layer share after their own pointer checks, in this order:
// linkGap finite and >= 0 (when gap is given), member inside the batch (when member is given), the batch within what a
// launch can index.
// Nothing here touches the device; the gap check needs no look at the handle, the other two read the host-side batch
// object, so they need a real one.                                                                       pb_cluster.hip
int pbClusterCheckArgs(const char *fn, const pbSim *S, const float *gap, const unsigned *member);
// k_dyn_scatter's launch, queued on the batch's stream: the positions of the whole batch as they are now, raw from the
// state arrays, into ORIGINAL order at pos (total entries).  The mark's own pass, shared with the strain analysis.
//                                                                                                        pb_dynamics.hip
int pbDynamicsScatter(pbSim *S, float2 *pos);
// k_contact_scan's three launches, queued on the batch's stream: offsets[0 .. n] = the exclusive prefix sum of
// degree[0 .. n), parts (ceil(n / 256) + 1 words at the least) the scan's block sums with the 64-bit total in
// parts[ceil(n / 256)].  Offsets are 32-bit: the caller reads the total before it trusts them.         pb_contacts.hip
int pbContactScan(pbSim *S, const uint32_t *degree, uint32_t n, unsigned long long *parts, uint32_t *offsets);
