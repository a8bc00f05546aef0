// pb_bonds.hip -- bond dynamics on gfx950: per member and lag, over all time origins while pbSimStep runs, how many of a
// bot's links survive (the bond-breaking correlation) and how far a bot moves RELATIVE TO THE NEIGHBOURS IT HAD (the
// cage-relative displacement), beside the plain displacement of the same bots (pbSimSetBondDynamics /
// pbSimBondDynamicsRecord / pbSimGetBondDynamics; include/particlebot_hip.h has the definitions).  The ring, its pairing
// and its book are the lag ring's (pb_engine.hpp); the filing, the walk over nine cells and the link rule are the
// analysis layer's (pb_cluster.hpp); the presence rule, the sort network, the intersection, the cage vector, the overlap
// and the cell's words are pb_bonds.hpp's.  None is restated here.
//
// A record is, on the batch's stream and without a wait:
//   pbClusterFile    the bots as they are now, filed on a wrapped grid of edge (2 maxRadius + linkGap)(1 + 2^-10): no
//                    read-back of the device's largest radius, and every accepted pair is at most one cell apart
//   k_bond_snapshot  one lane per bot in FILED order: the walk and the link rule with the presence test on both ends; the
//                    first eight accepted neighbours' member-local original indices sit in eight named registers, a
//                    fixed network sorts them, and the head (qx, qy, degree, 0) and the list leave as three 16-byte
//                    stores to ring[slot][member n + orig].  (The filed posrad of a present bot is the state arrays' bit
//                    for bit: the filing only replaces the position of a bot that is non-finite, which is absent.)
//   k_bond_pairs     the hot path, all paired lags in one launch: at most PB_BOND_BLOCKS workgroups of 256 lanes per
//                    (member, lag) through pbLagPair.  A lane loads both heads and both lists of its bot (coalesced
//                    16-byte loads), intersects the lists in registers, and gathers head_then[j] and head_now[j] of its
//                    up to eight earlier neighbours from the dense 16-byte array: the 2 k random gathers are its cost.
//                    The scalar columns are summed per lane, then over the wave; the per-k columns go straight into the
//                    workgroup's copy of the cell in LDS (336 bytes) with 64-bit integer atomics, so that no register is
//                    ever indexed by k; at the end one global 64-bit atomic per workgroup and non-zero word.
// Everything that is added is an integer: nothing depends on the slot order, on the kernel form that stepped or on the
// order of the adds.  No float atomics, no atomic wider than 64 bits, no scratch memory, no private array.
#include <limits.h>
#include <math.h>

#include "pb_bonds.hpp"
#include "pb_cluster.hpp"
#include "pb_fixed.hpp"

static_assert(sizeof(pbBondRow) == 360, "a lag's row is 360 bytes");
static_assert(PB_BOND_WIDTH == 8u, "eight named registers, a network of eight, two 16-byte words");
static_assert(CT == PB_LAG_LANES, "the filing's and the lag ring's workgroups are the same 256 lanes");

namespace {

constexpr const char *WHAT = "bond recorder";

// what the range check of the ring is taken on: a head and a list per bot and slot
struct PbBondEntry {
  int4 head;
  uint4 list[2];
};
static_assert(sizeof(PbBondEntry) == 48, "a bot and slot cost 48 bytes");

PB_DEV PbBondList listOf(const uint4 &a, const uint4 &b) { return {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}; }

__global__ __launch_bounds__(CT) void k_bond_snapshot(const float4 *__restrict__ cpr, const uint32_t *__restrict__ start,
                                                      uint32_t n, ClusterGrid G, float gap, float maxRadius,
                                                      int4 *__restrict__ heads, uint4 *__restrict__ lists) {
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  if (l >= n) return;
  const uint32_t member = blockIdx.y, base = member * n, t = base + l;  // the batch is below 2^28 bots
  const float4 me = cpr[t];
  const uint32_t o = __float_as_uint(me.w) - base;
  // (a layout is a permutation of 0 .. n - 1; were it not, nothing is written outside the member's block: k_tc_snapshot)
  if (o >= n) return;
  PbBondList e = {PB_BOND_NONE, PB_BOND_NONE, PB_BOND_NONE, PB_BOND_NONE,
                  PB_BOND_NONE, PB_BOND_NONE, PB_BOND_NONE, PB_BOND_NONE};
  uint32_t deg = 0u;
  int4 head = make_int4(PB_BOND_ABSENT, 0, 0, 0);
  if (pbBondPresent(me.x, me.y, me.z, maxRadius)) {
    pbWalkNine<false>(cpr, start, member, G, t, me, [&](uint32_t j, const float4 &q, float, float, float d2) {
      pbWhenLinked(t, me, j, q, d2, gap, [&](float, float) {
        if (pbBondPresent(q.x, q.y, q.z, maxRadius)) {
          const uint32_t oj = __float_as_uint(q.w) - base;
          e.e0 = deg == 0u ? oj : e.e0, e.e1 = deg == 1u ? oj : e.e1, e.e2 = deg == 2u ? oj : e.e2;
          e.e3 = deg == 3u ? oj : e.e3, e.e4 = deg == 4u ? oj : e.e4, e.e5 = deg == 5u ? oj : e.e5;
          e.e6 = deg == 6u ? oj : e.e6, e.e7 = deg == 7u ? oj : e.e7;
          deg++;
        }
      });
    });
    pbBondSort(e);
    head = make_int4((int)pbFixedQuantise(me.x), (int)pbFixedQuantise(me.y), (int)deg, 0);
  }
  const size_t at = (size_t)base + o;
  heads[at] = head;
  lists[2u * at] = make_uint4(e.e0, e.e1, e.e2, e.e3);
  lists[2u * at + 1u] = make_uint4(e.e4, e.e5, e.e6, e.e7);
}

__global__ __launch_bounds__(CT) void k_bond_pairs(const int4 *__restrict__ ring, const uint4 *__restrict__ lists,
                                                   uint32_t n, uint32_t total, uint32_t lags, uint32_t slotNow,
                                                   uint32_t nLags, uint32_t blocksPerLag, long long qa,
                                                   unsigned long long *__restrict__ table) {
  __shared__ unsigned long long sCell[PB_BOND_WORDS];  // the workgroup's copy of the cell
  const PbLagPair<int4> pair = pbLagPair(ring, n, total, lags, slotNow, nLags, blocksPerLag);
  const uint32_t member = pair.member, lag = pair.lag, b = pair.block;
  const int4 *__restrict__ now = pair.now, *__restrict__ then = pair.then;
  // the lists lie beside the heads, two 16-byte words per entry
  const uint4 *__restrict__ listNow = lists + 2u * (size_t)(now - ring);
  const uint4 *__restrict__ listThen = lists + 2u * (size_t)(then - ring);
  if (threadIdx.x < (uint32_t)PB_BOND_WORDS) sCell[threadIdx.x] = 0ull;
  __syncthreads();
  // a lane meets at most 2^28 / (256 x 256) = 4096 bots of at most eight bonds: 32-bit counts do
  uint32_t cSamples = 0u, cCrowded = 0u, cThen = 0u, cNow = 0u, cKept = 0u, cUnchanged = 0u, cLost = 0u, cGained = 0u;
  unsigned long long plainLo = 0ull, plainHi = 0ull;
#pragma unroll 1
  for (uint32_t i = b * CT + threadIdx.x; i < n; i += blocksPerLag * CT) {
    const int4 hn = now[i], ht = then[i];
    const uint4 n0 = listNow[2u * (size_t)i], n1 = listNow[2u * (size_t)i + 1u];
    const uint4 t0 = listThen[2u * (size_t)i], t1 = listThen[2u * (size_t)i + 1u];
    if (hn.x == PB_BOND_ABSENT || ht.x == PB_BOND_ABSENT) continue;
    const uint32_t w = (uint32_t)hn.z, t = (uint32_t)ht.z;
    if (w > PB_BOND_WIDTH || t > PB_BOND_WIDTH) {  // crowded at either record: it takes part in nothing else
      cCrowded++;
      continue;
    }
    const PbBondList ln = listOf(n0, n1), lt = listOf(t0, t1);
    const uint32_t kept = pbBondKept(lt, ln);
    cSamples++, cThen += t, cNow += w, cKept += kept;
    cUnchanged += kept == t && kept == w ? 1u : 0u;
    cLost += kept < t ? 1u : 0u, cGained += kept < w ? 1u : 0u;
    if (t == 0u) continue;  // no cage
    // the earlier neighbours' displacements: every one must be present now (and, the ring being what it is, then)
    long long sumX = 0ll, sumY = 0ll;
    bool all = true;
    const auto gather = [&](uint32_t j) __attribute__((always_inline)) {
      if (j == PB_BOND_NONE) return;
      if (j >= n) {  // (never: the snapshot stores indices of the member; a stale entry gathers nothing out of bounds)
        all = false;
        return;
      }
      const int4 a = then[j], z = now[j];
      all = all && a.x != PB_BOND_ABSENT && z.x != PB_BOND_ABSENT;
      sumX += (long long)z.x - (long long)a.x, sumY += (long long)z.y - (long long)a.y;
    };
    gather(lt.e0), gather(lt.e1), gather(lt.e2), gather(lt.e3);
    gather(lt.e4), gather(lt.e5), gather(lt.e6), gather(lt.e7);
    const long long dqx = (long long)hn.x - (long long)ht.x, dqy = (long long)hn.y - (long long)ht.y;
    unsigned long long s;
    if (!all || !pbBondCage(t, dqx, dqy, sumX, sumY, s)) continue;
    unsigned long long lo, hi;
    pbBondPlainSplit(dqx, dqy, lo, hi);
    plainLo += lo, plainHi += hi;
    const uint32_t k = t - 1u;  // 0 ... 7: an LDS address, not a register index
    __hip_atomic_fetch_add(sCell + PB_BOND_CAGE_SAMPLES + k, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (pbBondOverlaps(s, t, qa))
      __hip_atomic_fetch_add(sCell + PB_BOND_CAGE_OVERLAP + k, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (s) {
      __hip_atomic_fetch_add(sCell + PB_BOND_CAGE_LO + k, pbFixedLow(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(sCell + PB_BOND_CAGE_HI + k, pbFixedRest(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  // the scalar columns: the wave's sums, then one lane per wave into the workgroup's cell
  cSamples = waveSumU32(cSamples), cCrowded = waveSumU32(cCrowded), cThen = waveSumU32(cThen), cNow = waveSumU32(cNow);
  cKept = waveSumU32(cKept), cUnchanged = waveSumU32(cUnchanged), cLost = waveSumU32(cLost), cGained = waveSumU32(cGained);
  plainLo = waveSumU64(plainLo), plainHi = waveSumU64(plainHi);
  if ((threadIdx.x & 63u) == 0u) {
    const auto add = [&](int word, unsigned long long v) __attribute__((always_inline)) {
      if (v) __hip_atomic_fetch_add(sCell + word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    add(PB_BOND_SAMPLES, cSamples), add(PB_BOND_CROWDED, cCrowded), add(PB_BOND_THEN, cThen), add(PB_BOND_NOW, cNow);
    add(PB_BOND_KEPT, cKept), add(PB_BOND_UNCHANGED, cUnchanged), add(PB_BOND_LOST, cLost), add(PB_BOND_GAINED, cGained);
    add(PB_BOND_PLAIN_LO, plainLo), add(PB_BOND_PLAIN_HI, plainHi);
  }
  __syncthreads();  // the workgroup's cell is complete
  if (threadIdx.x < (uint32_t)PB_BOND_WORDS) {
    const unsigned long long v = sCell[threadIdx.x];
    if (v)
      (void)__hip_atomic_fetch_add(table + ((size_t)member * lags + lag) * PB_BOND_WORDS + threadIdx.x, v,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace

int pbBondDynamicsRecord(pbSim *S) {
  PbBondDynamics &B = S->bd;
  int filed = PB_OK;
  const int rc = pbLagRecord(S, B.lag, [&](dim3 grid, int4 *heads) {
    // the reach does not depend on the device's largest radius: nothing is read back and nothing waits
    filed = pbClusterFile(S, 2.0 * (double)B.maxRadius + (double)B.gap, 0.0);
    if (filed != PB_OK) return;
    const PbClusterScratch *C = S->cluster;
    const int4 *first = B.lag.ring;
    uint4 *lists = B.lists + 2u * (size_t)(heads - first);
    hipLaunchKernelGGL(k_bond_snapshot, grid, dim3(CT), 0, S->stream, C->cpr, C->start, S->n, gridOf(C), B.gap,
                       B.maxRadius, heads, lists);
  }, [&](dim3 grid, uint32_t slot, uint32_t nLags, uint32_t bpl) {
    if (filed != PB_OK) return;
    hipLaunchKernelGGL(k_bond_pairs, grid, dim3(CT), 0, S->stream, B.lag.ring, B.lists, S->n, S->total, B.lag.book.lags,
                       slot, nLags, bpl, B.qa, B.lag.table);
  });
  return filed != PB_OK ? filed : rc;
}

extern "C" {

int pbSimSetBondDynamics(pbSim *S, float interval, unsigned lags, float linkGap, float maxRadius, float overlapRadius) {
  const char *fn = "pbSimSetBondDynamics";
  if (!S) return pbFail(fn, ": null handle");
  if (const int rc = pbLagCheckArgs(fn, interval, lags)) return rc;
  if (lags) {  // (lags == 0 switches off: the gap and the radii are not read)
    const float inf = __builtin_inff();
    if (!(linkGap >= 0.0f && linkGap < inf)) return pbFail(fn, ": linkGap must be finite and >= 0");
    if (!(maxRadius > 0.0f && maxRadius < inf)) return pbFail(fn, ": maxRadius must be finite and > 0");
    if (!(2.0 * (double)maxRadius + (double)linkGap < 2048.0))
      return pbFail(fn, ": 2 maxRadius + linkGap must be below 2048");
    if (!(overlapRadius >= 0.0f && overlapRadius < 256.0f)) return pbFail(fn, ": overlapRadius must be in [0, 256)");
  }
  if (const int rc = pbLagCheckBatch<PbBondEntry>(fn, S, lags)) return rc;
  return pbLagSwitch(S, S->bd, interval, lags, PB_BOND_WORDS, [&](PbBondDynamics &B) -> int {
    B.gap = linkGap, B.maxRadius = maxRadius, B.radius = overlapRadius;
    B.qa = pbBondRadiusQuanta(overlapRadius);  // 8 qa < 2^31
    PB_TRY(B.lists.alloc(2u * (size_t)lags * S->total));
    return pbClusterEnsureScratch(S);  // a record files the bots: it finds the shared scratch made
  });
}

int pbSimBondDynamicsRecord(pbSim *S) {
  return pbLagManualRecord("pbSimBondDynamicsRecord", S, &pbSim::bd, WHAT, pbBondDynamicsRecord);
}

int pbSimGetBondDynamicsInfo(pbSim *S, float *interval, unsigned *lags, float *linkGap, float *maxRadius,
                             float *overlapRadius, unsigned long long *records) {
  const char *fn = "pbSimGetBondDynamicsInfo";
  if (!S) return pbFail(fn, ": null handle");
  if (!interval && !lags && !linkGap && !maxRadius && !overlapRadius && !records)
    return pbFail(fn, ": interval, lags, linkGap, maxRadius, overlapRadius and records are all null");
  if (interval) *interval = S->bd.lag.interval;
  if (lags) *lags = S->bd.lag.book.lags;
  if (linkGap) *linkGap = S->bd.gap;
  if (maxRadius) *maxRadius = S->bd.maxRadius;
  if (overlapRadius) *overlapRadius = S->bd.radius;
  if (records) *records = S->bd.lag.book.records;
  return PB_OK;
}

int pbSimGetBondDynamics(pbSim *S, pbBondRow *rows) {
  const char *fn = "pbSimGetBondDynamics";
  if (!S || !rows) return pbFail(fn, ": null handle or rows");
  const PbLagBook &book = S->bd.lag.book;
  std::vector<unsigned long long> acc;
  // (crowded bots are beside the samples: with them a cell could hold more bots than samples, but every sum is over samples)
  if (const int rc = pbLagFetch(fn, S, S->bd.lag, WHAT, acc, PB_BOND_SAMPLES, PB_BOND_WORDS)) return rc;
  for (size_t g = 0; g < (size_t)S->nsims * book.lags; g++) {
    const unsigned long long *w = &acc[g * PB_BOND_WORDS];
    pbBondRow &r = rows[g];
    book.columns((unsigned)(g % book.lags), r);
    r.reserved = 0u, r.samples = w[PB_BOND_SAMPLES], r.crowded = w[PB_BOND_CROWDED];
    r.bonds_then = w[PB_BOND_THEN], r.bonds_now = w[PB_BOND_NOW], r.bonds_kept = w[PB_BOND_KEPT];
    r.bots_unchanged = w[PB_BOND_UNCHANGED], r.bots_lost = w[PB_BOND_LOST], r.bots_gained = w[PB_BOND_GAINED];
    r.plain_q2 = pbFixedNormalised(pbBondPlain(w[PB_BOND_PLAIN_LO], w[PB_BOND_PLAIN_HI]));
    for (unsigned k = 0; k < PB_BOND_WIDTH; k++) {
      r.cage_samples[k] = w[PB_BOND_CAGE_SAMPLES + k], r.cage_overlap[k] = w[PB_BOND_CAGE_OVERLAP + k];
      r.cage_q2[k] = pbFixedNormalised(pbFixedCompose(w[PB_BOND_CAGE_LO + k], w[PB_BOND_CAGE_HI + k]));
    }
  }
  return PB_OK;
}

int pbSimGetBondDynamicsTimes(pbSim *S, unsigned long long *records, float *last_device_ms) {
  return pbLagTimes("pbSimGetBondDynamicsTimes", S, &pbSim::bd, records, last_device_ms);
}

}  // extern "C"
