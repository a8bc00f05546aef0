// pb_dynamics.hip -- rearrangement analysis on gfx950: a marked reference held on the device, and one sweep that
// compares the link network and the positions of the resident state with it (pbSimMarkReference /
// pbSimRearrangementStats / pbSimRearrangementOf, include/particlebot_hip.h has the definitions).
//
// The front end is the cluster analysis' (pbClusterFile, pb_cluster.hip): the bots filed afresh on a wrapped
// power-of-two grid, the sorted posrad array, dense cell starts.  Mark and compare each re-file, at the mark's gap.
// The mark, for the whole batch at once (no union-find: pbClusterAnalyse does more than is needed):
//   k_dyn_count     every bot's degree under the link rule, ORIGINAL order (pbWalkNine and pbWhenLinked, pb_cluster.hpp,
//                   as k_struct_psi6 counts its neighbours)
//   k_contact_scan  (pb_contacts.hip, pbContactScan) the exclusive prefix sum over all `total` bots; the 8-byte total
//                   goes back to the host, which sizes the entries
//   k_dyn_fill      the same walk and rule; every accepted neighbour's member-local original index at offsets[o] + k.
//                   The store is guarded by offsets[o + 1], and a lane whose count differs from its degree raises a
//                   flag: the host reports it and holds no mark
//   k_dyn_order     one lane per bot: insertion sort of its 4-byte entries in place (about 6 at contact gaps)
//   k_dyn_scatter   the positions into ORIGINAL order, from the state arrays themselves: the front end's sorted copy
//                   holds NaN for a bot with a non-finite radius, and the mark keeps every position bit for bit
// The compare:
//   k_dyn_compare   one bot per lane in sorted order over the whole batch (a workgroup may straddle members).  The
//                   bot's share of the marked CSR and its marked position are requested before the walk.  Every
//                   neighbour the link rule accepts counts for `now` and is looked up in the bot's marked list: a list
//                   of up to 8 entries sits in eight registers (compared one by one, no indexing), a longer one is
//                   searched by bisection in global memory.  now, kept, dx, dy are stored in ORIGINAL order; the
//                   members' rows are reduced with wave shuffles and ballots, the four waves through LDS, then one set
//                   of integer atomics per workgroup and member.
// Everything that is added is an integer: nothing depends on the order of the adds.  No float atomics, no scratch
// memory, no private array.
#include <string.h>

#include <vector>

#include "pb_cluster.hpp"

static_assert(sizeof(pbRearrangementStats) == 80, "a member's row is 80 bytes");

namespace {

__global__ __launch_bounds__(CT) void k_dyn_count(const float4 *__restrict__ cpr, const uint32_t *__restrict__ start,
                                                  uint32_t n, ClusterGrid G, float gap, uint32_t *__restrict__ degree) {
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  if (l >= n) return;
  const uint32_t t = blockIdx.y * n + l;
  const float4 me = cpr[t];
  uint32_t deg = 0u;
  if (me.x == me.x) {  // a bot with a non-finite position or radius has no links
    pbWalkNine<false>(cpr, start, blockIdx.y, G, t, me, [&](uint32_t j, const float4 &q, float, float, float d2) {
      pbWhenLinked(t, me, j, q, d2, gap, [&](float, float) { deg++; });
    });
  }
  degree[__float_as_uint(me.w)] = deg;
}

__global__ __launch_bounds__(CT) void k_dyn_fill(const float4 *__restrict__ cpr, const uint32_t *__restrict__ start,
                                                 uint32_t n, ClusterGrid G, float gap,
                                                 const uint32_t *__restrict__ offsets, uint32_t *__restrict__ other,
                                                 unsigned long long *__restrict__ flag) {
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  if (l >= n) return;
  const uint32_t base = blockIdx.y * n, t = base + l;
  const float4 me = cpr[t];
  const uint32_t o = __float_as_uint(me.w);
  const uint32_t first = offsets[o], end = offsets[o + 1u];
  uint32_t k = 0u;
  if (me.x == me.x) {
    pbWalkNine<false>(cpr, start, blockIdx.y, G, t, me, [&](uint32_t j, const float4 &q, float, float, float d2) {
      pbWhenLinked(t, me, j, q, d2, gap, [&](float, float) {
        if (first + k < end)  // never outside this bot's share of the buffer, whatever the count pass said
          other[first + k] = __float_as_uint(q.w) - base;
        k++;
      });
    });
  }
  if (k != end - first) __atomic_store_n(flag, 1ull, __ATOMIC_RELAXED);
}

__global__ __launch_bounds__(CT) void k_dyn_order(const uint32_t *__restrict__ offsets, uint32_t *__restrict__ other,
                                                  uint32_t total) {
  const uint32_t o = blockIdx.x * CT + threadIdx.x;
  if (o >= total) return;
  const uint32_t lo = offsets[o], hi = offsets[o + 1u];
  for (uint32_t a = lo + 1u; a < hi; a++) {
    const uint32_t e = other[a];
    uint32_t b = a;
    while (b > lo) {
      const uint32_t p = other[b - 1u];
      if (p <= e) break;
      other[b] = p;
      b--;
    }
    if (b != a) other[b] = e;
  }
}

__global__ __launch_bounds__(CT) void k_dyn_scatter(const float4 *__restrict__ pr, const uint32_t *__restrict__ orig,
                                                    uint32_t n, float2 *__restrict__ pos0) {
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  if (l >= n) return;
  const uint32_t base = blockIdx.y * n, s = base + l;  // a member's slots are its own block of the arrays
  const float4 q = pr[s];
  pos0[base + orig[s]] = make_float2(q.x, q.y);
}

// the columns of the row reduction
enum { R_MARKED, R_NOW, R_KEPT, R_UNCHANGED, R_LOST, R_GAINED, R_MEASURED, R_QX, R_QY, R_LO, R_HI, R_MAX, R_COLS };

__global__ __launch_bounds__(CT) void k_dyn_compare(const float4 *__restrict__ cpr, const uint32_t *__restrict__ start,
                                                    const float4 *__restrict__ pr,
                                                    const uint32_t *__restrict__ sortedSlots, uint32_t n, uint32_t total,
                                                    ClusterGrid G, float gap, const uint32_t *__restrict__ offsets,
                                                    const uint32_t *__restrict__ other, const float2 *__restrict__ pos0,
                                                    uint32_t *__restrict__ now, uint32_t *__restrict__ kept,
                                                    float2 *__restrict__ disp, pbRearrangementStats *__restrict__ rows) {
  __shared__ unsigned long long sRed[CT / 64][R_COLS];
  const uint32_t t0 = blockIdx.x * CT;
  const bool live = t0 + threadIdx.x < total;
  const uint32_t t = live ? t0 + threadIdx.x : total - 1u;
  const float4 me = cpr[t];
  const uint32_t o = __float_as_uint(me.w);
  const uint32_t member = t / n, base = member * n;  // the keys carry the member: slot t is one of member t / n
  // the bot's marked list and marked position: in flight during the walk's first range
  const uint32_t first = offsets[o], end = offsets[o + 1u];
  const float2 p0 = pos0[o];
  const uint32_t len = end - first;
  const bool small = len <= 8u;
  const uint32_t NONE = 0xFFFFFFFFu;  // no index: indices are below 2^28
  const uint32_t e0 = small && len > 0u ? other[first] : NONE, e1 = small && len > 1u ? other[first + 1u] : NONE;
  const uint32_t e2 = small && len > 2u ? other[first + 2u] : NONE, e3 = small && len > 3u ? other[first + 3u] : NONE;
  const uint32_t e4 = small && len > 4u ? other[first + 4u] : NONE, e5 = small && len > 5u ? other[first + 5u] : NONE;
  const uint32_t e6 = small && len > 6u ? other[first + 6u] : NONE, e7 = small && len > 7u ? other[first + 7u] : NONE;
  uint32_t nw = 0u, kp = 0u;
  float xn = me.x, yn = me.y;
  if (live) {
    if (me.x == me.x) {  // a bot that is non-finite now has no links now
      pbWalkNine<false>(cpr, start, member, G, t, me, [&](uint32_t j, const float4 &q, float, float, float d2) {
        pbWhenLinked(t, me, j, q, d2, gap, [&](float, float) {
          nw++;
          const uint32_t oj = __float_as_uint(q.w) - base;
          bool hit;
          if (small) {
            hit = (oj == e0) | (oj == e1) | (oj == e2) | (oj == e3) | (oj == e4) | (oj == e5) | (oj == e6) | (oj == e7);
          } else {  // the first entry not below oj
            uint32_t lo = first, hi = end;
            while (lo < hi) {
              const uint32_t mid = lo + ((hi - lo) >> 1);
              if (other[mid] < oj) lo = mid + 1u;
              else hi = mid;
            }
            hit = lo < end && other[lo] == oj;
          }
          kp += hit ? 1u : 0u;
        });
      });
    } else {  // the sorted copy holds NaN for it; the displacement is taken from the position as it is
      const float4 raw = pr[sortedSlots[t]];
      xn = raw.x, yn = raw.y;
    }
  }
  const float dx = xn - p0.x, dy = yn - p0.y;
  // a dx in range implies that both of its coordinates are finite (inf - inf is NaN, inf - finite is inf)
  const bool measured = live && pbFixedInRange(dx) && pbFixedInRange(dy);
  long long qx = 0ll, qy = 0ll;
  unsigned long long s = 0ull;
  if (measured) {
    qx = pbFixedQuantise(dx), qy = pbFixedQuantise(dy);
    s = (unsigned long long)(qx * qx) + (unsigned long long)(qy * qy);
  }
  if (live) {
    now[o] = nw;
    kept[o] = kp;
    disp[o] = make_float2(dx, dy);
  }
  // the members' rows: per member the sums over each wave, the four waves through LDS, one set of atomics
  const uint32_t tLast = (total - t0 < (uint32_t)CT ? total : t0 + CT) - 1u;
  const uint32_t mFirst = t0 / n, mLast = tLast / n;
#pragma unroll 1
  for (uint32_t m = mFirst; m <= mLast; m++) {
    const bool mine = live && member == m;
    const bool add = mine && measured;
    unsigned long long r[R_COLS], v;
    r[R_MARKED] = waveSumU64(mine ? len : 0u), r[R_NOW] = waveSumU64(mine ? nw : 0u);
    r[R_KEPT] = waveSumU64(mine ? kp : 0u);
    r[R_UNCHANGED] = __popcll(__ballot(mine && kp == len && kp == nw));
    r[R_LOST] = __popcll(__ballot(mine && kp < len));
    r[R_GAINED] = __popcll(__ballot(mine && kp < nw));
    r[R_MEASURED] = __popcll(__ballot(add));
    r[R_QX] = waveSumU64(add ? (unsigned long long)qx : 0ull);
    r[R_QY] = waveSumU64(add ? (unsigned long long)qy : 0ull);
    r[R_LO] = waveSumU64(add ? pbFixedLow(s) : 0ull), r[R_HI] = waveSumU64(add ? pbFixedRest(s) : 0ull);
    r[R_MAX] = waveMaxU64(add ? s : 0ull);
    const auto opOf = [](uint32_t c) { return c == (uint32_t)R_MAX ? PB_FOLD_MAX_UNSIGNED : PB_FOLD_SUM; };
    if (blockFold(sRed, r, opOf, v)) {
      const uint32_t c = threadIdx.x;
      pbRearrangementStats *row = rows + m;
      if (v) {  // (a signed sum that is zero adds nothing either)
        if (c == R_MARKED) atomicAdd(&row->bonds_marked, v);
        else if (c == R_NOW) atomicAdd(&row->bonds_now, v);
        else if (c == R_KEPT) atomicAdd(&row->bonds_kept, v);
        else if (c == R_UNCHANGED) atomicAdd(&row->bots_unchanged, (unsigned)v);
        else if (c == R_LOST) atomicAdd(&row->bots_lost, (unsigned)v);
        else if (c == R_GAINED) atomicAdd(&row->bots_gained, (unsigned)v);
        else if (c == R_MEASURED) atomicAdd(&row->measured, (unsigned)v);
        else if (c == R_QX) atomicAdd((unsigned long long *)&row->sum_qx, v);  // two's complement: the signed sum modulo 2^64
        else if (c == R_QY) atomicAdd((unsigned long long *)&row->sum_qy, v);
        else if (c == R_LO) atomicAdd(&row->sum_q2_lo, v);  // the two partial sums: the host composes them
        else if (c == R_HI) atomicAdd(&row->sum_q2_hi, v);
        else atomicMax(&row->max_q2, v);
      }
    }
    __syncthreads();  // sRed is written again for the next member
  }
}

void dropMark(PbClusterScratch *C) {
  C->dMarked = false;
  C->dGap = C->dTime = 0.0f;
  C->dEntries = 0ull;
}

void freeMark(PbClusterScratch *C) {
  C->dPos0.reset(), C->dOffsets.reset(), C->dOther.reset(), C->dParts.reset();
  dropMark(C);
}

// files the bots at the mark's gap and leaves now, kept, disp and the rows (partial sums in sum_q2_*) on the device
int compareSweep(pbSim *S) {
  const float gap = S->cluster->dGap;
  const int rc = pbClusterFile(S, (double)gap, 2.0);
  if (rc != PB_OK) return rc;
  PbClusterScratch *C = S->cluster;
  const ClusterGrid G = gridOf(C);
  const size_t total = S->total;  // (each on its own: a failed allocation leaves the rest to the next call)
  PB_TRY(C->dNow.ensure(total));
  PB_TRY(C->dKept.ensure(total));
  PB_TRY(C->dDisp.ensure(total));
  PB_TRY(C->dRows.ensure(S->nsims));
  PB_TRY(hipMemsetAsync(C->dRows, 0, sizeof(pbRearrangementStats) * S->nsims, S->stream));
  hipLaunchKernelGGL(k_dyn_compare, dim3(cdiv(S->total, CT)), dim3(CT), 0, S->stream, C->cpr, C->start, S->pr[S->cur],
                     C->vals[C->sortedIn], S->n, S->total, G, gap, C->dOffsets, C->dOther, C->dPos0, C->dNow, C->dKept,
                     C->dDisp, C->dRows);
  PB_TRY(hipGetLastError());
  return pbClockStop(S, C->dynamicsClock);
}

}  // namespace

int pbDynamicsScatter(pbSim *S, float2 *pos) {
  hipLaunchKernelGGL(k_dyn_scatter, dim3(cdiv(S->n, CT), S->nsims), dim3(CT), 0, S->stream, S->pr[S->cur],
                     S->orig[S->cur], S->n, pos);
  PB_TRY(hipGetLastError());
  return PB_OK;
}

int pbSimMarkReference(pbSim *S, float linkGap) {
  if (!S) return pbFail("pbSimMarkReference", ": null handle");
  int rc = pbClusterCheckArgs("pbSimMarkReference", S, &linkGap, nullptr);
  if (rc != PB_OK) return rc;
  if (S->cluster) dropMark(S->cluster);  // whatever happens below, the old mark is gone
  rc = pbClusterFile(S, (double)linkGap, 2.0);
  if (rc != PB_OK) return rc;
  PbClusterScratch *C = S->cluster;
  const ClusterGrid G = gridOf(C);
  const uint32_t n = S->n, total = S->total, blocks = cdiv(total, CT);
  PB_TRY(C->dPos0.ensure((size_t)total));
  PB_TRY(C->dOffsets.ensure((size_t)total + 1));
  PB_TRY(C->dParts.ensure((size_t)blocks + 2));
  const dim3 b(CT), gBots(cdiv(n, CT), S->nsims);
  unsigned long long *sum = C->dParts + blocks, *flag = sum + 1;
  PB_TRY(hipMemsetAsync(sum, 0, sizeof(unsigned long long) * 2, S->stream));
  hipLaunchKernelGGL(k_dyn_count, gBots, b, 0, S->stream, C->cpr, C->start, n, G, linkGap, C->degree);
  PB_TRY(hipGetLastError());
  rc = pbContactScan(S, C->degree, total, C->dParts, C->dOffsets);
  if (rc != PB_OK) return rc;
  unsigned long long count = 0ull;
  PB_TRY(hipMemcpyAsync(&count, sum, sizeof count, hipMemcpyDeviceToHost, S->stream));
  PB_TRY(hipStreamSynchronize(S->stream));
  if (count >= (1ull << 31))
    return pbFail("pbSimMarkReference", ": the batch has 2^31 directed entries or more (offsets are 32-bit)");
  PB_TRY(C->dOther.ensure(count ? count : 1ull));
  hipLaunchKernelGGL(k_dyn_fill, gBots, b, 0, S->stream, C->cpr, C->start, n, G, linkGap, C->dOffsets, C->dOther, flag);
  hipLaunchKernelGGL(k_dyn_order, dim3(blocks), b, 0, S->stream, C->dOffsets, C->dOther, total);
  PB_TRY(hipGetLastError());
  rc = pbDynamicsScatter(S, C->dPos0);
  if (rc != PB_OK) return rc;
  rc = pbClockMark(S, C->dynamicsClock);  // the mark ends here: the flag's way back is not part of its device time
  if (rc != PB_OK) return rc;
  unsigned long long raised = 0ull;
  PB_TRY(hipMemcpyAsync(&raised, flag, sizeof raised, hipMemcpyDeviceToHost, S->stream));
  rc = pbClockRead(S, C->dynamicsClock);  // one drain serves the clock and the flag
  if (rc != PB_OK) return rc;
  if (raised) {
    pbLastError() = "reference mark: count and fill disagree";
    return PB_ERR_HIP;
  }
  C->dMarked = true;
  C->dGap = linkGap, C->dTime = S->time;
  C->dEntries = count;
  return PB_OK;
}

int pbSimClearReference(pbSim *S) {
  if (!S) return pbFail("pbSimClearReference", ": null handle");
  if (S->cluster) {
    useDevice(S);
    freeMark(S->cluster);
  }
  return PB_OK;
}

int pbSimGetReferenceInfo(pbSim *S, int *marked, float *linkGap, float *time, unsigned long long *entries) {
  if (!S) return pbFail("pbSimGetReferenceInfo", ": null handle");
  const PbClusterScratch *C = S->cluster;
  const bool held = C && C->dMarked;
  if (marked) *marked = held ? 1 : 0;
  if (linkGap) *linkGap = held ? C->dGap : 0.0f;
  if (time) *time = held ? C->dTime : 0.0f;
  if (entries) *entries = held ? C->dEntries : 0ull;
  return PB_OK;
}

int pbSimRearrangementStats(pbSim *S, pbRearrangementStats *rows) {
  if (!S || !rows) return pbFail("pbSimRearrangementStats", ": null handle or rows");
  int rc = pbClusterCheckArgs("pbSimRearrangementStats", S, nullptr, nullptr);
  if (rc == PB_OK) rc = pbNeedMark("pbSimRearrangementStats", S);
  if (rc == PB_OK) rc = compareSweep(S);
  if (rc != PB_OK) return rc;
  PB_TRY(hipMemcpy(rows, S->cluster->dRows, sizeof(pbRearrangementStats) * S->nsims, hipMemcpyDeviceToHost));
  for (uint32_t m = 0; m < S->nsims; m++) {  // the two partial sums as one 128-bit integer
    const unsigned __int128 v = (unsigned __int128)pbFixedCompose(rows[m].sum_q2_lo, rows[m].sum_q2_hi);
    rows[m].sum_q2_lo = (unsigned long long)v;
    rows[m].sum_q2_hi = (unsigned long long)(v >> 64);
  }
  return PB_OK;
}

int pbSimRearrangementOf(pbSim *S, unsigned member, float *disp, unsigned *marked, unsigned *now, unsigned *kept) {
  if (!S) return pbFail("pbSimRearrangementOf", ": null handle");
  if (!disp && !marked && !now && !kept)
    return pbFail("pbSimRearrangementOf", ": disp, marked, now and kept are all null");
  int rc = pbClusterCheckArgs("pbSimRearrangementOf", S, nullptr, &member);
  if (rc == PB_OK) rc = pbNeedMark("pbSimRearrangementOf", S);
  if (rc == PB_OK) rc = compareSweep(S);
  if (rc != PB_OK) return rc;
  PbClusterScratch *C = S->cluster;
  const size_t n = S->n, base = (size_t)member * n;
  std::vector<uint32_t> off;
  if (disp) PB_TRY(hipMemcpyAsync(disp, C->dDisp + base, sizeof(float2) * n, hipMemcpyDeviceToHost, S->stream));
  if (now) PB_TRY(hipMemcpyAsync(now, C->dNow + base, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, S->stream));
  if (kept) PB_TRY(hipMemcpyAsync(kept, C->dKept + base, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, S->stream));
  if (marked) {
    off.resize(n + 1);
    PB_TRY(hipMemcpyAsync(off.data(), C->dOffsets + base, sizeof(uint32_t) * (n + 1), hipMemcpyDeviceToHost, S->stream));
  }
  PB_TRY(hipStreamSynchronize(S->stream));
  if (marked)
    for (size_t i = 0; i < n; i++) marked[i] = off[i + 1] - off[i];
  return PB_OK;
}

int pbSimGetRearrangementTimes(pbSim *S, unsigned long long *analyses, float *last_device_ms) {
  return pbClockGet("pbSimGetRearrangementTimes", S, &PbClusterScratch::dynamicsClock, analyses, last_device_ms);
}
