// pb_contacts.hip -- the contact network of one member on gfx950: who touches whom, how deep, and with what force
// (pbSimContactsOf / pbSimContactVirialOf, include/particlebot_hip.h has the definition).
//
// The front end is the cluster analysis' (pbClusterAnalyse, pb_cluster.hip): a fresh grid, the sorted posrad array and
// every bot's degree under the link predicate.  On top of it, for the requested member only:
//   k_contact_scan        exclusive prefix sum of the member's degrees into offsets[0..n], ORIGINAL order, in three
//                         launches: block sums (wave shuffles, then the wave totals through LDS), one workgroup over the
//                         block sums, and the offsets themselves.  Sums are 64-bit, so a member with 2^31 entries or more
//                         is seen as such; the total (8 bytes) goes back to the host, which sizes the link buffer
//   k_contact_gather_vel  the member's velocities in sorted order next to cpr, its positions in ORIGINAL order
//   k_contact_fill        the walk over the nine cells and the link rule that counted the degrees (pbWalkNine and
//                         pbWhenLinked, pb_cluster.hpp); every accepted neighbour goes through pbPair (zeroed accumulator,
//                         this bot as A) and becomes one 16-byte entry at offsets[o] + k.  The store is guarded by
//                         offsets[o + 1], and a lane whose count differs from its degree raises a flag: the host reports
//                         it instead of a torn list
//   k_contact_order       one lane per bot: insertion sort of its entries by `other`, in place in global memory (lists are
//                         about 6 long at contact gaps; long lists of a large linkGap stay correct and are slow), then
//                         the four virial sums over the ordered list when a virial buffer is attached
// Count and fill agree because both evaluate the one link rule, compiled without contraction, on the same bytes of cpr
// over the one walk's ranges.  No scratch memory: a list is never staged in a private array.
#include <string.h>

#include "pb_cluster.hpp"

static_assert(sizeof(pbContactLink) == 16 && sizeof(uint4) == 16, "a link entry is one 16-byte access");

namespace {

// one link entry as the compiler's own 16-byte vector (other, gap, fx, fy as bit patterns): a single dwordx4 access
typedef uint32_t LinkBits __attribute__((ext_vector_type(4)));

// phase 0: parts[b] = sum of workgroup b's degrees.  phase 1 (one workgroup): parts[0 .. blocks) becomes its own
// exclusive prefix, parts[blocks] the total.  phase 2: offsets[l] = parts[b] + the prefix inside workgroup b, and
// offsets[n] behind the last bot.
__global__ __launch_bounds__(CT) void k_contact_scan(int phase, const uint32_t *__restrict__ degree, uint32_t n,
                                                     uint32_t blocks, unsigned long long *__restrict__ parts,
                                                     uint32_t *__restrict__ offsets) {
  __shared__ unsigned long long sWave[CT / 64];
  unsigned long long tot;
  if (phase == 1) {
    unsigned long long carry = 0ull;
    for (uint32_t c0 = 0u; c0 < blocks; c0 += CT) {
      const uint32_t i = c0 + threadIdx.x;
      const unsigned long long v = i < blocks ? parts[i] : 0ull;
      const unsigned long long ex = blockScanExclusive(v, sWave, tot);
      if (i < blocks) parts[i] = carry + ex;
      carry += tot;
    }
    if (threadIdx.x == 0) parts[blocks] = carry;
    return;
  }
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  const unsigned long long v = l < n ? degree[l] : 0u;
  const unsigned long long ex = blockScanExclusive(v, sWave, tot);
  if (phase == 0) {
    if (threadIdx.x == 0) parts[blockIdx.x] = tot;
    return;
  }
  if (l < n) {
    const unsigned long long off = parts[blockIdx.x] + ex;
    offsets[l] = (uint32_t)off;
    if (l == n - 1u) offsets[n] = (uint32_t)(off + v);
  }
}

}  // namespace

// The scan's three launches (pb_cluster.hpp).
int pbContactScan(pbSim *S, const uint32_t *degree, uint32_t n, unsigned long long *parts, uint32_t *offsets) {
  const uint32_t blocks = cdiv(n, CT);
  for (int phase = 0; phase < 3; phase++)
    hipLaunchKernelGGL(k_contact_scan, phase == 1 ? dim3(1) : dim3(blocks), dim3(CT), 0, S->stream, phase, degree, n,
                       blocks, parts, offsets);
  PB_TRY(hipGetLastError());
  return PB_OK;
}

namespace {

__global__ __launch_bounds__(CT) void k_contact_gather_vel(const float4 *__restrict__ cpr,
                                                           const uint32_t *__restrict__ sortedSlots,
                                                           const float2 *__restrict__ vel, uint32_t base, uint32_t n,
                                                           float2 *__restrict__ cVel, float2 *__restrict__ cPos) {
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  if (l >= n) return;
  const uint32_t t = base + l;
  cVel[l] = vel[sortedSlots[t]];  // keys carry the member: the slot is one of this member's
  const float4 q = cpr[t];
  cPos[__float_as_uint(q.w) - base] = make_float2(q.x, q.y);
}

__global__ __launch_bounds__(CT) void k_contact_fill(const float4 *__restrict__ cpr, const uint32_t *__restrict__ start,
                                                     const float2 *__restrict__ cVel,
                                                     const PbDevParams *__restrict__ dP, uint32_t member, uint32_t n,
                                                     ClusterGrid G, float gap, const uint32_t *__restrict__ offsets,
                                                     LinkBits *__restrict__ links, unsigned long long *__restrict__ flag) {
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  if (l >= n) return;
  const uint32_t base = member * n, t = base + l;
  const float4 me = cpr[t];
  const uint32_t o = __float_as_uint(me.w) - base;
  const uint32_t first = offsets[o], end = offsets[o + 1u];
  uint32_t k = 0u;
  if (me.x == me.x) {  // a bot with a non-finite position or radius has no links
    const PbDevParams &P = dP[member];
    // the payload's attractionFactor for whichever end is the payload bot (pb_sweep.hpp: P.attraction * q.w * att1)
    const bool payloadMode = P.nDead == -1;
    const uint32_t payloadIdx = P.nCells - 1u;
    const float att1 = (payloadMode && o == payloadIdx) ? P.attractionFactor : 1.0f;
    const float2 v = cVel[l];
    pbWalkNine<false>(cpr, start, member, G, t, me, [&](uint32_t j, const float4 &q, float, float, float d2) {
      pbWhenLinked(t, me, j, q, d2, gap, [&](float dist, float R) {
        const float g = dist - R;
        const uint32_t oj = __float_as_uint(q.w) - base;
        const float att2 = (payloadMode && oj == payloadIdx) ? P.attractionFactor : 1.0f;
        PbForce F = {0.0f, 0.0f, 0.0f, 0.0f};
        pbPair(P, me.x, me.y, v.x, v.y, me.z, q.x, q.y, q.z, P.attraction * att2 * att1,
               [&]() { return cVel[j - base]; }, F);
        if (first + k < end)  // never outside this bot's share of the buffer, whatever the count pass said
          links[first + k] = LinkBits{oj, __float_as_uint(g), __float_as_uint(F.fx), __float_as_uint(F.fy)};
        k++;
      });
    });
  }
  if (k != end - first) __atomic_store_n(flag, 1ull, __ATOMIC_RELAXED);
}

__global__ __launch_bounds__(CT) void k_contact_order(const uint32_t *__restrict__ offsets, LinkBits *__restrict__ links,
                                                      const float2 *__restrict__ cPos, uint32_t n,
                                                      double *__restrict__ virial) {
  const uint32_t o = blockIdx.x * CT + threadIdx.x;
  if (o >= n) return;
  const uint32_t lo = offsets[o], hi = offsets[o + 1u];
  for (uint32_t a = lo + 1u; a < hi; a++) {
    const LinkBits e = links[a];
    uint32_t b = a;
    while (b > lo) {
      const LinkBits p = links[b - 1u];
      if (p.x <= e.x) break;
      links[b] = p;
      b--;
    }
    if (b != a) links[b] = e;
  }
  if (!virial) return;
  const float2 pi = cPos[o];
  double sxx = 0.0, sxy = 0.0, syx = 0.0, syy = 0.0;
  for (uint32_t a = lo; a < hi; a++) {
    const LinkBits e = links[a];
    const float2 pj = cPos[e.x < n ? e.x : o];  // (an entry the fill never wrote: the host reports the flag, nothing is read outside)
    const double rx = (double)(pj.x - pi.x), ry = (double)(pj.y - pi.y);  // the fp32 differences, widened
    const double fx = (double)__uint_as_float(e.z), fy = (double)__uint_as_float(e.w);
    sxx = sxx + rx * fx;  // each product is exact in fp64 (24 + 24 bits)
    sxy = sxy + rx * fy;
    syx = syx + ry * fx;
    syy = syy + ry * fy;
  }
  double *out = virial + 4u * (size_t)o;
  out[0] = sxx, out[1] = sxy, out[2] = syx, out[3] = syy;
}

int ensureContactScratch(pbSim *S) {
  PbClusterScratch *C = S->cluster;
  const size_t n = S->n;  // (each on its own: a failed allocation leaves the rest to the next call)
  PB_TRY(C->cOffsets.ensure(n + 1));
  PB_TRY(C->cParts.ensure((size_t)cdiv(S->n, CT) + 2));
  PB_TRY(C->cVel.ensure(n));
  PB_TRY(C->cPos.ensure(n));
  PB_TRY(C->cVirial.ensure(4 * n));
  return PB_OK;
}

// The export up to the device's buffers: offsets always; links (ordered) and the virial when asked for.  *entries is
// set as soon as the count is known.  cap: the caller's room for links (checked only with wantLinks).
int exportContacts(const char *fn, pbSim *S, uint32_t member, float gap, bool wantLinks, unsigned long long cap,
                   bool wantVirial, unsigned long long *entries) {
  int rc = pbClusterAnalyse(S, gap);
  if (rc != PB_OK) return rc;
  rc = ensureContactScratch(S);
  if (rc != PB_OK) return rc;
  PbClusterScratch *C = S->cluster;
  const uint32_t n = S->n, base = member * n, blocks = cdiv(n, CT);
  const dim3 b(CT), g(blocks);
  unsigned long long *total = C->cParts + blocks, *flag = total + 1;
  PB_TRY(hipMemsetAsync(total, 0, sizeof(unsigned long long) * 2, S->stream));
  rc = pbContactScan(S, C->degree + base, n, C->cParts, C->cOffsets);
  if (rc != PB_OK) return rc;
  unsigned long long count = 0ull;
  PB_TRY(hipMemcpyAsync(&count, total, sizeof count, hipMemcpyDeviceToHost, S->stream));
  PB_TRY(hipStreamSynchronize(S->stream));
  *entries = count;
  if (count >= (1ull << 31)) return pbFail(fn, ": the member has 2^31 directed entries or more (offsets are 32-bit)");
  if (wantLinks && cap < count)
    return pbFail(fn, ": links holds fewer entries than the member has (call with links NULL to size)");
  unsigned long long raised = 0ull;
  if (wantLinks || wantVirial) {
    PB_TRY(C->cLinks.ensure(count ? count : 1ull));
    const ClusterGrid G = gridOf(C);
    hipLaunchKernelGGL(k_contact_gather_vel, g, b, 0, S->stream, C->cpr, C->vals[C->sortedIn], S->vel[S->cur], base, n,
                       C->cVel, C->cPos);
    hipLaunchKernelGGL(k_contact_fill, g, b, 0, S->stream, C->cpr, C->start, C->cVel, S->dP, member, n, G, gap,
                       C->cOffsets, (LinkBits *)C->cLinks.get(), flag);
    hipLaunchKernelGGL(k_contact_order, g, b, 0, S->stream, C->cOffsets, (LinkBits *)C->cLinks.get(), C->cPos, n,
                       wantVirial ? C->cVirial : (double *)nullptr);
    PB_TRY(hipGetLastError());
    rc = pbClockMark(S, C->contactClock);  // the export ends here: the flag's way back is not part of its device time
    if (rc != PB_OK) return rc;
    PB_TRY(hipMemcpyAsync(&raised, flag, sizeof raised, hipMemcpyDeviceToHost, S->stream));
    rc = pbClockRead(S, C->contactClock);  // one drain serves the clock and the flag
  } else {
    rc = pbClockStop(S, C->contactClock);
  }
  if (rc != PB_OK) return rc;
  if (raised) {
    pbLastError() = "contact export: count and fill disagree";
    return PB_ERR_HIP;
  }
  return PB_OK;
}

}  // namespace

int pbSimContactsOf(pbSim *S, unsigned member, float linkGap, unsigned *offsets, pbContactLink *links,
                    unsigned long long cap, unsigned long long *entries) {
  if (!S || !entries) return pbFail("pbSimContactsOf", ": null handle or entries");
  int rc = pbClusterCheckArgs("pbSimContactsOf", S, &linkGap, &member);
  if (rc != PB_OK) return rc;
  rc = exportContacts("pbSimContactsOf", S, member, linkGap, links != nullptr, cap, false, entries);
  if (rc != PB_OK) return rc;
  PbClusterScratch *C = S->cluster;
  if (offsets)
    PB_TRY(hipMemcpyAsync(offsets, C->cOffsets, sizeof(uint32_t) * ((size_t)S->n + 1), hipMemcpyDeviceToHost, S->stream));
  if (links && *entries)
    PB_TRY(hipMemcpyAsync(links, C->cLinks, sizeof(pbContactLink) * *entries, hipMemcpyDeviceToHost, S->stream));
  PB_TRY(hipStreamSynchronize(S->stream));
  return PB_OK;
}

int pbSimContactVirialOf(pbSim *S, unsigned member, float linkGap, double *virial) {
  if (!S || !virial) return pbFail("pbSimContactVirialOf", ": null handle or virial");
  int rc = pbClusterCheckArgs("pbSimContactVirialOf", S, &linkGap, &member);
  if (rc != PB_OK) return rc;
  unsigned long long entries = 0ull;
  rc = exportContacts("pbSimContactVirialOf", S, member, linkGap, false, 0ull, true, &entries);
  if (rc != PB_OK) return rc;
  PB_TRY(hipMemcpy(virial, S->cluster->cVirial, sizeof(double) * 4 * S->n, hipMemcpyDeviceToHost));
  return PB_OK;
}

int pbSimGetContactTimes(pbSim *S, unsigned long long *exports, float *last_device_ms) {
  return pbClockGet("pbSimGetContactTimes", S, &PbClusterScratch::contactClock, exports, last_device_ms);
}
