// pb_fourpoint.hip -- four-point dynamics on gfx950: per member and lag the exact integer sums over time origins of Q and
// Q^2, Q being the number of bots that stayed within an overlap radius of where they were, and per wavevector of a
// caller's list those of the masked density mode W = sum_i w_i exp(i k . r_i(then)) and of |W|^2, while pbSimStep runs
// (pbSimSetFourPoint / pbSimFourPointRecord / pbSimGetFourPoint; include/particlebot_hip.h has the definitions): the
// susceptibility chi_4 and the structure factor S_4(k, tau) of the slow bots.  The ring of quantised positions in
// ORIGINAL order, its pairing lag by lag, its book and the shells of the entry points are the lag ring's (pb_engine.hpp,
// PbLagBook ... pbLagTimes); the turn, the index and the table are pb_phasor.hpp's; the overlap rule, the cells and what
// an origin adds are pb_fourpoint.hpp's, on pb_coherent.hpp's product and 192-bit add; none is restated here.
//
//   k_fp_snapshot  the scattering's rule, restated with the same two functions: one pass over pr[cur] and orig[cur] in
//                  SLOT order, one int2 (qx, qy) per bot to ring[slot][member * n + orig], (INT32_MIN, 0) for an
//                  out-of-range bot.
//   k_fp_modes     the hot path, N x lags x K look-ups per record.  One workgroup of 256 lanes per (member, lag, bot
//                  block), at most PB_FOURPOINT_BLOCKS blocks per member and lag, all lags of a record in one launch.
//                  The table is copied into LDS once (32 KiB); 256 pairs at a time are staged from coalesced 8-byte
//                  loads of the two snapshots as (qx_then << shift, qy_then << shift, mask), the mask all ones for a
//                  measured pair that overlaps and all zeros otherwise and past the member's end.  The lanes are
//                  (stripe, vector) as in k_scat_accumulate, and a lane keeps A and B in two 64-bit registers.  Unlike
//                  the scattering's, whole tiles here hold few entries that count, at long lags most of them, so the
//                  COMPACTED form ships: a tile's overlapping entries are moved to its front (a ballot prefix and the
//                  waves' counts through LDS: one more barrier per tile), the zero masks behind them, and every lane
//                  walks up to the tile's last overlapping entry: the tile's count, rounded up to whole unrolled
//                  groups, is the trip count, so it stays workgroup-uniform and the unrolled look-ups overlap (DESIGN
//                  7n).  With -DPB_FOURPOINT_COMPACT=0 every lane walks Vp entries of the tile as staged, whatever it
//                  holds: the MASKED form (DESIGN 7o has both costs).  The stripes of a wave are folded with shuffles
//                  and one lane per (wave, vector) adds into the record's scratch mode with 64-bit integer atomics.
//                  m and Q are the staging ballots' popcounts, one pair of atomics per wave.
//   k_fp_fold      one launch per record, one lane per (member, lag, vector): the lane loads its origin's mode and adds
//                  A, B and A^2 + B^2 into its own cell with plain loads and stores; the lane of vector 0 also adds m, Q
//                  and Q^2 into the (member, lag) words.  A cell has one owner and the launches of a stream are ordered:
//                  no atomics, no LDS.
// The scratch of modes and counts is zeroed on the stream in front of k_fp_modes.  Everything that is added is an integer,
// so nothing depends on the slot order, on the kernel form that stepped or on the order of the adds.  No float atomics,
// no atomics wider than 64 bits, no scratch memory.  A record is these launches on the batch's stream between two events;
// the host never waits for them.
#include <limits.h>

#include "pb_engine.hpp"
#include "pb_fixed.hpp"
#include "pb_fourpoint.hpp"
#include "pb_phasor.hpp"

static_assert(sizeof(pbFourPointRow) == 128, "a four-point row is 128 bytes");
static_assert(PB_FOURPOINT_MAX_VECTORS == 256u, "a workgroup of 256 lanes holds the whole list: one vector per lane");
static_assert(sizeof(ulonglong2) == sizeof(unsigned long long) * PB_FP_MODE_WORDS &&
                  sizeof(ulonglong2) == sizeof(unsigned long long) * PB_FP_COUNT_WORDS,
              "a mode and a pair of counts are 16 bytes each");

// k_fp_modes' staging: 1 (ships) the compacted form (a tile's overlapping entries are moved to its front and the walk
// ends behind the last), 0 the masked form (every lane walks the whole tile).  A build-time choice
// (EXTRA_DEVFLAGS=-DPB_FOURPOINT_COMPACT=0); DESIGN 7o and profiles/four_point.txt have both costs.
#ifndef PB_FOURPOINT_COMPACT
#define PB_FOURPOINT_COMPACT 1
#endif

namespace {

constexpr int FT = PB_LAG_LANES;
constexpr const char *WHAT = "four-point recorder";

__global__ __launch_bounds__(FT) void k_fp_snapshot(const float4 *__restrict__ pr, const uint32_t *__restrict__ orig,
                                                    uint32_t n, int2 *__restrict__ snap) {
  const uint32_t l = blockIdx.x * FT + threadIdx.x;
  if (l >= n) return;
  const uint32_t s = blockIdx.y * n + l;  // the batch is below 2^28 bots
  const uint32_t o = orig[s];
  // (a layout is a permutation of 0 .. n - 1; were it not, nothing is written outside the member's block: k_tc_snapshot)
  if (o >= n) return;
  const float4 q = pr[s];
  const bool ok = pbFixedInRange(q.x) && pbFixedInRange(q.y);
  // |q| <= 2^31 - 128: INT32_MIN is free to say "unmeasured"
  snap[blockIdx.y * n + o] = ok ? make_int2((int)pbFixedQuantise(q.x), (int)pbFixedQuantise(q.y)) : make_int2(INT_MIN, 0);
}

__global__ __launch_bounds__(FT) void k_fp_modes(const int2 *__restrict__ ring, uint32_t n, uint32_t total,
                                                 uint32_t lags, uint32_t slotNow, uint32_t nLags, uint32_t blocksPerLag,
                                                 int shift, long long qa, unsigned long long a2,
                                                 const int2 *__restrict__ vectors, uint32_t nvec, uint32_t vp,
                                                 const int2 *__restrict__ phasors,
                                                 unsigned long long *__restrict__ modes,
                                                 unsigned long long *__restrict__ counts) {
  __shared__ int2 sTab[PB_PHASOR_STEPS];  // (C[j], S[j])
  __shared__ int4 sBot[FT];               // (qx_then << shift, qy_then << shift, mask, 0) of the tile's pairs
#if PB_FOURPOINT_COMPACT
  __shared__ uint32_t sWave[FT / 64];     // the overlapping pairs each wave staged
#endif
  const auto [member, lag, b, now, then] = pbLagPair(ring, n, total, lags, slotNow, nLags, blocksPerLag);
  for (uint32_t j = threadIdx.x; j < PB_PHASOR_STEPS; j += FT) sTab[j] = phasors[j];
  // vp is a power of two, nvec <= vp <= 256: lane t is vector t & (vp - 1) of stripe t / vp, 256 / vp stripes
  const uint32_t k = threadIdx.x & (vp - 1u), stripe = threadIdx.x / vp, stripes = (uint32_t)FT / vp;
  const bool mine = k < nvec;
  // (wave-uniform) a wave whose first vector is past the end of the list walks nothing (vp >= 128 only); it still
  // stages pairs and meets every barrier
  const bool walks = ((threadIdx.x & ~63u) & (vp - 1u)) < nvec;
  const int2 nv = mine ? vectors[k] : make_int2(0, 0);
  const uint32_t nx = (uint32_t)nv.x, ny = (uint32_t)nv.y;
  unsigned long long re = 0ull, im = 0ull;
  uint32_t nMeasured = 0u, nOverlap = 0u;  // wave-uniform
#pragma unroll 1
  for (uint32_t t0 = b * FT; t0 < n; t0 += blocksPerLag * FT) {  // (workgroup-uniform)
    const uint32_t i = t0 + threadIdx.x;
    int4 s = make_int4(0, 0, 0, 0);
    bool ok = false, w = false;
    if (i < n) {
      const int2 u = now[i], z = then[i];
      ok = u.x != INT_MIN && z.x != INT_MIN;
      w = ok && pbFpOverlaps(u.x, u.y, z.x, z.y, qa, a2);
      if (w) {
        s.x = (int)((uint32_t)z.x << shift), s.y = (int)((uint32_t)z.y << shift);
        s.z = -1;
      }
    }
    const unsigned long long slow = __ballot(w);
    nMeasured += (uint32_t)__popcll(__ballot(ok));
    nOverlap += (uint32_t)__popcll(slow);
    __syncthreads();  // the tile before this one has been walked (and, the first time, the table is stored)
#if PB_FOURPOINT_COMPACT
    // The tile's overlapping entries first, in order, the zero masks behind them: a wave's count through LDS, a lane's
    // place from the ballot's prefix.  Every lane stores one entry, so the 256 are a permutation and none is stale.
    const uint32_t wave = threadIdx.x >> 6, lane64 = threadIdx.x & 63u;
    if (lane64 == 0u) sWave[wave] = (uint32_t)__popcll(slow);
    __syncthreads();
    uint32_t before = 0u, count = 0u;
#pragma unroll
    for (uint32_t v = 0; v < (uint32_t)FT / 64u; v++) {
      const uint32_t c = sWave[v];
      before += v < wave ? c : 0u, count += c;
    }
    const uint32_t rank = (uint32_t)__popcll(slow & ((1ull << lane64) - 1ull));
    sBot[w ? before + rank : count + (64u * wave - before) + (lane64 - rank)] = s;
    __syncthreads();
    // the tile's count, rounded up to whole unrolled groups of trips, is the trip count of every lane
    const uint32_t need = ((count + stripes - 1u) / stripes + 3u) & ~3u, trips = need < vp ? need : vp;
#else
    sBot[threadIdx.x] = s;
    __syncthreads();
    const uint32_t trips = vp;
#endif
    if (walks) {
      // A lane walks the same number of entries as every other, zero masks included (masked form: its vp = 256 / stripes
      // entries of the whole tile; compacted form: up to the tile's last overlapping entry), so the unrolled look-ups
      // overlap instead of waiting for each other's exit test
#pragma unroll 4
      for (uint32_t trip = 0, j = stripe; trip < trips; trip++, j += stripes) {
        const int4 p = sBot[j];  // the same address in every lane of a stripe: a broadcast
        // (nx qx + ny qy) << shift == nx (qx << shift) + ny (qy << shift) mod 2^32: the turn with the shift staged
        const int2 cs = sTab[pbPhasorIndex(pbPhasorTurn(nx, ny, (uint32_t)p.x, (uint32_t)p.y, 0))];
        re += (unsigned long long)(long long)(cs.x & p.z);
        im += (unsigned long long)(long long)(cs.y & p.z);
      }
    }
  }
  // the stripes that share a wave: lanes l, l ^ vp, l ^ 2 vp, ... own the same vector (all 64 lanes take part)
#pragma unroll 1
  for (uint32_t m = 32u; m >= vp; m >>= 1) {
    re += shflXor64(re, (int)m);
    im += shflXor64(im, (int)m);
  }
  const uint32_t lane = threadIdx.x & 63u;
  const size_t cell = (size_t)member * lags + lag;
  if (mine && lane < vp) {
    unsigned long long *mode = modes + (cell * nvec + k) * PB_FP_MODE_WORDS;
    if (re) (void)__hip_atomic_fetch_add(mode + PB_FP_A, re, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // no-return
    if (im) (void)__hip_atomic_fetch_add(mode + PB_FP_B, im, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (lane == 0u) {
    unsigned long long *count = counts + cell * PB_FP_COUNT_WORDS;
    if (nMeasured)
      (void)__hip_atomic_fetch_add(count + PB_FP_M, (unsigned long long)nMeasured, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (nOverlap)
      (void)__hip_atomic_fetch_add(count + PB_FP_Q, (unsigned long long)nOverlap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(FT) void k_fp_fold(const ulonglong2 *__restrict__ modes, const ulonglong2 *__restrict__ counts,
                                                uint32_t nsims, uint32_t nvec, uint32_t lags, uint32_t nLags,
                                                unsigned long long *__restrict__ cells,
                                                unsigned long long *__restrict__ lagCells) {
  const uint32_t g = blockIdx.x * FT + threadIdx.x;  // nsims x lags x nvec is below 2^25 (the table's bound)
  if (g >= nsims * nLags * nvec) return;
  const uint32_t rest = g / nvec, k = g - rest * nvec;
  const uint32_t member = rest / nLags, lag = rest - member * nLags;
  const size_t c = (size_t)member * lags + lag;
  const ulonglong2 mode = modes[c * nvec + k];
  pbFpMode(cells + (c * nvec + k) * PB_FP_WORDS, (long long)mode.x, (long long)mode.y);
  if (k == 0u) {
    const ulonglong2 mq = counts[c];
    pbFpCounts(lagCells + c * PB_FP_LAG_WORDS, mq.x, mq.y);
  }
}

// the table the structure factor exports, fetched once per process
const int *phasorTable() {
  static const std::vector<int> table = [] {
    std::vector<int> t(2u * PB_PHASOR_STEPS);
    (void)pbPhasorTable(t.data(), 2u * PB_PHASOR_STEPS);
    return t;
  }();
  return table.data();
}

size_t cellsOf(const pbSim *S, const PbFourPoint &K) { return (size_t)S->nsims * K.lag.book.lags * K.nvec; }

}  // namespace

int pbFourPointRecord(pbSim *S) {
  PbFourPoint &K = S->fp;
  uint32_t vp = 1u;
  while (vp < K.nvec) vp <<= 1;
  const int c = S->cur;
  const uint32_t slot = K.lag.book.slot(), nLags = K.lag.book.paired(), lags = K.lag.book.lags;
  const uint32_t perMember = cdiv(S->n, FT);
  const uint32_t bpl = perMember < PB_FOURPOINT_BLOCKS ? perMember : PB_FOURPOINT_BLOCKS;
  const size_t cells = cellsOf(S, K), pairs = (size_t)S->nsims * lags;
  unsigned long long *modes = K.scratch, *counts = K.scratch + cells * PB_FP_MODE_WORDS;
  PB_TRY(K.lag.clock.start(S->stream));
  hipLaunchKernelGGL(k_fp_snapshot, dim3(perMember, S->nsims), dim3(FT), 0, S->stream, S->pr[c], S->orig[c], S->n,
                     K.lag.ring + (size_t)slot * S->total);
  PB_TRY(hipMemsetAsync(modes, 0, sizeof(unsigned long long) * cells * PB_FP_MODE_WORDS, S->stream));
  PB_TRY(hipMemsetAsync(counts, 0, sizeof(unsigned long long) * pairs * PB_FP_COUNT_WORDS, S->stream));
  hipLaunchKernelGGL(k_fp_modes, dim3(pbLagGrid(S->nsims, nLags, bpl)), dim3(FT), 0, S->stream, K.lag.ring, S->n,
                     S->total, lags, slot, nLags, bpl, pbPhasorShift(K.boxLog2), K.qa, K.a2, K.vectors, K.nvec, vp,
                     K.phasors, modes, counts);
  hipLaunchKernelGGL(k_fp_fold, dim3(cdiv(S->nsims * nLags * K.nvec, FT)), dim3(FT), 0, S->stream,
                     (const ulonglong2 *)modes, (const ulonglong2 *)counts, S->nsims, K.nvec, lags, nLags, K.lag.table,
                     K.lag.table + cells * PB_FP_WORDS);
  PB_TRY(hipGetLastError());
  PB_TRY(K.lag.clock.stop(S->stream));
  K.lag.book.recorded(S->stats.steps);
  return PB_OK;
}

extern "C" {

int pbSimSetFourPoint(pbSim *S, float interval, unsigned lags, float overlapRadius, int boxLog2, const int *vectors,
                      unsigned nvec) {
  const char *fn = "pbSimSetFourPoint";
  if (!S) return pbFail(fn, ": null handle");
  if (const int rc = pbLagCheckArgs(fn, interval, lags)) return rc;
  if (lags) {  // (lags == 0 switches off: the radius, the box and the list are not read)
    if (!(overlapRadius >= 0.0f && overlapRadius < 2048.0f)) return pbFail(fn, ": overlapRadius must be in [0, 2048)");
    if (!vectors) return pbFail(fn, ": null vectors");
    if (boxLog2 < PB_SK_MIN_LOG2 || boxLog2 > PB_SK_MAX_LOG2) return pbFail(fn, ": boxLog2 must be -8 ... 12");
    if (nvec < 1u || nvec > PB_FOURPOINT_MAX_VECTORS) return pbFail(fn, ": nvec must be 1 ... 256");
  }
  if (const int rc = pbLagCheckBatch<int2>(fn, S, lags)) return rc;
  if (lags && (unsigned long long)S->nsims * lags * nvec * (sizeof(unsigned long long) * (PB_FP_WORDS + PB_FP_MODE_WORDS)) > (1ull << 31))
    return pbFail(fn, ": the table (members x lags x nvec x (64 + 16) bytes) must not exceed 2^31 bytes");
  // per member and lag: the cells of the list and the four words of the pair counts
  return pbLagSwitch(S, S->fp, interval, lags, (size_t)nvec * PB_FP_WORDS + PB_FP_LAG_WORDS, [&](PbFourPoint &K) -> int {
    K.nvec = nvec, K.boxLog2 = boxLog2, K.radius = overlapRadius;
    K.qa = pbFpRadiusQuanta(overlapRadius), K.a2 = (unsigned long long)(K.qa * K.qa);  // qa < 2^31
    K.list.assign(vectors, vectors + 2u * (size_t)nvec);  // the list is copied at the call
    PB_TRY(K.scratch.alloc((size_t)S->nsims * lags * ((size_t)nvec * PB_FP_MODE_WORDS + PB_FP_COUNT_WORDS)));
    PB_TRY(K.phasors.alloc(PB_PHASOR_STEPS));
    PB_TRY(K.vectors.alloc(nvec));
    PB_TRY(hipMemcpyAsync(K.phasors, phasorTable(), sizeof(int2) * PB_PHASOR_STEPS, hipMemcpyHostToDevice, S->stream));
    PB_TRY(hipMemcpyAsync(K.vectors, K.list.data(), sizeof(int2) * nvec, hipMemcpyHostToDevice, S->stream));
    PB_TRY(hipStreamSynchronize(S->stream));  // (the two copies read host memory that may go with the next switch)
    return PB_OK;
  });
}

int pbSimFourPointRecord(pbSim *S) {
  return pbLagManualRecord("pbSimFourPointRecord", S, &pbSim::fp, WHAT, pbFourPointRecord);
}

int pbSimGetFourPointInfo(pbSim *S, float *interval, unsigned *lags, float *overlapRadius, int *boxLog2, unsigned *nvec,
                          unsigned long long *records) {
  const char *fn = "pbSimGetFourPointInfo";
  if (!S) return pbFail(fn, ": null handle");
  if (!interval && !lags && !overlapRadius && !boxLog2 && !nvec && !records)
    return pbFail(fn, ": interval, lags, overlapRadius, boxLog2, nvec and records are all null");
  if (interval) *interval = S->fp.lag.interval;
  if (lags) *lags = S->fp.lag.book.lags;
  if (overlapRadius) *overlapRadius = S->fp.radius;
  if (boxLog2) *boxLog2 = S->fp.boxLog2;
  if (nvec) *nvec = S->fp.nvec;
  if (records) *records = S->fp.lag.book.records;
  return PB_OK;
}

int pbSimGetFourPoint(pbSim *S, pbFourPointRow *rows) {
  const char *fn = "pbSimGetFourPoint";
  if (!S || !rows) return pbFail(fn, ": null handle or rows");
  const PbFourPoint &K = S->fp;
  if (const int rc = K.lag.checkOn(fn, WHAT)) return rc;
  for (unsigned long long origins : K.lag.book.origins)  // the book knows the count on the host: nothing is read back first
    if (origins >= (1ull << 31)) return pbFail(fn, std::string(": a lag holds 2^31 origins or more: restart the ") + WHAT);
  useDevice(S);
  const size_t cells = cellsOf(S, K);
  std::vector<unsigned long long> acc(K.lag.table.capacity());
  PB_TRY(hipMemcpyAsync(acc.data(), K.lag.table, sizeof(unsigned long long) * acc.size(), hipMemcpyDeviceToHost, S->stream));
  PB_TRY(hipStreamSynchronize(S->stream));
  const unsigned long long *lagCells = acc.data() + cells * PB_FP_WORDS;
  for (size_t c = 0; c < cells; c++) {
    const size_t g = c / K.nvec, k = c - g * K.nvec;
    const unsigned long long *w = acc.data() + c * PB_FP_WORDS, *p = lagCells + g * PB_FP_LAG_WORDS;
    pbFourPointRow &r = rows[c];
    K.lag.book.columns((unsigned)(g % K.lag.book.lags), r);
    r.nx = K.list[2u * k], r.ny = K.list[2u * k + 1u], r.reserved = 0u, r.reserved2 = 0ull;
    r.samples = p[PB_FP_SAMPLES], r.overlap = p[PB_FP_OVERLAP];
    for (int l = 0; l < 2; l++)
      r.overlap2[l] = p[PB_FP_OVERLAP2 + l], r.re[l] = w[PB_FP_RE + l], r.im[l] = w[PB_FP_IM + l];
    for (int l = 0; l < 3; l++) r.power[l] = w[PB_FP_POWER + l];
  }
  return PB_OK;
}

int pbSimGetFourPointTimes(pbSim *S, unsigned long long *records, float *last_device_ms) {
  return pbLagTimes("pbSimGetFourPointTimes", S, &pbSim::fp, records, last_device_ms);
}

}  // extern "C"
