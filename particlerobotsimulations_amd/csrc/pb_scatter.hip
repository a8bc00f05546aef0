// pb_scatter.hip -- the self-intermediate scattering function on gfx950: per member, lag and wavevector of a caller's
// list, the integer sums  sum C[idx]  and  sum S[idx]  over the measured (bot, origin) pairs, idx being the table step of
// k . (r(t + tau) - r(t)), averaged over time origins while pbSimStep runs (pbSimSetScattering / pbSimScatteringRecord /
// pbSimGetScattering; include/particlebot_hip.h has the definitions).  The ring of snapshots, its pairing lag by lag, its
// book and the shells of the entry points are the lag ring's (pb_engine.hpp, PbLagBook ... pbLagTimes); the turn, the
// index and the table are pb_phasor.hpp's; neither is restated here.  The table is two 64-bit words per member, lag and
// wavevector, and one sample counter per member and lag behind them.
//
//   k_scat_snapshot    one pass over pr[cur] and orig[cur] in SLOT order (coalesced reads); each lane quantises one bot
//                      and writes one int2 (qx, qy) to ring[slot][member * n + orig]; an out-of-range bot is stored as
//                      (INT32_MIN, 0), which no measured bot can be.  The scattered 8-byte store is the only uncoalesced
//                      access.
//   k_scat_accumulate  the hot path, N x lags x K.  One workgroup of 256 lanes per (member, lag, bot block), at most
//                      PB_SCATTER_BLOCKS blocks per member and lag, all lags of a record in one launch.  A workgroup
//                      copies the table into LDS once (32 KiB, cosine and sine interleaved: one 8-byte read per look-up)
//                      and stages 256 pairs at a time from coalesced 8-byte loads of the two snapshots in ORIGINAL order:
//                      (dqx << shift, dqy << shift, mask), the shift of the turn applied once per pair instead of once
//                      per (pair, k) -- it distributes over the sum mod 2^32 -- and the mask all ones, or all zeros for
//                      an unmeasured pair and for a slot past the member's end, so that such a pair adds nothing.
//                      The lanes are (stripe, vector): Vp is nvec rounded up to a power of two, lane t owns vector
//                      t & (Vp - 1) and walks the staged pairs stripe, stripe + 256 / Vp, ... with stripe = t / Vp.  The
//                      lanes of a stripe read the same staged pair (an LDS broadcast), so nothing is reduced per
//                      (pair, k), and with 8 ... 64 vectors every lane works.  A lane keeps re and im in two 64-bit
//                      registers.  At the end the stripes that share a wave (Vp < 64) are folded with a butterfly of
//                      64-bit shuffles, and one lane per (wave, vector) adds the two sums into the (member, lag, k) cell
//                      with 64-bit integer atomics: at most 2 x 256 atomics per workgroup whatever nvec.  (The other
//                      choice, folding all stripes through LDS to 2 x Vp atomics, would reuse the table's LDS behind one
//                      more barrier; it was not built: see profiles/intermediate_scattering.txt.)
//                      The samples are the staging ballots' popcounts, added once per wave to the (member, lag) counter.
// Everything that is added is an integer, so nothing depends on the slot order, on the kernel form that stepped or on the
// order of the adds.  |C| <= 2^30 and fewer than 2^31 samples: one signed 64-bit word holds a sum (below 2^61), so there
// are no split accumulators, no float atomics, no 128-bit atomics and no scratch memory.  A record is these launches on
// the batch's stream between two events; the host never waits for them.
#include <limits.h>

#include "pb_engine.hpp"
#include "pb_fixed.hpp"
#include "pb_phasor.hpp"

static_assert(sizeof(pbScatteringRow) == 56, "a scattering row is 56 bytes");
static_assert(PB_SCATTER_MAX_VECTORS == 256u, "a workgroup of 256 lanes holds the whole list: one vector per lane");

namespace {

constexpr int SC = PB_LAG_LANES;
enum { C_RE, C_IM, C_WORDS };  // the words of a table cell

__global__ __launch_bounds__(SC) void k_scat_snapshot(const float4 *__restrict__ pr, const uint32_t *__restrict__ orig,
                                                      uint32_t n, int2 *__restrict__ snap) {
  const uint32_t l = blockIdx.x * SC + threadIdx.x;
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

__global__ __launch_bounds__(SC) void k_scat_accumulate(const int2 *__restrict__ ring, uint32_t n, uint32_t total,
                                                        uint32_t lags, uint32_t slotNow, uint32_t nLags,
                                                        uint32_t blocksPerLag, int shift,
                                                        const int2 *__restrict__ vectors, uint32_t nvec, uint32_t vp,
                                                        const int2 *__restrict__ phasors,
                                                        unsigned long long *__restrict__ cells,
                                                        unsigned long long *__restrict__ samples) {
  __shared__ int2 sTab[PB_PHASOR_STEPS];  // (C[j], S[j])
  __shared__ int4 sPair[SC];              // (dqx << shift, dqy << shift, mask, 0) of the tile's pairs
  const auto [member, lag, b, now, then] = pbLagPair(ring, n, total, lags, slotNow, nLags, blocksPerLag);
  for (uint32_t j = threadIdx.x; j < PB_PHASOR_STEPS; j += SC) sTab[j] = phasors[j];
  // vp is a power of two, nvec <= vp <= 256: lane t is vector t & (vp - 1) of stripe t / vp, 256 / vp stripes
  const uint32_t k = threadIdx.x & (vp - 1u), stripe = threadIdx.x / vp, stripes = (uint32_t)SC / vp;
  const bool mine = k < nvec;
  // (wave-uniform) a wave whose first vector is past the end of the list walks nothing (vp >= 128 only); it still
  // stages pairs and meets every barrier
  const bool walks = ((threadIdx.x & ~63u) & (vp - 1u)) < nvec;
  const int2 nv = mine ? vectors[k] : make_int2(0, 0);
  const uint32_t nx = (uint32_t)nv.x, ny = (uint32_t)nv.y;
  unsigned long long re = 0ull, im = 0ull;
  uint32_t nMeasured = 0u;  // wave-uniform
#pragma unroll 1
  for (uint32_t t0 = b * SC; t0 < n; t0 += blocksPerLag * SC) {  // (workgroup-uniform)
    const uint32_t i = t0 + threadIdx.x;
    int4 s = make_int4(0, 0, 0, 0);
    bool ok = false;
    if (i < n) {
      const int2 u = now[i], z = then[i];
      ok = u.x != INT_MIN && z.x != INT_MIN;
      if (ok) {
        s.x = (int)(((uint32_t)u.x - (uint32_t)z.x) << shift), s.y = (int)(((uint32_t)u.y - (uint32_t)z.y) << shift);
        s.z = -1;
      }
    }
    nMeasured += (uint32_t)__popcll(__ballot(ok));
    __syncthreads();  // the tile before this one has been walked (and, the first time, the table is stored)
    sPair[threadIdx.x] = s;
    __syncthreads();
    if (walks) {
      const uint32_t count = n - t0 < (uint32_t)SC ? n - t0 : (uint32_t)SC;
#pragma unroll 4
      for (uint32_t j = stripe; j < count; j += stripes) {
        const int4 p = sPair[j];  // the same address in every lane of a stripe: a broadcast
        // (nx dqx + ny dqy) << shift == nx (dqx << shift) + ny (dqy << shift) mod 2^32: the turn with the shift staged
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
  if (mine && lane < vp) {
    unsigned long long *cell = cells + (((size_t)member * lags + lag) * nvec + k) * C_WORDS;
    if (re) (void)__hip_atomic_fetch_add(cell + C_RE, re, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // no-return
    if (im) (void)__hip_atomic_fetch_add(cell + C_IM, im, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (lane == 0u && nMeasured)
    (void)__hip_atomic_fetch_add(samples + (size_t)member * lags + lag, (unsigned long long)nMeasured, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
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

size_t cellsOf(const pbSim *S, const PbScattering &K) { return (size_t)S->nsims * K.lag.book.lags * K.nvec; }

}  // namespace

int pbScatteringRecord(pbSim *S) {
  PbScattering &K = S->sc;
  uint32_t vp = 1u;
  while (vp < K.nvec) vp <<= 1;
  const int c = S->cur;
  return pbLagRecord(S, K.lag, [&](dim3 grid, int2 *snap) {
    hipLaunchKernelGGL(k_scat_snapshot, grid, dim3(SC), 0, S->stream, S->pr[c], S->orig[c], S->n, snap);
  }, [&](dim3 grid, uint32_t slot, uint32_t nLags, uint32_t bpl) {
    hipLaunchKernelGGL(k_scat_accumulate, grid, dim3(SC), 0, S->stream, K.lag.ring, S->n, S->total, K.lag.book.lags,
                       slot, nLags, bpl, pbPhasorShift(K.boxLog2), K.vectors, K.nvec, vp, K.phasors, K.lag.table,
                       K.lag.table + cellsOf(S, K) * C_WORDS);
  });
}

extern "C" {

int pbSimSetScattering(pbSim *S, float interval, unsigned lags, int boxLog2, const int *vectors, unsigned nvec) {
  const char *fn = "pbSimSetScattering";
  if (!S) return pbFail(fn, ": null handle");
  if (const int rc = pbLagCheckArgs(fn, interval, lags)) return rc;
  if (lags) {  // (lags == 0 switches off: the box and the list are not read)
    if (!vectors) return pbFail(fn, ": null vectors");
    if (boxLog2 < PB_SK_MIN_LOG2 || boxLog2 > PB_SK_MAX_LOG2) return pbFail(fn, ": boxLog2 must be -8 ... 12");
    if (nvec < 1u || nvec > PB_SCATTER_MAX_VECTORS) return pbFail(fn, ": nvec must be 1 ... 256");
  }
  if (const int rc = pbLagCheckBatch<int2>(fn, S, lags)) return rc;
  if (lags && (unsigned long long)S->nsims * lags * nvec * (sizeof(unsigned long long) * C_WORDS) > (1ull << 31))
    return pbFail(fn, ": the table (members x lags x nvec x 16 bytes) must not exceed 2^31 bytes");
  // per member and lag: the cells of the list and one sample counter (below 2^28 + 2^22 words in all)
  return pbLagSwitch(S, S->sc, interval, lags, (size_t)nvec * C_WORDS + 1u, [&](PbScattering &K) -> int {
    K.nvec = nvec, K.boxLog2 = boxLog2;
    K.list.assign(vectors, vectors + 2u * (size_t)nvec);  // the list is copied at the call
    PB_TRY(K.phasors.alloc(PB_PHASOR_STEPS));
    PB_TRY(K.vectors.alloc(nvec));
    PB_TRY(hipMemcpyAsync(K.phasors, phasorTable(), sizeof(int2) * PB_PHASOR_STEPS, hipMemcpyHostToDevice, S->stream));
    PB_TRY(hipMemcpyAsync(K.vectors, K.list.data(), sizeof(int2) * nvec, hipMemcpyHostToDevice, S->stream));
    PB_TRY(hipStreamSynchronize(S->stream));  // (the two copies read host memory that may go with the next switch)
    return PB_OK;
  });
}

int pbSimScatteringRecord(pbSim *S) {
  return pbLagManualRecord("pbSimScatteringRecord", S, &pbSim::sc, "scattering", pbScatteringRecord);
}

int pbSimGetScatteringInfo(pbSim *S, float *interval, unsigned *lags, int *boxLog2, unsigned *nvec,
                           unsigned long long *records) {
  if (!S) return pbFail("pbSimGetScatteringInfo", ": null handle");
  if (!interval && !lags && !boxLog2 && !nvec && !records)
    return pbFail("pbSimGetScatteringInfo", ": interval, lags, boxLog2, nvec and records are all null");
  if (interval) *interval = S->sc.lag.interval;
  if (lags) *lags = S->sc.lag.book.lags;
  if (boxLog2) *boxLog2 = S->sc.boxLog2;
  if (nvec) *nvec = S->sc.nvec;
  if (records) *records = S->sc.lag.book.records;
  return PB_OK;
}

int pbSimGetScattering(pbSim *S, pbScatteringRow *rows) {
  if (!S || !rows) return pbFail("pbSimGetScattering", ": null handle or rows");
  const PbScattering &K = S->sc;
  const size_t cells = cellsOf(S, K);
  std::vector<unsigned long long> acc;
  if (const int rc = pbLagFetch("pbSimGetScattering", S, K.lag, "scattering", acc, cells * C_WORDS, 1u)) return rc;
  const unsigned long long *count = acc.data() + cells * C_WORDS;
  for (size_t c = 0; c < cells; c++) {
    const size_t g = c / K.nvec, k = c - g * K.nvec;
    pbScatteringRow &r = rows[c];
    K.lag.book.columns((unsigned)(g % K.lag.book.lags), r);
    r.nx = K.list[2u * k], r.ny = K.list[2u * k + 1u], r.reserved = 0u, r.samples = count[g];
    r.re = (long long)acc[c * C_WORDS + C_RE], r.im = (long long)acc[c * C_WORDS + C_IM];
  }
  return PB_OK;
}

int pbSimGetScatteringTimes(pbSim *S, unsigned long long *records, float *last_device_ms) {
  return pbLagTimes("pbSimGetScatteringTimes", S, &pbSim::sc, records, last_device_ms);
}

}  // extern "C"
