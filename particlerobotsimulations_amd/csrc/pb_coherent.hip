// pb_coherent.hip -- the coherent intermediate scattering function on gfx950: per member, lag and wavevector of a
// caller's list, the exact integer sum over time origins of  rho_k(t + tau) conj(rho_k(t)),  rho_k being the density mode
// (sum C[idx], sum S[idx]) over the measured bots, while pbSimStep runs (pbSimSetCoherent / pbSimCoherentRecord /
// pbSimGetCoherent; include/particlebot_hip.h has the definitions).  The book, the span clock, the interval rules and the
// shells of the entry points are the lag ring's (pb_engine.hpp, PbLagBook ... pbLagTimes); the ring itself holds modes,
// 16 bytes per (slot, member, vector) and a measured count per (slot, member), not bots.  The turn, the index and the
// table are pb_phasor.hpp's; the product, the 192-bit add and the cell are pb_coherent.hpp's; none is restated here.
//
//   k_coh_modes      the hot path, N x K per record, whatever the lag count.  The grid is (bot block, member), at most
//                    PB_COHERENT_BLOCKS blocks per member.  A workgroup of 256 lanes copies the table into LDS once
//                    (32 KiB, cosine and sine interleaved: one 8-byte read per look-up) and stages 256 bots at a time as
//                    k_sk_accumulate<PB_SK_DENSITY> does: posrad of the current copy in SLOT order, coalesced, each lane
//                    quantising one bot into (qx << shift, qy << shift, mask) -- the shift of the turn distributes over
//                    the sum mod 2^32 -- with the mask all ones, or all zeros for an unmeasured bot and for a slot past
//                    the member's end; orig is never read.  The lanes are k_scat_accumulate's (stripe, vector): Vp is
//                    nvec rounded up to a power of two, lane t owns vector t & (Vp - 1) and walks the staged bots stripe,
//                    stripe + 256 / Vp, ..., Vp of them whatever the member's end, so that the trip count is uniform
//                    and the unrolled look-ups overlap; the lanes of a stripe read the same staged bot (an LDS
//                    broadcast).  A lane keeps C and S in two 64-bit registers (|C| <= 2^30, fewer than 2^28 bots).
//                    The stripes that share a wave are folded with 64-bit shuffles and one lane per (wave, vector) adds
//                    into the ring slot's mode with 64-bit integer atomics.  The measured count is the staging ballots'
//                    popcounts, added once per wave.  The slot's modes and counts are zeroed on the stream in front of the launch.
//   k_coh_correlate  one launch per record for all the lags it is paired with, one lane per (member, lag, vector): the
//                    lane loads the two modes, forms the four signed 64 x 64 -> 128-bit products and adds re, im and the
//                    two counts into its own cell of eight words with plain loads and stores.  A cell has one owner and
//                    the launches of a stream are ordered, so there are no atomics here and no LDS.
// Everything that is added is an integer, so nothing depends on the slot order, on the kernel form that stepped or on the
// order of the adds.  No float atomics, no atomics wider than 64 bits, no scratch memory.  A record is these launches on
// the batch's stream between two events; the host never waits for them.
#include "pb_coherent.hpp"
#include "pb_engine.hpp"
#include "pb_fixed.hpp"
#include "pb_phasor.hpp"

static_assert(sizeof(pbCoherentRow) == 96, "a coherent row is 96 bytes");
static_assert(PB_COHERENT_MAX_VECTORS == 256u, "a workgroup of 256 lanes holds the whole list: one vector per lane");
static_assert(sizeof(ulonglong2) == sizeof(unsigned long long) * PB_COH_MODE_WORDS, "a mode is the ring's entry");

namespace {

constexpr int CT = PB_LAG_LANES;
constexpr const char *WHAT = "coherent scattering";

__global__ __launch_bounds__(CT) void k_coh_modes(const float4 *__restrict__ pr, uint32_t n, int shift,
                                                  const int2 *__restrict__ vectors, uint32_t nvec, uint32_t vp,
                                                  const int2 *__restrict__ phasors,
                                                  unsigned long long *__restrict__ modes,
                                                  uint32_t *__restrict__ measured) {
  __shared__ int2 sTab[PB_PHASOR_STEPS];  // (C[j], S[j])
  __shared__ int4 sBot[CT];               // (qx << shift, qy << shift, mask, 0) of the tile's bots
  const uint32_t member = blockIdx.y;
  const uint32_t base = member * n;  // a member's slots are its own block of the arrays; the batch is below 2^28 bots
  for (uint32_t j = threadIdx.x; j < PB_PHASOR_STEPS; j += CT) sTab[j] = phasors[j];
  // vp is a power of two, nvec <= vp <= 256: lane t is vector t & (vp - 1) of stripe t / vp, 256 / vp stripes
  const uint32_t k = threadIdx.x & (vp - 1u), stripe = threadIdx.x / vp, stripes = (uint32_t)CT / vp;
  const bool mine = k < nvec;
  // (wave-uniform) a wave whose first vector is past the end of the list walks nothing (vp >= 128 only); it still
  // stages bots and meets every barrier
  const bool walks = ((threadIdx.x & ~63u) & (vp - 1u)) < nvec;
  const int2 nv = mine ? vectors[k] : make_int2(0, 0);
  const uint32_t nx = (uint32_t)nv.x, ny = (uint32_t)nv.y;
  unsigned long long re = 0ull, im = 0ull;
  uint32_t nMeasured = 0u;  // wave-uniform
  const uint32_t stride = gridDim.x * CT;
#pragma unroll 1
  for (uint32_t t0 = blockIdx.x * CT; t0 < n; t0 += stride) {  // (workgroup-uniform)
    const uint32_t i = t0 + threadIdx.x;
    int4 s = make_int4(0, 0, 0, 0);
    bool ok = false;
    if (i < n) {
      const float4 q = pr[base + i];
      ok = pbFixedInRange(q.x) && pbFixedInRange(q.y);
      if (ok) {
        s.x = (int)((uint32_t)pbFixedQuantise(q.x) << shift), s.y = (int)((uint32_t)pbFixedQuantise(q.y) << shift);
        s.z = -1;
      }
    }
    nMeasured += (uint32_t)__popcll(__ballot(ok));
    __syncthreads();  // the tile before this one has been walked (and, the first time, the table is stored)
    sBot[threadIdx.x] = s;
    __syncthreads();
    if (walks) {
      // A lane walks its vp = 256 / stripes entries of the whole tile, the zero masks past the member's end included:
      // the trip count is the same in every lane, so the unrolled look-ups overlap instead of waiting for each other's
      // exit test
#pragma unroll 4
      for (uint32_t trip = 0, j = stripe; trip < vp; trip++, j += stripes) {
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
  if (mine && lane < vp) {
    unsigned long long *mode = modes + ((size_t)member * nvec + k) * PB_COH_MODE_WORDS;
    if (re) (void)__hip_atomic_fetch_add(mode + PB_COH_C, re, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // no-return
    if (im) (void)__hip_atomic_fetch_add(mode + PB_COH_S, im, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (lane == 0u && nMeasured) atomicAdd(measured + member, nMeasured);
}

__global__ __launch_bounds__(CT) void k_coh_correlate(const ulonglong2 *__restrict__ ring,
                                                      const uint32_t *__restrict__ measured, uint32_t nsims,
                                                      uint32_t nvec, uint32_t lags, uint32_t slotNow, uint32_t nLags,
                                                      unsigned long long *__restrict__ cells) {
  const uint32_t g = blockIdx.x * CT + threadIdx.x;  // nsims x lags x nvec is below 2^25 (the table's bound)
  if (g >= nsims * nLags * nvec) return;
  const uint32_t rest = g / nvec, k = g - rest * nvec;
  const uint32_t member = rest / nLags, lag = rest - member * nLags;
  const uint32_t slotThen = slotNow >= lag ? slotNow - lag : slotNow + lags - lag;  // lag < nLags <= lags
  const ulonglong2 now = ring[((size_t)slotNow * nsims + member) * nvec + k];
  const ulonglong2 then = ring[((size_t)slotThen * nsims + member) * nvec + k];
  pbCohPair(cells + (((size_t)member * lags + lag) * nvec + k) * PB_COH_WORDS, (long long)now.x, (long long)now.y,
            (long long)then.x, (long long)then.y, measured[slotNow * nsims + member], measured[slotThen * nsims + member]);
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

size_t cellsOf(const pbSim *S, const PbCoherent &K) { return (size_t)S->nsims * K.lag.book.lags * K.nvec; }

}  // namespace

int pbCoherentRecord(pbSim *S) {
  PbCoherent &K = S->co;
  uint32_t vp = 1u;
  while (vp < K.nvec) vp <<= 1;
  if (!S->coherentStripes) vp = (uint32_t)CT;  // one stripe: lane t owns vector t, as in k_sk_accumulate
  const uint32_t slot = K.lag.book.slot(), nLags = K.lag.book.paired();
  const uint32_t perMember = cdiv(S->n, CT);
  const uint32_t blocks = perMember < PB_COHERENT_BLOCKS ? perMember : PB_COHERENT_BLOCKS;
  const size_t perSlot = (size_t)S->nsims * K.nvec;
  ulonglong2 *modes = K.lag.ring + slot * perSlot;
  uint32_t *measured = K.measured + (size_t)slot * S->nsims;
  PB_TRY(K.lag.clock.start(S->stream));
  PB_TRY(hipMemsetAsync(modes, 0, sizeof(ulonglong2) * perSlot, S->stream));
  PB_TRY(hipMemsetAsync(measured, 0, sizeof(uint32_t) * S->nsims, S->stream));
  hipLaunchKernelGGL(k_coh_modes, dim3(blocks, S->nsims), dim3(CT), 0, S->stream, S->pr[S->cur], S->n,
                     pbPhasorShift(K.boxLog2), K.vectors, K.nvec, vp, K.phasors, (unsigned long long *)modes, measured);
  hipLaunchKernelGGL(k_coh_correlate, dim3(cdiv(S->nsims * nLags * K.nvec, CT)), dim3(CT), 0, S->stream, K.lag.ring,
                     K.measured, S->nsims, K.nvec, K.lag.book.lags, slot, nLags, K.lag.table);
  PB_TRY(hipGetLastError());
  PB_TRY(K.lag.clock.stop(S->stream));
  K.lag.book.recorded(S->stats.steps);
  return PB_OK;
}

extern "C" {

int pbSimSetCoherent(pbSim *S, float interval, unsigned lags, int boxLog2, const int *vectors, unsigned nvec) {
  const char *fn = "pbSimSetCoherent";
  if (!S) return pbFail(fn, ": null handle");
  if (const int rc = pbLagCheckArgs(fn, interval, lags)) return rc;
  if (lags) {  // (lags == 0 switches off: the box and the list are not read)
    if (!vectors) return pbFail(fn, ": null vectors");
    if (boxLog2 < PB_SK_MIN_LOG2 || boxLog2 > PB_SK_MAX_LOG2) return pbFail(fn, ": boxLog2 must be -8 ... 12");
    if (nvec < 1u || nvec > PB_COHERENT_MAX_VECTORS) return pbFail(fn, ": nvec must be 1 ... 256");
  }
  if (lags) {  // (a batch that can never have the recorder on may still switch it off)
    if (S->nsims > 65535u) return pbFail(fn, ": the batch must hold at most 65535 members");  // the member is a grid's y
    if (const int rc = pbCheckBatch(fn, S)) return rc;
    if ((unsigned long long)S->nsims * lags * nvec * (sizeof(ulonglong2) + 48u) > (1ull << 31))
      return pbFail(fn, ": the ring and the sums (members x lags x nvec x (16 + 48) bytes) must not exceed 2^31 bytes");
  }
  return pbLagSwitch(S, S->co, interval, lags, (size_t)nvec * PB_COH_WORDS, [&](PbCoherent &K) -> int {
    K.nvec = nvec, K.boxLog2 = boxLog2;
    K.list.assign(vectors, vectors + 2u * (size_t)nvec);  // the list is copied at the call
    PB_TRY(K.measured.alloc((size_t)lags * S->nsims));
    PB_TRY(K.phasors.alloc(PB_PHASOR_STEPS));
    PB_TRY(K.vectors.alloc(nvec));
    PB_TRY(hipMemcpyAsync(K.phasors, phasorTable(), sizeof(int2) * PB_PHASOR_STEPS, hipMemcpyHostToDevice, S->stream));
    PB_TRY(hipMemcpyAsync(K.vectors, K.list.data(), sizeof(int2) * nvec, hipMemcpyHostToDevice, S->stream));
    PB_TRY(hipStreamSynchronize(S->stream));  // (the two copies read host memory that may go with the next switch)
    return PB_OK;
  }, (size_t)S->nsims * nvec);
}

int pbSimCoherentRecord(pbSim *S) {
  return pbLagManualRecord("pbSimCoherentRecord", S, &pbSim::co, WHAT, pbCoherentRecord);
}

int pbSimGetCoherentInfo(pbSim *S, float *interval, unsigned *lags, int *boxLog2, unsigned *nvec,
                         unsigned long long *records) {
  if (!S) return pbFail("pbSimGetCoherentInfo", ": null handle");
  if (!interval && !lags && !boxLog2 && !nvec && !records)
    return pbFail("pbSimGetCoherentInfo", ": interval, lags, boxLog2, nvec and records are all null");
  if (interval) *interval = S->co.lag.interval;
  if (lags) *lags = S->co.lag.book.lags;
  if (boxLog2) *boxLog2 = S->co.boxLog2;
  if (nvec) *nvec = S->co.nvec;
  if (records) *records = S->co.lag.book.records;
  return PB_OK;
}

int pbSimGetCoherent(pbSim *S, pbCoherentRow *rows) {
  const char *fn = "pbSimGetCoherent";
  if (!S || !rows) return pbFail(fn, ": null handle or rows");
  const PbCoherent &K = S->co;
  if (const int rc = K.lag.checkOn(fn, WHAT)) return rc;
  for (unsigned long long origins : K.lag.book.origins)  // the book knows the count on the host: nothing is read back first
    if (origins >= (1ull << 31)) return pbFail(fn, std::string(": a lag holds 2^31 origins or more: restart the ") + WHAT);
  useDevice(S);
  const size_t cells = cellsOf(S, K);
  std::vector<unsigned long long> acc(cells * PB_COH_WORDS);
  PB_TRY(hipMemcpyAsync(acc.data(), K.lag.table, sizeof(unsigned long long) * acc.size(), hipMemcpyDeviceToHost, S->stream));
  PB_TRY(hipStreamSynchronize(S->stream));
  for (size_t c = 0; c < cells; c++) {
    const size_t g = c / K.nvec, k = c - g * K.nvec;
    const unsigned long long *w = acc.data() + c * PB_COH_WORDS;
    pbCoherentRow &r = rows[c];
    K.lag.book.columns((unsigned)(g % K.lag.book.lags), r);
    r.nx = K.list[2u * k], r.ny = K.list[2u * k + 1u], r.reserved = 0u;
    r.bots_now = w[PB_COH_BOTS_NOW], r.bots_then = w[PB_COH_BOTS_THEN];
    for (int l = 0; l < 3; l++) r.re[l] = w[PB_COH_RE + l], r.im[l] = w[PB_COH_IM + l];
  }
  return PB_OK;
}

int pbSimGetCoherentTimes(pbSim *S, unsigned long long *records, float *last_device_ms) {
  return pbLagTimes("pbSimGetCoherentTimes", S, &pbSim::co, records, last_device_ms);
}

}  // extern "C"
