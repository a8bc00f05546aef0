// pb_sfactor.hip -- the structure factor on gfx950: per member and wavevector of a caller's list, the integer sums
// sum a C[idx] and sum a S[idx] over the measured bots, the phasor of a bot being one entry of pb_phasor.hpp's table
// (pbSimStructureFactor / pbSimStructureFactorOf; include/particlebot_hip.h has the definitions).
//
//   k_sk_clear            zeroes the sums (2 / 4 / 8 64-bit words per member and wavevector) and the members' counters
//   k_sk_accumulate<KIND> the hot path, N x K: every measured bot against every wavevector.  The grid is (tile of 256
//                         wavevectors, bot chunk, member), at most PB_SK_BLOCKS chunks per member.  A workgroup copies
//                         the table into LDS once (32 KiB, cosine and sine interleaved: one 8-byte read per look-up),
//                         then stages 256 bots at a time, read in SLOT order (orig is never read), each lane quantising
//                         one bot into (qx, qy, a, a2), and walks the tile: a lane owns ONE wavevector and keeps its
//                         sums in registers; all lanes read the same staged bot, an LDS broadcast, so nothing is reduced
//                         per (bot, k).  An unmeasured bot, or a slot past the member's end, is staged with weights
//                         that add nothing (a = a2 = 0; for the density an all-zero mask instead of the all-ones one).
//                         At the end a lane adds its sums into the (member, k) cell with 64-bit integer atomics, and
//                         the tile-0 workgroups add the ballots' popcounts to the member's counter.
//                         PB_SK_DENSITY is its own instantiation: no multiply and two accumulators (|C| <= 2^30 and
//                         fewer than 2^28 bots: one signed 64-bit word holds the sum).  The others split every product
//                         with pb_fixed.hpp's pbFixedSplitAdd: |a C| <= 2^61, so a low accumulator stays below 2^60
//                         and a rest below 2^57.
// Everything that is added is an integer, so nothing depends on the slot order, on the kernel form or on the order of the
// adds.  No float atomics, no 128-bit atomics, no scratch memory.
#include <string.h>

#include "pb_engine.hpp"
#include "pb_fixed.hpp"
#include "pb_phasor.hpp"

static_assert(sizeof(pbStructureFactorRow) == 80, "a structure-factor row is 80 bytes");

namespace {

constexpr int ST = 256;
constexpr uint32_t SK_Z = 65535u;  // members per launch: the grid's third axis
// the words of a device cell: the density's two are whole signed sums, the others are split (low, rest)
enum { D_RE, D_IM, D_WORDS };
enum { W_RE_LO, W_RE_HI, W_IM_LO, W_IM_HI, W_RE2_LO, W_RE2_HI, W_IM2_LO, W_IM2_HI, W_WORDS };
constexpr uint32_t wordsOf(int kind) { return kind == PB_SK_DENSITY ? D_WORDS : kind == PB_SK_RADIUS ? W_RE2_LO : W_WORDS; }

__global__ __launch_bounds__(ST) void k_sk_clear(unsigned long long *__restrict__ cells, uint32_t words,
                                                 uint32_t *__restrict__ measured, uint32_t members) {
  const uint32_t i = blockIdx.x * ST + threadIdx.x;
  if (i < words) cells[i] = 0ull;
  if (i < members) measured[i] = 0u;
}

__device__ __forceinline__ void skAdd(unsigned long long *p, unsigned long long v) {
  if (v) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // no-return
}

template <int KIND>
__global__ __launch_bounds__(ST) void k_sk_accumulate(const float4 *__restrict__ pr, const float2 *__restrict__ vel,
                                                      uint32_t n, uint32_t firstMember, int shift,
                                                      const int2 *__restrict__ vectors, uint32_t nvec,
                                                      const int2 *__restrict__ table,
                                                      unsigned long long *__restrict__ cells,
                                                      uint32_t *__restrict__ measured) {
  __shared__ int2 sTab[PB_PHASOR_STEPS];  // (C[j], S[j])
  __shared__ int4 sBot[ST];               // (qx, qy, a, a2) of the tile's bots
  constexpr uint32_t WORDS = wordsOf(KIND);
  const uint32_t m = blockIdx.z, k = blockIdx.x * ST + threadIdx.x, lane = threadIdx.x & 63u;
  const uint32_t base = (firstMember + m) * n;  // a member's slots are its own block of the arrays; the batch is below 2^28 bots
  for (uint32_t j = threadIdx.x; j < PB_PHASOR_STEPS; j += ST) sTab[j] = table[j];
  const bool mine = k < nvec;
  // (wave-uniform) a wave past the end of the list walks no tile; it still stages bots and meets every barrier
  const bool walks = blockIdx.x * ST + (threadIdx.x & ~63u) < nvec;
  const int2 nv = mine ? vectors[k] : make_int2(0, 0);
  const uint32_t nx = (uint32_t)nv.x, ny = (uint32_t)nv.y;
  unsigned long long acc[WORDS];
#pragma unroll
  for (uint32_t c = 0; c < WORDS; c++) acc[c] = 0ull;
  uint32_t nMeasured = 0u;  // wave-uniform
  const uint32_t stride = gridDim.y * ST;
#pragma unroll 1
  for (uint32_t t0 = blockIdx.y * ST; t0 < n; t0 += stride) {  // (workgroup-uniform)
    const uint32_t i = t0 + threadIdx.x;
    int4 s = make_int4(0, 0, 0, 0);
    bool ok = false;
    if (i < n) {
      const float4 q = pr[base + i];
      ok = pbFixedInRange(q.x) && pbFixedInRange(q.y);
      float a = 0.0f, a2 = 0.0f;
      if (KIND == PB_SK_RADIUS) a = q.z;
      if (KIND == PB_SK_VELOCITY) {
        const float2 v = vel[base + i];
        a = v.x, a2 = v.y;
      }
      ok = ok && pbFixedInRange(a) && pbFixedInRange(a2);
      if (ok) {
        s.x = (int)pbFixedQuantise(q.x), s.y = (int)pbFixedQuantise(q.y);
        s.z = KIND == PB_SK_DENSITY ? -1 : (int)pbFixedQuantise(a);
        s.w = (int)pbFixedQuantise(a2);
      }
    }
    nMeasured += (uint32_t)__popcll(__ballot(ok));
    __syncthreads();  // the tile before this one has been walked (and, the first time, the table is stored)
    sBot[threadIdx.x] = s;
    __syncthreads();
    if (walks) {
      const uint32_t count = n - t0 < (uint32_t)ST ? n - t0 : (uint32_t)ST;
#pragma unroll 4
      for (uint32_t j = 0; j < count; j++) {
        const int4 p = sBot[j];  // the same address in every lane: a broadcast
        const int2 cs = sTab[pbPhasorIndex(pbPhasorTurn(nx, ny, (uint32_t)p.x, (uint32_t)p.y, shift))];
        if (KIND == PB_SK_DENSITY) {
          acc[D_RE] += (unsigned long long)(long long)(cs.x & p.z);
          acc[D_IM] += (unsigned long long)(long long)(cs.y & p.z);
        } else {
          pbFixedSplitAdd((long long)p.z * (long long)cs.x, acc[W_RE_LO], acc[W_RE_HI]);
          pbFixedSplitAdd((long long)p.z * (long long)cs.y, acc[W_IM_LO], acc[W_IM_HI]);
          if (KIND == PB_SK_VELOCITY) {
            pbFixedSplitAdd((long long)p.w * (long long)cs.x, acc[W_RE2_LO], acc[W_RE2_HI]);
            pbFixedSplitAdd((long long)p.w * (long long)cs.y, acc[W_IM2_LO], acc[W_IM2_HI]);
          }
        }
      }
    }
  }
  if (mine) {
    unsigned long long *cell = cells + ((size_t)m * nvec + k) * WORDS;
#pragma unroll
    for (uint32_t c = 0; c < WORDS; c++) skAdd(cell + c, acc[c]);
  }
  if (blockIdx.x == 0u && lane == 0u && nMeasured) atomicAdd(measured + m, nMeasured);
}

// the table, built once per process
const int *phasorTable() {
  static const std::vector<int> table = [] {
    std::vector<int> t(2u * PB_PHASOR_STEPS);
    pbPhasorBuild(t.data());
    return t;
  }();
  return table.data();
}

template <int KIND>
void launchAccumulate(pbSim *S, dim3 grid, uint32_t firstMember, int shift, uint32_t nvec, unsigned long long *cells,
                      uint32_t *measured) {
  hipLaunchKernelGGL(k_sk_accumulate<KIND>, grid, dim3(ST), 0, S->stream, S->pr[S->cur], S->vel[S->cur], S->n,
                     firstMember, shift, S->sk.vectors, nvec, S->sk.table, cells, measured);
}

// the rows of every member, or of member `firstMember` alone: the checks, the launches, the read-back
int structureFactor(const char *fn, pbSim *S, uint32_t firstMember, bool one, int kind, int boxLog2, const int *vectors,
                    unsigned nvec, pbStructureFactorRow *rows) {
  if (!S || !vectors || !rows) return pbFail(fn, ": null handle, vectors or rows");
  if (kind != PB_SK_DENSITY && kind != PB_SK_RADIUS && kind != PB_SK_VELOCITY)
    return pbFail(fn, ": kind must be PB_SK_DENSITY, PB_SK_RADIUS or PB_SK_VELOCITY");
  if (boxLog2 < PB_SK_MIN_LOG2 || boxLog2 > PB_SK_MAX_LOG2) return pbFail(fn, ": boxLog2 must be -8 ... 12");
  if (nvec < 1u || nvec > PB_SK_MAX_VECTORS) return pbFail(fn, ": nvec must be 1 ... 4096");
  // (the handle is read from here on: what comes before holds for any handle)
  if (one && firstMember >= S->nsims) return pbFail(fn, ": member out of range");
  const uint32_t members = one ? 1u : S->nsims;
  if ((unsigned long long)members * nvec * sizeof(pbStructureFactorRow) > (1ull << 31))
    return pbFail(fn, ": members x nvec x 80 bytes must not exceed 2^31 bytes");
  const int rc = pbCheckBatch(fn, S);
  if (rc != PB_OK) return rc;
  useDevice(S);
  PbSfactor &K = S->sk;
  const uint32_t W = wordsOf(kind);
  const size_t words = (size_t)members * nvec * W;  // below 2^28
  if (!K.table) {
    PB_TRY(K.table.alloc(PB_PHASOR_STEPS));
    PB_TRY(hipMemcpyAsync(K.table, phasorTable(), sizeof(int2) * PB_PHASOR_STEPS, hipMemcpyHostToDevice, S->stream));
  }
  PB_TRY(K.vectors.ensure(PB_SK_MAX_VECTORS));
  PB_TRY(K.cells.ensure(words));
  PB_TRY(K.measured.ensure(S->nsims));  // (4 bytes per member, whichever entry asks first)
  PB_TRY(hipMemcpyAsync(K.vectors, vectors, sizeof(int2) * nvec, hipMemcpyHostToDevice, S->stream));
  const uint32_t perMember = cdiv(S->n, ST);
  const uint32_t chunks = perMember < PB_SK_BLOCKS ? perMember : PB_SK_BLOCKS;
  const int shift = pbPhasorShift(boxLog2);
  PB_TRY(K.clock.start(S->stream));
  hipLaunchKernelGGL(k_sk_clear, dim3(cdiv((uint32_t)(words > members ? words : members), ST)), dim3(ST), 0, S->stream,
                     K.cells, (uint32_t)words, K.measured, members);
  for (uint32_t m0 = 0; m0 < members; m0 += SK_Z) {  // (one launch unless the batch has more than 65535 members)
    const uint32_t mz = members - m0 < SK_Z ? members - m0 : SK_Z;
    const dim3 grid(cdiv(nvec, ST), chunks, mz);
    unsigned long long *cells = K.cells + (size_t)m0 * nvec * W;
    if (kind == PB_SK_DENSITY) launchAccumulate<PB_SK_DENSITY>(S, grid, firstMember + m0, shift, nvec, cells, K.measured + m0);
    else if (kind == PB_SK_RADIUS) launchAccumulate<PB_SK_RADIUS>(S, grid, firstMember + m0, shift, nvec, cells, K.measured + m0);
    else launchAccumulate<PB_SK_VELOCITY>(S, grid, firstMember + m0, shift, nvec, cells, K.measured + m0);
  }
  PB_TRY(hipGetLastError());
  PB_TRY(K.clock.stop(S->stream));
  K.analyses++;
  // the counters ride behind the sums in one staging vector (two 32-bit counters per word)
  const size_t counterWords = ((size_t)members + 1u) / 2u;
  K.host.resize(words + counterWords);
  PB_TRY(hipMemcpyAsync(K.host.data(), K.cells, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, S->stream));
  PB_TRY(hipMemcpyAsync(K.host.data() + words, K.measured, sizeof(uint32_t) * members, hipMemcpyDeviceToHost, S->stream));
  PB_TRY(hipStreamSynchronize(S->stream));
  const pbMoment128 zero = pbFixedNormalised((__int128)0);
  for (uint32_t m = 0; m < members; m++) {
    uint32_t count;
    memcpy(&count, (const char *)(K.host.data() + words) + sizeof(uint32_t) * m, sizeof count);
    for (uint32_t k = 0; k < nvec; k++) {
      const unsigned long long *w = K.host.data() + ((size_t)m * nvec + k) * W;
      pbStructureFactorRow &r = rows[(size_t)m * nvec + k];
      r.nx = vectors[2u * k], r.ny = vectors[2u * k + 1u];
      r.measured = count, r.reserved = 0u;
      r.re2 = r.im2 = zero;
      if (kind == PB_SK_DENSITY) {
        r.re = pbFixedNormalised((__int128)(long long)w[D_RE]);
        r.im = pbFixedNormalised((__int128)(long long)w[D_IM]);
        continue;
      }
      r.re = pbFixedNormalised(pbFixedCompose(w[W_RE_LO], w[W_RE_HI]));
      r.im = pbFixedNormalised(pbFixedCompose(w[W_IM_LO], w[W_IM_HI]));
      if (kind == PB_SK_VELOCITY) {
        r.re2 = pbFixedNormalised(pbFixedCompose(w[W_RE2_LO], w[W_RE2_HI]));
        r.im2 = pbFixedNormalised(pbFixedCompose(w[W_IM2_LO], w[W_IM2_HI]));
      }
    }
  }
  return PB_OK;
}

}  // namespace

extern "C" {

int pbSimStructureFactor(pbSim *S, int kind, int boxLog2, const int *vectors, unsigned nvec, pbStructureFactorRow *rows) {
  return structureFactor("pbSimStructureFactor", S, 0u, false, kind, boxLog2, vectors, nvec, rows);
}

int pbSimStructureFactorOf(pbSim *S, unsigned member, int kind, int boxLog2, const int *vectors, unsigned nvec,
                           pbStructureFactorRow *rows) {
  return structureFactor("pbSimStructureFactorOf", S, member, true, kind, boxLog2, vectors, nvec, rows);
}

int pbSimGetStructureFactorTimes(pbSim *S, unsigned long long *analyses, float *last_device_ms) {
  if (!S) return pbFail("pbSimGetStructureFactorTimes", ": null handle");
  return pbSpanGet(S, S->sk.clock, S->sk.analyses, analyses, last_device_ms);
}

int pbPhasorTable(int *cosSin, unsigned cap) {
  if (!cosSin) return pbFail("pbPhasorTable", ": null table");
  if (cap < 2u * PB_PHASOR_STEPS) return pbFail("pbPhasorTable", ": cap must be at least 8192");
  memcpy(cosSin, phasorTable(), sizeof(int) * 2u * PB_PHASOR_STEPS);
  return PB_OK;
}

}  // extern "C"
