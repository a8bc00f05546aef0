// pb_field.hip -- field maps on gfx950: per cell of a regular grid over a view, the bots in it, the dead among them and
// the integer sums of radius, radius^2, velocity and |v|^2 (pbSimFieldMap / pbSimFieldMapOf; include/particlebot_hip.h
// has the definitions).
//
//   k_field_clear       zeroes the map (eight 64-bit words per cell) and the totals (four 32-bit words per member)
//   k_field_accumulate  the hot path: one pass over pr[cur], vel[cur] and dead[cur] of the members asked for in SLOT order
//                       (16 + 8 + 4 bytes per bot, coalesced; orig is never read).  Up to PB_FIELD_BLOCKS workgroups per
//                       member, each wave a grid-stride loop over its member's slots.  Per trip a lane holds one bot: its
//                       cell key and eight 64-bit values.  The state is kept cell-sorted, so the lanes of a wave mostly
//                       share a few keys: a LEADER LOOP takes the first remaining lane's key, ballots the lanes that hold
//                       the same key, sums the eight values over them with a wave butterfly and has lanes 0 ... 7 add one
//                       word each, one 64-byte atomic instruction for the whole group (a group of one lane skips the
//                       butterfly).  After PB_FIELD_ROUNDS rounds (wave-uniform) whatever is left, a wave over a map so
//                       fine that every lane has a cell of its own, goes out as eight atomics per lane.
//                       PB_FIELD_ROUNDS=0 is the plain form, eight atomics per counted bot and no combine; it is built
//                       only for tools/field_cost.py, which records both.
// The counters of a member (measured, inside, outside, unmeasured) are ballots' popcounts kept wave-uniform and added
// once per wave.
// Everything that is added is an integer, so nothing depends on the slot order, on the kernel form or on the order of the
// adds.  No float atomics, no 128-bit atomics, no scratch memory.  The bounds are pb_fixed.hpp's: a cell
// holds fewer than 2^28 bots, so every word stays below 2^60.
#include <math.h>
#include <string.h>

#include "pb_engine.hpp"
#include "pb_fixed.hpp"

static_assert(sizeof(pbFieldCell) == 64, "a map cell is 64 bytes");
static_assert(sizeof(pbFieldTotals) == 16, "a member's totals are 16 bytes");
static_assert(sizeof(pbFieldView) == 24, "a view is 24 bytes");

#ifndef PB_FIELD_ROUNDS
#define PB_FIELD_ROUNDS 4  // leader-loop rounds per wave and trip before the per-lane fallback, by measurement (profiles/field_maps.txt)
#endif

namespace {

constexpr int FT = 256;
constexpr uint32_t NO_CELL = 0xFFFFFFFFu;
// the words of a device cell; F_COUNT holds count + (dead << 32)
enum { F_COUNT, F_QR, F_WX, F_WY, F_RR_LO, F_RR_HI, F_VV_LO, F_VV_HI, F_WORDS };
static_assert(F_WORDS * sizeof(unsigned long long) == sizeof(pbFieldCell), "device and host cell are the same size");
// the words of a member's totals
enum { N_MEASURED, N_INSIDE, N_OUTSIDE, N_UNMEASURED, N_WORDS };

// what the host derives from the view once: tx = (x - x0) * sx, inside iff 0 <= tx < fnx
struct FieldGrid {
  float x0, sx, y0, sy, fnx, fny;
  uint32_t nx, cells;  // cells = nx * ny
};

__global__ __launch_bounds__(FT) void k_field_clear(unsigned long long *__restrict__ cells, uint32_t words,
                                                    uint32_t *__restrict__ totals, uint32_t totalWords) {
  const uint32_t i = blockIdx.x * FT + threadIdx.x;
  if (i < words) cells[i] = 0ull;
  if (i < totalWords) totals[i] = 0u;
}

__device__ __forceinline__ void fieldAdd(unsigned long long *p, unsigned long long v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // no-return
}

__global__ __launch_bounds__(FT) void k_field_accumulate(const float4 *__restrict__ pr, const float2 *__restrict__ vel,
                                                         const int *__restrict__ dead, uint32_t n, uint32_t firstMember,
                                                         uint32_t blocksPerMember, FieldGrid G,
                                                         unsigned long long *__restrict__ cells,
                                                         uint32_t *__restrict__ totals) {
  const uint32_t m = blockIdx.x / blocksPerMember, b = blockIdx.x - m * blocksPerMember;
  const uint32_t base = (firstMember + m) * n;  // a member's slots are its own block of the arrays; the batch is below 2^28 bots
  unsigned long long *__restrict__ map = cells + (size_t)m * G.cells * F_WORDS;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t nMeasured = 0u, nInside = 0u, nLive = 0u;  // wave-uniform
  // the trip's first slot is wave-uniform: every lane of a wave runs the same trips and meets every ballot and shuffle.
  // A wave has few trips' worth of company on its SIMD, so the next trip's loads are issued ahead of this trip's work.
  const uint32_t stride = blocksPerMember * FT;
  uint32_t w0 = b * FT + (threadIdx.x & ~63u);
  float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float2 v = make_float2(0.0f, 0.0f);
  int isDead = 0;
  if (w0 < n) {
    const uint32_t s = base + (w0 + lane < n ? w0 + lane : w0);
    q = pr[s], v = vel[s], isDead = dead[s];
  }
#pragma unroll 1
  while (w0 < n) {
    const uint32_t i = w0 + lane, next = w0 + stride;
    const bool live = i < n;
    float4 qNext = q;
    float2 vNext = v;
    int deadNext = isDead;
    if (next < n) {
      const uint32_t s = base + (next + lane < n ? next + lane : next);
      qNext = pr[s], vNext = vel[s], deadNext = dead[s];
    }
    const bool measured = live && pbFixedInRange(q.x) && pbFixedInRange(q.y) && pbFixedInRange(v.x) &&
                          pbFixedInRange(v.y) && pbFixedInRange(q.z);
    const float tx = (q.x - G.x0) * G.sx, ty = (q.y - G.y0) * G.sy;  // two roundings each
    const bool inside = measured && tx >= 0.0f && tx < G.fnx && ty >= 0.0f && ty < G.fny;  // (-0.0f is inside, in 0)
    const uint32_t key = inside ? (uint32_t)(int)ty * G.nx + (uint32_t)(int)tx : NO_CELL;
    nLive += (uint32_t)__popcll(__ballot(live));
    nMeasured += (uint32_t)__popcll(__ballot(measured));
    unsigned long long remaining = __ballot(inside);
    nInside += (uint32_t)__popcll(remaining);
    unsigned long long a[F_WORDS];
    {
      // (a bot that is not counted stands in as zeros: its values are read by no one, and none is converted)
      const long long qr = pbFixedQuantise(inside ? q.z : 0.0f), wx = pbFixedQuantise(inside ? v.x : 0.0f);
      const long long wy = pbFixedQuantise(inside ? v.y : 0.0f);
      const long long rr = qr * qr, vv = wx * wx + wy * wy;  // below 2^62 and 2^63
      a[F_COUNT] = 1ull + ((unsigned long long)(isDead != 0) << 32);
      a[F_QR] = (unsigned long long)qr, a[F_WX] = (unsigned long long)wx, a[F_WY] = (unsigned long long)wy;
      a[F_RR_LO] = pbFixedLow(rr), a[F_RR_HI] = pbFixedRest(rr);
      a[F_VV_LO] = pbFixedLow(vv), a[F_VV_HI] = pbFixedRest(vv);
    }
#pragma unroll 1
    for (int round = 0; round < PB_FIELD_ROUNDS && remaining; round++) {
      const int leader = __ffsll((long long)remaining) - 1;
      const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);  // a cell: never NO_CELL
      const bool same = key == k;
      const unsigned long long group = __ballot(same);
      remaining &= ~group;
      unsigned long long *cell = map + (size_t)k * F_WORDS;
      if (group == (1ull << leader)) {  // (wave-uniform) a group of one: its lane adds its own eight words
        if (same) {
#pragma unroll
          for (int c = 0; c < F_WORDS; c++)
            if (a[c]) fieldAdd(cell + c, a[c]);
        }
        continue;
      }
      unsigned long long t[F_WORDS];
#pragma unroll
      for (int c = 0; c < F_WORDS; c++) t[c] = same ? a[c] : 0ull;
      waveSumRolled(t, [](int) {});
      // every lane holds the group's eight sums: lane c adds word c, one 64-byte atomic instruction
      unsigned long long mine = t[0];
#pragma unroll
      for (int c = 1; c < F_WORDS; c++) mine = lane == (uint32_t)c ? t[c] : mine;
      if (lane < (uint32_t)F_WORDS && mine) fieldAdd(cell + lane, mine);  // (a signed sum that is zero adds nothing)
    }
    if ((remaining >> lane) & 1ull) {  // past the rounds, or the plain form: eight atomics per lane
      unsigned long long *cell = map + (size_t)key * F_WORDS;
#pragma unroll
      for (int c = 0; c < F_WORDS; c++)
        if (a[c]) fieldAdd(cell + c, a[c]);
    }
    q = qNext, v = vNext, isDead = deadNext, w0 = next;
  }
  if (lane == 0u) {
    uint32_t *t = totals + (size_t)m * N_WORDS;
    if (nMeasured) atomicAdd(t + N_MEASURED, nMeasured);
    if (nInside) atomicAdd(t + N_INSIDE, nInside);
    if (nMeasured - nInside) atomicAdd(t + N_OUTSIDE, nMeasured - nInside);
    if (nLive - nMeasured) atomicAdd(t + N_UNMEASURED, nLive - nMeasured);
  }
}

// one map of every member, or of member `firstMember` alone: the checks, the two launches, the read-back
int fieldMap(const char *fn, pbSim *S, uint32_t firstMember, bool one, const pbFieldView *view, pbFieldCell *out,
             pbFieldTotals *totals) {
  if (!S || !view || !out) return pbFail(fn, ": null handle, view or cells");
  if (view->nx < 1u || view->nx > PB_FIELD_MAX_AXIS || view->ny < 1u || view->ny > PB_FIELD_MAX_AXIS)
    return pbFail(fn, ": nx and ny must be 1 ... 1024");
  const float inf = __builtin_inff();
  if (!(view->halfX > 0.0f) || !(view->halfX < inf) || !(view->halfY > 0.0f) || !(view->halfY < inf))
    return pbFail(fn, ": halfX and halfY must be finite and > 0");
  FieldGrid G;
  G.x0 = view->centerX - view->halfX, G.y0 = view->centerY - view->halfY;
  G.sx = (float)view->nx / (view->halfX + view->halfX), G.sy = (float)view->ny / (view->halfY + view->halfY);
  G.fnx = (float)view->nx, G.fny = (float)view->ny;
  G.nx = view->nx, G.cells = view->nx * view->ny;
  if (!(fabsf(G.x0) < inf) || !(fabsf(G.y0) < inf) || !(fabsf(G.sx) < inf) || !(fabsf(G.sy) < inf))
    return pbFail(fn, ": the view's origin and scale must be finite");
  // (the handle is read from here on: what comes before holds for any handle)
  if (one && firstMember >= S->nsims) return pbFail(fn, ": member out of range");
  const uint32_t members = one ? 1u : S->nsims;
  if ((unsigned long long)members * G.cells * sizeof(pbFieldCell) > (1ull << 31))
    return pbFail(fn, ": members x nx x ny x 64 bytes must not exceed 2^31 bytes");
  const int rc = pbCheckBatch(fn, S);
  if (rc != PB_OK) return rc;
  useDevice(S);
  PbField &F = S->field;
  const size_t words = (size_t)members * G.cells * F_WORDS, totalWords = (size_t)S->nsims * N_WORDS;
  PB_TRY(F.cells.ensure(words));
  PB_TRY(F.totals.ensure(totalWords));  // (16 bytes per member, whichever entry asks first)
  const uint32_t perMember = cdiv(S->n, FT);
  const uint32_t bpm = perMember < PB_FIELD_BLOCKS ? perMember : PB_FIELD_BLOCKS;
  PB_TRY(F.clock.start(S->stream));
  hipLaunchKernelGGL(k_field_clear, dim3(cdiv((uint32_t)words, FT)), dim3(FT), 0, S->stream, F.cells, (uint32_t)words,
                     F.totals, members * (uint32_t)N_WORDS);
  hipLaunchKernelGGL(k_field_accumulate, dim3(members * bpm), dim3(FT), 0, S->stream, S->pr[S->cur], S->vel[S->cur],
                     S->dead[S->cur], S->n, firstMember, bpm, G, F.cells, F.totals);
  PB_TRY(hipGetLastError());
  PB_TRY(F.clock.stop(S->stream));
  F.maps++;
  // the device cell has the size of the caller's: it lands in place and is rewritten there
  PB_TRY(hipMemcpyAsync(out, F.cells, sizeof(pbFieldCell) * (size_t)members * G.cells, hipMemcpyDeviceToHost, S->stream));
  uint32_t counters[4 * N_WORDS];
  std::vector<uint32_t> many;
  uint32_t *tot = counters;
  if (totals) {
    if (members > 4u) many.resize((size_t)members * N_WORDS), tot = many.data();
    PB_TRY(hipMemcpyAsync(tot, F.totals, sizeof(uint32_t) * members * N_WORDS, hipMemcpyDeviceToHost, S->stream));
  }
  PB_TRY(hipStreamSynchronize(S->stream));
  for (size_t k = 0; k < (size_t)members * G.cells; k++) {
    unsigned long long w[F_WORDS];
    memcpy(w, out + k, sizeof w);
    pbFieldCell &c = out[k];
    c.count = (unsigned)w[F_COUNT], c.dead = (unsigned)(w[F_COUNT] >> 32);
    c.sum_qr = (long long)w[F_QR], c.sum_wx = (long long)w[F_WX], c.sum_wy = (long long)w[F_WY];
    c.rr = pbFixedNormalised(pbFixedCompose(w[F_RR_LO], w[F_RR_HI]));
    c.vv = pbFixedNormalised(pbFixedCompose(w[F_VV_LO], w[F_VV_HI]));
  }
  if (totals)
    for (uint32_t k = 0; k < members; k++) {
      const uint32_t *t = tot + (size_t)k * N_WORDS;
      totals[k].measured = t[N_MEASURED], totals[k].inside = t[N_INSIDE];
      totals[k].outside = t[N_OUTSIDE], totals[k].unmeasured = t[N_UNMEASURED];
    }
  return PB_OK;
}

}  // namespace

extern "C" {

int pbSimFieldMap(pbSim *S, const pbFieldView *view, pbFieldCell *cells, pbFieldTotals *totals) {
  return fieldMap("pbSimFieldMap", S, 0u, false, view, cells, totals);
}

int pbSimFieldMapOf(pbSim *S, unsigned member, const pbFieldView *view, pbFieldCell *cells, pbFieldTotals *totals) {
  return fieldMap("pbSimFieldMapOf", S, member, true, view, cells, totals);
}

int pbSimGetFieldTimes(pbSim *S, unsigned long long *maps, float *last_device_ms) {
  if (!S) return pbFail("pbSimGetFieldTimes", ": null handle");
  return pbSpanGet(S, S->field.clock, S->field.maps, maps, last_device_ms);
}

}  // extern "C"
