// pb_engine.hpp -- what the translation units of the pbSim engine share (not part of the public C-ABI):
// the batch object, the launch plan, the launchers each kernel family exports, and the lag ring of the lagged analyses
// (PbLagBook, PbLagRing, pbLagPair, pbLag...: the one place that knows the ring's format).
//
//   pb_engine.hip    the object, the schedule (stepMany and its table of host events), re-sort / phase update / I/O
//                    kernels, the C-ABI
//   pb_force.hip     k_force: the exact per-step force kernel in all its forms + the forms table
//   pb_stream.hip    k_force_stream: the opt-in streamlined (tolerance) force kernel
//   pb_resident.hip  k_resident: the multi-step one-workgroup-per-simulation kernel
//   pb_display.hip   the reference's display kernels (colours, centroid trail)
//   pb_render.hip    the frame rasteriser behind pbSimRenderOf
//   pb_cluster.hip   cluster analysis: connected components of the contact graph (pbSimClusterStats)
//   pb_contacts.hip  the contact network of one member: links, gaps, pair forces, virial (pbSimContactsOf)
//   pb_structure.hip structure analysis: radial pair counts and the hexatic order (pbSimRadialCounts, pbSimStructureStats)
//   pb_dynamics.hip  rearrangement analysis: a marked reference, bond survival and displacements (pbSimMarkReference)
//   pb_moments.hip   time series: integer moment rows per member, now or recorded while stepping (pbSimSetSeries)
//   pb_timecorr.hip  time correlations: MSD, VACF and overlap per lag over a lag ring (pbSimSetTimeCorrelation)
//   pb_field.hip     field maps: count, dead and integer sums of radius and velocity per grid cell (pbSimFieldMap)
//   pb_sfactor.hip   structure factor: integer phasor sums per member and wavevector (pbSimStructureFactor)
//   pb_scatter.hip   self-intermediate scattering: integer phasor sums per member, lag and wavevector over a lag ring
//                    (pbSimSetScattering)
//   pb_vanhove.hip   self van Hove function: displacement histograms per lag over a lag ring (pbSimSetVanHove)
//   pb_vanhove_distinct.hip  distinct van Hove function: pair histograms per lag, a neighbour sweep around every bot's
//                    earlier position (pbSimSetVanHoveDistinct)
//   pb_coherent.hip  coherent intermediate scattering: a ring of density modes per member and wavevector, and 192-bit
//                    sums of their products per lag (pbSimSetCoherent); pb_coherent.hpp holds the arithmetic
//   pb_fourpoint.hip four-point dynamics: masked density modes per origin pair over a lag ring, and the exact sums of the
//                    overlap count, its square, the modes and their squared magnitudes per lag (pbSimSetFourPoint);
//                    pb_fourpoint.hpp holds the arithmetic
//   pb_bonds.hip     bond dynamics: a ring of neighbour lists, and per lag the surviving links and the cage-relative
//                    displacements of a record against the ring's (pbSimSetBondDynamics); pb_bonds.hpp holds the
//                    arithmetic
//   pb_strain.hip    local strain and D2min: the Falk-Langer fit of every bot's marked bonds onto its present ones, a
//                    gather over the rearrangement analysis' mark (pbSimStrainStats); pb_strain.hpp holds the fit
//   pb_selftest.hip  exhaustive / sampled on-device proofs of the fast exact math, shader-clock sampler
//   pb_sweep.hpp     the neighbour sweep (device code shared by k_force and k_resident)
//   pb_memory.hpp    the owners of device memory, pinned memory, events and streams the batch object is made of, and
//                    the span clock (two events around a span of launches)
//   pb_fixed.hpp     the fixed-point kit of the integer analyses: quantiser, split accumulators, wave and workgroup
//                    sums, the host's way back to a pbMoment128; the one statement of their bound
//   pb_phasor.hpp    the phasor kit of the reciprocal-space analyses: the turn of a bot, its table index, the table
#pragma once

#include <string>
#include <vector>

#include "particlebot_hip.h"
#include "pb_device.hpp"
#include "pb_internal.hpp"
#include "pb_memory.hpp"

// thread-local text behind pbGetLastErrorString (defined in pb_engine.hip)
std::string &pbLastError();

#define PB_TRY(expr)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) {                                                                           \
      pbLastError() = std::string(hipGetErrorName(e_)) + " at " + __FILE__ + ":" + std::to_string(__LINE__) + \
                      " in " #expr;                                                                   \
      return PB_ERR_HIP;                                                                              \
    }                                                                                                 \
  } while (0)

// an argument the entry point `fn` refuses: the text behind pbGetLastErrorString is fn + what
inline int pbFail(const char *fn, const std::string &what) {
  pbLastError() = std::string(fn) + what;
  return PB_ERR_ARG;
}

#ifndef PB_TILE
#define PB_TILE 256
#endif
constexpr int TILE = PB_TILE;

static inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

struct PbClusterScratch;  // pb_cluster.hpp

// The state of a layer that is switched on and off as a unit: "off" is the assignment of a fresh value.
// centroid trail (pb_display.hip, pbSimSetCentroidTrail)
struct PbTrail {
  PbDevBuf<float2> ring;  // nsims x steps rings; empty: trail off
  PbDevBuf<float2> tmp;   // 2 x nsims x ceil(n / 64): the tree's temporaries
  float interval = 0.0f;
  int steps = 0;
  std::vector<float> times;  // start time of the step that wrote each slot (NaN: never)
  unsigned records = 0;
};
// frame rasteriser (pb_render.hip, pbSimRenderOf): allocated by the first render, re-allocated when the frame grows
struct PbRender {
  PbDevBuf<uint32_t> ids;   // one key per pixel; its capacity is the frame both buffers hold
  PbDevBuf<uint32_t> out;   // packed RGB8, padded to whole groups of four pixels
  PbDevBuf<uint32_t> rgb8;  // n: a member's bot colours in original order
  PbSpanClock clock;
  unsigned long long renders = 0;
  float lastMs = 0.0f;
};
// time series (pb_moments.hip): the ring when on (pbSimSetSeries)
struct PbSeries {
  PbDevBuf<pbMomentsRow> ring;  // nsims x cap, member-major: record r of member m at [m * cap + r % cap]
  float interval = 0.0f;        // 0: in front of every step
  unsigned cap = 0;
  unsigned long long records = 0;
  std::vector<float> times;               // per slot: start time of the step the record was taken in front of
  std::vector<unsigned long long> steps;  // per slot: stats.steps at that moment
};
// ---- the lag ring: what the lagged analyses (pb_timecorr.hip, pb_scatter.hip, pb_vanhove.hip,
// pb_vanhove_distinct.hip, pb_coherent.hip, pb_fourpoint.hip, pb_bonds.hip) share ----------------------------------------
// A ring of `lags` snapshots of the whole batch in ORIGINAL order, lags x total entries of Snap.  Record r goes into
// slot r % lags and is paired with the records r - l for l = 0 ... min(r, lags - 1); all pairs of a record are added
// into `table` by one launch over pbLagGrid() workgroups of PB_LAG_LANES lanes, which pbLagPair() takes apart again.
// (The coherent scattering keeps modes, not bots: lags x nsims x nvec entries, which a kernel of its own pairs.)
// Everything that knows this format is in this file: the book and the ring value here, pbLagPair (device) and the
// pbLag... host functions behind pbSim.  An analysis adds its snapshot kernel, its accumulate body and its row writer.
constexpr int PB_LAG_LANES = 256;
constexpr unsigned PB_LAG_MAX_LAGS = 64u, PB_LAG_BLOCKS = 256u;  // (the public header states both per analysis)
static_assert(PB_TCORR_MAX_LAGS == PB_LAG_MAX_LAGS && PB_SCATTER_MAX_LAGS == PB_LAG_MAX_LAGS &&
                  PB_VANHOVE_MAX_LAGS == PB_LAG_MAX_LAGS && PB_COHERENT_MAX_LAGS == PB_LAG_MAX_LAGS &&
                  PB_FOURPOINT_MAX_LAGS == PB_LAG_MAX_LAGS && PB_BOND_MAX_LAGS == PB_LAG_MAX_LAGS,
              "one bound on the lags");  // (the distinct part uses the self part's)
static_assert(PB_TCORR_BLOCKS == PB_LAG_BLOCKS && PB_SCATTER_BLOCKS == PB_LAG_BLOCKS &&
                  PB_VANHOVE_BLOCKS == PB_LAG_BLOCKS && PB_FOURPOINT_BLOCKS == PB_LAG_BLOCKS &&
                  PB_BOND_BLOCKS == PB_LAG_BLOCKS,
              "one bound on the blocks per lag");

// the host's counters of a ring
struct PbLagBook {
  unsigned lags = 0;
  unsigned long long records = 0;                     // records taken so far
  std::vector<unsigned long long> steps;              // per slot: stats.steps at that moment
  std::vector<unsigned long long> origins, sumSteps;  // per lag: record pairs added, and their step differences
  void start(unsigned n) {
    lags = n, records = 0;
    steps.assign(n, 0ull), origins.assign(n, 0ull), sumSteps.assign(n, 0ull);
  }
  uint32_t slot() const { return (uint32_t)(records % lags); }  // where the next record goes
  uint32_t paired() const { return (uint32_t)(records < lags - 1u ? records : lags - 1u) + 1u; }  // the lags it is paired with
  void recorded(unsigned long long stepsNow) {  // the next record was taken at stats.steps == stepsNow
    const uint32_t s = slot(), n = paired();
    steps[s] = stepsNow;
    for (uint32_t l = 0; l < n; l++) origins[l]++, sumSteps[l] += stepsNow - steps[(s + lags - l) % lags];
    records++;
  }
  template <typename Row>  // the book's three columns of a lag's row
  void columns(unsigned lag, Row &r) const { r.lag = lag, r.origins = origins[lag], r.sum_steps = sumSteps[lag]; }
};
// the ring when on (`ring` is set), with the analysis' table behind it
template <typename Snap>
struct PbLagRing {
  PbDevBuf<Snap> ring;                 // lags x total, ORIGINAL order: record r at slot r % lags
  PbDevBuf<unsigned long long> table;  // the analysis' 64-bit words, zeroed when the ring is made
  float interval = 0.0f;               // 0: in front of every step; -1: manual records only
  PbLagBook book;                      // lags (0: off), records, steps per slot, origins and step sums per lag
  PbSpanClock clock;                   // around the last record's launches
  // an entry point that needs the analysis on refuses when the `what` ("correlation", "scattering", ...) is off
  int checkOn(const char *fn, const char *what) const {
    return ring ? PB_OK : pbFail(fn, std::string(": the ") + what + " is off");
  }
};
// workgroups of a record's accumulate launch: blocksPerLag blocks of bots per member and lag the record is paired with
inline uint32_t pbLagGrid(uint32_t nsims, uint32_t nLags, uint32_t blocksPerLag) { return nsims * nLags * blocksPerLag; }
// ... and what workgroup blockIdx.x of that grid works on: block `block` of the bots of `member`, as they are in the
// record just taken (`now`) and were `lag` records before it (`then`); lag < nLags <= lags
template <typename Snap>
struct PbLagPair {
  uint32_t member, lag, block;
  const Snap *now, *then;
};
template <typename Snap>
__device__ inline PbLagPair<Snap> pbLagPair(const Snap *ring, uint32_t n, uint32_t total, uint32_t lags,
                                            uint32_t slotNow, uint32_t nLags, uint32_t blocksPerLag) {
  const uint32_t perMember = nLags * blocksPerLag;
  const uint32_t member = blockIdx.x / perMember, rest = blockIdx.x - member * perMember;
  const uint32_t lag = rest / blocksPerLag, b = rest - lag * blocksPerLag;
  const uint32_t slotThen = slotNow >= lag ? slotNow - lag : slotNow + lags - lag;
  return {member, lag, b, ring + (size_t)slotNow * total + (size_t)member * n,
          ring + (size_t)slotThen * total + (size_t)member * n};
}

// time correlations (pb_timecorr.hip): float4 (x, y, vx, vy) snapshots and nsims x lags cells of nine words, member-major
// (pbSimSetTimeCorrelation)
struct PbTimeCorr {
  PbLagRing<float4> lag;
  float radius = 0.0f;
  unsigned long long a2 = 0;  // rint(radius * 2^20) squared
};

// field maps (pb_field.hip): the scratch of the largest map asked for so far, made by the first call (pbSimFieldMap)
struct PbField {
  PbDevBuf<unsigned long long> cells;  // eight words per cell of the map a call computes
  PbDevBuf<uint32_t> totals;           // four words per member
  PbSpanClock clock;                   // around the last map's launches
  unsigned long long maps = 0;
};

// structure factor (pb_sfactor.hip): the phasor table, the wavevectors and the sums of the largest call so far, made
// by the first call (pbSimStructureFactor)
struct PbSfactor {
  PbDevBuf<int2> table;                // the 4096 (cos, sin) entries of pb_phasor.hpp
  PbDevBuf<int2> vectors;              // PB_SK_MAX_VECTORS (nx, ny) pairs
  PbDevBuf<unsigned long long> cells;  // 2 / 4 / 8 words per member and wavevector of the call in flight
  PbDevBuf<uint32_t> measured;         // one word per member
  std::vector<unsigned long long> host;  // the read-back before it is written as rows
  PbSpanClock clock;                   // around the last analysis' launches
  unsigned long long analyses = 0;
};

// self-intermediate scattering (pb_scatter.hip): int2 snapshots of the quantised positions ((INT32_MIN, 0): unmeasured)
// and nsims x lags x nvec cells of (re, im), then nsims x lags sample counters (pbSimSetScattering)
struct PbScattering {
  PbLagRing<int2> lag;
  PbDevBuf<int2> phasors;  // the 4096 (cos, sin) entries of pb_phasor.hpp
  PbDevBuf<int2> vectors;  // nvec (nx, ny) pairs
  std::vector<int> list;   // the host's copy of the list, as passed
  unsigned nvec = 0;
  int boxLog2 = 0;
};

// self van Hove function (pb_vanhove.hip): float2 (x, y) snapshots and nsims x lags cells of 10 + 5 bins words, member-
// major: ten moments, then the radial, x and y histograms (pb_vanhove.hpp; pbSimSetVanHove)
struct PbVanHove {
  PbLagRing<float2> lag;
  float width = 0.0f;
  uint32_t qw = 0, bins = 0;              // rint(width * 2^20); counters per radial histogram
  PbDevBuf<unsigned long long> edges;  // bins + 1: E_k = min((k qw)^2, 2^63)
};

// coherent intermediate scattering (pb_coherent.hip): a ring of lags x nsims x nvec modes (C, S) with lags x nsims
// measured counts beside it, and nsims x lags x nvec cells of eight words (pb_coherent.hpp; pbSimSetCoherent)
struct PbCoherent {
  PbLagRing<ulonglong2> lag;    // the modes; the book, the interval, the clock and the table are the lag ring's
  PbDevBuf<uint32_t> measured;  // lags x nsims: the measured bots of each mode's record
  PbDevBuf<int2> phasors;       // the 4096 (cos, sin) entries of pb_phasor.hpp
  PbDevBuf<int2> vectors;       // nvec (nx, ny) pairs
  std::vector<int> list;        // the host's copy of the list, as passed
  unsigned nvec = 0;
  int boxLog2 = 0;
};

// four-point dynamics (pb_fourpoint.hip): the scattering's int2 snapshots, nsims x lags x nvec cells of eight words (re,
// im, power), then nsims x lags cells of four (samples, overlap, overlap2), and the per-record scratch of one origin's
// modes and counts (pb_fourpoint.hpp; pbSimSetFourPoint)
struct PbFourPoint {
  PbLagRing<int2> lag;
  PbDevBuf<unsigned long long> scratch;  // nsims x lags x nvec modes (A, B), then nsims x lags counts (m, Q)
  PbDevBuf<int2> phasors;                // the 4096 (cos, sin) entries of pb_phasor.hpp
  PbDevBuf<int2> vectors;                // nvec (nx, ny) pairs
  std::vector<int> list;                 // the host's copy of the list, as passed
  unsigned nvec = 0;
  int boxLog2 = 0;
  float radius = 0.0f;
  long long qa = 0;           // rint(radius * 2^20) ...
  unsigned long long a2 = 0;  // ... squared
};

// bond dynamics (pb_bonds.hip): int4 heads (qx, qy, degree, 0), (INT32_MIN, 0, 0, 0) for an absent bot, in the ring; the
// lists of eight neighbour indices beside it, two uint4 per bot and slot in the ring's order; and nsims x lags cells of
// PB_BOND_WORDS words (pb_bonds.hpp; pbSimSetBondDynamics)
struct PbBondDynamics {
  PbLagRing<int4> lag;
  PbDevBuf<uint4> lists;  // lags x total x 2
  float gap = 0.0f, maxRadius = 0.0f, radius = 0.0f;
  long long qa = 0;  // rint(radius * 2^20)
};

// distinct van Hove function (pb_vanhove_distinct.hip): float2 (x, y) snapshots, NaN for an absent bot, and nsims x lags
// cells of 2 + bins words, member-major: centres, partners, then the radial histogram of ordered pairs (pb_vanhove.hpp;
// pbSimSetVanHoveDistinct)
struct PbVanHoveDistinct {
  PbLagRing<float2> lag;
  float width = 0.0f;
  uint32_t qw = 0, bins = 0;           // rint(width * 2^20) with qw bins < 2^31; counters per histogram
  PbDevBuf<unsigned long long> edges;  // bins + 1: E_k = (k qw)^2
};

// Members release in reverse declaration order behind ~pbSim's body: the stream and the events are declared first
// and go last.
struct pbSim {
  ~pbSim();  // selects the device, drains the stream, frees the cluster analysis' scratch       pb_engine.hip
  PbStream stream;
  PbEvent ev0, ev1;
  int device = 0;  // the device the batch lives on; every entry point makes it the calling thread's current one
  std::vector<PbDevParams> hP;  // one parameter block per simulation
  PbDevBuf<PbDevParams> dP;
  SimParams host;  // schedule-relevant fields (shared by the batch): max_time, phase_update_interval, control
  uint32_t nsims = 1, n = 0, total = 0;

  PbDevBuf<float4> pr[2];
  PbDevBuf<float2> vel[2];
  PbDevBuf<float> phase[2];
  PbDevBuf<int> dead[2];
  PbDevBuf<float> absA[2];
  PbDevBuf<float> absR[2];
  PbDevBuf<uint32_t> orig[2];  // LOCAL original index of each slot
  int cur = 0;                 // which copy of every array is live

  PbDevBuf<uint32_t> cellS;  // nsims x (numCells+1), global slot indices
  PbDevBuf<uint32_t> keys[2], vals[2], hist, slotOf;
  uint32_t *sortedKeys = nullptr;  // keys[0] or keys[1] (not owned): composite keys of the slots, as of the last sort
  std::vector<uint32_t> layoutOrig, layoutKeys;  // host staging of pbSimSetLayoutOf
  std::vector<char> layoutGiven;
  PbDevBuf<pbRngState> rngState;  // total, ORIGINAL order; only with an XORWOW generator (rng != 0)
  PbDevBuf<uint32_t> dMin;  // 2 nsims: minima | last-NaN indices
  PbDevBuf<float> dMinD;    // nsims
  PbPinned<uint32_t> hMin;  // 2 nsims
  PbPinned<float> hMinD;    // nsims
  PbDevBuf<char> stage;     // 36 n bytes: pos 8n | vel 8n | rad 4n | phase 4n | dead 4n | absA 4n | absR 4n
  PbDevBuf<float2> comPos;  // total
  PbDevBuf<double2> comPartial, comOut;
  PbPinned<double2> hCom;  // nsims

  float time = 0.0f;
  uint32_t phaseDraws = 0;
  bool haveCells = false;
  bool resortEveryStep = false;
  bool payload = false, fastOk = false;
  bool xcdMembers = true;   // batches of >= 8 small members: all tiles of a member on one XCD (PB_XCD_MEMBERS=0 under PB_ALLOW_ENV_OVERRIDES: the plain (tile, member) grid, for A/B)
  bool xcdTilesAll = true;   // the XCD-contiguous tile order for the multi-lane forms too (PB_XCD_TILES_ALL=0 under PB_ALLOW_ENV_OVERRIDES: only for one bot per lane, as rounds 1-4)
  bool magOk = false;   // every member passes pbAttractionMagnitudeSafe (fast path of the both-sums throughput form)
  int variant = 2;  // force kernel: 0 reference-shaped branches, 1 branch-free, 2 (default) + fast exact math
  int resident = 0;     // 0 automatic, 1 never, 2 whenever the simulation fits one workgroup (n <= 1024)
  int lanesPerBot = 0;  // lanes per bot of the per-step force kernel: 0 automatic; 1 (throughput form), 2, 4, 8, 16
  // k_force_stream's neighbour walk (pb_stream.hip, WALK): -1 chosen at every re-sort from the batch's cell lists
  // (chooseStreamWalk), 0 row by row, 1 flattened (pbSimSetStreamWalk).  Bit-identical either way.
  int streamWalk = -1;
  bool streamWalkAuto = false;
  PbDevBuf<unsigned long long> walkTrips;  // 2, allocated by the first choice of the walk
  unsigned long long walkTripsHost[2] = {0, 0};
  uint32_t cuCount = 0;  // compute units of the device (pbTailTiles; 0 until first asked)
  int tailTiles = -1;  // split-lane tail tiles per XCD of the throughput form: -1 automatic (pbTailTiles), else that many
  bool wideOffsets = false;  // run the 64-bit-offset throughput sweep on a batch below 2^28 bots (pbSimSelectForceForm, tests)
  unsigned debugLdsBytes = 0;  // PB_DEBUG_LDS_BYTES under PB_ALLOW_ENV_OVERRIDES=1 (tools/occupancy_sweep.py --lds)
  int rng = 0;          // phase noise: 0 PB-RNG v1 (counter based), 1 cuRAND-compatible XORWOW (pb_xorwow.hpp)
  int minDistanceMode = 0;  // phase update: 0 device min of squares + host root, 1 the reference's host loop (pbSimSetMinDistanceMode)
  std::vector<float> hostPos;  // mode 1: one simulation's positions, original order
  int forceSums = 0;    // 0: Sum|F_attr| only when a member reads it (constrained_contraction), 1: always
  bool anyConstrained = false;  // some member has constrained_contraction != 0
  // display (pb_display.hip): per-member display_shadow, and the centroid trail when on (pbSimSetCentroidTrail)
  std::vector<uint32_t> displayShadow;
  std::vector<float> centroidInt;
  std::vector<int> centroidSteps;
  PbDevBuf<float4> colors;  // n, allocated by the first pbSimGetColorsOf
  PbTrail trail;
  std::vector<float> centroidRadius;
  PbRender render;
  // cluster analysis (pb_cluster.hip): scratch of its own, allocated by the first analysis, freed by ~pbSim
  PbClusterScratch *cluster = nullptr;
  PbSeries series;
  // the one-shot rows of pbSimMoments and the clock around the last moments pass, series record or not: made on first
  // use and kept when the series is switched
  PbDevBuf<pbMomentsRow> momRows;  // nsims
  PbSpanClock momClock;
  PbTimeCorr tc;
  PbField field;
  PbSfactor sk;
  PbScattering sc;
  PbVanHove vh;
  PbVanHoveDistinct vd;
  PbCoherent co;
  // k_coh_modes' lanes as (stripe, vector); false: one lane per vector, for A/B (PB_COHERENT_STRIPES=0 under
  // PB_ALLOW_ENV_OVERRIDES)
  bool coherentStripes = true;
  PbFourPoint fp;
  PbBondDynamics bd;
  pbSimStats stats{};
};

static inline dim3 gridOf(const pbSim *S) { return dim3(cdiv(S->n, TILE), S->nsims); }

// HIP's current device is per host thread (a new thread starts on device 0): a caller that drives
// several batches from several threads must not have to remember that
static inline void useDevice(const pbSim *S) { (void)hipSetDevice(S->device); }

// a launch of the analysis layer indexes the batch's bots with 32 bits and room to spare
inline int pbCheckBatch(const char *fn, const pbSim *S) {
  return S->total >= (1u << 28) ? pbFail(fn, ": the batch must hold fewer than 2^28 bots") : PB_OK;
}
// the body of pbSimGet{Series,TimeCorrelation,Field}Times behind the handle check: `count` spans so far, and the device
// time of the last one (0 before any; the call waits for its end)
inline int pbSpanGet(const pbSim *S, const PbSpanClock &K, unsigned long long count, unsigned long long *spans,
                     float *last_device_ms) {
  if (spans) *spans = count;
  if (last_device_ms) {
    if (K.timed()) useDevice(S);
    PB_TRY(K.ms(last_device_ms));
  }
  return PB_OK;
}
// The interval of a recorder that stepMany fires: 0 in front of every step, > 0 the schedule's fp32 gate, and, where
// `manual` allows it, -1 for records by hand only (pbRecordDue in pb_engine.hip reads it by the same rule).
inline int pbCheckInterval(const char *fn, float interval, bool manual) {
  if ((manual && interval == -1.0f) || (interval >= 0.0f && interval < __builtin_inff())) return PB_OK;
  return pbFail(fn, std::string(": interval must be finite and >= 0") + (manual ? ", or -1 for manual records only" : ""));
}

// ---- the host side of the lag ring (the format is stated at PbLagBook) ------------------------------------------------
// A setter's checks of interval and lags, which read no handle, ...
inline int pbLagCheckArgs(const char *fn, float interval, unsigned lags) {
  if (const int rc = pbCheckInterval(fn, interval, true)) return rc;
  return lags > PB_LAG_MAX_LAGS ? pbFail(fn, ": lags must be at most 64") : PB_OK;
}
// ... and, behind the analysis' own argument checks, those of the batch
template <typename Snap>
int pbLagCheckBatch(const char *fn, const pbSim *S, unsigned lags) {
  if (S->nsims > 65535u) return pbFail(fn, ": the batch must hold at most 65535 members");  // the member is a grid's y
  if (const int rc = pbCheckBatch(fn, S)) return rc;
  if ((unsigned long long)lags * S->total * sizeof(Snap) > (1ull << 33))
    return pbFail(fn, ": the ring (lags x bots x " + std::to_string(sizeof(Snap)) + " bytes) must not exceed 2^33 bytes");
  return PB_OK;
}
// the ring of perSlot entries per slot and the zeroed table of `words` words into R; on an error the caller drops R
template <typename Snap>
int pbLagAllocate(pbSim *S, PbLagRing<Snap> &R, unsigned lags, size_t words, size_t perSlot) {
  PB_TRY(R.ring.alloc((size_t)lags * perSlot));
  PB_TRY(R.table.alloc(words));
  PB_TRY(hipMemsetAsync(R.table, 0, sizeof(unsigned long long) * words, S->stream));
  return PB_OK;
}
// Switches the analysis `held` (S->tc, S->sc, S->vh, S->vd, S->co, S->fp, S->bd) off and, unless lags is 0, on again: a fresh value
// with a ring of `lags` snapshots (of perSlot entries each; 0: one per bot of the batch), a zeroed table of wordsPerLag
// words per member and lag, a book at record 0, and what fill(fresh) sets of the analysis' own.  When any of it fails,
// what was made goes and the analysis stays off.
template <typename A, typename Fill>
int pbLagSwitch(pbSim *S, A &held, float interval, unsigned lags, size_t wordsPerLag, Fill fill, size_t perSlot = 0) {
  useDevice(S);
  PB_TRY(hipStreamSynchronize(S->stream));  // a record of the old ring may still be in flight
  held = A();
  if (!lags) return PB_OK;
  A fresh;
  int rc = pbLagAllocate(S, fresh.lag, lags, (size_t)S->nsims * lags * wordsPerLag, perSlot ? perSlot : S->total);
  if (rc == PB_OK) rc = fill(fresh);
  if (rc != PB_OK) {          // (a ring that took the last free memory, say)
    (void)hipGetLastError();  // (the failure is reported here, not by the next launch check of the schedule)
    return rc;
  }
  fresh.lag.interval = interval, fresh.lag.book.start(lags);
  held = std::move(fresh);
  return PB_OK;
}
// One record of the state as it is: snapshot(grid, slot) stores every bot into the ring's next slot, then
// accumulate(grid, slotNow, nLags, blocksPerLag) adds its pairs with the lags it is paired with.  Both launch on the
// batch's stream; nothing waits.
template <typename Snap, typename Shot, typename Acc>
int pbLagRecord(pbSim *S, PbLagRing<Snap> &R, Shot snapshot, Acc accumulate) {
  const uint32_t slot = R.book.slot(), nLags = R.book.paired();
  const uint32_t perMember = cdiv(S->n, PB_LAG_LANES);
  const uint32_t bpl = perMember < PB_LAG_BLOCKS ? perMember : PB_LAG_BLOCKS;
  PB_TRY(R.clock.start(S->stream));
  snapshot(dim3(perMember, S->nsims), R.ring + (size_t)slot * S->total);
  accumulate(dim3(pbLagGrid(S->nsims, nLags, bpl)), slot, nLags, bpl);
  PB_TRY(hipGetLastError());
  PB_TRY(R.clock.stop(S->stream));
  R.book.recorded(S->stats.steps);
  return PB_OK;
}
// the body of pbSim...Record: one record by hand, of the state as it is
template <typename A>
int pbLagManualRecord(const char *fn, pbSim *S, A pbSim::*which, const char *what, int (*record)(pbSim *)) {
  if (!S) return pbFail(fn, ": null handle");
  if (const int rc = (S->*which).lag.checkOn(fn, what)) return rc;
  useDevice(S);
  return record(S);
}
// The table as it stands, read back into acc for the analysis' row writer.  Refused when the analysis is off or any of
// the nsims x lags sample counters, acc[samplesAt + g * samplesStride], is at its cap.
template <typename Snap>
int pbLagFetch(const char *fn, pbSim *S, const PbLagRing<Snap> &R, const char *what,
               std::vector<unsigned long long> &acc, size_t samplesAt, size_t samplesStride) {
  if (const int rc = R.checkOn(fn, what)) return rc;
  useDevice(S);
  acc.resize(R.table.capacity());
  PB_TRY(hipMemcpyAsync(acc.data(), R.table, sizeof(unsigned long long) * acc.size(), hipMemcpyDeviceToHost, S->stream));
  PB_TRY(hipStreamSynchronize(S->stream));
  for (size_t g = 0; g < (size_t)S->nsims * R.book.lags; g++)
    if (acc[samplesAt + g * samplesStride] >= (1ull << 31))  // the counts are exact whatever the state: the other sums may not be
      return pbFail(fn, std::string(": a lag holds 2^31 samples or more: restart the ") + what);
  return PB_OK;
}
// the body of pbSimGet...Times
template <typename A>
int pbLagTimes(const char *fn, pbSim *S, A pbSim::*which, unsigned long long *records, float *last_device_ms) {
  if (!S) return pbFail(fn, ": null handle");
  return pbSpanGet(S, (S->*which).lag.clock, (S->*which).lag.book.records, records, last_device_ms);
}

// absForce_a has a reader (impl.cuh:167-169) or the caller asked for it (pbSimSetForceSums)
static inline bool pbStreamWalk(const pbSim *S) { return S->streamWalk >= 0 ? S->streamWalk == 1 : S->streamWalkAuto; }
static inline bool attractionSumsKept(const pbSim *S) { return S->forceSums != 0 || S->anyConstrained; }

// What a per-step force launch of this batch will be: the streamlined kernel or an exact one
// (kind 0 reference-shaped branches, 1 branch-free, 2 branch-free + fast exact math), and the lanes
// per bot of the exact branch-free kernels.  One place decides (pbForcePlan, pb_force.hip), so
// pbSimGetConfig reports what runs.
struct PbForcePlan {
  bool stream;
  int kind;
  int form;   // lanes per bot (1 = throughput form)
  bool asum;  // the launch maintains absForce_a (false: dead-sum form)
  bool big;   // 64-bit byte offsets in the throughput sweep
};
PbForcePlan pbForcePlan(const pbSim *S);
#ifndef PB_TAIL_LANES
#define PB_TAIL_LANES 2  // lanes per bot of the throughput form's split-lane tail workgroups (k_force)
#endif
// Workgroup tileX of a throughput-form grid in XCD order with perXcd tiles per XCD, the last `tail` of them split
// (8 * (perXcd + tail * (PB_TAIL_LANES - 1)) workgroups; round-robin dispatch puts workgroups b, b+8, ... on one
// XCD): its first bot, and whether it is a tail workgroup (TILE / PB_TAIL_LANES bots, PB_TAIL_LANES lanes each;
// else TILE bots, one lane each).  Together the workgroups cover bots [0, 8 * perXcd * TILE) once each.
__host__ __device__ inline bool pbXcdTile(uint32_t tileX, uint32_t perXcd, uint32_t tail, uint32_t &first) {
  const uint32_t x = tileX & 7u, k = tileX >> 3, mainK = perXcd - tail;
  if (k < mainK) {
    first = (x * perXcd + k) * TILE;
    return false;
  }
  first = (x * perXcd + mainK) * TILE + (k - mainK) * (TILE / PB_TAIL_LANES);
  return true;
}
// split-lane tail tiles per XCD of the next per-step force launch (0: none; pbSimSetTailTiles)             pb_force.hip
uint32_t pbForceTailTiles(pbSim *S);

// step n's forces + kick into the other copy of posrad/vel; fuse: also step n+1's radius + integration
void pbLaunchForce(pbSim *S, bool fuse, int c, int o, float dt, float tNext, int doRadiusNext);          // pb_force.hip
void pbLaunchForceStream(pbSim *S, bool fuse, int c, int o, float dt, float tNext, int doRadiusNext);    // pb_stream.hip
// profiler-style names of the kernels above ("k_force<...>(argument types)"): pbSimForceKernelName
std::string pbKernelArgs(const char *mangledPointerType);                                                // pb_force.hip
std::string pbForceStreamName(const pbSim *S);                                                           // pb_stream.hip
// m whole timesteps from time t0 in one launch (simulations of <= 1024 bots)
bool pbResidentWanted(const pbSim *S);                                                                    // pb_resident.hip
void pbLaunchResident(pbSim *S, float dt, float t0, int m, int lightWave);
// frees the cluster analysis' scratch, if any (~pbSim: PbClusterScratch is incomplete here)              pb_cluster.hip
void pbClusterFree(pbSim *S);
// What stepMany's table of host events fires from other files: one record of every member, of the state as it is, ...
int pbSeriesRecord(pbSim *S, float t);  // ... in front of the step that starts at t                        pb_moments.hip
int pbTimeCorrRecord(pbSim *S);         // ... a snapshot and its lags (pbLagRecord)                        pb_timecorr.hip
int pbScatteringRecord(pbSim *S);       // ... a quantised snapshot and its lags (pbLagRecord)              pb_scatter.hip
int pbVanHoveRecord(pbSim *S);          // ... a position snapshot and its lags (pbLagRecord)               pb_vanhove.hip
int pbVanHoveDistinctRecord(pbSim *S);  // ... a filing, a snapshot and its lags (pbLagRecord)     pb_vanhove_distinct.hip
int pbCoherentRecord(pbSim *S);         // ... the density modes and their products with the ring's         pb_coherent.hip
int pbFourPointRecord(pbSim *S);        // ... a quantised snapshot, the masked modes of its lags, their fold  pb_fourpoint.hip
int pbBondDynamicsRecord(pbSim *S);     // ... a filing, the heads and lists, and their pairs with the ring's    pb_bonds.hip
