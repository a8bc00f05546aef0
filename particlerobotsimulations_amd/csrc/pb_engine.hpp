// pb_engine.hpp -- what the translation units of the pbSim engine share (not part of the public C-ABI):
// the batch object, the launch plan, and the launchers each kernel family exports.
//
//   pb_engine.hip    the object, the schedule (stepMany), re-sort / phase update / I/O kernels, the C-ABI
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
//   pb_timecorr.hip  time correlations: MSD, VACF and overlap per lag over a ring of snapshots (pbSimSetTimeCorrelation)
//   pb_selftest.hip  exhaustive / sampled on-device proofs of the fast exact math, shader-clock sampler
//   pb_sweep.hpp     the neighbour sweep (device code shared by k_force and k_resident)
#pragma once

#include <string>
#include <vector>

#include "particlebot_hip.h"
#include "pb_device.hpp"
#include "pb_internal.hpp"

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

#ifndef PB_TILE
#define PB_TILE 256
#endif
constexpr int TILE = PB_TILE;

static inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

struct PbClusterScratch;  // pb_cluster.hpp

struct pbSim {
  std::vector<PbDevParams> hP;  // one parameter block per simulation
  PbDevParams *dP = nullptr;
  SimParams host;  // schedule-relevant fields (shared by the batch): max_time, phase_update_interval, control
  uint32_t nsims = 1, n = 0, total = 0;
  int device = 0;  // the device the batch lives on; every entry point makes it the calling thread's current one
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;

  float4 *pr[2] = {nullptr, nullptr};
  float2 *vel[2] = {nullptr, nullptr};
  float *phase[2] = {nullptr, nullptr};
  int *dead[2] = {nullptr, nullptr};
  float *absA[2] = {nullptr, nullptr};
  float *absR[2] = {nullptr, nullptr};
  uint32_t *orig[2] = {nullptr, nullptr};  // LOCAL original index of each slot
  int cur = 0;                             // which copy of every array is live

  uint32_t *cellS = nullptr;  // nsims x (numCells+1), global slot indices
  uint32_t *keys[2] = {nullptr, nullptr}, *vals[2] = {nullptr, nullptr}, *hist = nullptr, *slotOf = nullptr;
  uint32_t *sortedKeys = nullptr;  // keys[0] or keys[1]: composite keys of the slots, as of the last sort
  std::vector<uint32_t> layoutOrig, layoutKeys;  // host staging of pbSimSetLayoutOf
  std::vector<char> layoutGiven;
  pbRngState *rngState = nullptr;  // total, ORIGINAL order; only with an XORWOW generator (rng != 0)
  uint32_t *dMin = nullptr;  // nsims
  float *dMinD = nullptr;    // nsims
  uint32_t *hMin = nullptr;  // pinned, nsims
  float *hMinD = nullptr;    // pinned, nsims
  char *stage = nullptr;     // 36 n bytes: pos 8n | vel 8n | rad 4n | phase 4n | dead 4n | absA 4n | absR 4n
  float2 *comPos = nullptr;  // total
  double2 *comPartial = nullptr, *comOut = nullptr;
  double2 *hCom = nullptr;  // pinned, nsims

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
  unsigned long long *walkTrips = nullptr, walkTripsHost[2] = {0, 0};
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
  float4 *colors = nullptr;      // n, allocated by the first pbSimGetColorsOf
  float2 *trail = nullptr;       // nsims x trailSteps rings; nullptr: trail off
  float2 *trailTmp = nullptr;    // 2 x nsims x ceil(n / 64): the tree's temporaries
  float trailInt = 0.0f;
  int trailSteps = 0;
  std::vector<float> trailTimes;  // start time of the step that wrote each slot (NaN: never)
  unsigned trailRecords = 0;
  // frame rasteriser (pb_render.hip, pbSimRenderOf): allocated by the first render, re-allocated when the frame grows
  std::vector<float> centroidRadius;
  uint32_t *renderIds = nullptr;   // one key per pixel
  uint32_t *renderOut = nullptr;   // packed RGB8, padded to whole groups of four pixels
  uint32_t *renderRgb8 = nullptr;  // n: a member's bot colours in original order
  size_t renderPixels = 0;         // capacity of renderIds / renderOut
  hipEvent_t renderEv0 = nullptr, renderEv1 = nullptr;
  unsigned long long renders = 0;
  float lastRenderMs = 0.0f;
  // cluster analysis (pb_cluster.hip): scratch of its own, allocated by the first analysis, freed by pbSimDestroy
  PbClusterScratch *cluster = nullptr;
  // time series (pb_moments.hip): the ring when on (pbSimSetSeries), the one-shot rows of pbSimMoments, the record's events
  pbMomentsRow *series = nullptr;   // nsims x seriesCap, member-major: record r of member m at [m * seriesCap + r % seriesCap]
  pbMomentsRow *momRows = nullptr;  // nsims, allocated by the first pbSimMoments
  float seriesInt = 0.0f;           // 0: in front of every step
  unsigned seriesCap = 0;
  unsigned long long seriesRecords = 0;
  std::vector<float> seriesTimes;   // per slot: start time of the step the record was taken in front of
  std::vector<unsigned long long> seriesSteps;  // per slot: stats.steps at that moment
  hipEvent_t momEv0 = nullptr, momEv1 = nullptr;  // around the last pass' launches
  bool momTimed = false;
  // time correlations (pb_timecorr.hip): the ring of snapshots and the table when on (pbSimSetTimeCorrelation)
  float4 *tcRing = nullptr;               // tcLags x total, ORIGINAL order: record r at slot r % tcLags
  unsigned long long *tcTable = nullptr;  // nsims x tcLags cells of nine words, member-major
  float tcInt = 0.0f;                     // 0: in front of every step; -1: manual records only
  float tcRadius = 0.0f;
  unsigned tcLags = 0;
  unsigned long long tcA2 = 0, tcRecords = 0;  // rint(tcRadius * 2^20) squared; records taken so far
  std::vector<unsigned long long> tcSteps;     // per slot: stats.steps at that moment
  std::vector<unsigned long long> tcOrigins, tcSumSteps;  // per lag: record pairs added, and their step differences
  hipEvent_t tcEv0 = nullptr, tcEv1 = nullptr;  // around the last record's launches
  bool tcTimed = false;
  pbSimStats stats{};
};

static inline dim3 gridOf(const pbSim *S) { return dim3(cdiv(S->n, TILE), S->nsims); }

// HIP's current device is per host thread (a new thread starts on device 0): a caller that drives
// several batches from several threads must not have to remember that
static inline void useDevice(const pbSim *S) { (void)hipSetDevice(S->device); }

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
// frees the cluster analysis' scratch, if any (pbSimDestroy)                                             pb_cluster.hip
void pbClusterFree(pbSim *S);
// one record of every member into the ring's next slot, in front of the step that starts at t (stepMany)   pb_moments.hip
int pbSeriesRecord(pbSim *S, float t);
// frees the ring, the one-shot rows and the events (pbSimDestroy)
void pbMomentsFree(pbSim *S);
// one snapshot of every member, as it is now, into the ring's next slot and its lags into the table      pb_timecorr.hip
int pbTimeCorrRecord(pbSim *S);
// frees the ring, the table and the events (pbSimDestroy)
void pbTimeCorrFree(pbSim *S);
