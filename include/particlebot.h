/*
 * particlebot.h -- class Particlebot, headless, on MI355X.
 *
 * Keeps the public surface of the reference's class (particlebot.h:14-67): constructor from
 * SimParams, update, reset, getArray/setArray, the buffer getters, dumpParticlebot, loadFromFile,
 * getWorldOrigin/getCellSize.  What changed underneath:
 *   - no OpenGL: the VBO getters return 0 / nullptr unless the legacy engine is selected, in which
 *     case they return the headless buffer ids / device pointers;
 *   - the per-step work runs in the resident fused engine (pbSim*, include/particlebot_hip.h) by
 *     default; PB_ENGINE=legacy (or Engine::Legacy) replays the reference's own call sequence
 *     through the `extern "C"` device boundary instead, kernel by kernel;
 *   - absForce_a / absForce_r start at zero (the reference reads them uninitialised at step 0);
 *   - phase noise uses this build's counter RNG, not cuRAND (parity unpinned).
 */
#ifndef PARTICLEBOT_H
#define PARTICLEBOT_H

#include <cmath>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "particlebot_hip.h"
#include "particlebot_kernel.h"

/* glibc's rand()/srand() (the TYPE_3 additive-feedback generator of random_r) as an object.  The
 * reference draws the placement and the dead-bot set from the process-global libc stream seeded
 * by srand(params.seed) in main (main.cpp:929).  A private stream with the same arithmetic gives
 * the same numbers, is not disturbed by other users of rand() in the process (the HIP runtime
 * draws from it while initialising) and lets many simulations live in one process. */
class PbLibcRand {
 public:
  explicit PbLibcRand(unsigned seed = 1) { reseed(seed); }
  void reseed(unsigned seed);
  int next(); /* == rand(): 31 bits */
  static constexpr int kMax = 2147483647; /* RAND_MAX */
  /* full generator state (for checkpoints): 34 table words + the two cursors */
  void getState(int out[36]) const;
  void setState(const int in[36]);

 private:
  int r[34];
  int f, b; /* front / rear indices into r[3..33] */
};

/* The reference's dump-row gate (particlebot.cpp:309): true when a CSV row is due at time t.  THE one definition:
 * class Particlebot, the ensemble's row schedule and its row count all ask it.  The fp32 expression and its operand
 * order decide which step writes a row; do not rearrange it. */
static inline bool pbDumpRowDue(float t, float dump_interval) {
  return !(t - dump_interval * floorf(t / dump_interval) > 0.01f);
}

/* One row of the reference's CSV (particlebot.cpp:303-367: "Seed", the header and the time-0 row come together) from
 * the fp32 coordinate sums of `count` bots: the text dumpParticlebot writes with testing = 0, which the ensemble's
 * member CSVs repeat byte for byte.  testingColumns(header), when given, writes the testing = 1 columns (their names
 * with header = true, else their values) where the reference has them.  Shared inside libparticlebot_host.so, not
 * exported. */
__attribute__((visibility("hidden"))) void pbWriteCsvRow(FILE *fp, float time, unsigned seed, float sumX, float sumY,
                                                         unsigned count, float light_x, float light_y,
                                                         const std::function<void(bool header)> &testingColumns = nullptr);

class Particlebot {
 public:
  /* HostOnly: no device objects at all -- placement, dead-bot draw and host mirrors only; used by
   * the ensemble driver, which keeps every member's device state in one batched pbSim */
  enum class Engine { Fused, Legacy, HostOnly };

  /* particlebot.h:17 -- engine taken from $PB_ENGINE ("legacy" or "fused", default fused);
   * wall half-extent 64 as in the reference */
  Particlebot(SimParams params);
  Particlebot(SimParams params, Engine engine, float wallHalf);
  ~Particlebot();

  /* particlebot.h:21.  One timestep (particlebot.cpp:170-300).  Like the reference, exits the
   * process with status 0 once time > max_time -- unless setExitOnMaxTime(false), after which it
   * just returns and finished() reports it. */
  void update(float deltaTime, float sort_interval);
  /* Extension: up to nsteps timesteps in one call (lets the fused engine keep one kernel per
   * step); never exits the process; returns the number of steps run. */
  int advance(float deltaTime, float sort_interval, int nsteps);
  void reset(); /* particlebot.h:22 */

  /* particlebot.h:24-25.  getArray returns the host mirror after copying n*width floats (the
   * reference copies nCells*4 floats from 1- and 2-float buffers, particlebot.cpp:830: not
   * replicated).  PHASE and DEAD are supported too. */
  float *getArray(ParticlebotArray array);
  void setArray(ParticlebotArray array, const float *data, int start, int count);

  unsigned int getCurrentReadBuffer() const { return posVbo; }
  unsigned int getColorBuffer() const { return colorVBO; }
  unsigned int getRadBuffer() const { return radVbo; }
  void *getCudaPosVBO() const { return (void *)cudaPosVBO; }
  void *getCudaColorVBO() const { return (void *)cudaColorVBO; }
  void *getCudaRadVBO() const { return (void *)cudaRadVBO; }

  /* particlebot.h:54-59 */
  void dumpParticlebot(uint start, uint count, FILE *fp, float dump_interval, uint testing, float light_x,
                       float light_y);
  void loadFromFile(uint start, uint count, FILE *fp, float dump_interval);

  float2 getWorldOrigin() { return params.worldOrigin; }
  float2 getCellSize() { return params.cellSize; }

  /* ---- extensions ---- */
  void setExitOnMaxTime(bool on) { exitOnMaxTime = on; }
  bool finished() const { return time > params.max_time; }
  float getTime() const { return time; }
  void setTime(float t);
  /* true if a dump row is due at the current time (the test at particlebot.cpp:309) */
  bool dumpDue(float dump_interval) const;
  /* steps until the next host-side event (dump row, dead-bot draw), for batching; >= 1 */
  int stepsUntilHostEvent(float deltaTime, float dump_interval, int maxSteps) const;
  Engine engine() const { return engineKind; }
  const SimParams &getParams() const { return params; }
  int *getDeadArray();
  /* quiet the reference's per-bot "Placing %d th disc" chatter (particlebot.cpp:645) */
  static void setVerbosePlacement(bool on);
  /* lattice pitch used by CONFIG_HEX placement; <= 0 selects the reference's 2*min_radius */
  void setHexSpacing(float pitch) { hexSpacing = pitch; }
  /* Extension: place the bots on a centred square lattice (pitch as setHexSpacing) instead of what
   * params.config says.  Unlike any hexagonal packing, four contacts per bot are numerically stable
   * under the reference's parameters: the O(N) placement for very large arenas. */
  void setSquareLattice(bool on) { squareLattice = on; }
  /* Extension (`pb_placement fastblob`): a random blob grown by the reference's rule (random anchor,
   * random angle, pivot to contact; particlebot.cpp:612-748) with the anchors drawn from the discs
   * that still have room: O(N), for blobs the reference's O(N^1.5) loop cannot reach (10^6 bots in
   * seconds).  Same kind of blob, different random stream: NOT the reference's placement. */
  void setFastBlob(bool on) { fastBlob = on; }
  /* Extension: phase-noise generator, PB_RNG_* of particlebot_hip.h (default PB_RNG_COUNTER; the
   * `pb_rng` key of a .cfg: "pbrng", "curand" or "rocrand").  Re-initialises the per-bot generator
   * states, as curand_setup does at construction (particlebot.cpp:165); call it before the first step. */
  void setRng(int kind);
  int rngKind() const { return rngKindV; }
  /* Extension (`pb_force_variant` key): the force kernel of the fused engine -- 0/1/2 the exact forms (2 the default),
   * 3 the opt-in tolerance kernel (not bit-identical; as close to the reference as an FMA-contracted build of its own
   * arithmetic).  No effect on the Legacy engine. */
  void setForceVariant(int variant);
  pbSim *engineHandle() { return sim; }
  /* host mirrors in original bot order (valid after reset(); refreshed by getArray/dump) */
  const float *hostPositions() const { return hPos; }
  const float *hostVelocities() const { return hVel; }
  const float *hostRadii() const { return hRad; }
  const float *hostPhases() const { return hphase; }
  const int *hostDead() const { return hDead; }
  /* true when the step starting at the current time is the one that draws the dead bots
   * (particlebot.cpp:178) */
  bool deadDrawDue(float deltaTime) const {
    return params.nDead > 0 && time >= params.time_to_dead && time < params.time_to_dead + deltaTime;
  }
  /* draws the dead set into the host mirror (and the engine, if any); returns the mirror */
  const int *drawDeadBotsNow() {
    drawDeadBots();
    return hDead;
  }
  /* Exact checkpoint (extension; fused engine): time, phase-noise draw counter, the private
   * generator's state, every state array INCLUDING phase / dead / absForce_a / absForce_r, and the
   * stale slot layout (which the reference's CSV resume loses): a run resumed from it continues
   * bit-identically.  Both return false on I/O or format errors. */
  bool saveCheckpoint(FILE *fp);
  bool loadCheckpoint(FILE *fp);
  /* Headless stand-in for the reference's display()/video path (main.cpp:354-470, colours from
   * updateCol_k, particlebot_kernel_impl.cuh:401-443): writes a binary PPM (P6) of width x height
   * pixels showing the square |x - centerX|, |y - centerY| <= halfExtent seen from above, x
   * mirrored as the reference draws it.  Bots are discs of their current radius: dead bots black,
   * live ones R = 30, G = 20 + 180 ((max_r - r)/(max_r - min_r))^2, B = 30 + 180
   * sqrt((r - min_r)/(max_r - min_r)); obstacles grey, the light a yellow disc of lightRadius.
   * (The display_shadow tint is not drawn.)  Returns false on I/O errors. */
  bool writeFramePPM(const char *path, int width, int height, float centerX, float centerY, float halfExtent,
                     float lightRadius = 0.25f);
  /* The same view in the reference's display colours: bots in the device colours of updateCol_k (getColorArray,
   * display_shadow tint included), each channel lrintf(c * 255) clamped to 0..255; then the centroid trail in slot
   * order as red discs of centroid_radius at (x, y - 2000), slots still at x = -5000 skipped (trail only with
   * setDisplay(true)).  Returns false on I/O errors. */
  bool writeFramePPMReference(const char *path, int width, int height, float centerX, float centerY,
                              float halfExtent, float lightRadius = 0.25f);
  /* The same pictures rasterised on the device from the engine's resident state (pbSimRenderOf): only the
   * 3 * width * height bytes of the frame leave the device, no state copy.  renderFrame fills `rgb` (rows top to
   * bottom, R G B); writeFramePPMDevice writes the header and payload bytes writeFramePPM / writeFramePPMReference
   * write for the same state.  Fused engine only: Legacy and HostOnly instances return false with a message on
   * stderr.  Also false on a bad size or extent, and on I/O errors. */
  bool renderFrame(std::vector<unsigned char> &rgb, int width, int height, float centerX, float centerY,
                   float halfExtent, float lightRadius = 0.25f, bool referenceStyle = false);
  bool writeFramePPMDevice(const char *path, int width, int height, float centerX, float centerY, float halfExtent,
                           float lightRadius = 0.25f, bool referenceStyle = false);
  /* frames rendered on the device so far and the device time of the last one's launches in milliseconds
   * (pbSimGetRenderStats); false unless the engine is the fused one */
  bool renderStats(unsigned long long &frames, float &lastDeviceMs);
  /* Cluster analysis of the resident state on the device (pbSimClusterStats / pbSimClusterLabelsOf,
   * include/particlebot_hip.h has the definition of a link, a cluster and a label): the stats row, or every bot's label
   * and degree in ORIGINAL order.  Fused engine only: Legacy and HostOnly instances return false with a message on
   * stderr.  Also false on a negative or non-finite linkGap. */
  bool clusterStats(float linkGap, pbClusterStats &out);
  bool clusterLabels(float linkGap, std::vector<unsigned> &labels, std::vector<unsigned> &degree);
  /* The contact network of the resident state from the device (pbSimContactsOf / pbSimContactVirialOf,
   * include/particlebot_hip.h has the definition): a CSR adjacency in ORIGINAL order (nCells + 1 offsets, one
   * pbContactLink per directed entry: other, gap, force on the owning bot), or the per-bot virial (4 nCells doubles).
   * Fused engine only: Legacy and HostOnly instances return false with a message on stderr.  Also false on a negative
   * or non-finite linkGap. */
  bool contacts(float linkGap, std::vector<unsigned> &offsets, std::vector<pbContactLink> &links);
  bool contactVirial(float linkGap, std::vector<double> &virial);
  /* Structure analysis of the resident state on the device (pbSimRadialCounts / pbSimStructureStats / pbSimHexaticOf,
   * include/particlebot_hip.h has the definitions): the radial pair counts (`bins` entries, ordered pairs), the
   * member's hexatic row, or every bot's psi6 (2 nCells doubles) and neighbour count in ORIGINAL order.  Fused engine
   * only: Legacy and HostOnly instances return false with a message on stderr.  Also false on a bad rMax, bins or
   * linkGap. */
  bool radialCounts(float rMax, unsigned bins, std::vector<unsigned long long> &counts);
  bool structureStats(float linkGap, pbStructureStats &out);
  bool hexatic(float linkGap, std::vector<double> &psi6, std::vector<unsigned> &neighbours);
  /* Rearrangement analysis of the resident state on the device (pbSimMarkReference / pbSimRearrangementStats /
   * pbSimRearrangementOf, include/particlebot_hip.h has the definitions): markReference keeps the positions and the
   * link network at linkGap on the device, clearReference frees them; rearrangementStats gives the row that compares
   * the state as it is now with the mark (bonds marked, now and kept, displacement sums); rearrangement every bot's
   * displacement (2 nCells floats: dx, dy) and its marked, present and kept bond counts in ORIGINAL order.  Fused engine
   * only: Legacy and HostOnly instances return false with a message on stderr.  Also false on a bad linkGap, and for a
   * compare with no mark held.  The mark is not part of a checkpoint. */
  bool markReference(float linkGap);
  bool clearReference();
  bool rearrangementStats(pbRearrangementStats &out);
  bool rearrangement(std::vector<float> &disp, std::vector<unsigned> &marked, std::vector<unsigned> &now,
                     std::vector<unsigned> &kept);
  /* Local strain and D2min of the resident state against the mark, on the device (pbSimStrainStats / pbSimStrainOf,
   * include/particlebot_hip.h has the definitions): strainStats gives the member's row of integers (fitted and unfitted
   * bots, bots with D2min above d2Threshold, used and dropped bonds, the sums of the moments and of D2min); strain
   * every bot's nine integer moments (9 nCells), its local deformation gradient (4 nCells: Jxx Jxy Jyx Jyy) and its
   * D2min (nCells, units of 2^-40) in ORIGINAL order.  Fused engine only: Legacy and HostOnly instances return false
   * with a message on stderr.  Also false on a bad d2Threshold, and with no mark held. */
  bool strainStats(float d2Threshold, pbStrainStats &out);
  bool strain(std::vector<long long> &moments, std::vector<double> &gradient, std::vector<double> &d2min);
  /* Time series of the resident state on the device (pbSimMoments / pbSimSetSeries / pbSimGetSeriesOf,
   * include/particlebot_hip.h has the definitions): moments gives the row of integer moments of the state as it is now;
   * setSeries(interval, capacity) starts a device ring that takes such a row in front of every step whose start time
   * passes the schedule's gate at `interval` (0: every step) while update() runs, capacity 0 switches it off; seriesInfo
   * gives the interval, the capacity and the records taken so far; seriesRows the records from number `first` up to the
   * last one taken, in order.  Fused engine only: Legacy and HostOnly instances return false with a message on stderr.
   * Also false on a bad interval or capacity, and for a read outside the ring's window or with the series off.  The
   * series is not part of a checkpoint. */
  bool moments(pbMomentsRow &out);
  bool setSeries(float interval, unsigned capacity);
  bool seriesInfo(float &interval, unsigned &capacity, unsigned long long &records);
  bool seriesRows(unsigned long long first, std::vector<pbMomentsRow> &rows);
  /* Pair correlations of the resident state on the device (pbSimPairCorrelation, include/particlebot_hip.h has the
   * definition): `bins` rows of pairs binned by distance up to rMax with the sums of a_i . a_j, ax and ay, and the
   * totals row; kind is PB_CORR_VELOCITY, PB_CORR_DISPLACEMENT (since markReference) or PB_CORR_RADIUS.  Fused engine
   * only: Legacy and HostOnly instances return false with a message on stderr.  Also false on an unknown kind, a bad
   * rMax or bins, and for displacements with no mark held. */
  bool pairCorrelation(int kind, float rMax, unsigned bins, std::vector<pbCorrelationBin> &rows,
                       pbCorrelationTotals &totals);
  /* Time correlations of the resident state on the device (pbSimSetTimeCorrelation / pbSimGetTimeCorrelation,
   * include/particlebot_hip.h has the definitions): setTimeCorrelation(interval, lags, overlapRadius) starts a device
   * ring of `lags` snapshots, taken in front of every step whose start time passes the schedule's gate at `interval`
   * (0: every step, -1: only by timeCorrelationRecord) while update() runs, and a table that sums squared displacement,
   * velocity products and the overlap count per lag over all time origins; lags 0 switches it off.
   * timeCorrelationRecord takes one record now; timeCorrelationInfo gives interval, lags, overlap radius and the records
   * taken so far; timeCorrelationRows the `lags` rows, lag 0 first.  Fused engine only: Legacy and HostOnly instances
   * return false with a message on stderr.  Also false on a bad interval, lags or radius, and for a record or a read
   * with the correlation off.  The correlation is not part of a checkpoint. */
  bool setTimeCorrelation(float interval, unsigned lags, float overlapRadius);
  bool timeCorrelationRecord();
  bool timeCorrelationInfo(float &interval, unsigned &lags, float &overlapRadius, unsigned long long &records);
  bool timeCorrelationRows(std::vector<pbTimeCorrelationRow> &rows);
  /* The self-intermediate scattering function of the resident state on the device (pbSimSetScattering /
   * pbSimGetScattering, include/particlebot_hip.h has the definitions): setScattering(interval, lags, boxLog2, vectors)
   * starts a device ring of `lags` snapshots of the quantised positions, taken as the time correlation takes its own
   * (0: every step, -1: only by scatteringRecord), and a table of exact integer phasor sums per lag and wavevector
   * (2 pi / 2^boxLog2)(nx, ny) of `vectors`, which holds nx, ny pairs; lags 0 switches it off.  scatteringRecord takes
   * one record now; scatteringInfo gives interval, lags, boxLog2, the vectors' count and the records taken so far;
   * scatteringRows the lags * nvec rows, lag-major.  Fused engine only: Legacy and HostOnly instances return false with
   * a message on stderr.  Also false on a bad interval, lags, boxLog2 or list, and for a record or a read with the
   * scattering off.  The scattering is not part of a checkpoint. */
  bool setScattering(float interval, unsigned lags, int boxLog2, const std::vector<int> &vectors);
  bool scatteringRecord();
  bool scatteringInfo(float &interval, unsigned &lags, int &boxLog2, unsigned &nvec, unsigned long long &records);
  bool scatteringRows(std::vector<pbScatteringRow> &rows);
  /* The self van Hove function of the resident state on the device (pbSimSetVanHove / pbSimGetVanHove,
   * include/particlebot_hip.h has the definitions): setVanHove(interval, lags, binWidth, bins) keeps a device ring of
   * `lags` position snapshots, one taken in front of every step whose start time passes the schedule's gate at `interval`
   * (0: every step, -1: only by vanHoveRecord), and a table of exact integer histograms per lag: `bins` radial bins of
   * binWidth, 2 bins of each signed component, and the sums of the displacement's second and fourth powers; lags 0
   * switches it off.  vanHoveRecord takes one record now; vanHoveInfo gives interval, lags, binWidth, bins and the
   * records taken so far; vanHoveRows the `lags` rows and the lags * 5 * bins counters, per lag radial | x | y.  Fused
   * engine only: Legacy and HostOnly instances return false with a message in lastError(), as do bad arguments, and a
   * record or a read with the analysis off.  It is not part of a checkpoint. */
  bool setVanHove(float interval, unsigned lags, float binWidth, unsigned bins);
  bool vanHoveRecord();
  bool vanHoveInfo(float &interval, unsigned &lags, float &binWidth, unsigned &bins, unsigned long long &records);
  bool vanHoveRows(std::vector<pbVanHoveRow> &rows, std::vector<unsigned long long> &counts);
  /* The distinct van Hove function of the resident state on the device (pbSimSetVanHoveDistinct /
   * pbSimGetVanHoveDistinct, include/particlebot_hip.h has the definitions), shaped as the self part above:
   * setVanHoveDistinct(interval, lags, binWidth, bins) keeps a ring of `lags` position snapshots and, per lag, `bins`
   * exact counters of the ordered pairs (a bot then, another bot now) by distance; bins * binWidth must stay below 2048.
   * vanHoveDistinctRows gives the `lags` rows and the lags * bins counters.  Fused engine only; not part of a
   * checkpoint. */
  bool setVanHoveDistinct(float interval, unsigned lags, float binWidth, unsigned bins);
  bool vanHoveDistinctRecord();
  bool vanHoveDistinctInfo(float &interval, unsigned &lags, float &binWidth, unsigned &bins,
                           unsigned long long &records);
  bool vanHoveDistinctRows(std::vector<pbVanHoveDistinctRow> &rows, std::vector<unsigned long long> &counts);
  /* The coherent intermediate scattering function of the resident state on the device (pbSimSetCoherent /
   * pbSimGetCoherent, include/particlebot_hip.h has the definitions), shaped as the scattering above:
   * setCoherent(interval, lags, boxLog2, vectors) keeps a device ring of `lags` records of the density modes
   * rho(k) of `vectors` and, per lag and wavevector, the exact 192-bit integer sums of rho_now conj(rho_then) over all
   * time origins; lags 0 switches it off.  coherentRecord takes one record now; coherentInfo gives interval, lags,
   * boxLog2, the vectors' count and the records taken so far; coherentRows the lags * nvec rows, lag-major.  Fused engine
   * only: Legacy and HostOnly instances return false with a message on stderr.  Not part of a checkpoint. */
  bool setCoherent(float interval, unsigned lags, int boxLog2, const std::vector<int> &vectors);
  bool coherentRecord();
  bool coherentInfo(float &interval, unsigned &lags, int &boxLog2, unsigned &nvec, unsigned long long &records);
  bool coherentRows(std::vector<pbCoherentRow> &rows);
  /* Four-point dynamics of the resident state on the device (pbSimSetFourPoint / pbSimGetFourPoint,
   * include/particlebot_hip.h has the definitions), shaped as the scattering above:
   * setFourPoint(interval, lags, overlapRadius, boxLog2, vectors) keeps a device ring of `lags` records of the quantised
   * positions and, per lag, the exact integer sums over all time origins of the overlap count Q and of Q^2, and per
   * wavevector those of the density mode of the overlapping bots and of its squared magnitude: chi_4 and S_4(k, lag);
   * lags 0 switches it off.  fourPointRecord takes one record now; fourPointInfo gives interval, lags, overlapRadius,
   * boxLog2, the vectors' count and the records taken so far; fourPointRows the lags * nvec rows, lag-major.  Fused
   * engine only: Legacy and HostOnly instances return false with a message on stderr.  Not part of a checkpoint. */
  bool setFourPoint(float interval, unsigned lags, float overlapRadius, int boxLog2, const std::vector<int> &vectors);
  bool fourPointRecord();
  bool fourPointInfo(float &interval, unsigned &lags, float &overlapRadius, int &boxLog2, unsigned &nvec,
                     unsigned long long &records);
  bool fourPointRows(std::vector<pbFourPointRow> &rows);
  /* Bond dynamics of the resident state on the device (pbSimSetBondDynamics / pbSimGetBondDynamics,
   * include/particlebot_hip.h has the definitions), shaped as the time correlations above:
   * setBondDynamics(interval, lags, linkGap, maxRadius, overlapRadius) keeps a device ring of `lags` records of every
   * bot's quantised position and neighbour list and, per lag, the exact integer sums over all time origins of the
   * surviving links and of the cage-relative and plain squared displacements; lags 0 switches it off.
   * bondDynamicsRecord takes one record now; bondDynamicsInfo gives interval, lags, linkGap, maxRadius, overlapRadius and
   * the records taken so far; bondDynamicsRows the `lags` rows, lag 0 first.  A bot whose radius is above maxRadius is
   * absent.  Fused engine only: Legacy and HostOnly instances return false with a message on stderr.  Not part of a
   * checkpoint. */
  bool setBondDynamics(float interval, unsigned lags, float linkGap, float maxRadius, float overlapRadius);
  bool bondDynamicsRecord();
  bool bondDynamicsInfo(float &interval, unsigned &lags, float &linkGap, float &maxRadius, float &overlapRadius,
                        unsigned long long &records);
  bool bondDynamicsRows(std::vector<pbBondRow> &rows);
  /* A field map of the resident state on the device (pbSimFieldMap, include/particlebot_hip.h has the definition):
   * ny x nx cells, row 0 the lowest y, with count, dead and the integer sums of radius and velocity per cell, and the
   * totals row.  Fused engine only: Legacy and HostOnly instances return false with a message on stderr.  Also false on
   * nx or ny outside 1 ... PB_FIELD_MAX_AXIS and on a view whose half extents are not finite and > 0. */
  bool fieldMap(const pbFieldView &view, std::vector<pbFieldCell> &cells, pbFieldTotals &totals);
  /* The structure factor of the resident state on the device (pbSimStructureFactor, include/particlebot_hip.h has the
   * definition): one row of exact integer phasor sums per wavevector (2 pi / 2^boxLog2)(nx, ny) of `vectors`, which
   * holds nx, ny pairs.  Fused engine only: Legacy and HostOnly instances return false with a message on stderr.  Also
   * false on an unknown kind, on boxLog2 outside -8 ... 12 and on fewer than 1 or more than PB_SK_MAX_VECTORS pairs. */
  bool structureFactor(int kind, int boxLog2, const std::vector<int> &vectors, std::vector<pbStructureFactorRow> &rows);
  /* Extension: the reference's display state (off by default; call before reset()).  Legacy engine: POSITION / RADII
   * carry the reference's centroid_steps + 1 display entries, a colour buffer of (nCells + centroid_steps + 1) x 4
   * floats with the reference's fills (particlebot.cpp:105-141) exists, and every update runs calcCOG and updateCol at
   * the reference's two places (particlebot.cpp:207-209, 254); getColorBuffer / getCudaColorVBO return it.  Fused
   * engine: the engine's centroid trail (pbSimSetCentroidTrail).  The dynamics are the same either way. */
  void setDisplay(bool on);
  bool displayOn() const { return display; }
  /* nCells x 4 floats (RGBA, original order): the colours updateCol gives the current state */
  const float *getColorArray();
  /* the centroid ring (2 centroid_steps floats, y still + 2000), the start time of the step that wrote each slot (NaN:
   * never) and the records made so far; false when setDisplay(true) was not called.  Not carried by checkpoints. */
  bool getCentroidTrail(std::vector<float> &xy, std::vector<float> &times, unsigned &records);
  /* HostOnly engines follow an external clock */
  void setHostTime(float t) { time = t; }
  /* The private placement / dead-draw generator's state and the host mirrors of a HostOnly instance: what an
   * ensemble checkpoint saves and restores for a member whose device state lives in a batched pbSim. */
  void getHostRngState(int out[36]) const { rng.getState(out); }
  void setHostRngState(const int in[36]) { rng.setState(in); }
  void restoreHostMirrors(const float *pos, const float *vel, const float *rad, const float *phase, const int *dead);
  /* Extension (ensemble pipeline: members of a sweep that share seed and geometry are placed ONCE).  placementKey():
   * every input reset() reads -- the seed of the private generator, nCells, min/max_radius, the payload flag
   * (nDead == -1) and radFactor with it, config and the pb_placement extensions, the lattice pitch, Nx as given, and
   * the grid the placement bins into (gridSize, worldOrigin, cellSize).  nDead >= 0 is NOT part of it: the reference's
   * placement reads nDead only for the payload (particlebot.cpp:731, 786).  Two instances with equal keys place
   * identically, so one may take the other's result: exportPlacement() right after reset() captures positions, radii,
   * phases, dead flags, Nx and the generator's state AFTER the placement draws (the dead draw continues that stream,
   * particlebot.cpp:178-194); importPlacement() installs it in place of reset().  HostOnly engines. */
  struct Placement {
    std::vector<float> pos, rad, phase;
    std::vector<int> dead;
    int rng[36];
    unsigned configX, configY, Nx;
  };
  std::string placementKey() const { return placementKeyOf(params, hexSpacing, squareLattice, fastBlob); }
  static std::string placementKeyOf(const SimParams &params, float hexSpacing, bool squareLattice, bool fastBlob);
  void exportPlacement(Placement &out) const;
  bool importPlacement(const Placement &in);

 protected:
  void _initialize();
  void _finalize();
  void initGrid(uint2 size, float spacing, float jitter, uint numParticles);
  void initHexGrid(uint numParticles, float spacing);
  void placeRandom();
  void placeFastBlob();
  void drawDeadBots();
  void pullState(bool pos, bool vel, bool rad);
  void legacyUpdate(float deltaTime, float sort_interval);
  bool writeFrame(const char *path, int width, int height, float centerX, float centerY, float halfExtent,
                  float lightRadius, bool referenceStyle);
  void resetDisplayRing();
  /* the analyses above: refuse (with a line on stderr) unless the engine is the fused one, then run `call` and report
   * what the engine says when it fails (particlebot.cpp) */
  template <class Call>
  bool onFusedEngine(const char *method, const char *family, Call call, bool reportFailure = true);

  /* host mirrors (original bot order) */
  std::vector<float> hPosV, hVelV, hRadV, hPhaseV, hFreqV;
  std::vector<int> hDeadV;
  float *hPos = nullptr, *hVel = nullptr, *hRad = nullptr, *hphase = nullptr;
  int *hDead = nullptr;

  /* fused engine */
  pbSim *sim = nullptr;

  /* legacy engine: the reference's device buffers (particlebot.h:93-123) */
  float *dVel = nullptr, *dAbsForce_a = nullptr, *dAbsForce_r = nullptr, *dphase = nullptr;
  int *dDead = nullptr;
  pbRngState *dState = nullptr;
  float *dSortedPos = nullptr, *dSortedVel = nullptr, *dSortedRad = nullptr;
  uint *dGridParticleHash = nullptr, *dGridParticleIndex = nullptr, *dCellStart = nullptr, *dCellEnd = nullptr;
  struct pbGraphicsResource *posRes = nullptr, *radRes = nullptr;

  uint posVbo = 0, colorVBO = 0, radVbo = 0;
  float *cudaPosVBO = nullptr, *cudaColorVBO = nullptr, *cudaRadVBO = nullptr;

  float time = 0.0f;
  SimParams params;
  std::vector<float> obsStore; /* owns copies of the caller's obstacle arrays */
  uint2 particlebotConfigSize;
  Engine engineKind = Engine::Fused;
  float wallHalf = 64.0f;
  bool exitOnMaxTime = true;
  float hexSpacing = 0.0f;
  bool squareLattice = false;
  bool fastBlob = false;
  int rngKindV = 0; /* PB_RNG_COUNTER */
  PbLibcRand rng; /* seeded with params.seed at construction */
  /* display (setDisplay) */
  bool display = false;
  struct pbGraphicsResource *colRes = nullptr;
  float *dTempPos1 = nullptr, *dTempPos2 = nullptr; /* calcCOG's temporaries (legacy) */
  std::vector<float> hColV, trailTimesV;
  std::vector<unsigned char> frameV; /* writeFramePPMDevice's frame, kept between calls */
  unsigned trailRecords = 0;
};

#endif /* PARTICLEBOT_H */
