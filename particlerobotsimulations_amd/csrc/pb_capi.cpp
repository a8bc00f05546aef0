// pb_capi.cpp -- C wrappers around the C++ host side (class Particlebot + .cfg loader) so that
// scripts and tests can drive it through ctypes.  Exported from libparticlebot_host.so.
#include <gnu/libc-version.h>
#include <sched.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "particlebot.h"
#include "pb_config.hpp"
#include "pb_xorwow.hpp"

extern "C" {

// flat, pointer-free view of a resolved configuration (for inspection from scripts)
struct pbFlatConfig {
  uint32_t gridSizeX, gridSizeY, numCells;
  float worldOriginX, worldOriginY, cellSizeX, cellSizeY;
  uint32_t nCells;
  int32_t nDead;
  float gravity, spring, damping, shear, attraction, boundaryDamping, friction;
  float massFactor, frictionFactor, radFactor, attractionFactor;
  float constraint, constraint_contraction;
  int32_t centroid_steps;
  float centroid_int, centroid_radius;
  float light_x, light_y, phase_update_interval;
  int32_t control, config;
  float min_radius, max_radius, rise_period, freq;
  int32_t nobstacles;
  float x1obs[PB_MAX_OBSTACLES], x2obs[PB_MAX_OBSTACLES], y1obs[PB_MAX_OBSTACLES], y2obs[PB_MAX_OBSTACLES];
  int32_t n_cir_obstacles;
  float x_cir_obs[PB_MAX_OBSTACLES], y_cir_obs[PB_MAX_OBSTACLES], r_cir_obs[PB_MAX_OBSTACLES];
  int32_t Nx;
  float phase_std;
  uint32_t seed;
  uint32_t light_shadow, testing, constrained_contraction, display_shadow;
  float time_to_dead, max_time;
  float timestep, sort_interval, dump_interval;
  float camera_x, camera_y, light_radius;
  int32_t display_interval, video_interval;
  char csv_filename[300];
  char video_filename[300];
  float wallHalf;
  int rngKind;  // pb_rng (PB_RNG_*)
  int forceVariant;  // pb_force_variant (-1: the engine's default)
};

}  // extern "C"

namespace {

void flatten(const PbRunConfig &cfg, pbFlatConfig *o) {
  memset(o, 0, sizeof(*o));
  const SimParams &p = cfg.params;
  o->gridSizeX = p.gridSize.x;
  o->gridSizeY = p.gridSize.y;
  o->numCells = p.numCells;
  o->worldOriginX = p.worldOrigin.x;
  o->worldOriginY = p.worldOrigin.y;
  o->cellSizeX = p.cellSize.x;
  o->cellSizeY = p.cellSize.y;
  o->nCells = p.nCells;
  o->nDead = p.nDead;
  o->gravity = p.gravity;
  o->spring = p.spring;
  o->damping = p.damping;
  o->shear = p.shear;
  o->attraction = p.attraction;
  o->boundaryDamping = p.boundaryDamping;
  o->friction = p.friction;
  o->massFactor = p.massFactor;
  o->frictionFactor = p.frictionFactor;
  o->radFactor = p.radFactor;
  o->attractionFactor = p.attractionFactor;
  o->constraint = p.constraint;
  o->constraint_contraction = p.constraint_contraction;
  o->centroid_steps = p.centroid_steps;
  o->centroid_int = p.centroid_int;
  o->centroid_radius = p.centroid_radius;
  o->light_x = p.light_x;
  o->light_y = p.light_y;
  o->phase_update_interval = p.phase_update_interval;
  o->control = (int32_t)p.control;
  o->config = (int32_t)p.config;
  o->min_radius = p.min_radius;
  o->max_radius = p.max_radius;
  o->rise_period = p.rise_period;
  o->freq = p.freq;
  o->nobstacles = p.nobstacles;
  o->n_cir_obstacles = p.n_cir_obstacles;
  for (int i = 0; i < PB_MAX_OBSTACLES; i++) {
    if (i < p.nobstacles && i < (int)cfg.x1obs.size()) {
      o->x1obs[i] = cfg.x1obs[i];
      o->x2obs[i] = cfg.x2obs[i];
      o->y1obs[i] = cfg.y1obs[i];
      o->y2obs[i] = cfg.y2obs[i];
    }
    if (i < p.n_cir_obstacles && i < (int)cfg.x_cir_obs.size()) {
      o->x_cir_obs[i] = cfg.x_cir_obs[i];
      o->y_cir_obs[i] = cfg.y_cir_obs[i];
      o->r_cir_obs[i] = cfg.r_cir_obs[i];
    }
  }
  o->Nx = p.Nx;
  o->phase_std = p.phase_std;
  o->seed = p.seed;
  o->light_shadow = p.light_shadow;
  o->testing = p.testing;
  o->constrained_contraction = p.constrained_contraction;
  o->display_shadow = p.display_shadow;
  o->time_to_dead = p.time_to_dead;
  o->max_time = p.max_time;
  o->timestep = cfg.timestep;
  o->sort_interval = cfg.sort_interval;
  o->dump_interval = cfg.dump_interval;
  o->camera_x = cfg.camera_x;
  o->camera_y = cfg.camera_y;
  o->light_radius = cfg.light_radius;
  o->display_interval = cfg.display_interval;
  o->video_interval = cfg.video_interval;
  snprintf(o->csv_filename, sizeof(o->csv_filename), "%s", cfg.csv_filename.c_str());
  snprintf(o->video_filename, sizeof(o->video_filename), "%s", cfg.video_filename.c_str());
  o->wallHalf = cfg.wallHalf();
  o->rngKind = cfg.rng_kind;
  o->forceVariant = cfg.force_variant;
}

struct HostSim {
  PbRunConfig cfg;
  Particlebot *bot = nullptr;
};

// a result to the caller's array, which may be NULL (not wanted)
template <class T>
void copyOut(T *dst, const std::vector<T> &src) {
  if (dst && !src.empty()) memcpy(dst, src.data(), src.size() * sizeof(T));
}

}  // namespace

extern "C" {

// Resolve a configuration exactly as main() does (defaults, file, overrides, derived values).
// cfg_path may be NULL (defaults only).  Returns 0, or -1 if the file cannot be opened.
int pbHostLoadConfig(const char *cfg_path, const char *overrides, pbFlatConfig *out) {
  PbRunConfig cfg;
  if (!cfg.resolve(cfg_path, overrides, nullptr)) return -1;
  flatten(cfg, out);
  return 0;
}

// main.cpp:913-952 without GL: load, srand(seed), construct.  engine: 0 fused, 1 legacy.
void *pbHostCreate(const char *cfg_path, const char *overrides, int engine) {
  HostSim *h = new HostSim();
  if (!h->cfg.resolve(cfg_path, overrides, nullptr)) {
    delete h;
    return nullptr;
  }
  srand(h->cfg.params.seed);  // main.cpp:929
  // engine: 0 fused, 1 legacy, 2 host only (placement and draws without any device: CPU tests)
  h->bot = new Particlebot(h->cfg.params,
                           engine == 2   ? Particlebot::Engine::HostOnly
                           : engine == 1 ? Particlebot::Engine::Legacy
                                         : Particlebot::Engine::Fused,
                           h->cfg.wallHalf());
  h->bot->setExitOnMaxTime(false);
  h->bot->setHexSpacing(h->cfg.hex_spacing);
  h->bot->setSquareLattice(h->cfg.square_lattice);
  h->bot->setFastBlob(h->cfg.fast_blob);
  h->bot->setRng(h->cfg.rng_kind);
  h->bot->setForceVariant(h->cfg.force_variant);
  return h;
}

void pbHostDestroy(void *hv) {
  HostSim *h = (HostSim *)hv;
  if (!h) return;
  delete h->bot;
  delete h;
}

void pbHostReset(void *hv) { ((HostSim *)hv)->bot->reset(); }

void pbHostUpdate(void *hv) {
  HostSim *h = (HostSim *)hv;
  h->bot->update(h->cfg.timestep, h->cfg.sort_interval);
}

int pbHostAdvance(void *hv, int nsteps) {
  HostSim *h = (HostSim *)hv;
  return h->bot->advance(h->cfg.timestep, h->cfg.sort_interval, nsteps);
}

// steps that can run before the next dump row (or the end of the run) is due; >= 1
int pbHostStepsUntilDump(void *hv, int maxSteps) {
  HostSim *h = (HostSim *)hv;
  return h->bot->stepsUntilHostEvent(h->cfg.timestep, h->cfg.dump_interval, maxSteps);
}

float pbHostTime(void *hv) { return ((HostSim *)hv)->bot->getTime(); }
void pbHostSetTime(void *hv, float t) { ((HostSim *)hv)->bot->setTime(t); }
int pbHostFinished(void *hv) { return ((HostSim *)hv)->bot->finished() ? 1 : 0; }

// display()'s `dumpParticlebot(0, nCells, fp, dump_interval, testing, light)` (main.cpp:360)
int pbHostDump(void *hv, const char *path, const char *mode) {
  HostSim *h = (HostSim *)hv;
  FILE *fp = fopen(path, mode);
  if (!fp) return -1;
  const SimParams &p = h->bot->getParams();
  h->bot->dumpParticlebot(0, p.nCells, fp, h->cfg.dump_interval, p.testing, p.light_x, p.light_y);
  fclose(fp);
  return 0;
}

int pbHostLoadFromFile(void *hv, const char *path) {
  HostSim *h = (HostSim *)hv;
  FILE *fp = fopen(path, "r");
  if (!fp) return -1;
  h->bot->loadFromFile(0, h->bot->getParams().nCells, fp, h->cfg.dump_interval);
  fclose(fp);
  return 0;
}

// half <= 0 selects the reference's camera: centred on (camera_x, 0), half extent camera_y * tan(30 deg)
int pbHostWriteFrame(void *hv, const char *path, int width, int height, float cx, float cy, float half) {
  HostSim *h = (HostSim *)hv;
  if (!(half > 0)) {
    cx = h->cfg.camera_x;
    cy = 0.0f;
    half = h->cfg.camera_y * 0.57735027f;
  }
  return h->bot->writeFramePPM(path, width, height, cx, cy, half, h->cfg.light_radius) ? 0 : -1;
}

// style 0: writeFramePPM, 1: writeFramePPMReference (the device colours and the centroid trail)
int pbHostWriteFrameStyle(void *hv, const char *path, int width, int height, float cx, float cy, float half, int style) {
  HostSim *h = (HostSim *)hv;
  if (style == 0) return pbHostWriteFrame(hv, path, width, height, cx, cy, half);
  if (!(half > 0)) {
    cx = h->cfg.camera_x;
    cy = 0.0f;
    half = h->cfg.camera_y * 0.57735027f;
  }
  return h->bot->writeFramePPMReference(path, width, height, cx, cy, half, h->cfg.light_radius) ? 0 : -1;
}

// the same frames rasterised on the device (Particlebot::renderFrame / writeFramePPMDevice; fused engine only):
// path != NULL writes the PPM, rgb != NULL receives the 3 * width * height bytes.  half <= 0: the reference's camera.
int pbHostRenderFrame(void *hv, const char *path, unsigned char *rgb, int width, int height, float cx, float cy,
                      float half, int style) {
  HostSim *h = (HostSim *)hv;
  if (!(half > 0)) {
    cx = h->cfg.camera_x;
    cy = 0.0f;
    half = h->cfg.camera_y * 0.57735027f;
  }
  if (path && !h->bot->writeFramePPMDevice(path, width, height, cx, cy, half, h->cfg.light_radius, style != 0)) return -1;
  if (rgb) {
    std::vector<unsigned char> img;
    if (!h->bot->renderFrame(img, width, height, cx, cy, half, h->cfg.light_radius, style != 0)) return -1;
    memcpy(rgb, img.data(), img.size());
  }
  return 0;
}

// frames rendered on the device and the last one's device milliseconds; -1 unless the engine is the fused one
int pbHostRenderStats(void *hv, unsigned long long *frames, float *last_device_ms) {
  unsigned long long f = 0;
  float ms = 0.0f;
  if (!((HostSim *)hv)->bot->renderStats(f, ms)) return -1;
  if (frames) *frames = f;
  if (last_device_ms) *last_device_ms = ms;
  return 0;
}

// cluster analysis of the resident state (Particlebot::clusterStats / clusterLabels; fused engine only): the 32-byte
// pbClusterStats row, or labels and degrees (nCells unsigned each, original order).  -1 on the other engines or a bad gap.
int pbHostClusterStats(void *hv, float gap, pbClusterStats *out) {
  return out && ((HostSim *)hv)->bot->clusterStats(gap, *out) ? 0 : -1;
}

int pbHostClusterLabels(void *hv, float gap, unsigned *labels, unsigned *degree) {
  std::vector<unsigned> l, d;
  if (!((HostSim *)hv)->bot->clusterLabels(gap, l, d)) return -1;
  copyOut(labels, l);
  copyOut(degree, d);
  return 0;
}

// the contact network of the resident state (Particlebot::contacts / contactVirial; fused engine only).  *entries is
// always set on success; offsets (nCells + 1) and links may each be NULL, links is filled only when cap holds every
// entry (-1 otherwise: call once with links NULL to size).  -1 on the other engines or a bad gap.
int pbHostContacts(void *hv, float gap, unsigned *offsets, pbContactLink *links, unsigned long long cap,
                   unsigned long long *entries) {
  std::vector<unsigned> o;
  std::vector<pbContactLink> l;
  if (!entries || !((HostSim *)hv)->bot->contacts(gap, o, l)) return -1;
  *entries = l.size();
  if (links && cap < l.size()) return -1;
  copyOut(offsets, o);
  copyOut(links, l);
  return 0;
}

int pbHostContactVirial(void *hv, float gap, double *virial) {
  std::vector<double> v;
  if (!virial || !((HostSim *)hv)->bot->contactVirial(gap, v)) return -1;
  copyOut(virial, v);
  return 0;
}

// structure analysis of the resident state (Particlebot::radialCounts / structureStats / hexatic; fused engine only):
// `bins` counts, the 56-byte pbStructureStats row, or psi6 (2 nCells doubles) and neighbour counts (nCells), original
// order, either of which may be NULL.  -1 on the other engines or a bad rMax, bins or gap.
int pbHostRadialCounts(void *hv, float rMax, unsigned bins, unsigned long long *counts) {
  std::vector<unsigned long long> c;
  if (!counts || !((HostSim *)hv)->bot->radialCounts(rMax, bins, c)) return -1;
  copyOut(counts, c);
  return 0;
}

int pbHostStructureStats(void *hv, float gap, pbStructureStats *out) {
  return out && ((HostSim *)hv)->bot->structureStats(gap, *out) ? 0 : -1;
}

int pbHostHexatic(void *hv, float gap, double *psi6, unsigned *neighbours) {
  std::vector<double> p;
  std::vector<unsigned> nb;
  if (!((HostSim *)hv)->bot->hexatic(gap, p, nb)) return -1;
  copyOut(psi6, p);
  copyOut(neighbours, nb);
  return 0;
}

// rearrangement analysis of the resident state (Particlebot::markReference / rearrangementStats / rearrangement; fused
// engine only): the mark at `gap`, the 80-byte pbRearrangementStats row, or the per-bot displacement (2 nCells floats)
// and marked, present and kept bond counts (nCells each), original order, any of which may be NULL.  -1 on the other
// engines, a bad gap, or a compare without a mark.
int pbHostMarkReference(void *hv, float gap) { return ((HostSim *)hv)->bot->markReference(gap) ? 0 : -1; }

int pbHostRearrangementStats(void *hv, pbRearrangementStats *out) {
  return out && ((HostSim *)hv)->bot->rearrangementStats(*out) ? 0 : -1;
}

int pbHostRearrangementOf(void *hv, float *disp, unsigned *marked, unsigned *now, unsigned *kept) {
  std::vector<float> d;
  std::vector<unsigned> m, w, k;
  if (!((HostSim *)hv)->bot->rearrangement(d, m, w, k)) return -1;
  copyOut(disp, d);
  copyOut(marked, m);
  copyOut(now, w);
  copyOut(kept, k);
  return 0;
}

// strain analysis of the resident state against the mark (Particlebot::strainStats / strain; fused engine only): the
// 184-byte pbStrainStats row at `threshold`, or the per-bot moments (9 nCells), deformation gradient (4 nCells) and
// D2min (nCells), original order, any of which may be NULL.  -1 on the other engines, a bad threshold, or with no mark.
int pbHostStrainStats(void *hv, float threshold, pbStrainStats *out) {
  return out && ((HostSim *)hv)->bot->strainStats(threshold, *out) ? 0 : -1;
}

int pbHostStrainOf(void *hv, long long *moments, double *gradient, double *d2min) {
  std::vector<long long> m;
  std::vector<double> g, d;
  if (!((HostSim *)hv)->bot->strain(m, g, d)) return -1;
  copyOut(moments, m);
  copyOut(gradient, g);
  copyOut(d2min, d);
  return 0;
}

// time series of the resident state (Particlebot::moments / setSeries / seriesInfo / seriesRows; fused engine only): the
// 152-byte pbMomentsRow of the state as it is, the recorder's switch, what it holds, and the records from `first` on
// (cap entries of room; *count = how many there are).  -1 on the other engines, a bad interval or capacity, a read
// outside the ring's window or with the series off, or too little room.
int pbHostMoments(void *hv, pbMomentsRow *out) { return out && ((HostSim *)hv)->bot->moments(*out) ? 0 : -1; }

int pbHostSetSeries(void *hv, float interval, unsigned capacity) {
  return ((HostSim *)hv)->bot->setSeries(interval, capacity) ? 0 : -1;
}

int pbHostSeriesInfo(void *hv, float *interval, unsigned *capacity, unsigned long long *records) {
  float i = 0.0f;
  unsigned c = 0;
  unsigned long long r = 0;
  if (!((HostSim *)hv)->bot->seriesInfo(i, c, r)) return -1;
  if (interval) *interval = i;
  if (capacity) *capacity = c;
  if (records) *records = r;
  return 0;
}

int pbHostSeriesRows(void *hv, unsigned long long first, pbMomentsRow *rows, unsigned long long cap,
                     unsigned long long *count) {
  std::vector<pbMomentsRow> v;
  if (!count || !((HostSim *)hv)->bot->seriesRows(first, v)) return -1;
  *count = v.size();
  if (rows && cap < v.size()) return -1;
  copyOut(rows, v);
  return 0;
}

// pair correlations of the resident state (Particlebot::pairCorrelation; fused engine only): `bins` 56-byte
// pbCorrelationBin rows and, unless NULL, the 48-byte pbCorrelationTotals row.  -1 on the other engines, an unknown
// kind, a bad rMax or bins, or displacements without a mark.
int pbHostPairCorrelation(void *hv, int kind, float rMax, unsigned bins, pbCorrelationBin *rows,
                          pbCorrelationTotals *totals) {
  std::vector<pbCorrelationBin> r;
  pbCorrelationTotals t;
  if (!rows || !((HostSim *)hv)->bot->pairCorrelation(kind, rMax, bins, r, t)) return -1;
  copyOut(rows, r);
  if (totals) *totals = t;
  return 0;
}

// time correlations of the resident state (Particlebot::setTimeCorrelation / timeCorrelationRecord / timeCorrelationInfo
// / timeCorrelationRows; fused engine only): the recorder's switch, one record now, what it holds, and the 96-byte
// pbTimeCorrelationRow of every lag (cap entries of room; *count = how many there are).  -1 on the other engines, a bad
// interval, lags or radius, a record or a read with the correlation off, or too little room.
int pbHostSetTimeCorrelation(void *hv, float interval, unsigned lags, float overlapRadius) {
  return ((HostSim *)hv)->bot->setTimeCorrelation(interval, lags, overlapRadius) ? 0 : -1;
}

int pbHostTimeCorrelationRecord(void *hv) { return ((HostSim *)hv)->bot->timeCorrelationRecord() ? 0 : -1; }

int pbHostTimeCorrelationInfo(void *hv, float *interval, unsigned *lags, float *overlapRadius,
                              unsigned long long *records) {
  float i = 0.0f, a = 0.0f;
  unsigned l = 0;
  unsigned long long r = 0;
  if (!((HostSim *)hv)->bot->timeCorrelationInfo(i, l, a, r)) return -1;
  if (interval) *interval = i;
  if (lags) *lags = l;
  if (overlapRadius) *overlapRadius = a;
  if (records) *records = r;
  return 0;
}

int pbHostTimeCorrelationRows(void *hv, pbTimeCorrelationRow *rows, unsigned long long cap, unsigned long long *count) {
  std::vector<pbTimeCorrelationRow> v;
  if (!count || !((HostSim *)hv)->bot->timeCorrelationRows(v)) return -1;
  *count = v.size();
  if (rows && cap < v.size()) return -1;
  copyOut(rows, v);
  return 0;
}

// the self-intermediate scattering function of the resident state (Particlebot::setScattering / scatteringRecord /
// scatteringInfo / scatteringRows; fused engine only): the recorder's switch, one record now, what it holds, and the
// 56-byte pbScatteringRow of every lag and vector (cap entries of room; *count = how many there are).  -1 on the other
// engines, a bad interval, lags, box or list, a record or a read with the scattering off, or too little room.
int pbHostSetScattering(void *hv, float interval, unsigned lags, int boxLog2, const int *vectors, unsigned nvec) {
  if (!vectors && nvec) return -1;
  if (nvec > PB_SCATTER_MAX_VECTORS) nvec = PB_SCATTER_MAX_VECTORS + 1u;  // (refused below all the same; a huge count is not read)
  return ((HostSim *)hv)->bot->setScattering(interval, lags, boxLog2, std::vector<int>(vectors, vectors + 2 * (size_t)nvec))
             ? 0
             : -1;
}

int pbHostScatteringRecord(void *hv) { return ((HostSim *)hv)->bot->scatteringRecord() ? 0 : -1; }

int pbHostScatteringInfo(void *hv, float *interval, unsigned *lags, int *boxLog2, unsigned *nvec,
                         unsigned long long *records) {
  float i = 0.0f;
  unsigned l = 0, k = 0;
  int e = 0;
  unsigned long long r = 0;
  if (!((HostSim *)hv)->bot->scatteringInfo(i, l, e, k, r)) return -1;
  if (interval) *interval = i;
  if (lags) *lags = l;
  if (boxLog2) *boxLog2 = e;
  if (nvec) *nvec = k;
  if (records) *records = r;
  return 0;
}

int pbHostScatteringRows(void *hv, pbScatteringRow *rows, unsigned long long cap, unsigned long long *count) {
  std::vector<pbScatteringRow> v;
  if (!count || !((HostSim *)hv)->bot->scatteringRows(v)) return -1;
  *count = v.size();
  if (rows && cap < v.size()) return -1;
  copyOut(rows, v);
  return 0;
}

// the self van Hove function of the resident state (Particlebot::setVanHove / vanHoveRecord / vanHoveInfo / vanHoveRows;
// fused engine only): the recorder's switch, one record now, what it holds, and the 96-byte pbVanHoveRow of every lag
// with the lag's 5 * bins counters (cap rows and 5 * bins * cap counters of room; *count = how many rows there are).
// -1 on the other engines, a bad interval, lags, width or bins, a record or a read with the analysis off, or too
// little room.
int pbHostSetVanHove(void *hv, float interval, unsigned lags, float binWidth, unsigned bins) {
  return ((HostSim *)hv)->bot->setVanHove(interval, lags, binWidth, bins) ? 0 : -1;
}

int pbHostVanHoveRecord(void *hv) { return ((HostSim *)hv)->bot->vanHoveRecord() ? 0 : -1; }

int pbHostVanHoveInfo(void *hv, float *interval, unsigned *lags, float *binWidth, unsigned *bins,
                      unsigned long long *records) {
  float i = 0.0f, w = 0.0f;
  unsigned l = 0, b = 0;
  unsigned long long r = 0;
  if (!((HostSim *)hv)->bot->vanHoveInfo(i, l, w, b, r)) return -1;
  if (interval) *interval = i;
  if (lags) *lags = l;
  if (binWidth) *binWidth = w;
  if (bins) *bins = b;
  if (records) *records = r;
  return 0;
}

int pbHostVanHoveRows(void *hv, pbVanHoveRow *rows, unsigned long long *counts, unsigned long long cap,
                      unsigned long long *count) {
  std::vector<pbVanHoveRow> v;
  std::vector<unsigned long long> c;
  if (!count || !((HostSim *)hv)->bot->vanHoveRows(v, c)) return -1;
  *count = v.size();
  if ((rows || counts) && cap < v.size()) return -1;
  copyOut(rows, v);
  copyOut(counts, c);
  return 0;
}

// the distinct van Hove function of the resident state (Particlebot::setVanHoveDistinct / vanHoveDistinctRecord /
// vanHoveDistinctInfo / vanHoveDistinctRows; fused engine only), shaped as the self part's: the 48-byte
// pbVanHoveDistinctRow of every lag with the lag's bins counters (cap rows and bins * cap counters of room).  -1 on the
// other engines, a bad interval, lags, width or bins, a record or a read with the analysis off, or too little room.
int pbHostSetVanHoveDistinct(void *hv, float interval, unsigned lags, float binWidth, unsigned bins) {
  return ((HostSim *)hv)->bot->setVanHoveDistinct(interval, lags, binWidth, bins) ? 0 : -1;
}

int pbHostVanHoveDistinctRecord(void *hv) { return ((HostSim *)hv)->bot->vanHoveDistinctRecord() ? 0 : -1; }

int pbHostVanHoveDistinctInfo(void *hv, float *interval, unsigned *lags, float *binWidth, unsigned *bins,
                              unsigned long long *records) {
  float i = 0.0f, w = 0.0f;
  unsigned l = 0, b = 0;
  unsigned long long r = 0;
  if (!((HostSim *)hv)->bot->vanHoveDistinctInfo(i, l, w, b, r)) return -1;
  if (interval) *interval = i;
  if (lags) *lags = l;
  if (binWidth) *binWidth = w;
  if (bins) *bins = b;
  if (records) *records = r;
  return 0;
}

int pbHostVanHoveDistinctRows(void *hv, pbVanHoveDistinctRow *rows, unsigned long long *counts, unsigned long long cap,
                              unsigned long long *count) {
  std::vector<pbVanHoveDistinctRow> v;
  std::vector<unsigned long long> c;
  if (!count || !((HostSim *)hv)->bot->vanHoveDistinctRows(v, c)) return -1;
  *count = v.size();
  if ((rows || counts) && cap < v.size()) return -1;
  copyOut(rows, v);
  copyOut(counts, c);
  return 0;
}

// the coherent intermediate scattering function of the resident state (Particlebot::setCoherent / coherentRecord /
// coherentInfo / coherentRows; fused engine only), shaped as the self part's: the 96-byte pbCoherentRow of every lag and
// vector (cap entries of room; *count = how many there are).  -1 on the other engines, a bad interval, lags, box or
// list, a record or a read with the recorder off, or too little room.
int pbHostSetCoherent(void *hv, float interval, unsigned lags, int boxLog2, const int *vectors, unsigned nvec) {
  if (!vectors && nvec) return -1;
  if (nvec > PB_COHERENT_MAX_VECTORS) nvec = PB_COHERENT_MAX_VECTORS + 1u;  // (refused below all the same; a huge count is not read)
  return ((HostSim *)hv)->bot->setCoherent(interval, lags, boxLog2, std::vector<int>(vectors, vectors + 2 * (size_t)nvec))
             ? 0
             : -1;
}

int pbHostCoherentRecord(void *hv) { return ((HostSim *)hv)->bot->coherentRecord() ? 0 : -1; }

int pbHostCoherentInfo(void *hv, float *interval, unsigned *lags, int *boxLog2, unsigned *nvec,
                       unsigned long long *records) {
  float i = 0.0f;
  unsigned l = 0, k = 0;
  int e = 0;
  unsigned long long r = 0;
  if (!((HostSim *)hv)->bot->coherentInfo(i, l, e, k, r)) return -1;
  if (interval) *interval = i;
  if (lags) *lags = l;
  if (boxLog2) *boxLog2 = e;
  if (nvec) *nvec = k;
  if (records) *records = r;
  return 0;
}

int pbHostCoherentRows(void *hv, pbCoherentRow *rows, unsigned long long cap, unsigned long long *count) {
  std::vector<pbCoherentRow> v;
  if (!count || !((HostSim *)hv)->bot->coherentRows(v)) return -1;
  *count = v.size();
  if (rows && cap < v.size()) return -1;
  copyOut(rows, v);
  return 0;
}

// four-point dynamics of the resident state (Particlebot::setFourPoint / fourPointRecord / fourPointInfo /
// fourPointRows; fused engine only), shaped as the coherent recorder's: the 128-byte pbFourPointRow of every lag and
// vector (cap entries of room; *count = how many there are).  -1 on the other engines, a bad interval, lags, radius, box
// or list, a record or a read with the recorder off, or too little room.
int pbHostSetFourPoint(void *hv, float interval, unsigned lags, float overlapRadius, int boxLog2, const int *vectors,
                       unsigned nvec) {
  if (!vectors && nvec) return -1;
  if (nvec > PB_FOURPOINT_MAX_VECTORS) nvec = PB_FOURPOINT_MAX_VECTORS + 1u;  // (refused below all the same; a huge count is not read)
  return ((HostSim *)hv)->bot->setFourPoint(interval, lags, overlapRadius, boxLog2,
                                            std::vector<int>(vectors, vectors + 2 * (size_t)nvec))
             ? 0
             : -1;
}

int pbHostFourPointRecord(void *hv) { return ((HostSim *)hv)->bot->fourPointRecord() ? 0 : -1; }

int pbHostFourPointInfo(void *hv, float *interval, unsigned *lags, float *overlapRadius, int *boxLog2, unsigned *nvec,
                        unsigned long long *records) {
  float i = 0.0f, a = 0.0f;
  unsigned l = 0, k = 0;
  int e = 0;
  unsigned long long r = 0;
  if (!((HostSim *)hv)->bot->fourPointInfo(i, l, a, e, k, r)) return -1;
  if (interval) *interval = i;
  if (lags) *lags = l;
  if (overlapRadius) *overlapRadius = a;
  if (boxLog2) *boxLog2 = e;
  if (nvec) *nvec = k;
  if (records) *records = r;
  return 0;
}

int pbHostFourPointRows(void *hv, pbFourPointRow *rows, unsigned long long cap, unsigned long long *count) {
  std::vector<pbFourPointRow> v;
  if (!count || !((HostSim *)hv)->bot->fourPointRows(v)) return -1;
  *count = v.size();
  if (rows && cap < v.size()) return -1;
  copyOut(rows, v);
  return 0;
}

// bond dynamics of the resident state (Particlebot::setBondDynamics / bondDynamicsRecord / bondDynamicsInfo /
// bondDynamicsRows; fused engine only), shaped as the four-point recorder's: the 360-byte pbBondRow of every lag (cap
// entries of room; *count = how many there are).  -1 on the other engines, a bad interval, lags, gap or radius, a record
// or a read with the recorder off, or too little room.
int pbHostSetBondDynamics(void *hv, float interval, unsigned lags, float linkGap, float maxRadius, float overlapRadius) {
  return ((HostSim *)hv)->bot->setBondDynamics(interval, lags, linkGap, maxRadius, overlapRadius) ? 0 : -1;
}

int pbHostBondDynamicsRecord(void *hv) { return ((HostSim *)hv)->bot->bondDynamicsRecord() ? 0 : -1; }

int pbHostBondDynamicsInfo(void *hv, float *interval, unsigned *lags, float *linkGap, float *maxRadius,
                           float *overlapRadius, unsigned long long *records) {
  float i = 0.0f, g = 0.0f, m = 0.0f, a = 0.0f;
  unsigned l = 0;
  unsigned long long r = 0;
  if (!((HostSim *)hv)->bot->bondDynamicsInfo(i, l, g, m, a, r)) return -1;
  if (interval) *interval = i;
  if (lags) *lags = l;
  if (linkGap) *linkGap = g;
  if (maxRadius) *maxRadius = m;
  if (overlapRadius) *overlapRadius = a;
  if (records) *records = r;
  return 0;
}

int pbHostBondDynamicsRows(void *hv, pbBondRow *rows, unsigned long long cap, unsigned long long *count) {
  std::vector<pbBondRow> v;
  if (!count || !((HostSim *)hv)->bot->bondDynamicsRows(v)) return -1;
  *count = v.size();
  if (rows && cap < v.size()) return -1;
  copyOut(rows, v);
  return 0;
}

// a field map of the resident state (Particlebot::fieldMap; fused engine only): ny * nx 64-byte pbFieldCell entries and,
// unless NULL, the 16-byte pbFieldTotals row.  -1 on the other engines and on a bad view.
int pbHostFieldMap(void *hv, const pbFieldView *view, pbFieldCell *cells, pbFieldTotals *totals) {
  std::vector<pbFieldCell> c;
  pbFieldTotals t;
  if (!view || !cells || !((HostSim *)hv)->bot->fieldMap(*view, c, t)) return -1;
  copyOut(cells, c);
  if (totals) *totals = t;
  return 0;
}

// the structure factor of the resident state (Particlebot::structureFactor; fused engine only): nvec 80-byte
// pbStructureFactorRow entries for the nvec (nx, ny) pairs of `vectors`.  -1 on the other engines and on a bad argument.
int pbHostStructureFactor(void *hv, int kind, int boxLog2, const int *vectors, unsigned nvec, pbStructureFactorRow *rows) {
  if (!vectors || !rows) return -1;
  std::vector<pbStructureFactorRow> r;
  if (!((HostSim *)hv)->bot->structureFactor(kind, boxLog2, std::vector<int>(vectors, vectors + 2 * (size_t)nvec), r))
    return -1;
  copyOut(rows, r);
  return 0;
}

void pbHostSetDisplay(void *hv, int on) { ((HostSim *)hv)->bot->setDisplay(on != 0); }

// the centroid ring (2 centroid_steps floats), the slots' start times and the record count; -1 with display off
int pbHostCentroidTrail(void *hv, float *xy, float *times, unsigned *records) {
  std::vector<float> a, b;
  unsigned r = 0;
  if (!((HostSim *)hv)->bot->getCentroidTrail(a, b, r)) return -1;
  copyOut(xy, a);
  copyOut(times, b);
  if (records) *records = r;
  return 0;
}

int pbHostSaveCheckpoint(void *hv, const char *path) {
  FILE *fp = fopen(path, "wb");
  if (!fp) return -1;
  const bool ok = ((HostSim *)hv)->bot->saveCheckpoint(fp);
  fclose(fp);
  return ok ? 0 : -2;
}

int pbHostLoadCheckpoint(void *hv, const char *path) {
  FILE *fp = fopen(path, "rb");
  if (!fp) return -1;
  const bool ok = ((HostSim *)hv)->bot->loadCheckpoint(fp);
  fclose(fp);
  return ok ? 0 : -2;
}

// draws the dead set now (what update() does at time_to_dead) and returns it; host mirrors only
int pbHostDrawDead(void *hv, int *out) {
  HostSim *h = (HostSim *)hv;
  const int *d = h->bot->drawDeadBotsNow();
  memcpy(out, d, sizeof(int) * h->bot->getParams().nCells);
  return 0;
}

// which: 0 POSITION (2n floats) 1 VELOCITY (2n) 2 RADII (n) 3 PHASE (n) 5 DEAD (n ints)
int pbHostGetArray(void *hv, int which, void *out) {
  HostSim *h = (HostSim *)hv;
  const size_t n = h->bot->getParams().nCells;
  switch (which) {
    case 0: memcpy(out, h->bot->getArray(POSITION), 8 * n); return 0;
    case 1: memcpy(out, h->bot->getArray(VELOCITY), 8 * n); return 0;
    case 2: memcpy(out, h->bot->getArray(RADII), 4 * n); return 0;
    case 3: memcpy(out, h->bot->getArray(PHASE), 4 * n); return 0;
    case 5: memcpy(out, h->bot->getDeadArray(), 4 * n); return 0;
    case 6: memcpy(out, h->bot->getColorArray(), 16 * n); return 0;  // RGBA (Particlebot::getColorArray)
    default: return -1;
  }
}

int pbHostSetArray(void *hv, int which, const float *data, int start, int count) {
  HostSim *h = (HostSim *)hv;
  if (which < 0 || which > 4) return -1;
  h->bot->setArray((ParticlebotArray)which, data, start, count);
  return 0;
}

// n draws of the class's glibc-compatible generator after seeding (for the CPU test against rand())
void pbHostLibcRandDraws(unsigned seed, int n, int *out) {
  PbLibcRand g(seed);
  for (int i = 0; i < n; i++) out[i] = g.next();
}

// ---- the libm properties the phase update rests on (pbSimSetMinDistanceMode 0) ---------------------
// The engine returns min_i (dx*dx + dy*dy) from the device and takes powf(., 0.5f) on the host, where the
// reference takes min_i powf(powf(dx,2) + powf(dy,2), 0.5f) (particlebot.cpp:215-228).  The two agree for every
// input iff, on THIS host's libm, powf(x, 2.0f) == x*x bit for bit for every float and powf(., 0.5f) is
// non-decreasing over the non-negative floats.  Checked exhaustively: every non-negative float (the square also
// for every 16th negative one; 2^31 values, ~15 s on 8 cores).  stride > 1 samples every stride-th float.
// Returns 0 when both hold.
int pbHostLibmCheck(int threads, unsigned stride, unsigned long long *checked, unsigned long long *square_mismatches,
                    unsigned long long *root_inversions) {
  if (threads < 1) threads = (int)std::max(1u, std::thread::hardware_concurrency());
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) threads = std::min(threads, CPU_COUNT(&set));
  threads = std::max(1, std::min(threads, 256));
  if (stride < 1) stride = 1;
  const uint64_t last = 0x7F800000ull;  // +inf included
  std::vector<unsigned long long> bad(threads, 0), inv(threads, 0), seen(threads, 0);
  auto work = [&](int t) {
    const uint64_t lo = last * (uint64_t)t / (uint64_t)threads, hi = last * (uint64_t)(t + 1) / (uint64_t)threads;
    // (each chunk starts one float early so that the monotonicity test spans the chunk boundaries)
    uint32_t b0 = (uint32_t)(lo == 0 ? 0 : lo - 1);
    float x0;
    memcpy(&x0, &b0, 4);
    float prev = powf(x0, 0.5f);
    const uint64_t end = (t == threads - 1) ? hi + 1 : hi;  // (+inf belongs to the last chunk)
    for (uint64_t b = lo; b < end; b += stride) {
      const uint32_t bits = (uint32_t)b;
      float x;
      memcpy(&x, &bits, 4);
      const float sq = powf(x, 2.0f), mul = x * x;
      if (memcmp(&sq, &mul, 4) != 0) bad[t]++;
      if ((bits & 15u) == 0u) {  // the negative argument: every 16th float
        const float sqn = powf(-x, 2.0f);
        if (memcmp(&sqn, &mul, 4) != 0) bad[t]++;
      }
      const float r = powf(x, 0.5f);
      if (r < prev) inv[t]++;
      prev = r;
      seen[t]++;
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; t++) pool.emplace_back(work, t);
  work(0);
  for (auto &th : pool) th.join();
  unsigned long long b = 0, i = 0, n = 0;
  for (int t = 0; t < threads; t++) b += bad[t], i += inv[t], n += seen[t];
  if (checked) *checked = n;
  if (square_mismatches) *square_mismatches = b;
  if (root_inversions) *root_inversions = i;
  return (b == 0 && i == 0) ? 0 : 1;
}

const char *pbHostLibcVersion(void) { return gnu_get_libc_version(); }

// ---- csrc/pb_xorwow.hpp on the host (CPU tests: the same code the kernels run) -------------------
static const uint32_t *hostJumpTable() {
  static std::vector<uint32_t> table;
  static std::once_flag once;
  std::call_once(once, [] {
    table.resize(PB_XW_TABLE_WORDS);
    pbXorwowBuildJumpTable(table.data());
  });
  return table.data();
}

// the first `count` raw outputs of curand_init(seed, subsequence, 0)
void pbHostXorwowOutputs(int kind, unsigned long long seed, unsigned subsequence, unsigned count, unsigned *out) {
  pbRngState s;
  pbXorwowSeed(s, seed, kind);
  pbXorwowSkipSubsequences(s, subsequence, hostJumpTable());
  for (unsigned i = 0; i < count; i++) out[i] = pbXorwowNext(s);
}

// `draws` normals of each of the bots 0..nbots-1 (out[draw][bot]), as add_normal_noise consumes them
void pbHostXorwowNormals(int kind, unsigned seed, unsigned nbots, unsigned draws, float *out) {
  for (unsigned i = 0; i < nbots; i++) {
    pbRngState s;
    pbXorwowSeed(s, (uint64_t)seed, kind);
    pbXorwowSkipSubsequences(s, i, hostJumpTable());
    for (unsigned k = 0; k < draws; k++) out[(size_t)k * nbots + i] = pbXorwowNormal(s);
  }
}

// table[k] (160 x 5 words), k = 0..31
void pbHostXorwowJumpMatrix(unsigned k, unsigned *rows) {
  memcpy(rows, hostJumpTable() + (size_t)(k & 31u) * PB_XW_MAT_WORDS, sizeof(uint32_t) * PB_XW_MAT_WORDS);
}

// the fused engine behind a HostSim (NULL for the other engines): lets a script reach pbSim* calls the
// class does not wrap
void *pbHostEngineHandle(void *hv) { return ((HostSim *)hv)->bot->engineHandle(); }

unsigned pbHostNumBots(void *hv) { return ((HostSim *)hv)->bot->getParams().nCells; }
int pbHostCentroidSteps(void *hv) { return ((HostSim *)hv)->bot->getParams().centroid_steps; }

}  // extern "C"

