// pb_runner.cpp -- headless replacement for the reference's GLUT main loop.
//
//   particlebot_run [config.cfg] [--set NAME VALUE]... [--engine fused|legacy] [--quiet]
//                   [--frames DIR [--frame-size PIXELS] [--frame-style plain|reference] [--frame-render host|device]]
//                   [--trail FILE] [--clusters FILE [--cluster-gap G]] [--contacts FILE [--contact-gap G]]
//                   [--structure FILE [--structure-gap G]] [--rdf FILE [--rdf-rmax R] [--rdf-bins B]]
//                   [--rearrange FILE [--rearrange-gap G] [--rearrange-window]]
//                   [--series FILE [--series-interval T] [--series-capacity N]]
//                   [--correlate FILE [--correlate-kind velocity|radius] [--correlate-rmax R] [--correlate-bins B]]
//                   [--timecorr FILE [--timecorr-interval T] [--timecorr-lags N] [--timecorr-overlap A]]
//                   [--field FILE [--field-cells N] [--field-half H]]
//                   [--sk FILE [--sk-kind density|radius|velocity] [--sk-box-log2 E] [--sk-nmax M]]
//                   [--scatter FILE [--scatter-interval T] [--scatter-lags N] [--scatter-box-log2 E] [--scatter-nmax M]]
//                   [--resume FILE [--overwrite-csv]] [--checkpoint FILE [--checkpoint-every SECONDS] [--checkpoint-steps N]]
//                   [--final-checkpoint FILE]
//
// --resume FILE continues a run (main.cpp:954-957 -> particlebot.cpp:369-411): FILE is either an exact checkpoint
// written by --checkpoint (time, every state array incl. phase / dead / force sums, the stale slot layout, both
// random generators, and the length the CSV had: the resumed run is bit-identical to the uninterrupted one and the
// CSV ends up byte-identical) or, as in the reference, a testing=1 CSV whose last complete row supplies time,
// positions, velocities and radii (phases, dead set and force sums start afresh: the reference's lossy resume).
// When that CSV is csv_filename itself -- the same file by device and inode, however the two paths are spelled -- the
// run appends to it as the reference does (main.cpp:940-956); when it is another file, an existing non-empty
// csv_filename is only truncated with --overwrite-csv.
// --checkpoint FILE is rewritten (write to FILE.tmp, rename) every --checkpoint-every SECONDS of wall time
// and/or every --checkpoint-steps timesteps, always at a point where the main loop is about to dump.
//
// main.cpp:823-967 minus the window: defaults, the .cfg file (default "example.cfg"), srand(seed),
// derived grid parameters, open the CSV, construct + reset, then `for(;;){ dump(); update(); }`
// (display(), main.cpp:354-361).  Between dump rows the steps are handed to the engine in one
// batch so that it can keep one fused kernel per timestep.  --frames DIR writes a PPM of the arena
// every VIDEO_INTERVAL timesteps (the reference's video cadence, main.cpp:455-470), viewed like the
// reference's camera: centred on (camera_x, 0), half extent camera_y * tan(30 deg); --frame-style reference draws them
// in the device colours of updateCol with the centroid trail (Particlebot::writeFramePPMReference).
// --frame-render device rasterises the frames on the GPU from the engine's resident state (Particlebot::writeFramePPMDevice:
// the same bytes, no state copy; fused engine only); host (default) is the class's CPU writer.  --trail FILE
// records the reference's centroid trail (Particlebot::setDisplay) and writes it at the end of the run as
// `slot,time,x,y` rows (slots holding a record; fp32 time and x to 9 digits), y as the double (stored y) - 2000, without the shader's +2000 (a resumed run starts a fresh trail).
// --clusters FILE appends, at every dump time (the gate dumpParticlebot uses), one row of the device's cluster analysis
// (Particlebot::clusterStats): `Time, Clusters, Largest, Isolated, Links, MaxDegree`, the header once at time 0;
// --cluster-gap G (default 0, finite and >= 0) is the analysis' linkGap.  Without --clusters nothing is analysed.
// --contacts FILE writes the contact network of the FINAL state once, when the run ends (Particlebot::contacts):
// the header `I, J, Gap, Fx, Fy`, then one row per directed entry in CSR order (I ascending, J ascending within I),
// floats as %.9g so that fp32 round-trips; --contact-gap G (default 0, finite and >= 0) is its linkGap.
// --structure FILE appends, at every dump time, one row of the device's hexatic analysis (Particlebot::structureStats):
// `Time, Bonds, Psi6Re, Psi6Im, C0, C1, C2, C3, C4, C5, C6, C7`, the header once at time 0, the sums as the integers
// they are (units of 2^-30); --structure-gap G (default 0, finite and >= 0) is its linkGap.
// --rdf FILE writes the radial pair counts of the FINAL state once, when the run ends (Particlebot::radialCounts): the
// header `RLo, RHi, Count`, then one row per bin, the edges b * R / B and (b + 1) * R / B in double as %.9g;
// --rdf-rmax R (default 10 * max_radius, finite and > 0) and --rdf-bins B (default 200, 1 ... 4096).
// --rearrange FILE marks a reference on the device at the run's first dump time (Particlebot::markReference; time 0, or
// the time a resumed run starts at: the mark is not part of a checkpoint) and appends, at every dump time, the first
// included, one row that compares the state with it (Particlebot::rearrangementStats): `Time, MarkTime, BondsMarked,
// BondsNow, BondsKept, Unchanged, Lost, Gained, Measured, SumQx, SumQy, SumQ2, MaxQ2`, the header once, every number
// the integer it is (bonds directed, SumQx / SumQy in units of 2^-20, SumQ2 / MaxQ2 of 2^-40; SumQ2 in decimal from its
// 128 bits); --rearrange-gap G (default 0, finite and >= 0) is the mark's linkGap; --rearrange-window marks again after
// each row, so that every row describes one dump interval.
// --series FILE switches the device's time-series recorder on (Particlebot::setSeries): while the engine steps, one row
// of integer moments of positions, velocities and radii (pbMomentsRow, include/particlebot_hip.h) is taken in front of
// every step whose start time passes the schedule's gate at --series-interval T (default dump_interval, so that the
// rows line up with the CSV; 0: every step; finite and >= 0) into a device ring of --series-capacity N rows (default
// 4096, 1 ... 1048576).  The runner drains the new records at every host stop of its loop and once after it, and never
// hands the engine more than N steps in one batch, so no record is overwritten unread.  FILE gets the header `Time,
// Step, Measured, SumQx, SumQy, MinQx, MaxQx, MinQy, MaxQy, SumXX, SumYY, SumXY, SumQr, SumRR, SumWx, SumWy, SumVV`
// once, then one line per record: Time as %.9g, every other number the integer it is (sums of q in units of 2^-20, sums
// of products of 2^-40, in decimal from their 128 bits, SumXY signed).  A resumed run appends from the resume point (the
// series is not part of a checkpoint).  (The usage line printed on a bad command line does not list these three.)
// --correlate FILE writes the pair correlations of the FINAL state once, when the run ends
// (Particlebot::pairCorrelation): line 1 the totals, `Kind, <kind>, Measured, <m>, SumAx, <..>, SumAy, <..>, SumA2, <..>,
// Pairs, <..>`; line 2 the header `RLo, RHi, Pairs, Dot, SumAx, SumAy`; then one row per bin, the edges as --rdf prints
// them, every other number the integer it is (Dot and SumA2 in units of 2^-40, the sums of a in units of 2^-20, in
// decimal from their 128 bits).  --correlate-kind velocity|radius (default velocity; displacements need a mark and are
// left to the API), --correlate-rmax R (default 10 * max_radius, finite and > 0) and --correlate-bins B (default 200,
// 1 ... 1024).  (The usage line does not list these four either.)
// --timecorr FILE switches the device's time correlations on (Particlebot::setTimeCorrelation): while the engine steps,
// a snapshot of positions and velocities is taken in front of every step whose start time passes the schedule's gate at
// --timecorr-interval T (default dump_interval; 0: every step; finite and >= 0) into a device ring of --timecorr-lags N
// snapshots (default 32, 1 ... 64), and every record is added against the N latest ones into one row per lag:
// squared displacement, velocity products and the count of bots that moved less than --timecorr-overlap A (default the
// configuration's min_radius, a default and not a claim; finite, 0 <= A < 2048).  Switched on behind a resume, like the
// series (the correlation is not part of a checkpoint).  At the end of the run FILE gets the header `Lag, Origins,
// SumSteps, Samples, SumQx, SumQy, SumQ2, SumWW, Overlap, MaxQ2`, then one line per lag, lag 0 first, every number the
// integer it is (SumQx / SumQy in units of 2^-20, SumQ2, SumWW and MaxQ2 of 2^-40, the 128-bit sums in decimal, SumWW
// signed); the mean lag of a row is SumSteps / Origins steps.  A lag's sums are exact only below 2^31 samples, and the
// engine refuses a table that holds more: the records the run will take (from max_time, the start time and the
// interval) times nCells must stay below 2^31 (10^6 bots: 2147 records), or the run is refused when it starts (exit
// 2, "--timecorr: ... 2^31 samples"), before a step is taken.  (The usage line does not list these four either.)
// --field FILE appends, at every dump time (the steps at which --clusters writes its rows), one block of the device's
// field map of the state (Particlebot::fieldMap): a square map of --field-cells N x N cells (default 64, 1 ... 1024)
// centred on (0, 0) with half extent --field-half H (default the wall half extent; finite and > 0).  FILE gets the
// header `time,step,ix,iy,count,dead,sum_qr,sum_wx,sum_wy,rr,vv` once, then per block one line per NON-EMPTY cell, row 0
// the lowest y: time as %.9g, step the steps taken so far, every other number the integer it is (the sums in units of
// 2^-20, rr and vv of 2^-40, in decimal from their 128 bits as --correlate prints them).  (The usage line does not list
// these three either.)
// --sk FILE appends, at every dump time, one block of the device's structure factor of the state
// (Particlebot::structureFactor): the wavevectors (2 pi / 2^E)(nx, ny) of the half plane ny > 0 || (ny == 0 && nx > 0)
// with |nx|, |ny| <= --sk-nmax M (default 16: 544 vectors; 1 ... 44, 45 would pass PB_SK_MAX_VECTORS), the box
// --sk-box-log2 E (default the smallest E with 2^E >= twice the wall half extent, at most 12; -8 ... 12) and the weight
// --sk-kind density|radius|velocity (default density).  A block is the line `time,<%.9g>,step,<steps so far>,kind,<kind>,
// box_log2,<E>,vectors,<count>` and then one line per vector, `nx,ny,measured,re,im,re2,im2`, every number the integer it
// is (units of 2^-30 for the density, 2^-50 otherwise, in decimal from their 128 bits, signed).  (The usage line does
// not list these four either.)
// --scatter FILE switches the device's self-intermediate scattering function on (Particlebot::setScattering): while the
// engine steps, a snapshot of the quantised positions is taken in front of every step whose start time passes the
// schedule's gate at --scatter-interval T (default dump_interval; 0: every step; finite and >= 0) into a device ring of
// --scatter-lags N snapshots (default 32, 1 ... 64), and every record is added against the N latest ones into one row
// per lag and wavevector: the integer phasor sums of every bot's displacement.  The wavevectors are --sk's half plane
// with |nx|, |ny| <= --scatter-nmax M (default 3: 24 vectors; 1 ... 10, 11 would pass PB_SCATTER_MAX_VECTORS) in the box
// --scatter-box-log2 E (default as --sk chooses it; -8 ... 12).  Switched on behind a resume, like --timecorr (the ring
// is not part of a checkpoint).  At the end of the run FILE gets the header `Lag, Nx, Ny, Origins, SumSteps, Samples, Re,
// Im, FsRe, FsIm`, then one line per lag and vector, lag 0 first, the vectors in list order: the integers as they are (Re
// and Im in units of 2^-30), then FsRe = Re / (2^30 Samples) and FsIm likewise as %.9g (nan with no sample).  As with
// --timecorr, a run whose records times nCells would reach 2^31 is refused when it starts (exit 2, "--scatter: ... 2^31
// samples").  (The usage line does not list these five either.)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

#include <chrono>

#include "particlebot.h"
#include "pb_config.hpp"

namespace {

// what the runner appends to the class's exact checkpoint: where its own loop was
struct RunTrailer {
  char magic[8] = {'P', 'B', 'R', 'U', 'N', 'v', '1', 0};
  long long csvBytes = 0;  // length of the CSV when the checkpoint was taken (rows written since are cut off)
  long long stepsDone = 0, frames = 0;
};

bool isExactCheckpoint(const std::string &path) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return false;
  char m[8] = {0};
  const bool ok = fread(m, 1, 8, f) == 8 && memcmp(m, "PBCKPT", 6) == 0;
  fclose(f);
  return ok;
}

bool readTrailer(const std::string &path, RunTrailer &t) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return false;
  RunTrailer got;
  const bool ok = fseek(f, -(long)sizeof got, SEEK_END) == 0 && fread(&got, sizeof got, 1, f) == 1 &&
                  memcmp(got.magic, t.magic, 8) == 0;
  fclose(f);
  if (ok) t = got;
  return ok;
}

// a 128-bit unsigned integer in decimal
std::string decimal128(unsigned long long hi, unsigned long long lo) {
  unsigned __int128 v = ((unsigned __int128)hi << 64) | lo;
  std::string s;
  do {
    s.insert(s.begin(), (char)('0' + (int)(v % 10)));
    v /= 10;
  } while (v != 0);
  return s;
}

// hi * 2^32 + lo, the two accumulators of a pbMoment128: a signed 128-bit integer in decimal
std::string decimal128(const pbMoment128 &m) {
  const __int128 v = (__int128)m.hi * ((__int128)1 << 32) + (__int128)m.lo;
  const unsigned __int128 mag = v < 0 ? -(unsigned __int128)v : (unsigned __int128)v;
  return (v < 0 ? "-" : "") + decimal128((unsigned long long)(mag >> 64), (unsigned long long)mag);
}

// a flag's value: the whole string a finite float, >= lowest (> lowest when `above`)
bool parseFloat(const char *text, float lowest, bool above, float &value) {
  char *end = nullptr;
  value = strtof(text, &end);
  return end != text && !*end && (above ? value > lowest : value >= lowest) && !std::isinf(value);
}

// an analysis output; NULL after saying so
FILE *openOutput(const std::string &path, const char *mode) {
  FILE *f = fopen(path.c_str(), mode);
  if (!f) fprintf(stderr, "cannot open %s\n", path.c_str());
  return f;
}

}  // namespace

int main(int argc, char **argv) {
  PbRunConfig cfg;
  std::string path = "example.cfg";
  std::vector<std::pair<std::string, std::string>> sets;
  Particlebot::Engine engine = Particlebot::Engine::Fused;
  bool quiet = false, overwriteCsv = false;
  std::string framesDir, resumePath, ckptPath, finalCkptPath;
  int frameSize = 800;
  bool referenceFrames = false, deviceFrames = false;
  std::string trailPath, clustersPath, contactsPath;
  float clusterGap = 0.0f, contactGap = 0.0f;
  std::string structurePath, rdfPath;
  float structureGap = 0.0f, rdfRmax = 0.0f;  // rdfRmax 0: 10 * max_radius, once the configuration is loaded
  long rdfBins = 200;
  std::string rearrangePath;
  float rearrangeGap = 0.0f;
  bool rearrangeWindow = false;
  std::string seriesPath;
  float seriesInterval = -1.0f;  // below 0: dump_interval, once the configuration is loaded
  long seriesCapacity = 4096;
  std::string correlatePath;
  int correlateKind = PB_CORR_VELOCITY;
  float correlateRmax = 0.0f;  // 0: 10 * max_radius, once the configuration is loaded
  long correlateBins = 200;
  std::string timecorrPath;
  float timecorrInterval = -1.0f, timecorrOverlap = -1.0f;  // below 0: dump_interval / min_radius, once the configuration is loaded
  long timecorrLags = 32;
  std::string fieldPath;
  long fieldCells = 64;
  float fieldHalf = 0.0f;  // 0: the wall half extent, once the configuration is loaded
  std::string skPath;
  int skKind = PB_SK_DENSITY;
  long skBoxLog2 = 0, skNmax = 16;
  bool skBoxGiven = false;  // else: the smallest box that holds the walls, once the configuration is loaded
  std::string scatterPath;
  float scatterInterval = -1.0f;  // below 0: dump_interval, once the configuration is loaded
  long scatterLags = 32, scatterBoxLog2 = 0, scatterNmax = 3;
  bool scatterBoxGiven = false;  // else: as --sk chooses it
  bool badArg = false;
  double ckptEverySeconds = 0.0;
  long ckptEverySteps = 0, stopAfterSteps = -1;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--set") && i + 2 < argc) {
      sets.emplace_back(argv[i + 1], argv[i + 2]);
      i += 2;
    } else if (!strcmp(argv[i], "--engine") && i + 1 < argc) {
      engine = !strcmp(argv[++i], "legacy") ? Particlebot::Engine::Legacy : Particlebot::Engine::Fused;
    } else if (!strcmp(argv[i], "--quiet")) {
      quiet = true;
    } else if (!strcmp(argv[i], "--overwrite-csv")) {
      overwriteCsv = true;
    } else if (!strcmp(argv[i], "--frames") && i + 1 < argc) {
      framesDir = argv[++i];
    } else if (!strcmp(argv[i], "--frame-size") && i + 1 < argc) {
      frameSize = atoi(argv[++i]);
    } else if (!strcmp(argv[i], "--frame-style") && i + 1 < argc &&
               (!strcmp(argv[i + 1], "plain") || !strcmp(argv[i + 1], "reference"))) {
      referenceFrames = !strcmp(argv[++i], "reference");
    } else if (!strcmp(argv[i], "--frame-render") && i + 1 < argc &&
               (!strcmp(argv[i + 1], "host") || !strcmp(argv[i + 1], "device"))) {
      deviceFrames = !strcmp(argv[++i], "device");
    } else if (!strcmp(argv[i], "--trail") && i + 1 < argc) {
      trailPath = argv[++i];
    } else if (!strcmp(argv[i], "--clusters") && i + 1 < argc) {
      clustersPath = argv[++i];
    } else if (!strcmp(argv[i], "--cluster-gap") && i + 1 < argc) {
      badArg = !parseFloat(argv[++i], 0.0f, false, clusterGap);
    } else if (!strcmp(argv[i], "--contacts") && i + 1 < argc) {
      contactsPath = argv[++i];
    } else if (!strcmp(argv[i], "--contact-gap") && i + 1 < argc) {
      badArg = !parseFloat(argv[++i], 0.0f, false, contactGap);
    } else if (!strcmp(argv[i], "--structure") && i + 1 < argc) {
      structurePath = argv[++i];
    } else if (!strcmp(argv[i], "--structure-gap") && i + 1 < argc) {
      badArg = !parseFloat(argv[++i], 0.0f, false, structureGap);
    } else if (!strcmp(argv[i], "--rdf") && i + 1 < argc) {
      rdfPath = argv[++i];
    } else if (!strcmp(argv[i], "--rdf-rmax") && i + 1 < argc) {
      badArg = !parseFloat(argv[++i], 0.0f, true, rdfRmax);
    } else if (!strcmp(argv[i], "--rdf-bins") && i + 1 < argc) {
      char *end = nullptr;
      rdfBins = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || rdfBins < 1 || rdfBins > (long)PB_RADIAL_MAX_BINS) badArg = true;
    } else if (!strcmp(argv[i], "--rearrange") && i + 1 < argc) {
      rearrangePath = argv[++i];
    } else if (!strcmp(argv[i], "--rearrange-gap") && i + 1 < argc) {
      badArg = !parseFloat(argv[++i], 0.0f, false, rearrangeGap);
    } else if (!strcmp(argv[i], "--rearrange-window")) {
      rearrangeWindow = true;
    } else if (!strcmp(argv[i], "--series") && i + 1 < argc) {
      seriesPath = argv[++i];
    } else if (!strcmp(argv[i], "--series-interval") && i + 1 < argc) {
      badArg = !parseFloat(argv[++i], 0.0f, false, seriesInterval);
    } else if (!strcmp(argv[i], "--series-capacity") && i + 1 < argc) {
      char *end = nullptr;
      seriesCapacity = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || seriesCapacity < 1 || seriesCapacity > (1l << 20)) badArg = true;
    } else if (!strcmp(argv[i], "--correlate") && i + 1 < argc) {
      correlatePath = argv[++i];
    } else if (!strcmp(argv[i], "--correlate-kind") && i + 1 < argc) {
      const char *kind = argv[++i];
      if (!strcmp(kind, "velocity")) correlateKind = PB_CORR_VELOCITY;
      else if (!strcmp(kind, "radius")) correlateKind = PB_CORR_RADIUS;
      else badArg = true;  // (displacement included: the runner holds no mark at the end of a run)
    } else if (!strcmp(argv[i], "--correlate-rmax") && i + 1 < argc) {
      badArg = !parseFloat(argv[++i], 0.0f, true, correlateRmax);
    } else if (!strcmp(argv[i], "--correlate-bins") && i + 1 < argc) {
      char *end = nullptr;
      correlateBins = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || correlateBins < 1 || correlateBins > (long)PB_CORR_MAX_BINS) badArg = true;
    } else if (!strcmp(argv[i], "--timecorr") && i + 1 < argc) {
      timecorrPath = argv[++i];
    } else if (!strcmp(argv[i], "--timecorr-interval") && i + 1 < argc) {
      badArg = !parseFloat(argv[++i], 0.0f, false, timecorrInterval);
    } else if (!strcmp(argv[i], "--timecorr-lags") && i + 1 < argc) {
      char *end = nullptr;
      timecorrLags = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || timecorrLags < 1 || timecorrLags > (long)PB_TCORR_MAX_LAGS) badArg = true;
    } else if (!strcmp(argv[i], "--timecorr-overlap") && i + 1 < argc) {
      badArg = !parseFloat(argv[++i], 0.0f, false, timecorrOverlap) || !(timecorrOverlap < 2048.0f);
    } else if (!strcmp(argv[i], "--field") && i + 1 < argc) {
      fieldPath = argv[++i];
    } else if (!strcmp(argv[i], "--field-cells") && i + 1 < argc) {
      char *end = nullptr;
      fieldCells = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || fieldCells < 1 || fieldCells > (long)PB_FIELD_MAX_AXIS) badArg = true;
    } else if (!strcmp(argv[i], "--field-half") && i + 1 < argc) {
      badArg = !parseFloat(argv[++i], 0.0f, true, fieldHalf);
    } else if (!strcmp(argv[i], "--sk") && i + 1 < argc) {
      skPath = argv[++i];
    } else if (!strcmp(argv[i], "--sk-kind") && i + 1 < argc) {
      const char *kind = argv[++i];
      if (!strcmp(kind, "density")) skKind = PB_SK_DENSITY;
      else if (!strcmp(kind, "radius")) skKind = PB_SK_RADIUS;
      else if (!strcmp(kind, "velocity")) skKind = PB_SK_VELOCITY;
      else badArg = true;
    } else if (!strcmp(argv[i], "--sk-box-log2") && i + 1 < argc) {
      char *end = nullptr;
      skBoxLog2 = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || skBoxLog2 < PB_SK_MIN_LOG2 || skBoxLog2 > PB_SK_MAX_LOG2) badArg = true;
      skBoxGiven = true;
    } else if (!strcmp(argv[i], "--sk-nmax") && i + 1 < argc) {
      char *end = nullptr;
      skNmax = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || skNmax < 1 || skNmax > 44) badArg = true;  // (45: 4140 vectors, past PB_SK_MAX_VECTORS)
    } else if (!strcmp(argv[i], "--scatter") && i + 1 < argc) {
      scatterPath = argv[++i];
    } else if (!strcmp(argv[i], "--scatter-interval") && i + 1 < argc) {
      badArg = !parseFloat(argv[++i], 0.0f, false, scatterInterval);
    } else if (!strcmp(argv[i], "--scatter-lags") && i + 1 < argc) {
      char *end = nullptr;
      scatterLags = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || scatterLags < 1 || scatterLags > (long)PB_SCATTER_MAX_LAGS) badArg = true;
    } else if (!strcmp(argv[i], "--scatter-box-log2") && i + 1 < argc) {
      char *end = nullptr;
      scatterBoxLog2 = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || scatterBoxLog2 < PB_SK_MIN_LOG2 || scatterBoxLog2 > PB_SK_MAX_LOG2) badArg = true;
      scatterBoxGiven = true;
    } else if (!strcmp(argv[i], "--scatter-nmax") && i + 1 < argc) {
      char *end = nullptr;
      scatterNmax = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || scatterNmax < 1 || scatterNmax > 10) badArg = true;  // (11: 264 vectors, past PB_SCATTER_MAX_VECTORS)
    } else if (!strcmp(argv[i], "--resume") && i + 1 < argc) {
      resumePath = argv[++i];
    } else if (!strcmp(argv[i], "--checkpoint") && i + 1 < argc) {
      ckptPath = argv[++i];
    } else if (!strcmp(argv[i], "--final-checkpoint") && i + 1 < argc) {
      finalCkptPath = argv[++i];
    } else if (!strcmp(argv[i], "--checkpoint-every") && i + 1 < argc) {
      ckptEverySeconds = atof(argv[++i]);
    } else if (!strcmp(argv[i], "--checkpoint-steps") && i + 1 < argc) {
      ckptEverySteps = atol(argv[++i]);
    } else if (!strcmp(argv[i], "--stop-after-steps") && i + 1 < argc) {
      stopAfterSteps = atol(argv[++i]);  // (tests: die like a killed process once this many steps have run)
    } else if (argv[i][0] != '-') {
      path = argv[i];
    } else {
      badArg = true;
    }
    if (badArg) {
      fprintf(stderr,
              "usage: %s [config.cfg] [--set NAME VALUE]... [--engine fused|legacy] [--quiet] "
              "[--frames DIR [--frame-size PIXELS] [--frame-style plain|reference] [--frame-render host|device]] [--trail FILE] [--clusters FILE [--cluster-gap G]] [--contacts FILE [--contact-gap G]] "
              "[--structure FILE [--structure-gap G]] [--rdf FILE [--rdf-rmax R] [--rdf-bins B]] [--rearrange FILE [--rearrange-gap G] [--rearrange-window]] [--resume FILE [--overwrite-csv]] [--checkpoint FILE "
              "[--checkpoint-every SECONDS] [--checkpoint-steps N]] [--final-checkpoint FILE]\n",
              argv[0]);
      return 2;
    }
  }
  const struct { const char *flag; const std::string &path; const char *noun; } fusedOnly[] = {
      {"--clusters", clustersPath, "analysis"},   {"--contacts", contactsPath, "export"},
      {"--structure", structurePath, "analysis"}, {"--rdf", rdfPath, "analysis"},
      {"--rearrange", rearrangePath, "analysis"}, {"--series", seriesPath, "recorder"},
      {"--correlate", correlatePath, "analysis"}, {"--timecorr", timecorrPath, "recorder"},
      {"--field", fieldPath, "analysis"},         {"--sk", skPath, "analysis"},
      {"--scatter", scatterPath, "recorder"}};
  for (const auto &f : fusedOnly)
    if (!f.path.empty() && engine != Particlebot::Engine::Fused) {
      fprintf(stderr, "%s needs the fused engine (the %s runs on its resident state)\n", f.flag, f.noun);
      return 2;
    }
  if (!cfg.loadFile(path)) fprintf(stderr, "warning: cannot open %s, running on defaults\n", path.c_str());
  for (auto &kv : sets) cfg.setParam(kv.first, kv.second);
  srand(cfg.params.seed);  // main.cpp:929 (the class itself draws from a private, identical stream)
  cfg.derive();

  // resuming from an exact checkpoint keeps the CSV written so far (cut back to the length it had when the
  // checkpoint was taken); every other start truncates it, as the reference's fopen("w+") does (main.cpp:944)
  RunTrailer trailer;
  const bool exactResume = !resumePath.empty() && isExactCheckpoint(resumePath);
  if (exactResume && !readTrailer(resumePath, trailer)) {
    fprintf(stderr, "%s: not a checkpoint written by particlebot_run --checkpoint\n", resumePath.c_str());
    return 1;
  }
  if (quiet) {
    // dumpParticlebot echoes "time cx cy" per row to stdout, as the reference does
    if (!freopen("/dev/null", "w", stdout)) return 1;
  }
  Particlebot sim(cfg.params, engine, cfg.wallHalf());
  sim.setExitOnMaxTime(false);
  sim.setHexSpacing(cfg.hex_spacing);
  sim.setSquareLattice(cfg.square_lattice);
  sim.setFastBlob(cfg.fast_blob);
  sim.setRng(cfg.rng_kind);
  sim.setForceVariant(cfg.force_variant);
  if (!trailPath.empty() || referenceFrames) sim.setDisplay(true);
  sim.reset();
  const SimParams &p = sim.getParams();
  const int frameEvery = cfg.video_interval > 0 ? cfg.video_interval : 100;
  long stepsDone = 0, frames = 0;
  if (!resumePath.empty()) {
    FILE *rf = fopen(resumePath.c_str(), exactResume ? "rb" : "r");
    if (!rf) {
      fprintf(stderr, "cannot open %s\n", resumePath.c_str());
      return 1;
    }
    if (exactResume) {
      if (!sim.loadCheckpoint(rf)) {
        fprintf(stderr, "%s does not match this configuration (bot count?) or is damaged\n", resumePath.c_str());
        return 1;
      }
      stepsDone = trailer.stepsDone;
      frames = trailer.frames;
    } else {
      sim.loadFromFile(0, p.nCells, rf, cfg.dump_interval);  // main.cpp:954-957
    }
    fclose(rf);
  }
  // the CSV: truncated on a fresh start (main.cpp:944); appended to when the run continues from its own last row
  // (main.cpp:940-956); cut back to the length the checkpoint recorded on an exact resume
  // "Its own": the SAME FILE, however it is spelled (./run.csv, an absolute path, a symlink) -- decided by device and
  // inode, not by comparing strings; a resume from ANOTHER CSV never truncates an existing csv_filename silently
  // (`--resume ./run.csv` with csv_filename run.csv destroyed every earlier row of the run).
  bool csvResumeInPlace = false;
  if (!resumePath.empty() && !exactResume) {
    struct stat a, b;
    const bool haveA = stat(resumePath.c_str(), &a) == 0, haveB = stat(cfg.csv_filename.c_str(), &b) == 0;
    csvResumeInPlace = haveA && haveB && a.st_dev == b.st_dev && a.st_ino == b.st_ino;
    if (!csvResumeInPlace && haveB && b.st_size > 0 && !overwriteCsv) {
      fprintf(stderr,
              "%s exists and is not the file being resumed (%s): refusing to truncate it; pass --overwrite-csv or "
              "choose another csv_filename\n",
              cfg.csv_filename.c_str(), resumePath.c_str());
      return 1;
    }
  }
  FILE *fp = fopen(cfg.csv_filename.c_str(), exactResume ? "r+" : csvResumeInPlace ? "a" : "w+");
  if (!fp) {
    fprintf(stderr, "cannot open %s\n", cfg.csv_filename.c_str());
    return 1;
  }
  if (exactResume) {
    if (ftruncate(fileno(fp), (off_t)trailer.csvBytes) != 0 || fseek(fp, 0, SEEK_END) != 0) {
      fprintf(stderr, "cannot cut %s back to %lld bytes\n", cfg.csv_filename.c_str(), trailer.csvBytes);
      return 1;
    }
  }
  auto writeCheckpoint = [&](const std::string &dest) {
    // the CSV first: the checkpoint records how long it is
    fflush(fp);
    RunTrailer t;
    t.csvBytes = (long long)ftell(fp);
    t.stepsDone = stepsDone;
    t.frames = frames;
    const std::string tmp = dest + ".tmp";
    FILE *cf = fopen(tmp.c_str(), "wb");
    bool ok = cf && sim.saveCheckpoint(cf) && fwrite(&t, sizeof t, 1, cf) == 1;
    if (cf) ok = (fclose(cf) == 0) && ok;
    if (!ok || rename(tmp.c_str(), dest.c_str()) != 0) {
      fprintf(stderr, "cannot write checkpoint %s\n", dest.c_str());
      return false;
    }
    return true;
  };
  auto lastCkptWall = std::chrono::steady_clock::now();
  long lastCkptStep = stepsDone;
  bool referenceMarked = false;
  float markTime = 0.0f;
  std::vector<int> skVectors;  // --sk: the (nx, ny) pairs, made at the first dump time
  // the time series: switched on here, behind a resume, so that the records start at the run's first step; drained at
  // every host stop below
  unsigned long long seriesWritten = 0;
  if (!seriesPath.empty()) {
    if (!sim.setSeries(seriesInterval < 0.0f ? cfg.dump_interval : seriesInterval, (unsigned)seriesCapacity)) return 1;
    FILE *sf = openOutput(seriesPath, resumePath.empty() ? "w" : "a");
    if (!sf) return 1;
    if (fseek(sf, 0, SEEK_END) == 0 && ftell(sf) == 0)  // a fresh file, or a resumed run that appends to none
      fprintf(sf, "Time, Step, Measured, SumQx, SumQy, MinQx, MaxQx, MinQy, MaxQy, SumXX, SumYY, SumXY, SumQr, SumRR, "
                  "SumWx, SumWy, SumVV\n");
    if (fclose(sf) != 0) return 1;
  }
  // the time correlations: switched on here too; their table stays on the device until the run ends, so a run whose
  // lag 0 would pass the 2^31 samples that the engine's exact sums hold is refused now, not after its last step
  if (!timecorrPath.empty()) {
    const float every = timecorrInterval < 0.0f ? cfg.dump_interval : timecorrInterval;
    const double left = std::max(0.0, (double)p.max_time - (double)sim.getTime());
    const double records = left / (double)(every > 0.0f ? every : cfg.timestep) + 2.0;  // (the gate's rounding: at most one more)
    if (!(records * (double)p.nCells < 2147483648.0)) {
      fprintf(stderr, "--timecorr: about %.0f records of %u bots would pass 2^31 samples per lag: raise --timecorr-interval "
                      "or lower max_time\n", records, (unsigned)p.nCells);
      return 2;
    }
    if (!sim.setTimeCorrelation(every, (unsigned)timecorrLags, timecorrOverlap < 0.0f ? p.min_radius : timecorrOverlap))
      return 1;
  }
  // the scattering function: switched on here as well, and refused by the same count
  if (!scatterPath.empty()) {
    const float every = scatterInterval < 0.0f ? cfg.dump_interval : scatterInterval;
    const double left = std::max(0.0, (double)p.max_time - (double)sim.getTime());
    const double records = left / (double)(every > 0.0f ? every : cfg.timestep) + 2.0;  // (the gate's rounding: at most one more)
    if (!(records * (double)p.nCells < 2147483648.0)) {
      fprintf(stderr, "--scatter: about %.0f records of %u bots would pass 2^31 samples per lag: raise --scatter-interval "
                      "or lower max_time\n", records, (unsigned)p.nCells);
      return 2;
    }
    std::vector<int> vectors;  // the half plane ny > 0 || (ny == 0 && nx > 0), as --sk lists it
    for (int nx = 1; nx <= (int)scatterNmax; nx++) vectors.push_back(nx), vectors.push_back(0);
    for (int ny = 1; ny <= (int)scatterNmax; ny++)
      for (int nx = -(int)scatterNmax; nx <= (int)scatterNmax; nx++) vectors.push_back(nx), vectors.push_back(ny);
    if (!scatterBoxGiven) {
      scatterBoxLog2 = PB_SK_MIN_LOG2;
      while (scatterBoxLog2 < PB_SK_MAX_LOG2 && std::ldexp(1.0, (int)scatterBoxLog2) < 2.0 * (double)cfg.wallHalf())
        scatterBoxLog2++;
    }
    if (!sim.setScattering(every, (unsigned)scatterLags, (int)scatterBoxLog2, vectors)) return 1;
  }
  auto drainSeries = [&]() {
    if (seriesPath.empty()) return true;
    std::vector<pbMomentsRow> rows;
    if (!sim.seriesRows(seriesWritten, rows)) return false;
    if (rows.empty()) return true;
    FILE *sf = openOutput(seriesPath, "a");
    if (!sf) return false;
    for (const pbMomentsRow &r : rows)
      fprintf(sf, "%.9g, %llu, %u, %lld, %lld, %d, %d, %d, %d, %s, %s, %s, %lld, %s, %lld, %lld, %s\n", (double)r.time,
              r.step, r.measured, r.sum_qx, r.sum_qy, r.min_qx, r.max_qx, r.min_qy, r.max_qy, decimal128(r.xx).c_str(),
              decimal128(r.yy).c_str(), decimal128(r.xy).c_str(), r.sum_qr, decimal128(r.rr).c_str(), r.sum_wx, r.sum_wy,
              decimal128(r.vv).c_str());
    seriesWritten += rows.size();
    return fclose(sf) == 0;
  };
  for (;;) {
    // a checkpoint is taken here, where the loop is about to dump: resuming re-enters at this very point
    if (!ckptPath.empty() && stepsDone > lastCkptStep) {
      const double since = std::chrono::duration<double>(std::chrono::steady_clock::now() - lastCkptWall).count();
      if ((ckptEverySteps > 0 && stepsDone - lastCkptStep >= ckptEverySteps) ||
          (ckptEverySeconds > 0 && since >= ckptEverySeconds)) {
        if (!writeCheckpoint(ckptPath)) return 1;
        lastCkptWall = std::chrono::steady_clock::now();
        lastCkptStep = stepsDone;
      }
    }
    if (stopAfterSteps >= 0 && stepsDone >= stopAfterSteps) _exit(9);  // (no flush, no destructors: a kill)
    sim.dumpParticlebot(0, p.nCells, fp, cfg.dump_interval, p.testing, p.light_x, p.light_y);
    if (!drainSeries()) return 1;
    if (!clustersPath.empty() && sim.dumpDue(cfg.dump_interval)) {
      pbClusterStats cs;
      if (!sim.clusterStats(clusterGap, cs)) return 1;
      FILE *cf = openOutput(clustersPath, sim.getTime() == 0.0f ? "w" : "a");
      if (!cf) return 1;
      if (sim.getTime() == 0.0f) fprintf(cf, "Time, Clusters, Largest, Isolated, Links, MaxDegree\n");
      fprintf(cf, "%f, %u, %u, %u, %llu, %u\n", sim.getTime(), cs.clusters, cs.largest, cs.isolated, cs.links,
              cs.max_degree);
      if (fclose(cf) != 0) return 1;
    }
    if (!structurePath.empty() && sim.dumpDue(cfg.dump_interval)) {
      pbStructureStats ss;
      if (!sim.structureStats(structureGap, ss)) return 1;
      FILE *sf = openOutput(structurePath, sim.getTime() == 0.0f ? "w" : "a");
      if (!sf) return 1;
      if (sim.getTime() == 0.0f) fprintf(sf, "Time, Bonds, Psi6Re, Psi6Im, C0, C1, C2, C3, C4, C5, C6, C7\n");
      fprintf(sf, "%f, %llu, %lld, %lld", sim.getTime(), ss.bonds, ss.psi6_re, ss.psi6_im);
      for (int k = 0; k < 8; k++) fprintf(sf, ", %u", ss.coordination[k]);
      fprintf(sf, "\n");
      if (fclose(sf) != 0) return 1;
    }
    if (!fieldPath.empty() && sim.dumpDue(cfg.dump_interval)) {
      pbFieldView view;
      view.nx = view.ny = (unsigned)fieldCells;
      view.centerX = view.centerY = 0.0f;
      view.halfX = view.halfY = fieldHalf > 0.0f ? fieldHalf : cfg.wallHalf();
      std::vector<pbFieldCell> cells;
      pbFieldTotals tot;
      if (!sim.fieldMap(view, cells, tot)) return 1;
      FILE *ff = openOutput(fieldPath, sim.getTime() == 0.0f ? "w" : "a");
      if (!ff) return 1;
      if (fseek(ff, 0, SEEK_END) == 0 && ftell(ff) == 0)  // a fresh file, or a resumed run that appends to none
        fprintf(ff, "time,step,ix,iy,count,dead,sum_qr,sum_wx,sum_wy,rr,vv\n");
      for (size_t k = 0; k < cells.size(); k++) {
        const pbFieldCell &c = cells[k];
        if (!c.count) continue;
        fprintf(ff, "%.9g,%ld,%zu,%zu,%u,%u,%lld,%lld,%lld,%s,%s\n", (double)sim.getTime(), stepsDone, k % view.nx,
                k / view.nx, c.count, c.dead, c.sum_qr, c.sum_wx, c.sum_wy, decimal128(c.rr).c_str(),
                decimal128(c.vv).c_str());
      }
      if (fclose(ff) != 0) return 1;
    }
    if (!skPath.empty() && sim.dumpDue(cfg.dump_interval)) {
      if (skVectors.empty()) {  // the run's first dump time: the half plane ny > 0 || (ny == 0 && nx > 0), and the box
        for (int nx = 1; nx <= (int)skNmax; nx++) skVectors.push_back(nx), skVectors.push_back(0);
        for (int ny = 1; ny <= (int)skNmax; ny++)
          for (int nx = -(int)skNmax; nx <= (int)skNmax; nx++) skVectors.push_back(nx), skVectors.push_back(ny);
        if (!skBoxGiven) {
          skBoxLog2 = PB_SK_MIN_LOG2;
          while (skBoxLog2 < PB_SK_MAX_LOG2 && std::ldexp(1.0, (int)skBoxLog2) < 2.0 * (double)cfg.wallHalf()) skBoxLog2++;
        }
      }
      std::vector<pbStructureFactorRow> rows;
      if (!sim.structureFactor(skKind, (int)skBoxLog2, skVectors, rows)) return 1;
      FILE *kf = openOutput(skPath, sim.getTime() == 0.0f ? "w" : "a");
      if (!kf) return 1;
      static const char *const kinds[] = {"density", "radius", "velocity"};
      fprintf(kf, "time,%.9g,step,%ld,kind,%s,box_log2,%ld,vectors,%zu\n", (double)sim.getTime(), stepsDone, kinds[skKind],
              skBoxLog2, rows.size());
      for (const pbStructureFactorRow &r : rows)
        fprintf(kf, "%d,%d,%u,%s,%s,%s,%s\n", r.nx, r.ny, r.measured, decimal128(r.re).c_str(), decimal128(r.im).c_str(),
                decimal128(r.re2).c_str(), decimal128(r.im2).c_str());
      if (fclose(kf) != 0) return 1;
    }
    if (!rearrangePath.empty() && sim.dumpDue(cfg.dump_interval)) {
      if (!referenceMarked) {  // the run's first dump time
        if (!sim.markReference(rearrangeGap)) return 1;
        referenceMarked = true;
        markTime = sim.getTime();
      }
      pbRearrangementStats rs;
      if (!sim.rearrangementStats(rs)) return 1;
      FILE *af = openOutput(rearrangePath, sim.getTime() == 0.0f ? "w" : "a");
      if (!af) return 1;
      if (fseek(af, 0, SEEK_END) == 0 && ftell(af) == 0)  // a fresh file, or a resumed run that appends to none
        fprintf(af, "Time, MarkTime, BondsMarked, BondsNow, BondsKept, Unchanged, Lost, Gained, Measured, SumQx, SumQy, "
                    "SumQ2, MaxQ2\n");
      fprintf(af, "%f, %f, %llu, %llu, %llu, %u, %u, %u, %u, %lld, %lld, %s, %llu\n", sim.getTime(), markTime,
              rs.bonds_marked, rs.bonds_now, rs.bonds_kept, rs.bots_unchanged, rs.bots_lost, rs.bots_gained, rs.measured,
              rs.sum_qx, rs.sum_qy, decimal128(rs.sum_q2_hi, rs.sum_q2_lo).c_str(), rs.max_q2);
      if (fclose(af) != 0) return 1;
      if (rearrangeWindow) {  // the next row describes the interval that starts here
        if (!sim.markReference(rearrangeGap)) return 1;
        markTime = sim.getTime();
      }
    }
    if (!framesDir.empty() && stepsDone % frameEvery == 0) {
      char name[64];
      snprintf(name, sizeof name, "/frame_%06ld.ppm", frames++);
      const std::string fpath = framesDir + name;
      const float half = cfg.camera_y * 0.57735027f;
      if (deviceFrames) {
        if (!sim.writeFramePPMDevice(fpath.c_str(), frameSize, frameSize, cfg.camera_x, 0.0f, half, cfg.light_radius,
                                     referenceFrames)) {
          fprintf(stderr, "cannot write %s%s\n", framesDir.c_str(), name);
          return 1;
        }
      } else if (!(referenceFrames ? sim.writeFramePPMReference(fpath.c_str(), frameSize, frameSize, cfg.camera_x, 0.0f, half,
                                                         cfg.light_radius)
                            : sim.writeFramePPM(fpath.c_str(), frameSize, frameSize, cfg.camera_x, 0.0f, half,
                                                cfg.light_radius))) {
        fprintf(stderr, "cannot write %s%s\n", framesDir.c_str(), name);
        return 1;
      }
    }
    if (sim.finished()) break;  // the reference exits from inside update() here
    int batch = sim.stepsUntilHostEvent(cfg.timestep, cfg.dump_interval, 1 << 20);
    if (!framesDir.empty()) batch = (int)std::min<long>(batch, frameEvery - stepsDone % frameEvery);
    if (ckptEverySteps > 0) batch = (int)std::min<long>(batch, ckptEverySteps - (stepsDone - lastCkptStep) > 0
                                                                   ? ckptEverySteps - (stepsDone - lastCkptStep)
                                                                   : 1);
    else if (ckptEverySeconds > 0) batch = std::min(batch, 20000);  // look at the clock now and then
    if (!seriesPath.empty()) batch = (int)std::min<long>(batch, seriesCapacity);  // records <= steps: none is lost
    const int ran = sim.advance(cfg.timestep, cfg.sort_interval, batch);
    if (ran == 0) break;
    stepsDone += ran;
  }
  if (!drainSeries()) return 1;
  if (!finalCkptPath.empty() && !writeCheckpoint(finalCkptPath)) return 1;
  fclose(fp);
  if (!trailPath.empty()) {
    std::vector<float> xy, times;
    unsigned records = 0;
    FILE *tf = fopen(trailPath.c_str(), "w");
    if (!tf || !sim.getCentroidTrail(xy, times, records)) {
      fprintf(stderr, "cannot write %s\n", trailPath.c_str());
      if (tf) fclose(tf);
      return 1;
    }
    fprintf(tf, "slot,time,x,y\n");
    for (size_t k = 0; k < times.size(); k++)
      if (!std::isnan(times[k]))  // a slot that holds a record
        fprintf(tf, "%zu,%.9g,%.9g,%.17g\n", k, (double)times[k], (double)xy[2 * k], (double)xy[2 * k + 1] - 2000.0);
    if (fclose(tf) != 0) return 1;
  }
  if (!contactsPath.empty()) {
    std::vector<unsigned> offsets;
    std::vector<pbContactLink> links;
    if (!sim.contacts(contactGap, offsets, links)) return 1;
    FILE *cf = openOutput(contactsPath, "w");
    if (!cf) return 1;
    fprintf(cf, "I, J, Gap, Fx, Fy\n");
    for (size_t i = 0; i + 1 < offsets.size(); i++)
      for (unsigned k = offsets[i]; k < offsets[i + 1]; k++)
        fprintf(cf, "%zu, %u, %.9g, %.9g, %.9g\n", i, links[k].other, (double)links[k].gap, (double)links[k].fx,
                (double)links[k].fy);
    if (fclose(cf) != 0) return 1;
  }
  if (!rdfPath.empty()) {
    const float rmax = rdfRmax > 0.0f ? rdfRmax : 10.0f * p.max_radius;
    std::vector<unsigned long long> counts;
    if (!sim.radialCounts(rmax, (unsigned)rdfBins, counts)) return 1;
    FILE *rf = openOutput(rdfPath, "w");
    if (!rf) return 1;
    fprintf(rf, "RLo, RHi, Count\n");
    for (size_t b = 0; b < counts.size(); b++)
      fprintf(rf, "%.9g, %.9g, %llu\n", (double)b * (double)rmax / (double)rdfBins,
              (double)(b + 1) * (double)rmax / (double)rdfBins, counts[b]);
    if (fclose(rf) != 0) return 1;
  }
  if (!timecorrPath.empty()) {
    std::vector<pbTimeCorrelationRow> rows;
    if (!sim.timeCorrelationRows(rows)) return 1;
    FILE *tf = openOutput(timecorrPath, "w");
    if (!tf) return 1;
    fprintf(tf, "Lag, Origins, SumSteps, Samples, SumQx, SumQy, SumQ2, SumWW, Overlap, MaxQ2\n");
    for (const pbTimeCorrelationRow &r : rows)
      fprintf(tf, "%u, %llu, %llu, %llu, %lld, %lld, %s, %s, %llu, %llu\n", r.lag, r.origins, r.sum_steps, r.samples,
              r.sum_qx, r.sum_qy, decimal128(r.msd).c_str(), decimal128(r.vacf).c_str(), r.overlap, r.max_q2);
    if (fclose(tf) != 0) return 1;
  }
  if (!scatterPath.empty()) {
    std::vector<pbScatteringRow> rows;
    if (!sim.scatteringRows(rows)) return 1;
    FILE *kf = openOutput(scatterPath, "w");
    if (!kf) return 1;
    fprintf(kf, "Lag, Nx, Ny, Origins, SumSteps, Samples, Re, Im, FsRe, FsIm\n");
    for (const pbScatteringRow &r : rows) {
      const long double unit = 1073741824.0L * (long double)r.samples;  // (both operands are exact in a long double)
      const double fsRe = r.samples ? (double)((long double)r.re / unit) : std::nan("");
      const double fsIm = r.samples ? (double)((long double)r.im / unit) : std::nan("");
      fprintf(kf, "%u, %d, %d, %llu, %llu, %llu, %lld, %lld, %.9g, %.9g\n", r.lag, r.nx, r.ny, r.origins, r.sum_steps,
              r.samples, r.re, r.im, fsRe, fsIm);
    }
    if (fclose(kf) != 0) return 1;
  }
  if (!correlatePath.empty()) {
    const float rmax = correlateRmax > 0.0f ? correlateRmax : 10.0f * p.max_radius;
    std::vector<pbCorrelationBin> rows;
    pbCorrelationTotals tot;
    if (!sim.pairCorrelation(correlateKind, rmax, (unsigned)correlateBins, rows, tot)) return 1;
    FILE *kf = openOutput(correlatePath, "w");
    if (!kf) return 1;
    fprintf(kf, "Kind, %s, Measured, %u, SumAx, %lld, SumAy, %lld, SumA2, %s, Pairs, %llu\n",
            correlateKind == PB_CORR_RADIUS ? "radius" : "velocity", tot.measured, tot.sum_ax, tot.sum_ay,
            decimal128(tot.sum_a2).c_str(), tot.pairs);
    fprintf(kf, "RLo, RHi, Pairs, Dot, SumAx, SumAy\n");
    for (size_t b = 0; b < rows.size(); b++)
      fprintf(kf, "%.9g, %.9g, %llu, %s, %s, %s\n", (double)b * (double)rmax / (double)correlateBins,
              (double)(b + 1) * (double)rmax / (double)correlateBins, rows[b].pairs, decimal128(rows[b].dot).c_str(),
              decimal128(rows[b].ax).c_str(), decimal128(rows[b].ay).c_str());
    if (fclose(kf) != 0) return 1;
  }
  return 0;
}
