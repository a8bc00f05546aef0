// pb_runner.cpp -- headless replacement for the reference's GLUT main loop.
//
//   particlebot_run [config.cfg] [--set NAME VALUE]... [--engine fused|legacy] [--quiet]
//                   [--frames DIR [--frame-size PIXELS] [--frame-style plain|reference] [--frame-render host|device]]
//                   [--trail FILE] [--clusters FILE [--cluster-gap G]] [--contacts FILE [--contact-gap G]]
//                   [--structure FILE [--structure-gap G]] [--rdf FILE [--rdf-rmax R] [--rdf-bins B]]
//                   [--rearrange FILE [--rearrange-gap G] [--rearrange-window]]
//                   [--strain FILE [--strain-threshold T] [--rearrange-gap G] [--rearrange-window]]
//                   [--series FILE [--series-interval T] [--series-capacity N]]
//                   [--correlate FILE [--correlate-kind velocity|radius] [--correlate-rmax R] [--correlate-bins B]]
//                   [--timecorr FILE [--timecorr-interval T] [--timecorr-lags N] [--timecorr-overlap A]]
//                   [--field FILE [--field-cells N] [--field-half H]]
//                   [--sk FILE [--sk-kind density|radius|velocity] [--sk-box-log2 E] [--sk-nmax M]]
//                   [--scatter FILE [--scatter-interval T] [--scatter-lags N] [--scatter-box-log2 E] [--scatter-nmax M]]
//                   [--vanhove FILE [--vanhove-interval T] [--vanhove-lags N] [--vanhove-width W] [--vanhove-bins B]]
//                   [--vanhove-distinct FILE [--vanhove-distinct-interval T] [--vanhove-distinct-lags N]
//                    [--vanhove-distinct-width W] [--vanhove-distinct-bins B]]
//                   [--coherent FILE [--coherent-interval T] [--coherent-lags N] [--coherent-box-log2 E] [--coherent-nmax M]]
//                   [--fourpoint FILE [--fourpoint-interval T] [--fourpoint-lags N] [--fourpoint-overlap A]
//                    [--fourpoint-box-log2 E] [--fourpoint-nmax M]]
//                   [--bonds FILE [--bonds-interval T] [--bonds-lags N] [--bonds-gap G] [--bonds-max-radius R]
//                    [--bonds-overlap A]]
//                   [--resume FILE [--overwrite-csv]] [--checkpoint FILE [--checkpoint-every SECONDS] [--checkpoint-steps N]]
//                   [--final-checkpoint FILE]
//
// The file reads top down: RunOptions and the flag table (what every flag takes), one writer or group of writers per
// output (what its file holds and when it is written), then main(): the reference's loop, which calls them.
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

// ---------------------------------------------------------------------------------------------------------------------
// The command line.  A value below a flag's range stands for "the default that needs the configuration": it is chosen
// once the .cfg file is loaded, by the writer that uses it.
struct RunOptions {
  std::string configPath = "example.cfg";
  std::vector<std::pair<std::string, std::string>> sets;
  Particlebot::Engine engine = Particlebot::Engine::Fused;
  bool quiet = false, overwriteCsv = false;
  std::string resumePath, ckptPath, finalCkptPath;
  double ckptEverySeconds = 0.0;
  long ckptEverySteps = 0, stopAfterSteps = -1;

  std::string framesDir;
  int frameSize = 800;
  int referenceFrames = 0, deviceFrames = 0;  // (ints: a choice's destination)
  std::string trailPath;

  std::string clustersPath, contactsPath, structurePath, rearrangePath;
  float clusterGap = 0.0f, contactGap = 0.0f, structureGap = 0.0f, rearrangeGap = 0.0f;
  bool rearrangeWindow = false;
  std::string strainPath;  // measured against --rearrange's mark, with or without --rearrange itself
  float strainThreshold = 0.0f;

  std::string rdfPath, correlatePath;
  float rdfRmax = 0.0f, correlateRmax = 0.0f;  // 0: 10 * max_radius
  long rdfBins = 200, correlateBins = 200;
  int correlateKind = PB_CORR_VELOCITY;

  std::string seriesPath, timecorrPath, scatterPath;
  float seriesInterval = -1.0f, timecorrInterval = -1.0f, scatterInterval = -1.0f;  // below 0: dump_interval
  long seriesCapacity = 4096, timecorrLags = 32, scatterLags = 32;
  float timecorrOverlap = -1.0f;  // below 0: min_radius (a default and not a claim)

  std::string fieldPath;
  long fieldCells = 64;
  float fieldHalf = 0.0f;  // 0: the wall half extent

  std::string skPath;
  int skKind = PB_SK_DENSITY;
  long skBoxLog2 = PB_SK_MIN_LOG2 - 1, scatterBoxLog2 = PB_SK_MIN_LOG2 - 1;  // below the range: boxLog2() chooses
  long skNmax = 16, scatterNmax = 3;  // 544 and 24 wavevectors

  std::string vanhovePath;
  float vanhoveInterval = -1.0f;  // below 0: dump_interval
  float vanhoveWidth = -1.0f;     // below 0: an eighth of min_radius (a default and not a claim)
  long vanhoveLags = 32, vanhoveBins = 64;

  std::string vanhoveDistinctPath;
  float vanhoveDistinctInterval = -1.0f;  // below 0: dump_interval
  float vanhoveDistinctWidth = -1.0f;     // below 0: an eighth of min_radius, at most 2047 / bins
  long vanhoveDistinctLags = 32, vanhoveDistinctBins = 64;

  std::string coherentPath;
  float coherentInterval = -1.0f;                // below 0: dump_interval
  long coherentLags = 32, coherentNmax = 3;      // 24 wavevectors, as --scatter
  long coherentBoxLog2 = PB_SK_MIN_LOG2 - 1;     // below the range: boxLog2() chooses

  std::string fourpointPath;
  float fourpointInterval = -1.0f;               // below 0: dump_interval
  float fourpointOverlap = -1.0f;                // below 0: min_radius, as --timecorr-overlap
  long fourpointLags = 32, fourpointNmax = 3;    // 24 wavevectors and (0, 0)
  long fourpointBoxLog2 = PB_SK_MIN_LOG2 - 1;    // below the range: boxLog2() chooses

  std::string bondsPath;
  float bondsInterval = -1.0f;                   // below 0: dump_interval
  float bondsGap = 0.0f;
  float bondsMaxRadius = 0.0f;                   // 0: max_radius of the cfg
  float bondsOverlap = -1.0f;                    // below 0: min_radius, as --timecorr-overlap
  long bondsLags = 32;
};

using Choice = std::pair<const char *, int>;  // a word and what it stands for

// One flag: its name and where its value goes, with the bounds or choices that hold for it.  A row sets one
// destination, and the destination's type is the flag's kind; a row that sets none is an oddity that parseOdd() knows.
struct Flag {
  const char *name;
  int values = 1;  // the arguments that follow it
  std::string RunOptions::*path = nullptr;
  const char *noun = nullptr;  // an output that needs the fused engine: what the engine check calls its producer
  bool RunOptions::*on = nullptr;
  float RunOptions::*real = nullptr;  // finite, >= lowest (> lowest when `above`) and < below
  float lowest = 0.0f, below = INFINITY;
  bool above = false;
  long RunOptions::*whole = nullptr;  // lo ... hi
  long lo = 0, hi = 0;
  int RunOptions::*pick = nullptr;
  std::vector<Choice> choices;

  Flag(const char *n, int values_) : name(n), values(values_) {}
  Flag(const char *n, std::string RunOptions::*to, const char *noun_ = nullptr) : name(n), path(to), noun(noun_) {}
  Flag(const char *n, bool RunOptions::*to) : name(n), values(0), on(to) {}
  Flag(const char *n, float RunOptions::*to, float lowest_, bool above_, float below_ = INFINITY)
      : name(n), real(to), lowest(lowest_), below(below_), above(above_) {}
  Flag(const char *n, long RunOptions::*to, long lo_, long hi_) : name(n), whole(to), lo(lo_), hi(hi_) {}
  Flag(const char *n, int RunOptions::*to, std::vector<Choice> words) : name(n), pick(to), choices(std::move(words)) {}
};

// Every flag.  The outputs that need the fused engine stand in the order in which the engine check speaks for them.
const Flag kFlags[] = {
    {"--set", 2},
    {"--engine", 1},  // fused for anything but `legacy`
    {"--quiet", &RunOptions::quiet},
    {"--resume", &RunOptions::resumePath},
    {"--overwrite-csv", &RunOptions::overwriteCsv},
    {"--checkpoint", &RunOptions::ckptPath},
    {"--final-checkpoint", &RunOptions::finalCkptPath},
    {"--checkpoint-every", 1},
    {"--checkpoint-steps", 1},
    {"--stop-after-steps", 1},  // (tests: die like a killed process once this many steps have run)

    {"--frames", &RunOptions::framesDir},
    {"--frame-size", 1},
    {"--frame-style", &RunOptions::referenceFrames, {{"plain", 0}, {"reference", 1}}},
    {"--frame-render", &RunOptions::deviceFrames, {{"host", 0}, {"device", 1}}},
    {"--trail", &RunOptions::trailPath},

    // the link gaps: the analysis' linkGap, default 0
    {"--clusters", &RunOptions::clustersPath, "analysis"},
    {"--cluster-gap", &RunOptions::clusterGap, 0.0f, false},
    {"--contacts", &RunOptions::contactsPath, "export"},
    {"--contact-gap", &RunOptions::contactGap, 0.0f, false},
    {"--structure", &RunOptions::structurePath, "analysis"},
    {"--structure-gap", &RunOptions::structureGap, 0.0f, false},

    {"--rdf", &RunOptions::rdfPath, "analysis"},
    {"--rdf-rmax", &RunOptions::rdfRmax, 0.0f, true},
    {"--rdf-bins", &RunOptions::rdfBins, 1, PB_RADIAL_MAX_BINS},

    {"--rearrange", &RunOptions::rearrangePath, "analysis"},
    {"--rearrange-gap", &RunOptions::rearrangeGap, 0.0f, false},
    {"--rearrange-window", &RunOptions::rearrangeWindow},
    {"--strain", &RunOptions::strainPath, "analysis"},
    {"--strain-threshold", &RunOptions::strainThreshold, 0.0f, false},

    // an interval of 0: a record in front of every step
    {"--series", &RunOptions::seriesPath, "recorder"},
    {"--series-interval", &RunOptions::seriesInterval, 0.0f, false},
    {"--series-capacity", &RunOptions::seriesCapacity, 1, 1l << 20},

    {"--correlate", &RunOptions::correlatePath, "analysis"},
    // (no `displacement`: it needs a mark, the runner holds none at the end of a run, and it is left to the API)
    {"--correlate-kind", &RunOptions::correlateKind, {{"velocity", PB_CORR_VELOCITY}, {"radius", PB_CORR_RADIUS}}},
    {"--correlate-rmax", &RunOptions::correlateRmax, 0.0f, true},
    {"--correlate-bins", &RunOptions::correlateBins, 1, PB_CORR_MAX_BINS},

    {"--timecorr", &RunOptions::timecorrPath, "recorder"},
    {"--timecorr-interval", &RunOptions::timecorrInterval, 0.0f, false},
    {"--timecorr-lags", &RunOptions::timecorrLags, 1, PB_TCORR_MAX_LAGS},
    {"--timecorr-overlap", &RunOptions::timecorrOverlap, 0.0f, false, 2048.0f},

    {"--field", &RunOptions::fieldPath, "analysis"},
    {"--field-cells", &RunOptions::fieldCells, 1, PB_FIELD_MAX_AXIS},
    {"--field-half", &RunOptions::fieldHalf, 0.0f, true},

    {"--sk", &RunOptions::skPath, "analysis"},
    {"--sk-kind", &RunOptions::skKind,
     {{"density", PB_SK_DENSITY}, {"radius", PB_SK_RADIUS}, {"velocity", PB_SK_VELOCITY}}},
    {"--sk-box-log2", &RunOptions::skBoxLog2, PB_SK_MIN_LOG2, PB_SK_MAX_LOG2},
    {"--sk-nmax", &RunOptions::skNmax, 1, 44},  // (45: 4140 vectors, past PB_SK_MAX_VECTORS)

    {"--scatter", &RunOptions::scatterPath, "recorder"},
    {"--scatter-interval", &RunOptions::scatterInterval, 0.0f, false},
    {"--scatter-lags", &RunOptions::scatterLags, 1, PB_SCATTER_MAX_LAGS},
    {"--scatter-box-log2", &RunOptions::scatterBoxLog2, PB_SK_MIN_LOG2, PB_SK_MAX_LOG2},
    {"--scatter-nmax", &RunOptions::scatterNmax, 1, 10},  // (11: 264 vectors, past PB_SCATTER_MAX_VECTORS)

    {"--vanhove", &RunOptions::vanhovePath, "recorder"},
    {"--vanhove-interval", &RunOptions::vanhoveInterval, 0.0f, false},
    {"--vanhove-lags", &RunOptions::vanhoveLags, 1, PB_VANHOVE_MAX_LAGS},
    {"--vanhove-width", &RunOptions::vanhoveWidth, 0.0f, true, 2048.0f},
    {"--vanhove-bins", &RunOptions::vanhoveBins, 1, PB_VANHOVE_MAX_BINS},

    {"--vanhove-distinct", &RunOptions::vanhoveDistinctPath, "recorder"},
    {"--vanhove-distinct-interval", &RunOptions::vanhoveDistinctInterval, 0.0f, false},
    {"--vanhove-distinct-lags", &RunOptions::vanhoveDistinctLags, 1, PB_VANHOVE_MAX_LAGS},
    {"--vanhove-distinct-width", &RunOptions::vanhoveDistinctWidth, 0.0f, true, 2048.0f},
    {"--vanhove-distinct-bins", &RunOptions::vanhoveDistinctBins, 1, PB_VANHOVE_MAX_BINS},

    {"--coherent", &RunOptions::coherentPath, "recorder"},
    {"--coherent-interval", &RunOptions::coherentInterval, 0.0f, false},
    {"--coherent-lags", &RunOptions::coherentLags, 1, PB_COHERENT_MAX_LAGS},
    {"--coherent-box-log2", &RunOptions::coherentBoxLog2, PB_SK_MIN_LOG2, PB_SK_MAX_LOG2},
    {"--coherent-nmax", &RunOptions::coherentNmax, 1, 10},  // (11: 264 vectors, past PB_COHERENT_MAX_VECTORS)

    {"--fourpoint", &RunOptions::fourpointPath, "recorder"},
    {"--fourpoint-interval", &RunOptions::fourpointInterval, 0.0f, false},
    {"--fourpoint-lags", &RunOptions::fourpointLags, 1, PB_FOURPOINT_MAX_LAGS},
    {"--fourpoint-overlap", &RunOptions::fourpointOverlap, 0.0f, false, 2048.0f},
    {"--fourpoint-box-log2", &RunOptions::fourpointBoxLog2, PB_SK_MIN_LOG2, PB_SK_MAX_LOG2},
    {"--fourpoint-nmax", &RunOptions::fourpointNmax, 1, 10},  // (11: 265 vectors, past PB_FOURPOINT_MAX_VECTORS)

    {"--bonds", &RunOptions::bondsPath, "recorder"},
    {"--bonds-interval", &RunOptions::bondsInterval, 0.0f, false},
    {"--bonds-lags", &RunOptions::bondsLags, 1, PB_BOND_MAX_LAGS},
    {"--bonds-gap", &RunOptions::bondsGap, 0.0f, false, 2048.0f},
    {"--bonds-max-radius", &RunOptions::bondsMaxRadius, 0.0f, true, 1024.0f},
    {"--bonds-overlap", &RunOptions::bondsOverlap, 0.0f, false, 256.0f},
};

// a flag's value: the whole string a finite float, >= lowest (> lowest when `above`)
bool parseFloat(const char *text, float lowest, bool above, float &value) {
  char *end = nullptr;
  value = strtof(text, &end);
  return end != text && !*end && (above ? value > lowest : value >= lowest) && !std::isinf(value);
}

// a flag's value: the whole string an integer in lo ... hi
bool parseLong(const char *text, long lo, long hi, long &value) {
  char *end = nullptr;
  value = strtol(text, &end, 10);
  return end != text && !*end && value >= lo && value <= hi;
}

// a flag's value: one of the words
bool parseWord(const char *text, const std::vector<Choice> &choices, int &value) {
  for (const Choice &c : choices)
    if (!strcmp(c.first, text)) return value = c.second, true;
  return false;
}

// the flags that fit no kind: unchecked numbers, as they always were, and the two that are not one value for one member
void parseOdd(const char *name, char **value, RunOptions &o) {
  if (!strcmp(name, "--set")) o.sets.emplace_back(value[0], value[1]);
  else if (!strcmp(name, "--engine"))
    o.engine = !strcmp(value[0], "legacy") ? Particlebot::Engine::Legacy : Particlebot::Engine::Fused;
  else if (!strcmp(name, "--frame-size")) o.frameSize = atoi(value[0]);
  else if (!strcmp(name, "--checkpoint-every")) o.ckptEverySeconds = atof(value[0]);
  else if (!strcmp(name, "--checkpoint-steps")) o.ckptEverySteps = atol(value[0]);
  else o.stopAfterSteps = atol(value[0]);
}

// false at the first argument that is no flag with its value(s) in range; a bare argument is the configuration file
bool parseArgs(int argc, char **argv, RunOptions &o) {
  for (int i = 1; i < argc; i++) {
    if (argv[i][0] != '-') {
      o.configPath = argv[i];
      continue;
    }
    const Flag *f =
        std::find_if(std::begin(kFlags), std::end(kFlags), [&](const Flag &k) { return !strcmp(k.name, argv[i]); });
    if (f == std::end(kFlags) || i + f->values >= argc) return false;
    char **value = argv + i + 1;
    i += f->values;
    bool good = true;
    if (f->path) o.*f->path = value[0];
    else if (f->on) o.*f->on = true;
    else if (f->real) good = parseFloat(value[0], f->lowest, f->above, o.*f->real) && o.*f->real < f->below;
    else if (f->whole) good = parseLong(value[0], f->lo, f->hi, o.*f->whole);
    else if (f->pick) good = parseWord(value[0], f->choices, o.*f->pick);
    else parseOdd(f->name, value, o);
    if (!good) return false;
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// What the writers share.

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

// an unsigned integer of little-endian 64-bit limbs in decimal
std::string decimalLimbs(std::vector<unsigned long long> v) {
  std::string s;
  bool more = true;
  while (more) {
    unsigned long long rem = 0;
    more = false;
    for (size_t k = v.size(); k-- > 0;) {
      const unsigned __int128 cur = ((unsigned __int128)rem << 64) | v[k];
      v[k] = (unsigned long long)(cur / 10), rem = (unsigned long long)(cur % 10);
      more = more || v[k] != 0;
    }
    s.insert(s.begin(), (char)('0' + (int)rem));
  }
  return s;
}

// a signed integer of three little-endian 64-bit limbs, two's complement, in decimal
std::string decimalSigned192(const unsigned long long (&w)[3]) {
  std::vector<unsigned long long> v(w, w + 3);
  const bool negative = (w[2] >> 63) != 0;
  if (negative) {  // the magnitude: every limb inverted, plus one
    unsigned long long carry = 1;
    for (unsigned long long &limb : v) limb = ~limb + carry, carry = carry && limb == 0 ? 1 : 0;
  }
  return (negative ? "-" : "") + decimalLimbs(v);
}

// such an integer as a long double (for a quotient that is printed to 9 digits)
long double real192(const unsigned long long (&w)[3]) {
  const bool negative = (w[2] >> 63) != 0;
  unsigned long long v[3] = {w[0], w[1], w[2]};
  if (negative) {
    unsigned long long carry = 1;
    for (unsigned long long &limb : v) limb = ~limb + carry, carry = carry && limb == 0 ? 1 : 0;
  }
  const long double mag = ((long double)v[2] * 18446744073709551616.0L + (long double)v[1]) * 18446744073709551616.0L + (long double)v[0];
  return negative ? -mag : mag;
}

// a signed integer of two little-endian 64-bit limbs, two's complement
__int128 signed128(const unsigned long long (&w)[2]) { return (__int128)(((unsigned __int128)w[1] << 64) | w[0]); }

std::string decimalSigned128(const unsigned long long (&w)[2]) {
  const __int128 v = signed128(w);
  const unsigned __int128 mag = v < 0 ? -(unsigned __int128)v : (unsigned __int128)v;
  return (v < 0 ? "-" : "") + decimal128((unsigned long long)(mag >> 64), (unsigned long long)mag);
}

// an analysis output; NULL after saying so
FILE *openOutput(const std::string &path, const char *mode) {
  FILE *f = fopen(path.c_str(), mode);
  if (!f) fprintf(stderr, "cannot open %s\n", path.c_str());
  return f;
}

// An output started afresh when `fresh`, else appended to.  Its header line, if it has one, goes in front of a fresh
// file (WhenFresh) or of an empty one (WhenEmpty: also a resumed run that appends to none).  The two rules differ for a
// run that is resumed, and each output keeps the one it has.
enum class Header { WhenFresh, WhenEmpty };
FILE *openWithHeader(const std::string &path, bool fresh, Header rule, const char *header) {
  FILE *f = openOutput(path, fresh ? "w" : "a");
  if (!f || !header) return f;
  if (rule == Header::WhenFresh ? fresh : (fseek(f, 0, SEEK_END) == 0 && ftell(f) == 0)) fprintf(f, "%s\n", header);
  return f;
}

// an output written whole when the run ends, its header line first
FILE *openWhole(const std::string &path, const char *header) {
  return openWithHeader(path, true, Header::WhenFresh, header);
}

// the first two columns of a radial bin's row: its edges b * R / B and (b + 1) * R / B in double
void printBinEdges(FILE *f, size_t b, float rmax, long bins) {
  fprintf(f, "%.9g, %.9g, ", (double)b * (double)rmax / (double)bins, (double)(b + 1) * (double)rmax / (double)bins);
}

// the (nx, ny) pairs of the half plane ny > 0 || (ny == 0 && nx > 0) with |nx|, |ny| <= nmax
std::vector<int> halfPlaneVectors(int nmax) {
  std::vector<int> v;
  for (int nx = 1; nx <= nmax; nx++) v.push_back(nx), v.push_back(0);
  for (int ny = 1; ny <= nmax; ny++)
    for (int nx = -nmax; nx <= nmax; nx++) v.push_back(nx), v.push_back(ny);
  return v;
}

// the box of the wavevectors (2 pi / 2^E)(nx, ny): the E given, else the smallest with 2^E >= twice the wall half
// extent, at most PB_SK_MAX_LOG2
int boxLog2(long given, const PbRunConfig &cfg) {
  if (given >= PB_SK_MIN_LOG2) return (int)given;
  int e = PB_SK_MIN_LOG2;
  while (e < PB_SK_MAX_LOG2 && std::ldexp(1.0, e) < 2.0 * (double)cfg.wallHalf()) e++;
  return e;
}

// the interval of a recorder: the one given, else dump_interval, so that the records line up with the CSV
float recordEvery(float given, const PbRunConfig &cfg) { return given < 0.0f ? cfg.dump_interval : given; }

// the reference's video cadence (main.cpp:455-470): a frame every VIDEO_INTERVAL timesteps
int frameEvery(const PbRunConfig &cfg) { return cfg.video_interval > 0 ? cfg.video_interval : 100; }

// ---------------------------------------------------------------------------------------------------------------------
// The run: the simulation, its configuration, the options, where the loop is, and one writer or group of writers per
// output, in the order of the flag table.  A writer whose flag was not given does nothing and says true; false is exit
// code 1.  "At every dump time" is the gate dumpParticlebot uses (Particlebot::dumpDue): main() asks it.
struct Run {
  Particlebot &sim;
  const PbRunConfig &cfg;
  const RunOptions &o;
  long stepsDone = 0, frames = 0;
  unsigned long long seriesWritten = 0;  // --series: the records drained so far
  bool referenceMarked = false;          // --rearrange and --strain: the mark and its time
  float markTime = 0.0f;

  // A lag's sums are exact only below 2^31 samples, and the engine refuses a table that holds more.  The tables stay on
  // the device until the run ends, so a run whose records (from max_time, the start time and the interval) times nCells
  // would reach 2^31 (10^6 bots: 2147 records) is refused when it starts, not after its last step.  False after saying
  // so.
  // the records a run from here to max_time takes at this interval (+ 2: the gate's rounding takes at most one more)
  double recordsAhead(float every) {
    const double left = std::max(0.0, (double)sim.getParams().max_time - (double)sim.getTime());
    return left / (double)(every > 0.0f ? every : cfg.timestep) + 2.0;
  }

  bool recordsFit(const char *flag, float every) {
    const SimParams &p = sim.getParams();
    const double records = recordsAhead(every);
    if (records * (double)p.nCells < 2147483648.0) return true;
    fprintf(stderr, "%s: about %.0f records of %u bots would pass 2^31 samples per lag: raise %s-interval "
                    "or lower max_time\n", flag, records, (unsigned)p.nCells, flag);
    return false;
  }

  // the reach of the two radial analyses: the one given, else 10 * max_radius
  float radialReach(float given) { return given > 0.0f ? given : 10.0f * sim.getParams().max_radius; }

  // the files that get a row or a block at a dump time start afresh at time 0
  FILE *openForDump(const std::string &path, Header rule, const char *header) {
    return openWithHeader(path, sim.getTime() == 0.0f, rule, header);
  }

  // --frames DIR: a PPM of the arena every frameEvery() timesteps, viewed like the reference's camera: centred on
  // (camera_x, 0), half extent camera_y * tan(30 deg).  --frame-style reference draws it in the device colours of
  // updateCol with the centroid trail (Particlebot::writeFramePPMReference); --frame-render device rasterises it on the
  // GPU from the engine's resident state (Particlebot::writeFramePPMDevice: the same bytes, no state copy; fused engine
  // only), host (default) is the class's CPU writer.
  bool writeFrame() {
    if (o.framesDir.empty() || stepsDone % frameEvery(cfg) != 0) return true;
    char name[64];
    snprintf(name, sizeof name, "/frame_%06ld.ppm", frames++);
    const std::string path = o.framesDir + name;
    const int n = o.frameSize;
    const float half = cfg.camera_y * 0.57735027f, cx = cfg.camera_x, light = cfg.light_radius;
    bool ok;
    if (o.deviceFrames) ok = sim.writeFramePPMDevice(path.c_str(), n, n, cx, 0.0f, half, light, o.referenceFrames);
    else if (o.referenceFrames) ok = sim.writeFramePPMReference(path.c_str(), n, n, cx, 0.0f, half, light);
    else ok = sim.writeFramePPM(path.c_str(), n, n, cx, 0.0f, half, light);
    if (!ok) fprintf(stderr, "cannot write %s\n", path.c_str());
    return ok;
  }

  // --trail FILE: the reference's centroid trail (Particlebot::setDisplay records it; a resumed run starts a fresh
  // one), written at the end of the run as `slot,time,x,y` rows: the slots that hold a record, fp32 time and x to 9
  // digits, y as the double (stored y) - 2000, without the shader's +2000.
  bool writeTrail() {
    if (o.trailPath.empty()) return true;
    std::vector<float> xy, times;
    unsigned records = 0;
    FILE *f = fopen(o.trailPath.c_str(), "w");
    if (!f || !sim.getCentroidTrail(xy, times, records)) {
      fprintf(stderr, "cannot write %s\n", o.trailPath.c_str());
      if (f) fclose(f);
      return false;
    }
    fprintf(f, "slot,time,x,y\n");
    for (size_t k = 0; k < times.size(); k++)
      if (!std::isnan(times[k]))  // a slot that holds a record
        fprintf(f, "%zu,%.9g,%.9g,%.17g\n", k, (double)times[k], (double)xy[2 * k], (double)xy[2 * k + 1] - 2000.0);
    return fclose(f) == 0;
  }

  // --clusters FILE: at every dump time one row of the device's cluster analysis (Particlebot::clusterStats), the
  // header at time 0.  Without the flag nothing is analysed.
  bool dumpClusters() {
    if (o.clustersPath.empty()) return true;
    pbClusterStats cs;
    if (!sim.clusterStats(o.clusterGap, cs)) return false;
    FILE *f = openForDump(o.clustersPath, Header::WhenFresh, "Time, Clusters, Largest, Isolated, Links, MaxDegree");
    if (!f) return false;
    fprintf(f, "%f, %u, %u, %u, %llu, %u\n", sim.getTime(), cs.clusters, cs.largest, cs.isolated, cs.links,
            cs.max_degree);
    return fclose(f) == 0;
  }

  // --contacts FILE: the contact network of the FINAL state (Particlebot::contacts), one row per directed entry in CSR
  // order (I ascending, J ascending within I), floats as %.9g so that fp32 round-trips.
  bool writeContacts() {
    if (o.contactsPath.empty()) return true;
    std::vector<unsigned> offsets;
    std::vector<pbContactLink> links;
    if (!sim.contacts(o.contactGap, offsets, links)) return false;
    FILE *f = openWhole(o.contactsPath, "I, J, Gap, Fx, Fy");
    if (!f) return false;
    for (size_t i = 0; i + 1 < offsets.size(); i++)
      for (unsigned k = offsets[i]; k < offsets[i + 1]; k++)
        fprintf(f, "%zu, %u, %.9g, %.9g, %.9g\n", i, links[k].other, (double)links[k].gap, (double)links[k].fx,
                (double)links[k].fy);
    return fclose(f) == 0;
  }

  // --structure FILE: at every dump time one row of the device's hexatic analysis (Particlebot::structureStats), the
  // header at time 0, the sums as the integers they are (units of 2^-30).
  bool dumpStructure() {
    if (o.structurePath.empty()) return true;
    pbStructureStats ss;
    if (!sim.structureStats(o.structureGap, ss)) return false;
    FILE *f = openForDump(o.structurePath, Header::WhenFresh,
                          "Time, Bonds, Psi6Re, Psi6Im, C0, C1, C2, C3, C4, C5, C6, C7");
    if (!f) return false;
    fprintf(f, "%f, %llu, %lld, %lld", sim.getTime(), ss.bonds, ss.psi6_re, ss.psi6_im);
    for (int k = 0; k < 8; k++) fprintf(f, ", %u", ss.coordination[k]);
    fprintf(f, "\n");
    return fclose(f) == 0;
  }

  // --rdf FILE: the radial pair counts of the FINAL state (Particlebot::radialCounts), one row per bin.
  bool writeRdf() {
    if (o.rdfPath.empty()) return true;
    const float rmax = radialReach(o.rdfRmax);
    std::vector<unsigned long long> counts;
    if (!sim.radialCounts(rmax, (unsigned)o.rdfBins, counts)) return false;
    FILE *f = openWhole(o.rdfPath, "RLo, RHi, Count");
    if (!f) return false;
    for (size_t b = 0; b < counts.size(); b++) {
      printBinEdges(f, b, rmax, o.rdfBins);
      fprintf(f, "%llu\n", counts[b]);
    }
    return fclose(f) == 0;
  }

  // --rearrange FILE: a reference is marked on the device at the run's first dump time (Particlebot::markReference;
  // time 0, or the time a resumed run starts at: the mark is not part of a checkpoint), and at every dump time, the
  // first included, one row compares the state with it (Particlebot::rearrangementStats).  Every number is the integer
  // it is: bonds directed, SumQx / SumQy in units of 2^-20, SumQ2 / MaxQ2 of 2^-40, SumQ2 in decimal from its 128 bits.
  // --rearrange-window marks again after each row, so that every row describes one dump interval.
  // --strain FILE [--strain-threshold T]: against the same mark (it is taken, at --rearrange-gap, and with
  // --rearrange-window renewed, whether --rearrange is given or not), one row of the strain analysis' integers at every
  // dump time (Particlebot::strainStats): fitted and unfitted bots, fitted bots whose D2min is above T, used and
  // dropped bonds, the eight sums of the moments, SumD2 and MaxD2, all of 2^-40 and the 128-bit ones in decimal.  Both
  // rows of a dump time are written before a window's re-mark.
  bool dumpRearrangement() {
    if (o.rearrangePath.empty() && o.strainPath.empty()) return true;
    if (!referenceMarked) {  // the run's first dump time
      if (!sim.markReference(o.rearrangeGap)) return false;
      referenceMarked = true;
      markTime = sim.getTime();
    }
    if (!writeRearrangementRow() || !writeStrainRow()) return false;
    if (o.rearrangeWindow) {  // the next row describes the interval that starts here
      if (!sim.markReference(o.rearrangeGap)) return false;
      markTime = sim.getTime();
    }
    return true;
  }

  bool writeStrainRow() {
    if (o.strainPath.empty()) return true;
    pbStrainStats ss;
    if (!sim.strainStats(o.strainThreshold, ss)) return false;
    FILE *f = openForDump(o.strainPath, Header::WhenEmpty,
                          "Time, MarkTime, Fitted, Unfitted, Above, BondsUsed, BondsDropped, Yxx, Yxy, Yyy, Xxx, Xxy, Xyx, "
                          "Xyy, W, SumD2, MaxD2");
    if (!f) return false;
    fprintf(f, "%f, %f, %u, %u, %u, %llu, %llu, %s, %s, %s, %s, %s, %s, %s, %s, %s, %llu\n", sim.getTime(), markTime,
            ss.fitted, ss.unfitted, ss.above, ss.bonds_used, ss.bonds_dropped, decimal128(ss.yxx).c_str(),
            decimal128(ss.yxy).c_str(), decimal128(ss.yyy).c_str(), decimal128(ss.xxx).c_str(),
            decimal128(ss.xxy).c_str(), decimal128(ss.xyx).c_str(), decimal128(ss.xyy).c_str(), decimal128(ss.w).c_str(),
            decimal128(ss.sum_d2).c_str(), ss.max_d2);
    return fclose(f) == 0;
  }

  bool writeRearrangementRow() {
    if (o.rearrangePath.empty()) return true;
    pbRearrangementStats rs;
    if (!sim.rearrangementStats(rs)) return false;
    FILE *f = openForDump(o.rearrangePath, Header::WhenEmpty,
                          "Time, MarkTime, BondsMarked, BondsNow, BondsKept, Unchanged, Lost, Gained, Measured, SumQx, "
                          "SumQy, SumQ2, MaxQ2");
    if (!f) return false;
    fprintf(f, "%f, %f, %llu, %llu, %llu, %u, %u, %u, %u, %lld, %lld, %s, %llu\n", sim.getTime(), markTime,
            rs.bonds_marked, rs.bonds_now, rs.bonds_kept, rs.bots_unchanged, rs.bots_lost, rs.bots_gained, rs.measured,
            rs.sum_qx, rs.sum_qy, decimal128(rs.sum_q2_hi, rs.sum_q2_lo).c_str(), rs.max_q2);
    return fclose(f) == 0;
  }

  // --series FILE: the device's time-series recorder (Particlebot::setSeries).  While the engine steps, one row of
  // integer moments of positions, velocities and radii (pbMomentsRow, include/particlebot_hip.h) is taken in front of
  // every step whose start time passes the schedule's gate at --series-interval, into a device ring of
  // --series-capacity rows.  It is switched on behind a resume, so that the records start at the run's first step and a
  // resumed run appends from the resume point (the series is not part of a checkpoint).  main() drains the new records
  // at every host stop of its loop and once after it, and never hands the engine more than the capacity in steps in one
  // batch, so no record is overwritten unread.  A line per record: Time as %.9g, every other number the integer it is
  // (sums of q in units of 2^-20, sums of products of 2^-40, in decimal from their 128 bits, SumXY signed).
  bool startSeries() {
    if (o.seriesPath.empty()) return true;
    if (!sim.setSeries(recordEvery(o.seriesInterval, cfg), (unsigned)o.seriesCapacity)) return false;
    FILE *f = openWithHeader(o.seriesPath, o.resumePath.empty(), Header::WhenEmpty,
                             "Time, Step, Measured, SumQx, SumQy, MinQx, MaxQx, MinQy, MaxQy, SumXX, SumYY, SumXY, "
                             "SumQr, SumRR, SumWx, SumWy, SumVV");
    return f && fclose(f) == 0;
  }

  bool drainSeries() {
    if (o.seriesPath.empty()) return true;
    std::vector<pbMomentsRow> rows;
    if (!sim.seriesRows(seriesWritten, rows)) return false;
    if (rows.empty()) return true;
    FILE *f = openOutput(o.seriesPath, "a");
    if (!f) return false;
    for (const pbMomentsRow &m : rows)
      fprintf(f, "%.9g, %llu, %u, %lld, %lld, %d, %d, %d, %d, %s, %s, %s, %lld, %s, %lld, %lld, %s\n", (double)m.time,
              m.step, m.measured, m.sum_qx, m.sum_qy, m.min_qx, m.max_qx, m.min_qy, m.max_qy, decimal128(m.xx).c_str(),
              decimal128(m.yy).c_str(), decimal128(m.xy).c_str(), m.sum_qr, decimal128(m.rr).c_str(), m.sum_wx,
              m.sum_wy, decimal128(m.vv).c_str());
    seriesWritten += rows.size();
    return fclose(f) == 0;
  }

  // --correlate FILE: the pair correlations of the FINAL state (Particlebot::pairCorrelation).  Line 1 the totals, line
  // 2 the header, then one row per bin, the edges as --rdf prints them, every other number the integer it is (Dot and
  // SumA2 in units of 2^-40, the sums of a in units of 2^-20, in decimal from their 128 bits).
  bool writeCorrelation() {
    if (o.correlatePath.empty()) return true;
    const float rmax = radialReach(o.correlateRmax);
    std::vector<pbCorrelationBin> rows;
    pbCorrelationTotals tot;
    if (!sim.pairCorrelation(o.correlateKind, rmax, (unsigned)o.correlateBins, rows, tot)) return false;
    FILE *f = openOutput(o.correlatePath, "w");
    if (!f) return false;
    fprintf(f, "Kind, %s, Measured, %u, SumAx, %lld, SumAy, %lld, SumA2, %s, Pairs, %llu\n",
            o.correlateKind == PB_CORR_RADIUS ? "radius" : "velocity", tot.measured, tot.sum_ax, tot.sum_ay,
            decimal128(tot.sum_a2).c_str(), tot.pairs);
    fprintf(f, "RLo, RHi, Pairs, Dot, SumAx, SumAy\n");
    for (size_t b = 0; b < rows.size(); b++) {
      printBinEdges(f, b, rmax, o.correlateBins);
      fprintf(f, "%llu, %s, %s, %s\n", rows[b].pairs, decimal128(rows[b].dot).c_str(), decimal128(rows[b].ax).c_str(),
              decimal128(rows[b].ay).c_str());
    }
    return fclose(f) == 0;
  }

  // --timecorr FILE: the device's time correlations (Particlebot::setTimeCorrelation).  While the engine steps, a
  // snapshot of positions and velocities is taken in front of every step whose start time passes the schedule's gate at
  // --timecorr-interval, into a device ring of --timecorr-lags snapshots, and every record is added against the latest
  // ones into one row per lag: squared displacement, velocity products and the count of bots that moved less than
  // --timecorr-overlap.  Switched on behind a resume, like the series (the correlation is not part of a checkpoint).
  // At the end of the run one line per lag, lag 0 first, every number the integer it is (SumQx / SumQy in units of
  // 2^-20, SumQ2, SumWW and MaxQ2 of 2^-40, the 128-bit sums in decimal, SumWW signed); the mean lag of a row is
  // SumSteps / Origins steps.  The start's result is main()'s exit code: 2 for a table that cannot fit (recordsFit).
  int startTimeCorrelation() {
    if (o.timecorrPath.empty()) return 0;
    const float every = recordEvery(o.timecorrInterval, cfg);
    if (!recordsFit("--timecorr", every)) return 2;
    const float overlap = o.timecorrOverlap < 0.0f ? sim.getParams().min_radius : o.timecorrOverlap;
    return sim.setTimeCorrelation(every, (unsigned)o.timecorrLags, overlap) ? 0 : 1;
  }

  bool writeTimeCorrelation() {
    if (o.timecorrPath.empty()) return true;
    std::vector<pbTimeCorrelationRow> rows;
    if (!sim.timeCorrelationRows(rows)) return false;
    FILE *f = openWhole(o.timecorrPath, "Lag, Origins, SumSteps, Samples, SumQx, SumQy, SumQ2, SumWW, Overlap, MaxQ2");
    if (!f) return false;
    for (const pbTimeCorrelationRow &t : rows)
      fprintf(f, "%u, %llu, %llu, %llu, %lld, %lld, %s, %s, %llu, %llu\n", t.lag, t.origins, t.sum_steps, t.samples,
              t.sum_qx, t.sum_qy, decimal128(t.msd).c_str(), decimal128(t.vacf).c_str(), t.overlap, t.max_q2);
    return fclose(f) == 0;
  }

  // --field FILE: at every dump time one block of the device's field map of the state (Particlebot::fieldMap): a square
  // map of --field-cells x --field-cells cells centred on (0, 0) with half extent --field-half.  The header goes in
  // front of an empty file; a block is one line per NON-EMPTY cell, row 0 the lowest y: time as %.9g, step the steps
  // taken so far, every other number the integer it is (the sums in units of 2^-20, rr and vv of 2^-40, in decimal from
  // their 128 bits).
  bool dumpField() {
    if (o.fieldPath.empty()) return true;
    pbFieldView view;
    view.nx = view.ny = (unsigned)o.fieldCells;
    view.centerX = view.centerY = 0.0f;
    view.halfX = view.halfY = o.fieldHalf > 0.0f ? o.fieldHalf : cfg.wallHalf();
    std::vector<pbFieldCell> cells;
    pbFieldTotals tot;
    if (!sim.fieldMap(view, cells, tot)) return false;
    FILE *f = openForDump(o.fieldPath, Header::WhenEmpty, "time,step,ix,iy,count,dead,sum_qr,sum_wx,sum_wy,rr,vv");
    if (!f) return false;
    for (size_t k = 0; k < cells.size(); k++) {
      const pbFieldCell &c = cells[k];
      if (!c.count) continue;
      fprintf(f, "%.9g,%ld,%zu,%zu,%u,%u,%lld,%lld,%lld,%s,%s\n", (double)sim.getTime(), stepsDone, k % view.nx,
              k / view.nx, c.count, c.dead, c.sum_qr, c.sum_wx, c.sum_wy, decimal128(c.rr).c_str(),
              decimal128(c.vv).c_str());
    }
    return fclose(f) == 0;
  }

  // --sk FILE: at every dump time one block of the device's structure factor of the state
  // (Particlebot::structureFactor) over halfPlaneVectors(--sk-nmax) in the box boxLog2(--sk-box-log2), weighted by
  // --sk-kind.  No header: a block is the line `time,<%.9g>,step,<steps so
  // far>,kind,<kind>,box_log2,<E>,vectors,<count>` and then one line per vector, `nx,ny,measured,re,im,re2,im2`, every
  // number the integer it is (units of 2^-30 for the density, 2^-50 otherwise, in decimal from their 128 bits, signed).
  bool dumpStructureFactor() {
    if (o.skPath.empty()) return true;
    const int box = boxLog2(o.skBoxLog2, cfg);
    std::vector<pbStructureFactorRow> rows;
    if (!sim.structureFactor(o.skKind, box, halfPlaneVectors((int)o.skNmax), rows)) return false;
    FILE *f = openForDump(o.skPath, Header::WhenFresh, nullptr);
    if (!f) return false;
    static const char *const kinds[] = {"density", "radius", "velocity"};
    fprintf(f, "time,%.9g,step,%ld,kind,%s,box_log2,%d,vectors,%zu\n", (double)sim.getTime(), stepsDone,
            kinds[o.skKind], box, rows.size());
    for (const pbStructureFactorRow &s : rows)
      fprintf(f, "%d,%d,%u,%s,%s,%s,%s\n", s.nx, s.ny, s.measured, decimal128(s.re).c_str(), decimal128(s.im).c_str(),
              decimal128(s.re2).c_str(), decimal128(s.im2).c_str());
    return fclose(f) == 0;
  }

  // --scatter FILE: the device's self-intermediate scattering function (Particlebot::setScattering).  While the engine
  // steps, a snapshot of the quantised positions is taken in front of every step whose start time passes the schedule's
  // gate at --scatter-interval, into a device ring of --scatter-lags snapshots, and every record is added against the
  // latest ones into one row per lag and wavevector: the integer phasor sums of every bot's displacement, over
  // halfPlaneVectors(--scatter-nmax) in the box boxLog2(--scatter-box-log2).  Switched on behind a resume, like
  // --timecorr (the ring is not part of a checkpoint), and refused by the same count.  At the end of the run one line
  // per lag and vector, lag 0 first, the vectors in list order: the integers as they are (Re and Im in units of 2^-30),
  // then FsRe = Re / (2^30 Samples) and FsIm likewise as %.9g (nan with no sample).
  int startScattering() {
    if (o.scatterPath.empty()) return 0;
    const float every = recordEvery(o.scatterInterval, cfg);
    if (!recordsFit("--scatter", every)) return 2;
    return sim.setScattering(every, (unsigned)o.scatterLags, boxLog2(o.scatterBoxLog2, cfg),
                               halfPlaneVectors((int)o.scatterNmax)) ? 0 : 1;
  }

  bool writeScattering() {
    if (o.scatterPath.empty()) return true;
    std::vector<pbScatteringRow> rows;
    if (!sim.scatteringRows(rows)) return false;
    FILE *f = openWhole(o.scatterPath, "Lag, Nx, Ny, Origins, SumSteps, Samples, Re, Im, FsRe, FsIm");
    if (!f) return false;
    for (const pbScatteringRow &s : rows) {
      const long double unit = 1073741824.0L * (long double)s.samples;  // (both operands are exact in a long double)
      const double fsRe = s.samples ? (double)((long double)s.re / unit) : std::nan("");
      const double fsIm = s.samples ? (double)((long double)s.im / unit) : std::nan("");
      fprintf(f, "%u, %d, %d, %llu, %llu, %llu, %lld, %lld, %.9g, %.9g\n", s.lag, s.nx, s.ny, s.origins, s.sum_steps,
              s.samples, s.re, s.im, fsRe, fsIm);
    }
    return fclose(f) == 0;
  }

  // --vanhove FILE: the device's self van Hove function (Particlebot::setVanHove).  While the engine steps, a snapshot of
  // the positions is taken in front of every step whose start time passes the schedule's gate at --vanhove-interval, into
  // a device ring of --vanhove-lags snapshots, and every record is added against the latest ones into the histograms of
  // every bot's displacement per lag: --vanhove-bins radial bins of --vanhove-width and twice as many of each component.
  // Switched on behind a resume, like --timecorr (the ring is not part of a checkpoint), and refused by the same count.
  // At the end of the run, per lag, lag 0 first: the radial bins (Axis r), then those of x, then of y, each axis followed
  // by one line with Bin -1 for its beyond count.  The lag's columns are repeated on each of its lines: the integers as
  // they are (SumQ2 in units of 2^-40, SumQ4 of 2^-80, in decimal from their 128 and 192 bits), then
  // Alpha2 = SumQ4 Samples / (2 SumQ2^2) - 1 as %.9g (nan where SumQ2 is 0).  Lower is the bin's lower edge in world
  // units as %.9g, a multiple of the quantised width; a beyond line has the radial histogram's end, and nan for an axis,
  // whose beyond count has two sides.
  int startVanHove() {
    if (o.vanhovePath.empty()) return 0;
    const float every = recordEvery(o.vanhoveInterval, cfg);
    if (!recordsFit("--vanhove", every)) return 2;
    const float width = o.vanhoveWidth > 0.0f ? o.vanhoveWidth : 0.125f * sim.getParams().min_radius;
    return sim.setVanHove(every, (unsigned)o.vanhoveLags, width, (unsigned)o.vanhoveBins) ? 0 : 1;
  }

  bool writeVanHove() {
    if (o.vanhovePath.empty()) return true;
    std::vector<pbVanHoveRow> rows;
    std::vector<unsigned long long> counts;
    float interval = 0.0f, width = 0.0f;
    unsigned lags = 0, bins = 0;
    unsigned long long records = 0;
    if (!sim.vanHoveRows(rows, counts) || !sim.vanHoveInfo(interval, lags, width, bins, records)) return false;
    FILE *f = openWhole(o.vanhovePath, "Lag, Origins, SumSteps, Samples, SumQ2, SumQ4, Alpha2, Axis, Bin, Lower, Count");
    if (!f) return false;
    const double qw = (double)std::nearbyint(width * 1048576.0f) / 1048576.0;  // the quantised width, as the engine's
    for (size_t l = 0; l < rows.size(); l++) {
      const pbVanHoveRow &v = rows[l];
      const long double q2 = std::ldexp((long double)v.msd.hi, 32) + (long double)v.msd.lo;
      const long double q4 = std::ldexp((long double)v.q4[2], 128) + std::ldexp((long double)v.q4[1], 64) + (long double)v.q4[0];
      const double alpha2 = q2 != 0.0L ? (double)(q4 * (long double)v.samples / (2.0L * q2 * q2) - 1.0L) : std::nan("");
      char lead[512];
      snprintf(lead, sizeof lead, "%u, %llu, %llu, %llu, %s, %s, %.9g", v.lag, v.origins, v.sum_steps, v.samples,
               decimal128(v.msd).c_str(), decimalLimbs({v.q4[0], v.q4[1], v.q4[2]}).c_str(), alpha2);
      const unsigned long long *c = &counts[l * 5u * bins];
      // an axis: its counters, where they start, the bin of its first counter, its beyond count and that line's edge
      const auto axis = [&](char name, size_t at, size_t count, long first, unsigned long long beyond, double end) {
        for (size_t j = 0; j < count; j++)
          fprintf(f, "%s, %c, %zu, %.9g, %llu\n", lead, name, j, (double)(first + (long)j) * qw, c[at + j]);
        fprintf(f, "%s, %c, -1, %.9g, %llu\n", lead, name, end, beyond);
      };
      axis('r', 0, bins, 0, v.beyond_r, (double)bins * qw);
      axis('x', bins, 2u * (size_t)bins, -(long)bins, v.beyond_x, std::nan(""));
      axis('y', 3u * (size_t)bins, 2u * (size_t)bins, -(long)bins, v.beyond_y, std::nan(""));
    }
    return fclose(f) == 0;
  }

  // --vanhove-distinct FILE: the device's distinct van Hove function (Particlebot::setVanHoveDistinct).  Records are
  // taken as --vanhove takes them, at --vanhove-distinct-interval into a ring of --vanhove-distinct-lags snapshots, and
  // every record is added against the latest ones into --vanhove-distinct-bins counters of --vanhove-distinct-width per
  // lag: the ordered pairs (a bot then, another bot now) by distance.  The default width is --vanhove's, an eighth of
  // min_radius, cut so that bins x width stays below 2048 as the engine asks.  Switched on behind a resume and refused by
  // the same count as --timecorr.  At the end of the run one line per lag and bin, lag 0 first; the lag's columns are
  // repeated on each of its lines, the integers as they are, and Lower is the bin's lower edge in world units as %.9g.
  int startVanHoveDistinct() {
    if (o.vanhoveDistinctPath.empty()) return 0;
    const float every = recordEvery(o.vanhoveDistinctInterval, cfg);
    if (!recordsFit("--vanhove-distinct", every)) return 2;
    const float most = 2047.0f / (float)o.vanhoveDistinctBins;
    const float width = o.vanhoveDistinctWidth > 0.0f ? o.vanhoveDistinctWidth
                                                      : std::min(0.125f * sim.getParams().min_radius, most);
    return sim.setVanHoveDistinct(every, (unsigned)o.vanhoveDistinctLags, width, (unsigned)o.vanhoveDistinctBins) ? 0 : 1;
  }

  bool writeVanHoveDistinct() {
    if (o.vanhoveDistinctPath.empty()) return true;
    std::vector<pbVanHoveDistinctRow> rows;
    std::vector<unsigned long long> counts;
    float interval = 0.0f, width = 0.0f;
    unsigned lags = 0, bins = 0;
    unsigned long long records = 0;
    if (!sim.vanHoveDistinctRows(rows, counts) || !sim.vanHoveDistinctInfo(interval, lags, width, bins, records))
      return false;
    FILE *f = openWhole(o.vanhoveDistinctPath, "Lag, Origins, SumSteps, Centres, Partners, Pairs, Bin, Lower, Count");
    if (!f) return false;
    const double qw = (double)std::nearbyint(width * 1048576.0f) / 1048576.0;  // the quantised width, as the engine's
    for (size_t l = 0; l < rows.size(); l++) {
      const pbVanHoveDistinctRow &v = rows[l];
      for (size_t j = 0; j < bins; j++)
        fprintf(f, "%u, %llu, %llu, %llu, %llu, %llu, %zu, %.9g, %llu\n", v.lag, v.origins, v.sum_steps, v.centres,
                v.partners, v.pairs, j, (double)j * qw, counts[l * bins + j]);
    }
    return fclose(f) == 0;
  }

  // --coherent FILE: the device's coherent intermediate scattering function (Particlebot::setCoherent).  Records are taken
  // as --scatter takes them, at --coherent-interval into a ring of --coherent-lags records of the density modes rho(k)
  // over halfPlaneVectors(--coherent-nmax) in the box boxLog2(--coherent-box-log2), and every record's modes are
  // multiplied with the latest ones' into one row per lag and wavevector.  Switched on behind a resume.  Its sums hold
  // whatever the bots: the one cap is 2^31 origins per lag, so a run is refused by its record count alone.  At the end
  // of the run one line per lag and vector, lag 0 first, the vectors in list order:
  // the integers as they are (Re and Im as exact signed decimals from their 192 bits, units of 2^-60), then
  // FRe = Re / (2^60 BotsThen) and FIm likewise as %.9g (nan with no bot).
  int startCoherent() {
    if (o.coherentPath.empty()) return 0;
    const float every = recordEvery(o.coherentInterval, cfg);
    if (const double records = recordsAhead(every); records >= 2147483648.0) {
      fprintf(stderr, "--coherent: about %.0f records would pass 2^31 origins per lag: raise --coherent-interval or "
                      "lower max_time\n", records);
      return 2;
    }
    return sim.setCoherent(every, (unsigned)o.coherentLags, boxLog2(o.coherentBoxLog2, cfg),
                           halfPlaneVectors((int)o.coherentNmax)) ? 0 : 1;
  }

  bool writeCoherent() {
    if (o.coherentPath.empty()) return true;
    std::vector<pbCoherentRow> rows;
    if (!sim.coherentRows(rows)) return false;
    FILE *f = openWhole(o.coherentPath, "Lag, Nx, Ny, Origins, SumSteps, BotsNow, BotsThen, Re, Im, FRe, FIm");
    if (!f) return false;
    for (const pbCoherentRow &c : rows) {
      const long double unit = 1152921504606846976.0L * (long double)c.bots_then;  // 2^60 BotsThen
      const double fRe = c.bots_then ? (double)(real192(c.re) / unit) : std::nan("");
      const double fIm = c.bots_then ? (double)(real192(c.im) / unit) : std::nan("");
      fprintf(f, "%u, %d, %d, %llu, %llu, %llu, %llu, %s, %s, %.9g, %.9g\n", c.lag, c.nx, c.ny, c.origins, c.sum_steps,
              c.bots_now, c.bots_then, decimalSigned192(c.re).c_str(), decimalSigned192(c.im).c_str(), fRe, fIm);
    }
    return fclose(f) == 0;
  }

  // --fourpoint FILE: the device's four-point recorder (Particlebot::setFourPoint).  Records are taken as --scatter takes
  // them, at --fourpoint-interval into a ring of --fourpoint-lags records of the quantised positions; per pair of
  // records the bots within --fourpoint-overlap (default min_radius) of where they were are counted, and their density
  // mode is formed over halfPlaneVectors(--fourpoint-nmax) and (0, 0), the list's last, in the box
  // boxLog2(--fourpoint-box-log2).  Switched on behind a resume; refused by its record count alone, as --coherent.  At
  // the end of the run one line per lag and vector, lag 0 first, the vectors in list order: the integers as they are
  // (Overlap2, Re, Im and Power as exact decimals from their limbs), then Chi4 = (Overlap2 O - Overlap^2) / (O Samples),
  // the numerator exact, and S4 = (Power O - Re^2 - Im^2) / (2^60 O Samples) in long double, both as %.9g (nan with no
  // sample).
  int startFourPoint() {
    if (o.fourpointPath.empty()) return 0;
    const float every = recordEvery(o.fourpointInterval, cfg);
    if (const double records = recordsAhead(every); records >= 2147483648.0) {
      fprintf(stderr, "--fourpoint: about %.0f records would pass 2^31 origins per lag: raise --fourpoint-interval or "
                      "lower max_time\n", records);
      return 2;
    }
    std::vector<int> vectors = halfPlaneVectors((int)o.fourpointNmax);
    vectors.push_back(0), vectors.push_back(0);
    const float overlap = o.fourpointOverlap < 0.0f ? sim.getParams().min_radius : o.fourpointOverlap;
    return sim.setFourPoint(every, (unsigned)o.fourpointLags, overlap, boxLog2(o.fourpointBoxLog2, cfg), vectors) ? 0 : 1;
  }

  bool writeFourPoint() {
    if (o.fourpointPath.empty()) return true;
    std::vector<pbFourPointRow> rows;
    if (!sim.fourPointRows(rows)) return false;
    FILE *f = openWhole(o.fourpointPath,
                        "Lag, Nx, Ny, Origins, SumSteps, Samples, Overlap, Overlap2, Re, Im, Power, Chi4, S4");
    if (!f) return false;
    for (const pbFourPointRow &c : rows) {
      double chi4 = std::nan(""), s4 = std::nan("");
      if (c.samples) {  // (then there are origins)
        const long double scale = (long double)c.origins * (long double)c.samples;
        // Overlap2 O < 2^118 and Overlap^2 < 2^118: the numerator is exact
        const unsigned __int128 q2 = ((unsigned __int128)c.overlap2[1] << 64) | c.overlap2[0];
        const __int128 num = (__int128)(q2 * c.origins) - (__int128)((unsigned __int128)c.overlap * c.overlap);
        chi4 = (double)((long double)num / scale);
        const long double re = (long double)signed128(c.re), im = (long double)signed128(c.im);
        s4 = (double)((real192(c.power) * (long double)c.origins - re * re - im * im) / (scale * 1152921504606846976.0L));
      }
      fprintf(f, "%u, %d, %d, %llu, %llu, %llu, %llu, %s, %s, %s, %s, %.9g, %.9g\n", c.lag, c.nx, c.ny, c.origins,
              c.sum_steps, c.samples, c.overlap, decimal128(c.overlap2[1], c.overlap2[0]).c_str(),
              decimalSigned128(c.re).c_str(), decimalSigned128(c.im).c_str(), decimalSigned192(c.power).c_str(), chi4, s4);
    }
    return fclose(f) == 0;
  }

  // --bonds FILE: the device's bond recorder (Particlebot::setBondDynamics).  Records are taken as --timecorr takes
  // them, at --bonds-interval into a ring of --bonds-lags records of every bot's quantised position and neighbour list
  // under the link rule at --bonds-gap, among the bots whose radius is at most --bonds-max-radius (default: max_radius of
  // the configuration).  A payload bot larger than max_radius is ABSENT, with no links and nobody's neighbour, unless
  // --bonds-max-radius is raised to hold it.  A caged bot overlaps if it moved less than --bonds-overlap (default
  // min_radius) relative to the neighbours it had.  Switched on behind a resume; refused by its record count alone, as
  // --timecorr.  At the end of the run one line per lag, lag 0 first: the row's integers as they are (the 128-bit sums
  // as exact decimals), then BondSurvival = BondsKept / BondsThen, FractionLost = BotsLost / Samples,
  // CageMsd = (sum_k CageQ2_k / k^2) / (2^40 C), PlainMsd = PlainQ2 / (2^40 C) and CageOverlap = (sum_k CageOverlap_k) / C
  // with C = sum_k CageSamples_k, in long double, as %.9g (nan where the denominator is 0).
  int startBonds() {
    if (o.bondsPath.empty()) return 0;
    const float every = recordEvery(o.bondsInterval, cfg);
    if (const double records = recordsAhead(every); records >= 2147483648.0) {
      fprintf(stderr, "--bonds: about %.0f records would pass 2^31 origins per lag: raise --bonds-interval or lower "
                      "max_time\n", records);
      return 2;
    }
    const float maxRadius = o.bondsMaxRadius > 0.0f ? o.bondsMaxRadius : sim.getParams().max_radius;
    const float overlap = o.bondsOverlap < 0.0f ? sim.getParams().min_radius : o.bondsOverlap;
    return sim.setBondDynamics(every, (unsigned)o.bondsLags, o.bondsGap, maxRadius, overlap) ? 0 : 1;
  }

  bool writeBonds() {
    if (o.bondsPath.empty()) return true;
    std::vector<pbBondRow> rows;
    if (!sim.bondDynamicsRows(rows)) return false;
    std::string header = "Lag, Origins, SumSteps, Samples, Crowded, BondsThen, BondsNow, BondsKept, BotsUnchanged, BotsLost, "
                         "BotsGained, PlainQ2";
    for (const char *column : {"CageSamples", "CageOverlap", "CageQ2"})
      for (unsigned k = 1; k <= PB_BOND_WIDTH; k++) header += std::string(", ") + column + std::to_string(k);
    header += ", BondSurvival, FractionLost, CageMsd, PlainMsd, CageOverlap";
    FILE *f = openWhole(o.bondsPath, header.c_str());
    if (!f) return false;
    const auto real = [](const pbMoment128 &m) { return (long double)m.hi * 4294967296.0L + (long double)m.lo; };
    const auto quotient = [](long double num, long double den) { return den > 0.0L ? (double)(num / den) : std::nan(""); };
    for (const pbBondRow &r : rows) {
      fprintf(f, "%u, %llu, %llu, %llu, %llu, %llu, %llu, %llu, %llu, %llu, %llu, %s", r.lag, r.origins, r.sum_steps,
              r.samples, r.crowded, r.bonds_then, r.bonds_now, r.bonds_kept, r.bots_unchanged, r.bots_lost, r.bots_gained,
              decimal128(r.plain_q2).c_str());
      long double caged = 0.0L, overlapping = 0.0L, cage = 0.0L;
      for (unsigned k = 0; k < PB_BOND_WIDTH; k++) {
        fprintf(f, ", %llu", r.cage_samples[k]);
        caged += (long double)r.cage_samples[k], overlapping += (long double)r.cage_overlap[k];
        cage += real(r.cage_q2[k]) / (long double)((k + 1u) * (k + 1u));
      }
      for (unsigned k = 0; k < PB_BOND_WIDTH; k++) fprintf(f, ", %llu", r.cage_overlap[k]);
      for (unsigned k = 0; k < PB_BOND_WIDTH; k++) fprintf(f, ", %s", decimal128(r.cage_q2[k]).c_str());
      const long double unit = 1099511627776.0L;  // 2^40
      fprintf(f, ", %.9g, %.9g, %.9g, %.9g, %.9g\n", quotient((long double)r.bonds_kept, (long double)r.bonds_then),
              quotient((long double)r.bots_lost, (long double)r.samples), quotient(cage, caged * unit),
              quotient(real(r.plain_q2), caged * unit), quotient(overlapping, caged));
    }
    return fclose(f) == 0;
  }
};

}  // namespace

// main.cpp:823-967 minus the window: defaults, the .cfg file (default "example.cfg"), srand(seed), derived grid
// parameters, open the CSV, construct + reset, then `for(;;){ dump(); update(); }` (display(), main.cpp:354-361).
// Between dump rows the steps are handed to the engine in one batch so that it can keep one fused kernel per timestep.
//
// --resume FILE continues a run (main.cpp:954-957 -> particlebot.cpp:369-411): FILE is either an exact checkpoint
// written by --checkpoint (time, every state array incl. phase / dead / force sums, the stale slot layout, both random
// generators, and the length the CSV had: the resumed run is bit-identical to the uninterrupted one and the CSV ends up
// byte-identical) or, as in the reference, a testing=1 CSV whose last complete row supplies time, positions, velocities
// and radii (phases, dead set and force sums start afresh: the reference's lossy resume).
// --checkpoint FILE is rewritten (write to FILE.tmp, rename) every --checkpoint-every SECONDS of wall time and/or every
// --checkpoint-steps timesteps, always at a point where the main loop is about to dump.
int main(int argc, char **argv) {
  RunOptions o;
  if (!parseArgs(argc, argv, o)) {
    // (the line stops at the flags it listed when --rearrange was the newest output: from --series on, the synopsis at
    // the head of this file lists a flag and this line does not)
    fprintf(stderr,
            "usage: %s [config.cfg] [--set NAME VALUE]... [--engine fused|legacy] [--quiet] "
            "[--frames DIR [--frame-size PIXELS] [--frame-style plain|reference] [--frame-render host|device]] [--trail FILE] [--clusters FILE [--cluster-gap G]] [--contacts FILE [--contact-gap G]] "
            "[--structure FILE [--structure-gap G]] [--rdf FILE [--rdf-rmax R] [--rdf-bins B]] [--rearrange FILE [--rearrange-gap G] [--rearrange-window]] [--resume FILE [--overwrite-csv]] [--checkpoint FILE "
            "[--checkpoint-every SECONDS] [--checkpoint-steps N]] [--final-checkpoint FILE]\n",
            argv[0]);
    return 2;
  }
  for (const Flag &f : kFlags)
    if (f.noun && !(o.*f.path).empty() && o.engine != Particlebot::Engine::Fused) {
      fprintf(stderr, "%s needs the fused engine (the %s runs on its resident state)\n", f.name, f.noun);
      return 2;
    }
  PbRunConfig cfg;
  if (!cfg.loadFile(o.configPath))
    fprintf(stderr, "warning: cannot open %s, running on defaults\n", o.configPath.c_str());
  for (auto &kv : o.sets) cfg.setParam(kv.first, kv.second);
  srand(cfg.params.seed);  // main.cpp:929 (the class itself draws from a private, identical stream)
  cfg.derive();

  // resuming from an exact checkpoint keeps the CSV written so far (cut back to the length it had when the
  // checkpoint was taken); every other start truncates it, as the reference's fopen("w+") does (main.cpp:944)
  RunTrailer trailer;
  const bool exactResume = !o.resumePath.empty() && isExactCheckpoint(o.resumePath);
  if (exactResume && !readTrailer(o.resumePath, trailer)) {
    fprintf(stderr, "%s: not a checkpoint written by particlebot_run --checkpoint\n", o.resumePath.c_str());
    return 1;
  }
  if (o.quiet) {
    // dumpParticlebot echoes "time cx cy" per row to stdout, as the reference does
    if (!freopen("/dev/null", "w", stdout)) return 1;
  }
  Particlebot sim(cfg.params, o.engine, cfg.wallHalf());
  sim.setExitOnMaxTime(false);
  sim.setHexSpacing(cfg.hex_spacing);
  sim.setSquareLattice(cfg.square_lattice);
  sim.setFastBlob(cfg.fast_blob);
  sim.setRng(cfg.rng_kind);
  sim.setForceVariant(cfg.force_variant);
  if (!o.trailPath.empty() || o.referenceFrames) sim.setDisplay(true);
  sim.reset();
  const SimParams &p = sim.getParams();
  Run run{sim, cfg, o};
  if (!o.resumePath.empty()) {
    FILE *rf = fopen(o.resumePath.c_str(), exactResume ? "rb" : "r");
    if (!rf) {
      fprintf(stderr, "cannot open %s\n", o.resumePath.c_str());
      return 1;
    }
    if (exactResume) {
      if (!sim.loadCheckpoint(rf)) {
        fprintf(stderr, "%s does not match this configuration (bot count?) or is damaged\n", o.resumePath.c_str());
        return 1;
      }
      run.stepsDone = trailer.stepsDone;
      run.frames = trailer.frames;
    } else {
      sim.loadFromFile(0, p.nCells, rf, cfg.dump_interval);  // main.cpp:954-957
    }
    fclose(rf);
  }
  // the CSV: truncated on a fresh start (main.cpp:944); appended to when the run continues from its own last row
  // (main.cpp:940-956); cut back to the length the checkpoint recorded on an exact resume
  // "Its own": the SAME FILE, however it is spelled (./run.csv, an absolute path, a symlink) -- decided by device and
  // inode, not by comparing strings; a resume from ANOTHER CSV never truncates an existing csv_filename silently
  // (`--resume ./run.csv` with csv_filename run.csv destroyed every earlier row of the run): it is
  // only truncated with --overwrite-csv.
  bool csvResumeInPlace = false;
  if (!o.resumePath.empty() && !exactResume) {
    struct stat a, b;
    const bool haveA = stat(o.resumePath.c_str(), &a) == 0, haveB = stat(cfg.csv_filename.c_str(), &b) == 0;
    csvResumeInPlace = haveA && haveB && a.st_dev == b.st_dev && a.st_ino == b.st_ino;
    if (!csvResumeInPlace && haveB && b.st_size > 0 && !o.overwriteCsv) {
      fprintf(stderr,
              "%s exists and is not the file being resumed (%s): refusing to truncate it; pass --overwrite-csv or "
              "choose another csv_filename\n",
              cfg.csv_filename.c_str(), o.resumePath.c_str());
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
    t.stepsDone = run.stepsDone;
    t.frames = run.frames;
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
  long lastCkptStep = run.stepsDone;
  // the recorders: switched on here, behind a resume and before the first dump
  if (!run.startSeries()) return 1;
  if (const int refused = run.startTimeCorrelation()) return refused;
  if (const int refused = run.startScattering()) return refused;
  if (const int refused = run.startVanHove()) return refused;
  if (const int refused = run.startVanHoveDistinct()) return refused;
  if (const int refused = run.startCoherent()) return refused;
  if (const int refused = run.startFourPoint()) return refused;
  if (const int refused = run.startBonds()) return refused;
  for (;;) {
    // a checkpoint is taken here, where the loop is about to dump: resuming re-enters at this very point
    if (!o.ckptPath.empty() && run.stepsDone > lastCkptStep) {
      const double since = std::chrono::duration<double>(std::chrono::steady_clock::now() - lastCkptWall).count();
      if ((o.ckptEverySteps > 0 && run.stepsDone - lastCkptStep >= o.ckptEverySteps) ||
          (o.ckptEverySeconds > 0 && since >= o.ckptEverySeconds)) {
        if (!writeCheckpoint(o.ckptPath)) return 1;
        lastCkptWall = std::chrono::steady_clock::now();
        lastCkptStep = run.stepsDone;
      }
    }
    if (o.stopAfterSteps >= 0 && run.stepsDone >= o.stopAfterSteps) _exit(9);  // (no flush, no destructors: a kill)
    sim.dumpParticlebot(0, p.nCells, fp, cfg.dump_interval, p.testing, p.light_x, p.light_y);
    if (!run.drainSeries()) return 1;
    if (sim.dumpDue(cfg.dump_interval) && !(run.dumpClusters() && run.dumpStructure() && run.dumpField() &&
                                            run.dumpStructureFactor() && run.dumpRearrangement()))
      return 1;
    if (!run.writeFrame()) return 1;
    if (sim.finished()) break;  // the reference exits from inside update() here
    int batch = sim.stepsUntilHostEvent(cfg.timestep, cfg.dump_interval, 1 << 20);
    if (!o.framesDir.empty()) batch = (int)std::min<long>(batch, frameEvery(cfg) - run.stepsDone % frameEvery(cfg));
    if (o.ckptEverySteps > 0) batch = (int)std::min<long>(batch, o.ckptEverySteps - (run.stepsDone - lastCkptStep) > 0
                                                                     ? o.ckptEverySteps - (run.stepsDone - lastCkptStep)
                                                                     : 1);
    else if (o.ckptEverySeconds > 0) batch = std::min(batch, 20000);  // look at the clock now and then
    if (!o.seriesPath.empty()) batch = (int)std::min<long>(batch, o.seriesCapacity);  // records <= steps: none is lost
    const int ran = sim.advance(cfg.timestep, cfg.sort_interval, batch);
    if (ran == 0) break;
    run.stepsDone += ran;
  }
  if (!run.drainSeries()) return 1;
  if (!o.finalCkptPath.empty() && !writeCheckpoint(o.finalCkptPath)) return 1;
  fclose(fp);
  const bool written = run.writeTrail() && run.writeContacts() && run.writeRdf() && run.writeTimeCorrelation() &&
                       run.writeScattering() && run.writeVanHove() && run.writeVanHoveDistinct() &&
                       run.writeCoherent() && run.writeFourPoint() && run.writeBonds() && run.writeCorrelation();
  return written ? 0 : 1;
}
