// pb_ensemble.cpp -- ensembles: many independent simulations in one batched pbSim (include/particlebot_ensemble.h).
// Member k = the base .cfg + common overrides + its own overrides (typically "seed\n<k>").  The
// host work of every member (random placement, dead-bot draw) runs in its own HostOnly Particlebot
// with its own private libc-compatible stream; the device work of all members runs in ONE batched
// pbSim, one launch per timestep.  Summaries (time, COMx, COMy, distance of the COM to the light) are
// taken whenever a dump row would be due.
#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>

#include "pb_ensemble.hpp"

// Host side of one member: configuration, placement (Particlebot::reset) and -- when the draw is due at the very
// first step -- the dead set, all from the member's PRIVATE random stream, so that it does not matter which thread
// builds which member, or when.  Returns false if the .cfg cannot be read.
bool configureMember(Member &m, const char *cfg_path, const char *common_overrides, const char *own_overrides) {
  m.cfg.reset(new PbRunConfig());
  if (!m.cfg->resolve(cfg_path, common_overrides, own_overrides)) return false;
  m.bot.reset(new Particlebot(m.cfg->params, Particlebot::Engine::HostOnly, m.cfg->wallHalf()));
  m.bot->setHexSpacing(m.cfg->hex_spacing);
  m.bot->setSquareLattice(m.cfg->square_lattice);
  m.bot->setFastBlob(m.cfg->fast_blob);
  m.bot->setRng(m.cfg->rng_kind);
  return true;
}

bool buildMember(Member &m, const char *cfg_path, const char *common_overrides, const char *own_overrides,
                 const Particlebot::Placement *shared, Particlebot::Placement *out) {
  if (!configureMember(m, cfg_path, common_overrides, own_overrides)) return false;
  Particlebot *bot = m.bot.get();
  if (shared) {
    if (!bot->importPlacement(*shared)) return false;
  } else {
    bot->reset();
    if (out) bot->exportPlacement(*out);
  }
  bot->setHostTime(0.0f);
  if (bot->deadDrawDue(m.cfg->timestep)) {  // particlebot.cpp:178: drawn at the top of the first update()
    (void)bot->drawDeadBotsNow();
    m.deadDrawn = true;
  }
  return true;
}

int groupPlacements(const char *cfg_path, const char *common_overrides, int nmembers,
                    const std::function<const char *(int)> &ownOverrides, std::vector<int> &keyOf) {
  keyOf.assign(nmembers, -1);
  const char *env = getenv("PB_SHARE_PLACEMENTS");
  if (env && env[0] == '0') return 0;
  std::map<std::string, std::vector<int>> byKey;
  for (int k = 0; k < nmembers; k++) {
    // (the key needs the configuration only, not a Particlebot with its host arrays)
    PbRunConfig c;
    if (!c.resolve(cfg_path, common_overrides, ownOverrides(k))) continue;
    byKey[Particlebot::placementKeyOf(c.params, c.hex_spacing, c.square_lattice, c.fast_blob)].push_back(k);
  }
  int ngroups = 0;
  for (auto &g : byKey) {
    if (g.second.size() < 2) continue;
    for (int k : g.second) keyOf[k] = ngroups;
    ngroups++;
  }
  return ngroups;
}

// device side: create the batched pbSim of already built members and upload their initial state
bool uploadEnsemble(Ensemble *e) {
  const int nmembers = (int)e->members.size();
  std::vector<SimParams> params;
  for (int k = 0; k < nmembers; k++) params.push_back(e->members[k]->bot->getParams());
  const PbRunConfig &c0 = *e->members[0]->cfg;
  // the force kernel and the phase-noise generator are chosen per BATCH: a member that asks for another one than
  // member 0 (a per-member override, `--sweep pb_force_variant 2 3`) would silently get member 0's -- refuse
  for (int k = 1; k < nmembers; k++) {
    const PbRunConfig &ck = *e->members[k]->cfg;
    if (ck.force_variant != c0.force_variant || ck.rng_kind != c0.rng_kind) {
      char msg[256];
      snprintf(msg, sizeof msg,
               "members of one batch must agree on pb_force_variant and pb_rng: member 0 has %d / %d, member %d has "
               "%d / %d (run them as separate ensembles)",
               c0.force_variant, c0.rng_kind, k, ck.force_variant, ck.rng_kind);
      fprintf(stderr, "pbEnsemble: %s\n", msg);
      return false;
    }
  }
  if (pbSimCreateBatch(&e->sim, params.data(), nmembers, c0.wallHalf()) != PB_OK) return false;
  if (c0.rng_kind != 0 && pbSimSetRng(e->sim, c0.rng_kind) != PB_OK) return false;
  if (c0.force_variant >= 0 && pbSimSetForceVariant(e->sim, c0.force_variant) != PB_OK) return false;  // pb_force_variant
  for (int k = 0; k < nmembers; k++) {
    const Particlebot *b = e->members[k]->bot.get();
    if (pbSimSetStateOf(e->sim, (unsigned)k, b->hostPositions(), b->hostVelocities(), b->hostRadii(), b->hostPhases(),
                        b->hostDead()) != PB_OK)
      return false;
  }
  return true;
}

// How many summary rows a run from t = 0 writes: the clock and the gate of runSteps below (fp32 t = t + dt; a row
// whenever pbDumpRowDue(t, di), the last one at the first t > max_time), for at most max_steps steps.
// Stops counting at `limit` + 1: callers only ask "does it fit".
long rowsNeeded(float dt, float di, float max_time, long max_steps, long limit) {
  long rows = 0, steps = 0;
  for (float t = 0.0f;; t = t + dt, steps++) {
    if (pbDumpRowDue(t, di) && ++rows > limit) break;
    if (t > max_time || steps >= max_steps) break;
    if (t + dt == t) return limit + 1;  // the fp32 clock has stopped short of max_time: rows without end
  }
  return rows;
}

// Runs every member of the batch for up to max_steps timesteps (or to max_time, whichever comes first); can be
// called again to continue.  Row r of member k goes to out[(k * max_rows + r) * 4 ..]: (time, COMx, COMy, distance
// of the COM to the light), one row whenever a dump row would be due (particlebot.cpp:309).
long runSteps(Ensemble *e, long max_steps, float *out, int max_rows, int *rows) {
  const int m = (int)e->members.size();
  const PbRunConfig &c0 = *e->members[0]->cfg;
  const float dt = c0.timestep, di = c0.dump_interval;
  std::vector<double> com(2 * (size_t)m);
  long steps = 0;
  int nrows = rows ? *rows : 0;
  float t = 0.0f;
  if (pbSimGetTime(e->sim, &t) != PB_OK) return -1;
  for (;;) {
    // a row is due at time t; e->rowTime remembers the last one written so that a call which stopped
    // exactly at a dump time does not write it twice when the run is continued
    const bool rowDue = pbDumpRowDue(t, di) && !(e->haveRow && e->rowTime == t);
    if (rowDue && !e->csvDir.empty() && (!out || nrows >= max_rows)) {
      // the member CSVs are documented as byte for byte the reference's: never a silently shortened file
      // (pbEnsemblePipelineRun refuses such a run before its first step; this is the stepwise API's guard)
      fprintf(stderr, "pbEnsemble: a CSV row is due at t = %g but the row buffer holds %d rows (max_rows %d): "
              "%s/member_*.csv would stop here; raise max_rows or the dump interval\n",
              (double)t, out ? nrows : 0, out ? max_rows : 0, e->csvDir.c_str());
      return -1;
    }
    if (rowDue && out && nrows >= max_rows) {
      // (the same for the summary rows themselves: a caller who passes a buffer gets every row or an error)
      fprintf(stderr, "pbEnsemble: a summary row is due at t = %g but the row buffer is full (max_rows %d); raise max_rows "
              "or the dump interval, or pass no buffer\n", (double)t, max_rows);
      return -1;
    }
    if (out && rowDue && nrows < max_rows) {
      if (pbSimCentroids(e->sim, com.data()) != PB_OK) return -1;
      for (int k = 0; k < m; k++) {
        const SimParams &p = e->members[k]->bot->getParams();
        float *row = out + ((size_t)k * max_rows + nrows) * 4;
        const double dx = com[2 * k] - p.light_x, dy = com[2 * k + 1] - p.light_y;
        row[0] = t;
        row[1] = (float)com[2 * k];
        row[2] = (float)com[2 * k + 1];
        row[3] = (float)sqrt(dx * dx + dy * dy);
      }
      if (!e->csvDir.empty()) {
        std::vector<float> sums(2 * (size_t)m);
        if (pbSimCentroidSums(e->sim, sums.data()) != PB_OK) return -1;
        if (e->csvFiles.empty()) e->csvFiles.assign(m, nullptr);
        for (int k = 0; k < m; k++) {
          if (!e->csvFiles[k]) {
            char name[64];
            snprintf(name, sizeof name, "/member_%06d.csv", e->csvIds[k]);
            e->csvFiles[k] = fopen((e->csvDir + name).c_str(), "w");
            if (!e->csvFiles[k]) {
              fprintf(stderr, "pbEnsemble: cannot write %s%s\n", e->csvDir.c_str(), name);
              return -1;
            }
          }
          const SimParams &p = e->members[k]->bot->getParams();
          pbWriteCsvRow(e->csvFiles[k], t, p.seed, sums[2 * k], sums[2 * k + 1], p.nCells, p.light_x, p.light_y);
          if (ferror(e->csvFiles[k])) {
            fprintf(stderr, "pbEnsemble: write error on %s/member_%06d.csv\n", e->csvDir.c_str(), e->csvIds[k]);
            return -1;
          }
        }
      }
      nrows++;
      e->haveRow = true;
      e->rowTime = t;
      if (!e->ckptDir.empty() &&
          !saveSubBatch(e, out, max_rows, nrows, e->stepsBefore + steps, t > c0.params.max_time)) {
        fprintf(stderr, "pbEnsemble: cannot write the checkpoint of sub-batch %d under %s\n", e->ckptSub, e->ckptDir.c_str());
        return -1;
      }
    }
    if (t > c0.params.max_time) {
      // the run is over: the member CSVs are complete only if every buffered byte reached the disk
      for (size_t k = 0; k < e->csvFiles.size(); k++) {
        FILE *f = e->csvFiles[k];
        e->csvFiles[k] = nullptr;
        if (f && fclose(f) != 0) {
          fprintf(stderr, "pbEnsemble: cannot finish %s/member_%06d.csv\n", e->csvDir.c_str(), e->csvIds[k]);
          return -1;
        }
      }
      break;
    }
    if (steps >= max_steps) break;
    // host events at this step: dead-bot draws (those due at time 0 came with the placement)
    for (int k = 0; k < m; k++) {
      Member *mk = e->members[k].get();
      Particlebot *b = mk->bot.get();
      b->setHostTime(t);
      if (b->deadDrawDue(dt) && !mk->deadDrawn) {
        mk->deadDrawn = true;
        if (pbSimSetStateOf(e->sim, (unsigned)k, nullptr, nullptr, nullptr, nullptr, b->drawDeadBotsNow()) != PB_OK)
          return -1;
      }
    }
    // run up to (not past) the next dump row or dead-bot draw of any member
    long run = 1;
    float tt = t + dt;
    for (;;) {
      bool stop = pbDumpRowDue(tt, di) || tt > c0.params.max_time || run >= (1 << 20) ||
                  steps + run >= max_steps;
      for (int k = 0; k < m && !stop; k++) {
        e->members[k]->bot->setHostTime(tt);
        stop = e->members[k]->bot->deadDrawDue(dt);
      }
      if (stop) break;
      tt = tt + dt;
      run++;
    }
    int done = 0;
    if (pbSimStep(e->sim, dt, c0.sort_interval, (int)run, &done) != PB_OK) return -1;
    steps += done;
    if (pbSimGetTime(e->sim, &t) != PB_OK) return -1;
    if (done == 0) break;
  }
  if (rows) *rows = nrows;
  return steps;
}

extern "C" {

void *pbEnsembleCreate(const char *cfg_path, const char *common_overrides, const char **member_overrides,
                       int nmembers) {
  if (nmembers < 1) return nullptr;
  std::unique_ptr<Ensemble> e(new Ensemble());
  e->members.resize(nmembers);
  // Members are independent (own configuration, own private random stream, own placement grid):
  // build them on all host cores.  The reference's random placement is O(N^1.5) (1.4 s for 10^5
  // bots), so a sweep of large members would otherwise spend minutes here.  (pbEnsemblePipeline* overlaps
  // this with the device work of the members built before.)
  // Members whose placement inputs agree (Particlebot::placementKey: a sweep under one seed) are placed ONCE, by the
  // thread that takes their group, and share the placed state + the generator state after it (as the pipeline does).
  auto own = [&](int k) { return member_overrides ? member_overrides[k] : nullptr; };
  std::vector<int> keyOf;
  std::vector<std::vector<int>> groups(groupPlacements(cfg_path, common_overrides, nmembers, own, keyOf));
  for (int k = 0; k < nmembers; k++) {
    if (keyOf[k] >= 0) groups[keyOf[k]].push_back(k);
    else groups.push_back({k});
  }
  std::atomic<int> next{0};
  std::atomic<bool> failed{false};
  auto worker = [&]() {
    for (int g = next++; g < (int)groups.size() && !failed; g = next++) {
      Particlebot::Placement placed;
      for (size_t j = 0; j < groups[g].size() && !failed; j++) {
        const int k = groups[g][j];
        e->members[k].reset(new Member());
        const bool first = j == 0, more = groups[g].size() > 1;
        if (!buildMember(*e->members[k], cfg_path, common_overrides, own(k), first ? nullptr : &placed,
                         first && more ? &placed : nullptr))
          failed = true;
      }
    }
  };
  const unsigned nthreads = std::min<unsigned>(hostThreads(0), (unsigned)groups.size());
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < nthreads; t++) pool.emplace_back(worker);
  worker();
  for (auto &th : pool) th.join();
  if (failed) return nullptr;
  if (!uploadEnsemble(e.get())) {
    fprintf(stderr, "pbEnsembleCreate: %s\n", pbGetLastErrorString());
    return nullptr;
  }
  return e.release();
}

void pbEnsembleDestroy(void *ev) { std::unique_ptr<Ensemble> e((Ensemble *)ev); }

// Runs every member for up to max_steps timesteps (or to max_time, whichever comes first) and can be
// called again to continue.  out: [nmembers][max_rows][4] floats (time, COMx, COMy, distance of the
// COM to the light), one row whenever a dump row would be due (particlebot.cpp:309); *rows counts
// the rows written per member so far (the same for all members) and is carried between calls.
// Returns the number of timesteps executed by this call, or -1 on error.
long pbEnsembleRunSteps(void *ev, long max_steps, float *out, int max_rows, int *rows) {
  return runSteps((Ensemble *)ev, max_steps, out, max_rows, rows);
}

// Runs every member to max_time (the whole run in one call).
long pbEnsembleRun(void *ev, float *out, int max_rows, int *rows) {
  int nrows = 0;
  const long steps = pbEnsembleRunSteps(ev, LONG_MAX, out, max_rows, &nrows);
  if (rows) *rows = nrows;
  return steps;
}

int pbEnsembleSynchronize(void *ev) { return pbSimSynchronize(((Ensemble *)ev)->sim); }

int pbEnsembleShard(int nmembers, int rank, int world) {
  if (nmembers < 0 || world < 1 || rank < 0 || rank >= world) return 0;
  return (nmembers - rank + world - 1) / world;  // members rank, rank + world, ... below nmembers
}

int pbEnsembleAssemble(int nmembers, int world, int rows, const float *gathered, float *out) {
  if (nmembers < 0 || world < 1 || rows < 0 || !gathered || !out) return 1;
  const int per = pbEnsembleShard(nmembers, 0, world);
  const size_t rowFloats = (size_t)rows * 4;
  for (int r = 0; r < world; r++) {
    const int mine = pbEnsembleShard(nmembers, r, world);
    for (int j = 0; j < mine; j++)
      memcpy(out + (size_t)(r + j * world) * rowFloats, gathered + ((size_t)r * per + j) * rowFloats,
             sizeof(float) * rowFloats);
  }
  return 0;
}

int pbEnsembleGetState(void *ev, int member, float *pos, float *vel, float *rad) {
  Ensemble *e = (Ensemble *)ev;
  return pbSimGetStateOf(e->sim, (unsigned)member, pos, vel, rad, nullptr, nullptr, nullptr, nullptr);
}

unsigned pbEnsembleNumBots(void *ev) { return ((Ensemble *)ev)->members[0]->bot->getParams().nCells; }

}  // extern "C"
