// pb_ensemble_pipeline.cpp -- the pipelined ensemble (pbEnsemblePipeline*, include/particlebot_ensemble.h): host
// placement of sub-batch k+1 overlapped with device stepping of sub-batch k.
// A rank's members are cut into sub-batches of `sub` members (in member order).  A pool of producer threads builds
// members in order (configuration, placement, early dead draw), never more than `ahead` sub-batches beyond the one
// on the device; the calling thread takes the sub-batches in order: waits until its members are built, creates the
// batched pbSim, uploads, steps it to the end, keeps what was asked for, frees it.  A member's trajectory does not
// depend on which members share its batch (every kernel form is bit-identical to the member's own oracle run; the
// centroid is a fixed-order per-member reduction), so the rows are independent of `sub`
// (tests/test_gpu_ensemble_pipeline.py).
#include <pthread.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>

#include "pb_ensemble.hpp"

namespace {

struct Pipeline {
  std::string cfgPath, common;
  bool haveCfg = false;
  std::vector<std::string> over;
  int nmembers = 0, sub = 0, threads = 1, ahead = 2;
  int lanes = 1;  // sub-batches stepped at the same time (pbEnsemblePipelineRun)
  std::string csvDir;       // pbEnsemblePipelineSetCsvDir
  std::vector<int> csvIds;  // [nmembers]
  bool keepStates = false;
  std::vector<std::unique_ptr<Member>> built;  // [nmembers], filled by the producers, taken by the consumer
  std::vector<char> ready;
  std::mutex mu;
  std::condition_variable cvReady, cvRoom;
  int nextToBuild = 0, consumedUpTo = 0;  // members < consumedUpTo have been taken by the consumer
  bool failed = false, stop = false;
  std::vector<std::thread> pool;
  std::vector<std::vector<float>> finalPos, finalVel, finalRad;
  unsigned nbots = 0;
  pbEnsembleTimings tm{};
  std::vector<double> cpuSeconds, wallSeconds;  // per producer thread: CPU time and wall time spent building members
  std::vector<int> pinCpus;                     // cores of the GPU's NUMA node (empty: producers are not pinned)
  int numaNode = -1;
  int device = -1;      // the creating thread's HIP device: Run may be called from another thread (which starts on 0)
  std::string ckptDir;  // checkpoints (pbEnsemblePipelineSetCheckpoint); empty: none
  bool resume = false;
  // One placement per distinct blob: members whose Particlebot::placementKey() agree -- a sweep of
  // nDead, light position, ... under one seed -- are placed once; the others take a copy of the placed state and of
  // the private generator's state after the placement, so every member is bit-identical to its stand-alone run.
  // keyOf[k] indexes `shared` (-1: groupPlacements gave this member no group, or the run is resumed).
  struct SharedPlacement {
    int state = 0;      // 0 nobody has started it, 1 being placed, 2 ready, -1 failed
    int usesLeft = 0;   // members that still have to take it (freed at 0)
    Particlebot::Placement placed;
  };
  std::vector<int> keyOf;
  std::vector<SharedPlacement> shared;
  std::condition_variable cvPlaced;
  int placementsRun = 0, placementsShared = 0;

  // what every member is resolved from: the .cfg (or none), the common overrides, its own
  const char *cfg() const { return haveCfg ? cfgPath.c_str() : nullptr; }
  bool build(Member &m, int k, const Particlebot::Placement *from = nullptr, Particlebot::Placement *out = nullptr) const {
    return buildMember(m, cfg(), common.c_str(), over[k].c_str(), from, out);
  }

  // (calling thread, before the pool starts) a resumed run restores or places every member for itself
  void groupMembers() {
    keyOf.assign(nmembers, -1);
    if (resume) return;
    shared.resize(groupPlacements(cfg(), common.c_str(), nmembers, [&](int k) { return over[k].c_str(); }, keyOf));
    for (int k : keyOf)
      if (k >= 0) shared[k].usesLeft++;
  }

  // Place shared blob `g` on this thread from member `k`'s configuration (its placement inputs are the group's) and
  // publish it.  Returns the member built along the way (placed, dead draw not yet done) or nullptr on failure.
  std::unique_ptr<Member> placeShared(int g, int k) {
    std::unique_ptr<Member> m(new Member());
    Particlebot::Placement placed;
    const bool ok = build(*m, k, nullptr, &placed);
    std::lock_guard<std::mutex> lock(mu);
    SharedPlacement &sp = shared[g];
    if (ok) {
      sp.placed = std::move(placed);
      sp.state = 2;
      placementsRun++;
    } else {
      sp.state = -1;
      m.reset();
    }
    cvPlaced.notify_all();
    return m;
  }

  // Member k of a shared group: take the group's placement, placing it first if nobody has.  While another thread is
  // placing it, this thread does not idle: it places the next group ahead that nobody has started (its members will
  // find it ready), then looks again.
  std::unique_ptr<Member> buildShared(int k) {
    const int g = keyOf[k];
    for (;;) {
      int other = -1, otherMember = -1;
      {
        std::unique_lock<std::mutex> lock(mu);
        SharedPlacement &sp = shared[g];
        if (sp.state == 0) {
          sp.state = 1;
          lock.unlock();
          std::unique_ptr<Member> m = placeShared(g, k);   // this member IS the one built along the way
          if (m) releaseShared(g);
          return m;
        }
        if (sp.state == -1) return nullptr;
        if (sp.state == 2) break;
        // being placed elsewhere: look ahead for work
        for (int j = k + 1; j < nmembers && other < 0; j++)
          if (keyOf[j] >= 0 && shared[keyOf[j]].state == 0) other = keyOf[j], otherMember = j;
        if (other >= 0) {
          shared[other].state = 1;
        } else {
          cvPlaced.wait(lock, [&] { return stop || failed || shared[g].state != 1; });
          if (stop || failed) return nullptr;
          continue;
        }
      }
      (void)placeShared(other, otherMember);   // (only the placement is kept; member `otherMember` is built in its turn)
    }
    std::unique_ptr<Member> m(new Member());
    // (state 2 entries are immutable until their last user has released them: read without the lock)
    if (!build(*m, k, &shared[g].placed)) return nullptr;
    {
      std::lock_guard<std::mutex> lock(mu);
      placementsShared++;
    }
    releaseShared(g);
    return m;
  }
  void releaseShared(int g) {
    std::lock_guard<std::mutex> lock(mu);
    if (--shared[g].usesLeft == 0) shared[g].placed = Particlebot::Placement();
  }

  // A member whose sub-batch has a complete checkpoint is restored, not placed: nullptr when there is none.  `ok`
  // turns false when there is one and it cannot be used.
  std::unique_ptr<Member> restoreMember(int k, bool &ok) {
    int gen = 0, nrows = 0, finished = 0;
    long steps = 0;
    if (!readManifest(ckptDir, k / sub, gen, nrows, finished, steps)) return nullptr;
    std::unique_ptr<Member> m(new Member());
    ok = configureMember(*m, cfg(), common.c_str(), over[k].c_str());
    if (ok && !loadMemberFile(*m, ckptDir, k, gen, nrows, steps)) {
      fprintf(stderr, "pbEnsemblePipeline: checkpoint of member %d under %s is unusable\n", k, ckptDir.c_str());
      ok = false;
    }
    if (!ok) m.reset();
    return m;
  }

  void producer(int tid) {
    for (;;) {
      int k;
      {
        std::unique_lock<std::mutex> lock(mu);
        // room: at most `ahead` sub-batches beyond the one the consumer is on
        cvRoom.wait(lock, [&] { return stop || failed || nextToBuild >= nmembers || nextToBuild < consumedUpTo + (ahead + 1) * sub; });
        if (stop || failed || nextToBuild >= nmembers) return;
        k = nextToBuild++;
      }
      const double t0 = nowSeconds(), c0 = threadCpuSeconds();
      bool ok = true;
      std::unique_ptr<Member> m;
      if (resume) m = restoreMember(k, ok);
      if (ok && !m) {
        if (keyOf[k] >= 0) {
          m = buildShared(k);
        } else {
          m.reset(new Member());
          if (!build(*m, k)) m.reset();
          if (m) {
            std::lock_guard<std::mutex> lock(mu);
            placementsRun++;
          }
        }
      }
      cpuSeconds[tid] += threadCpuSeconds() - c0;
      wallSeconds[tid] += nowSeconds() - t0;
      std::lock_guard<std::mutex> lock(mu);
      if (!m) {
        failed = true;
      } else {
        built[k] = std::move(m);
        ready[k] = 1;
      }
      cvReady.notify_all();
      cvRoom.notify_all();
      cvPlaced.notify_all();
    }
  }
  void start() {
    cpuSeconds.assign(threads, 0.0);
    wallSeconds.assign(threads, 0.0);
    for (int t = 0; t < threads; t++) pool.emplace_back(&Pipeline::producer, this, t);
    if (!pinCpus.empty()) {
      // the whole pool on the cores next to the GPU (the scheduler spreads the threads inside the set)
      cpu_set_t set;
      CPU_ZERO(&set);
      for (int c : pinCpus) CPU_SET(c, &set);
      bool ok = true;
      for (auto &th : pool) ok = pthread_setaffinity_np(th.native_handle(), sizeof set, &set) == 0 && ok;
      tm.pinned = ok ? 1 : 0;
    }
  }
  void shutdown() {
    {
      std::lock_guard<std::mutex> lock(mu);
      stop = true;
    }
    cvRoom.notify_all();
    cvReady.notify_all();
    cvPlaced.notify_all();
    for (auto &th : pool) th.join();
    pool.clear();
    for (auto &m : built) m.reset();
  }
  ~Pipeline() { shutdown(); }

  // The consumer's side of the hand-over, for Run and DryRun alike: waits until members first .. first + count - 1 are
  // built, takes them and tells the producers that there is room.  False once the pipeline has failed.  *aheadSeen
  // (DryRun) is raised to the members claimed by producers beyond the consumed ones, as seen just before the take.
  bool takeSubBatch(int first, int count, std::vector<std::unique_ptr<Member>> &members, int *aheadSeen = nullptr) {
    {
      std::unique_lock<std::mutex> lock(mu);
      cvReady.wait(lock, [&] {
        if (failed) return true;
        for (int k = first; k < first + count; k++)
          if (!ready[k]) return false;
        return true;
      });
      if (failed) return false;
      if (aheadSeen) *aheadSeen = std::max(*aheadSeen, nextToBuild - consumedUpTo);
      for (int k = first; k < first + count; k++) members.push_back(std::move(built[k]));
      consumedUpTo = std::max(consumedUpTo, first + count);
    }
    cvRoom.notify_all();
    return true;
  }
};

// ---- pbEnsemblePipelineRun: one sub-batch from "its members are placed" to "its rows are in `out`" ------------------
struct RunArgs {
  long max_steps;
  float *out;  // the whole ensemble's rows, or NULL
  int max_rows;
};
struct SubResult {
  long steps = 0;
  int nrows = 0;
  unsigned nbots = 0;
  double waitS = 0.0, uploadS = 0.0, deviceS = 0.0;
};

// refuse a run whose rows cannot fit BEFORE its first step, not hours into it
bool rowsFit(const PbRunConfig &c0, const RunArgs &a) {
  const long need = a.out ? rowsNeeded(c0.timestep, c0.dump_interval, c0.params.max_time, a.max_steps, a.max_rows) : 0;
  if (need <= a.max_rows) return true;
  fprintf(stderr, "pbEnsemblePipelineRun: the run writes more than %d summary rows per member (dump_interval %g, "
          "max_time %g) and the row buffer holds %d: raise max_rows (particlebot_ensemble --max-rows) or the dump "
          "interval; nothing was stepped\n", a.max_rows, (double)c0.dump_interval, (double)c0.params.max_time, a.max_rows);
  return false;
}

// restored from a checkpoint?  (all members of a sub-batch or none: they share one manifest)  -1: only partly
int restoredMembers(const Ensemble &e, int sub) {
  int n = 0;
  for (const auto &mk : e.members) n += mk->saved ? 1 : 0;
  if (n != 0 && n != (int)e.members.size()) {
    fprintf(stderr, "pbEnsemblePipelineRun: sub-batch %d is only partly in the checkpoint\n", sub);
    return -1;
  }
  return n;
}

// the checkpoint says this sub-batch has nothing left to run: the rows are the result
bool finishedFromCheckpoint(const Ensemble &e, float *outSub, int max_rows, SubResult &r) {
  const MemberSaved &s0 = *e.members[0]->saved;
  r.nrows = s0.nrows;
  r.steps = s0.steps;
  if (r.nrows > max_rows) return false;
  for (size_t k = 0; k < e.members.size() && outSub; k++)
    memcpy(outSub + k * max_rows * 4, e.members[k]->saved->rows.data(), sizeof(float) * 4 * (size_t)r.nrows);
  return true;
}

// the batch onto the device: placed members as they are, restored ones with their rows, layout, clock and generation
bool uploadOrRestore(Ensemble &e, bool restored, float *outSub, int max_rows, SubResult &r) {
  if (restored) {
    int r0 = 0, fin = 0;
    long st = 0;
    (void)readManifest(e.ckptDir, e.ckptSub, e.ckptGen, r0, fin, st);
    r.nrows = e.members[0]->saved->nrows;
    if (r.nrows > max_rows || !outSub) return false;
  }
  if (restored ? !uploadRestored(&e, outSub, max_rows) : !uploadEnsemble(&e)) {
    fprintf(stderr, "pbEnsemblePipelineRun: %s\n", pbGetLastErrorString());
    return false;
  }
  return true;
}

bool stepToTheEnd(Ensemble &e, long max_steps, float *outSub, int max_rows, SubResult &r) {
  const long more = runSteps(&e, max_steps - e.stepsBefore, outSub, max_rows, &r.nrows);
  if (more < 0 || pbSimSynchronize(e.sim) != PB_OK) return false;
  r.steps = e.stepsBefore + more;
  return true;
}

// the end of this sub-batch's run: finished (past max_time) or stopped by max_steps (resumable)
bool finalCheckpoint(Ensemble &e, float *outSub, int max_rows, const SubResult &r) {
  float tEnd = 0.0f;
  if (pbSimGetTime(e.sim, &tEnd) != PB_OK) return false;
  const bool finished = tEnd > e.members[0]->cfg->params.max_time;
  if (!outSub || !saveSubBatch(&e, outSub, max_rows, r.nrows, r.steps, finished)) {
    fprintf(stderr, "pbEnsemblePipelineRun: cannot write the checkpoint of sub-batch %d\n", e.ckptSub);
    return false;
  }
  return true;
}

bool keepStates(Pipeline *p, const Ensemble &e, int first, size_t n) {
  for (int k = 0; k < (int)e.members.size(); k++) {
    p->finalPos[first + k].resize(2 * n);
    p->finalVel[first + k].resize(2 * n);
    p->finalRad[first + k].resize(n);
    if (pbSimGetStateOf(e.sim, (unsigned)k, p->finalPos[first + k].data(), p->finalVel[first + k].data(),
                        p->finalRad[first + k].data(), nullptr, nullptr, nullptr, nullptr) != PB_OK)
      return false;
  }
  return true;
}

// Sub-batch b of the run.  Runs on the calling thread, or -- with two lanes -- on two threads that take the sub-batches
// alternately, each on its batch's own stream: a launch's ramp and drain (~13 us of every step) then overlap the
// other sub-batch's steady state.  (~Ensemble frees the sub-batch's device memory and its members.)
bool runSubBatch(Pipeline *p, int b, const RunArgs &a, SubResult &r) {
  const int first = b * p->sub;
  const int count = std::min(p->sub, p->nmembers - first);
  Ensemble e;
  const double w0 = nowSeconds();
  if (!p->takeSubBatch(first, count, e.members)) return false;
  if (!rowsFit(*e.members[0]->cfg, a)) return false;
  const double u0 = nowSeconds();
  r.waitS = u0 - w0;
  float *const outSub = a.out ? a.out + (size_t)first * a.max_rows * 4 : nullptr;
  const int nRestored = restoredMembers(e, b);
  if (nRestored < 0) return false;
  if (!p->csvDir.empty()) {
    e.csvDir = p->csvDir;
    e.csvIds.assign(p->csvIds.begin() + first, p->csvIds.begin() + first + count);
  }
  e.ckptDir = p->ckptDir;
  e.ckptSub = b;
  e.ckptFirst = first;
  if (nRestored && e.members[0]->saved->finished) {
    if (!finishedFromCheckpoint(e, outSub, a.max_rows, r)) return false;
    r.uploadS = nowSeconds() - u0;
  } else {
    if (!uploadOrRestore(e, nRestored != 0, outSub, a.max_rows, r)) return false;
    const double d0 = nowSeconds();
    r.uploadS = d0 - u0;
    if (!stepToTheEnd(e, a.max_steps, outSub, a.max_rows, r)) return false;
    if (!p->ckptDir.empty() && !finalCheckpoint(e, outSub, a.max_rows, r)) return false;
    r.deviceS = nowSeconds() - d0;
  }
  r.nbots = e.members[0]->bot->getParams().nCells;
  return !(p->keepStates && e.sim) || keepStates(p, e, first, r.nbots);
}

}  // namespace

extern "C" {

// The automatic sub-batch size (sub_batch -1) for members of `bots_per_member` bots and `producers` threads: whole
// placement rounds of the pool (every producer places one member per round; 1 ... 8 rounds) that bring a sub-batch
// to ~3 x 10^6 bots.  Measured on BASELINE configs[4] whole (1 024 members of 10^5 bots, 12 000 steps, 15 producers,
// one MI355X, end to end): sub-batches of 15 / 30 / 45 / 60 / 120 members = 96 / 90.1 / 93.3 / 97.1 / 96.0 s.  Small
// sub-batches pay a launch's ramp and drain on every step; large ones (> ~200 MB of state) leave the Infinity Cache,
// which the force kernel's neighbour reads of an evolving blob live on (and the first sub-batch is waited for).
int pbEnsemblePipelineAutoSubBatch(unsigned bots_per_member, int producers) {
  const int threads = std::max(producers, 1);
  const double want = 3.0e6 / (double)std::max(bots_per_member, 1u);
  const int rounds = std::max(1, std::min(8, (int)(want / threads + 0.5)));
  // ... but never more bots than the cache target, however many producers the host has (127 producers x 10^5 bots
  // would be 12.7 x 10^6 bots in flight over the two lanes, 4 x the target; with 10^6-bot members (ahead + 1 + lanes)
  // sub-batches of placed members are alive on the host): a pool larger than the sub-batch simply works further ahead
  const int cap = std::max(1, (int)(want + 0.5));
  return std::min(threads * rounds, std::max(cap, 1));
}

void *pbEnsemblePipelineCreateCheckpointed(const char *cfg_path, const char *common_overrides,
                                           const char **member_overrides, int nmembers, int sub_batch, int host_threads,
                                           int keep_final_states, const char *checkpoint_dir, int resume) {
  if (nmembers < 1) return nullptr;
  std::unique_ptr<Pipeline> p(new Pipeline());
  p->haveCfg = cfg_path != nullptr;
  if (cfg_path) p->cfgPath = cfg_path;
  if (common_overrides) p->common = common_overrides;
  for (int k = 0; k < nmembers; k++) p->over.emplace_back(member_overrides && member_overrides[k] ? member_overrides[k] : "");
  p->nmembers = nmembers;
  if (checkpoint_dir && checkpoint_dir[0]) p->ckptDir = checkpoint_dir;
  p->resume = resume != 0 && !p->ckptDir.empty();
  // the calling thread drives the device: leave it a core when there are several
  pbHostResources res;
  describeResources(res, host_threads);
  const unsigned avail = (unsigned)res.host_threads;
  if (res.pin_producers) {
    std::string bus;
    p->numaNode = numaOfDevice(res.device, bus, p->pinCpus);
  }
  p->tm.numa_node = res.numa_node;
  p->threads = (int)std::max(1u, std::min<unsigned>(host_threads > 0 ? avail : (avail > 1 ? avail - 1 : 1), (unsigned)nmembers));
  // sub_batch -1: pbEnsemblePipelineAutoSubBatch for members of this size (0 bots when member 0 cannot be resolved)
  PbRunConfig c0;
  const unsigned botsPerMember = c0.resolve(cfg_path, common_overrides, p->over[0].c_str()) ? c0.params.nCells : 0;
  int autoSub = pbEnsemblePipelineAutoSubBatch(botsPerMember, p->threads);
  // Members that share their placement cost the pool one placement per group, not one per member: when most members
  // are copies (a parameter sweep under a few seeds), the "whole placement rounds of the pool" bound above says
  // nothing -- a one-producer rank would step sub-batches of 4 members of 10^5 bots, paying a launch's ramp and drain
  // on a tenth of the chip -- and the cache target alone sizes the sub-batch.
  p->groupMembers();
  int distinct = (int)p->shared.size();
  for (int k : p->keyOf) distinct += k < 0 ? 1 : 0;
  if (distinct * 4 <= nmembers)
    autoSub = std::max(autoSub, pbEnsemblePipelineAutoSubBatch(botsPerMember, 1 << 20));
  // The automatic decomposition steps TWO sub-batches of half that size at the same time (a launch's ramp and drain
  // overlap the other sub-batch's steady state, and together they still fit the Infinity Cache: configs[4] slice of
  // 240 members, one pipeline of 30-member sub-batches 22.0 s, two lanes of 15 21.2 s, three of 10 21.1 s;
  // tools/experiments/two_pipelines.py).  PB_PIPELINE_LANES overrides (1: one at a time, as an explicit sub_batch).
  if (sub_batch == -1) {
    p->lanes = 2;
    if (const char *e = getenv("PB_PIPELINE_LANES")) p->lanes = std::max(1, std::min(4, atoi(e)));
    if (p->lanes > 1) autoSub = std::max(1, autoSub / p->lanes);
  }
  p->sub = sub_batch == -1 ? std::min(autoSub, nmembers) : (sub_batch < 1 || sub_batch > nmembers) ? nmembers : sub_batch;
  // a sweep resumed with the automatic size continues with the size it was started with, whatever the number of
  // producer threads is this time (the directory belongs to one decomposition)
  if (sub_batch == -1 && p->resume) (void)runInfoSubBatch(p->ckptDir, nmembers, p->sub);
  p->keepStates = keep_final_states != 0;
  p->built.resize(nmembers);
  p->ready.assign(nmembers, 0);
  if (p->keepStates) {
    p->finalPos.resize(nmembers);
    p->finalVel.resize(nmembers);
    p->finalRad.resize(nmembers);
  }
  p->tm.host_threads = p->threads;
  p->tm.sub_batch = p->sub;
  if (pbGetDevice(&p->device) != PB_OK) p->device = -1;  // (no device: the dry-run consumer of the CPU tests)
  if (!p->ckptDir.empty()) {
    (void)mkdir(checkpoint_dir, 0777);
    // a checkpoint directory belongs to ONE decomposition of the ensemble
    if (p->resume ? !checkRunInfo(p->ckptDir, nmembers, p->sub) : !startRunInfo(p->ckptDir, nmembers, p->sub)) return nullptr;
  }
  p->start();  // placement starts now, before the caller asks for the first step
  return p.release();
}

void *pbEnsemblePipelineCreate(const char *cfg_path, const char *common_overrides, const char **member_overrides,
                               int nmembers, int sub_batch, int host_threads, int keep_final_states) {
  return pbEnsemblePipelineCreateCheckpointed(cfg_path, common_overrides, member_overrides, nmembers, sub_batch,
                                              host_threads, keep_final_states, nullptr, 0);
}

void pbEnsemblePipelineDestroy(void *pv) { std::unique_ptr<Pipeline> p((Pipeline *)pv); }

int pbEnsemblePipelineHostThreads(void *pv) { return pv ? ((Pipeline *)pv)->threads : 0; }

// Every member also writes DIR/member_<id>.csv in the reference's own format (testing = 0: seed, header, one row per
// dump interval with the reference's fp32 centroid), ids[k] = the number of this pipeline's member k in the whole
// ensemble (NULL: k).  Before Run; not together with checkpoints (a resumed run could not rewrite the rows it skips).
int pbEnsemblePipelineSetCsvDir(void *pv, const char *dir, const int *ids) {
  Pipeline *p = (Pipeline *)pv;
  if (!p || p->consumedUpTo != 0 || !dir || !dir[0] || !p->ckptDir.empty()) return -1;
  (void)mkdir(dir, 0777);
  p->csvDir = dir;
  p->csvIds.resize(p->nmembers);
  for (int k = 0; k < p->nmembers; k++) p->csvIds[k] = ids ? ids[k] : k;
  return 0;
}

// Sub-batches stepped at the same time by Run (1 ... 4; before Run).  Rows and states do not depend on it.
int pbEnsemblePipelineSetLanes(void *pv, int lanes) {
  Pipeline *p = (Pipeline *)pv;
  if (!p || p->consumedUpTo != 0 || lanes < 1 || lanes > 4) return -1;
  p->lanes = lanes;
  return 0;
}

long pbEnsemblePipelineRun(void *pv, long max_steps, float *out, int max_rows, int *rows, pbEnsembleTimings *timings) {
  Pipeline *p = (Pipeline *)pv;
  if (!p || p->consumedUpTo != 0) return -1;  // one run per pipeline
  if (p->device >= 0 && pbSetDevice(p->device) != PB_OK) return -1;  // this thread may be new: batches go where Create was
  const double t0 = nowSeconds();
  const RunArgs args = {max_steps, out, max_rows};
  long steps = -1;
  int nrowsAll = 0;
  const int nsub = (p->nmembers + p->sub - 1) / p->sub;
  const int lanes = std::max(1, std::min(p->lanes, nsub));
  std::mutex resMu;            // steps / nrowsAll / the timing sums
  double waitS = 0.0, uploadS = 0.0, deviceS = 0.0;
  auto runSub = [&](int b) -> int {
    SubResult r;
    if (!runSubBatch(p, b, args, r)) return -1;
    // account: every sub-batch must have run the same steps and rows
    std::lock_guard<std::mutex> lock(resMu);
    p->nbots = r.nbots;
    if (steps < 0) {
      steps = r.steps;
      nrowsAll = r.nrows;
    } else if (r.steps != steps || r.nrows != nrowsAll) {
      fprintf(stderr, "pbEnsemblePipelineRun: sub-batches disagree on the step or row count (%ld/%d vs %ld/%d)\n", r.steps,
              r.nrows, steps, nrowsAll);
      return -1;
    }
    waitS += r.waitS, uploadS += r.uploadS, deviceS += r.deviceS;
    p->tm.sub_batches++;
    return 0;
  };
  if (lanes == 1) {
    for (int b = 0; b < nsub; b++)
      if (runSub(b) != 0) return -1;
  } else {
    std::atomic<int> next{0};
    std::atomic<bool> bad{false};
    auto lane = [&](bool setDevice) {
      if (setDevice && p->device >= 0 && pbSetDevice(p->device) != PB_OK) bad = true;
      for (int b; !bad && (b = next++) < nsub;)
        if (runSub(b) != 0) {
          bad = true;
          std::lock_guard<std::mutex> lock(p->mu);  // (wake a lane that waits for members)
          p->failed = true;
          p->cvReady.notify_all();
          p->cvRoom.notify_all();
        }
    };
    std::vector<std::thread> extra;
    for (int l = 1; l < lanes; l++) extra.emplace_back(lane, true);
    lane(false);
    for (std::thread &t : extra) t.join();
    if (bad) return -1;
  }
  // (per lane: the lanes wait, upload and step at the same time)
  p->tm.placement_wait_s = waitS / lanes, p->tm.upload_s = uploadS / lanes, p->tm.device_s = deviceS / lanes;
  p->tm.lanes = lanes;
  p->tm.wall_s = nowSeconds() - t0;
  p->tm.placement_cpu_s = p->tm.placement_thread_wall_s = 0.0;
  for (double c : p->cpuSeconds) p->tm.placement_cpu_s += c;
  for (double c : p->wallSeconds) p->tm.placement_thread_wall_s += c;
  {
    std::lock_guard<std::mutex> lock(p->mu);
    p->tm.placements_run = p->placementsRun, p->tm.placements_shared = p->placementsShared;
  }
  if (rows) *rows = nrowsAll;
  if (timings) *timings = p->tm;
  return steps;
}

// The consumer side WITHOUT a device (CPU tests of the pipeline's ordering): takes the sub-batches in order through
// the same Pipeline::takeSubBatch as Run, and instead of stepping them records, per member, a checksum of the placed
// state (positions, radii, dead flags) and dwells `dwell_ms` per sub-batch so that the producers run into the
// look-ahead bound.  *max_ahead receives the largest number of members that were ever claimed by producers beyond the
// consumed ones.
int pbEnsemblePipelineDryRun(void *pv, int dwell_ms, unsigned long long *checksums, int *max_ahead) {
  Pipeline *p = (Pipeline *)pv;
  if (!p || p->consumedUpTo != 0 || !checksums) return -1;
  int worst = 0;
  for (int first = 0; first < p->nmembers; first += p->sub) {
    const int count = std::min(p->sub, p->nmembers - first);
    std::vector<std::unique_ptr<Member>> mine;
    if (!p->takeSubBatch(first, count, mine, &worst)) return -1;
    for (int k = 0; k < count; k++) {
      const Particlebot *b = mine[k]->bot.get();
      const size_t n = b->getParams().nCells;
      p->nbots = (unsigned)n;
      unsigned long long h = 1469598103934665603ull;
      auto mix = [&](const void *data, size_t bytes) {
        const unsigned char *c = (const unsigned char *)data;
        for (size_t i = 0; i < bytes; i++) h = (h ^ c[i]) * 1099511628211ull;
      };
      mix(b->hostPositions(), 8 * n);
      mix(b->hostRadii(), 4 * n);
      mix(b->hostDead(), 4 * n);
      checksums[first + k] = h;
      mine[k].reset();
    }
    if (dwell_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(dwell_ms));
    {
      std::lock_guard<std::mutex> lock(p->mu);
      worst = std::max(worst, p->nextToBuild - p->consumedUpTo);
    }
  }
  if (max_ahead) *max_ahead = worst;
  return 0;
}

unsigned pbEnsemblePipelineNumBots(void *pv) { return ((Pipeline *)pv)->nbots; }

void pbEnsemblePipelinePlacementCounts(void *pv, int *run, int *shared) {
  Pipeline *p = (Pipeline *)pv;
  if (!p) return;
  std::lock_guard<std::mutex> lock(p->mu);
  if (run) *run = p->placementsRun;
  if (shared) *shared = p->placementsShared;
}

int pbEnsemblePipelineGetState(void *pv, int member, float *pos, float *vel, float *rad) {
  Pipeline *p = (Pipeline *)pv;
  if (!p || !p->keepStates || member < 0 || member >= p->nmembers || p->finalRad[member].empty()) return 1;
  const size_t n = p->nbots;
  if (pos) memcpy(pos, p->finalPos[member].data(), 8 * n);
  if (vel) memcpy(vel, p->finalVel[member].data(), 8 * n);
  if (rad) memcpy(rad, p->finalRad[member].data(), 4 * n);
  return 0;
}

}  // extern "C"
