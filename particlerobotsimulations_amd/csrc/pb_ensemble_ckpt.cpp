// pb_ensemble_ckpt.cpp -- ensemble checkpoints (pbEnsemblePipelineSetCheckpoint): the files of a checkpoint directory.
// DIR/run.info          "members N sub_batch S": the one decomposition of the ensemble the directory belongs to
// DIR/sub_<b>.manifest  "generation rows finished steps" of sub-batch b, written (tmp + rename) AFTER the member files
//                       of that generation are complete: the members of one sub-batch share a clock, so a
//                       checkpoint is only usable when all of them are from the same row
// DIR/member_<k>.<generation>  header, the member's summary rows so far and -- unless it has finished -- every state
//                       array, the stale slot layout and both generators (the exact checkpoint of class Particlebot,
//                       per member of a batch).  Generations alternate 0/1 so that the previous complete one survives
//                       a kill in the middle of writing the next.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "pb_ensemble.hpp"

namespace {

struct MemberFileHeader {
  char magic[8];
  uint32_t nbots;
  float time;
  uint32_t draws;
  int32_t rngKind, sorted, deadDrawn, nrows, finished;
  int32_t rs[36];
};
const char kMemberMagic[8] = {'P', 'B', 'E', 'N', 'S', 'M', '1', 0};

std::string memberPath(const std::string &dir, int k, int gen) {
  char name[64];
  snprintf(name, sizeof name, "/member_%06d.%d", k, gen);
  return dir + name;
}
std::string manifestPath(const std::string &dir, int sub) {
  char name[64];
  snprintf(name, sizeof name, "/sub_%06d.manifest", sub);
  return dir + name;
}
std::string runInfoLine(int nmembers, int sub) {
  char line[128];
  snprintf(line, sizeof line, "members %d sub_batch %d\n", nmembers, sub);
  return line;
}

template <class T>
bool putv(FILE *fp, const T *p, size_t count) { return fwrite(p, sizeof(T), count, fp) == count; }
template <class T>
bool getv(FILE *fp, T *p, size_t count) { return fread(p, sizeof(T), count, fp) == count; }

// The state arrays of an unfinished member of n bots, in FILE ORDER: io(array, elements) for each until one fails.
// saveSubBatch writes through it and loadMemberFile reads through it, so the two cannot disagree on the order.
struct StateArrays {
  float *pos, *vel, *rad, *phase;
  int *dead;
  float *absA, *absR;
  unsigned *orig, *keys;
};
template <class Io>
bool eachStateArray(const StateArrays &a, size_t n, Io io) {
  return io(a.pos, 2 * n) && io(a.vel, 2 * n) && io(a.rad, n) && io(a.phase, n) && io(a.dead, n) && io(a.absA, n) &&
         io(a.absR, n) && io(a.orig, n) && io(a.keys, n);
}

// dest appears complete or not at all: written as dest.tmp (`body` says whether its writes succeeded; so must fclose),
// then renamed
template <class Body>
bool writeThenRename(const std::string &dest, const char *mode, Body body) {
  const std::string tmp = dest + ".tmp";
  FILE *f = fopen(tmp.c_str(), mode);
  bool ok = f && body(f);
  if (f) ok = (fclose(f) == 0) && ok;
  return ok && rename(tmp.c_str(), dest.c_str()) == 0;
}

}  // namespace

bool readManifest(const std::string &dir, int sub, int &gen, int &nrows, int &finished, long &steps) {
  FILE *f = fopen(manifestPath(dir, sub).c_str(), "r");
  if (!f) return false;
  const bool ok = fscanf(f, "%d %d %d %ld", &gen, &nrows, &finished, &steps) == 4 && (gen == 0 || gen == 1) &&
                  nrows >= 0 && nrows <= (1 << 24) && steps >= 0;
  fclose(f);
  return ok;
}

bool runInfoSubBatch(const std::string &dir, int nmembers, int &sub) {
  int m0 = 0, s0 = 0;
  FILE *f = fopen((dir + "/run.info").c_str(), "r");
  const bool ok = f && fscanf(f, "members %d sub_batch %d", &m0, &s0) == 2 && m0 == nmembers && s0 >= 1 && s0 <= nmembers;
  if (f) fclose(f);
  if (ok) sub = s0;
  return ok;
}

bool checkRunInfo(const std::string &dir, int nmembers, int sub) {
  const std::string want = runInfoLine(nmembers, sub);
  char got[128] = {0};
  FILE *f = fopen((dir + "/run.info").c_str(), "r");
  const bool same = f && fgets(got, sizeof got, f) && want == got;
  if (f) fclose(f);
  if (!same)
    fprintf(stderr, "pbEnsemblePipeline: %s was written for another decomposition (%s) than this one (%s)\n", dir.c_str(),
            got, want.c_str());
  return same;
}

bool startRunInfo(const std::string &dir, int nmembers, int sub) {
  FILE *f = fopen((dir + "/run.info").c_str(), "w");
  if (!f || fputs(runInfoLine(nmembers, sub).c_str(), f) < 0 || fclose(f) != 0) {
    fprintf(stderr, "pbEnsemblePipeline: cannot write under %s\n", dir.c_str());
    return false;
  }
  // (manifests of an earlier run in the same directory must not be mistaken for this run's)
  for (int b = 0; b * sub < nmembers; b++) (void)remove(manifestPath(dir, b).c_str());
  return true;
}

bool loadMemberFile(Member &m, const std::string &dir, int k, int gen, int wantRows, long steps) {
  FILE *f = fopen(memberPath(dir, k, gen).c_str(), "rb");
  if (!f) return false;
  MemberFileHeader h;
  const size_t n = m.bot->getParams().nCells;
  std::unique_ptr<MemberSaved> sv(new MemberSaved());
  bool ok = getv(f, &h, 1) && memcmp(h.magic, kMemberMagic, 8) == 0 && h.nbots == n && h.nrows == wantRows &&
            h.rngKind == m.cfg->rng_kind;
  if (ok) {
    sv->rows.resize((size_t)h.nrows * 4);
    ok = getv(f, sv->rows.data(), sv->rows.size());
  }
  if (ok && !h.finished) {
    std::vector<float> pos(2 * n), vel(2 * n), rad(n), phase(n);
    std::vector<int> dead(n);
    sv->absA.resize(n), sv->absR.resize(n), sv->orig.resize(n), sv->keys.resize(n);
    const StateArrays arrays = {pos.data(),      vel.data(),      rad.data(),      phase.data(),   dead.data(),
                                sv->absA.data(), sv->absR.data(), sv->orig.data(), sv->keys.data()};
    ok = eachStateArray(arrays, n, [&](auto *p, size_t count) { return getv(f, p, count); });
    if (ok) m.bot->restoreHostMirrors(pos.data(), vel.data(), rad.data(), phase.data(), dead.data());
  }
  fclose(f);
  if (!ok) return false;
  sv->time = h.time, sv->draws = h.draws, sv->sorted = h.sorted, sv->finished = h.finished, sv->nrows = h.nrows;
  sv->steps = steps;
  m.bot->setHostRngState(h.rs);
  m.bot->setHostTime(h.time);
  m.deadDrawn = h.deadDrawn != 0;
  m.saved = std::move(sv);
  return true;
}

bool saveSubBatch(Ensemble *e, const float *out, int max_rows, int nrows, long steps, bool finished) {
  const int m = (int)e->members.size();
  const int gen = e->ckptGen ^ 1;
  const size_t n = e->members[0]->bot->getParams().nCells;
  float t = 0.0f;
  unsigned draws = 0;
  if (pbSimGetTime(e->sim, &t) != PB_OK || pbSimGetPhaseDraws(e->sim, &draws) != PB_OK) return false;
  std::vector<float> pos(2 * n), vel(2 * n), rad(n), phase(n), absA(n), absR(n);
  std::vector<int> dead(n);
  std::vector<unsigned> orig(n), keys(n);
  const StateArrays arrays = {pos.data(),  vel.data(),  rad.data(),  phase.data(), dead.data(),
                              absA.data(), absR.data(), orig.data(), keys.data()};
  pbSimConfig conf;
  if (pbSimGetConfig(e->sim, &conf) != PB_OK) return false;
  for (int k = 0; k < m; k++) {
    MemberFileHeader h;
    memcpy(h.magic, kMemberMagic, 8);
    h.nbots = (uint32_t)n, h.time = t, h.draws = draws, h.rngKind = e->members[k]->cfg->rng_kind;
    h.deadDrawn = e->members[k]->deadDrawn ? 1 : 0, h.nrows = nrows, h.finished = finished ? 1 : 0;
    int sorted = 0;
    if (!finished) {
      if (pbSimGetStateOf(e->sim, (unsigned)k, pos.data(), vel.data(), rad.data(), phase.data(), dead.data(), absA.data(),
                          absR.data()) != PB_OK ||
          pbSimGetLayoutOf(e->sim, (unsigned)k, orig.data(), keys.data(), &sorted) != PB_OK)
        return false;
      if (!conf.attraction_sums) std::fill(absA.begin(), absA.end(), 0.0f);  // (not maintained: never NaN on disk)
    }
    h.sorted = sorted;
    e->members[k]->bot->getHostRngState(h.rs);
    if (!writeThenRename(memberPath(e->ckptDir, e->ckptFirst + k, gen), "wb", [&](FILE *f) {
          return putv(f, &h, 1) && putv(f, out + (size_t)k * max_rows * 4, (size_t)nrows * 4) &&
                 (finished || eachStateArray(arrays, n, [&](const auto *p, size_t count) { return putv(f, p, count); }));
        }))
      return false;
  }
  if (!writeThenRename(manifestPath(e->ckptDir, e->ckptSub), "w",
                       [&](FILE *f) { return fprintf(f, "%d %d %d %ld\n", gen, nrows, finished ? 1 : 0, steps) > 0; }))
    return false;
  e->ckptGen = gen;
  return true;
}

bool uploadRestored(Ensemble *e, float *out, int max_rows) {
  if (!uploadEnsemble(e)) return false;  // (the host mirrors hold the restored state)
  const int m = (int)e->members.size();
  const MemberSaved &s0 = *e->members[0]->saved;
  for (int k = 0; k < m; k++) {
    const MemberSaved &sv = *e->members[k]->saved;
    if (sv.time != s0.time || sv.draws != s0.draws || sv.sorted != s0.sorted || sv.nrows != s0.nrows) return false;
    if (sv.sorted && pbSimSetLayoutOf(e->sim, (unsigned)k, sv.orig.data(), sv.keys.data()) != PB_OK) return false;
  }
  for (int k = 0; k < m; k++) {
    // (the layout is installed once every member has provided one: the state goes in afterwards, in that order)
    const Member &mk = *e->members[k];
    const Particlebot *b = mk.bot.get();
    if (pbSimSetStateOf(e->sim, (unsigned)k, b->hostPositions(), b->hostVelocities(), b->hostRadii(), b->hostPhases(),
                        b->hostDead()) != PB_OK ||
        pbSimSetForcesOf(e->sim, (unsigned)k, mk.saved->absA.data(), mk.saved->absR.data()) != PB_OK)
      return false;
    if (out) memcpy(out + (size_t)k * max_rows * 4, mk.saved->rows.data(), sizeof(float) * mk.saved->rows.size());
  }
  if (pbSimSetTime(e->sim, s0.time) != PB_OK || pbSimSetPhaseDraws(e->sim, s0.draws) != PB_OK) return false;
  e->haveRow = true;  // the row at the checkpoint's time is among the restored ones
  e->rowTime = s0.time;
  e->stepsBefore = s0.steps;
  return true;
}
