// pb_ensemble.hpp -- what the units of the ensemble layer share (pb_ensemble.cpp, pb_ensemble_ckpt.cpp,
// pb_ensemble_pipeline.cpp, pb_host_resources.cpp).  Internal to libparticlebot_host.so and not installed: the
// public surface is include/particlebot_ensemble.h.
#pragma once

#include <sched.h>

#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "particlebot.h"
#include "particlebot_ensemble.h"
#include "pb_config.hpp"

#pragma GCC visibility push(hidden)  // (the library's exported symbols are a fixed list)

// what an ensemble checkpoint holds of one member beyond the host mirrors (pbEnsemblePipelineSetCheckpoint)
struct MemberSaved {
  float time = 0.0f;
  unsigned draws = 0;
  int sorted = 0, finished = 0, nrows = 0;
  long steps = 0;
  std::vector<float> rows, absA, absR;
  std::vector<unsigned> orig, keys;
};

// one member: its resolved configuration and the HostOnly object that places it and draws its dead set
struct Member {
  std::unique_ptr<PbRunConfig> cfg;
  std::unique_ptr<Particlebot> bot;
  bool deadDrawn = false;              // the dead set was drawn with the placement (a draw due at time 0)
  std::unique_ptr<MemberSaved> saved;  // restored from a checkpoint instead of placed
};

// A batch of members on the device: ONE pbSim, one launch per timestep.
struct Ensemble {
  std::vector<std::unique_ptr<Member>> members;
  pbSim *sim = nullptr;
  bool haveRow = false;  // runSteps: a summary row has been written at time rowTime
  float rowTime = 0.0f;
  // checkpointing (pipeline): directory, this sub-batch's number and first member, steps done before this call
  std::string ckptDir;
  int ckptSub = 0, ckptFirst = 0, ckptGen = 0;
  long stepsBefore = 0;
  // per-member CSV files in the reference's own format (pbEnsemblePipelineSetCsvDir): directory, the members' numbers
  // in the whole ensemble, the open files
  std::string csvDir;
  std::vector<int> csvIds;
  std::vector<FILE *> csvFiles;
  ~Ensemble() {
    for (FILE *f : csvFiles)
      if (f) fclose(f);
    if (sim) pbSimDestroy(sim);
  }
};

// ---- pb_ensemble.cpp ----------------------------------------------------------------------------------------------
// Host side of one member: configuration and a HostOnly Particlebot; false if the .cfg cannot be read
bool configureMember(Member &m, const char *cfg_path, const char *common_overrides, const char *own_overrides);
// ... plus placement and the early dead draw.  `shared`: a placement another member with the same
// Particlebot::placementKey() produced (installed instead of reset()); `out`: capture this member's own.
bool buildMember(Member &m, const char *cfg_path, const char *common_overrides, const char *own_overrides,
                 const Particlebot::Placement *shared = nullptr, Particlebot::Placement *out = nullptr);
// Members whose placement inputs agree (Particlebot::placementKeyOf of their resolved configurations) form a group:
// the lowest-numbered member places, the others import.  keyOf[k] = member k's group, or -1: nobody shares its key
// (groups of one are not groups), its configuration does not load (it fails where it is built), or sharing is off
// (PB_SHARE_PLACEMENTS=0; read here and nowhere else).  Returns the number of groups.
int groupPlacements(const char *cfg_path, const char *common_overrides, int nmembers,
                    const std::function<const char *(int)> &ownOverrides, std::vector<int> &keyOf);
// device side: create the batched pbSim of already built members and upload their initial state
bool uploadEnsemble(Ensemble *e);
// rows a run from t = 0 writes in at most max_steps steps; stops counting at limit + 1
long rowsNeeded(float dt, float di, float max_time, long max_steps, long limit);
long runSteps(Ensemble *e, long max_steps, float *out, int max_rows, int *rows);

// ---- pb_ensemble_ckpt.cpp (the file format is described there) ----------------------------------------------------
bool readManifest(const std::string &dir, int sub, int &gen, int &nrows, int &finished, long &steps);
// run.info ties a directory to ONE decomposition: the sub-batch size it was started with, if it matches nmembers;
// the check on resume (message on stderr); the fresh start (also clears an earlier run's manifests)
bool runInfoSubBatch(const std::string &dir, int nmembers, int &sub);
bool checkRunInfo(const std::string &dir, int nmembers, int sub);
bool startRunInfo(const std::string &dir, int nmembers, int sub);
// writes generation (ckptGen ^ 1) of every member of the batch (state as of now, `nrows` rows each), then the manifest
bool saveSubBatch(Ensemble *e, const float *out, int max_rows, int nrows, long steps, bool finished);
// the member's file of generation gen -> m.saved (+ host mirrors, generator, dead-draw flag); false if unusable
bool loadMemberFile(Member &m, const std::string &dir, int k, int gen, int wantRows, long steps);
// device side of a sub-batch whose members were restored from a checkpoint (all from the same row)
bool uploadRestored(Ensemble *e, float *out, int max_rows);

// ---- pb_host_resources.cpp ----------------------------------------------------------------------------------------
void describeResources(pbHostResources &r, int wanted);
int numaOfDevice(int device, std::string &busId, std::vector<int> &cpus);
unsigned hostThreads(int wanted);  // host threads for placement: this rank's share of the cores it may really use
double threadCpuSeconds();
double nowSeconds();

#pragma GCC visibility pop
