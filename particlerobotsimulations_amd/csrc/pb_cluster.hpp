// pb_cluster.hpp -- what pb_cluster.hip shares with pb_contacts.hip and pb_structure.hip: the scratch object, the fresh
// grid, the front end that files the bots (rmax, hash, sort, gather, cell starts) and the link pass on top of it.
#pragma once

#include "pb_engine.hpp"

struct PbClusterScratch {
  uint32_t *keys[2] = {nullptr, nullptr}, *vals[2] = {nullptr, nullptr}, *hist = nullptr;
  float4 *cpr = nullptr;        // total + 2: sorted posrad, .w = global original index
  uint32_t *start = nullptr;    // nsims * cells + 1
  uint32_t *parent = nullptr, *degree = nullptr, *size = nullptr;  // total each, ORIGINAL order
  uint32_t *labels = nullptr;   // n: one member's labels
  unsigned long long *acc = nullptr;  // 4 words per member
  pbClusterStats *rows = nullptr;     // nsims
  uint32_t *flag = nullptr;           // [0] changed, [1] rmax bits
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  uint32_t gxLog2 = 2, gyLog2 = 2;
  unsigned long long analyses = 0;
  float lastMs = 0.0f;
  unsigned rounds = 0;
  // what the last analysis left behind for the contact export (pb_contacts.hip)
  double invCell = 0.0;  // the grid's 1 / edge
  int sortedIn = 0;      // vals[sortedIn] holds the slots in sorted order
  // contact export (pb_contacts.hip): allocated by the first export, links grown when a call needs more
  uint32_t *cOffsets = nullptr;              // n + 1, ORIGINAL order
  unsigned long long *cParts = nullptr;      // ceil(n / 256) + 2: block sums, then [blocks] the total, [blocks + 1] the flag
  float2 *cVel = nullptr;                    // n: the member's velocities in sorted order
  float2 *cPos = nullptr;                    // n: the member's positions in ORIGINAL order
  double *cVirial = nullptr;                 // 4 n, ORIGINAL order
  uint4 *cLinks = nullptr;                   // cLinksCap entries of 16 bytes (pbContactLink)
  unsigned long long cLinksCap = 0;
  hipEvent_t cEv1 = nullptr;                 // the export's last launch (its first is the front end's ev0)
  unsigned long long exports = 0;
  float lastExportMs = 0.0f;
  // structure analysis (pb_structure.hip): allocated by the first call that needs each, counts grown with bins
  unsigned long long *sCounts = nullptr;     // nsims * sCountsBins: the radial histograms
  unsigned sCountsBins = 0;
  long long *sRe = nullptr, *sIm = nullptr;  // total each, ORIGINAL order: per-bot sums of qre, qim
  uint32_t *sNb = nullptr;                   // total, ORIGINAL order: neighbours
  pbStructureStats *sRows = nullptr;         // nsims
  double *sPsi = nullptr;                    // 2 n: one member's psi6
  hipEvent_t sEv1 = nullptr;                 // the analysis' last launch (its first is the front end's ev0)
  unsigned long long structures = 0;
  float lastStructureMs = 0.0f;
};

namespace {

constexpr int CT = 256;

struct ClusterGrid {
  double invCell;
  uint32_t gxLog2, gyLog2;
};

// the grid the last pbClusterFile left in the scratch object
inline ClusterGrid gridOf(const PbClusterScratch *C) {
  ClusterGrid G;
  G.invCell = C->invCell;
  G.gxLog2 = C->gxLog2, G.gyLog2 = C->gyLog2;
  return G;
}

PB_DEV bool finitePosRad(const float4 &q) {
  const float inf = __builtin_inff();
  return fabsf(q.x) < inf && fabsf(q.y) < inf && fabsf(q.z) < inf;
}

// floor(v) as an int, clamped so that positions outside the guaranteed range convert without overflow
PB_DEV int cellCoord(double v) {
  const double f = floor(v);
  return (int)fmin(fmax(f, -1073741824.0), 1073741824.0);
}

PB_DEV uint32_t cellX(const ClusterGrid &G, float x) {
  return (uint32_t)cellCoord((double)x * G.invCell) & ((1u << G.gxLog2) - 1u);
}
PB_DEV uint32_t cellY(const ClusterGrid &G, float y) {
  return (uint32_t)cellCoord((double)y * G.invCell) & ((1u << G.gyLog2) - 1u);
}

}  // namespace

// The filing front end: records ev0, files every bot of the batch on a wrapped power-of-two grid of edge
// (perRmax * rmax + reach) (1 + 2^-10), never below 2^-8 (rmax: the largest finite radius, reduced on the device and
// read back only when perRmax != 0), and leaves cpr (sorted posrad, .w = global original index), the cell starts,
// vals[sortedIn], parent[o] = o and size[o] = 0 on the device, the grid (invCell, gxLog2, gyLog2) in the scratch object.
// Allocates the scratch on first use.  Launches are queued on the batch's stream, not waited for.       pb_cluster.hip
int pbClusterFile(pbSim *S, double reach, double perRmax);
// The whole cluster pipeline (the front end with reach = gap, perRmax = 2); leaves cpr, the cell starts, parent (roots),
// degree and the rows on the device and the stream drained.                                             pb_cluster.hip
int pbClusterAnalyse(pbSim *S, float gap);
// the argument checks the entry points share; nothing here touches the device (the batch check reads the host-side
// batch object, so it needs a real handle)
int pbClusterCheckGap(const char *fn, float gap);
int pbClusterCheckBatch(const char *fn, const pbSim *S);
// frees the contact export's buffers, if any (pbClusterFree)                                           pb_contacts.hip
void pbContactsFree(PbClusterScratch *C);
// frees the structure analysis' buffers, if any (pbClusterFree)                                       pb_structure.hip
void pbStructureFree(PbClusterScratch *C);
