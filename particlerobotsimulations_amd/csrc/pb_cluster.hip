// pb_cluster.hip -- cluster analysis on gfx950: the connected components of every member's contact graph, from the
// engine's resident state (pbSimClusterStats / pbSimClusterLabelsOf, include/particlebot_hip.h has the definition).
//
// The engine's own cell lists are stale between re-sorts, so the analysis files the bots afresh, in scratch of its
// own, and leaves the simulation untouched.  The filing front end (pbClusterFile: the first five kernels below) takes
// the cell edge and also serves the contact export, the structure analysis and the rearrangement analysis
// (pb_contacts.hip, pb_structure.hip, pb_dynamics.hip).
// For the whole batch at once:
//   k_cluster_rmax      the largest finite radius (bit-pattern max, one atomic per workgroup), 4 bytes read back
//   k_cluster_hash      key = member * cells + cell of a wrapped power-of-two grid whose edge is a little more than
//                       2 rmax + linkGap; the cell index is floor(x / edge) in fp64, whose rounding (2^-24 of a cell for
//                       |x| <= 2^20 and the smallest edge) is far inside the edge's 2^-10 margin: a linked pair is
//                       never further apart than one cell.  Wrapping only folds distant bots into one list.
//   pbRadixSortPairs    (pb_sort.hip) slots by key
//   k_cluster_gather    posrad in sorted order with the GLOBAL original index in .w; a bot with a non-finite position
//                       or radius becomes a NaN position, which no comparison links; parent[o] = o, size[o] = 0
//   k_cluster_starts    dense cell starts: a lower bound in the sorted keys per cell (as k_cell_scan)
//   k_cluster_links     the hot path: one bot per lane over the nine cells (pbWalkNine, pb_cluster.hpp: three slot
//                       ranges away from the x-wrap, the next neighbour's posrad in flight); evaluates the link rule
//                       (pbWhenLinked, pb_cluster.hpp), counts the degree and hooks
//                       every link once (from its larger index) into a union-find forest over original indices:
//                       find with path halving, hook the larger root under the smaller with atomicCAS.  Roots only
//                       ever get smaller, so a component's root is its smallest original index: the label.
//   k_cluster_compress  every bot follows its chain to the root and points at it; repeated until a device flag says
//                       nothing changed (4 bytes read back per round; the forest is shallow after path halving).  A
//                       pass chases all the way to the root, so the second pass normally finds nothing to do and
//                       pbClusterStats.rounds is 3: the hook round, one pass that moves pointers, one that confirms
//   k_cluster_sizes     size[root] += 1, lanes of a wave that share a root combined into one atomic
//   k_cluster_reduce    per member: roots, the largest (size, smallest label) as one 64-bit max, isolated bots, the
//                       degree sum and maximum; wave shuffles, LDS, one set of atomics per workgroup
//   k_cluster_rows      one 32-byte pbClusterStats row per member
//   k_cluster_labels    one member's labels, local indices (pbSimClusterLabelsOf)
// No LDS beyond the reduction's few words, no scratch memory.
#include <string.h>

#include "pb_cluster.hpp"

namespace {

constexpr unsigned MAX_ROUNDS = 1024;

__global__ __launch_bounds__(CT) void k_cluster_rmax(const float4 *__restrict__ pr, uint32_t total,
                                                     uint32_t *__restrict__ out) {
  __shared__ uint32_t part[CT / 64];
  uint32_t best = 0u;  // bit pattern of the largest finite positive radius: such floats order like their bits
  for (uint32_t s = blockIdx.x * CT + threadIdx.x; s < total; s += gridDim.x * CT) {
    const float r = pr[s].z;
    if (r > 0.0f && r < __builtin_inff()) {
      const uint32_t b = __float_as_uint(r);
      best = b > best ? b : best;
    }
  }
  best = waveMaxU32(best);
  if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < CT / 64; w++) best = part[w] > best ? part[w] : best;
    if (best) atomicMax(out, best);
  }
}

__global__ __launch_bounds__(CT) void k_cluster_hash(const float4 *__restrict__ pr, uint32_t n, ClusterGrid G,
                                                     uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  if (l >= n) return;
  const uint32_t s = blockIdx.y * n + l;
  const float4 q = pr[s];
  uint32_t cell = 0u;
  if (finitePosRad(q)) cell = (cellY(G, q.y) << G.gxLog2) | cellX(G, q.x);
  keys[s] = (blockIdx.y << (G.gxLog2 + G.gyLog2)) + cell;
  vals[s] = s;
}

__global__ __launch_bounds__(CT) void k_cluster_gather(const float4 *__restrict__ pr, const uint32_t *__restrict__ orig,
                                                       const uint32_t *__restrict__ sortedSlots, uint32_t n,
                                                       float4 *__restrict__ cpr, uint32_t *__restrict__ parent,
                                                       uint32_t *__restrict__ size) {
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  if (l >= n) return;
  const uint32_t base = blockIdx.y * n, t = base + l;
  const uint32_t src = sortedSlots[t];  // keys carry the member: src stays inside this member's block
  float4 q = pr[src];
  const uint32_t o = base + orig[src];
  if (!finitePosRad(q)) q.x = q.y = __builtin_nanf("");
  q.w = __uint_as_float(o);
  cpr[t] = q;
  parent[o] = o;
  size[o] = 0u;
}

__global__ __launch_bounds__(CT) void k_cluster_starts(const uint32_t *__restrict__ sortedKeys, uint32_t total,
                                                       uint32_t numKeys, uint32_t *__restrict__ start) {
  const uint32_t c = blockIdx.x * CT + threadIdx.x;
  if (c > numKeys) return;
  uint32_t lo = 0, hi = total;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (sortedKeys[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  start[c] = lo;
}

// The forest is read and written by many lanes at once: relaxed atomic accesses (plain vector loads and stores that the
// compiler may not cache or tear).  Every value ever stored in parent[v] is an ancestor of v and at most v.
PB_DEV uint32_t ldRelaxed(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
PB_DEV void stRelaxed(uint32_t *p, uint32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

// the root of x, halving the path on the way (a root is never written here: only the hook's atomicCAS changes one)
PB_DEV uint32_t findRoot(uint32_t *__restrict__ parent, uint32_t x) {
  uint32_t curr = ldRelaxed(parent + x);
  if (curr != x) {
    uint32_t prev = x, next;
    while (curr > (next = ldRelaxed(parent + curr))) {
      stRelaxed(parent + prev, next);
      prev = curr;
      curr = next;
    }
  }
  return curr;
}

PB_DEV void hook(uint32_t *__restrict__ parent, uint32_t a, uint32_t b) {
  a = findRoot(parent, a);
  b = findRoot(parent, b);
  while (a != b) {
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicCAS(parent + a, a, b);  // a > b: the larger root goes under the smaller
    if (old == a) break;
    a = old;  // a was no root any more: climb from what it points at
  }
}

__global__ __launch_bounds__(CT) void k_cluster_links(const float4 *__restrict__ cpr, const uint32_t *__restrict__ start,
                                                      uint32_t n, ClusterGrid G, float gap,
                                                      uint32_t *__restrict__ parent, uint32_t *__restrict__ degree) {
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  if (l >= n) return;
  const uint32_t t = blockIdx.y * n + l;
  const float4 me = cpr[t];
  const uint32_t o = __float_as_uint(me.w);
  uint32_t deg = 0u;
  if (me.x == me.x) {  // a bot with a non-finite position or radius has no links
    pbWalkNine<false>(cpr, start, blockIdx.y, G, t, me, [&](uint32_t j, const float4 &q, float, float, float d2) {
      pbWhenLinked(t, me, j, q, d2, gap, [&](float, float) {
        deg++;
        const uint32_t oj = __float_as_uint(q.w);
        if (oj < o) hook(parent, o, oj);
      });
    });
  }
  degree[o] = deg;
}

__global__ __launch_bounds__(CT) void k_cluster_compress(uint32_t *__restrict__ parent, uint32_t total,
                                                         uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * CT + threadIdx.x;
  bool changed = false;
  if (i < total) {
    const uint32_t p = ldRelaxed(parent + i);
    uint32_t r = p, g;
    while ((g = ldRelaxed(parent + r)) != r) r = g;
    if (r != p) {
      stRelaxed(parent + i, r);
      changed = true;
    }
  }
  if (__any(changed) && (threadIdx.x & 63u) == 0u) stRelaxed(flag, 1u);
}

__global__ __launch_bounds__(CT) void k_cluster_sizes(const uint32_t *__restrict__ parent, uint32_t total,
                                                      uint32_t *__restrict__ size) {
  const uint32_t i = blockIdx.x * CT + threadIdx.x;
  bool todo = i < total;
  const uint32_t r = todo ? parent[i] : 0u;
  // neighbours in original order mostly share a root: the lanes that share the first pending lane's root add once
#pragma unroll 1
  for (int turn = 0; turn < 4; turn++) {
    const unsigned long long pending = __ballot(todo);
    if (!pending) return;
    const int lead = __ffsll((long long)pending) - 1;
    const uint32_t r0 = (uint32_t)__shfl((int)r, lead);
    const bool mine = todo && r == r0;
    const unsigned long long group = __ballot(mine);
    if (mine) {
      if ((int)(threadIdx.x & 63u) == lead) atomicAdd(size + r0, (uint32_t)__popcll(group));
      todo = false;
    }
  }
  if (todo) atomicAdd(size + r, 1u);
}

// acc[4 m + 0] (size << 32 | ~label) of the best root, [1] degree sum, [2] roots | isolated << 32, [3] max degree
__global__ __launch_bounds__(CT) void k_cluster_reduce(const uint32_t *__restrict__ parent,
                                                       const uint32_t *__restrict__ size,
                                                       const uint32_t *__restrict__ degree, uint32_t n,
                                                       unsigned long long *__restrict__ acc) {
  __shared__ unsigned long long sBest[CT / 64], sDeg[CT / 64];
  __shared__ uint32_t sRoots[CT / 64], sIso[CT / 64], sMax[CT / 64];
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  const uint32_t i = blockIdx.y * n + l;
  unsigned long long best = 0ull, degSum = 0ull;
  uint32_t roots = 0u, iso = 0u, maxDeg = 0u;
  if (l < n) {
    if (parent[i] == i) {
      roots = 1u;
      best = ((unsigned long long)size[i] << 32) | (unsigned long long)(0xFFFFFFFFu - l);
    }
    const uint32_t d = degree[i];
    degSum = d;
    maxDeg = d;
    iso = d == 0u ? 1u : 0u;
  }
  best = waveMaxU64(best);
  degSum = waveSumU64(degSum);
  roots = waveSumU32(roots);
  iso = waveSumU32(iso);
  maxDeg = waveMaxU32(maxDeg);
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) sBest[w] = best, sDeg[w] = degSum, sRoots[w] = roots, sIso[w] = iso, sMax[w] = maxDeg;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < CT / 64; k++) {
      best = sBest[k] > best ? sBest[k] : best;
      degSum += sDeg[k];
      roots += sRoots[k];
      iso += sIso[k];
      maxDeg = sMax[k] > maxDeg ? sMax[k] : maxDeg;
    }
    unsigned long long *a = acc + 4u * (size_t)blockIdx.y;
    if (best) atomicMax(a + 0, best);
    if (degSum) atomicAdd(a + 1, degSum);
    if (roots | iso) atomicAdd(a + 2, (unsigned long long)roots | ((unsigned long long)iso << 32));
    if (maxDeg) atomicMax(a + 3, (unsigned long long)maxDeg);
  }
}

__global__ __launch_bounds__(CT) void k_cluster_rows(const unsigned long long *__restrict__ acc, uint32_t nsims,
                                                     unsigned rounds, pbClusterStats *__restrict__ rows) {
  const uint32_t m = blockIdx.x * CT + threadIdx.x;
  if (m >= nsims) return;
  const unsigned long long *a = acc + 4u * (size_t)m;
  pbClusterStats r;
  r.clusters = (unsigned)a[2];
  r.largest = (unsigned)(a[0] >> 32);
  r.largest_label = 0xFFFFFFFFu - (unsigned)a[0];
  r.isolated = (unsigned)(a[2] >> 32);
  r.links = a[1] >> 1;
  r.max_degree = (unsigned)a[3];
  r.rounds = rounds;
  rows[m] = r;
}

__global__ __launch_bounds__(CT) void k_cluster_labels(const uint32_t *__restrict__ parent, uint32_t base, uint32_t n,
                                                       uint32_t *__restrict__ labels) {
  const uint32_t l = blockIdx.x * CT + threadIdx.x;
  if (l < n) labels[l] = parent[base + l] - base;
}

int ensureScratch(pbSim *S, uint32_t numKeys) {
  if (S->cluster) return PB_OK;
  PbClusterScratch *C = new PbClusterScratch();
  S->cluster = C;  // ~pbSim frees whatever a failed allocation below leaves behind
  const size_t total = S->total;
  for (int k = 0; k < 2; k++) {
    PB_TRY(C->keys[k].alloc(total));
    PB_TRY(C->vals[k].alloc(total));
  }
  PB_TRY(C->hist.alloc(pbSortHistEntries(S->total)));
  PB_TRY(C->cpr.alloc(total + 2));
  PB_TRY(hipMemset(C->cpr, 0, sizeof(float4) * (total + 2)));
  PB_TRY(C->start.alloc((size_t)numKeys + 1));
  PB_TRY(C->parent.alloc(total));
  PB_TRY(C->degree.alloc(total));
  PB_TRY(C->size.alloc(total));
  PB_TRY(C->labels.alloc(S->n));
  PB_TRY(C->acc.alloc(4 * (size_t)S->nsims));
  PB_TRY(C->rows.alloc(S->nsims));
  PB_TRY(C->flag.alloc(2));
  PB_TRY(C->ev0.create());
  return PB_OK;
}

// the grid's shape depends on the batch alone: cells = max(16, n rounded up to a power of two) per member
uint32_t gridBits(const pbSim *S) {
  uint32_t bits = 4;
  while (bits < 31 && (1u << bits) < S->n) bits++;
  return bits;
}

}  // namespace

// The scratch of the filing front end, for a caller that must not allocate later (pb_cluster.hpp).
int pbClusterEnsureScratch(pbSim *S) {
  useDevice(S);
  return ensureScratch(S, S->nsims << gridBits(S));
}

// The filing front end (pb_cluster.hpp): everything up to, but not including, the link pass.
int pbClusterFile(pbSim *S, double reach, double perRmax) {
  useDevice(S);
  const uint32_t bits = gridBits(S);
  const uint32_t gxLog2 = (bits + 1) / 2, gyLog2 = bits / 2;
  const uint32_t cells = 1u << bits, numKeys = S->nsims * cells;
  const int rc = ensureScratch(S, numKeys);
  if (rc != PB_OK) return rc;
  PbClusterScratch *C = S->cluster;
  C->gxLog2 = gxLog2, C->gyLog2 = gyLog2;
  const uint32_t n = S->n, total = S->total;
  const int c = S->cur;
  const dim3 b(CT), gBots(cdiv(n, CT), S->nsims);
  PB_TRY(hipEventRecord(C->ev0, S->stream));
  PB_TRY(hipMemsetAsync(C->flag, 0, sizeof(uint32_t) * 2, S->stream));
  float rmax = 0.0f;
  if (perRmax != 0.0) {
    const uint32_t rmaxBlocks = cdiv(total, CT) < 1024u ? cdiv(total, CT) : 1024u;
    hipLaunchKernelGGL(k_cluster_rmax, dim3(rmaxBlocks), b, 0, S->stream, S->pr[c], total, C->flag + 1);
    uint32_t rmaxBits = 0;
    PB_TRY(hipMemcpyAsync(&rmaxBits, C->flag + 1, sizeof rmaxBits, hipMemcpyDeviceToHost, S->stream));
    PB_TRY(hipStreamSynchronize(S->stream));
    memcpy(&rmax, &rmaxBits, sizeof rmax);
  }
  // the cluster analysis' edge >= 2 rmax + gap, rounded up by 2^-10 (fp32 rounding of the predicate and fp64 rounding of
  // the cell index are below 2^-20 of it); never below 2^-8, so that |x| <= 2^20 gives a cell index below 2^28
  double edge = (perRmax * (double)rmax + reach) * (1.0 + 1.0 / 1024.0);
  if (!(edge > 1.0 / 256.0)) edge = 1.0 / 256.0;
  ClusterGrid G;
  G.invCell = 1.0 / edge;
  G.gxLog2 = gxLog2, G.gyLog2 = gyLog2;
  C->invCell = G.invCell;
  hipLaunchKernelGGL(k_cluster_hash, gBots, b, 0, S->stream, S->pr[c], n, G, C->keys[0], C->vals[0]);
  hipError_t e;
  const int where = pbRadixSortPairs(C->keys[0], C->vals[0], C->keys[1], C->vals[1], C->hist, total,
                                     pbKeyBits(numKeys), S->stream, &e);
  if (where < 0) PB_TRY(e);
  C->sortedIn = where;
  hipLaunchKernelGGL(k_cluster_gather, gBots, b, 0, S->stream, S->pr[c], S->orig[c], C->vals[where], n, C->cpr,
                     C->parent, C->size);
  hipLaunchKernelGGL(k_cluster_starts, dim3(cdiv(numKeys + 1u, CT)), b, 0, S->stream, C->keys[where], total, numKeys,
                     C->start);
  PB_TRY(hipGetLastError());
  return PB_OK;
}

// The whole pipeline; leaves parent (roots), degree and the rows on the device and the stream drained.
int pbClusterAnalyse(pbSim *S, float gap) {
  const int rc = pbClusterFile(S, (double)gap, 2.0);
  if (rc != PB_OK) return rc;
  PbClusterScratch *C = S->cluster;
  const ClusterGrid G = gridOf(C);
  const uint32_t n = S->n, total = S->total;
  const dim3 b(CT), gBots(cdiv(n, CT), S->nsims), gAll(cdiv(total, CT));
  PB_TRY(hipMemsetAsync(C->acc, 0, sizeof(unsigned long long) * 4 * S->nsims, S->stream));
  hipLaunchKernelGGL(k_cluster_links, gBots, b, 0, S->stream, C->cpr, C->start, n, G, gap, C->parent, C->degree);
  PB_TRY(hipGetLastError());
  unsigned rounds = 1;  // the hook round
  for (;;) {
    uint32_t changed = 0;
    hipLaunchKernelGGL(k_cluster_compress, gAll, b, 0, S->stream, C->parent, total, C->flag);
    PB_TRY(hipMemcpyAsync(&changed, C->flag, sizeof changed, hipMemcpyDeviceToHost, S->stream));
    PB_TRY(hipStreamSynchronize(S->stream));
    rounds++;
    if (!changed) break;
    if (rounds >= MAX_ROUNDS) {
      pbLastError() = "cluster analysis: the forest did not settle";
      return PB_ERR_HIP;
    }
    PB_TRY(hipMemsetAsync(C->flag, 0, sizeof(uint32_t), S->stream));
  }
  hipLaunchKernelGGL(k_cluster_sizes, gAll, b, 0, S->stream, C->parent, total, C->size);
  hipLaunchKernelGGL(k_cluster_reduce, gBots, b, 0, S->stream, C->parent, C->size, C->degree, n, C->acc);
  hipLaunchKernelGGL(k_cluster_rows, dim3(cdiv(S->nsims, CT)), b, 0, S->stream, C->acc, S->nsims, rounds, C->rows);
  PB_TRY(hipGetLastError());
  C->rounds = rounds;
  return pbClockStop(S, C->clusterClock);
}

// The argument checks of the entry points (pb_cluster.hpp).
int pbClusterCheckArgs(const char *fn, const pbSim *S, const float *gap, const unsigned *member) {
  if (gap && (!(*gap >= 0.0f) || !(*gap < __builtin_inff()))) return pbFail(fn, ": linkGap must be finite and >= 0");
  if (member && *member >= S->nsims) return pbFail(fn, ": member out of range");
  if (S->nsims > 65535u)  // the member is a launch's grid y
    return pbFail(fn, ": the batch must hold at most 65535 members");
  return pbCheckBatch(fn, S);
}

void pbClusterFree(pbSim *S) {
  delete S->cluster;
  S->cluster = nullptr;
}

int pbSimClusterStats(pbSim *S, float linkGap, pbClusterStats *stats) {
  if (!S || !stats) return pbFail("pbSimClusterStats", ": null handle or stats");
  int rc = pbClusterCheckArgs("pbSimClusterStats", S, &linkGap, nullptr);
  if (rc != PB_OK) return rc;
  rc = pbClusterAnalyse(S, linkGap);
  if (rc != PB_OK) return rc;
  PB_TRY(hipMemcpy(stats, S->cluster->rows, sizeof(pbClusterStats) * S->nsims, hipMemcpyDeviceToHost));
  return PB_OK;
}

int pbSimClusterLabelsOf(pbSim *S, unsigned member, float linkGap, unsigned *labels, unsigned *degree) {
  if (!S) return pbFail("pbSimClusterLabelsOf", ": null handle");
  if (!labels && !degree) return pbFail("pbSimClusterLabelsOf", ": labels and degree are both null");
  int rc = pbClusterCheckArgs("pbSimClusterLabelsOf", S, &linkGap, &member);
  if (rc != PB_OK) return rc;
  rc = pbClusterAnalyse(S, linkGap);
  if (rc != PB_OK) return rc;
  PbClusterScratch *C = S->cluster;
  const uint32_t n = S->n, base = member * n;
  if (labels) {
    hipLaunchKernelGGL(k_cluster_labels, dim3(cdiv(n, CT)), dim3(CT), 0, S->stream, C->parent, base, n, C->labels);
    PB_TRY(hipGetLastError());
    PB_TRY(hipMemcpyAsync(labels, C->labels, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, S->stream));
  }
  if (degree)
    PB_TRY(hipMemcpyAsync(degree, C->degree + base, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, S->stream));
  PB_TRY(hipStreamSynchronize(S->stream));
  return PB_OK;
}

int pbSimGetClusterTimes(pbSim *S, unsigned long long *analyses, float *last_device_ms) {
  return pbClockGet("pbSimGetClusterTimes", S, &PbClusterScratch::clusterClock, analyses, last_device_ms);
}
