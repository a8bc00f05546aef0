/*
 * particlebot_hip.h -- C-ABI of libparticlebot_hip.so (MI355X / gfx950).
 *
 * Two seams:
 *
 *  (1) The reference's own `extern "C"` device boundary, particlebot.cuh:15-121 (bodies in
 *      particlebot_cuda.cu:26-384).  Same names, same argument order and meaning, same
 *      "void + print + exit(EXIT_FAILURE) on error" convention (include/helper_cuda.h:1000-1029).
 *      Each declaration cites the reference line it replaces.  One global parameter block, default
 *      stream, caller owns every buffer: exactly the reference's contract.
 *
 *  (2) `pbSim*`: the resident, fused engine (new).  Per-instance parameters (many simulations per
 *      process), status-returning, state kept cell-sorted in HBM between re-sorts, one fused kernel
 *      per timestep.  This is what Particlebot::update drives by default and what bench.py times.
 *
 * Plain pointers and sizes only; no C++ or framework types cross this boundary.
 */
#ifndef PARTICLEBOT_HIP_H
#define PARTICLEBOT_HIP_H

#include <stddef.h>

#include "particlebot_kernel.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Opaque handle standing in for `struct cudaGraphicsResource` (particlebot.cuh:25-30).  In the
 * headless build a "GL buffer object" is a plain device buffer created with pbCreateBuffer(). */
struct pbGraphicsResource;

/* Phase-noise generators.  PB_RNG_COUNTER (default) is this project's own counter-based generator
 * (seed, bot, draw) -> N(0,1), bit-identical between the HIP kernels and the CPU oracle.
 * PB_RNG_XORWOW_CURAND restates cuRAND's published XORWOW algorithm (curand_init(seed, bot, 0) +
 * curand_normal; particlebot_kernel_impl.cuh:36-51): integer stream cuRAND-compatible by construction,
 * unverifiable in an image without CUDA.  PB_RNG_XORWOW_ROCRAND is the same generator with rocRAND's
 * seeding constants, bit-identical to rocrand_device::xorwow_engine (csrc/pb_xorwow.hpp). */
enum { PB_RNG_COUNTER = 0, PB_RNG_XORWOW_CURAND = 1, PB_RNG_XORWOW_ROCRAND = 2 };

/* Per-bot RNG state crossing the boundary where the reference passes `curandState*`
 * (particlebot.cuh:73-78, particlebot.h:98): 48 bytes, the size of cuRAND's curandStateXORWOW, so a
 * caller that allocates sizeof(curandState) * nCells gets the same bytes. */
typedef struct pbRngState {
  unsigned d;           /* XORWOW: Weyl sequence value          | counter generator: the seed */
  unsigned v[5];        /* XORWOW: the five xorshift words      | counter generator: v[0] = draws so far */
  int boxmuller_flag;   /* XORWOW: nonzero while boxmuller_extra holds the second normal of a pair */
  int kind;             /* PB_RNG_* */
  float boxmuller_extra;
  float reserved[3];
} pbRngState;

/* Generator that the legacy boundary's curand_setup() initialises (process-wide, like the reference's
 * one global parameter block); PB_RNG_COUNTER until changed.  Returns 0, or nonzero for a bad kind. */
int pbSetRngKind(int kind);
int pbGetRngKind(void);

/* ------------------------------------------------------------------------------------------ */
/* (1) reference device boundary                                                               */
/* ------------------------------------------------------------------------------------------ */

void cudaInit(int argc, char **argv);   /* particlebot.cuh:18  ; particlebot_cuda.cu:29-41  */
void cudaGLInit(int argc, char **argv); /* main.cpp:97         ; particlebot_cuda.cu:43-47  */

/* particlebot.cuh:20 declares `int size` but particlebot_cuda.cu:49 defines `size_t size`
 * (latent ABI mismatch in the reference); the definition's size_t is what is exported here. */
void allocateArray(void **devPtr, size_t size);
void freeArray(void *devPtr); /* particlebot.cuh:21 */
void threadSync(void);        /* particlebot.cuh:23 */

/* particlebot.cuh:25-26.  If `res` is non-NULL the device pointer is taken from the mapped buffer
 * object instead of `device` (particlebot_cuda.cu:97-113). */
void copyArrayFromDevice(void *host, const void *device, struct pbGraphicsResource **res, int size);
void copyArrayToDevice(void *device, const void *host, int offset, int size);

/* particlebot.cuh:27-30 (GL interop in the reference; plain device buffers here) */
void registerGLBufferObject(uint vbo, struct pbGraphicsResource **res);
void unregisterGLBufferObject(struct pbGraphicsResource *res);
void *mapGLBufferObject(struct pbGraphicsResource **res);
void unmapGLBufferObject(struct pbGraphicsResource *res);

/* Headless replacements for the GL calls Particlebot makes on its buffer objects
 * (glGenBuffers+glBufferData particlebot.cpp:871-880; glBufferSubData :843,:862;
 * glDeleteBuffers :909-912).  Buffers are zero-filled on creation. */
uint pbCreateBuffer(size_t size);
void pbBufferSubData(uint vbo, size_t offset, size_t size, const void *data);
void pbDeleteBuffer(uint vbo);

void setParameters(SimParams *hostParams); /* particlebot.cuh:33 ; particlebot_cuda.cu:111-123 */
/* Extension: half-extent of the integrator's wall clamp.  The reference hard-codes 64
 * (particlebot_kernel_impl.cuh:75-97); that is the default. */
void pbSetWallHalfExtent(float half);

/* particlebot.cuh:35-40 */
void integrateSystem(float *pos, float *vel, float *rad, float deltaTime, uint nCells, float time);
/* particlebot.cuh:42-45 */
void calcHash(uint *gridParticlebotHash, uint *gridParticlebotIndex, float *pos, int nCells);
/* particlebot.cuh:47-58 */
void reorderDataAndFindCellStart(uint *cellStart, uint *cellEnd, float *sortedPos, float *sortedVel,
                                 float *sortedRad, uint *gridParticlebotHash,
                                 uint *gridParticlebotIndex, float *oldPos, float *oldVel,
                                 float *oldRad, uint nCells, uint numCells);
/* particlebot.cuh:63-71 */
void updateRad_light_wave(float *pos, float *absForce_a, float *absForce_r, float *rad, float *phase,
                          float time, float deltaTime, int *dead, int nCells);
/* particlebot.cuh:73 */
void curand_setup(pbRngState *state, int N);
/* particlebot.cuh:75-78 */
void add_normal_noise(pbRngState *state, float *val, float std, int N);
/* particlebot.cuh:80-85 */
void updatePhase(float *pos, float *phase, float spacing, float max_d, float min_d, int nCells);
/* particlebot.cuh:89-94 (display only: feeds the renderer).  rgb of col[4i .. 4i+2] for i < nCells, bit for bit
 * the reference's updateCol_k (display_shadow tint included); alpha and everything past nCells untouched. */
void updateCol(float *rad, float *col, int nCells, float *pos, float *phase, int *dead);
/* particlebot.cuh:96-107 */
void collide(float *newVel, float *absForce_a, float *absForce_r, float *sortedPos, float *sortedVel,
             float *sortedRad, uint *gridParticlebotIndex, uint *cellStart, uint *cellEnd, uint nCells,
             uint numCells, float deltaTime);
/* particlebot.cuh:109-115 (display only: centroid trail).  Writes exactly the two floats at pos + 2 (ind + nCells),
 * ind = (int)(time / hist_int) % hist_steps: the centroid of pos[0 .. nCells) in the reference's summation order,
 * y + 2000.  temppos / temppos1 (nCells float2 each) hold unspecified values afterwards.  Deviation: writes nothing
 * for nCells <= 0, hist_steps <= 0, hist_int <= 0 or a negative ind (negative time), where the reference writes in
 * front of the ring or divides by zero. */
void calcCOG(float *pos, float *temppos, float *temppos1, int nCells, float time, int hist_steps,
             float hist_int);
/* particlebot.cuh:117-119 */
void sortParticlebots(uint *dGridParticlebotHash, uint *dGridParticlebotIndex, uint nCells);

/* ------------------------------------------------------------------------------------------ */
/* (2) resident fused engine                                                                   */
/* ------------------------------------------------------------------------------------------ */

typedef struct pbSim pbSim;

enum {
  PB_OK = 0,
  PB_ERR_HIP = 1,      /* a HIP runtime call failed; see pbGetLastErrorString() */
  PB_ERR_ARG = 2,      /* bad argument (null handle, grid not a power of two >= 8, ...) */
  PB_ERR_NO_DEVICE = 3 /* no gfx950 device visible */
};

typedef struct pbSimStats {
  unsigned long long steps;          /* timesteps executed */
  unsigned long long fused_launches; /* collide + next radius/integrate in one kernel */
  unsigned long long plain_launches; /* collide-only kernel */
  unsigned long long state_launches; /* stand-alone radius+integrate kernel */
  unsigned long long resorts;
  unsigned long long phase_updates;
  unsigned long long resident_launches; /* multi-step one-workgroup-per-simulation kernel */
} pbSimStats;

const char *pbGetLastErrorString(void);

/* The calling THREAD's current HIP device.  A batch lives on the device that was current when it was created
 * (pbSimCreate*), and HIP's current device is per host thread -- a new thread starts on device 0 -- so a program that
 * creates batches from worker threads (one process per GPU, LOCAL_RANK > 0) sets the device in each of them first.
 * (Every other pbSim* call switches to its batch's device by itself.)  The ensemble pipeline does this for the thread
 * that calls pbEnsemblePipelineRun. */
int pbGetDevice(int *device);
int pbSetDevice(int device);
/* "0000:c1:00.0"-style PCI address of a device (cap >= 13): the key under /sys/bus/pci/devices whose numa_node /
 * local_cpulist say which host cores sit next to the GPU (pbHostGetResources, include/particlebot_ensemble.h). */
int pbDevicePciBusId(int device, char *out, int cap);
/* Device and pinned host memory this library holds right now, process-wide: blocks and their bytes, over every batch,
 * analysis scratch and self-test (not the caller-owned arrays of the reference boundary, nor the XORWOW jump table).
 * Either pointer may be NULL.  Equal values before a pbSimCreate* and after the pbSimDestroy say that nothing leaked,
 * whatever other processes do on the device. */
int pbDeviceMemoryLive(unsigned long long *buffers, unsigned long long *bytes);

/* Creates a simulation of params->nCells bots on the current device.  The parameter block is
 * copied (obstacle arrays included, at most PB_MAX_OBSTACLES each).  wallHalf <= 0 selects the
 * reference's 64.  gridSize must be a power of two >= 8 in each dimension.  State starts zeroed
 * with time = 0; absForce_a/r are zero (the reference reads them uninitialised at step 0). */
int pbSimCreate(pbSim **out, const SimParams *params, float wallHalf);
void pbSimDestroy(pbSim *sim);

/* A BATCH of nsims independent simulations (an ensemble: seeds, sweep points) stepped together by
 * the same kernel launches: params is an array of nsims blocks (at most 2^32 - 32 bots in total: slots are 32-bit;
 * from 2^28 bots on the throughput sweep switches from 32-bit to 64-bit byte offsets).  All
 * members must share nCells,
 * the grid, max_time, phase_update_interval, control and payload mode (nDead == -1 or not);
 * everything else (seed, light, obstacles, physics constants) may differ.  pbSimStep & co. advance
 * every member; the *Of functions address one member; pbSimCreate is the nsims == 1 case and the
 * un-suffixed state functions address member 0. */
int pbSimCreateBatch(pbSim **out, const SimParams *params, int nsims, float wallHalf);
int pbSimBatchSize(pbSim *sim, unsigned *nsims, unsigned *nbots);
int pbSimSetStateOf(pbSim *sim, unsigned member, const float *pos, const float *vel, const float *rad,
                    const float *phase, const int *dead);
/* The same for the bots [start, start + count) of the ORIGINAL order only (the arrays hold count
 * entries); every other bot keeps its device state.  This is what Particlebot::setArray(array, data,
 * start, count) needs once the simulation has stepped (particlebot.cpp:834-867 touches only that
 * range). */
int pbSimSetStateRangeOf(pbSim *sim, unsigned member, unsigned start, unsigned count, const float *pos,
                         const float *vel, const float *rad, const float *phase, const int *dead);
int pbSimGetStateOf(pbSim *sim, unsigned member, float *pos, float *vel, float *rad, float *phase, int *dead,
                    float *absForce_a, float *absForce_r);
/* Exact checkpoints.  Between re-sorts the cell lists are STALE by design (the reference re-hashes
 * only every sort_interval), so a bit-identical resume needs, besides the state arrays, the layout:
 * orig[i] = original index of the bot in slot i, keys[i] = the cell hash slot i was filed under at
 * the last sort (ascending).  *sorted is 0 if the simulation has not been sorted yet.  After
 * pbSimSetLayoutOf for every member, restore the state with pbSimSetStateOf + pbSimSetForcesOf,
 * pbSimSetTime and pbSimSetPhaseDraws. */
int pbSimGetLayoutOf(pbSim *sim, unsigned member, unsigned *orig, unsigned *keys, int *sorted);
int pbSimSetLayoutOf(pbSim *sim, unsigned member, const unsigned *orig, const unsigned *keys);
int pbSimSetForcesOf(pbSim *sim, unsigned member, const float *absForce_a, const float *absForce_r);
/* centre of mass of every member: cxcy[2*k], cxcy[2*k+1]; reduced on the device in a fixed order */
int pbSimCentroids(pbSim *sim, double *cxcy);
/* The reference's own centroid SUMS of every simulation of the batch (sumxy[2k], sumxy[2k+1]): fp32, the bots added
 * serially in original order as dumpParticlebot does (particlebot.cpp:335-338) -- bit for bit what its CSV's
 * "Centroid X, Centroid Y" columns are divided from (pbSimCentroids above is the accurately rounded mean). */
int pbSimCentroidSums(pbSim *sim, float *sumxy);
/* Display (the reference's updateCol / calcCOG on the engine's state; the dynamics are untouched either way).
 * GetColorsOf: one member's RGBA (4 n floats, ORIGINAL order) computed now from its state, bit for bit the legacy
 * updateCol on the same state with alpha 1.
 * SetCentroidTrail(1): one ring of centroid_steps float2 per member, reset to (-5000, 0); from then on every step
 * whose start time t passes the reference's gate t - centroid_int floorf(t / centroid_int) < dt records calcCOG of
 * the positions at the start of that step into slot (int)(t / centroid_int) % centroid_steps.  PB_ERR_ARG when the
 * members disagree on centroid_int or centroid_steps, or either is <= 0.  SetCentroidTrail(0) (the default) frees
 * it: no allocation, no launch.
 * GetCentroidTrailOf: xy = the ring verbatim (2 centroid_steps floats, y still + 2000), times = the fp32 start time of
 * the step that wrote each slot (NaN: never written), records = the records made so far; NULL pointers are skipped.
 * The trail is not part of a checkpoint: a resumed run starts a fresh ring. */
int pbSimGetColorsOf(pbSim *sim, unsigned member, float *rgba);
int pbSimSetCentroidTrail(pbSim *sim, int on);
int pbSimGetCentroidTrailOf(pbSim *sim, unsigned member, float *xy, float *times, unsigned *records);

/* Host arrays in ORIGINAL bot order; NULL pointers leave that array unchanged.
 * pos, vel: 2*n floats; rad, phase: n floats; dead: n ints. */
int pbSimSetState(pbSim *sim, const float *pos, const float *vel, const float *rad, const float *phase,
                  const int *dead);
/* Same layout; also absForce_a / absForce_r (n floats each).  NULL pointers are skipped. */
int pbSimGetState(pbSim *sim, float *pos, float *vel, float *rad, float *phase, int *dead,
                  float *absForce_a, float *absForce_r);
int pbSimSetTime(pbSim *sim, float time);
int pbSimGetTime(pbSim *sim, float *time);
/* Number of phase-noise draws made so far (the k of the counter RNG); settable for resume. */
int pbSimGetPhaseDraws(pbSim *sim, unsigned *draws);
int pbSimSetPhaseDraws(pbSim *sim, unsigned draws);

/* Runs up to nsteps iterations of Particlebot::update's schedule (particlebot.cpp:170-300) minus
 * the host-side dead-bot draw (:178-194, done by the caller through pbSimSetState): phase update
 * every phase_update_interval, radius actuation, integration, re-hash + stable sort every
 * sort_interval, neighbour forces, fp32 `time += dt`.  Stops before a step whose start time
 * exceeds max_time (the reference calls exit(0) there).  *steps_done receives the count.
 * Asynchronous with respect to the host except at phase updates (4-byte read-back). */
int pbSimStep(pbSim *sim, float deltaTime, float sort_interval, int nsteps, int *steps_done);
/* Same, bracketed by HIP events on the simulation's stream; *elapsed_ms is device time. */
int pbSimStepTimed(pbSim *sim, float deltaTime, float sort_interval, int nsteps, int *steps_done,
                   float *elapsed_ms);
/* Same, and *wall_ms (if not NULL) = the HOST's clock over the region: from entry -- the caller has synchronised, the
 * stream is idle -- through every launch to the drained stream (the end event has completed; hipStreamQuery confirms).  The host polls for the
 * end of the region instead of sleeping on an interrupt, so for a region of a few milliseconds wall and device time
 * differ only by the dispatch and completion latencies (~10 us; PB_TIMED_TRACE=1 prints where the host's time went).
 * bench.py's `value` is over this clock, its `roofline` over *elapsed_ms, of the same launches. */
int pbSimStepTimedWall(pbSim *sim, float deltaTime, float sort_interval, int nsteps, int *steps_done,
                       float *elapsed_ms, double *wall_ms);
int pbSimSynchronize(pbSim *sim);

/* Centre of mass, reduced on the device in a fixed order (double accumulation). */
int pbSimCentroid(pbSim *sim, double *cx, double *cy);
int pbSimGetStats(pbSim *sim, pbSimStats *stats);
/* 0: stale cell lists re-sorted every sort_interval (reference behaviour, default);
 * 1: re-sort every step (never the default: it changes trajectories). */
int pbSimSetResortEveryStep(pbSim *sim, int on);

/* How the phase update finds the distance from the light to the nearest bot (particlebot.cpp:214-228: a host
 * loop of powf(powf(dx,2) + powf(dy,2), 0.5f) over every position).  0 (default): the device reduces
 * min(dx*dx + dy*dy), 4 bytes per simulation come back and the host takes powf(., 0.5f) -- the reference's value
 * provided the host libm has powf(x,2) == x*x for every float and a non-decreasing powf(., 0.5f), which
 * pbHostLibmCheck (libparticlebot_host.so; tests/test_libm_pin.py) verifies exhaustively.  1: the reference's own
 * loop on the host over all positions (8 n bytes per simulation): no assumption.  pbSetMinDistanceMode sets the
 * default of batches created afterwards (process-wide); the environment variable PB_MIN_DISTANCE_MODE (0 or 1) seeds
 * that default for a whole process tree, read once at the first batch.  Precedence: a batch's own
 * pbSimSetMinDistanceMode > pbSetMinDistanceMode > the environment > 0.  pbGetMinDistanceMode returns the default a
 * batch created now would get. */
int pbSimSetMinDistanceMode(pbSim *sim, int mode);
int pbSetMinDistanceMode(int mode);
int pbGetMinDistanceMode(void);

/* The smallest non-negative float x with sqrtf(x) >= c (0 when c <= 0 or NaN): `length(v) < c` of the static-friction
 * hold (particlebot_impl.cuh:809-811) is decided as `dot(v,v) < pbHostSqrtThreshold(c)`, the same decision for every
 * input because sqrtf is correctly rounded and therefore monotone.  Host-only (no GPU needed); exported for
 * tests/test_sqrt_threshold.py. */
float pbHostSqrtThreshold(float c);

/* Force-kernel variant of a simulation: 0 reference-shaped branches, 1 branch-free, 2 branch-free
 * with the fast exact sqrt/division forms (default; falls back to 1 when the simulation's
 * constants are outside their proven domain).  Variants 0-2 give bit-identical results.
 * 3 = STREAMLINED arithmetic (opt-in, NOT bit-identical): distance and unit vector from one
 * reciprocal square root, 1/gap^2 from one reciprocal, |F_attr| from its coefficient, FMA
 * contraction, a bot's contact terms added after its attraction terms.  About twice as fast;
 * agrees with variants 0-2 to ~1e-7 relative per 10 steps except where a bot lands on the other
 * side of one of the reference's force-law discontinuities.  It only
 * replaces the throughput form (batches above 131072 bots, or lanes-per-bot forced to 1); smaller
 * batches keep running the exact kernels. */
int pbSimSetForceVariant(pbSim *sim, int variant);
/* The two per-bot magnitude sums of the force kernel, absForce_a (Sum|F_attr|) and absForce_r
 * (Sum|F_rep|), are private scratch arrays of the reference (no getArray case, not in the dump);
 * their only reader is the next step's radius actuation, which reads absForce_a solely under
 * `if (params.constrained_contraction)` (particlebot_kernel_impl.cuh:167-169; 0 by default and in all
 * shipped examples).  mode 0 (default): absForce_a is maintained only when some member of the batch
 * has constrained_contraction set -- otherwise it is a dead value, the branch-free force kernels
 * (variants 1 and 2, every lanes-per-bot form, the resident kernel) do not compute it (one exact square
 * root per candidate pair less) and pbSimGetState returns NaN for it.  mode 1: always maintained (valid from the next step on).  Positions,
 * velocities, radii, phases and absForce_r do not depend on the mode. */
int pbSimSetForceSums(pbSim *sim, int mode);
/* Lanes per bot in the per-step force kernel: 1 = throughput form (one bot per lane); 2, 4, 8, 16, 32,
 * 64 = that many adjacent lanes share a bot's neighbour list and add the terms in list order (batches
 * too small to fill the chip: the serial neighbour loop is the limit); 0 = automatic (default:
 * 64 up to 1280 bots in the batch, 32 up to 2560, 16 up to 8192, 8 up to 40960, 4 up to 131072, else 1).
 * Results do not depend on it. */
int pbSimSetLanesPerBot(pbSim *sim, int lanes);
/* Split-lane tail of the throughput form (one lane per bot, 32-bit offsets): the last `tiles` tiles of every
 * XCD's share of the grid -- the last workgroups to be dispatched -- run with PB_TAIL_LANES lanes per bot, so
 * that the launch's final workgroups have shorter serial neighbour chains.  -1 = automatic (default: the rule
 * of pbTailTiles, pb_force.hip), 0 = off, else that many tiles per XCD (capped at the XCD's share).  What the
 * next launch uses is pbSimConfig.tail_tiles.  Results do not depend on it. */
int pbSimSetTailTiles(pbSim *sim, int tiles);
/* The throughput grid's workgroup -> bots mapping (no device needed): workgroup `workgroup` of a grid with
 * `per_xcd` tiles per XCD, `tail_tiles` of them split, covers bots [*first_bot, *first_bot + *bots).  PB_ERR_ARG
 * for a workgroup beyond the grid (8 * (per_xcd + tail_tiles * (lanes - 1)) workgroups) or tail_tiles > per_xcd. */
int pbForceXcdTile(unsigned workgroup, unsigned per_xcd, unsigned tail_tiles, unsigned *first_bot, unsigned *bots);
/* Resident form for simulations of at most 1024 bots: one workgroup per simulation keeps the state
 * in registers/LDS and runs every timestep up to the next re-sort, phase update or end of the
 * pbSimStep call in ONE launch.  0 = automatic (default: a cost model fitted to MI355X measurements
 * picks it for a lone simulation of ~100 bots and for ensembles of many small ones),
 * 1 = never, 2 = whenever the simulation fits.  Results do not depend on it. */
int pbSimSetResident(pbSim *sim, int mode);

/* What the next pbSimStep will launch for this batch (after the automatic choices): the force variant
 * as set and the kind of kernel that really runs (0-2 exact, 3 streamlined; 2 falls back to 1 when the
 * constants are outside the fast forms' domain), the effective lanes per bot of the per-step kernel,
 * whether the resident multi-step kernel is used, and the phase-noise generator.  bench.py echoes it
 * into its JSON line so a reader can see which kernel a number belongs to. */
/* One frame of one member, rasterised on the device from the resident state (csrc/pb_render.hip): byte for byte the
 * picture Particlebot::writeFramePPM (style 0) / writeFramePPMReference (style 1) paints on the host from the same
 * state -- background 245, rectangle obstacles, circle obstacles, the light disc of lightRadius, the bots in ORIGINAL
 * index order (a pixel keeps the highest index that covers it), and in style 1 with the centroid trail on
 * (pbSimSetCentroidTrail) the recorded trail slots as red discs of centroid_radius on top.  scale =
 * 0.5f * height / halfExtent pixels per world unit, x mirrored, y up.  `rgb` is a host buffer of 3 * width * height
 * bytes, rows top to bottom, R G B per pixel.  Only the picture leaves the device.
 * Rendering reads the state and changes nothing: not the slot layout, not the counters of pbSimStats.  Buffers
 * (4 + 3 bytes per pixel, 4 per bot) are allocated by the first call, kept, and freed by pbSimDestroy.
 * PB_ERR_ARG, before the device is touched: NULL handle, view or buffer; member out of range; width or height <= 0 or
 * width * height > PB_RENDER_MAX_PIXELS; halfExtent not > 0; style other than 0 or 1.
 * Non-finite positions or radii are outside the contract (the host writer's conversion of them to int is undefined):
 * the device does not fault on them and draws nothing for such a bot.  The lanes per bot are chosen from
 * max_radius * scale; a bot far larger than that is drawn correctly, but by too few lanes.
 * pbSimGetRenderStats: frames rendered so far, and the device time of the last frame's launches (clear, scatter,
 * resolve; without the copy to the host) in milliseconds.  Either pointer may be NULL. */
#define PB_RENDER_MAX_PIXELS 67108864ull /* 2^26 */
typedef struct pbRenderView {
  int width, height;                  /* > 0, width * height <= PB_RENDER_MAX_PIXELS */
  float centerX, centerY, halfExtent; /* halfExtent > 0: world units from the centre to the top edge */
  float lightRadius;
  int style;                          /* 0 plain, 1 reference (device colours + centroid trail) */
} pbRenderView;
int pbSimRenderOf(pbSim *sim, unsigned member, const pbRenderView *view, unsigned char *rgb);
int pbSimGetRenderStats(pbSim *sim, unsigned long long *renders, float *last_device_ms);

/* Cluster analysis on the device (csrc/pb_cluster.hip): the connected components of every member's contact graph, from
 * the resident state.
 * Nodes: all nCells bots of a member, dead bots and the payload bot of payload mode included.
 * Bots i != j of the same member are LINKED iff, in fp32 with no contraction,
 *     rx = xj - xi;  ry = yj - yi;  dist = sqrtf(rx*rx + ry*ry);      (the pair law's dist, correctly rounded)
 *     (dist - (ri + rj)) < linkGap
 * The predicate is symmetric.  linkGap = 0 is exactly the pair law's contact test dist < ra + rb; coincident bots are
 * linked.  A positive linkGap also links bots held by attraction across a gap (0.0019f: the outer edge of the law's
 * linear band).  A bot with a non-finite position or radius has no links and does not fault.  Results are guaranteed for
 * finite positions with |x|, |y| <= 2^20; outside that range the call does not fault and may return anything.
 * A CLUSTER is a connected component of that graph; a bot's LABEL is the smallest ORIGINAL index in its component, so
 * labels are canonical and every output is an integer that can be compared exactly.
 * pbSimClusterStats: one row per member (nsims entries).  pbSimClusterLabelsOf: one member's labels and degrees, n each,
 * ORIGINAL order; a NULL pointer is skipped.  Each call analyses the state as it is now.  pbSimGetClusterTimes: analyses
 * run so far, and the time in milliseconds that the last one took on the batch's stream, from its first launch to its
 * last (HIP events): the kernels plus the gaps in which the host reads 4 bytes back (the largest radius, and the
 * "nothing changed" flag once per compress round) -- what one analysis costs the device's queue, not the sum of the
 * kernels' own times.  Either pointer may be NULL.
 * PB_ERR_ARG, before the device is touched: NULL handle; NULL stats; member out of range; labels and degree both NULL;
 * linkGap negative, NaN or infinite; a batch of 2^28 bots or more, or of more than 65535 members.
 * The analysis only reads the simulation: not the slot layout, keys or cell lists (which are stale between re-sorts and
 * are not used to find links: the bots are filed afresh), not the counters of pbSimStats, not the time, the RNG or the
 * render buffers.  Its scratch -- 44 bytes per bot of the batch, 4 bytes per cell of its grid (max(16, nCells rounded
 * up to a power of two) cells per member), 4 bytes per bot of one member, the sort's histogram and 64 bytes per
 * member -- is allocated by the first call, kept, and freed by pbSimDestroy. */
typedef struct pbClusterStats {        /* 32 bytes */
  unsigned clusters;       /* components, single bots included */
  unsigned largest;        /* bots in the largest component */
  unsigned largest_label;  /* its label; the smallest label among ties */
  unsigned isolated;       /* bots of degree 0 */
  unsigned long long links;/* undirected links */
  unsigned max_degree;
  unsigned rounds;         /* hook/compress rounds the device ran (diagnostic) */
} pbClusterStats;
int pbSimClusterStats(pbSim *sim, float linkGap, pbClusterStats *stats /* nsims entries */);
int pbSimClusterLabelsOf(pbSim *sim, unsigned member, float linkGap,
                         unsigned *labels, unsigned *degree /* n each, ORIGINAL order; NULL skipped */);
int pbSimGetClusterTimes(pbSim *sim, unsigned long long *analyses, float *last_device_ms);

/* The contact network of one member, from the device (csrc/pb_contacts.hip): who touches whom, how deep, and with what
 * force.  The front end is the cluster analysis' (fresh grid, sorted posrad, degrees), so everything said above holds:
 * the link predicate, non-finite bots (no links), the |x|, |y| <= 2^20 guarantee, and what a call leaves untouched
 * (slot layout, keys, cell lists, pbSimStats, time, RNG, render buffers).  Each call analyses the state as it is now.
 * LINKS: bots i != j are linked exactly when pbSimClusterLabelsOf counts them in each other's degree for this linkGap.
 * LAYOUT: a CSR adjacency in ORIGINAL bot order.  offsets[0..n], offsets[0] = 0; bot i owns entries
 * offsets[i] .. offsets[i+1], strictly ascending in `other`; every undirected link appears twice, once under each end;
 * offsets[i+1] - offsets[i] is the cluster analysis' degree[i].
 * ENTRY (16 bytes): other = the neighbour's original index within the member; gap = dist - (ri + rj), the fp32 value
 * the predicate compared (negative in contact); (fx, fy) = the force ON bot i FROM other: what the reference's
 * collideSpheres adds into a zeroed accumulator for this ordered pair (A = bot i, B = other), with the velocities of the
 * state as it is now, the member's own parameters, and in payload mode attraction * attractionFactor for whichever end
 * is the payload bot (collideCell's expression and order).  It is the force of the pair law for this pair whether or not
 * the stale 5x5 stencil of the stepping kernels currently sees the pair.  Coincident bots are linked and carry the
 * reference's own non-finite force (0 / 0).
 * VIRIAL (pbSimContactVirialOf): per bot four doubles sxx = sum rx fx, sxy = sum rx fy, syx = sum ry fx, syy = sum ry fy
 * over the bot's entries in CSR order; rx = xj - xi, ry = yj - yi in fp32, widened; fx, fy the entry's fp32 values,
 * widened; each product formed in double (exact: 24 + 24 bits), acc = acc + product from +0.0.
 * pbSimContactsOf: *entries = the member's directed entries (2 x undirected links).  offsets (n + 1) and links may each
 * be NULL.  links != NULL with cap < entries: PB_ERR_ARG, *entries still set, links untouched (call once with links NULL
 * to size, then again with room).
 * PB_ERR_ARG, before the device is touched: NULL handle; NULL entries / virial; member out of range; linkGap negative, NaN
 * or infinite; a batch of 2^28 bots or more, or of more than 65535 members.  After the count pass: a member with 2^31
 * entries or more (offsets are 32-bit).  PB_ERR_HIP "contact export: count and fill disagree" if the two passes ever
 * differed (the fill never writes outside a bot's share; a torn list is not returned).
 * Cost: one cluster analysis of the whole batch, then for the member a prefix sum, a fill and a per-bot insertion sort
 * of each list in place: about 6 entries at contact gaps; the long lists of a large linkGap stay correct and are slow
 * (quadratic in the list length, one lane per bot).  Read back besides the results: 8 bytes (the count) between the
 * passes and the 8-byte disagreement flag.
 * Scratch on top of the cluster analysis', allocated by the first export, kept, freed by pbSimDestroy: per bot of ONE
 * member 4 bytes of offsets (n + 1), 8 of velocities, 8 of positions and 32 of virial; 8 bytes per 256 bots for the
 * scan; 16 bytes per entry of the largest export so far (the link buffer grows when a call needs more).
 * pbSimGetContactTimes: exports run so far and the span of the last one on the batch's stream in milliseconds, from the
 * first launch of its front end to its last kernel (HIP events), as pbSimGetClusterTimes.  Either pointer may be NULL. */
typedef struct pbContactLink {         /* 16 bytes */
  unsigned other;
  float gap;
  float fx, fy;
} pbContactLink;
/* entries = directed entries of the member (2 x undirected links).  offsets (n + 1) and links may each be NULL.
 * links != NULL with cap < entries: PB_ERR_ARG, *entries still set, links untouched (call once with links NULL to size). */
int pbSimContactsOf(pbSim *sim, unsigned member, float linkGap, unsigned *offsets,
                    pbContactLink *links, unsigned long long cap, unsigned long long *entries);
int pbSimContactVirialOf(pbSim *sim, unsigned member, float linkGap, double *virial /* 4 n, ORIGINAL order */);
int pbSimGetContactTimes(pbSim *sim, unsigned long long *exports, float *last_device_ms);

/* Structure analysis on the device (csrc/pb_structure.hip): radial pair counts (the raw material of g(r)) and the
 * hexatic bond-orientational order psi6 of every member, from the resident state.  The bots are filed afresh exactly as
 * for the cluster analysis, so what is said there holds: nodes are all nCells bots of a member (dead bots and the
 * payload bot included), a bot with a non-finite position or radius takes part in nothing and does not fault, results
 * are guaranteed for |x|, |y| <= 2^20, and a call only reads the simulation (slot layout, keys, cell lists, pbSimStats,
 * time, RNG and render buffers stay untouched).  Each call analyses the state as it is now.
 * All arithmetic is fp32 without FMA contraction, sqrtf and / correctly rounded.  For bots i != j of the same member
 *     rx = xj - xi;  ry = yj - yi;  dist = sqrtf(rx*rx + ry*ry);
 * Every number that leaves the device is an integer, or derived from integers by exactly rounded operations: results do
 * not depend on the order in which the device adds, and can be compared exactly.
 * RADIAL PAIR COUNTS (pbSimRadialCounts): scale = (float)bins / rMax, one fp32 division on the host.  The ORDERED pair
 * (i, j) falls into bin b = (int)(dist * scale), truncated, and is counted iff b < bins -- decided as
 * fl(dist * scale) < (float)bins, the same decision for every finite product; when scale overflows to infinity (rMax
 * below bins / FLT_MAX) nothing is counted.  Coincident bots land in bin 0.  counts holds nsims * bins entries, one
 * histogram per member, over ordered pairs: every count is even.  Normalising to g(r) needs a number density, which for
 * a free blob is the caller's choice and stays out of this interface.
 * HEXATIC ORDER: bots i and j are BONDED exactly when the cluster analysis links them for the same linkGap,
 * (dist - (ri + rj)) < linkGap, so a bot's neighbour count equals pbSimClusterLabelsOf's degree.  A bond with dist > 0
 * contributes
 *     ux = rx / dist;  uy = ry / dist;
 *     c2 = ux*ux - uy*uy;   s2 = (ux*uy) + (ux*uy);
 *     c4 = c2*c2 - s2*s2;   s4 = (c2*s2) + (c2*s2);
 *     c6 = c4*c2 - s4*s2;   s6 = s4*c2 + c4*s2;                        (every product rounded before the add or subtract)
 *     qre = (long long)rint(c6 * 1073741824.0f);   qim = (long long)rint(s6 * 1073741824.0f);
 * (the scaling by 2^30 is exact, the conversion rounds to nearest even); a bond with dist == 0 counts as a neighbour and
 * contributes 0.  Per bot: Sre = sum qre, Sim = sum qim over its bonds, 64-bit integers in units of 2^-30, and
 * psi6[2i] = ((double)Sre / 1073741824.0) / (double)neighbours, psi6[2i+1] likewise from Sim; (0, 0) for a bot without
 * neighbours.  Per member one pbStructureStats row; its sums (and a bot's) are exact while the member has fewer than
 * 2^32 directed bonds.
 * pbSimStructureStats: one row per member.  pbSimHexaticOf: one member's psi6 (2 n doubles) and neighbour counts (n), in
 * ORIGINAL order; either pointer may be NULL, not both.  pbSimGetStructureTimes: analyses run so far (radial and
 * hexatic calls alike) and the span of the last one on the batch's stream in milliseconds, from the first launch of its
 * front end to its last kernel (HIP events), as pbSimGetClusterTimes.  Either pointer may be NULL.
 * PB_ERR_ARG, before the device is touched: NULL handle; NULL counts / rows; psi6 and neighbours both NULL; member out of
 * range; rMax not finite or not > 0; bins outside 1 ... PB_RADIAL_MAX_BINS; linkGap negative, NaN or infinite; a batch
 * of 2^28 bots or more, or of more than 65535 members.
 * Scratch on top of the cluster analysis', allocated on first use, kept, freed by pbSimDestroy: 8 bytes per bin and
 * member of the largest histogram asked for so far; for the hexatic calls 20 bytes per bot of the batch, 56 per member
 * and 16 per bot of one member. */
#define PB_RADIAL_MAX_BINS 4096u
typedef struct pbStructureStats {      /* 56 bytes */
  unsigned long long bonds;            /* directed bonds = sum of neighbours */
  long long psi6_re, psi6_im;          /* sum of qre, qim over all directed bonds, units of 2^-30 */
  unsigned coordination[8];            /* bots with 0..6 neighbours; [7]: 7 or more */
} pbStructureStats;
int pbSimRadialCounts(pbSim *sim, float rMax, unsigned bins, unsigned long long *counts /* nsims * bins */);
int pbSimStructureStats(pbSim *sim, float linkGap, pbStructureStats *rows /* nsims entries */);
int pbSimHexaticOf(pbSim *sim, unsigned member, float linkGap, double *psi6 /* 2 n, ORIGINAL order */,
                   unsigned *neighbours /* n */);
int pbSimGetStructureTimes(pbSim *sim, unsigned long long *analyses, float *last_device_ms);

/* Rearrangement analysis on the device (csrc/pb_dynamics.hip): the one analysis that compares two instants.  A MARK keeps
 * a reference on the device; a COMPARE says, for the state as it is now, which bonds of the reference survive and how
 * far every bot has moved since.  The bots are filed afresh exactly as for the cluster analysis, so what is said there
 * holds: nodes are all nCells bots of a member (dead bots and the payload bot included), a bot with a non-finite
 * position or radius has no links and does not fault, results are guaranteed for |x|, |y| <= 2^20, and a call only
 * reads the simulation (slot layout, keys, cell lists, pbSimStats, time, RNG and render buffers stay untouched).
 * LINKS are the cluster analysis': bots i != j of one member are linked at linkGap iff (dist - (ri + rj)) < linkGap,
 * dist = sqrtf(rx*rx + ry*ry) in fp32 without contraction.
 * MARK (pbSimMarkReference): for every member of the batch the device keeps the positions as they are now, in ORIGINAL
 * order, bit for bit; the link network N0 at linkGap as a CSR in ORIGINAL order over the whole batch (32-bit offsets,
 * one 4-byte entry per directed link: `other`, the member-local original index; a bot's entries strictly ascending);
 * linkGap itself and the fp32 time.  A new mark replaces the old one.  The mark is addressed by original index:
 * re-sorts, pbSimSetState* and pbSimSetLayoutOf do not invalidate it.  It is not part of a checkpoint (like the centroid
 * trail).  pbSimClearReference frees it, pbSimDestroy frees everything.  A mark refused for its arguments changes
 * nothing; one that fails later leaves no mark held.
 * pbSimGetReferenceInfo: *marked = 1 with the mark's linkGap, time and directed entries (of the whole batch), or
 * *marked = 0 and zeros; any pointer may be NULL.
 * COMPARE, on the state as it is now; N1 is the link network now, at the mark's linkGap.  Per bot i:
 *     marked[i] = |N0(i)|;   now[i] = |N1(i)|;   kept[i] = |N0(i) n N1(i)|
 * marked[i] is what pbSimClusterLabelsOf gave as degree at the mark, now[i] the degree it gives now; kept is symmetric
 * (j counts for i exactly when i counts for j).  A bot that is non-finite now has now = kept = 0: its marked bonds count
 * as broken at both ends.
 *     dx = x_now - x_mark;   dy = y_now - y_mark                                                          (fp32)
 * The bot is MEASURED iff all four coordinates are finite and fabsf(dx) < 2048.0f and fabsf(dy) < 2048.0f.  Then
 *     qx = (long long)rint(dx * 1048576.0f);   qy likewise;   s = qx*qx + qy*qy
 * (the scaling by 2^20 is exact, the conversion rounds to nearest even, |qx| < 2^31, s < 2^63).
 * Per member one pbRearrangementStats row.  Every number is an integer, so results do not depend on the order in which
 * the device adds and can be compared exactly; with fewer than 2^28 bots |sum q| < 2^59.  The device sums the low and
 * the high 32 bits of every s in two 64-bit accumulators (each below 2^60); the host composes the 128-bit value
 * hi_part * 2^32 + lo_part.  No float atomics, no 128-bit atomics.
 * pbSimRearrangementStats: one row per member.  pbSimRearrangementOf: one member's per-bot results in ORIGINAL order;
 * disp holds dx, dy verbatim (2 n floats), unmeasured bots included; any of the four pointers may be NULL, not all.
 * pbSimGetRearrangementTimes: marks and compares run so far, counted alike, and the span of the last one on the batch's
 * stream in milliseconds, from the first launch of its front end to its last kernel (HIP events), as
 * pbSimGetClusterTimes.  Either pointer may be NULL.
 * PB_ERR_ARG, before the device is touched: NULL handle; NULL rows; all four per-bot pointers NULL; member out of range;
 * linkGap negative, NaN or infinite; a batch of 2^28 bots or more, or of more than 65535 members; a compare with no mark
 * held ("no reference marked").  After the mark's count pass: a batch with 2^31 directed entries or more (offsets are
 * 32-bit).  PB_ERR_HIP "reference mark: count and fill disagree" if the mark's two passes ever differed (the fill never
 * writes outside a bot's share).
 * Cost: a mark files the batch, counts, scans, fills and orders each bot's list by insertion (about 6 entries at contact
 * gaps; the long lists of a large linkGap stay correct and are slow to mark).  A compare files the batch and runs one
 * sweep; a neighbour is looked up in the marked list held in registers (up to 8 entries) or by a binary search in
 * global memory (longer lists).  Read back besides the results: 8 bytes (the count) between the mark's passes and its
 * 8-byte disagreement flag.
 * Scratch on top of the cluster analysis': for the mark 8 + 4 bytes per bot of the batch (positions, offsets), 4 per
 * directed entry of the largest mark so far and 8 per 256 bots for the scan, freed by pbSimClearReference; for the
 * compare 16 bytes per bot of the batch (now, kept, dx, dy) and 80 per member (the row, whose sum_q2 fields hold the two
 * partial sums on the device), allocated by the first compare, kept, freed by pbSimDestroy. */
typedef struct pbRearrangementStats {  /* 80 bytes */
  unsigned long long bonds_marked, bonds_now, bonds_kept; /* directed; all even */
  unsigned bots_unchanged;  /* kept == marked && kept == now: the same neighbour set */
  unsigned bots_lost;       /* kept < marked */
  unsigned bots_gained;     /* kept < now */
  unsigned measured;
  long long sum_qx, sum_qy;                    /* over measured bots, units of 2^-20 */
  unsigned long long sum_q2_lo, sum_q2_hi;     /* sum of s as one 128-bit integer, units of 2^-40 */
  unsigned long long max_q2;                   /* largest s; 0 with no measured bot */
} pbRearrangementStats;
int pbSimMarkReference(pbSim *sim, float linkGap);
int pbSimClearReference(pbSim *sim);
int pbSimGetReferenceInfo(pbSim *sim, int *marked, float *linkGap, float *time, unsigned long long *entries);
int pbSimRearrangementStats(pbSim *sim, pbRearrangementStats *rows /* nsims entries */);
int pbSimRearrangementOf(pbSim *sim, unsigned member, float *disp /* 2 n: dx, dy verbatim, unmeasured bots included */,
                         unsigned *marked, unsigned *now, unsigned *kept /* n each, ORIGINAL order; NULL skipped */);
int pbSimGetRearrangementTimes(pbSim *sim, unsigned long long *analyses, float *last_device_ms);

/* Time series on the device (csrc/pb_moments.hip): one row of integer moments of positions, velocities and radii per
 * member, taken now on request (pbSimMoments) or recorded into a device ring at a chosen interval while pbSimStep runs
 * (pbSimSetSeries) and read back afterwards (pbSimGetSeriesOf).  Off by default; a run that does not ask for it is
 * unchanged.
 * THE ROW.  Nodes are all nCells bots of a member, dead bots and the payload bot included.  A bot is MEASURED iff x, y,
 * vx, vy, rad are all finite and each has fabsf(.) < 2048.0f (the rearrangement analysis' bound and scale).  For a
 * measured bot, in fp32 scaling and with round-to-nearest-even conversion,
 *     qx = (long long)rint(x * 1048576.0f);   qy, wx (from vx), wy (from vy), qr (from rad) likewise
 * (the scaling is exact, |q| < 2^31, every product of two q is below 2^62 in magnitude).  Unmeasured bots take part in
 * nothing.  Per member:
 *     time      fp32, the start time of the step in front of which the row was taken
 *     step      pbSimStats.steps at that moment
 *     measured
 *     sum_qx, sum_qy, sum_qr, sum_wx, sum_wy     signed 64-bit; with fewer than 2^28 bots they stay below 2^59
 *     min_qx, max_qx, min_qy, max_qy             32-bit signed, the bounding box; all four 0 when measured == 0
 *     xx = sum qx*qx,  yy = sum qy*qy,  xy = sum qx*qy (signed),  rr = sum qr*qr,  vv = sum (wx*wx + wy*wy)
 * the last five 128-bit sums, each as a pair {unsigned long long lo; long long hi} with value hi * 2^32 + lo: per bot
 * the 64-bit product p is split as lo += (unsigned)p and hi += p >> 32 with an arithmetic shift (the two's-complement
 * split, so the signed product needs no special case); the two device accumulators stay below 2^60 in magnitude.
 * No float atomics and no 128-bit atomics.  Every number is an integer: results do not depend on slot order, on the
 * kernel form that stepped, or on the order in which the device adds, and can be compared exactly.
 * pbSimMoments returns the state as it is now, one row per member (time = the batch's time, the start time of the next
 * step).  It reads only: the slot layout, keys, cell lists, pbSimStats, time, RNG, render buffers and every other
 * analysis' scratch stay untouched.
 * pbSimSetSeries with capacity > 0 allocates a device ring of `capacity` rows per member (152 bytes each) and resets
 * the record counter to 0; calling it again restarts the series.  capacity == 0 frees the ring: no allocation and no
 * launch (the default).  interval > 0 records in front of every executed step whose fp32 start time t passes the
 * schedule's own gate t - interval floorf(t / interval) < dt, the test the dump, phase-update and trail gates use, so a
 * series at dump_interval lines up with the CSV.  interval == 0 records in front of every executed step (the gate with
 * interval == dt need not be that: fp32 rounding can drop steps).
 * A RECORD is the row pbSimMoments would return had the caller stopped pbSimStep just before that step: positions and
 * radii from the previous step's update, velocities from the previous step's kick.  This holds on all three stepping
 * paths: with separate state launches the record is taken before the state kernel; no launch is fused across a series
 * gate, because the state in front of a gate step never exists on the device once the previous launch has run ahead;
 * a resident stretch ends in front of a series gate, exactly as it ends in front of a trail gate.  Recording changes no
 * state bit.  It only changes which launches carry the steps, so the launch counters of pbSimStats differ from a run
 * without the series (as with the centroid trail, which ends resident stretches too), and interval == 0 costs the fusion
 * of every step.
 * THE RING.  Record number r, counted from 0, goes to slot r % capacity.  The host keeps time and step per slot; the
 * sums stay on the device until asked for; recording never waits for the device.  No record is taken for a step that
 * does not run because t > max_time.  pbSimGetSeriesInfo: the interval, the capacity (0: off) and the records taken so
 * far; any pointer may be NULL, not all.  pbSimGetSeriesOf copies records first .. first + count of one member, in the
 * order taken; PB_ERR_ARG unless that range lies inside [records - min(records, capacity), records); count == 0 is
 * allowed.  pbSimGetSeriesTimes: records so far and the span of the last row's launches (a record's, or pbSimMoments')
 * on the batch's stream in milliseconds (HIP events), as pbSimGetClusterTimes; either pointer may be NULL.
 * The series is not part of a checkpoint, like the trail: pbSimSetState*, pbSimSetTime and pbSimSetLayoutOf leave it
 * alone; pbSimDestroy frees it.
 * PB_ERR_ARG, before the device is touched: NULL handle or NULL rows; member out of range; interval negative, NaN or
 * infinite; capacity x nsims x 152 above 2^31 bytes; a batch of 2^28 bots or more; the pointers of pbSimGetSeriesInfo
 * all NULL; a read with the series off.
 * Cost: one pass over posrad and velocities of the whole batch in slot order (24 bytes per bot, coalesced; the original
 * indices are never read), at most PB_MOMENTS_BLOCKS workgroups of 256 lanes per member, each adding its sums into the
 * member's row with one set of integer atomics.
 * Out of scope: recording inside the resident kernel without ending the stretch; phase moments (they need a
 * transcendental and would not be exact); neighbour-based quantities per record such as bonds or psi6 (they need the
 * fresh filing); the ensemble layer's summary rows and its RCCL gather; the legacy engine. */
#define PB_MOMENTS_BLOCKS 512u /* workgroups per member: one pass of the launch covers 131072 bots of a member */
typedef struct pbMoment128 {           /* 16 bytes: the value is hi * 2^32 + lo */
  unsigned long long lo;
  long long hi;
} pbMoment128;
typedef struct pbMomentsRow {          /* 152 bytes */
  unsigned long long step;
  float time;
  unsigned measured;
  long long sum_qx, sum_qy, sum_qr, sum_wx, sum_wy;  /* over measured bots, units of 2^-20 */
  int min_qx, max_qx, min_qy, max_qy;
  pbMoment128 xx, yy, xy, rr, vv;                    /* units of 2^-40 */
} pbMomentsRow;
int pbSimMoments(pbSim *sim, pbMomentsRow *rows /* nsims entries */);
int pbSimSetSeries(pbSim *sim, float interval, unsigned capacity);
int pbSimGetSeriesInfo(pbSim *sim, float *interval, unsigned *capacity, unsigned long long *records);
int pbSimGetSeriesOf(pbSim *sim, unsigned member, unsigned long long first, unsigned count, pbMomentsRow *rows);
int pbSimGetSeriesTimes(pbSim *sim, unsigned long long *records, float *last_device_ms);

/* Pair correlations on the device (csrc/pb_correlate.hip): how far a per-bot quantity is coordinated across the blob.
 * All pairs of a member are binned by distance and the dot products a_i . a_j of a per-bot integer vector a = (ax, ay)
 * are summed per bin: velocity alignment, the radius wave (a correlation that changes sign with distance) and
 * cooperative rearrangement are this one measurement with three choices of a.  Read-only: state, slot layout,
 * pbSimStats, time, the generators, the mark and the other analyses' results stay as they were.
 * Nodes are all nCells bots of a member, dead bots and the payload bot included; a bot with a non-finite position or
 * radius takes part in nothing, as in pbSimRadialCounts.  `kind` selects a; scaling is in fp32 and the conversion rounds
 * to nearest even, as in pbSimMoments and pbSimRearrangementOf:
 *     PB_CORR_VELOCITY      a = (rint(vx * 2^20), rint(vy * 2^20));  MEASURED iff the bot is a node and vx, vy are
 *                           finite with fabsf(.) < 2048.0f
 *     PB_CORR_DISPLACEMENT  a = (qx, qy) of the rearrangement analysis, since the mark; MEASURED iff the bot is a node
 *                           and that analysis measures it (fabsf(dx) < 2048.0f and fabsf(dy) < 2048.0f).  Needs a mark
 *                           (pbSimMarkReference), which the call leaves alone
 *     PB_CORR_RADIUS        a = (rint(rad * 2^20), 0);  MEASURED iff the bot is a node and fabsf(rad) < 2048.0f
 * An unmeasured bot is in no pair.  Distance and bin are pbSimRadialCounts', word for word: dist = sqrtf(rx*rx + ry*ry)
 * without contraction, scale = (float)bins / rMax, the ORDERED pair (i, j) goes to bin b = (int)(dist * scale) iff
 * fl(dist * scale) < (float)bins; coincident bots land in bin 0.  Per member and bin, over the ordered pairs (i, j),
 * i != j, both measured, that fall into it:
 *     pairs = their number (even);   dot = sum (ax_i*ax_j + ay_i*ay_j);   ax = sum ax_i;   ay = sum ay_i
 * dot, ax and ay are signed 128-bit integers in units of 2^-40 (dot) and 2^-20: pbMoment128, value hi * 2^32 + lo,
 * NORMALISED by the host to 0 <= lo < 2^32 with hi the floor quotient, the same form however the device splits its
 * adds.  The totals row of a member (totals may be NULL): measured, sum_ax, sum_ay, sum_a2 = sum (ax^2 + ay^2)
 * (normalised) over its measured bots, and pairs over all bins.  With m = sum_a / measured the connected correlation of
 * a bin is (dot - 2 m . (ax, ay) + |m|^2 pairs) / pairs: it comes from these integers alone, with no second pass and no
 * mean known in advance.
 * EXACTNESS.  pairs is always exact.  The other sums are exact whenever no bin of any member holds 2^31 ordered pairs
 * or more; the call checks the counts it is about to return, and if a bin holds more it answers PB_ERR_ARG ("a bin
 * holds 2^31 pairs or more: raise bins or lower rMax") without writing rows or totals.
 * pbSimGetCorrelationTimes: analyses run so far and the span of the last one on the batch's stream in milliseconds, from
 * the first launch of its front end to its last kernel (HIP events), as pbSimGetClusterTimes; either pointer may be NULL.
 * PB_ERR_ARG, before the device is touched: NULL handle or rows; unknown kind; rMax not finite or not > 0; bins outside
 * 1 ... PB_CORR_MAX_BINS; a batch of 2^28 bots or more or of more than 65535 members; PB_CORR_DISPLACEMENT with no
 * reference marked.
 * Cost: the front end's re-filing on a grid of edge rMax (1 + 2^-10); one launch that writes a per sorted slot (8 bytes)
 * and reduces the totals; one sweep over the nine cells, a pair met once, five 64-bit LDS atomics per counted pair into
 * the workgroup's table of 40 bytes per bin, flushed once per workgroup.  Scratch on top of the cluster analysis': 8
 * bytes per bot of the batch, 72 per bin and 40 per member.  Read back: 72 bytes per bin and 40 per member.
 * Out of scope: phase correlations (they need a transcendental and would not be exact); correlations per series
 * record; time correlations (pbSimSetTimeCorrelation, below); normalisation to g(r); the ensemble layer's summary rows; the legacy engine. */
#define PB_CORR_MAX_BINS 1024u
enum { PB_CORR_VELOCITY = 0, PB_CORR_DISPLACEMENT = 1, PB_CORR_RADIUS = 2 };
typedef struct pbCorrelationBin {      /* 56 bytes */
  unsigned long long pairs;
  pbMoment128 dot, ax, ay;
} pbCorrelationBin;
typedef struct pbCorrelationTotals {   /* 48 bytes */
  unsigned measured, reserved;
  long long sum_ax, sum_ay;
  pbMoment128 sum_a2;
  unsigned long long pairs;
} pbCorrelationTotals;
int pbSimPairCorrelation(pbSim *sim, int kind, float rMax, unsigned bins, pbCorrelationBin *rows /* nsims * bins */,
                         pbCorrelationTotals *totals /* nsims entries, may be NULL */);
int pbSimGetCorrelationTimes(pbSim *sim, unsigned long long *analyses, float *last_device_ms);

/* Time correlations on the device (csrc/pb_timecorr.hip): the mean squared displacement, the velocity autocorrelation
 * and the overlap function per lag, averaged over time origins while pbSimStep runs.  The analyses above describe one
 * instant or compare with one marked instant; a series row cannot supply sum x(t) . x(t - tau), which needs both
 * instants per bot in ORIGINAL order while the slots are re-sorted in between.  Off by default; a run that does not ask
 * for it is unchanged: same launches, same pbSimStats, same bits.
 * A RECORD keeps (x, y, vx, vy) of every bot of every member, bit for bit, in ORIGINAL order: record number r, counted
 * from 0, goes into slot r % lags of a device ring of 16 bytes per bot and slot.  The host keeps
 * pbSimStats.steps per slot (lags are reported in steps; a record's time is not kept).  A record is the state pbSimGetState would return had the caller stopped pbSimStep just
 * before that step: positions from the previous step's update, velocities from the previous step's kick (the state a
 * series record describes).  After the snapshot is stored, record r is paired with the records r - l for
 * l = 0 ... min(r, lags - 1); l = 0 pairs the record with itself, and its vacf is sum |w|^2, the normaliser.
 * A PAIR.  Nodes are all nCells bots of a member, dead bots and the payload bot included.  For a bot and a pair of
 * records (now, then), in fp32 without contraction, dx = x_now - x_then and dy likewise.  The pair is MEASURED iff all
 * eight inputs are finite, fabsf(dx) < 2048.0f, fabsf(dy) < 2048.0f, and all four velocity components have
 * fabsf(.) < 2048.0f (the rearrangement analysis' bound and scale).  Then, in fp32 scaling and with round-to-nearest-even
 * conversion,
 *     qx = (long long)rint(dx * 1048576.0f);   qy likewise;   wx, wy from the velocities of each instant likewise
 *     s = qx*qx + qy*qy   (below 2^63);        p = wx_now*wx_then + wy_now*wy_then   (|p| below 2^63)
 * and a2 = qa*qa with qa = rint(overlapRadius * 2^20), computed once on the host.  An unmeasured pair takes part in
 * nothing.  Per member and lag, over the measured (bot, origin) pairs, one pbTimeCorrelationRow:
 *     lag        in RECORDS: record r against record r - lag
 *     origins    record pairs added so far;  sum_steps the sum over them of step(r) - step(r - lag), so that the mean
 *                lag is sum_steps / origins steps (both are the same for every member)
 *     samples    the measured pairs;  sum_qx, sum_qy the drift, units of 2^-20
 *     msd = sum s,  vacf = sum p (signed), units of 2^-40, 128-bit sums as pbMoment128, value hi * 2^32 + lo: per
 *                sample the 64-bit value v is split as lo += (unsigned)v and hi += v >> 32 with an arithmetic shift
 *                (the two's-complement split of pbSimMoments); NORMALISED by the host to 0 <= lo < 2^32 with hi the
 *                floor quotient, as pbSimPairCorrelation does
 *     overlap    the samples with s < a2 (so overlapRadius == 0 counts nothing);  max_q2 the largest s, 0 with no sample
 * One table cell per (member, lag) lives on the device; pbSimSetTimeCorrelation zeroes it and every record adds to it:
 * the average over time origins happens on the device and nothing comes back per record.  Every added value is an
 * integer: results do not depend on slot order, on the kernel form that stepped, or on the order in which the device
 * adds, and can be compared exactly.  No float atomics and no 128-bit atomics.
 * EXACTNESS.  samples, origins and sum_steps cannot wrap (a cell gains at most nCells < 2^28 samples per record).  The
 * other sums are exact while a cell holds fewer than 2^31 samples: each half-accumulator then stays below 2^63 in
 * magnitude (DESIGN.md has the derivation).  pbSimGetTimeCorrelation checks the counts it is about to return, and if a
 * cell holds more it answers PB_ERR_ARG ("a lag holds 2^31 samples or more: restart the correlation") and writes no rows.
 * WHEN RECORDS ARE TAKEN.  interval > 0: in front of every executed step whose fp32 start time t passes the schedule's
 * own gate t - interval floorf(t / interval) < dt, the series' rule.  interval == 0: in front of every executed step.
 * interval == -1.0f exactly: manual only.  pbSimTimeCorrelationRecord takes one record now, of the state as it is,
 * whatever the interval, whenever the correlation is on, with the batch's time and pbSimStats.steps.  lags == 0 switches
 * off and frees everything: no allocation and no launch (the default).  Calling pbSimSetTimeCorrelation again restarts
 * from record 0.  Everything said about series records on the three stepping paths holds here: no launch is fused
 * across a gate, a resident stretch ends in front of one, no record is taken for a step that does not run because
 * t > max_time, and no state bit changes, only which launches carry the steps.  When the series and the correlation are
 * both due in front of a step, the series record comes first.
 * The correlation is not part of a checkpoint: pbSimSetState*, pbSimSetTime and pbSimSetLayoutOf leave the ring alone
 * (snapshots are addressed by original index, so re-sorts do not invalidate them); pbSimDestroy frees it.  Reading or
 * recording leaves alone: the slot layout, keys, cell lists, pbSimStats, time, RNG, the mark, the series and every other
 * analysis' scratch.  Recording never waits for the device.
 * pbSimGetTimeCorrelationInfo: the interval, the lags (0: off), the overlap radius and the records taken so far; any
 * pointer may be NULL, not all.  pbSimGetTimeCorrelation: nsims * lags rows, member-major, lag 0 first; a lag that no
 * record has reached yet has origins == 0 and zeros.  pbSimGetTimeCorrelationTimes: records so far and the span of the
 * last record's launches on the batch's stream in milliseconds (HIP events), as pbSimGetSeriesTimes; either pointer may
 * be NULL.
 * PB_ERR_ARG, before the device is touched: NULL handle or rows; interval NaN, infinite, or negative other than -1;
 * lags > PB_TCORR_MAX_LAGS; overlapRadius not in [0, 2048) or NaN; a ring above 2^33 bytes (lags x total x 16); a batch
 * of 2^28 bots or more or of more than 65535 members; the pointers of pbSimGetTimeCorrelationInfo all NULL; a record or
 * a read with the correlation off.
 * Cost: a record is one pass over posrad, velocities and original indices in slot order that scatters 16 bytes per bot
 * into the ring (the only uncoalesced access), and one launch for all lags that reads two snapshots per lag as coalesced
 * 16-byte loads in original order, at most PB_TCORR_BLOCKS workgroups of 256 lanes per member and lag, each adding its
 * nine sums into the cell with one set of 64-bit integer atomics.
 * Out of scope: logarithmic or multi-tau lag spacing; the non-Gaussian parameter here (sum s^2 does not fit a pair of
 * words; the van Hove function keeps it in four: pbSimSetVanHove, below); phase correlations (they need a transcendental; the self-intermediate scattering function does not any more:
 * pbSimSetScattering, below); per-bot
 * outputs; neighbour-based quantities per lag such as bond lifetime; recording inside the resident kernel without ending
 * the stretch; the ensemble layer's summary rows and its RCCL gather; the legacy engine. */
#define PB_TCORR_MAX_LAGS 64u
#define PB_TCORR_BLOCKS 256u /* workgroups per member and lag: one pass covers 65536 bots of a member */
typedef struct pbTimeCorrelationRow {  /* 96 bytes */
  unsigned lag, reserved;              /* lag in RECORDS: record r against record r - lag */
  unsigned long long origins;          /* record pairs added so far (the same for every member) */
  unsigned long long sum_steps;        /* sum over those pairs of step(r) - step(r - lag): mean lag = sum_steps / origins steps */
  unsigned long long samples;          /* measured (bot, origin) pairs */
  long long sum_qx, sum_qy;            /* sum of the displacement, units of 2^-20: the drift */
  pbMoment128 msd;                     /* sum of s = qx*qx + qy*qy, units of 2^-40 */
  pbMoment128 vacf;                    /* sum of wx_now*wx_then + wy_now*wy_then (signed), units of 2^-40 */
  unsigned long long overlap;          /* samples with s < a2 */
  unsigned long long max_q2;           /* largest s; 0 with no sample */
} pbTimeCorrelationRow;
int pbSimSetTimeCorrelation(pbSim *sim, float interval, unsigned lags, float overlapRadius);
int pbSimTimeCorrelationRecord(pbSim *sim);   /* one record now, of the state as it is */
int pbSimGetTimeCorrelationInfo(pbSim *sim, float *interval, unsigned *lags, float *overlapRadius,
                                unsigned long long *records);
int pbSimGetTimeCorrelation(pbSim *sim, pbTimeCorrelationRow *rows /* nsims * lags, member-major, lag 0 first */);
int pbSimGetTimeCorrelationTimes(pbSim *sim, unsigned long long *records, float *last_device_ms);

/* Field maps on the device (csrc/pb_field.hip): WHERE in the blob something happens.  A regular grid of map cells is
 * laid over a view, and per cell the call returns the bots in it, how many of them are dead, and the integer sums of
 * radius, radius^2, velocity and |v|^2.  From these a caller forms number density, area fraction (sum r^2), the mean
 * velocity field, the kinetic temperature (sum |v|^2 minus the mean flow) and the radius wave (mean radius per cell)
 * with no second pass.  Nothing is allocated or launched unless a map is asked for.
 * NODES.  All nCells bots of a member are nodes, dead bots and the payload bot included.
 * MEASURED.  A bot is MEASURED by pbSimMoments' rule: x, y, vx, vy and rad are finite and each has fabsf(.) < 2048.0f.
 * The quantisation is pbSimMoments': q = (long long)rint(v * 1048576.0f) in fp32 scaling, round to nearest even; it
 * gives qr (from rad), wx (from vx) and wy (from vy).  Positions are not quantised; they only choose the cell.
 * CELL OF A MEASURED BOT.  Everything is fp32 with no contraction.  The host computes once
 *     x0 = centerX - halfX;   sx = (float)nx / (halfX + halfX)
 * and the device computes tx = (x - x0) * sx, with two roundings.  The bot is inside in x iff tx >= 0.0f &&
 * tx < (float)nx; then ix = (int)tx.  A tx of -0.0f is inside, in column 0.  y works the same way with y0, sy, ny; row 0
 * is the lowest y.  The cell index is iy * nx + ix; cells are member-major: member m's cell at cells[(m * ny + iy) * nx + ix].
 * COUNTING.  A measured bot that is inside in both axes adds to its cell: count += 1, dead += (dead != 0),
 * sum_qr += qr, sum_wx += wx, sum_wy += wy, rr += qr*qr, vv += wx*wx + wy*wy.  rr and vv are 128-bit sums as
 * pbMoment128, value hi * 2^32 + lo, added with the two's-complement lo/hi split of pbSimMoments and NORMALISED by the
 * host to 0 <= lo < 2^32 with hi the floor quotient, as pbSimPairCorrelation does.  A measured bot that is outside adds
 * only to totals.outside; an unmeasured bot adds only to totals.unmeasured.  Per member
 *     measured = inside + outside   and   measured + unmeasured = nCells.
 * Every number is an integer: results do not depend on slot order, on the kernel form, or on the order in which the
 * device adds, and can be compared exactly.  No float atomics and no 128-bit atomics.
 * EXACTNESS.  A cell holds fewer than 2^28 bots (the batch's bound), so every half-accumulator stays below 2^60
 * (DESIGN.md 7h has the derivation): nothing wraps, whatever the state.
 * pbSimFieldMap maps every member with the same view; pbSimFieldMapOf one member into ny * nx cells and one totals row.
 * totals may be NULL.  pbSimGetFieldTimes: maps computed so far and the span of the last one's launches on the batch's
 * stream in milliseconds (HIP events), as pbSimGetSeriesTimes; either pointer may be NULL.
 * A call only reads: the state, slot layout, keys, cell lists, pbSimStats, time, RNG, the mark, the series, the time
 * correlation and every other analysis' scratch stay as they were.
 * PB_ERR_ARG, before the device is touched: a NULL handle, view or cells; a member out of range; nx or ny outside
 * 1 ... PB_FIELD_MAX_AXIS; halfX or halfY not finite or not > 0; any of x0, y0, sx, sy not finite; nsims * nx * ny * 64
 * above 2^31 bytes (pbSimFieldMapOf counts one member); a batch of 2^28 bots or more.
 * Cost: one launch that zeroes the map and the totals; one pass over posrad, velocities and dead flags in slot order
 * (28 bytes per bot, coalesced; the original indices are never read), at most PB_FIELD_BLOCKS workgroups of 256 lanes
 * per member.  The state is kept cell-sorted, so the lanes of a wave mostly share a few map cells: lanes with the same
 * cell are summed inside the wave first and go out as one 64-byte integer atomic; past a fixed number of distinct cells
 * per wave (a map finer than the blob's spacing) the rest goes out as eight 64-bit atomics per bot.  Scratch: 64 bytes
 * per cell of the largest map asked for so far plus 16 bytes per member, allocated by the first call, grown when a call
 * needs more, freed by pbSimDestroy.  Read back: the same bytes.
 * Out of scope: maps per series record; phase fields (they need a transcendental and would not be exact); per-member
 * views in one call; stress fields (the per-bot virial is pbSimContactVirialOf's); normalisation to densities; the
 * ensemble layer's summary rows; the legacy engine. */
#define PB_FIELD_MAX_AXIS 1024u
#define PB_FIELD_BLOCKS 256u /* workgroups per member: one pass of the launch covers 65536 bots of a member */
typedef struct pbFieldView { unsigned nx, ny; float centerX, centerY, halfX, halfY; } pbFieldView;
typedef struct pbFieldCell {            /* 64 bytes */
  unsigned count, dead;                 /* measured bots in the cell; those of them with dead != 0 */
  long long sum_qr, sum_wx, sum_wy;     /* units of 2^-20 */
  pbMoment128 rr, vv;                   /* sum qr*qr, sum (wx*wx + wy*wy); units of 2^-40; normalised by the host */
} pbFieldCell;
typedef struct pbFieldTotals { unsigned measured, inside, outside, unmeasured; } pbFieldTotals;  /* 16 bytes */
int pbSimFieldMap(pbSim *sim, const pbFieldView *view, pbFieldCell *cells /* nsims * ny * nx */,
                  pbFieldTotals *totals /* nsims entries, may be NULL */);
int pbSimFieldMapOf(pbSim *sim, unsigned member, const pbFieldView *view, pbFieldCell *cells /* ny * nx */,
                    pbFieldTotals *totals /* 1 entry, may be NULL */);
int pbSimGetFieldTimes(pbSim *sim, unsigned long long *maps, float *last_device_ms);

/* Structure factor on the device (csrc/pb_sfactor.hip, csrc/pb_phasor.hpp): the reciprocal-space companion of the
 * analyses above.  Per member and wavevector of a caller's list the call returns rho(k) = sum a exp(i k.r) over the
 * bots as exact integers: the phasor of a bot is one entry of an integer cosine/sine table, chosen by integer
 * arithmetic on the quantised position, so no transcendental is evaluated and every sum can be compared with ==.
 * Nothing is allocated or launched unless a structure factor is asked for.
 * NODES.  All nCells bots of a member are nodes, dead bots and the payload bot included.
 * QUANTISATION.  pbSimMoments': q = (long long)rint(v * 1048576.0f) of a value with fabsf(v) < 2048.0f, in fp32 scaling,
 * round to nearest even.  It gives qx, qy from the position, qr from rad, and wx, wy from the velocity.
 * KINDS.  PB_SK_DENSITY: weight a = 1; a bot is MEASURED iff x and y are in range.  PB_SK_RADIUS: a = qr; measured iff
 * x, y and rad are in range.  PB_SK_VELOCITY: two weights, a = wx and a2 = wy; measured iff x, y, vx and vy are in
 * range.  A NaN or an infinity is out of range.  An unmeasured bot takes part in nothing.
 * WAVEVECTORS.  The box is L = 2^e with the integer e = boxLog2, PB_SK_MIN_LOG2 <= e <= PB_SK_MAX_LOG2; L = 4096 is the
 * whole measured range.  The caller passes nvec integer pairs (nx, ny), each any int; the wavevector is
 * k = (2 pi / L)(nx, ny).
 * TURN OF A BOT.  All arithmetic is on 32-bit unsigned words and wraps mod 2^32:
 *     u = (uint32)nx * (uint32)qx + (uint32)ny * (uint32)qy
 *     t = u << (12 - e)                          k.r / 2 pi mod 1 as a 32-bit binary fraction
 *     idx = ((t + 0x80000u) >> 20) & 4095u       the phase rounded to the nearest of 4096 table steps
 * so huge |n| are well defined: they alias, as they must.
 * THE TABLE (PB_PHASOR_BITS = 12).  C[j] = rint(cos(2 pi j / 4096) * 2^30), S[j] = rint(sin(2 pi j / 4096) * 2^30), both
 * int, and S[j] = C[(j - 1024) & 4095].  The table is a property of the library, not of the host's libm: every entry
 * is at least 7e-4 away from a rounding tie, and the CRC-32 (zlib) of the 4096 interleaved little-endian int32 pairs
 * (C[j], S[j]) is 3228437924.  pbPhasorTable exports it (2 * 4096 ints, interleaved; PB_ERR_ARG on a NULL pointer or
 * cap < 8192), so tests and callers see exactly what the device adds.
 * PER MEMBER AND WAVEVECTOR, over the measured bots, one pbStructureFactorRow: nx, ny as passed; measured;
 *     re = sum a * C[idx],   im = sum a * S[idx],   and for PB_SK_VELOCITY re2, im2 with a2 (zero otherwise)
 * each a signed 128-bit sum as pbMoment128, value hi * 2^32 + lo, NORMALISED by the host to 0 <= lo < 2^32 with hi the
 * floor quotient.  Units: 2^-30 for PB_SK_DENSITY, 2^-50 otherwise.  The caller forms
 * S(k) = (re^2 + im^2) / (2^60 * measured) from the integers.
 * EXACTNESS.  |a * C| <= 2^61 and a batch has fewer than 2^28 bots, so with the two's-complement split of pbSimMoments
 * the low accumulator stays below 2^60 and the rest below 2^57 (PB_SK_DENSITY adds |C| <= 2^30 to one 64-bit word,
 * below 2^58): nothing wraps, whatever the state.  Integer adds commute: results do not depend on slot
 * order, on the kernel form or on the order in which the device adds.  No float atomics and no 128-bit atomics.
 * ERROR AGAINST THE CONTINUOUS DEFINITION (derived, not measured).  Per bot the phase is off by at most pi / 4096 from
 * the table step plus 2 pi (|nx| + |ny|) 2^-21 / L from the position quantum, and the entry by 2^-30 from its rounding:
 *     |rho_device / 2^30 - rho_float64| <= measured * (pi / 4096 + 2 pi (|nx| + |ny|) 2^-21 / L + 2^-30)
 * for PB_SK_DENSITY when u does not wrap.  The mean amplitude loss is sinc(pi / 4096), about 1 - 1e-7.
 * pbSimStructureFactor computes every member's rows with the same list; pbSimStructureFactorOf one member's nvec rows.
 * pbSimGetStructureFactorTimes: analyses so far and the span of the last one's launches on the batch's stream in
 * milliseconds (HIP events), as pbSimGetFieldTimes; either pointer may be NULL.
 * A call only reads: the state, slot layout, keys, cell lists, pbSimStats, time, RNG, the mark, the series, the time
 * correlation and every other analysis' scratch stay as they were.
 * PB_ERR_ARG, before the device is touched: a NULL handle, vectors or rows; an unknown kind; boxLog2 outside
 * PB_SK_MIN_LOG2 ... PB_SK_MAX_LOG2; nvec outside 1 ... PB_SK_MAX_VECTORS; a member out of range; nsims * nvec * 80
 * above 2^31 bytes (pbSimStructureFactorOf counts one member); a batch of 2^28 bots or more.
 * Cost: measured * nvec table look-ups with 64-bit adds.  The launch grid is (tile of 256 wavevectors, bot chunk,
 * member), at most PB_SK_BLOCKS chunks per member.  A workgroup of 256 lanes keeps the table in LDS (32 KiB, cosine and
 * sine interleaved), stages 256 quantised bots at a time (posrad, and velocities for PB_SK_VELOCITY, in slot order,
 * coalesced; the original indices are never read) and walks them: every lane owns one wavevector, keeps its sums in
 * registers and reads the same bot as its neighbours, so nothing is reduced per (bot, k); at the end a lane adds its
 * sums into the (member, k) cell with 64-bit integer atomics.  Scratch: the table and the list (32 KiB each), 4 bytes
 * per member, and 16 / 32 / 64 bytes per member and wavevector (density / radius / velocity) of the largest call so
 * far, allocated by the first call, grown when a call needs more, freed by pbSimDestroy.
 * Out of scope: per-lag k-space quantities other than the self-intermediate scattering function (pbSimSetScattering,
 * below) and the coherent one (pbSimSetCoherent, further below); phase moments, phase
 * correlations and phase fields on the table; a finer table or an angle-addition refinement; radial averaging of S(k)
 * and normalisations; records inside the series ring; the ensemble layer's summary rows; the legacy engine. */
#define PB_SK_MAX_VECTORS 4096u
enum { PB_SK_MIN_LOG2 = -8, PB_SK_MAX_LOG2 = 12 };
#define PB_SK_BLOCKS 256u /* bot chunks per member and tile of wavevectors: one pass covers 65536 bots of a member */
#define PB_PHASOR_BITS 12
enum { PB_SK_DENSITY = 0, PB_SK_RADIUS = 1, PB_SK_VELOCITY = 2 };
typedef struct pbStructureFactorRow {   /* 80 bytes */
  int nx, ny;                           /* the wavevector's integers, as passed */
  unsigned measured, reserved;          /* measured bots of the member (the same in all its rows); 0 */
  pbMoment128 re, im, re2, im2;         /* units of 2^-30 (density) or 2^-50; re2, im2 zero unless PB_SK_VELOCITY */
} pbStructureFactorRow;
int pbSimStructureFactor(pbSim *sim, int kind, int boxLog2, const int *vectors /* 2 * nvec */, unsigned nvec,
                         pbStructureFactorRow *rows /* nsims * nvec, member-major */);
int pbSimStructureFactorOf(pbSim *sim, unsigned member, int kind, int boxLog2, const int *vectors, unsigned nvec,
                           pbStructureFactorRow *rows /* nvec */);
int pbSimGetStructureFactorTimes(pbSim *sim, unsigned long long *analyses, float *last_device_ms);
int pbPhasorTable(int *cosSin /* 2 * 4096, interleaved */, unsigned cap);

/* Self-intermediate scattering on the device (csrc/pb_scatter.hip): where the time correlations and the phasor kit meet.
 *     F_s(k, tau) = < (1/N) sum_i exp(i k . (r_i(t + tau) - r_i(t))) >_t
 * per member, lag and wavevector of a caller's list, averaged over time origins while pbSimStep runs, as exact integers:
 * relaxation times at a chosen wavelength, caging, and a k-resolved separation of collective drift (the imaginary part)
 * from rearrangement (the decay of the real part).  The ring, the records and the pairing are the time correlation's
 * (pbSimSetTimeCorrelation, above); the turn, the index and the table are the structure factor's.  Off by default: a run
 * that does not ask for it makes the same launches, has the same pbSimStats and the same bits.
 * pbSimSetScattering(sim, interval, lags, boxLog2, vectors, nvec).  interval follows the time correlation's rules
 * exactly: > 0 the schedule's gate, 0 every step, -1.0f manual only.  lags is 1 ... PB_SCATTER_MAX_LAGS; lags == 0
 * switches off and frees everything (boxLog2, vectors and nvec are then not read).  boxLog2 is e of the box L = 2^e,
 * PB_SK_MIN_LOG2 ... PB_SK_MAX_LOG2.  vectors holds nvec int pairs (nx, ny), nvec 1 ... PB_SCATTER_MAX_VECTORS, each any
 * int; k = (2 pi / L)(nx, ny).  The list is copied at the call.  Calling again restarts from record 0.
 * A RECORD is taken at the same instant and describes the same state as a time-correlation record.  It stores, per bot
 * of every member in ORIGINAL order, the quantised position (qx, qy) = (rint(x * 2^20), rint(y * 2^20)) (pbSimMoments'
 * quantisation, units of 2^-20): 8 bytes per bot and ring slot, into slot r % lags.  A bot whose x or y is out of range
 * (not fabsf(.) < 2048.0f; a NaN or an infinity is out of range) is stored as UNMEASURED (qx == INT32_MIN, which no
 * measured bot has: |q| <= 2^31 - 128).  Quantising once at the snapshot means that the pairing does not do it up to 64
 * times.
 * A PAIR (now, then) of a bot is MEASURED iff both instants are.  Then, on 32-bit unsigned words mod 2^32,
 *     u   = nx * (qx_now - qx_then) + ny * (qy_now - qy_then)      == u_now - u_then of the structure factor's turn
 *     t   = u << (12 - e);   idx = ((t + 0x80000u) >> 20) & 4095u
 *     re += C[idx];   im += S[idx]                                  the structure factor's table, nothing new
 * The displacement here is the DIFFERENCE OF THE QUANTISED POSITIONS, not the quantised fp32 difference that the time
 * correlation uses: only this choice makes the turn linear in the position and exact.
 * PAIRING.  Record r is paired with the records r - l for l = 0 ... min(r, lags - 1).  Lag 0 pairs a record with itself:
 * re = samples * 2^30, im = 0.
 * PER MEMBER, LAG AND WAVEVECTOR one pbScatteringRow: lag in RECORDS; nx, ny as passed; origins, sum_steps and samples
 * as in pbTimeCorrelationRow (samples is the same for every vector of a member and lag); re and im in units of 2^-30.
 * The caller forms F_s = re / (2^30 samples) and the imaginary part likewise.
 * EXACTNESS.  |C|, |S| <= 2^30, so a cell with fewer than 2^31 samples keeps |re|, |im| < 2^61 in one signed 64-bit
 * word: no split accumulators, no float atomics, no 128-bit atomics.  Integer adds commute: results do not depend on
 * slot order, on the kernel form that stepped or on the order in which the device adds.  pbSimGetScattering checks the
 * counts it is about to return, and if a cell holds 2^31 samples or more it answers PB_ERR_ARG ("a lag holds 2^31
 * samples or more: restart the scattering") and writes no rows.
 * ERROR AGAINST THE CONTINUOUS DEFINITION (derived, not measured).  Per measured pair the phase is off by at most
 *     pi / 4096  +  2 pi (|nx| + |ny|) 2^-20 / L
 * (the table step, plus two position quanta of 2^-21 each per axis, one per instant), and the table entry by 2^-30 from
 * its rounding; cos and sin have slope at most 1, so, when u does not wrap,
 *     |re / (2^30 samples) - mean cos(k . dr)| <= pi / 4096 + 2 pi (|nx| + |ny|) 2^-20 / L + 2^-30
 * with dr the float64 difference of the fp32 positions, and the same for im and sin.
 * OTHER CALLS.  pbSimScatteringRecord: one record now, of the state as it is, whatever the interval.
 * pbSimGetScatteringInfo: interval, lags (0: off), boxLog2, nvec and the records taken so far; any pointer may be NULL,
 * not all.  pbSimGetScattering: nsims * lags * nvec rows, member-major, then the lag, then the vector in list order; a
 * lag that no record has reached yet has origins == 0 and zeros.  pbSimGetScatteringTimes: records so far and the span of
 * the last record's launches on the batch's stream in milliseconds (HIP events); either pointer may be NULL.
 * When several records are due in front of a step the order is: series, time correlation, scattering.  No launch is
 * fused across the scattering's gate and a resident stretch ends in front of it, as for the other two.
 * The scattering ring is not part of a checkpoint: pbSimSetState*, pbSimSetTime and pbSimSetLayoutOf leave it alone;
 * pbSimDestroy frees it.  Recording never waits for the device.  It only reads: the state, slot layout, keys, cell
 * lists, pbSimStats, time, RNG, the mark, the series, the time correlation and every other analysis' scratch stay as
 * they were.
 * PB_ERR_ARG, before the device is touched: a NULL handle, vectors or rows; interval NaN, infinite, or negative other
 * than -1; lags > PB_SCATTER_MAX_LAGS; boxLog2 outside PB_SK_MIN_LOG2 ... PB_SK_MAX_LOG2; nvec outside
 * 1 ... PB_SCATTER_MAX_VECTORS; a ring above 2^33 bytes (lags x total x 8); a table above 2^31 bytes (nsims x lags x
 * nvec x 16); a batch of 2^28 bots or more or of more than 65535 members; the pointers of pbSimGetScatteringInfo all
 * NULL; a record or a read with the scattering off.
 * Cost: a record is one pass over posrad and original indices in slot order that scatters 8 bytes per bot into the ring,
 * and one launch for all lags: one workgroup of 256 lanes per (member, lag, bot block), at most PB_SCATTER_BLOCKS blocks
 * per member and lag.  A workgroup keeps the table in LDS (32 KiB), stages 256 displacements at a time from coalesced
 * 8-byte loads of the two snapshots and walks them with its lanes laid out as (stripe, vector): nvec is rounded up to a
 * power of two Vp, and 256 / Vp stripes each take their share of the tile, so that 8 ... 64 vectors keep every lane
 * busy.  A lane owns one vector and keeps re and im in registers; at the end the stripes of a wave are folded with
 * shuffles and one lane per wave and vector adds into the cell with 64-bit integer atomics.  Read back: 16 bytes per
 * (member, lag, vector) and 8 per (member, lag).
 * Out of scope: weights other than 1; logarithmic lag spacing; the ensemble layer's summary rows;
 * the legacy engine.  (The coherent F(k, tau), a product of two rho(k) sums, has a recorder of its own:
 * pbSimSetCoherent, below.  So has chi_4, whose phasor sum is squared once per origin: pbSimSetFourPoint, further
 * below.) */
#define PB_SCATTER_MAX_LAGS 64u
#define PB_SCATTER_MAX_VECTORS 256u
#define PB_SCATTER_BLOCKS 256u /* workgroups per member and lag: one pass covers 65536 bots of a member */
typedef struct pbScatteringRow {       /* 56 bytes */
  unsigned lag;                        /* lag in RECORDS: record r against record r - lag */
  int nx, ny;                          /* the wavevector's integers, as passed */
  unsigned reserved;                   /* 0 */
  unsigned long long origins;          /* record pairs added so far (the same for every member and vector) */
  unsigned long long sum_steps;        /* sum over those pairs of step(r) - step(r - lag) */
  unsigned long long samples;          /* measured (bot, origin) pairs (the same for every vector of a member and lag) */
  long long re, im;                    /* sum C[idx], sum S[idx]; units of 2^-30 */
} pbScatteringRow;
int pbSimSetScattering(pbSim *sim, float interval, unsigned lags, int boxLog2, const int *vectors /* 2 * nvec */,
                       unsigned nvec);
int pbSimScatteringRecord(pbSim *sim);   /* one record now, of the state as it is */
int pbSimGetScatteringInfo(pbSim *sim, float *interval, unsigned *lags, int *boxLog2, unsigned *nvec,
                           unsigned long long *records);
int pbSimGetScattering(pbSim *sim, pbScatteringRow *rows /* nsims * lags * nvec: member, lag, vector */);
int pbSimGetScatteringTimes(pbSim *sim, unsigned long long *records, float *last_device_ms);

/* Self van Hove function on the device (csrc/pb_vanhove.hip): the distribution whose moments the time correlation gives.
 *     G_s(r, tau) = < (1/N) sum_i delta(r - (r_i(t + tau) - r_i(t))) >_t
 * per member and lag as exact integer histograms, averaged over time origins while pbSimStep runs: a histogram of the
 * displacement's length, one of each signed component (the drift towards the light skews these), and the sums of the
 * second and fourth powers, from which the non-Gaussian parameter alpha_2 follows.  The ring, the records and the
 * pairing are the time correlation's (pbSimSetTimeCorrelation, above).  Off by default: a run that does not ask for it
 * makes the same launches, has the same pbSimStats and the same bits, and nothing is allocated.
 * pbSimSetVanHove(sim, interval, lags, binWidth, bins).  interval follows the time correlation's rules exactly: > 0 the
 * schedule's gate, 0 every step, -1.0f manual only.  lags is 1 ... PB_VANHOVE_MAX_LAGS; lags == 0 switches off and
 * frees everything (binWidth and bins are then not read).  bins is 1 ... PB_VANHOVE_MAX_BINS.  binWidth is finite, > 0
 * and < 2048, and its quantised value qw = rint(binWidth * 2^20) (pbSimMoments' quantisation) must be >= 1.  Calling
 * again restarts from record 0 with a zeroed table.
 * A RECORD is taken at the same instant and describes the same state as a time-correlation record.  It stores, per bot
 * of every member in ORIGINAL order, the fp32 position (x, y): 8 bytes per bot and ring slot, into slot r % lags.
 * A PAIR (now, then) of a bot is MEASURED iff dx = x_now - x_then and dy = y_now - y_then, formed in fp32, both satisfy
 * fabsf(.) < 2048.0f: the time correlation's rule without its velocity terms; a NaN or an infinity fails it.  Then
 *     qx = rint(dx * 2^20),  qy = rint(dy * 2^20),  s = qx^2 + qy^2 < 2^63
 * which is the s of the time correlation: the histogram is the distribution whose second moment its msd is.
 * PAIRING.  Record r is paired with the records r - l for l = 0 ... min(r, lags - 1).  Lag 0 pairs a record with itself:
 * every measured pair lands in radial bin 0 and in index bins of x and of y.
 * PER MEMBER AND LAG, over the measured (bot, origin) pairs:
 *   RADIAL HISTOGRAM, bins counters.  The edges are E_k = min((k qw)^2, 2^63) for k = 0 ... bins, computed by the host
 *     in 128-bit arithmetic and held as 64-bit words.  A pair goes to bin b = max{k : E_k <= s} iff s < E_bins, else to
 *     beyond_r.  An edge belongs to the upper bin; a displacement of zero lands in bin 0.
 *   AXIS HISTOGRAMS, 2 bins counters each for x and y.  bx = floor(qx / qw), floor towards minus infinity, is counted at
 *     index bx + bins iff -bins <= bx < bins, else in beyond_x; the same for y.  Index j covers
 *     [(j - bins) qw, (j - bins + 1) qw).
 *   MOMENTS.  samples; msd = sum s, a 128-bit sum as pbMoment128 (NORMALISED: 0 <= lo < 2^32, hi the floor quotient),
 *     units of 2^-40; q4 = sum s^2, 192 bits as three little-endian 64-bit limbs, units of 2^-80.
 * These identities hold whatever the state:
 *     sum radial + beyond_r = samples,   sum x + beyond_x = samples,   sum y + beyond_y = samples.
 * The caller forms <r^2> = msd / (2^40 samples), <r^4> = q4 / (2^80 samples) and, in two dimensions,
 * alpha_2 = <r^4> / (2 <r^2>^2) - 1.
 * One pbVanHoveRow per member and lag: lag in RECORDS; origins, sum_steps and samples as in pbTimeCorrelationRow.
 * EXACTNESS.  The bins are found in integers: a binary search in the exact edges and an integer division, no floating
 * point guess.  s splits into two 64-bit accumulators as the time correlation's msd.  s^2 < 2^126 is the 128-bit
 * product, added as its four 32-bit pieces to four 64-bit accumulators: each gains less than 2^32 per sample, so with
 * fewer than 2^31 samples none wraps, and the host composes a0 + a1 2^32 + a2 2^64 + a3 2^96.  Integer adds commute:
 * results do not depend on slot order, on the kernel form that stepped or on the order in which the device adds.  No
 * float atomics and no 128-bit atomics.  pbSimGetVanHove checks the counts it is about to return, and if a cell holds
 * 2^31 samples or more it answers PB_ERR_ARG ("a lag holds 2^31 samples or more: restart the van Hove function") and
 * writes nothing.
 * OTHER CALLS.  pbSimVanHoveRecord: one record now, of the state as it is, whatever the interval.
 * pbSimGetVanHoveInfo: interval, lags (0: off), binWidth, bins and the records taken so far; any pointer may be NULL,
 * not all.  pbSimGetVanHove: nsims * lags rows, member-major, and nsims * lags * 5 * bins counters, per member and lag
 * the bins radial counters, then the 2 bins of x, then the 2 bins of y; either pointer may be NULL, not both; a lag
 * that no record has reached yet has origins == 0 and zeros.  pbSimGetVanHoveTimes: records so far and the span of the
 * last record's launches on the batch's stream in milliseconds (HIP events); either pointer may be NULL.
 * When several records are due in front of a step the order is: series, time correlation, scattering, van Hove.  No
 * launch is fused across the gate and a resident stretch ends in front of it, as for the other three.
 * The ring is not part of a checkpoint: pbSimSetState*, pbSimSetTime and pbSimSetLayoutOf leave it alone; pbSimDestroy
 * frees it.  Recording never waits for the device.  It only reads: the state, slot layout, keys, cell lists,
 * pbSimStats, time, RNG, the mark, the series, the time correlation, the scattering and every other analysis' scratch
 * stay as they were.
 * PB_ERR_ARG, before the device is touched: a NULL handle; rows and counts both NULL; interval NaN, infinite, or
 * negative other than -1; lags > PB_VANHOVE_MAX_LAGS; bins outside 1 ... PB_VANHOVE_MAX_BINS; binWidth not in (0, 2048)
 * or below half a quantum; a ring above 2^33 bytes (lags x total x 8); a table above 2^31 bytes (nsims x lags x
 * (10 + 5 bins) x 8); a batch of 2^28 bots or more or of more than 65535 members; the pointers of pbSimGetVanHoveInfo
 * all NULL; a record or a read with the analysis off.
 * Cost: a record is one pass over posrad and original indices in slot order that scatters 8 bytes per bot into the ring,
 * and one launch for all lags: one workgroup of 256 lanes per (member, lag, bot block), at most PB_VANHOVE_BLOCKS blocks
 * per member and lag.  A workgroup keeps the edges (8 KiB at most) and a histogram of 5 bins 32-bit counters (20 KiB at
 * most) in LDS, reads the two snapshots as coalesced 8-byte loads, adds three LDS counters per pair and keeps the
 * moments in registers; at the end each non-zero counter is one 64-bit integer atomic into the cell.  Device memory:
 * the ring, (10 + 5 bins) x 8 bytes per member and lag, and (bins + 1) x 8 bytes of edges.
 * Out of scope: logarithmic bins or lag spacing; a two-dimensional histogram of (dx, dy);
 * displacements relative to the centroid; the ensemble layer's summary rows; the legacy engine. */
#define PB_VANHOVE_MAX_LAGS 64u
#define PB_VANHOVE_MAX_BINS 1024u
#define PB_VANHOVE_BLOCKS 256u /* workgroups per member and lag: one pass covers 65536 bots of a member */
typedef struct pbVanHoveRow {          /* 96 bytes */
  unsigned lag, reserved;              /* lag in RECORDS: record r against record r - lag; 0 */
  unsigned long long origins;          /* record pairs added so far (the same for every member) */
  unsigned long long sum_steps;        /* sum over those pairs of step(r) - step(r - lag) */
  unsigned long long samples;          /* measured (bot, origin) pairs */
  unsigned long long beyond_r;         /* measured pairs with s >= E_bins */
  unsigned long long beyond_x;         /* ... with floor(qx / qw) outside -bins ... bins - 1 */
  unsigned long long beyond_y;
  pbMoment128 msd;                     /* sum s; units of 2^-40 */
  unsigned long long q4[3];            /* sum s^2, 192 bits little-endian; units of 2^-80 */
} pbVanHoveRow;
int pbSimSetVanHove(pbSim *sim, float interval, unsigned lags, float binWidth, unsigned bins);
int pbSimVanHoveRecord(pbSim *sim);   /* one record now, of the state as it is */
int pbSimGetVanHoveInfo(pbSim *sim, float *interval, unsigned *lags, float *binWidth, unsigned *bins,
                        unsigned long long *records);
int pbSimGetVanHove(pbSim *sim, pbVanHoveRow *rows /* nsims * lags, or NULL */,
                    unsigned long long *counts /* nsims * lags * 5 * bins: radial | x | y, or NULL; not both NULL */);
int pbSimGetVanHoveTimes(pbSim *sim, unsigned long long *records, float *last_device_ms);

/* Distinct van Hove function on the device (csrc/pb_vanhove_distinct.hip): the other half of the van Hove function,
 *     G_d(r, tau) = < (1/N) sum_i sum_{j != i} delta(r - |r_j(t + tau) - r_i(t)|) >_t
 * per member and lag as an exact integer histogram of ordered pairs, averaged over time origins while pbSimStep runs:
 * where the OTHER bots are, tau later, relative to where a bot was.  Its tau = 0 limit is the radial pair count behind
 * g(r); its decay says how long the neighbour shells survive, the filling of the hole at r = 0 when bots take each
 * other's places.  Off by default: a run that does not ask for it makes the same launches, has the same pbSimStats and
 * the same bits, and nothing is allocated.
 * pbSimSetVanHoveDistinct(sim, interval, lags, binWidth, bins).  interval and lags (1 ... PB_VANHOVE_MAX_LAGS) follow
 * the time correlation's rules exactly: > 0 the schedule's gate, 0 every step, -1.0f manual only; lags == 0 switches off
 * and frees everything (binWidth and bins are then not read).  bins is 1 ... PB_VANHOVE_MAX_BINS.  binWidth is finite,
 * > 0, and its quantised value qw = rint(binWidth * 2^20) (pbSimMoments' quantisation) must be >= 1 and satisfy
 * qw * bins < 2^31: rMax = bins * binWidth < 2048, so no edge saturates and every pair in range is inside the
 * fixed-point bound.  Calling again restarts from record 0 with a zeroed table.
 * A RECORD is taken at the same instant and describes the same state as a time-correlation record.  A bot is PRESENT
 * at a record iff x, y and rad are all finite (the rule by which every analysis files its bots).  The ring stores,
 * per bot of every member in ORIGINAL order, the fp32 position (x, y), NaN for an absent bot: 8 bytes per bot and ring
 * slot, into slot r % lags.  Results are guaranteed for |x|, |y| <= 2^20, as for every analysis that files.
 * PAIRING.  Record r is paired with the records r - l for l = 0 ... min(r, lags - 1).  For a lag every ORDERED pair
 * (i at the earlier record, j at the later record) of one member takes part whose original indices differ, with i
 * present then and j present now.  With dx = x_j(now) - x_i(then) and dy = y_j(now) - y_i(then) formed in fp32 without
 * contraction: if fabsf(dx) < 2048 and fabsf(dy) < 2048,
 *     qx = rint(dx * 2^20),  qy = rint(dy * 2^20),  s = qx^2 + qy^2
 * and the pair is counted in radial bin b = max{k : (k qw)^2 <= s} iff s < (bins qw)^2: pbSimSetVanHove's radial edges
 * and rule.  An edge belongs to the upper bin; coincident bots land in bin 0.  Pairs out of range are counted nowhere.
 * The self pair i == j is excluded even when another bot sits exactly on i's old position (that other pair is counted).
 * With the same width and bins, radial_self[k] + radial_distinct[k] is the histogram over all ordered (i, j) pairs.
 * Lag 0 pairs a record with itself: the ordered pair counts of that state, so every count is even.
 * One pbVanHoveDistinctRow per member and lag: lag in RECORDS; origins and sum_steps as in pbTimeCorrelationRow; centres,
 * the sum over the origins of the bots present at the earlier record; partners, the same at the later record; pairs,
 * the sum of the lag's histogram, formed by the host.  Plus bins 64-bit counters per member and lag.
 * EXACTNESS.  The bin starts from an fp32 guess and is settled by integer comparisons with the exact 64-bit edges,
 * E_b <= s < E_(b + 1), which hold whatever the guess was.  Everything added is an integer: results do not
 * depend on slot order, on the kernel form that stepped or on the order in which the device adds.  No float atomics and
 * no 128-bit atomics.  pbSimGetVanHoveDistinct checks centres, and if a lag holds 2^31 or more it answers PB_ERR_ARG
 * ("a lag holds 2^31 samples or more: restart the distinct van Hove function") and writes nothing.
 * OTHER CALLS, shaped as the self part's.  pbSimVanHoveDistinctRecord: one record now, whatever the interval.
 * pbSimGetVanHoveDistinctInfo: interval, lags (0: off), binWidth, bins and the records so far; any pointer may be NULL,
 * not all.  pbSimGetVanHoveDistinct: nsims * lags rows, member-major, and nsims * lags * bins counters; either pointer
 * may be NULL, not both; a lag that no record has reached yet has origins == 0 and zeros.
 * pbSimGetVanHoveDistinctTimes: records so far and the span of the last record's launches in milliseconds.
 * When several records are due in front of a step the order is: series, time correlation, scattering, van Hove,
 * distinct van Hove.  No launch is fused across the gate and a resident stretch ends in front of it.
 * The ring is not part of a checkpoint.  Recording never waits for the device and only reads the simulation.  It does
 * re-file the analysis layer's shared scratch, exactly as any on-demand analysis call does (the setter makes that
 * scratch, so that no record allocates); it leaves alone the rearrangement mark, every analysis' result buffers, and
 * every clock and run counter of the on-demand analyses.
 * PB_ERR_ARG, before the device is touched: a NULL handle; rows and counts both NULL; interval NaN, infinite, or
 * negative other than -1; lags > PB_VANHOVE_MAX_LAGS; bins outside 1 ... PB_VANHOVE_MAX_BINS; binWidth not in (0, 2048)
 * or below half a quantum; qw * bins >= 2^31; a ring above 2^33 bytes (lags x total x 8); a table above 2^31 bytes
 * (nsims x lags x (2 + bins) x 8); a batch of 2^28 bots or more or of more than 65535 members; the pointers of
 * pbSimGetVanHoveDistinctInfo all NULL; a record or a read with the analysis off.
 * Cost: a record files the bots on a grid of edge rMax (1 + 2^-10) (the sort of pbSimRadialCounts), copies (x, y) of the
 * filed bots into the ring, and makes one launch for all lags: grid (blocks of 256 bots, member, lag).  A lane reads its
 * bot's earlier position (an 8-byte gather) and walks the nine cells around THAT position over the current filing, so
 * the work per lag is that of one pbSimRadialCounts at rMax counting both ends.  A workgroup keeps the edges (8 KiB at
 * most) and bins 32-bit counters (4 KiB at most) in LDS; at the end each non-zero counter is one 64-bit integer atomic.
 * Device memory: the ring, (2 + bins) x 8 bytes per member and lag, (bins + 1) x 8 bytes of edges, the shared scratch.
 * Out of scope: angle-resolved or two-dimensional (dx, dy) histograms; normalisation to g(r) or a density; one ring for
 * the self and the distinct part; logarithmic bins or lag spacing; chi_4; the ensemble layer's summary rows; the legacy
 * engine.  (The reciprocal-space companion is pbSimSetCoherent, below.) */
typedef struct pbVanHoveDistinctRow {  /* 48 bytes */
  unsigned lag, reserved;              /* lag in RECORDS: record r against record r - lag; 0 */
  unsigned long long origins;          /* record pairs added so far (the same for every member) */
  unsigned long long sum_steps;        /* sum over those pairs of step(r) - step(r - lag) */
  unsigned long long centres;          /* sum over the origins of the bots present at the earlier record */
  unsigned long long partners;         /* ... at the later record */
  unsigned long long pairs;            /* ordered pairs counted: the sum of the lag's histogram */
} pbVanHoveDistinctRow;
int pbSimSetVanHoveDistinct(pbSim *sim, float interval, unsigned lags, float binWidth, unsigned bins);
int pbSimVanHoveDistinctRecord(pbSim *sim);   /* one record now, of the state as it is */
int pbSimGetVanHoveDistinctInfo(pbSim *sim, float *interval, unsigned *lags, float *binWidth, unsigned *bins,
                                unsigned long long *records);
int pbSimGetVanHoveDistinct(pbSim *sim, pbVanHoveDistinctRow *rows /* nsims * lags, or NULL */,
                            unsigned long long *counts /* nsims * lags * bins, or NULL; not both NULL */);
int pbSimGetVanHoveDistinctTimes(pbSim *sim, unsigned long long *records, float *last_device_ms);

/* Coherent intermediate scattering on the device (csrc/pb_coherent.hip; the arithmetic is csrc/pb_coherent.hpp): the
 * collective companion of pbSimSetScattering in reciprocal space, as the distinct van Hove function is in real space.
 *     F(k, tau) = < (1/N) rho_k(t + tau) conj(rho_k(t)) >_t ,    rho_k(t) = sum_i exp(i k . r_i(t))
 * per member, lag and wavevector of a caller's list, averaged over time origins while pbSimStep runs, as exact integers:
 * how a density fluctuation of a given wavelength decays (the real part) or travels (the imaginary part).  With the same
 * list given to both recorders F - F_s is the distinct part in k-space, and lag 0 is the time-averaged S(k).  The book,
 * the records and the pairing are the time correlation's (pbSimSetTimeCorrelation, above); the nodes, the measured rule,
 * the turn, the index and the table are the structure factor's.  Off by default: a run that does not ask for it makes
 * the same launches, has the same pbSimStats and the same bits, and nothing is allocated.
 * pbSimSetCoherent(sim, interval, lags, boxLog2, vectors, nvec).  interval, lags, boxLog2 and the list follow
 * pbSimSetScattering exactly: interval > 0 the schedule's gate, 0 every step, -1.0f manual only.  lags is
 * 1 ... PB_COHERENT_MAX_LAGS; lags == 0 switches off and frees everything (boxLog2, vectors and nvec are then not read).
 * boxLog2 is e of the box L = 2^e, PB_SK_MIN_LOG2 ... PB_SK_MAX_LOG2.  vectors holds nvec int pairs (nx, ny), nvec
 * 1 ... PB_COHERENT_MAX_VECTORS, each any int; k = (2 pi / L)(nx, ny).  The list is copied at the call.  Calling again
 * restarts from record 0 with a zeroed table.
 * A RECORD is taken at the same instant and describes the same state as the other recorders' records.  Nodes, the
 * measured rule and the quantisation are PB_SK_DENSITY's: every bot of a member is a node, and a bot is MEASURED iff x
 * and y are in range.  Per member and wavevector the record computes the MODE
 *     (C, S) = (sum C[idx], sum S[idx])   over the measured bots, units of 2^-30
 * with the turn, the index and the table of pbSimStructureFactor, and the member's measured count.  By definition these
 * are the re, im and measured of pbSimStructureFactor(PB_SK_DENSITY) for the same state, list and box.  They go into
 * slot r % lags of a ring of modes: 16 bytes per (slot, member, vector) and 4 per (slot, member).  No per-bot snapshot
 * is kept, and the N x nvec table look-ups are done once per record, not once per lag.
 * PAIRING.  Record r is paired with the records r - l for l = 0 ... min(r, lags - 1).  Per member, lag and vector, on
 * exact integers:
 *     re += C_now * C_then + S_now * S_then
 *     im += S_now * C_then - C_now * S_then
 *     bots_now += measured_now
 *     bots_then += measured_then
 * which is rho_now conj(rho_then) in units of 2^-60.  Lag 0 pairs a record with itself: im == 0 and
 * re = sum (C^2 + S^2), the summed numerators of S(k).
 * EXACTNESS.  |C|, |S| <= measured * 2^30 < 2^58 (a batch has fewer than 2^28 bots).  So each product is below 2^116 in
 * magnitude and each of re's and im's increments, a sum or a difference of two products, below 2^117.  With fewer than
 * 2^31 origins a sum stays below 2^148: a signed 192-bit two's-complement word in three little-endian 64-bit limbs holds
 * it, whatever the state.  A (member, lag, vector) cell has one owner on the device, which adds with carries through
 * the limbs: no atomic wider than 64 bits and no float atomics.  Integer adds commute: results do not depend on slot
 * order, on the kernel form that stepped or on the order in which the device adds.  pbSimGetCoherent answers PB_ERR_ARG
 * ("a lag holds 2^31 origins or more: restart the coherent scattering") and writes nothing if a lag has 2^31 origins
 * or more; the count is the host's own, so nothing is read back first.
 * PER MEMBER, LAG AND WAVEVECTOR one pbCoherentRow: lag in RECORDS; nx, ny as passed; origins and sum_steps as in
 * pbScatteringRow; bots_now and bots_then, the measured counts of the later and of the earlier record summed over the
 * origins (the same for every vector of a member and lag); re and im, each value = limb[0] + limb[1] 2^64 + limb[2] 2^128
 * read as a signed 192-bit two's-complement word, units of 2^-60.  The caller forms F = re / (2^60 * bots_then) and the
 * imaginary part likewise.
 * ERROR AGAINST THE CONTINUOUS DEFINITION (derived, not measured).  Let eps be the per-bot bound of pbSimStructureFactor,
 *     eps = pi / 4096 + 2 pi (|nx| + |ny|) 2^-21 / L + 2^-30.
 * As a complex number a bot's table entry is within eps of exp(i k.r): the chord is no longer than the phase error, and
 * the two roundings of at most 2^-31 each move the entry by less than 2^-30.  So each mode is within measured * eps of
 * its float64 value, in magnitude, and a float64 mode is at most measured in magnitude.  With
 * (a + da) conj(b + db) - a conj(b) = a conj(db) + da conj(b) + da conj(db), each origin's product is within
 *     measured_now * measured_then * (2 eps + eps^2)
 * of the float64 product in magnitude, hence in re and in im, when u does not wrap; a sum over origins adds the bounds.
 * OTHER CALLS.  pbSimCoherentRecord: one record now, of the state as it is, whatever the interval.
 * pbSimGetCoherentInfo: interval, lags (0: off), boxLog2, nvec and the records taken so far; any pointer may be NULL,
 * not all.  pbSimGetCoherent: nsims * lags * nvec rows, member-major, then the lag, then the vector in list order; a lag
 * that no record has reached yet has origins == 0 and zeros.  pbSimGetCoherentTimes: records so far and the span of the
 * last record's launches on the batch's stream in milliseconds (HIP events); either pointer may be NULL.
 * When several records are due in front of a step the order is: series, time correlation, scattering, van Hove,
 * distinct van Hove, coherent scattering, four-point; then the centroid trail and the phase update.  No launch is fused
 * across the gate and a resident stretch ends in front of it.
 * The ring is not part of a checkpoint: pbSimSetState*, pbSimSetTime and pbSimSetLayoutOf leave it alone; pbSimDestroy
 * frees it.  Recording never waits for the device.  It only reads: the state, slot layout, keys, cell lists,
 * pbSimStats, time, RNG, the mark and every other recorder's and analysis' memory stay as they were.
 * PB_ERR_ARG, before the device is touched: a NULL handle, vectors or rows; interval NaN, infinite, or negative other
 * than -1; lags > PB_COHERENT_MAX_LAGS; boxLog2 outside PB_SK_MIN_LOG2 ... PB_SK_MAX_LOG2; nvec outside
 * 1 ... PB_COHERENT_MAX_VECTORS; a ring plus sums above 2^31 bytes (nsims x lags x nvec x (16 + 48): the modes and the
 * sums; with the cell's two counts the footprint at that bound is 2.5 GiB, see Device memory below); a batch of more
 * than 65535 members or of 2^28 bots or more (neither is asked when lags == 0: any batch may switch off); the pointers of
 * pbSimGetCoherentInfo all NULL; a record or a read with the coherent scattering off.
 * Cost: a record zeroes its slot, makes one pass over posrad in slot order (the original indices are never read) with
 * measured * nvec table look-ups, and one small launch for all lags.  The first grid is (bot block, member), at most
 * PB_COHERENT_BLOCKS blocks per member: a workgroup of 256 lanes keeps the table in LDS (32 KiB), stages 256 quantised
 * bots at a time and walks them with its lanes laid out as (stripe, vector), nvec rounded up to a power of two Vp and
 * 256 / Vp stripes, so that 8 ... 64 vectors keep every lane busy; the stripes of a wave are folded with shuffles and
 * one lane per wave and vector adds into the mode with 64-bit integer atomics.  The second has one lane per (member, lag,
 * vector): four 64 x 64 -> 128-bit products and a cell of eight 64-bit words updated with plain loads and stores.
 * Device memory: 80 bytes per (member, lag, vector), 16 of the ring's mode and 64 of the cell (48 of sums, 16 of counts);
 * 4 bytes per (member, lag) of measured counts; the phasor table and the list.  Read back: the cells.
 * Measured on one MI355X, medians of 20 records into a full ring (profiles/coherent_scattering.txt): the 10^6-bot arena
 * 0.048 / 0.080 / 0.179 ms with 8 / 24 / 256 vectors at 16 lags and the same at 64; a scattering record with the same
 * list 0.23 / 0.34 / 1.80 ms at 16 lags and 0.64 / 1.15 / 6.84 ms at 64; one pbSimStructureFactor(PB_SK_DENSITY) call
 * with its read-back, the route a caller had per sample before, 0.23 / 0.23 / 0.24 ms.  256 members of 1000 bots:
 * 0.021 / 0.025 / 0.075 ms at 16 lags and 0.024 / 0.035 / 0.182 ms at 64 (at 256 vectors the per-lag launch shows).
 * Out of scope: current correlations, that is weights other than 1 (the radius and velocity kinds have 128-bit modes and
 * would need 256-bit products); logarithmic lag spacing; radial averaging; the ensemble layer's summary rows; the
 * legacy engine.  (chi_4 and S_4(k, tau), which square a lag-dependent masked mode per origin, are pbSimSetFourPoint's,
 * next.) */
#define PB_COHERENT_MAX_LAGS 64u
#define PB_COHERENT_MAX_VECTORS 256u
#define PB_COHERENT_BLOCKS 256u /* bot blocks per member: one pass covers 65536 bots of a member */
typedef struct pbCoherentRow {         /* 96 bytes */
  unsigned lag;                        /* lag in RECORDS: record r against record r - lag */
  int nx, ny;                          /* the wavevector's integers, as passed */
  unsigned reserved;                   /* 0 */
  unsigned long long origins;          /* record pairs added so far (the same for every member and vector) */
  unsigned long long sum_steps;        /* sum over those pairs of step(r) - step(r - lag) */
  unsigned long long bots_now;         /* sum over the origins of the bots measured at the later record */
  unsigned long long bots_then;        /* ... at the earlier record */
  unsigned long long re[3], im[3];     /* signed 192-bit sums, little-endian limbs; units of 2^-60 */
} pbCoherentRow;
int pbSimSetCoherent(pbSim *sim, float interval, unsigned lags, int boxLog2, const int *vectors /* 2 * nvec */,
                     unsigned nvec);
int pbSimCoherentRecord(pbSim *sim);   /* one record now, of the state as it is */
int pbSimGetCoherentInfo(pbSim *sim, float *interval, unsigned *lags, int *boxLog2, unsigned *nvec,
                         unsigned long long *records);
int pbSimGetCoherent(pbSim *sim, pbCoherentRow *rows /* nsims * lags * nvec: member, lag, vector */);
int pbSimGetCoherentTimes(pbSim *sim, unsigned long long *records, float *last_device_ms);

/* Four-point dynamics on the device (csrc/pb_fourpoint.hip; the arithmetic is csrc/pb_fourpoint.hpp): how the overlap of
 * the time correlation FLUCTUATES, and whether the bots that stayed put form domains.
 *     Q(t, tau) = sum_i w_i ,   w_i = 1 iff bot i is within overlapRadius of where it was tau earlier
 *     W_k(t, tau) = sum_i w_i exp(i k . r_i(t))          (r_i(t) the EARLIER position of the pair)
 *     chi_4(tau) = (<Q^2> - <Q>^2) / N ,   S_4(k, tau) = (<|W_k|^2> - |<W_k>|^2) / N
 * per member, lag and wavevector of a caller's list, the averages over time origins while pbSimStep runs, as exact
 * integers: the four-point susceptibility and the structure factor of the slow bots, the standard measure of dynamic
 * heterogeneity.  The scattering recorder cannot give it (it sums phasors over origins before anything is squared) and
 * neither can the coherent one (it squares modes that do not depend on the lag): here a MASKED phasor sum is formed per
 * (origin pair, member, wavevector) and squared exactly once per origin.  The book, the records and the pairing are the
 * time correlation's (pbSimSetTimeCorrelation, above); the ring is the scattering's; the turn, the index and the table
 * are the structure factor's.  Off by default: a run that does not ask for it makes the same launches, has the same
 * pbSimStats and the same bits, and nothing is allocated.
 * pbSimSetFourPoint(sim, interval, lags, overlapRadius, boxLog2, vectors, nvec).  interval and lags follow the other
 * lagged recorders exactly: interval > 0 the schedule's gate, 0 every step, -1.0f manual only; lags is
 * 1 ... PB_FOURPOINT_MAX_LAGS; lags == 0 switches off and frees everything (the radius, boxLog2, vectors and nvec are then
 * not read).  overlapRadius is in [0, 2048), as for the time correlation.  boxLog2, vectors and nvec are the
 * scattering's: e of the box L = 2^e, PB_SK_MIN_LOG2 ... PB_SK_MAX_LOG2; nvec int pairs (nx, ny), nvec
 * 1 ... PB_FOURPOINT_MAX_VECTORS, each any int; k = (2 pi / L)(nx, ny).  The list is copied at the call.  Calling again
 * restarts from record 0 with a zeroed table.
 * A RECORD is the scattering's: per bot in ORIGINAL order the quantised position (qx, qy), or (INT32_MIN, 0) for an
 * unmeasured bot (x or y out of range), 8 bytes per bot and slot, into slot r % lags of a ring of its own.  It is taken
 * at the same instant and describes the same state as the other recorders' records.
 * A PAIR (now, then) of a bot is MEASURED iff both instants are.
 * OVERLAP.  qa = (long long)rint(overlapRadius * 1048576.0f) and a2 = qa * qa, both computed once on the host
 * (qa < 2^31).  With dqx = qx_now - qx_then and dqy likewise, as 64-bit integers: w = 1 iff the pair is measured and
 * dqx^2 + dqy^2 < a2.  The device tests |dqx| < qa && |dqy| < qa first: the sum of squares implies both, and they keep
 * every square below 2^62.  The displacement is the difference of the QUANTISED positions, the scattering's choice, not
 * the time correlation's quantised fp32 difference: the two agree wherever the fp32 difference is exact.
 * overlapRadius == 0 overlaps nothing; equality dqx^2 + dqy^2 == a2 does not overlap.
 * MODE of an origin pair.  Per member and wavevector, with the turn, the index and the table of pbSimStructureFactor
 * taken at the EARLIER position, u = nx * qx_then + ny * qy_then mod 2^32:
 *     A = sum_i w_i C[idx_i]     B = sum_i w_i S[idx_i]     Q = sum_i w_i     m = the measured pairs
 * in units of 2^-30.
 * PAIRING.  Record r is paired with the records r - l for l = 0 ... min(r, lags - 1).  On exact integers, per (member,
 * lag):
 *     samples += m     overlap += Q     overlap2 += Q^2
 * and per (member, lag, vector):
 *     re += A     im += B     power += A^2 + B^2
 * At lag 0 every measured bot overlaps itself when qa >= 1: power is then the coherent recorder's lag-0 re.
 * EXACTNESS.  A batch has fewer than 2^28 bots and a read is refused at 2^31 origins, so:
 *     Q < 2^28                       sum Q < 2^59             one 64-bit word
 *     Q^2 < 2^56                     sum Q^2 < 2^87           two little-endian limbs
 *     |A|, |B| < 2^58                sums below 2^89          signed 128-bit two's complement, two limbs
 *     A^2 + B^2 < 2^117              sum < 2^148              three limbs, as pbCoherentRow.re
 * A cell has one owner on the device, which adds with plain loads and stores and carries through the limbs: no atomic
 * wider than 64 bits and no float atomics.  Integer adds commute: results do not depend on slot order, on the kernel form
 * that stepped or on the order in which the device adds.  pbSimGetFourPoint answers PB_ERR_ARG ("a lag holds 2^31
 * origins or more: restart the four-point recorder") and writes nothing if a lag has 2^31 origins or more; the count is
 * the host's own, so nothing is read back first.
 * PER MEMBER, LAG AND WAVEVECTOR one pbFourPointRow: lag in RECORDS; nx, ny as passed; origins and sum_steps as in
 * pbScatteringRow; samples, overlap and overlap2 (the same in every vector's row of a member and lag); re, im and power.
 * The caller forms, with Nbar = samples / origins and <.> = (.) / origins,
 *     chi_4 = (<Q^2> - <Q>^2) / Nbar          S_4 = (<|W|^2> - |<W>|^2) / (2^60 Nbar).
 * ERROR AGAINST THE CONTINUOUS DEFINITION (derived, not measured).  Let eps be the per-bot bound of pbSimStructureFactor,
 *     eps = pi / 4096 + 2 pi (|nx| + |ny|) 2^-21 / L + 2^-30.
 * For a given w each mode is within Q * eps of its float64 value, in magnitude.  w itself can differ from a float64 rule
 * |r_now - r_then| < overlapRadius only for a pair whose displacement length is within two position quanta (2^-20) of
 * the radius: quantising moves each instant's position by at most half a quantum per axis, hence the displacement by
 * at most one per axis and its length by at most sqrt 2, and the radius by at most half a quantum.
 * OTHER CALLS.  pbSimFourPointRecord: one record now, of the state as it is, whatever the interval.
 * pbSimGetFourPointInfo: interval, lags (0: off), overlapRadius, boxLog2, nvec and the records taken so far; any pointer
 * may be NULL, not all.  pbSimGetFourPoint: nsims * lags * nvec rows, member-major, then the lag, then the vector in list
 * order; a lag that no record has reached yet has origins == 0 and zeros.  pbSimGetFourPointTimes: records so far and the
 * span of the last record's launches on the batch's stream in milliseconds (HIP events); either pointer may be NULL.
 * When several records are due in front of a step the order is: series, time correlation, scattering, van Hove,
 * distinct van Hove, coherent scattering, four-point; then the centroid trail and the phase update.  No launch is fused
 * across the gate and a resident stretch ends in front of it.
 * The ring is not part of a checkpoint: pbSimSetState*, pbSimSetTime and pbSimSetLayoutOf leave it alone; pbSimDestroy
 * frees it.  Recording never waits for the device.  It only reads: the state, slot layout, keys, cell lists,
 * pbSimStats, time, RNG, the mark and every other recorder's and analysis' memory stay as they were.
 * PB_ERR_ARG, before the device is touched: a NULL handle, vectors or rows; interval NaN, infinite, or negative other
 * than -1; lags > PB_FOURPOINT_MAX_LAGS; overlapRadius NaN or outside [0, 2048); boxLog2 outside
 * PB_SK_MIN_LOG2 ... PB_SK_MAX_LOG2; nvec outside 1 ... PB_FOURPOINT_MAX_VECTORS; a ring above 2^33 bytes
 * (lags x total x 8); a table above 2^31 bytes (nsims x lags x nvec x (64 + 16): the cells and the per-record modes); a
 * batch of more than 65535 members or of 2^28 bots or more; the pointers of pbSimGetFourPointInfo all NULL; a record or
 * a read with the four-point recorder off.
 * Cost: a record makes one pass over posrad and the original indices, zeroes its scratch, and does
 * N x lags x nvec table look-ups in one launch for all lags: one workgroup of 256 lanes per (member, lag, bot block), at
 * most PB_FOURPOINT_BLOCKS blocks per member and lag, keeps the table in LDS (32 KiB), stages 256 pairs at a time from
 * coalesced 8-byte loads of both snapshots as (qx_then << shift, qy_then << shift, mask), moves the tile's overlapping
 * entries to its front (a ballot prefix; the waves' counts through LDS) and walks them with its lanes laid out as
 * (stripe, vector), up to the tile's last overlapping entry: the tile's count sets the trip count, the same in every
 * lane; the stripes of a wave are folded with shuffles and one lane per wave and vector adds into the record's scratch
 * with 64-bit integer atomics; m and Q are the staging ballots' popcounts.  One more launch, a lane per (member, lag,
 * vector), folds the scratch into the cells: two 128-bit adds, two 64 x 64 -> 128-bit products and a 192-bit add.  This
 * compacted staging ships; the masked form, in which every lane walks the whole tile, is a build-time switch
 * (PB_FOURPOINT_COMPACT=0) and was measured beside it.
 * Device memory: the ring, 8 bytes per bot and lag; 80 bytes per (member, lag, vector), 64 of the cell and 16 of the
 * scratch mode; 48 bytes per (member, lag); the phasor table and the list.  Read back: the cells.
 * Measured on one MI355X, medians of 20 records into a full ring under a walk that lets 0.47 of the pairs overlap at
 * lag 1 and 0.014 at lag 63 (profiles/four_point.txt): the 10^6-bot arena 0.356 / 0.358 / 0.541 ms with 8 / 24 / 256
 * vectors at 16 lags and 0.715 / 0.790 / 1.040 ms at 64 (the masked form: 0.308 / 0.350 / 1.501 and 0.780 / 1.067 /
 * 5.442 ms); a scattering record with the same list 0.236 / 0.338 / 1.794 ms at 16 lags and 0.645 / 1.155 / 6.825 ms at
 * 64: cheaper at 8 vectors, and at 24 vectors and 16 lags; the bare pos copy of a host route 0.19 ms: cheaper than any
 * record.  256 members of 1000 bots: 0.107 / 0.119 / 0.327 ms at 16 lags and 0.352 / 0.375 / 0.707 ms at 64.
 * Out of scope: the phasor at the later position; weights other than the overlap; a mobility (fast-bot) variant;
 * logarithmic lags; radial averaging; the ensemble layer's summary rows; the legacy engine. */
#define PB_FOURPOINT_MAX_LAGS 64u
#define PB_FOURPOINT_MAX_VECTORS 256u
#define PB_FOURPOINT_BLOCKS 256u /* workgroups per member and lag: one pass covers 65536 bots of a member */
typedef struct pbFourPointRow {        /* 128 bytes */
  unsigned lag;                        /* lag in RECORDS: record r against record r - lag */
  int nx, ny;                          /* the wavevector's integers, as passed */
  unsigned reserved;                   /* 0 */
  unsigned long long origins;          /* record pairs added so far (the same for every member and vector) */
  unsigned long long sum_steps;        /* sum over those pairs of step(r) - step(r - lag) */
  unsigned long long samples;          /* sum over the origins of the measured pairs m */
  unsigned long long overlap;          /* ... of the overlapping pairs Q */
  unsigned long long overlap2[2];      /* ... of Q^2: little-endian limbs */
  unsigned long long re[2], im[2];     /* sums of A and of B: signed 128-bit, little-endian limbs; units of 2^-30 */
  unsigned long long power[3];         /* sum of A^2 + B^2: 192-bit, little-endian limbs; units of 2^-60 */
  unsigned long long reserved2;        /* 0 */
} pbFourPointRow;
int pbSimSetFourPoint(pbSim *sim, float interval, unsigned lags, float overlapRadius, int boxLog2,
                      const int *vectors /* 2 * nvec */, unsigned nvec);
int pbSimFourPointRecord(pbSim *sim);  /* one record now, of the state as it is */
int pbSimGetFourPointInfo(pbSim *sim, float *interval, unsigned *lags, float *overlapRadius, int *boxLog2,
                          unsigned *nvec, unsigned long long *records);
int pbSimGetFourPoint(pbSim *sim, pbFourPointRow *rows /* nsims * lags * nvec: member, lag, vector */);
int pbSimGetFourPointTimes(pbSim *sim, unsigned long long *records, float *last_device_ms);

/* Bond dynamics on the device (csrc/pb_bonds.hip; the arithmetic is csrc/pb_bonds.hpp): relaxation measured on a bot's
 * NEIGHBOURS instead of its own displacement.  The recorders above are all built on a bot's displacement, which for this
 * system is the wrong observable twice over: a collective that translates, turns or breathes has a decaying MSD, F_s and
 * overlap although no bot has changed its neighbours, and in two dimensions long-wavelength (Mermin-Wagner) fluctuations
 * make the plain MSD and F_s decay even in a solid.  Per member and lag, over all time origins while pbSimStep runs:
 *     the BOND-BREAKING correlation: the share of a bot's links at t that are still its links at t + tau
 *     the CAGE-RELATIVE displacement: a bot's displacement minus the mean displacement of the neighbours it had at t
 * and, on the same bots, the plain squared displacement, so that the two MSDs are compared on identical samples.  The
 * book, the records, the interval rules and the pairing are the time correlation's (pbSimSetTimeCorrelation, above); the
 * link rule is the cluster analysis' (pbSimClusterStats); the quantiser is the scattering's.  What this recorder adds is
 * a ring of NEIGHBOUR LISTS.  Off by default: a run that does not ask for it makes the same launches, has the same
 * pbSimStats and the same bits, and nothing is allocated.
 * pbSimSetBondDynamics(sim, interval, lags, linkGap, maxRadius, overlapRadius).  interval and lags follow the other
 * lagged recorders exactly: interval > 0 the schedule's gate, 0 every step, -1.0f manual only; lags is
 * 1 ... PB_BOND_MAX_LAGS; lags == 0 switches off and frees everything (the gap and the radii are then not read).
 * linkGap is the cluster analysis' gap, finite and >= 0.  maxRadius, finite and > 0, is the largest radius of a bot that
 * takes part; 2 maxRadius + linkGap < 2048.  overlapRadius is in [0, 256).  Calling again restarts from record 0 with a
 * zeroed table.  The filing's scratch is made at this call, so that no record allocates.
 * A RECORD, of the state pbSimGetState would return in front of the step:
 *   Bot i is PRESENT iff |x| < 2048 and |y| < 2048 (the scattering's rule; a NaN or an infinity fails it) and its radius
 *   is finite and <= maxRadius.  Positions and radii are the state arrays' own bits.
 *   Present bots i != j of one member are LINKED iff fl(dist - (ri + rj)) < linkGap in fp32 without contraction, dist the
 *   correctly rounded root of fl(fl(dx dx) + fl(dy dy)): the cluster analysis' rule, order of operations included.  An
 *   absent bot has no links and is nobody's neighbour.
 *   The bots are filed on a grid of edge (2 maxRadius + linkGap)(1 + 2^-10).  A linked pair has
 *   dist < ri + rj + linkGap <= 2 maxRadius + linkGap, so it is at most one cell apart and the walk over nine cells meets
 *   it; and because the edge does not depend on the device's largest radius nothing is read back: a record never waits.
 *   Per bot, in ORIGINAL order, slot r % lags of the ring keeps a HEAD of four 32-bit words (qx, qy, degree, 0), the
 *   position quantised as rint(v 2^20), and (INT32_MIN, 0, 0, 0) for an absent bot (|q| <= 2^31 - 128: the value is
 *   free); and a LIST of PB_BOND_WIDTH 32-bit words, the member-local original indices of its neighbours, strictly
 *   ascending, padded with 0xFFFFFFFF.  A bot with degree > PB_BOND_WIDTH is CROWDED at that record: its degree is
 *   stored, its list holds the first eight neighbours the walk met and is never read.  48 bytes per bot and slot, heads
 *   and lists in arrays of their own: the neighbours' heads are gathered at random, from the dense 16-byte array.
 * A PAIR of records (now; then = lag records earlier; lag 0 pairs a record with itself).  For each bot i:
 *   SAMPLED iff i is present at both records and crowded at neither.  `crowded` counts the bots that are present at both
 *   and crowded at either; such a bot takes part in nothing else.
 *   For a sampled bot t = |N_then|, w = |N_now|, kept = |N_then n N_now|: they add into bonds_then, bonds_now and
 *   bonds_kept (directed: a link counts once from each end that is sampled).  bots_unchanged counts kept == t && kept == w,
 *   bots_lost kept < t, bots_gained kept < w.
 *   CAGE.  Let k = t and dq_x = q_now(x) - q_then(x), as 64-bit integers, for any bot x.  Bot i is CAGED iff k >= 1,
 *   every j in N_then(i) is present now, and cx = k dq_i.x - sum_j dq_j.x and cy likewise satisfy |cx|, |cy| < 2^31.
 *   Then s = cx^2 + cy^2 is k^2 times the squared cage-relative displacement in units of 2^-40.  Per k = 1 ... 8 the cell
 *   keeps cage_samples[k - 1]; cage_overlap[k - 1], the count with s < (k qa)^2, qa = rint(overlapRadius 2^20) formed
 *   once on the host (equality does not overlap; overlapRadius == 0 overlaps nothing); and cage_q2[k - 1], the sum of s.
 *   The caller divides by k^2; nothing on the device is divided.  plain_q2 is the sum of dq_i.x^2 + dq_i.y^2 over the same
 *   caged bots, in units of 2^-40.
 * EXACTNESS.  |q| <= 2^31 - 128, so |dq| <= 2^32 - 256 < 2^32; k <= 8, so |k dq| and |sum_j dq_j| are below 2^35 and c
 * below 2^36 in magnitude: no 64-bit word wraps in front of the range test.  An accepted c has |c| < 2^31, hence
 * s < 2^63, which is added as its low 32 bits and the rest (the time correlation's split); k qa <= 8 (2^28 - 16) < 2^31,
 * so (k qa)^2 < 2^62.  dq^2 < 2^64 is one word, but dq_x^2 + dq_y^2 may pass 2^64: each square is split on its own, the
 * two low halves (below 2^33 together) into one word, the two high halves (below 2^33 too) into another.  pbSimGetBondDynamics
 * refuses a table in which a cell holds 2^31 samples or more ("a lag holds 2^31 samples or more: restart the bond
 * recorder"), so every partial sum stays below 2^64 and the composed sums are exact: cage_q2[k - 1] < 2^94 and
 * plain_q2 < 2^96.  (plain_q2.hi, a signed word, is below 2^63 while plain_q2 < 2^95: for fewer than 2^30 caged samples
 * in the cell whatever they did, and for any count if no displacement reaches 2896 world units.)  Integer adds commute:
 * results do not depend on slot order, on the kernel form that stepped or on the order in which the device adds.  No
 * float atomics and no atomic wider than 64 bits.
 * PER MEMBER AND LAG one pbBondRow: lag in RECORDS; origins and sum_steps as in pbTimeCorrelationRow; the counts; the
 * 128-bit sums as pbMoment128 (value = hi 2^32 + lo, 0 <= lo < 2^32).  The caller forms
 *     bond survival = bonds_kept / bonds_then          fraction lost = bots_lost / samples
 *     cage MSD = (sum_k cage_q2[k - 1] / k^2) / (sum_k cage_samples[k - 1]) 2^-40
 *     plain MSD = plain_q2 / (sum_k cage_samples[k - 1]) 2^-40.
 * OTHER CALLS.  pbSimBondDynamicsRecord: one record now, of the state as it is, whatever the interval.
 * pbSimGetBondDynamicsInfo: interval, lags (0: off), linkGap, maxRadius, overlapRadius and the records taken so far; any
 * pointer may be NULL, not all.  pbSimGetBondDynamics: nsims * lags rows, member-major, lag 0 first; a lag that no record
 * has reached yet has origins == 0 and zeros.  pbSimGetBondDynamicsTimes: records so far and the span of the last
 * record's launches on the batch's stream in milliseconds (HIP events); either pointer may be NULL.
 * ORDER.  The bond record is taken behind the four-point record and in front of the centroid trail and the phase update,
 * of the same state as the other recorders' records.  No launch is fused across the gate and a resident stretch ends in
 * front of it.
 * The ring is not part of a checkpoint: pbSimSetState*, pbSimSetTime and pbSimSetLayoutOf leave it alone; pbSimDestroy
 * frees it.  Recording never waits for the device.  It only reads the state, slot layout, keys, cell lists, pbSimStats,
 * time, RNG, the mark and every other recorder's memory; it re-files the bots in the analysis layer's shared scratch, as a
 * distinct van Hove record does, which every on-demand analysis re-files for itself.
 * PB_ERR_ARG, before the device is touched: a NULL handle or rows; interval NaN, infinite, or negative other than -1;
 * lags > PB_BOND_MAX_LAGS; linkGap or maxRadius negative, NaN or infinite; maxRadius == 0;
 * 2 maxRadius + linkGap >= 2048; overlapRadius NaN or outside [0, 256); a batch of more than 65535 members or of 2^28
 * bots or more; a ring above 2^33 bytes (lags x total x 48); the pointers of pbSimGetBondDynamicsInfo all NULL; a record
 * or a read with the bond recorder off.
 * Cost: a record files the bots (hash, sort, gather, cell starts), walks every bot's nine cells once (k_bond_snapshot)
 * and pairs the record with its lags in one launch (k_bond_pairs): per bot and lag two coalesced 48-byte entries and
 * 2 k random 16-byte gathers, k the bot's earlier degree.  Device memory: 48 bytes per bot and lag, 336 bytes per
 * (member, lag).  Read back: the cells.  profiles/bond_dynamics.txt has the registers and the measurements.
 * Out of scope: per-bot outputs; logarithmic lags; lists wider than 8; a rotation-corrected cage (the Falk-Langer fit per
 * lag); neighbour exchange (T1) counting; the ensemble layer's summary rows; the legacy engine. */
#define PB_BOND_MAX_LAGS 64u
#define PB_BOND_BLOCKS 256u /* workgroups per member and lag: one pass covers 65536 bots of a member */
#define PB_BOND_WIDTH 8u    /* neighbours a bot's list holds; a bot with more is crowded */
typedef struct pbBondRow {             /* 360 bytes */
  unsigned lag, reserved;              /* lag in RECORDS: record r against record r - lag; 0 */
  unsigned long long origins, sum_steps;                 /* the book's columns */
  unsigned long long samples, crowded; /* sampled bots; bots present at both records and crowded at either */
  unsigned long long bonds_then, bonds_now, bonds_kept;  /* directed */
  unsigned long long bots_unchanged, bots_lost, bots_gained;
  pbMoment128 plain_q2;                /* sum of dq^2 over the caged bots, units of 2^-40 */
  unsigned long long cage_samples[8], cage_overlap[8];   /* per k = 1 ... 8 earlier neighbours */
  pbMoment128 cage_q2[8];              /* sum of s = k^2 x (cage-relative displacement)^2, units of 2^-40 */
} pbBondRow;
int pbSimSetBondDynamics(pbSim *sim, float interval, unsigned lags, float linkGap, float maxRadius, float overlapRadius);
int pbSimBondDynamicsRecord(pbSim *sim);  /* one record now, of the state as it is */
int pbSimGetBondDynamicsInfo(pbSim *sim, float *interval, unsigned *lags, float *linkGap, float *maxRadius,
                             float *overlapRadius, unsigned long long *records);
int pbSimGetBondDynamics(pbSim *sim, pbBondRow *rows /* nsims * lags, member-major, lag 0 first */);
int pbSimGetBondDynamicsTimes(pbSim *sim, unsigned long long *records, float *last_device_ms);

/* Local strain and non-affine displacement D2min on the device (csrc/pb_strain.hip; the fit itself is
 * csrc/pb_strain.hpp): the Falk-Langer fit against the mark of the rearrangement analysis.  For every bot, the best
 * local affine map that carries its MARKED bond vectors onto its present ones (the local deformation gradient: strain
 * and rotation), and the residual D2min, the non-affine part.  A blob that translates, rotates or breathes has large
 * displacements and D2min = 0; a neighbourhood that rearranges has not.  Summed over a member the same moments give the
 * macroscopic deformation gradient of the whole collective.  A mark must be held (pbSimMarkReference).  Read-only: the
 * simulation, the mark, and every other analysis' buffers and answers stay bit for bit as they were.  No spatial filing:
 * the bots are not filed afresh, the walk is over the marked CSR.
 * N0(i) is bot i's marked list, p0 the marked positions, p1 the positions as they are now, raw from the state arrays
 * (not a filing's copy, which holds NaN for a bot with a non-finite radius).
 * BOND VECTORS.  For j in N0(i), all in fp32 without contraction:
 *     d0x = x0_j - x0_i;   d0y = y0_j - y0_i;   dx = x1_j - x1_i;   dy = y1_j - y1_i
 * The bond is USED iff all four values are finite and each has fabsf(.) < PB_STRAIN_REACH (8.0f); otherwise it is
 * DROPPED: counted, and it contributes nothing.  For a used bond q = (long long)rint(v * 1048576.0f) (the scaling is
 * exact, the conversion rounds to nearest even), so |q| <= 2^23 and a product of two is at most 2^46.
 * PER-BOT INTEGER MOMENTS over the used bonds, nine 64-bit words in this order:
 *     k    number of used bonds
 *     Yxx = sum q0x*q0x;   Yxy = sum q0x*q0y;   Yyy = sum q0y*q0y
 *     Xxx = sum qx*q0x;    Xxy = sum qx*q0y;    Xyx = sum qy*q0x;    Xyy = sum qy*q0y
 *     W   = sum (qx*qx + qy*qy)
 * All exact while the bot has fewer than 2^16 marked entries (every sum stays below 2^63).  A bot with more is
 * unfitted, all its bonds are counted as dropped and its moments are zero.
 * THE FIT, in binary64: every operation rounded once, no contraction, the order of operations exactly as written,
 * integers converted with round-to-nearest:
 *     a = Yxx, b = Yxy, c = Yyy;   det = a*c - b*b
 *     FITTED iff k >= 3 and det > 0
 *     Jxx = (Xxx*c - Xxy*b)/det;   Jxy = (Xxy*a - Xxx*b)/det
 *     Jyx = (Xyx*c - Xyy*b)/det;   Jyy = (Xyy*a - Xyx*b)/det
 *     d2  = W - ((Jxx*Xxx + Jxy*Xxy) + (Jyx*Xyx + Jyy*Xyy));   d2 = d2 > 0 ? d2 : 0              (units of 2^-40)
 * J maps marked bond vectors onto present ones (d ~ J d0): the identity for an unmoved neighbourhood, a rotation matrix
 * for a rotated one.  An unfitted bot has J = 0 and d2 = 0.  The device and the host (pbSimStrainOf's gradient) evaluate
 * the same function, so the device's d2 is the value the host derives from the device's moments, bit for bit.
 * PER MEMBER one pbStrainStats row; everything in it is an integer, so nothing depends on the order of the adds:
 *     fitted, unfitted (fitted + unfitted = nCells);  above: fitted bots with d2 > (double)d2Threshold * 2^40
 *     bonds_used, bonds_dropped (their sum is the member's marked directed entries)
 *     Yxx ... W   the eight sums over all used bonds of the member (fitted bots or not), pbMoment128 NORMALISED by the
 *                 host to 0 <= lo < 2^32 with hi the floor quotient; the device adds low 32 bits and the rest apart
 *     sum_d2      over fitted bots the sum of e = (unsigned long long)rint(d2); an e of 2^63 or more, which only the
 *                 rounding of an ill-conditioned fit can produce, counts as 2^63.  max_d2: the largest e
 * With F = X Y^-1 formed from the member's sums the caller has the macroscopic deformation gradient.
 * pbSimStrainStats: one row per member.  pbSimStrainOf: one member's per-bot results in ORIGINAL order: moments, 9 words
 * per bot in the order above; gradient, Jxx Jxy Jyx Jyy per bot, derived on the host from the moments with the shared
 * function; d2min, the device's value.  Any pointer may be NULL, not all three.  pbSimGetStrainTimes: calls so far and
 * the span of the last one's launches on the batch's stream in milliseconds (HIP events); either pointer may be NULL.
 * PB_ERR_ARG, before the device is touched: NULL handle; NULL rows; all three per-bot pointers NULL; member out of
 * range; d2Threshold negative, NaN or infinite; a batch of 2^28 bots or more, or of more than 65535 members; no mark held
 * ("no reference marked").
 * Cost: one pass that puts the present positions into ORIGINAL order (the mark's own scatter kernel) and one kernel with
 * a lane per bot that walks the bot's marked list and gathers two positions per entry.  No float atomics, no scratch
 * memory.  Scratch on top of the mark: 8 + 80 bytes per bot of the batch (present positions; nine moments and d2) and
 * 184 per member (the rows), allocated by the first call, kept, freed by pbSimDestroy. */
#define PB_STRAIN_REACH 8.0f
enum { PB_STRAIN_K, PB_STRAIN_YXX, PB_STRAIN_YXY, PB_STRAIN_YYY, PB_STRAIN_XXX, PB_STRAIN_XXY, PB_STRAIN_XYX,
       PB_STRAIN_XYY, PB_STRAIN_W, PB_STRAIN_MOMENTS };
typedef struct pbStrainStats {         /* 184 bytes */
  unsigned fitted, unfitted, above, reserved;        /* reserved: 0 */
  unsigned long long bonds_used, bonds_dropped;
  pbMoment128 yxx, yxy, yyy, xxx, xxy, xyx, xyy, w;  /* units of 2^-40 */
  pbMoment128 sum_d2;                                /* units of 2^-40 */
  unsigned long long max_d2;                         /* 0 with no fitted bot */
} pbStrainStats;
int pbSimStrainStats(pbSim *sim, float d2Threshold, pbStrainStats *rows /* nsims entries */);
int pbSimStrainOf(pbSim *sim, unsigned member, long long *moments /* 9 n */,
                  double *gradient /* 4 n: Jxx Jxy Jyx Jyy */, double *d2min /* n; ORIGINAL order; NULL skipped */);
int pbSimGetStrainTimes(pbSim *sim, unsigned long long *analyses, float *last_device_ms);

/* Phase-noise generator of a batch (PB_RNG_*; default PB_RNG_COUNTER).  Selecting an XORWOW kind builds
 * one 48-byte state per bot -- curand_init(member's seed, bot, 0): the 2^67-step subsequence skip is a
 * 160x160 GF(2) jump per set bit of the bot index -- and restarts the draw counter.
 * pbSimSetPhaseDraws(k) afterwards replays k draws (exact checkpoint resume). */
int pbSimSetRng(pbSim *sim, int kind);
/* The generator states of one member in ORIGINAL bot order (n x pbRngState); PB_ERR_ARG with the
 * counter generator, which has none. */
int pbSimGetRngStatesOf(pbSim *sim, unsigned member, pbRngState *states);

/* The FORMS of the exact per-step force kernel (csrc/pb_force.hip): one table shared by the dispatch and by
 * the parity tests, so that every shape that can run is enumerable.  flat 0 = reference-shaped branches
 * (force variant 0), 1 = branch-free (variants 1 and 2; whether the fast exact forms are used is decided at
 * run time per wave); lanes_per_bot as pbSimSetLanesPerBot; attraction_sums 0 = the dead-sum form (no
 * Sum|F_attr|, pbSimSetForceSums); offsets64 1 = 64-bit byte offsets in the throughput sweep (what batches of
 * 2^28 bots and more run).  Every row exists for both payload modes.  All rows give bit-identical results.
 * pbSimSelectForceForm pins a batch to row `index` (and to per-step launches: the resident form is switched
 * off); -1 returns to the automatic choices.  A dead-sum row is refused (PB_ERR_ARG) for a batch in which a
 * member reads absForce_a (constrained_contraction). */
typedef struct pbForceForm {
  int flat;
  int lanes_per_bot;
  int attraction_sums;
  int offsets64;
} pbForceForm;
int pbForceFormCount(void);
int pbForceFormGet(int index, pbForceForm *form);
int pbSimSelectForceForm(pbSim *sim, int index);
/* The per-step force kernel this batch launches next, named as rocprofv3 names it (template arguments and
 * argument types, no "void", no namespace): "k_force<false, true, 1, 1, false, true>(PbDevParams const*, ...)".
 * bench.py matches it against the signature recorded in profiles/latest_traffic*.json before quoting that
 * profile's counters.  PB_ERR_ARG when `cap` is too small. */
int pbSimForceKernelName(pbSim *sim, char *buf, size_t cap);
/* The same for row `index` of the forms table (no device needed). */
int pbForceFormKernelName(int index, int payload, char *buf, size_t cap);

/* How the streamlined kernel (force variant 3) visits a bot's 25-cell stencil: 0 row by row (the wave runs the longest
 * row of its 64 lanes, five times), 1 flattened (every lane walks its own five ranges back to back; the wave runs its
 * longest list), -1 (default) chosen for the batch at every re-sort from the trip counts of both (flattened when it
 * saves >= 7 % of the trips: random blobs -- BASELINE configs[4] steps 7-9 % faster --, not the bench lattice).  Same
 * candidates in the same order: the results do not depend on it, bit for bit.  No effect on the exact kernels.
 * pbSimGetStreamWalkTrips: the two trip counts of the last choice (0, 0 before one was made). */
int pbSimSetStreamWalk(pbSim *sim, int mode);
int pbSimGetStreamWalkTrips(pbSim *sim, unsigned long long *row_by_row, unsigned long long *flattened);

typedef struct pbSimConfig {
  int force_variant;
  int force_kind;
  int lanes_per_bot;
  int resident;
  int fast_math_ok;
  int payload;
  int rng; /* 0 PB-RNG v1 (default), 1 cuRAND-compatible XORWOW */
  int offsets64; /* 1: the throughput sweep runs with 64-bit byte offsets (batches of 2^28 bots and more) */
  int attraction_sums; /* 1: absForce_a is maintained (pbSimSetForceSums) */
  int dead_sum_form;   /* 1: the force kernel that runs is a form without Sum|F_attr| */
  int stream_walk;     /* 1: the streamlined kernel runs and walks its stencil flattened (pbSimSetStreamWalk) */
  int tail_tiles;      /* split-lane tail tiles per XCD of the next force launch (pbSimSetTailTiles; 0: none) */
  int tail_lanes;      /* lanes per bot of those tail tiles (0 when there are none) */
} pbSimConfig;
int pbSimGetConfig(pbSim *sim, pbSimConfig *cfg);

/* Shader clock under load (diagnostic for the roofline report).  Begin launches ONE sleeping wave on
 * a stream of its own that spans `seconds` of the 100 MHz real-time counter; End waits for it and
 * returns shader cycles / real time in MHz over that span.  Run the workload in between: the figure
 * is the clock the chip holds under THAT load (it lowers its clock under dense VALU work). */
typedef struct pbClockSample pbClockSample;
int pbClockSampleBegin(pbClockSample **out, double seconds);
int pbClockSampleEnd(pbClockSample *sample, double *mhz, double *seconds_sampled);

/* On-device check that the fast exact forms equal the compiler's IEEE sqrtf and division: every
 * float in the sqrt domain (pbSqrtFast, and the root of the one-transcendental pair geometry
 * pbDistUnitFast), and div_samples sampled (numerator, numerator, denominator) triples inside the
 * division domain (pbDiv2Fast; pbDistUnitFast's unit vector on sampled (d2, dx, dy)).  Reports how many
 * values were checked and how many differed.  (tools/rsq_form_test.hip is the exhaustive check of
 * pbDistUnitFast's quotients: all 2^47 mantissa pairs.) */
int pbSelfTest(unsigned long long div_samples, unsigned long long *sqrt_checked,
               unsigned long long *sqrt_mismatches, unsigned long long *div_checked,
               unsigned long long *div_mismatches);

/* The EXHAUSTIVE form of the pair-geometry check: pbDistUnitFast (as the kernels call it) for every d2 of
 * `slices` consecutive slices (of 64) of [1, 4) -- together all 2^24 mantissa x exponent-parity cases --
 * against every numerator mantissa (2^23): the root against sqrtf and both quotients against IEEE division.
 * `checked` counts (d2, numerator) pairs (2^41 per slice, ~1.5 s of one MI355X); all 64 slices are the proof
 * DESIGN.md section 4 quotes (2^47 pairs, 0 mismatches). */
/* The static-friction hold's squared-length threshold for the constant c (pbHostSqrtThreshold) against the device's
 * IEEE sqrtf: `sqrtf(x) < c` and `x < T(c)` compared for EVERY non-negative float bit pattern x (2^31, NaNs included). */
int pbSelfTestHoldThreshold(float c, unsigned long long *checked, unsigned long long *mismatches);
/* The root of the both-sums throughput form's attraction magnitude (one v_rsq_f32, one Newton step, no clamp) against
 * sqrtf for every float of [2^-96, FLT_MAX) -- a superset of what that form can hand it: 1 879 048 191 values. */
int pbSelfTestMagnitudeRoot(unsigned long long *checked, unsigned long long *mismatches);
/* The root the both-sums throughput form takes of every pair term's squared magnitude, contact terms included: for
 * every one of the 2^32 float bit patterns, either the form's wave-uniform guard sends it to sqrtf, or the clamped
 * one-Newton-step root equals sqrtf bit for bit (two NaNs count as equal).  `checked` is 2^32. */
int pbSelfTestTermRoot(unsigned long long *checked, unsigned long long *mismatches);
int pbSelfTestPairGeometry(unsigned first_slice, unsigned slices, unsigned long long *checked,
                           unsigned long long *mismatches);
/* The same for pbDiv2Fast (the division of the attraction term by gap^2): every denominator mantissa of
 * `slices` of the 64 slices of [1, 2) against every numerator mantissa: 2^40 quotients per slice, 2^46 in all. */
int pbSelfTestDivision(unsigned first_slice, unsigned slices, unsigned long long *checked,
                       unsigned long long *mismatches);

#ifdef __cplusplus
}
#endif
#endif /* PARTICLEBOT_HIP_H */
