/*
 * pfslam.h -- C-ABI of libpfslam_hip.so: the MI355X-native particle-filter SLAM
 * inner loop (disperse -> KD scan-match score -> min/max/argmax + weight
 * normalise -> single-step ICP/SVD pose -> point-cloud map update -> weighted
 * resample), the drop-in for the path the reference implements in
 * src/kernel.cu behind src/kernel.h.
 *
 * Plain pointers and sizes only: no C++ types, no torch types.  Every entry
 * point returns 0 on success, non-zero on failure (pfslam_last_error() gives
 * the message); nothing in the library calls exit() (the reference does,
 * kernel.h:42-60).  One handle = one GPU = one host thread.
 *
 * Reference interface each entry replaces (file:line under the reference repo):
 *   pfslam_create / pfslam_destroy     particleFilterInit(Scene*) / particleFilterFree()
 *                                      + particleFilterInitPC / FreePC    kernel.h:14-15,22-23 (kernel.cu:107-178,1096-1122)
 *   pfslam_step                        particleFilter(uchar4*, int frame, Lidar*)   kernel.h:16 (kernel.cu:1702-1762)
 *   pfslam_get_pose/particles/map      getPCData(...)                     kernel.h:19 (kernel.cu:803-813)
 *   pfslam_motion_update               PFMotionUpdate / kernAddNoise      kernel.cu:375-418
 *   pfslam_score_kd                    kernEvaluateParticlesKD            kernel.cu:1198-1308
 *   pfslam_measurement_update          PFMeasurementUpdateKD host logic   kernel.cu:1311-1348
 *   pfslam_icp                         transformPointICP                  kernel.cu:993-1093
 *   pfslam_update_map_kd               PFUpdateMapKD                      kernel.cu:1406-1540
 *   pfslam_resample                    PFResample / kernWeightedSample    kernel.cu:420-511
 *   pfslam_score_grid/update_map_grid  kernEvaluateParticles / PFUpdateMap kernel.cu:243-372,513-621
 *   pfslam_kd_create/insert_list/insert_node/balance   KDTree::Create/InsertList/InsertNode/Balance  kdtree.cpp:25-105
 *   pfslam_step_grid                   the frame loop of kernel.cu:1702-1762 with the 2-D stages
 *                                      PFMeasurementUpdate / PFUpdateMap  kernel.cu:307-339, 551-577
 *   pfslam_traverse                    findCorrespondenceIndexKD          kernel.cu:924-972
 *   pfslam_nearest / pfslam_register   no counterpart: the exact nearest map node, and transformPointICP iterated on the device with
 *                                      its three defects optional (see pfslam_register below)
 *   pfslam_register_batch              no counterpart: pfslam_register from many start poses in one launch, and the pick of the best run
 *   pfslam_search                      no counterpart: every pose of a window scored against a distance field of the map, the best returned
 *   pfslam_search_scan                 no counterpart: pfslam_search's window scored against a field built from another scan's end points; no map needed
 *   pfslam_search_cov, _scan_cov       no counterpart: either search, plus the weighted mean pose, 3x3 covariance and Neff of its score volume
 *   pfslam_search_wide                 no counterpart: the same winner over windows of up to 2^31 - 1 candidates, by branch and bound
 *   pfslam_search_best                 no counterpart: the best candidate of each of the N best cells of such a window, by the same descent
 *   pfslam_cast, pfslam_map_raster     no counterpart: the ranges the map predicts for a scan from any pose, by a walk through a raster of its nodes; that raster
 *   pfslam_cast_score                  no counterpart: a measured scan compared beam by beam with those ranges, reduced on the device to eight integers per pose, and the pick
 *   pfslam_topology_update, find_walls,
 *   check_loop_closure, get_topology   UpdateTopology / FindWalls / CheckLoopClosure   kernel.cu:623-795
 *   pfslam_shard_disperse / score / weights / finish   particleFilter split where a multi-GPU caller places its three
 *                                      all-gathers (no reference counterpart: the reference is single-GPU)
 */
#ifndef PFSLAM_H
#define PFSLAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* KDTree::Node (kdtree.hpp:16-27): 32 bytes, children/parent are array indices, -1 = none */
typedef struct pfslam_node {
    int32_t axis, left, right, parent;
    float x, y, z, w;
} pfslam_node;

/* Particle (sceneStructs.h:33-38): 32 bytes, pos@0 (x, y, heading), w@12, cluster@16, map ptr@24 */
typedef struct pfslam_particle {
    float x, y, theta, w;
    uint8_t cluster;
    uint8_t pad_[7];
    void *map;
} pfslam_particle;

typedef struct pfslam_config {
    int32_t n_particles;   /* PARTICLE_COUNT (kernel.cu:30), runtime here; particles owned by THIS handle */
    int32_t n_beams;       /* LIDAR_SIZE (kernel.cu:43) = 1081 */
    float map_scale_x, map_scale_y; /* Patch.scale (data/map_settings.txt: 40 40) */
    float map_res_x, map_res_y;     /* Patch.resolution (0.025).  int(scale / res) must be the same in x and y: the
                                     * reference indexes cell (x, y) as x * dim.x + y (kernel.cu:120, 539, 1438), which is
                                     * only well defined on a square grid; pfslam_create refuses anything else.  The rays' cells
                                     * come from a closed form of the reference's Bresenham walk whose product k * deltay is 32-bit:
                                     * it is exact while a ray is shorter than 46 341 cells, that is while 20 m / res stays below
                                     * that (res above about 0.43 mm).  Oblong cells (map_res_x != map_res_y) are supported by
                                     * every frame and stage call, bit for bit like square ones, the persistent lattice-cell rows
                                     * included (tests/test_gpu_oblong_cells.py); the pfslam_search* entry points refuse them where
                                     * their comments below say so */
    int32_t kd_capacity;   /* KD_MAX_SIZE (kernel.cu:77); nodes, at most 2^27 - 1.  A frame whose new walls do not fit inserts
                            * none of them and fails ("kd_capacity exhausted"; reported by the call that books the frame, see
                            * pfslam_step) -- the reference has no bound check at all */
    int32_t device;        /* HIP device ordinal */
    int32_t strict_host_mirror; /* 1 = reproduce the half-array weight read-back of kernel.cu:1341 (H11) */
    int32_t free_upload_bug;    /* 1 = reproduce kernel.cu:1475 (free list tail zero) (H6); 0 = full list */
    int32_t balance_period;     /* 100 = KDTree::Balance at frame%100==5 (kernel.cu:1707); 0 = never */
    /* multi-GPU particle sharding: this handle holds global particles [global_offset, global_offset+n_particles)
     * of global_n; RNG streams are keyed by the GLOBAL index so results do not depend on the sharding.
     * Layout: rank r owns [r * shard_stride, min((r + 1) * shard_stride, global_n)) -- every rank but the last is full,
     * the last may be shorter (not empty); the exchange buffers are padded to shard_stride so that all-gather counts are
     * equal on every rank. */
    int32_t global_offset;
    int32_t global_n;      /* 0 -> n_particles */
    int32_t shard_stride;  /* 0 -> n_particles (equal shards) */
    int32_t reserved_[2];
} pfslam_config;

typedef struct pfslam_handle pfslam_handle;

/* defaults of the reference: 1000 particles, 1081 beams, 40x40 m @ 0.025 m, kd_capacity = KD_MAX_SIZE = 10 M nodes,
 * balance_period 100, strict_host_mirror = 1 (H11 reproduced), free_upload_bug = 0 (H6 NOT reproduced: the full free list is
 * applied -- the reference's truncated upload reads uninitialised device memory, which has no defined result to match) */
void pfslam_default_config(pfslam_config *cfg);
int pfslam_create(const pfslam_config *cfg, pfslam_handle **out);
int pfslam_destroy(pfslam_handle *h);
const char *pfslam_last_error(void);
/* number of visible HIP devices, or <0 with the HIP error negated */
int pfslam_device_count(void);
/* launch on this HIP stream (hipStream_t as void*) instead of the handle's own */
int pfslam_set_stream(pfslam_handle *h, void *hip_stream);
/* books every frame in flight (see pfslam_step), then waits for the stream */
int pfslam_synchronize(pfslam_handle *h);

/* ---- whole step (kernel.h:16) ----
 * pfslam_step ENQUEUES the frame -- dispersion, scan-match, weights, ICP, map update including the insert of the new walls
 * (KDTree::InsertNode on the device), resample decided on the device -- copies the scan into a pinned slot of its own, and
 * then books the frame `lag` steps back (default 1): trace, pose, map size and deferred errors come from a 128-byte header the
 * device writes into pinned memory.  Successive calls therefore overlap the host with the device and leave no idle gap between
 * frames.  EVERY other entry point first books all frames in flight, so pfslam_step followed by any getter behaves like the
 * reference's synchronous particleFilter.  A deferred error (kd_capacity exhausted, cell list overflow) is returned by the call
 * that books the frame: the next pfslam_step, a getter, or pfslam_synchronize.  The first scan (it seeds the map on the host),
 * re-balance frames and handles with pfslam_set_topology(h, 1) are booked at once.
 * One deferred error is fatal for the handle: "a stream gate ... gave up waiting" (a cross-stream edge of the frame was not served
 * within 1 s: streams sharing a hardware queue, a multi-GPU peer that never arrived).  The launches behind that gate have run without
 * what they waited for, so map, weights and particles are undefined from that frame on; the error is sticky -- destroy the handle.
 * pfslam_set_lag: 0 = every pfslam_step books its own frame before it returns, up to 2 frames in flight. */
int pfslam_step(pfslam_handle *h, int frame, const float *scan_host);
int pfslam_set_lag(pfslam_handle *h, int frames);
/* The same frame loop with the reference's 2-D occupancy-grid stages (PFMotionUpdate kernel.cu:400-418,
 * PFMeasurementUpdate 307-339, PFUpdateMap 551-577, PFResample 447-511): pose = best particle, grid updated
 * in place.  The grid starts at -100 everywhere (kernel.cu:124) unless pfslam_set_grid replaced it. */
int pfslam_step_grid(pfslam_handle *h, int frame, const float *scan_host);

/* ---- read-back (kernel.h:19): non-owning pointers into the handle's host mirrors, valid until the next call */
int pfslam_get_pose(pfslam_handle *h, float pose[3]);
int pfslam_get_particles(pfslam_handle *h, const pfslam_particle **out, int *n);
int pfslam_get_map(pfslam_handle *h, const pfslam_node **out, int *n);
int pfslam_get_grid(pfslam_handle *h, const int8_t **grid, int *dimx, int *dimy);
/* per-step trace of the last pfslam_step: [best, resampled, n_wall, n_free, n_insert, neff(float bits), kd_size, 0] */
int pfslam_get_trace(pfslam_handle *h, int32_t out[8]);
/* ascending cell indices (x*dimx+y) of the last map update; which: 0 = wall, 1 = free. Returns count via *n. */
int pfslam_get_cells(pfslam_handle *h, int which, int32_t *out, int cap, int *n);

/* ---- state upload ---- */
/* pfslam_set_map: a tree as KDTree::Create / InsertNode leave it.  Refused (non-zero, pfslam_last_error names the node, the loaded map
 * stays): a link or axis out of range, n above kd_capacity, and a weight that is NaN or infinite -- kernUpdateWeights converts the smallest
 * fit to int (kernel.cu:297-304), which has no defined result for such a sum, and thrust::minmax_element never selects a NaN.  Every finite
 * weight is accepted and scored; pfslam_measurement_update and the frames behind it are defined only while the smallest fit fits an int,
 * i.e. while n_beams x the largest |weight| < 2^31 -- beyond that the reference's conversion has no defined result either.  Integer weights with n_beams x the largest |weight| <= 2^24 (every map the SLAM step builds: +-113) are summed in
 * beam chunks, exact in any order; any other map is summed beam by beam in the reference's order, in one chunk per particle -- the same
 * bits as kernEvaluateParticlesKD either way, the second slower.  Coordinates may be anything: a node that is off the lattice of the
 * configured resolution, beyond 2^20 cells from the origin, NaN or infinite only turns the lattice-cell rows off for the whole map (the
 * distance to a NaN node is NaN and never the smallest, as in the reference).  KDTree::Create and Balance (pfslam_kd_create, the
 * re-balance of frame % balance_period == 5) sort the coordinates and are not defined on NaN.
 * pfslam_set_particles: n = cfg.n_particles poses and weights, any float.  A NaN, infinite or huge pose scores what the reference's
 * traversal gives it (a NaN or infinite query ends at the root) and costs the other particles nothing but the organisation of the pass:
 * its wave takes the plain traversal, and a non-finite mean of the first 1024 particles leaves the window of the cell rows where it is.
 * The 2-D map update converts the pose to int (kernel.cu:551-577): pfslam_step_grid is defined for finite poses only. */
int pfslam_set_map(pfslam_handle *h, const pfslam_node *nodes, int n);
int pfslam_set_particles(pfslam_handle *h, const pfslam_particle *p, int n);
int pfslam_set_scan(pfslam_handle *h, const float *scan_host, int n_beams);
int pfslam_set_pose(pfslam_handle *h, const float pose[3]);
int pfslam_set_grid(pfslam_handle *h, const int8_t *grid, int dimx, int dimy);

/* ---- stage entry points (operate on the handle's device-resident state) ---- */
int pfslam_motion_update(pfslam_handle *h, int frame);
/* odometry hook (no reference counterpart: the reference's filter has no motion model besides the diffusion of kernel.cu:375-397):
 * every pose the filter holds -- all particles and robotPos -- moves by delta = (dx, dy, dtheta), one float addition per
 * component.  Enqueued behind the frames in flight, no host wait.  Sharded handles: call it on every rank. */
int pfslam_shift_particles(pfslam_handle *h, const float delta[3]);
/* fit_host may be NULL (result stays on the device; no synchronisation) */
int pfslam_score_kd(pfslam_handle *h, float *fit_host);
/* min/max/first-argmax of fit + weight update; outputs may be NULL */
int pfslam_measurement_update(pfslam_handle *h, int *best, float *fmin, float *fmax);
/* ICP around the handle's current pose (the PREVIOUS robotPos, kernel.cu:1013) from `start`; dbg29 optional:
 * A[9], mu_tar[3], mu_cor[3], R[9], t[3], theta, n_valid */
int pfslam_icp(pfslam_handle *h, const float start[3], float pose_out[3], float *dbg29);
int pfslam_update_map_kd(pfslam_handle *h);
int pfslam_resample(pfslam_handle *h, int frame, int *resampled, float *neff);
/* the two halves of pfslam_resample for callers that drive the STAGES of a sharded handle themselves (the sharded frame
 * pfslam_shard_* needs neither): plan = Neff + cdf + source indices on the GLOBAL weights (device buffer 10, filled by the
 * caller's all-gather); gather = pull the chosen particles out of the GLOBAL pose blocks (device buffer 17, all-gathered by the
 * caller from buffer 16 when plan reports resampled = 1) */
int pfslam_resample_plan(pfslam_handle *h, int frame, int *resampled, float *neff);
int pfslam_resample_gather(pfslam_handle *h);
int pfslam_score_grid(pfslam_handle *h, int32_t *fit_host);
int pfslam_update_map_grid(pfslam_handle *h);

/* batch KD "nearest neighbour" with the reference traversal (findCorrespondenceIndexKD, kernel.cu:924-972);
 * xyz_host: n*3 floats; best_host: n ints */
int pfslam_traverse(pfslam_handle *h, const float *xyz_host, int n, int32_t *best_host);

/* ---- topology graph / loop-closure proposal (UpdateTopology, FindWalls, CheckLoopClosure: kernel.cu:623-795).
 * The reference leaves both calls commented out of its step (kernel.cu:1750-1751) and discards the clusters it builds
 * (kernel.cu:776), so they are explicit entry points, and part of the frame loops only after pfslam_set_topology(h, 1).
 * They act on the current robot pose
 * and on the 2-D occupancy grid (pfslam_set_grid / pfslam_update_map_grid).
 * topology_update: adds a graph node when the pose is > 2.5 m from every node; *n_nodes receives the node count.
 * find_walls: cells with occupancy > 30 on the Bresenham ray between two world points (exact count; the reference's
 *   CheckVisibility accumulates non-atomically).
 * check_loop_closure: pairs (candidate node j, visible node k) for every node j closer than 6 m on the map and
 *   farther than 20 m along the graph; returns the pair count in *n (pairs beyond cap are counted, not written).
 * get_topology: nodes as (x, y, dist) triples; *node_idx = index of the current node. */
/* pfslam_set_topology(h, 2): the same calls, made when the frame is BOOKED (`lag` steps after it was enqueued, see pfslam_step)
 *   instead of at once: KD frames stay in flight (their visibility test reads the 2-D grid, which KD frames never write; the counts
 *   run on a stream of their own), 2-D frames are still booked at once.  The graph and every frame's proposals are unchanged;
 *   pfslam_get_closures returns those of the last booked frame (any getter books everything first).
 * pfslam_set_topology(h, 1): pfslam_step and pfslam_step_grid then run UpdateTopology and CheckLoopClosure at the end of every
 *   frame, exactly where the reference has the two calls commented out (kernel.cu:1750-1751); pfslam_get_closures returns the
 *   pairs the LAST frame proposed (count in *n; pairs beyond cap are counted, not written).  In the KD frame loop FindWalls
 *   reads the 2-D grid the KD path never updates (dev_occupancyGrid, kernel.cu:680: all -100, every node visible); in the 2-D
 *   frame loop it reads the live map. */
int pfslam_set_topology(pfslam_handle *h, int enable);
int pfslam_get_closures(pfslam_handle *h, int32_t *pairs, int cap, int *n);
int pfslam_topology_update(pfslam_handle *h, int *n_nodes);
int pfslam_find_walls(pfslam_handle *h, const float a_xy[2], const float b_xy[2], int *n_walls);
int pfslam_check_loop_closure(pfslam_handle *h, int32_t *pairs, int cap, int *n);
int pfslam_get_topology(pfslam_handle *h, float *nodes_xyd, int cap, int *n, int *node_idx);

/* the frame % balance_period == 5 re-balance that pfslam_step performs first (kernel.cu:1707-1711), as its own
 * entry for callers that drive the stages themselves; pfslam_kd_size = number of map nodes (kdSize) */
int pfslam_maybe_balance(pfslam_handle *h, int frame);
int pfslam_kd_size(pfslam_handle *h);

/* ---- multi-GPU (particles sharded over ranks; the collectives are the caller's, e.g. RCCL over xGMI) ----
 * The sharded frame.  Like pfslam_step it is only ENQUEUED: no call waits for the device, the frame is booked one step later
 * from its pinned header, and the schedule of the caller's collectives is FIXED -- three all-gathers in every frame, none of
 * them data-dependent (the resample is decided on the device, on the gathered weights, and reads its sources from the gathered
 * pose blocks).  The four calls are the four parts of the very frame pfslam_step enqueues, and every collective goes straight into
 * one of that frame's streams -- pfslam_shard_stream names it; stream order is all the ordering the caller has to provide (no event,
 * no stream of the caller's own: launch the collective with that stream as its stream argument):
 *   pfslam_shard_disperse   scan upload, re-balance if due; dispersion and lane order of this shard; the cells' passes; the ICP solve.
 *                           *seeded = 1 when the frame only seeded the map (first scan): nothing else to do for this frame.
 *   [all-gather buffer 16 -> buffer 17, stream 0]   pose blocks [x | y | theta] in ONE piece of 3 * shard_stride floats per rank.  They
 *                           are final right after the dispersion; the stream has nothing else to do until the reduce, so the
 *                           collective runs UNDER the scan-match kernel
 *   pfslam_shard_score      scan-match, reduce -> this rank's 16-byte record in buffer 14: its packed {int64 max key, int64 negated-min
 *                           key}; key = (orderable_u32(fit) << 32) | (0xFFFFFFFF - global_index)
 *   [all-gather buffer 14 -> buffer 15, stream 1]   16 bytes per rank: the one collective on the frame's critical chain
 *   pfslam_shard_weights    global min / max / first argmax from the gathered keys; the best particle's pose is read out of the gathered
 *                           pose blocks; pose = best particle + increment of the ICP solve; walls at that pose, insert, cell rows;
 *                           weight update of this shard
 *   [all-gather buffer 5 -> buffer 10, stream 0]    weights, shard_stride floats per rank
 *   pfslam_shard_finish     sums + Neff on the gathered weights, frame header, gated resample (sources from buffer 17); the free
 *                           cells' chain of the replicated map update; booking of the frame `lag` steps back
 * The library orders every reader of buffers 10 / 15 / 17 behind the collective that fills it (the stream it rides, or an edge from it:
 * the chain and free-cell streams wait for the pose blocks through k_theta_gmax on stream 0), and every collective of the next frame
 * behind this frame's last readers of its buffer; the edge list is in csrc/pfslam_frame.hip.inc.
 * Results are bit-identical for any number of ranks.  Buffers 14 and 16 alternate between two allocations from frame to frame: query
 * 16 after pfslam_shard_disperse, 14 after pfslam_shard_score of the same frame.
 * A handle that holds ALL particles (global_n == n_particles) may be driven through the same calls (world 1): buffers 10 / 17
 * then alias 5 / 16, nothing reads buffer 15, and there is no collective to issue. */
int pfslam_shard_disperse(pfslam_handle *h, int frame, const float *scan_host, int *seeded);
int pfslam_shard_score(pfslam_handle *h);
int pfslam_shard_weights(pfslam_handle *h);
int pfslam_shard_finish(pfslam_handle *h);
/* the stream collective `which` (0 pose blocks, 1 keys, 2 weights) of the frame being enqueued is to be issued on: a hipStream_t */
int pfslam_shard_stream(pfslam_handle *h, int which, void **hip_stream);
/* Multi-GPU re-balance, ONE host build per node (the ranks hold identical maps): after pfslam_set_shard_balance(h, 1) the sharded
 * frame does not re-balance by itself.  In front of pfslam_shard_disperse every rank calls pfslam_shard_balance_due (books the frames
 * in flight when the period hits; *n_nodes = map size).  If due: the root rank calls pfslam_shard_balance_build (KDTree::Balance,
 * kdtree.cpp:31-40, on the host with all usable cores), every rank broadcasts pfslam_device_ptr buffers 20 (hot records, 16 B per
 * node), 21 (parents), 22 (z / z-level links), 23 (weights; 4 B per node each: the first n_nodes entries) and 24 (16 bytes of
 * state) from the root on the handle's stream, and the other ranks call pfslam_shard_balance_adopt. */
int pfslam_set_shard_balance(pfslam_handle *h, int external);
int pfslam_shard_balance_due(pfslam_handle *h, int frame, int *due, int *n_nodes);
int pfslam_shard_balance_build(pfslam_handle *h, int frame);
int pfslam_shard_balance_adopt(pfslam_handle *h);
/* stage-level merge hooks (the sharded frame above does not need them): local packed keys into the stats buffer 0
 * ([0] max key, [1] negated-min key: MAX-reduce across ranks), then weights + this rank's share of the best pose in buffer 8
 * (zero on non-owners: SUM-reduce across ranks) */
int pfslam_measurement_local(pfslam_handle *h);  /* score must have run; fills the stats buffer */
int pfslam_measurement_apply(pfslam_handle *h, int *best_global, float *fmin, float *fmax); /* after the MAX merge */
/* device pointers of the handle's buffers, for zero-copy wrapping by the harness.
 * which: 0 stats (8 x i64), 1 fit (n x f32), 2 x, 3 y, 4 theta (n x f32 each; inside buffer 16), 5 w (shard_stride x f32, the
 *        first n valid), 6 weight tile sums, 7 scan (n_beams x f32), 8 best-particle pose (4 x f32), 9 robot pose (4 x f32),
 *        10 global w (world * shard_stride x f32, rank-major, the first global_n valid; aliases 5 when unsharded),
 *        11 ICP targets, 12 ICP correspondences (n_beams x float4 each): what the last ICP left behind -- kernGetWallsKD's target cloud at
 *        the previous pose (rejected beams: zero, H2) and findCorrespondenceKD's matched node (x, y, z, w) of every target, as pfslam_icp
 *        writes them; a frame of pfslam_step leaves the same arrays with w = 0 in the correspondences (test support:
 *        tests/test_gpu_devlib_frames.py compares them with the reference's kernels),
 *        14 this rank's 16-byte measurement record (its packed max / negated-min keys), 15 the gathered records (world x 16 B),
 *        16 local pose block [x | y | theta] (3 * shard_stride x f32; moves when a resample swaps the double buffer),
 *        17 global pose blocks (world x 3 * shard_stride x f32, rank-major; aliases 16 when unsharded) */
int pfslam_device_ptr(pfslam_handle *h, int which, void **ptr, size_t *bytes);

/* ---- measurement support ----
 * pfslam_time_score_kd: `iters` back-to-back scoring passes (lane order + scan-match kernel + partial-sum reduce, i.e. all of
 *   pfslam_score_kd's device work) between two HIP events on the handle's stream; average milliseconds per pass.
 * pfslam_set_timing: 0 = off; 1 = HIP events on the handle's stream bracket every launch of the scan-match kernel (only that
 *   kernel) inside pfslam_step / pfslam_shard_score; 2 = additionally the four phases the reference times per frame
 *   (kernel.cu:1727-1760: motion, measurement incl. ICP, map update incl. its host part, resample).  Resets the accumulators.
 *   Mode 2 is for pfslam_step only -- its frames leave the round-5 frame for the staged chain, with the same results -- and
 *   pfslam_shard_disperse refuses a handle in that mode.
 * pfslam_get_timers -> out[2k] = total ms, out[2k+1] = count, k = 0 scan-match kernel, 1 motion, 2 measurement, 3 map,
 *   4 resample, 5 the planning launches that precede the scan-match kernel (pose boxes + shared-prefix plan).
 * pfslam_score_census: what one scoring launch on the handle's CURRENT particles, scan and map issues, counted by a counting
 *   instantiation of the same kernel with the same launch shape and lane order: out[0] wave-level trips of the descent loop
 *   (= wave-level 16-byte gathers of node records), out[1] active lanes in them (= node visits), out[2] wave-level
 *   parent-hyperplane tests (one 4-byte + one 16-byte wave gather each), out[3] lanes in them, out[4] trips in which every
 *   active lane stood on the same node, out[5] those of them on the common path of all 64 lanes from the root.
 * pfslam_set_variant: how the scoring pass is organised (results are bit-identical; A/B measurements and tests): 0 = default
 *   (lanes along a Hilbert curve: counting sort over cells of the cloud; from ~4.6 k particles on a planar map: lattice-cell rows
 *   when every map point lies on the lattice k * resolution -- true of every map the SLAM step builds --, the round-2
 *   shared-prefix plan otherwise), 1 = identity lane order, 2 = the plain per-lane traversal, 3 = cell rows / plan at any
 *   particle count, 4 = like 3 but always the shared-prefix plan.  The environment variable PFSLAM_VARIANT sets the initial value. */
int pfslam_time_score_kd(pfslam_handle *h, int iters, float *ms_per_launch);
int pfslam_set_timing(pfslam_handle *h, int enable);
int pfslam_get_timers(pfslam_handle *h, double out[12]);
int pfslam_score_census(pfslam_handle *h, unsigned long long out[8]);
/* census log: while enabled, every scoring pass of pfslam_step / pfslam_shard_score / pfslam_score_kd is followed by the counting
 * instantiation of the scan-match kernel on the very SAME inputs (particles, scan, map, lane order, plan) -- one record of eight
 * counters (the layout of pfslam_score_census) per pass, up to 1024 passes.  bench.py replays its timed frames on a second
 * handle with the log on: the frame loop is deterministic, so the replay's launches are the timed launches.
 * pfslam_get_census_log: *n = passes logged, out[k * 8 + c] for k < min(*n, cap). */
int pfslam_set_census(pfslam_handle *h, int enable);
int pfslam_get_census_log(pfslam_handle *h, unsigned long long *out, int cap, int *n);
/* the chip's wave-level 16-byte gather rate measured live by a micro-benchmark (cache-resident 2 MB table, 8 waves per SIMD):
 * out[0] = wave gathers per second (whole chip), out[1] = compute units, out[2] = nominal clock in GHz, out[3] = cycles per
 * wave gather per CU at the nominal clock.  The scan-match kernel issues one such gather per node visit of a wave. */
int pfslam_ubench_gather(pfslam_handle *h, double out[4]);
/* the shared-prefix plan of the LAST scoring pass (kd_device.h): out[0] rows (waves x beams), [1] mean length of the root path
 * common to a wave's 64 queries, [2] mean candidates kept of it, [3] fraction of rows whose first descent is complete,
 * [4] fraction without a plan, [5] fraction with a full candidate list, [6..8] mean extent of a wave's pose box in x, y (m) and
 * heading (rad), [9] waves.  All zero when no plan was made (non-planar map, few particles, variant 2). */
int pfslam_plan_stats(pfslam_handle *h, double out[10]);
/* the persistent lattice-cell rows (csrc/kd_cells.hip.inc): out[0] lattice cells claimed since the last wipe, [1] live rows (one per
 * sub-cell: up to four per cell), [2] mean first-descent candidates per row, [3] mean re-descent candidates per row, [4] sub-cells
 * without a row (too many candidates, the pool exhausted, or the four of a cell that a full list refused), [5] 16-byte pool slots used, [6] [7] index of the window's corner in sub-cells (two per lattice cell and axis), [8 .. 11] since the last wipe:
 * cells walked from the root / extensions (one of the cell's links had gained a node) / looks that found a cell unchanged / cells
 * claimed, [12] device flags (1 list full, 2 pool full, 8 cloud far from the window centre), [13] publishing updates since the
 * last wipe (divide [9] and [10] by it for per-frame figures), [14] wipes so far, [15] 1 = suspended: the list / pool overflowed
 * in two frames whose frame numbers -- the `frame` arguments of pfslam_step / pfslam_shard_disperse, not a count of calls -- differ,
 * the second one's at most 16 above the first one's (a lower number counts as well; numbers more than 16 apart never suspend): a
 * cloud too wide for the table, the round-2 plan scores until the map is replaced or re-balanced.
 * [0 .. 13] are zero when the last scoring pass did not use cell rows. */
int pfslam_cell_stats(pfslam_handle *h, double out[16]);
/* mean duration (ms) of the 2-D scan-match kernel alone and of the whole 2-D scoring pass (kernel + partial sums + min / max / argmax +
 * weights) over `iters` launches each, HIP events on the handle's stream.  The weights (and their host mirror) are put back behind the
 * last pass: like pfslam_time_score_kd the call leaves particles, pose and maps as it found them. */
int pfslam_time_score_grid(pfslam_handle *h, int iters, float *ms_kernel, float *ms_pass);
int pfslam_set_variant(pfslam_handle *h, int variant);
/* Transcendentals.  0 (default) = the specification of csrc/pf_math.h: fixed sequences of IEEE double operations rounded once, which the
 * CPU oracle follows bit for bit.  1 = the device library's cosf / sinf in CleanLidarScan (kernel.cu:182-187) and erfcinvf in the
 * dispersion (kernel.cu:375-397) -- what the reference's own text compiles to on this platform: with it the product's kernels equal the
 * reference's kernels built for gfx950 with zero mismatches (tests/test_gpu_ref_kernels.py: the stage entry points;
 * tests/test_gpu_devlib_frames.py: whole frames of pfslam_step / pfslam_step_grid / pfslam_shard_* against a frame composed of those
 * stage calls, and the frame's own scan-match and ICP launches against the reference's kernels); results then differ from the oracle's in
 * the last place of an end point now and then. */
int pfslam_set_trig(pfslam_handle *h, int devlib);
/* Resampler: where thread i of a resample takes its rnd from.  Everything else of PFResample is the same in every mode, bit for bit: Neff
 * from the canonical sums, the gate Neff < 0.7 N decided on the device, the inclusive scan, "first idx with rnd <= cdf[idx]" (exact for a
 * non-monotone cdf too, H8), the gather from a snapshot (H3), w = 1 afterwards, the H11 mirror.  With i the GLOBAL particle index, gn the
 * global particle count and maxv = cdf[gn - 1]:
 *   0 (default) = the reference's scheme (kernel.cu:429-444), collisions included (H5):
 *       rnd_i = uniform_real(engine_seed((int)Neff, frame, i), 0, maxv)
 *     engine_seed(iter, index, depth) hashes the key (1 << 31) | (depth << 22) | iter, so i contributes its low 9 bits only: every resample
 *     draws 512 distinct numbers whatever gn is, and a resampled cloud holds at most 512 distinct poses.
 *   1 = one multinomial draw per particle, from the same seeding function with the particle index in the argument that is hashed whole:
 *       rnd_i = uniform_real(engine_seed((int)Neff, i, frame), 0, maxv)
 *     utilhash is a bijection on 32 bits, so seeds collide only through the final % (2^31 - 1) (999 870 distinct seeds among 1 000 000
 *     particles).  The frame number now lands in the 9-bit field: two frames 512 apart that also share (int)Neff draw alike.
 *   2 = systematic (low-variance) resampling, one draw per frame:
 *       u     = uniform_real(engine_seed((int)Neff, frame, 0), 0.0f, 1.0f)
 *       rnd_i = (float)((((double)i + (double)u) * (double)maxv) / (double)gn)
 *     in exactly this order, in double, rounded to float once.  For positive weights the sources are non-decreasing in i and every particle
 *     is copied floor or ceil of its expectation gn * w / sum(w) times.
 * Above 512 particles a caller who does not need parity with the reference should choose 2.
 * Like every entry point but the step functions the call first books the frames in flight; the mode holds from the next stage call or
 * enqueued frame.  A mode outside 0..2 returns non-zero (pfslam_last_error) and leaves the handle's mode as it was.  On a sharded job EVERY
 * rank must set the same mode (the caller's duty: nothing checks it); the draw depends on global quantities only, so results then stay
 * bit-identical for any number of ranks. */
int pfslam_set_resampler(pfslam_handle *h, int mode);
/* Posterior estimate (no reference counterpart): weighted mean pose, 3x3 covariance and Neff of the whole cloud, reduced on the device.
 * Reads state, writes none.  With gn the global particle count, (x_i, y_i, theta_i, w_i) the particle with GLOBAL index i, p_k one of
 * x, y, theta, and csum the canonical sum (64 lanes, lane l adds elements l, l + 64, ... in ascending order, then an xor butterfly 32 .. 1;
 * above 4096 elements the 4096-element tiles are summed that way, then the tile sums the same way), all in float, one rounding per
 * operation, in the order written (no contraction; divisions correctly rounded):
 *     S0    = csum(w_i)                          S2 = csum(w_i * w_i)
 *     m_k   = csum(w_i * p_k,i) / S0             k = x, y, theta
 *     d_k,i = p_k,i - m_k
 *     C_kl  = csum((w_i * d_k,i) * d_l,i) / S0   (k, l) = xx, xy, xtheta, yy, ytheta, thetatheta
 *     Neff  = (S0 * S0) / S2
 *   out[0..2] = m, out[3..8] = C in the order above, out[9] = Neff, out[10] = S0, out[11] = S2, out[12] = (float)gn, out[13..15] = 0.
 * Two passes -- the means, then the centred moments: sum(w x^2) - m^2 would cancel (x is tens of metres, the cloud's sigma centimetres).
 * Scaling every weight by a power of two leaves m, C and Neff bit-identical.
 * Heading: the mean is LINEAR on purpose.  Nothing in the filter wraps theta -- dispersion, ICP and pfslam_shift_particles only add -- so a
 * cloud's headings are a contiguous set of reals and their linear mean and spread are the cloud's.  A caller who uploads headings wrapped
 * into (-pi, pi] through pfslam_set_particles, with a cloud that straddles the cut, gets a meaningless theta row and column.
 * Refused (non-zero, pfslam_last_error names the cause, out untouched): S0 not finite or not > 0; gn above 4096 * 4096.
 * Like every entry point but the step functions the call first books the frames in flight, then runs on the handle's stream: it describes
 * exactly the arrays pfslam_get_particles would return at that moment -- after a frame that resampled, the resampled cloud with w = 1.
 * Sharded handles (global_n > n_particles) read the caller's gathered buffers, like pfslam_resample_plan: buffer 10, the global weights, and
 * buffer 17, the global pose blocks -- the caller must have all-gathered both from buffers 5 and 16 after the last frame.  The sums run in
 * global index order (tile edges at multiples of 4096 of the GLOBAL index), so every rank's result is bit-identical for any number of ranks
 * and equals the unsharded handle's.  Unsharded handles read their own arrays (10 and 17 alias 5 and 16). */
int pfslam_estimate(pfslam_handle *h, float out[16]);
/* ---- scan-to-map registration (no reference counterpart) ----
 * pfslam_icp restates the reference's transformPointICP bit for bit: ONE step, with three properties that keep a caller from iterating it
 * into a scan matcher (measured with the CPU oracle on a 4000-point synthetic map, 1081 beams):
 *   1. its correspondences are not nearest neighbours: findCorrespondenceIndexKD (pfslam_traverse) returned the true nearest map point for
 *      78 of 697 and 82 of 810 in-range beams at the true pose; the median match was 0.37 m and 0.24 m away, the true nearest point 6 mm;
 *   2. rejected beams poison the fit: beams outside the +-20 m reject stay in as (0, 0, 0) targets and are matched (H2) -- iterating the
 *      step from 0.10 m / 0.03 rad off walks the pose 17 m away within 30 iterations;
 *   3. the pose update is wrong under rotation: it is start + (t.x, t.y, theta) while the fit rotates about the world origin; the robot
 *      position should become R r + t, the step drops the lever arm (R - I) r.
 * pfslam_nearest and pfslam_register work on the handle's device-resident map and scan.  Like every entry point but the step functions both
 * first book the frames in flight; both honour pfslam_set_trig.  Neither writes state that any other entry point reads -- not the pose, not
 * buffers 11 / 12, not the tree: their scratch is their own.  No option makes a frame call them.
 *
 * pfslam_nearest: the exact nearest map node of n query points (xyz_host: n * 3 floats; best_host: n ints; d2_host: n floats or NULL), the
 * counterpart of pfslam_traverse.  In float, one rounding per operation, in this order, no contraction:
 *     d2(q, node) = ((nx - qx) * (nx - qx) + (ny - qy) * (ny - qy)) + (nz - qz) * (nz - qz)
 * The result is the node with the smallest d2, the lowest node index among equal ones; a query with a non-finite coordinate gets index -1
 * (and d2 = +inf).  A node with a NaN coordinate has d2 = NaN and is never the result.  Exact for every tree the library can hold --
 * KDTree::Create / Balance, grown by InsertNode, non-planar --: a
 * branch-and-bound descent that backtracks through the parent links, no stack, no depth limit.
 *
 * pfslam_register: up to max_iters ICP iterations on the device, no host round trip in between (one launch, one copy, one wait).
 *   start     float[3], or NULL = the handle's pose, read on the device
 *   pose_out  float[3]
 *   info      float[8] = {status, iterations completed, pairs, mean squared residual, 0, 0, 0, 0}; pairs and residual are those of the last
 *             completed iteration (0 when there is none), except that status 2 reports the pair count that was too small
 *   trace     NULL or max_iters x 8 floats; row k = {x', y', theta', x' - x, y' - y, theta' - theta, pairs, e}, written for completed
 *             iterations only
 *   status    0 = max_iters done, 1 = converged (eps), 2 = too few pairs, 3 = the pose turned non-finite
 * Refused (non-zero, pfslam_last_error names the cause, outputs untouched): no map; n_beams > 4096; an option out of range (max_iters outside
 * 1 .. 64, match / select / update outside 0 .. 1, max_dist not finite, an eps negative or not finite).
 * Iteration k runs from p = (x, y, theta), p_0 = start.  All arithmetic is float, one rounding per operation, in the order written; csum is
 * the canonical sum of pfslam_estimate above (n_beams <= 4096: one tile); R, A and t are indexed as in pfslam_icp's dbg29:
 *   1. targets          (wx, wy) = CleanLidarScan(i, scan[i], theta)          in_i = |wx| < 20 && |wy| < 20
 *                       t_i = in_i ? (x + wx, y + wy, 0) : (0, 0, 0)
 *   2. correspondences  c_i = (x, y, z) of the node `match` selects for t_i; d2_i as in pfslam_nearest (a t_i that is not finite has no
 *                       nearest node under match 1: c_i and d2_i are NaN)
 *   3. validity         select 0: v_i = 1.   select 1: v_i = in_i && (max_dist <= 0 || d2_i <= max_dist * max_dist)
 *                       nv = sum v_i;  select 1 and nv < max(min_pairs, 1): status 2, the result is p, stop
 *   4. fit              mu = csum(v_i ? component : 0) / (float)nv for the six components
 *                       A[j * 3 + r] = csum(v_i ? (t_i[r] + (-mu_t[r])) * (c_i[j] + (-mu_c[j])) : 0)
 *                       svd3, R = U V^T, t = mu_c - R mu_t, theta = asin(R[1]) exactly as in pfslam_icp (select 0: that step bit for bit)
 *   5. residual         e = csum(v_i ? d2_i : 0) / (float)nv
 *   6. update           update 0: x' = x + t[0], y' = y + t[1]
 *                       update 1: x' = (R[0] * x + R[3] * y) + t[0], y' = (R[1] * x + R[4] * y) + t[1]
 *                       both: theta' = theta + theta_fit
 *   7. stopping         x', y' or theta' not finite: status 3, the result is p, stop (the iteration does not count)
 *                       otherwise p <- p', the trace row is written; status 1 and stop when |x' - x| < eps_xy && |y' - y| < eps_xy &&
 *                       |theta' - theta| < eps_theta (an eps of 0 never passes); status 0 after max_iters
 * With the defaults (exact neighbours, a 0.5 m gate, rejected beams left out, the rigid update) the six cases of
 * tests/test_register_spec.py end within one map cell and one beam step of the pose their scan was cast from. */
typedef struct pfslam_register_opts {
    int32_t max_iters;  /* 1 .. 64 */
    int32_t match;      /* 0 = the reference's traversal (pfslam_traverse), 1 = exact nearest neighbour (pfslam_nearest) */
    int32_t select;     /* 0 = every beam, rejected ones as zero targets (the reference, H2);
                           1 = in-range beams whose correspondence passes the gate */
    int32_t update;     /* 0 = the reference's increment, 1 = rigid */
    float   max_dist;   /* select 1: accepted when d2 <= max_dist * max_dist (float product); <= 0: no gate */
    float   eps_xy, eps_theta;  /* stop when |dx| < eps_xy && |dy| < eps_xy && |dtheta| < eps_theta; 0: never */
    int32_t min_pairs;  /* select 1: fewer accepted pairs ends the run; values below 1 count as 1 */
} pfslam_register_opts;
/* {40, 1, 1, 1, 0.5f, 1e-4f, 1e-5f, 3} */
void pfslam_register_default_opts(pfslam_register_opts *opts);
int pfslam_nearest(pfslam_handle *h, const float *xyz_host, int n, int32_t *best_host, float *d2_host);
int pfslam_register(pfslam_handle *h, const float start[3], const pfslam_register_opts *opts, float pose_out[3], float info[8], float *trace);
/* pfslam_register_batch: m independent registrations of the handle's scan against the handle's map from m start poses -- one launch, one
 * copy back, one wait; one workgroup per run, so up to a whole device's compute units work where pfslam_register uses one.
 *   starts     m x 3 floats (none may be left out: there is no "handle's pose" row)
 *   poses_out  m x 3 floats
 *   info       m x 8 floats, row r as pfslam_register's info
 *   best       NULL or one int
 * Rows.  Row r of poses_out and info is bit for bit what pfslam_register(h, starts + 3 r, opts, ...) returns: that call is the definition,
 * for a start that is not finite and for rows that end with status 2 or 3 as well.  Runs do not wait for one another: one that stops early
 * makes room for the next.  There is no per-iteration trace; pfslam_register from the same start is the same run and has one.
 * *best is decided from info alone, on the host:
 *   eligible    rows with status 0 or 1, at least one completed iteration and a finite residual
 *   P           the largest pair count among the eligible rows
 *   candidates  the eligible rows with 2 * pairs >= P
 *   best        the candidate with the smallest residual; among equal residuals the one with more pairs, then the lowest row;
 *               -1 when no row is eligible
 *   Why both: a run that keeps a handful of pairs can have any residual (42 beams that happen to lie on a wall fit it perfectly), so the
 *   residual alone is no measure; the pair count alone picks wrong too -- from a 3 x 3 x 3 grid of starts (+-0.4 m, +-0.15 rad) around
 *   (0.5, 0.3, 0.1) on the 4000-point map of tests/test_register_spec.py it chose a run with 802 pairs that ended 48 mm off over one with
 *   801 pairs that ended 0.5 mm off.  Many starts are needed at all because from (10, -8, 0.3) only 6 of the 27 runs of that grid end
 *   within one map cell and one beam step (tests/test_register_batch_spec.py).
 * Refused (non-zero, pfslam_last_error names the cause, outputs untouched): a NULL argument other than best; m outside 1 .. 4096; no map;
 * n_beams > 4096; every option pfslam_register refuses.
 *   The cap of 4096 bounds one launch.  Measured on one MI355X: 4096 rows of 40 iterations each, none stopping early, 1081 beams, take
 *   0.41 s on a 100 000-point map and 0.16 s on a 4000-point map (profiles/register_batch.txt; the estimate had been about a second).
 * Like pfslam_register it first books the frames in flight and then runs on the handle's stream, honours pfslam_set_trig, reads the handle's
 * device-resident map and scan and writes no state another entry point reads: its start and result buffers are its own (they belong to
 * the handle, grow when a call needs more and go with pfslam_destroy), the per-run scratch is on chip.  The map and the scan of a sharded
 * handle are replicated, so every rank gets the unsharded handle's bits. */
int pfslam_register_batch(pfslam_handle *h, const float *starts /* m x 3 */, int m, const pfslam_register_opts *opts,
                          float *poses_out /* m x 3 */, float *info /* m x 8 */, int *best /* may be NULL */);
/* pfslam_search: windowed correlative scan-to-map search (no reference counterpart).  Every pose of a window around `centre` is scored
 * against a distance field of the map -- one field lookup per beam instead of a tree search -- and the best one is returned: the wide-basin
 * start pfslam_register lacks (ICP is local, see pfslam_register_batch above), an answer to "where in this window does the scan fit best"
 * after a bad resample, and a check of the pairs pfslam_check_loop_closure proposes.
 *   centre    float[3], or NULL = the handle's pose (read back first, as pfslam_get_pose does: the one case with a second copy and wait)
 *   pose_out  float[3]: the winning candidate
 *   info      float[8] = {status, (float)k, in-range beams at the winner's heading, fdiv((float)S * u, (float)n_in), (float)S,
 *             (float)candidates, (float)qcap, 0}; status 0 = ok, 2 = no heading has an in-range beam: pose_out is the centre and
 *             info = {2, -1, 0, 0, 0, candidates, qcap, 0}
 *   scores    NULL or one int32 per candidate: S(k), INT32_MAX for the candidates of a heading without an in-range beam
 * All arithmetic is float, one rounding per operation, in the order written, no contraction, divisions (fdiv) correctly rounded.  It needs
 * map_res_x == map_res_y; res is that resolution, (cx, cy, ct) the centre, hx, hy, ht the three halves:
 *   unit, cap    u = (res * res) * 0.0625f           qcap = (int)rintf(fdiv(max_dist * max_dist, u)), refused unless 1 <= qcap <= 65535
 *   field        the cell with lattice index (kx, ky) has q = min((int)rintf(fdiv(d2, u)), qcap), d2 being pfslam_nearest's d2 of the query
 *                ((float)kx * res, (float)ky * res, 0); qcap where that query has no nearest node.  (A d2 too large for the conversion
 *                saturates.)  The call builds the bounding box of the end-point cells of all its headings, grown by hx * stride and
 *                hy * stride cells: every cell a candidate can touch, so there is no cell outside it to define.
 *   candidates   k = (a * (2 hy + 1) + j) * (2 hx + 1) + i, i, j, a counted from 0
 *                theta_a = ct + (float)(a - ht) * step_theta
 *                x_i = cx + (float)((i - hx) * stride) * res         y_j = cy + (float)((j - hy) * stride) * res
 *   end points   for heading a and beam b: (wx, wy) = CleanLidarScan(b, scan[b], theta_a), in = |wx| < 20 && |wy| < 20,
 *                ex = (int)rintf(fdiv(cx + wx, res)), ey = (int)rintf(fdiv(cy + wy, res)); an in-range beam whose ex or ey is not finite or
 *                exceeds +-2^20 counts as qcap for every candidate.  End points depend on the heading only: a translation of the window is
 *                a pure index shift of `stride` cells, which is the point of the design.
 *   score        S(k) = sum over the in-range beams of q[ex + (i - hx) * stride, ey + (j - hy) * stride]; integers, S <= 4096 * 65535 < 2^31:
 *                exact in any order
 *   result       the candidate with the smallest S, the lowest k among equal ones; a heading with no in-range beam takes no part
 * Refused (non-zero, pfslam_last_error names the cause, outputs untouched): a NULL argument other than centre or scores; a half < 0, stride
 * outside 1 .. 64, step_theta not finite or (half_theta > 0) not > 0, max_dist not finite or not > 0, reserved_ non-zero; qcap outside
 * 1 .. 65535; a centre that is not finite; no map; n_beams > 4096; map_res_x != map_res_y; more than 2^24 candidates; more than 2^24 end
 * points ((2 half_theta + 1) * n_beams); a field above 2^26 cells, bounded BEFORE the launch by
 *     (rint((cx + 20) / res) - rint((cx - 20) / res) + 1 + 2 hx stride) * (the same in y)   (each rint held inside +-2^20):
 * 1641 x 1641 cells for the defaults at res = 0.025.  The box a call really builds is that of its scan's end points and much smaller.
 *   The cap of 2^24 candidates bounds one call.  Measured on one MI355X, 1081 beams, the benchmark's 100 000-point map (profiles/search.txt):
 *   scoring takes 0.38 ms per 10^6 candidates at stride 1 and 0.36 ms at stride 2 once the window fills the device (5.5e5 candidates; the
 *   891 waves of a default window do not: its scoring kernel takes 0.10 ms); the field kernel alone, from a kernel trace, 0.92 ms for
 *   the 0.082 M cells of a default call there -- the launch is as long as its slowest tree searches -- and 1.6 ms for the 1.8 M cells of
 *   the same call on a 4000-point map (0.88 ms per 10^6 cells); a whole default call of 55 473 candidates 1.06 ms; a call of 16 776 177
 *   candidates, just under the cap, 9.0 ms.  In the 0.41 s of a full pfslam_register_batch launch (4096 rows x 40 iterations, same
 *   map) 45 calls at the cap score 7.6e8 candidates.
 *   Kernel resources (VGPRs / LDS bytes per workgroup / waves per SIMD): end points 94 / 80 / 5, field 18 / 0 / 8, scoring 25 / 0 / 8.
 * What the search is for, measured with the restatement (tests/test_search_spec.py, profiles/search.txt): in pfslam_register_batch's scenario
 * -- the scan cast from (10, -8, 0.3), where pfslam_register alone ends at the pose from 6 of the 27 starts of a +-0.4 m, +-0.15 rad grid --
 * a window of +-0.5 m at stride 2 and +-0.2 rad at 0.0125 rad around each of the 26 off-centre starts puts the winner within one step of
 * the pose, and pfslam_register from the winner ends within one map cell and one beam step, from 26 of 26.  Those starts lie on the
 * window's own lattice, so the pose itself is a candidate; with every centre moved a third of a step off it in each coordinate the count
 * is 26 of 26 again (winner 0.017 m and 0.004 rad off, 7 mm after the registration).  max_dist 0.1, 0.2 and 0.5 give the same winners: next
 * to the pose no beam is near saturation, so this scenario does not tell them apart.
 * Like pfslam_register it first books the frames in flight and then runs on the handle's stream, honours pfslam_set_trig, reads the handle's
 * device-resident map and scan and writes no state another entry point reads: the field, the end points, the score volume and the result
 * are its own buffers (they belong to the handle, grow when a call needs more and go with pfslam_destroy).  One result copy and one wait
 * per call; the score volume is copied only when `scores` is not NULL.  The map and the scan of a sharded handle are replicated, so every
 * rank gets the unsharded handle's bits. */
typedef struct pfslam_search_opts {
    int32_t half_x, half_y, half_theta; /* window: (2 hx + 1)(2 hy + 1)(2 ht + 1) candidates, each half >= 0 */
    int32_t stride;                     /* translation step in map cells, 1 .. 64 */
    float   step_theta;                 /* heading step (rad), finite, > 0 unless half_theta == 0 */
    float   max_dist;                   /* saturation distance (m), finite, > 0 */
    int32_t reserved_[2];               /* must be 0 */
} pfslam_search_opts;
/* {20, 20, 16, 1, 0.0125f, 0.2f, {0, 0}} */
void pfslam_search_default_opts(pfslam_search_opts *opts);
int pfslam_search(pfslam_handle *h, const float centre[3] /* NULL = the handle's pose */, const pfslam_search_opts *opts, float pose_out[3],
                  float info[8], int32_t *scores /* NULL or one int per candidate */);
/* pfslam_search_scan: correlative scan-to-scan search (no reference counterpart) -- "how did the robot move between these two scans".
 * pfslam_search's window, scored against a distance field built from the END POINTS OF A REFERENCE SCAN instead of the map's nodes: the
 * lidar-only source of the `delta` pfslam_shift_particles takes, a match before and beside the map (the handle needs NO map), and the check
 * of a pair pfslam_check_loop_closure proposes, its two scans against each other.
 *   ref_scan_host  n_beams ranges: the scan the field is built from
 *   ref_pose       float[3], the pose ref_scan was taken at; NULL = (0, 0, 0)
 *   scan_host      n_beams ranges: the scan that is searched; NULL = the handle's scan (pfslam_set_scan, the last frame's)
 *   centre         float[3], the middle of the window; NULL = ref_pose
 * With ref_pose = NULL, pose_out is the searched scan's pose in the reference scan's frame: the relative motion.  With ref_pose = the world
 * pose of the previous frame, pose_out - ref_pose is the delta of pfslam_shift_particles.
 * The candidates k, theta_a, x_i, y_j, the end points of the searched scan, the unit u and qcap, S(k) and the tie rule, pose_out,
 * info[0..6], status 2 and the `scores` volume are pfslam_search's, word for word.  Only the field's source changes:
 *   points       for beam b of ref_scan: (wx, wy) = CleanLidarScan(b, ref_scan[b], ref_theta), in range iff |wx| < 20 && |wy| < 20, then
 *                P_b = (rx + wx, ry + wy): step 1 of pfslam_register at ref_pose (it honours pfslam_set_trig).  A beam out of range gives
 *                no point.  info[7] = (float) number of points.
 *   field        the cell (kx, ky) has q = min((int)rintf(fdiv(d2, u)), qcap), d2 = the minimum over all points of dx * dx + dy * dy with
 *                dx = px - (float)kx * res, dy = py - (float)ky * res (pfslam_nearest's d2 with both z at 0; float, one rounding per
 *                operation, in that order, no contraction).  A d2 too large for the conversion, infinite, or with no point at all gives
 *                qcap.  With no point the call still succeeds: every cell is qcap, info[7] = 0, the winner follows the ordinary rule.
 * Nothing of the handle's map, pose or particles is read.
 * Refused (non-zero, pfslam_last_error names the cause under this function's name, outputs untouched), in this order: a NULL handle, opts,
 * pose_out or info; a NULL ref_scan_host; a half < 0, stride outside 1 .. 64, step_theta, max_dist, reserved_ as pfslam_search; a ref_pose
 * that is not finite; a centre that is not finite; more than 2^24 candidates; n_beams > 4096; map_res_x != map_res_y; qcap outside
 * 1 .. 65535; more than 2^24 end points; a field above 2^26 cells (pfslam_search's bound, around the centre).
 * Method.  k_search_ends, k_search_score and k_search_result are pfslam_search's kernels, unchanged; the field is left in the layout they
 * read.  One thread per reference beam makes the points and counts them.  The field builder -- a function of a point list -- fills the box
 * with qcap and then splats: a wave per point lowers the (2R + 1)^2 cells around the point's own cell, clipped to the box, to the point's q,
 * R = ceil(max_dist / res) + 2 (a cell farther out saturates: the argument is next to the kernel); an integer minimum is exact in any
 * order.  Sixteen-bit cells have no atomic minimum: a lane owns an aligned 32-bit word, two adjacent cells, and lowers both halves with one
 * compare-and-swap, after a plain load that usually shows there is nothing to lower.  Its cost grows with the points and R, not with the
 * box.  Measured: profiles/search_scan.txt.
 * Like pfslam_search it first books the frames in flight and then runs on the handle's stream.  It writes no state another entry point
 * reads: not the handle's scan (an uploaded scan_host goes to a buffer of its own), not the pose, not pfslam_search's results.  The field,
 * the end points, the counts and the volume are pfslam_search's buffers (every call of either rebuilds them); the two scans, the points
 * and the result row are its own; all belong to the handle, grow when a call needs more and go with pfslam_destroy.  One result copy and
 * one wait per call.  Nothing is sharded, so every rank of a sharded handle gets the unsharded bits. */
int pfslam_search_scan(pfslam_handle *h, const float *ref_scan_host, const float ref_pose[3] /* NULL = (0, 0, 0) */,
                       const float *scan_host /* NULL = the handle's scan */, const float centre[3] /* NULL = ref_pose */,
                       const pfslam_search_opts *opts, float pose_out[3], float info[8], int32_t *scores /* NULL or one int per candidate */);
/* pfslam_search_cov / pfslam_search_scan_cov: pfslam_search / pfslam_search_scan, and how well the winner is determined (no reference
 * counterpart).  A winner alone says nothing about its uncertainty: in a corridor it is arbitrary along the corridor.  The score volume is
 * up to 2^24 poses that lack only weights; these calls give it weights and run pfslam_estimate's reduction over it: the information a
 * pose-graph constraint needs, the trust a filter puts into the match, the spread of the `delta` pfslam_shift_particles takes.
 * Definition by reference.  pose_out, info and scores are bit for bit what pfslam_search / pfslam_search_scan return for the same
 * arguments, status 2 and info[7] (the point count of the scan form) included; the candidates k, theta_a, x_i, y_j and S(k) are theirs,
 * word for word.  Only cov_out is new.  All arithmetic is float, one rounding per operation, in the order written, no contraction,
 * divisions (fdiv) correctly rounded, except where stated.
 *   scale     hs = fdiv(u * 1.442695f, (2.0f * sigma) * sigma)     (the constant has the float bits 0x3fb8aa3b; u is the search's unit)
 *             The model: independent Gaussian beam errors, likelihood proportional to exp(-S u / (2 sigma^2)).
 *   weights   Smin = the winner's S.  A candidate of a heading that takes no part has w_k = 0; every other one
 *             t_k = (float)(S_k - Smin) * hs     (the difference is an exact int32; the conversion rounds to nearest even above 2^24)
 *             w_k = exp2m(t_k)
 *   exp2m(t), t >= 0:  0.0f if !(t < 64.0f); else n = (int)t, f = (double)t - (double)n (exact, in [0, 1)), in double p = C16, then for
 *             k = 15 down to 0  p = p * f + C_k  (a multiply, then an add: two roundings, never an fma), w = (float)(p * 2^-n) (the
 *             scaling is exact: one rounding to float).  C_k = (-ln 2)^k / k! as these doubles:
 *               C0  0x1p+0                    C1  -0x1.62e42fefa39efp-1     C2  0x1.ebfbdff82c58ep-3      C3  -0x1.c6b08d704a0bfp-5
 *               C4  0x1.3b2ab6fba4e77p-7      C5  -0x1.5d87fe78a6730p-10    C6  0x1.430912f86c786p-13     C7  -0x1.ffcbfc588b0c5p-17
 *               C8  0x1.62c0223a5c822p-20     C9  -0x1.b5253d395e7c1p-24    C10 0x1.e4cf5158b8ec7p-28     C11 -0x1.e8cac7351bb22p-32
 *               C12 0x1.c3bd650fc2983p-36     C13 -0x1.816193166d0f7p-40    C14 0x1.314964d5878a7p-44     C15 -0x1.c36e843b0401ep-49
 *               C16 0x1.38e89ae79f8b1p-53
 *             p is within 4.5e-16 relative of 2^-f (measured over 200 000 arguments); w(0) = 1 exactly, so S0 >= 1 whenever a heading takes
 *             part; the cut at t >= 64 loses nothing a float sum of 2^24 terms next to a 1 can hold.  (pf::exp2m in csrc/pf_math.h.)
 *   moments   pfslam_estimate's, word for word: particle i becomes candidate k, its pose (x_i, y_j, theta_a) of k, gn the number of
 *             candidates, csum the canonical sum over k ascending with tiles of 4096 consecutive k (2^24 candidates are exactly the
 *             4096 x 4096 a csum can hold).
 *   cov_out   [0..2] mean m   [3..8] C: xx, xy, xtheta, yy, ytheta, thetatheta   [9] Neff = (S0 * S0) / S2   [10] S0   [11] S2
 *             [12] (float)candidates   [13] border share = fdiv(csum(e_k ? w_k : 0), S0)   [14] hs   [15] 0
 *             e_k: k lies on the first or the last index of a dimension that has more than one candidate.  A border share that is not
 *             small says the window cuts the distribution; C is then a lower bound.
 *             With status 2 the call succeeds and cov_out is all zero except [12] and [14].
 * Remarks.  The heading mean is linear, as in pfslam_estimate: headings are not wrapped.  Neff near 1 means the posterior is narrower
 * than the lattice; the caller then adds the quantisation variance (stride res)^2 / 12 per axis (step_theta^2 / 12 for the heading).  The
 * beams of a scan are not independent: a caller who wants n_ind effective beams out of n_in passes sigma_beam * sqrt(n_in / n_ind); the
 * default 0.2 is such a tempered value (at sigma = 0.05 the posteriors of the two scenarios below are narrower than the lattice, Neff 1.0
 * to 2.3).  The products w d d can reach float denormals and are kept: nothing is flushed, on the device or in the restatement.
 *   Measured with the restatement (tests/test_search_cov_spec.py), scan to scan, 1081 beams, window 21 x 21 x 9 at stride 1, the searched
 *   scan cast 0.1 m / 0.05 m / 0.0125 rad from the reference scan and the window centred there, sigma 0.2: between two walls y = +-1 from x = -30 to 30 the winner is
 *   0.1 m off along the corridor with nothing to show for it, and the covariance says so: sd_x 0.106 m, sd_y 0.0030 m, sd_theta
 *   0.00037 rad, Neff 11.9, border share 0.040.  In a closed 6 m x 4 m room the winner is the pose: sd 0.014 m / 0.0049 m / 0.0050 rad,
 *   Neff 2.9, border share 2e-17.
 * Refused (non-zero, pfslam_last_error names the cause under the new function's name, outputs untouched): everything pfslam_search (or
 * pfslam_search_scan) refuses, in its order and wording, a NULL cov or cov_out joining the first check; behind those and before any
 * launch: sigma not finite or not > 0; a reserved_ of pfslam_cov_opts that is not 0; hs not finite or not > 0.
 * Method.  k_search_ends, k_search_field / the scan splat, k_search_score and k_search_result run unchanged; the volume is always built
 * on the device and copied only when `scores` is not NULL.  The reduction is pfslam_estimate's three passes ordered by the stream --
 * moments, centred moments with the means re-derived per workgroup from the tile sums, the final sums -- one workgroup per tile of 4096
 * consecutive k, staged into LDS as float [4][4096] = (w, x, y, theta): one coalesced load of S_k per candidate, w_k from exp2m (recomputed
 * in the second pass, not stored: the same function of the same bits), the pose from k, which a thread divides into (a, j, i) once and
 * then steps.  The border sum is a twelfth quantity, summed by the wave that is idle in the moment pass.  Up to one tile one workgroup
 * does all three passes.  The summation order is the device functions' of pfslam_estimate, reused as they are.
 *   Measured on one MI355X, 1081 beams, the benchmark's 100 000-point map (profiles/search_cov.txt; HIP events around whole calls, beside
 *   pfslam_search with scores = NULL in the same process): the default window of 55 473 candidates 1.10 ms against 1.06 ms; 549 153
 *   candidates 1.38 ms against 1.34 ms; 16 776 177 candidates, just under the cap, 10.9 ms against 10.0 ms (on the 4000-point map 1.77 /
 *   1.73 ms, 2.15 / 2.11 ms, 11.8 / 10.9 ms); pfslam_search_scan_cov's default call without a map 0.22 ms against 0.18 ms.  The three
 *   reduction launches alone, from a kernel trace: 34 us for the default window (14 tiles), 40 us for 135 tiles, 0.87 ms for 4096
 *   tiles -- moments 139 us, centred moments 587 us, final sums 147 us; 450 us of the second pass are the means re-derived by every
 *   wave of every workgroup from 4 x 4096 tile sums, as pfslam_estimate's kernel does.
 *   Kernel resources (VGPRs / LDS bytes per workgroup / waves per SIMD): moments 18 / 65 536 / 3, centred moments 19 / 65 536 / 3, final
 *   sums 33 / 0 / 8, the one-workgroup form 31 / 65 536 / 3 (pfslam_estimate's: 23, 23, 32, 28): LDS is the only limit.
 * Like pfslam_search the call first books the frames in flight, runs on the handle's stream and honours pfslam_set_trig; one result copy
 * (cov_out rides with the result row) and one wait (+ one for a NULL centre of pfslam_search_cov).  The field, end points, counts and
 * volume are pfslam_search's buffers, the scans and points pfslam_search_scan's; the tile sums and the result row are buffers of its own
 * that belong to the handle, grow when a call needs more and go with pfslam_destroy.  No state another entry point reads is written.
 * Nothing is sharded, so every rank of a sharded handle gets the unsharded bits. */
typedef struct pfslam_cov_opts {
    float   sigma;         /* metres; finite, > 0 */
    int32_t reserved_[3];  /* must be 0 */
} pfslam_cov_opts;
/* {0.2f, {0, 0, 0}} */
void pfslam_search_cov_default_opts(pfslam_cov_opts *o);
int pfslam_search_cov(pfslam_handle *h, const float centre[3] /* NULL = the handle's pose */, const pfslam_search_opts *opts,
                      const pfslam_cov_opts *cov, float pose_out[3], float info[8], float cov_out[16],
                      int32_t *scores /* NULL or one int per candidate */);
int pfslam_search_scan_cov(pfslam_handle *h, const float *ref_scan_host, const float ref_pose[3] /* NULL = (0, 0, 0) */,
                           const float *scan_host /* NULL = the handle's scan */, const float centre[3] /* NULL = ref_pose */,
                           const pfslam_search_opts *opts, const pfslam_cov_opts *cov, float pose_out[3], float info[8], float cov_out[16],
                           int32_t *scores /* NULL or one int per candidate */);
/* pfslam_move_particles: the odometry motion model (no reference counterpart: the reference's filter has no motion model besides the
 * diffusion of kernel.cu:375-397).  pfslam_shift_particles adds one world-frame increment to every pose, which is wrong as soon as the
 * cloud's headings differ, and drops the increment's uncertainty.  Here every particle moves by the increment ROTATED INTO ITS OWN FRAME
 * and gets correlated Gaussian noise drawn from a 3 x 3 covariance laid out as pfslam_search_cov / pfslam_search_scan_cov write it:
 * cov = cov_out + 3, with delta = pose_out - ref_pose and ref_theta = ref_pose[2] of the same search.  The draw is deterministic, keyed
 * by `frame` and the GLOBAL particle index, and bit-identical for any sharding.
 * Specification.  All arithmetic is float, one rounding per operation, in the order written, no contraction; fdiv and fsqrt are
 * correctly rounded.
 *   factor L (host, once per call)
 *             c = cov, or zeros when cov is NULL
 *             a00 = cov_scale * c[0] + sigma_xy_min * sigma_xy_min
 *             a10 = cov_scale * c[1]
 *             a20 = cov_scale * c[2]
 *             a11 = cov_scale * c[3] + sigma_xy_min * sigma_xy_min
 *             a21 = cov_scale * c[4]
 *             a22 = cov_scale * c[5] + sigma_theta_min * sigma_theta_min
 *             Cholesky, lower:
 *             p0 = a00;                          L00 = fsqrt(p0), L10 = fdiv(a10, L00), L20 = fdiv(a20, L00)
 *             p1 = a11 - L10 * L10;              L11 = fsqrt(p1), L21 = fdiv(a21 - L20 * L10, L11)
 *             p2 = a22 - (L20 * L20 + L21 * L21); L22 = fsqrt(p2)
 *             A pivot that is exactly 0 makes its whole column of L zero, with no division.  A pivot that is negative or not finite is
 *             refused ("covariance is not positive semi-definite").
 *   particle  with LOCAL index i and GLOBAL index g = global_offset + i:
 *             e = engine_seed(frame, g, 1)        (depth 1: a stream of its own beside the dispersion's engine_seed(frame, g, 0))
 *             z1, z2, z3 = normal(e, 0, 1), three successive draws (pf::normal of csrc/pf_math.h; pfslam_set_trig picks its device-library
 *             form, as in the dispersion)
 *             mx  = delta[0] + L00 * z1
 *             my  = delta[1] + (L10 * z1 + L11 * z2)
 *             mt  = delta[2] + ((L20 * z1 + L21 * z2) + L22 * z3)
 *             phi = theta_i - ref_theta
 *             (s, c) = sincosf_spec(phi)          (pfslam_set_trig 1: the device library's sinf / cosf)
 *             x'     = x + ((c * mx) - (s * my))
 *             y'     = y + ((s * mx) + (c * my))
 *             theta' = theta + mt
 *   robot pose  the same formulas with z1 = z2 = z3 = 0 and phi = pose.theta - ref_theta.
 *   weights     untouched.
 * Identity.  With cov == NULL, zero floors and every heading equal to ref_theta (phi = 0: s = 0, c = 1) the particles are those of
 * pfslam_shift_particles(delta) bit for bit, for operands that are not signed zeros.
 * Remarks.  A cov from a search whose Neff is near 1 says the posterior is narrower than the search's lattice: it needs the floors, the
 * quantisation deviations sigma_xy_min = stride res / sqrt(12) and sigma_theta_min = step_theta / sqrt(12) (see pfslam_search_cov's
 * remarks).  cov_scale tempers or inflates the covariance as a whole (0: the floors alone).  Headings are not wrapped, as everywhere.
 * The host's bound on |heading| (it selects the scan-match kernel's instantiation) grows at once by
 * |delta[2]| + 7 (|L20| + |L21| + |L22|): 7 is the next integer above the largest |normal(., 0, 1)| the generator can return (the draw
 * u = 0, 6.2303).
 * Refused (non-zero, pfslam_last_error names the cause under this function's name, nothing is enqueued), in this order: a NULL h, delta
 * or opts; a delta, cov entry, ref_theta, cov_scale or floor that is not finite; a negative cov_scale or floor; a reserved_ that is not
 * 0; a bad pivot.
 * Method.  k_move (csrc/pfslam_move.hip.inc): one thread per particle, coalesced SoA, 256-thread workgroups, like the dispersion's
 * kernel; L, delta, ref_theta, frame, the global offset and the trig mode are kernel arguments; no LDS, no scratch, no atomics; its cost
 * is three erfcinv evaluations and one sincos in fp64.  One thread moves the robot's pose and, by the pose's increment, the cloud
 * statistics the next frame's lane order starts from (performance only).  Like pfslam_shift_particles the call does NOT book the frames
 * in flight: it is enqueued behind them on the particle stream, with the same edges, and there is no host wait.  Sharded handles: every
 * rank calls it with the same arguments; only g enters the draw, so the concatenated shards equal the unsharded handle bit for bit.
 * Measured: profiles/move_particles.txt. */
typedef struct pfslam_move_opts {
    float   ref_theta;        /* heading (rad) of the frame `delta` and `cov` are expressed in; finite */
    float   cov_scale;        /* finite, >= 0 */
    float   sigma_xy_min;     /* m,   finite, >= 0 */
    float   sigma_theta_min;  /* rad, finite, >= 0 */
    int32_t reserved_[4];     /* must be 0 */
} pfslam_move_opts;
/* {0, 1, 0, 0, {0, 0, 0, 0}} */
void pfslam_move_default_opts(pfslam_move_opts *o);
int pfslam_move_particles(pfslam_handle *h, int frame, const float delta[3],
                          const float cov[6] /* NULL = zero; xx, xy, xtheta, yy, ytheta, thetatheta: cov_out + 3 of pfslam_search*_cov */,
                          const pfslam_move_opts *opts);
/* pfslam_search_wide: pfslam_search's winner over windows far beyond its cap (no reference counterpart) -- "where on this map was this scan
 * taken", at any heading: the kidnapped robot, a restart on a saved map, a loop-closure candidate checked at every heading.  +-20 m and a
 * full turn on a 40 m map at 0.025 m are 1601 x 1601 x 503 = 1 289 290 103 candidates: 77 pfslam_search calls at the cap.
 * Definition by reference.  The candidates k, theta_a, x_i, y_j, the end points, the field, S(k), the tie rule (the smallest S, the
 * lowest k among equal ones; a heading with no in-range beam takes no part), pose_out, info and status 2 are pfslam_search's, word for
 * word.  For every call pfslam_search accepts, pose_out and info are bit for bit what pfslam_search returns.  HOW the winner is found is
 * not part of the specification (see "Method").  There is no `scores` array: the volume can pass 2^30 entries.
 *   stats     NULL or int64[8]: info[1] = (float)k and info[5] = (float)candidates round above 2^24, so stats carries them exactly:
 *             [0] k (-1 with status 2)   [1] candidates   [2] nodes bounded above level 0   [3] level-0 candidates scored
 *             [4] top level used         [5] batches      [6] cells of the field box the call built   [7] 0
 *             [2], [3] and [5] describe what the implementation did; they are not specified values.
 * Caps: at most 2^31 - 1 candidates, so that k stays a non-negative int32 and the 64-bit key (S << 32 | k) is kept;
 * (2 half_x + 1)(2 half_y + 1) <= 2^24; at most 2^24 end points; the field is bounded as pfslam_search's, 2^26 cells.  Every other refusal
 * of pfslam_search applies, in the same order and with the same wording under this function's name.
 * Method.  Candidates lie on a lattice and a translation is an index shift into one field, so the sum of the same lookups into a
 * min-pooled copy of the field bounds S from below for a whole block of translations at once.  M_0 = q; M_L[x, y] = min of M_{L-1} at
 * (x, y), (x + h, y), (x, y + h), (x + h, y + h), h = 2^(L-1) stride, terms outside the box skipped: the smallest q of a 2^L x 2^L block
 * of the window's own lattice.  A node is (heading a, block origin (I, J), level L); LB = sum over the in-range beams of
 * M_L[ex + (I - hx) stride, ey + (J - hy) stride] <= S of every candidate of the block, and = S at level 0.  The block's origin is a
 * candidate, the block's lowest k, and its exact S is the same index into M_0: every node scored also offers its origin to the key.
 * From the top level (the smallest L <= 7 with 2^L >= the window's longer side) down: score a level, then drop a node only if
 * (LB << 32 | k_origin) > the key -- never on LB = S alone, which would lose the lowest-k tie -- and split the others into their up to
 * four children inside the window.  The frontier is bounded: a level is worked through in batches of a quarter of a frontier buffer
 * (2^22 nodes), each batch taken down to level 0 before the next, so poor pruning costs time, never the result.
 * Memory: a call holds (top level + 1) fields of the box's size, at worst 8 x 128 MB, and (top level + 2) frontier buffers of 16 MB.
 * Host waits: one per batch above level 0 (it reads how many children the batch left) and one for the result; a call whose levels fit a
 * batch each makes at most top level + 1 waits, at most 8 (+ one for a NULL centre).
 * The counts in stats[2], [3] and [5] are the same from run to run while every level fits one batch; beyond that the order in which a level's
 * survivors were appended decides which share a batch, and the counts (never the result) can differ by a few.
 *   Measured on one MI355X, 1081 beams, the scan cast from (10, -8, 0.3) (profiles/search_wide.txt; HIP events around whole calls): the
 *   whole map, 1601 x 1601 x 503 = 1 289 290 103 candidates around (0, 0, 0), takes 13.3 ms on the 4000-point map (206 727 nodes bounded,
 *   4 candidates scored, 8 batches; the field of 10.2 M cells is 10.3 ms of it, the scoring 2.5 ms, the seven pyramid levels 0.2 ms) and
 *   14.5 ms on the benchmark's 100 000-point map (3.46 M nodes bounded, 40 candidates scored, 16 - 17 batches; field 6.4 ms, scoring 7.2 ms).
 *   The same winner from 503 pfslam_search calls, one per heading -- the only exact way before -- takes 3622 ms and 3634 ms: 273 and 251
 *   times as long (two runs each, 2 ms and 7 ms apart).  713 x 713 x 33, just under pfslam_search's cap: 3.0 ms and 2.4 ms against 10.3 ms
 *   and 9.5 ms for the one pfslam_search call; 725 x 725 x 33, just above it: 3.0 ms and 2.6 ms against 91 ms and 76 ms for 33 per-heading
 *   calls.  The default window, where the pyramid is overhead: 1.63 ms and 0.94 ms against pfslam_search's 1.48 ms and 0.82 ms.
 *   Kernel resources (VGPRs / LDS bytes per workgroup / waves per SIMD): pyramid 9 / 0 / 8, top level 14 / 0 / 8, scoring 59 / 0 / 8 (44 at
 *   level 0), expansion 18 / 0 / 8.
 * Like pfslam_search it first books the frames in flight and then runs on the handle's stream, honours pfslam_set_trig, reads the handle's
 * device-resident map and scan and writes no state another entry point reads: the fields, the end points, the frontier and the result are
 * its own buffers (they belong to the handle, grow when a call needs more and go with pfslam_destroy).  The map and the scan of a sharded
 * handle are replicated, so every rank gets the unsharded handle's bits. */
int pfslam_search_wide(pfslam_handle *h, const float centre[3] /* NULL = the handle's pose */, const pfslam_search_opts *opts,
                       float pose_out[3], float info[8], int64_t stats[8] /* may be NULL */);
/* pfslam_search_best: the N best separated poses of a search window (no reference counterpart) -- the best candidate of each of the N best
 * REGIONS of the window, because the N smallest scores alone all sit next to the winner.  Corridors, repeated rooms and a short scan give
 * several basins with nearly equal scores, and the global minimum of a saturated, quantised score can be the wrong one: the rows are what
 * pfslam_register_batch takes as `starts`, and what a particle filter is seeded with.  As wide as pfslam_search_wide, and exact.
 * Definition by reference.  The candidates k = (a * ny + j) * nx + i, theta_a, x_i, y_j, the end points, the field, S(k) and the rule that a
 * heading with no in-range beam takes no part are pfslam_search's, word for word (nx = 2 half_x + 1, ny, na likewise).
 *   key              of a candidate: S(k) << 32 | k.  Keys are distinct, so their order is total.
 *   cells            the candidates are partitioned: with Ls = tile_log2 and G = group_theta, candidate (a, j, i) belongs to cell
 *                    ((a / G) * ty + (j >> Ls)) * tx + (i >> Ls), tx = ((nx - 1) >> Ls) + 1, ty likewise, ceil(na / G) heading groups.  A tile is
 *                    2^Ls x 2^Ls translations of the window's own lattice, counted from i = 0, j = 0 (the alignment of the blocks
 *                    pfslam_search_wide descends through); a group is G consecutive headings.
 *   representative   of a cell: the smallest key among its candidates that take part; a cell without one has none.
 *   result           the `count` cells with the smallest representatives, in ascending key order.  *found = the rows written, smaller than
 *                    `count` only when fewer cells have a representative.  Row r: index[r] = k_r, exact; poses_out[3 r ..] the pose of k_r;
 *                    info[8 r ..] = {0, (float)k_r, n_in of its heading, fdiv((float)S * u, (float)n_in), (float)S, (float)candidates,
 *                    (float)qcap, 0}: pfslam_search's info for that candidate.  Rows beyond *found are left untouched.  When no heading has
 *                    an in-range beam the call succeeds with *found = 0 and writes no row.
 *   stats            NULL or int64[8], pfslam_search_wide's: [0] k of row 0 (-1 with no row) [1] candidates [2] nodes bounded above level 0
 *                    [3] level-0 candidates scored [4] top level used [5] batches [6] cells of the field box [7] the cells of the call.
 *                    [2], [3] and [5] describe what the implementation did; they are not specified values.
 * Consequences.  Row 0 is pfslam_search_wide's winner bit for bit, for every tile_log2 and group_theta.  With count = 1, pose and info equal
 * pfslam_search_wide's on every call both functions accept.  The separation is by partition, not by distance: two rows can be neighbours
 * across a tile border.  A caller who wants one row per basin refines the rows with pfslam_register_batch, where they converge.
 * Refused (non-zero, pfslam_last_error names the cause, outputs untouched): everything pfslam_search_wide refuses, in its order and wording
 * under this function's name; then a NULL best, poses_out, info, index or found; count outside 1 .. 64; tile_log2 outside 0 .. 7;
 * group_theta < 1; reserved_ non-zero; more than 2^22 cells, which bounds the table of representatives to 32 MB (the whole map at the
 * defaults is 201 x 201 x 63 = 2 545 263 cells).
 * Method.  pfslam_search_wide's descent (the same pyramid, nodes, batches of a quarter of a frontier buffer and one host wait per batch;
 * the test hook that shrinks its frontier shrinks this one too) over a table T of one key per cell, all ones at the start.  Every node scored
 * offers its origin's exact key to T[cell of the origin] with a 64-bit atomicMin, and to the minimum of the cell's slice (cell c lies in
 * slice c mod 4096).  After a batch's scoring launch one workgroup selects thr, the count-th smallest of the 4096 slice minima (all ones
 * with fewer set): entries of T only fall and the minima of different slices belong to different cells, so thr bounds the final count-th
 * smallest representative from above.  A node with key nk = LB << 32 | k_origin is dropped (1) if nk > thr, or (2) if L <= Ls -- its block
 * then lies inside one cell -- and nk > T[that cell].  Equality never drops a node, as in pfslam_search_wide.  At the end the cells with
 * T <= thr are compacted, copied (the list has room for every cell, so a long list costs a copy, never the result) and sorted on the
 * host; a last kernel fills the rows.  Memory beyond pfslam_search_wide's: 16 bytes a cell.  Host waits: pfslam_search_wide's, + 2.
 *   Measured on one MI355X, 1081 beams, the scan cast from (10, -8, 0.3) (profiles/search_best.txt; HIP events around whole calls):
 *   the whole map, 1601 x 1601 x 503 candidates in 201 x 201 x 63 = 2 545 263 cells around (0, 0, 0), at the defaults (count 8) takes 15.2 ms
 *   on the 4000-point map (344 545 nodes bounded, 64 candidates scored, 8 batches) and 19.0 ms on the benchmark's 100 000-point map (5.19 M
 *   nodes bounded, 1012 candidates scored, 24 batches), beside pfslam_search_wide's 13.1 ms and 14.5 ms in the same process: 1.16 and 1.31
 *   times as long.  The same eight rows the only other exact way -- 503 pfslam_search calls with their volumes copied back and the cells
 *   reduced on the host -- take 14.2 s and 8.7 s of wall clock: 930 and 459 times as long.  count = 1: 13.3 ms and 14.9 ms, 1.01 and 1.02
 *   times pfslam_search_wide (the same nodes); count = 64: 22.2 ms and 24.6 ms, 1.69 times.  713 x 713 x 33: 3.2 ms and 2.8 ms against
 *   pfslam_search_wide's 3.0 ms and 2.4 ms; 725 x 725 x 33: 3.3 ms and 2.9 ms against 3.1 ms and 2.6 ms; the default window: 1.79 ms and
 *   1.10 ms against 1.64 ms and 0.96 ms.
 *   Kernel resources (VGPRs / LDS bytes per workgroup / waves per SIMD): scoring 59 / 0 / 8 (44 at level 0), threshold 26 / 34 944 / 4 (one
 *   workgroup a launch), expansion 19 / 0 / 8, compaction 5 / 0 / 8, rows 16 / 0 / 8.
 * Like pfslam_search_wide it first books the frames in flight and then runs on the handle's stream, honours pfslam_set_trig, reads the
 * handle's device-resident map and scan and writes no state another entry point reads: the fields, end points and frontier are
 * pfslam_search_wide's scratch, the table, the list and the rows its own buffers (they belong to the handle, grow when a call needs more and
 * go with pfslam_destroy).  The map and the scan of a sharded handle are replicated, so every rank gets the unsharded handle's bits. */
typedef struct pfslam_best_opts {
    int32_t count;        /* rows wanted, 1 .. 64 */
    int32_t tile_log2;    /* Ls, 0 .. 7: a tile is 2^Ls x 2^Ls translations of the window's own lattice */
    int32_t group_theta;  /* G >= 1: a group is G consecutive headings */
    int32_t reserved_;    /* must be 0 */
} pfslam_best_opts;
/* {8, 3, 8, 0} */
void pfslam_search_best_default_opts(pfslam_best_opts *opts);
int pfslam_search_best(pfslam_handle *h, const float centre[3] /* NULL = the handle's pose */, const pfslam_search_opts *opts,
                       const pfslam_best_opts *best, float *poses_out /* count x 3 */, float *info /* count x 8 */,
                       int64_t *index /* count */, int *found, int64_t stats[8] /* may be NULL */);
/* pfslam_cast / pfslam_map_raster: the scan the point-cloud map PREDICTS from a pose (no reference counterpart).  Every other question
 * the library answers about its map is an end-point question ("how close is this beam's end to a node"); this one walks each beam through
 * an occupancy raster of the nodes until it meets an occupied cell.  It gives per-beam residuals between a measured and an expected
 * range (a beam through a mapped wall still ends "near a point"), a beam-model check of the poses pfslam_search_best and
 * pfslam_register_batch return, visibility on the KD path, and an occupancy raster of the map for export.
 *   max_range   m; finite, > 0; max_range / map_res_x and max_range / map_res_y both <= 16384
 *   w_min       a node takes part iff w >= w_min (false for a NaN weight); finite
 *   no_hit      the range reported for a ray that hits nothing; any float
 *   inflate     0 .. 8: a node occupies the (2 inflate + 1)^2 cells around its own
 *   skip_cells  >= 0: the first cell index of the walk that can be a hit (0 = the robot's own cell)
 *   reserved_   must be 0
 * All arithmetic is float, one rounding per operation, in the order written, no contraction; fdiv and fsqrt are the correctly rounded
 * division and square root; integers are exact.  res_x = map_res_x, res_y = map_res_y (they may differ: nothing here needs square cells).
 *   raster      a node (x, y, z, w) has the cell nx = rintf(fdiv(x, res_x)), ny = rintf(fdiv(y, res_y)); z is ignored.  It qualifies iff
 *               w >= w_min && |nx| <= 2^20 && |ny| <= 2^20 (each false for a NaN).  The occupied set O holds the cells (kx, ky) for which
 *               some qualifying node has |kx - nx| <= inflate && |ky - ny| <= inflate.  The box x0, y0, W, H is the bounding box of the
 *               qualifying cells grown by inflate.  With no qualifying node the box is {0, 0, 0, 0}, every ray misses, the call succeeds.
 *   ray         of pose (x, y, theta) and beam b: (wx, wy) = CleanLidarScan(b, max_range, theta) (it honours pfslam_set_trig);
 *               sx = rintf(fdiv(x, res_x)), ex = rintf(fdiv(x + wx, res_x)), sy and ey likewise.  The ray misses if one of the four is
 *               not finite or lies beyond +-2^20.  dx = ex - sx, dy = ey - sy, n = max(|dx|, |dy|); with n == 0 the ray misses.
 *   walk        anchored at the robot, every cell a closed form of its index t, t = skip_cells .. n:
 *                 |dx| >= |dy|:  kx = sx + sgn(dx) t,  ky = sy + sgn(dy) ((2 t |dy| + n) div (2 n))
 *                 otherwise:     ky = sy + sgn(dy) t,  kx = sx + sgn(dx) ((2 t |dx| + n) div (2 n))
 *               (the products stay below 2^31 by the bound on max_range).  The hit is the smallest t whose cell is in O.
 *   range       fsqrt(ddx * ddx + ddy * ddy) with ddx = (float)kx * res_x - x, ddy = (float)ky * res_y - y.  A ray that misses reports
 *               no_hit and the cell (INT32_MIN, INT32_MIN).
 *   outputs     ranges_out[r * n_beams + b]; cells_out[(r * n_beams + b) * 2 + {0, 1}] = kx, ky; stats: [0] rays, [1] hits,
 *               [2] qualifying nodes, [3] |O|, [4..7] x0, y0, W, H -- all eight are specified values.
 * pfslam_map_raster builds the same raster: stats as above with [0] = [1] = 0, occ[(kx - x0) * H + (ky - y0)] = 1 iff (kx, ky) is in O.
 * occ == NULL returns the stats only (the two-call pattern: ask for W and H, allocate, ask again).
 * Refused (non-zero, pfslam_last_error names the cause under the function's name, outputs untouched): a NULL handle, opts or ranges_out
 * (pfslam_map_raster: a NULL stats); m outside 1 .. 65536 or m * n_beams > 2^24; poses == NULL with m != 1; an option outside its range
 * or reserved_ non-zero; no map; W * H > 2^28 (found on the device: one extra wait, like pfslam_search_wide's); cap < W * H.  A pose that
 * is not finite is not refused: all of its rays miss.
 * Method.  One thread per node merges the box into four biased words with atomicMax (k_search_ends' scheme) and counts the qualifying
 * nodes; the host reads the words (the extra wait) and sizes the raster: 8 x 8-cell tiles of one 64-bit word each.  A clear, then one
 * thread per node ORs the node's cells into at most 3 x 3 tiles (an OR is exact in any order), then a count of |O|.  The cast is one lane
 * per ray, adjacent lanes the adjacent beams of one pose.  Because every cell is a closed form of t a ray jumps: to the first t inside
 * the box (a start outside enters by it), and out of every empty tile to the first t that leaves it along either axis; inside a tile
 * that holds something it steps cell by cell.  How the hit is found is no part of the specification.  Measured: profiles/cast.txt.
 * Like every entry point but the step functions both calls first book the frames in flight and then run on the handle's stream.  They
 * read the device-resident map and, for poses == NULL, the pose (on the device).  They write no state another entry point reads: not the
 * pose, the particles, the tree, the 2-D grid, buffers 11 / 12 or the search buffers.  The raster, the pose list and the outputs are
 * buffers of their own: they belong to the handle, are allocated on first use, grow when a call needs more and go with pfslam_destroy.
 * Every call rebuilds the raster (the map changes every frame).  The map of a sharded handle is replicated: every rank gets the
 * unsharded bits. */
typedef struct pfslam_cast_opts {
    float   max_range;
    float   w_min;
    float   no_hit;
    int32_t inflate;
    int32_t skip_cells;
    int32_t reserved_[3];
} pfslam_cast_opts;
/* {30.0f, 1.0f, 30.0f, 1, 1, {0, 0, 0}} */
void pfslam_cast_default_opts(pfslam_cast_opts *o);
int pfslam_cast(pfslam_handle *h, const float *poses /* m x 3; NULL = the handle's pose, m must be 1 */, int m,
                const pfslam_cast_opts *opts, float *ranges_out /* m x n_beams */,
                int32_t *cells_out /* NULL or m x n_beams x 2 */, int64_t stats[8] /* may be NULL */);
int pfslam_map_raster(pfslam_handle *h, const pfslam_cast_opts *opts, int64_t stats[8],
                      uint8_t *occ /* NULL or W * H bytes */, size_t cap);
/* pfslam_cast_score: the beam-model score of poses -- a measured scan compared beam by beam with the scan pfslam_cast expects from each
 * pose, fused into the cast and reduced per pose on the device (no reference counterpart).  The rest of the pose family (pfslam_search*,
 * pfslam_register*, the filter's own scan match) asks where a beam ENDS; a pose whose beams pass through mapped walls can score well on
 * that question (the symmetric-room and corridor ambiguities pfslam_search_best lists).  This call separates them, and it is the last
 * link of search_best -> register_batch -> pick.  The poses are a list, the handle's pose, or the handle's own particles, which are read
 * where they live; what comes back is eight integers per pose, not m x n_beams ranges.
 *   tol         m: |measured - expected| <= tol agrees; finite, >= 1e-4
 *   clip        m: the residual saturates here; finite
 *   z_min,z_max a measured range takes part iff z >= z_min && z <= z_max (false for a NaN); finite, z_min <= z_max
 *   count_miss  0 / 1: a measured beam whose ray hits nothing costs qcap
 *   source      0 = `poses` (NULL: the handle's pose, m == 1), 1 = the handle's own particles (poses NULL, m == n_particles)
 *   reserved_   must be 0
 * All arithmetic is float, one rounding per operation, in the order written, no contraction; fdiv is the correctly rounded division;
 * integers are exact.
 *   expected    the raster, the ray, the walk and the range are pfslam_cast's, word for word, for the same `cast` options: for pose r and
 *               beam b, hit and e are exactly what pfslam_cast reports.  cast->no_hit is not read.  pfslam_set_trig is honoured.
 *   unit        u = tol * 0.0625f; qcap = (int)rintf(fdiv(clip, u)), refused unless 16 <= qcap <= 32767.
 *   measured    z = scan[b] (scan_host, or the handle's scan when that is NULL); valid = z >= z_min && z <= z_max.
 *   residual    d = z - e, a = fabsf(d), fq = rintf(fdiv(a, u)), q = fq >= (float)qcap ? qcap : (int)fq (the compare comes before the
 *               conversion: a huge a has a defined result).
 *   class       of a beam, as written to classes_out[r * n_beams + b]: 0 not valid; 1 valid, the ray misses; 2 agree: valid, hit,
 *               a <= tol; 3 through: valid, hit, d > tol (the measured beam ends behind a mapped wall); 4 short: every other valid hit.
 *   row r       rows_out[r * 8 + ..]: [0] valid beams, [1] agree, [2] through, [3] short, [4] valid misses, [5] Q1 = sum of q over the
 *               classes 2 .. 4, [6] Q2 = sum of q * q over class 2 (q <= 16 there, exactly), [7] cost = Q1 + (count_miss ? qcap * [4] : 0).
 *               Everything is an integer below 2^31 (4096 x 32767): exact in any summation order, like the search family's scores.
 *   *best       decided on the host from the rows alone: eligible rows have [1] > 0; among them the smallest cost wins, then the larger
 *               [1], then the lowest row; -1 when no row is eligible.  [0] depends on the scan only, so costs compare across rows.
 *   stats       pfslam_cast's eight specified values; [1] counts every ray that hits, whether its beam is valid or not.
 *   source 1    row r is the local particle r of the handle, read on the device from the pose block (pfslam_device_ptr buffer 16,
 *               [x | y | theta] with shard_stride between the blocks); no particle is copied to the host.  A sharded rank scores its own
 *               shard.
 * m is 1 .. 65536 and n_beams at most 4096.  No per-ray output exists unless classes_out is given, so pfslam_cast's cap of 2^24 rays
 * applies only then.
 * Refused (non-zero, pfslam_last_error names the cause under this function's name, outputs untouched, the handle goes on), in this
 * order: a NULL handle, cast, opts or rows_out; m out of range; n_beams > 4096; source outside 0 .. 1; source 0 with poses == NULL and
 * m != 1; source 1 with poses != NULL or m != n_particles; classes_out with more than 2^24 rays; everything pfslam_cast refuses in its
 * options; tol, clip, z_min, z_max, count_miss or reserved_ out of range; qcap out of range; no map; the raster above 2^28 cells.  A
 * pose that is not finite is not refused: all of its rays miss.
 * Method.  The raster is built as for pfslam_cast (with its one extra wait).  Then one lane per ray, adjacent lanes the adjacent beams of
 * one pose, the walk the cast's own function.  The poses come through three pointers and a stride, so one kernel reads a list (stride 3)
 * and the particle block (stride 1).  A lane holds the seven counters of its beam and its hit; a wave adds them up by pose with a
 * segmented reduction across its lanes, and the first lane of each pose in the wave adds what is not zero to the pose's row, which the
 * call cleared.  On the device the row's last word is the pose's hits; the host sums them into stats[1] and writes the cost there, so no
 * address is shared between poses: only the waves of one pose add to its row.  Class bytes are written only when asked for.  The other
 * layout -- one 256-thread workgroup per pose, the beams strided over its threads, the row stored and neither cleared nor added to -- was
 * built and measured first and lost at every size (2.3 x at one pose): profiles/cast_score.txt.
 * Like pfslam_cast it first books the frames in flight and then runs on the handle's stream.  It reads the map, the scan and (source 1)
 * the pose block, and writes no state another entry point reads.  It reuses the cast's raster buffers and pose list; its scan copy, its
 * rows and its class bytes are buffers of its own on the handle, allocated on first use, grown when a call needs more, freed by
 * pfslam_destroy.  Beyond the raster's wait it makes one wait, for the rows, the state words and (when asked for) the classes. */
typedef struct pfslam_cast_score_opts {
    float   tol;
    float   clip;
    float   z_min, z_max;
    int32_t count_miss;
    int32_t source;
    int32_t reserved_[2];
} pfslam_cast_score_opts;
/* {0.1f, 1.0f, 0.1f, 20.0f, 1, 0, {0, 0}} */
void pfslam_cast_score_default_opts(pfslam_cast_score_opts *o);
int pfslam_cast_score(pfslam_handle *h, const float *poses /* m x 3, or NULL (see source) */, int m,
                      const float *scan_host /* n_beams; NULL = the handle's scan */, const pfslam_cast_opts *cast,
                      const pfslam_cast_score_opts *opts, int32_t *rows_out /* m x 8 */, uint8_t *classes_out /* NULL or m x n_beams */,
                      int *best /* may be NULL */, int64_t stats[8] /* may be NULL */);
/* ---- round-5 frame loop: test and measurement support (no reference counterpart) ----
 * pfslam_set_serial(h, 1): every launch of every frame on ONE stream, in the order the four chains of a frame are enqueued (what the
 * environment variable PFSLAM_SERIAL=1 sets at creation).  Results and the cell rows' bookkeeping are the same as with the chains on their
 * own streams; tests/test_gpu_frame.py steps the same cases both ways and compares.
 * pfslam_debug_check_cells: the invariants of the persistent cell rows checked on the device, with no frame in flight -- out[0] records,
 * [1] never walked, [2] walked and not yet published, [3] published, [4] row words in the table, [5] pending words, [6] fallback words,
 * [7] records without rows; VIOLATIONS (all zero or the bookkeeping is broken): [8] claimed cell neither walked nor pending, [9] unpublished
 * record whose claim word is not pending (or a malformed word), [10] row outside its record's pool allocation, [11] row slot that is not a
 * candidate of its record (or out of order), [12] a watched link that has gained a node and was not extended (a stale row waiting to
 * happen), [13] malformed link word, [14] record without rows that has one, [15] the table does not hold what the counters say.
 * pfslam_set_probe(h, frames) / pfslam_get_probe: the first thread of every launch of a round-5 frame stores the 100 MHz wall clock;
 * out[f][32] for the last n tickets (0 = that launch did not run), slot names from pfslam_probe_name. */
int pfslam_set_serial(pfslam_handle *h, int serial);
int pfslam_debug_check_cells(pfslam_handle *h, long long out[16]);
int pfslam_set_probe(pfslam_handle *h, int frames);
int pfslam_get_probe(pfslam_handle *h, unsigned long long *out, int cap_frames, int *n_frames, int *last_ticket);
const char *pfslam_probe_name(int slot);
/* out[0] 1 = the last frame ran as a round-5 frame, [1] 1 = its cross-stream edges are gates (0 = events), [2] 1 = one-stream mode, [3] publication lag */
int pfslam_frame_mode(pfslam_handle *h, int out[4]);

/* ---- host-side map structure (kdtree.cpp counterpart; no GPU needed) ---- */
int pfslam_kd_create(const float *pts_xyzw, int n, pfslam_node *out);
/* KDTree::InsertList (kdtree.cpp:46-67): sub-tree of n points in pre-order at list[idx ...] below `parent` (-1: root) */
int pfslam_kd_insert_list(const float *pts_xyzw, int n, pfslam_node *list, int idx, int parent);
int pfslam_kd_insert_node(const float p[4], pfslam_node *list, int list_size);
int pfslam_kd_balance(pfslam_node *list, int n);
/* 1 = the host build sorts on several threads (libstdc++ only; a start-up self-check against std::sort on a heavily tied array
 * must have passed), 0 = plain std::sort.  Either way the tree is std::sort's. */
int pfslam_kd_parallel_sort(void);
/* threads a host-side build may use: usable cores (scheduler affinity, cgroup quota) / LOCAL_WORLD_SIZE; PFSLAM_SORT_THREADS overrides */
int pfslam_kd_sort_threads(void);
/* 1: lift the LOCAL_WORLD_SIZE split (the caller is the node's only builder while the other ranks wait: pfslam_shard_balance_build
 * does this around its build), 0: back to the per-rank share.  No reference counterpart (the reference is single-process). */
void pfslam_kd_whole_node(int on);

#ifdef __cplusplus
}
#endif
#endif
