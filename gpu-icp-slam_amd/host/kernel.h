// kernel.h -- drop-in for the reference's src/kernel.h:14-24: same free functions, same structs, implemented on
// libpfslam_hip.so (MI355X).  pbo arguments are accepted and ignored exactly as particleFilter() ignores its own
// (kernel.cu:1702, H9); drawMap is a no-op (visualisation is out of scope).
#pragma once
#include <vector>
#include "kdtree.hpp"
#include "lidar.h"
#include "scene.h"

#ifndef __HIP_PLATFORM_AMD__
struct uchar4 { unsigned char x, y, z, w; };
#endif

// The reference chooses between its GPU and CPU branches of the 2-D path at compile time (kernel.h:9-12; no #ifndef there, so
// they cannot be overridden).  Every stage runs on the GPU here; the macros exist so that callers naming them still compile.
#ifndef GPU_MOTION
#define GPU_MOTION 1
#endif
#ifndef GPU_MEASUREMENT
#define GPU_MEASUREMENT 1
#endif
#ifndef GPU_MAP
#define GPU_MAP 1
#endif
#ifndef GPU_RESAMPLE
#define GPU_RESAMPLE 1
#endif

// floor(log2 x) and ceil(log2 x) helpers of kernel.h:26-36 (x >= 1; ilog2(0) = 0 as there)
inline int ilog2(int x) { return x > 1 ? 31 - __builtin_clz((unsigned)x) : 0; }
inline int ilog2ceil(int x) { return ilog2(x - 1) + 1; }

void particleFilterInit(Scene *scene);
void particleFilterFree();
void particleFilter(uchar4 *pbo, int frame, Lidar *lidar);
void drawMap(uchar4 *pbo);
void getPCData(Particle **ptrParticles, MAP_TYPE **ptrMap, KDTree::Node **ptrKD, int *nParticles, int *nKD, glm::vec3 &pos);
void particleFilterInitPC();
void particleFilterFreePC();
// declared by the reference (kernel.h:24) but never defined there; here it is the point-cloud frame: particleFilter without
// the unused pbo
void particleFilterPC(int frame, Lidar *lidar);

// PARTICLE_COUNT is a compile-time 1000 in the reference (kernel.cu:30); here it is a runtime setting read by the
// next particleFilterInit (also: environment variable PFSLAM_PARTICLES).
void pfslamSetParticleCount(int n);
// The reference keeps both map representations in the source and wires the point-cloud one (kernel.cu:1730-1745);
// this selects which stages particleFilter() runs: false = KD point cloud (default), true = 2-D occupancy grid
// (PFMeasurementUpdate / PFUpdateMap).  Also: environment variable PFSLAM_MAP=grid.
void pfslamUseGridMap(bool on);
// The reference has UpdateTopology() / CheckLoopClosure() commented out at the end of particleFilter (kernel.cu:1750-1751):
// this enables them there (also: environment variable PFSLAM_TOPOLOGY=1).  pfslamLoopClosures returns the
// (candidate node, visible node) pairs the last frame proposed.
void pfslamUseTopology(bool on);
std::vector<std::pair<int, int>> pfslamLoopClosures();
// PFResample's draw (no reference counterpart; include/pfslam.h, pfslam_set_resampler): 0 = the reference's seeding, 512 distinct draws
// whatever the particle count (default), 1 = one multinomial draw per particle, 2 = systematic resampling.  Read by the next
// particleFilterInit (a live filter takes it from its next frame); a mode outside 0..2 prints and exits like every other error.
void pfslamSetResampler(int mode);
// Posterior of the live filter (no reference counterpart; include/pfslam.h, pfslam_estimate): weighted mean pose (x, y, heading -- a LINEAR
// mean: the filter never wraps headings), row-major symmetric 3x3 covariance and Neff, reduced on the device; like getPCData it first waits
// for the frames in flight.  cov and neff may be null.  false (and a line on stderr): no live filter, or the weights do not sum to a
// positive finite number; the outputs are then untouched.
bool pfslamPoseEstimate(glm::vec3 &mean, float cov[9], float *neff);
// Scan-to-map registration of the live filter's scan against its map (no reference counterpart; include/pfslam.h, pfslam_register): up to
// max_iters ICP iterations on the device from `start`, with exact nearest neighbours, the rejected beams left out, a 0.5 m gate and the
// rigid update (pfslam_register_default_opts; max_iters <= 0 keeps its 40).  Reads the filter, changes nothing in it; like getPCData it
// first waits for the frames in flight.  status: 0 max_iters done, 1 converged, 2 too few pairs, 3 not finite; iterations may be null.
// false (and a line on stderr): no live filter, no map yet, or an option out of range; the outputs are then untouched.
bool pfslamRegister(glm::vec3 start, int max_iters, glm::vec3 &pose, int *status, int *iterations);
// pfslamRegister from m start poses in one launch (include/pfslam.h, pfslam_register_batch): poses[r] and status[r] are what pfslamRegister
// gives from starts[r]; *best is the row the library's rule picks -- the smallest residual among the runs that kept at least half as many
// pairs as the run that kept most -- or -1 when no run completed an iteration.  status and best may be null.  false (and a line on
// stderr): no live filter, no map yet, m outside 1 .. 4096 or an option out of range; the outputs are then untouched.
bool pfslamRegisterBatch(const glm::vec3 *starts, int m, int max_iters, glm::vec3 *poses, int *status, int *best);
// Windowed correlative search of the live filter's scan against its map (no reference counterpart; include/pfslam.h, pfslam_search): every
// pose of the default window (pfslam_search_default_opts: +-20 cells, +-16 heading steps of 0.0125 rad) around `centre` scored against a
// distance field of the map; pose is the best candidate, *index its number (-1: no heading has an in-range beam, pose is the centre).
// Reads the filter, changes nothing in it; like getPCData it first waits for the frames in flight.  index may be null.  false (and a
// line on stderr): no live filter or no map yet; the outputs are then untouched.
bool pfslamSearch(glm::vec3 centre, glm::vec3 &pose, int *index);
// Correlative scan-to-scan search (no reference counterpart; include/pfslam.h, pfslam_search_scan): the default window around `ref_pose`
// scored against a distance field built from the end points of `ref_scan` (1081 ranges) taken at `ref_pose` -- no map is needed.  The scan
// that is searched is `scan` (1081 ranges), or with scan == nullptr the live filter's scan (the last frame's).  pose is the best candidate,
// *index its number (-1: no heading has an in-range beam, pose is ref_pose); pose - ref_pose is the delta pfslamShiftParticles takes.
// Reads the filter, changes nothing in it; like getPCData it first waits for the frames in flight.  index may be null.  false (and a line
// on stderr): no live filter or a null ref_scan; the outputs are then untouched.
bool pfslamSearchScan(const float *ref_scan, glm::vec3 ref_pose, glm::vec3 &pose, int *index, const float *scan = nullptr);
// pfslamSearch / pfslamSearchScan and how well their winner is determined (include/pfslam.h, pfslam_search_cov and pfslam_search_scan_cov):
// the same call and the same pose and *index, and on top cov[16] = the weighted mean pose [0..2], the covariance xx, xy, xtheta, yy, ytheta,
// thetatheta [3..8], the effective number of candidates [9] and the share of the weight on the window's border [13] of the score volume,
// weighted with the likelihood of independent Gaussian beam errors of `sigma` metres (the library's default: 0.2).  false as above, and
// for a sigma that is not finite or not > 0; the outputs are then untouched.
bool pfslamSearchCov(glm::vec3 centre, float sigma, glm::vec3 &pose, float cov[16], int *index);
bool pfslamSearchScanCov(const float *ref_scan, glm::vec3 ref_pose, float sigma, glm::vec3 &pose, float cov[16], int *index, const float *scan = nullptr);
// The odometry hook (include/pfslam.h, pfslam_shift_particles): every particle and the robot's pose += delta.
void pfslamShiftParticles(glm::vec3 delta);
// The odometry motion model (include/pfslam.h, pfslam_move_particles): every particle moves by `delta`, given in the frame of heading
// `ref_theta`, rotated into its own frame, plus Gaussian noise of covariance cov_scale * cov + the floors sigma_xy_min^2 (x, y) and
// sigma_theta_min^2 (heading), drawn per (frame, particle); the robot's pose moves without noise.  cov: the six entries xx, xy, xtheta, yy,
// ytheta, thetatheta -- cov + 3 of pfslamSearchCov / pfslamSearchScanCov, with delta = pose - ref_pose and ref_theta = ref_pose.z of that
// search --, or null for none.  Enqueued behind the frames in flight.  false (and a line on stderr): no live filter, a value that is not
// finite, a negative scale or floor, or a covariance that is not positive semi-definite; nothing has moved then.
bool pfslamMoveParticles(int frame, glm::vec3 delta, const float cov[6], float ref_theta, float sigma_xy_min = 0.0f, float sigma_theta_min = 0.0f,
                         float cov_scale = 1.0f);
// The same winner over a window too large to score candidate by candidate (include/pfslam.h, pfslam_search_wide): +-half_metres in x and
// y at stride 1 (rounded to map cells) and +-half_radians in steps of 0.0125 rad (rounded down) around `centre`, the default max_dist;
// found by branch and bound, exactly.  *index is the exact candidate number (it can pass 2^24, where a float rounds), -1 as above; it
// may be null.  false (and a line on stderr): no live filter, no map yet, or a window beyond the entry point's caps.
bool pfslamSearchWide(glm::vec3 centre, float half_metres, float half_radians, glm::vec3 &pose, long long *index);
// The best candidate of each of the `count` (1 .. 64) best cells of pfslamSearchWide's window (include/pfslam.h, pfslam_search_best; the
// default cells: tiles of 8 x 8 translations, groups of 8 headings): poses[r] and index[r] in ascending key order, row 0 pfslamSearchWide's
// winner -- the starts pfslamRegisterBatch takes when one pose is not enough.  Returns the rows found (fewer than `count` only when fewer
// cells hold a candidate, 0 when no heading has an in-range beam), or -1 (and a line on stderr): no live filter, no map yet, a count or a
// window beyond the entry point's caps; the outputs are then untouched.  index may be null.
int pfslamSearchBest(glm::vec3 centre, float half_metres, float half_radians, int count, glm::vec3 *poses, long long *index);
// The scan the live filter's map predicts from `pose` (no reference counterpart; include/pfslam.h, pfslam_cast, the default options: a
// node with w >= 1 occupies its cell and the eight around it, 30 m): ranges[1081], 30 for a beam that hits nothing; *hits the beams that
// hit.  Reads the filter, changes nothing in it; like getPCData it first waits for the frames in flight.  hits may be null.  false (and a
// line on stderr): no live filter or no map yet; the outputs are then untouched.
bool pfslamCastScan(glm::vec3 pose, float *ranges, int *hits);
// The beam-model score of `m` poses (no reference counterpart; include/pfslam.h, pfslam_cast_score, the default options of the cast and
// of the score): the live filter's scan compared beam by beam with the scan its map predicts from each pose, reduced on the device.
// rows[r * 8 + ..] = valid beams, agree (within 0.1 m), through (the measured beam ends behind a mapped wall), short, valid misses, Q1,
// Q2, cost; *best the row with the smallest cost among those with an agreeing beam, -1 when there is none.  Reads the filter, changes
// nothing in it; like getPCData it first waits for the frames in flight.  best may be null.  false (and a line on stderr): no live
// filter, no map yet or m outside 1 .. 65536; the outputs are then untouched.
bool pfslamCastScore(const glm::vec3 *poses, int m, int *rows /* m x 8 */, int *best);
// Map export for an end-to-end comparison: the point-cloud map as the reference's viewer filters it
// (nodes with w > -100, main.cpp:269-284) -> PREFIX.kd.bin (float x, y, z, w per point, in node order) + PREFIX.kd.csv, and
// the 2-D occupancy grid -> PREFIX.grid.i8 (dim.x * dim.y signed bytes, cell (x, y) at x * dim.x + y) + PREFIX.grid.pgm
// (value + 128, one row per x).  Returns the number of exported points.
int pfslamExportMap(const char *prefix);

// error convention of the reference: print and exit (kernel.h:42-60).  checkCUDAErrorFn(msg, file, line) waits for the device
// (every frame in flight is booked: a deferred error of the frame pipeline surfaces here) and exits on failure.
void checkPfslamErrorFn(int rc, const char *msg, const char *file, int line);
void checkCUDAErrorFn(const char *msg, const char *file, int line);
#define checkCUDAError(msg) checkCUDAErrorFn(msg, __FILE__, __LINE__)
