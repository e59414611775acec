// pfslam_frame.hip.inc -- round 5: the KD frame loop of pfslam_step as FOUR in-order chains with a fixed set of edges between them.
// Included by pfslam_hip.hip behind pfslam_stages.hip.inc (same translation unit).
//
// What the next frame's scan-match kernel waits for is a chain of dependent launches (reference order: kernel.cu:1727-1748):
//     scan-match -> min/max/argmax -> pose = best particle + ICP increment -> new walls of the scan at that pose -> KDTree::InsertNode
//     -> the lattice-cell rows that insert touched -> next scan-match.
// Round 4 ran that chain through seven kernels, three event records and four event waits (0.18 ms between two 0.38 ms scan-match
// kernels).  Here it is SIX launches on one stream with no event between them (0.12-0.14 ms):
//
//   C (chain)      [gate ORDER]  k_score_kd_cells -> k_reduce_groups -> k_wall_runs (stores REDUCED, spins for ICP; the frame's pose from
//                  the keys; the scan's wall cells at that pose, sorted in runs) -> k_walls_rank_traverse -> k_walls<3> (new-wall test,
//                  KDTree::InsertNode for all of them) -> k_cells_update<true> (stores TREE)
//   P (particles)  scan upload, k_motion_count -> k_cell_scan -> k_cell_scatter  [wait ev_ftail of the previous frame]  [signal ORDER]  |
//                  [gate REDUCED]  [wait ev_marked, ev_walked of earlier frames]  k_weights_tiles -> k_scan_apply2 (sums, Neff, header part A)
//                  -> k_sample_gather
//   F (free cells) [gate ORDER]  k_icp_fused (stores ICP)  [gate REDUCED]  k_get_walls -> k_count_cells -> k_scatter_cells -> k_free_traverse
//                  (the -1 pass of kernUpdateMapKD on the tree AS IT WAS before this frame's insert: kd_resume<BOUNDED>)  [gate TREE]
//                  k_wall_weights (the +4 pass, behind the -1 pass as in the reference; header part B)  [record ev_ftail]
//   K (cells)      [gate ORDER]  k_group_box -> k_cells_mark  [record ev_marked]  [gate TREE of the previous frame]  k_cells_update<false>
//                  (bounded walk of the new cells)  [record ev_walked]
//
// An edge is a GATE -- a word in device memory the producer stream's next kernel stores the frame's ticket into, a one-wave kernel that
// spins on it on the consumer stream (k_gate below says why) -- or, when the handle's streams do not make progress independently, an
// event.  Every buffer two chains share and what orders it: DESIGN.md section 5.  PFSLAM_SERIAL=1 (and every frame that wipes the cell
// rows, re-balances or times its phases) runs the very same launches, in the order they are enqueued here, on ONE stream: results AND
// bookkeeping (claimed cells, records, pool slots, extensions) are the same by construction -- tests/test_gpu_frame.py asserts it.
// (Tried and dropped: the ICP solve straight behind the previous frame's free-cell chain instead of behind the lane order -- no gain
// at any particle count, one more event; its first version forgot that the previous frame may have run on ONE stream and raced it.)

#define PF_FRAME_RING 4 /* per-frame device words and events are kept for this many tickets (frames in flight <= PF_MAX_LAG + 1) */
// frame state (ints), device side: fs[PF_FS_BOUND + s] = nodes of the tree before the insert of the frame with ticket & 3 == s (what the
// frame's bounded passes may see); fs[PF_FS_WALKED + s] = records walked when that frame's walk pass started (a later publishing pass
// takes records below it); fs[PF_FS_TICKET] = arrival counter of k_reduce_groups; fs[PF_FS_ICP] = ... of k_icp_fused
enum { PF_FS_BOUND = 0, PF_FS_WALKED = 4, PF_FS_TICKET = 8, PF_FS_ICP = 9, PF_FS_WORDS = 16 };
// wall-chain counts (ints), written by k_walls: [0] wall cells  [1] new walls  [2] header flags  [3] map size after the insert
enum { PF_WC_WALLS = 0, PF_WC_NEW, PF_WC_FLAGS, PF_WC_SIZE, PF_WC_WORDS = 4 };

// ---- stream gates (PFSLAM_GATES=1) ------------------------------------------------------------------------------------------------------
// An event between two kernels of a stream is expensive on this runtime: the launch behind a hipEventRecord starts ~13 us after its
// predecessor ended (4 us without the record), and a launch behind a hipStreamWaitEvent on an event that fired long ago as late -- four of
// them sat on the frame's critical chain (40 of its 143 us).  A gate does the same job through a word in device memory: the producer
// stream's NEXT kernel stores the frame's ticket in front of its own work (a kernel boundary has then made everything before it visible
// to the device), the consumer stream runs a one-wave kernel that spins until the word has reached the ticket (the launch behind it starts
// with the usual acquire).  Tickets only grow, so nothing is ever reset.  A gate gives up after a second (a minute in a multi-GPU job, where
// it may wait for a peer: g_gate_ticks) and says so in pinned memory
// (the call that books the frame fails).  Gates are only used when pfslam_create's self-test has seen the handle's four streams make
// progress independently of one another (two streams on one hardware queue would make a gate wait for work queued behind itself).
enum { PF_FL_REDUCED = 0, PF_FL_TREE, PF_FL_ORDER, PF_FL_ICP, PF_FL_SCAN, PF_FL_FTAIL, PF_FL_POSEG /* sharded: the gathered pose blocks are there */, PF_FL_WORDS = 8 };
__device__ __forceinline__ void flag_store(int *word, int ticket) { __hip_atomic_store(word, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool flag_wait(const int *word, int ticket, int *err)
{
    const unsigned long long t0 = wall_clock64(), limit = g_gate_ticks;
    while (__hip_atomic_load(word, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - ticket < 0) {
        __builtin_amdgcn_s_sleep(8);
        if (wall_clock64() - t0 > limit) { // 1 s at 100 MHz (60 s for a shard of a multi-GPU job: pfslam_create)
            if (err) __hip_atomic_store(err, ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return false;
        }
    }
    return true;
}
__global__ void k_gate(const int *__restrict__ word, int ticket, int *__restrict__ err)
{
    if (threadIdx.x == 0) flag_wait(word, ticket, err);
}
// a gate that first says that its own stream has got this far (everything enqueued in front of it is done): the free-cell stream's first
// launch of a frame announces the previous frame's tail this way -- an event recorded behind k_wall_weights cost the particle stream's
// wait for it (and with it the lane order, the one thing the next scan-match kernel waits for) ~8 us at 1000 / 10 000 particles
__global__ void k_gate_signal(int *__restrict__ done_word, int done_ticket, const int *__restrict__ word, int ticket, int *__restrict__ err)
{
    if (threadIdx.x != 0) return;
    flag_store(done_word, done_ticket);
    flag_wait(word, ticket, err);
}
// self-test: a gate that gives up after `ticks` (100 MHz) and reports whether it saw the word arrive
__global__ void k_gate_test(const int *__restrict__ word, int ticket, unsigned long long ticks, int *__restrict__ ok)
{
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = wall_clock64();
    int seen = 0;
    while (!(seen = (__hip_atomic_load(word, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - ticket >= 0)) && wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
    // (seen, but only after 0.2 ms: the signal's queue was not served while this one spun -- time-sliced hardware queues are no better than shared ones)
    *ok = seen && wall_clock64() - t0 < 20000ull;
}
__global__ void k_signal(int *__restrict__ word, int ticket)
{
    if (threadIdx.x == 0) flag_store(word, ticket);
}

// ---- C: beam-chunk partials -> scores, packed min / max keys, best pose ------------------------------------------------------------
// The scan-match kernel leaves its 16-bit partials group-major ([group][chunk][lane], out_mode 4): one wave reads a group's
// `chunks` x 128 bytes as 16-byte pieces of one contiguous run -- piece q holds chunk q / 8, lanes 8 (q & 7) .. + 7 -- so lane l only
// ever adds into the eight slots 8 (l & 7) + j, three xor steps (8, 16, 32) finish the sums, eight more shuffles hand lane l slot l.
// Integer sums: exact in any order (that is what 16-bit partials require in the first place).  17.6 us -> ~6 us for 100 k particles x 84
// chunks.  SPLIT = 4: the four waves of a workgroup share ONE group (few particles, up to 1081 chunks).
// The frame's pose -- best particle + ICP increment (kernel.cu:1081-1092) -- is formed from the max key by every kernel that needs it
// (frame_pose; k_walls stores it and resets the keys of the NEXT frame): no k_best_pose, no k_stats_reset launch on the chain.  (A last-
// workgroup ticket in here was tried first: its agent-scope fence costs ~33 ns PER WORKGROUP, one after the other -- 13 us with 391
// workgroups, 50 us with 1563.)
#define PF_REDUCE_WGS 128
template <int SPLIT>
__global__ __launch_bounds__(256) void k_reduce_groups(const short *__restrict__ pg, int n, int groups, int chunks, const int *__restrict__ order,
                                                       float *__restrict__ fit, long long *__restrict__ stats, unsigned long long *__restrict__ probe, int goff)
{
    pf_stamp(probe);
    __shared__ int s_part[4][64];
    __shared__ long long smax[4], smin[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long kmax = LLONG_MIN, kmin = LLONG_MIN;
    // SPLIT == 1: a workgroup takes every gridDim.x-th quadruple of groups (a grid of at most PF_REDUCE_WGS workgroups).  One workgroup per
    // quadruple ended with 2 x 391 atomics on the two keys' cache line within a microsecond at 100 k particles; they are applied one after the
    // other (~16 ns each) and the next launch of the stream waited ~9 us for them -- longer than the kernel's own 4 us.
    for (int gq = blockIdx.x; SPLIT == 1 ? gq * 4 < groups : gq == (int)blockIdx.x; gq += gridDim.x) {
    const int g = SPLIT == 1 ? gq * 4 + wave : gq;
    int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (g < groups) {
        const uint4 *src = (const uint4 *)(pg + (size_t)g * chunks * 64);
        const int npiece = chunks * 8;
        // twelve 16-byte loads per lane in flight at a time (84 chunks are 10.5 per lane: one batch; with four at a time the kernel took
        // three trips to memory one after the other)
        for (int q0 = lane + (SPLIT == 1 ? 0 : 64 * wave); q0 < npiece; q0 += 12 * 64 * SPLIT) {
            uint4 v[12];
#pragma unroll
            for (int k = 0; k < 12; k++) {
                const int q = q0 + k * 64 * SPLIT;
                v[k] = q < npiece ? src[q] : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int k = 0; k < 12; k++) {
                acc[0] += (int)(short)(v[k].x & 0xffffu); acc[1] += (int)(short)(v[k].x >> 16);
                acc[2] += (int)(short)(v[k].y & 0xffffu); acc[3] += (int)(short)(v[k].y >> 16);
                acc[4] += (int)(short)(v[k].z & 0xffffu); acc[5] += (int)(short)(v[k].z >> 16);
                acc[6] += (int)(short)(v[k].w & 0xffffu); acc[7] += (int)(short)(v[k].w >> 16);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        acc[j] += __shfl_xor(acc[j], 8, 64);
        acc[j] += __shfl_xor(acc[j], 16, 64);
        acc[j] += __shfl_xor(acc[j], 32, 64);
    }
    int v = 0; // slot `lane` of the group: element lane & 7 of any lane whose low three bits are lane >> 3
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int t = __shfl(acc[j], lane >> 3, 64);
        v = (lane & 7) == j ? t : v;
    }
    if (SPLIT != 1) {
        s_part[wave][lane] = v;
        __syncthreads();
        v = (s_part[0][lane] + s_part[1][lane]) + (s_part[2][lane] + s_part[3][lane]);
    }
    const int slot = g * 64 + lane;
    if (g < groups && slot < n && (SPLIT == 1 || wave == 0)) {
        const float a = (float)v; // |sum| <= n_beams x largest |weight| <= 2^24 (upload_tree)
        const int i = order ? order[slot] : slot;
        fit[i] = a;
        const long long k1 = ((long long)f32_to_ordered(a) << 32) | (long long)(0xFFFFFFFFu - (uint32_t)(goff + i)); // (the GLOBAL index: a shard's keys merge with the other ranks')
        const long long k2 = ((long long)f32_to_ordered(-a) << 32);
        kmax = k1 > kmax ? k1 : kmax;
        kmin = k2 > kmin ? k2 : kmin;
    }
    }
    kmax = wave_max_i64(kmax);
    kmin = wave_max_i64(kmin);
    if (lane == 0) {
        smax[wave] = kmax;
        smin[wave] = kmin;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < 4; k++) {
        kmax = smax[k] > kmax ? smax[k] : kmax;
        kmin = smin[k] > kmin ? smin[k] : kmin;
    }
    atomicMax(&stats[0], kmax);
    atomicMax(&stats[1], kmin);
    if (probe) atomicMax(probe + (PB_REDUCE_END - PB_REDUCE), (unsigned long long)wall_clock64());
}

// ---- C: the wall half of PFUpdateMapKD (kernel.cu:1406-1540) in ONE workgroup --------------------------------------------------------
// The scan has at most one wall cell per beam (kernGetWalls, kernel.cu:524-549), and what the next scan-match kernel waits for -- the
// insert of the frame's new walls and the cell rows behind it -- needs the WALL list only.  So: wall cell of every beam at the frame's
// pose (the very expressions of k_get_walls), a bitonic sort of the <= 4096 cell indices in LDS + duplicates dropped (= the x-major
// order the reference's double loop over the local grid produces, kernel.cu:1435-1461; k_scatter_cells makes the same list from the
// mask on the free-cell stream, k_wall_weights checks that the two agree), cell_to_point, the whole traversal of every wall
// (findCorrespondenceIndexKD, kernel.cu:924-972: nearest index + the link its first descent falls off), kernTestCorrespondance
// (kernel.cu:1367-1379), ordered compaction, KDTree::InsertNode for the new walls in list order (k_test_new's rounds).  The weight
// passes of kernUpdateMapKD are NOT here: the walls' +4 has to follow the free cells' -1 (clamping does not commute), both ride on the
// free-cell stream (k_free_traverse, k_wall_weights).
// PART 0: all of it in one launch (trees that are not planar).  PART 3: test + insert (one workgroup) behind k_wall_runs and
// k_walls_rank_traverse, which spread the ranking and the traversals over many compute units: 1081 traversals of ~50 visits each are
// ISSUE-bound on one compute unit (30 us; a second pass over the very same, now cached, nodes still took 25), not latency-bound.
template <int PART>
__global__ __launch_bounds__(1024) void k_walls(const float *__restrict__ scan, const pf::BeamParts *__restrict__ beams, int nb, int sort_n,
                                               PoseSrc src, float *__restrict__ start_out, float *__restrict__ pose_out, long long *__restrict__ stats_next,
                                               int cx, int cy,
                                               int dimx, int dimy, float resx, float resy, float scalex, float scaley, pf::KdView tree,
                                               uint4 *hot, int *parent, float *kz, float *kw, int *__restrict__ kd_state, int kd_cap, int cap,
                                               int *__restrict__ wall_c2, int *__restrict__ wcounts, int *__restrict__ bound_next,
                                               const int *__restrict__ cell_state, int *__restrict__ touched, unsigned long long *__restrict__ probe,
                                               float2 *__restrict__ wall_xy2, int *__restrict__ wall_leaf2, int *__restrict__ wall_new2,
                                               int *__restrict__ flags, int ticket, int *__restrict__ gate_err,
                                               const uint32_t *__restrict__ keys_s = nullptr, const int *__restrict__ c2_s = nullptr, int wait_poseg = 0,
                                               int trig = 0)
{
    if (PART != 3) pf_stamp(probe);
    if (flags && PART != 3) { // stream gates: the reduce in front of this launch is done (say so); the ICP increment must be there (wait for it)
        if (threadIdx.x == 0) {
            flag_store(flags + PF_FL_REDUCED, ticket);
            flag_wait(flags + PF_FL_ICP, ticket, gate_err);
            if (wait_poseg) flag_wait(flags + PF_FL_POSEG, ticket, gate_err); // (sharded: the best particle's pose is read out of the gathered blocks)
        }
        __syncthreads();
    }
    // LDS (9 x cap words; cap = the beams rounded up to whole waves): the new walls as nodes {x, y, z, left, right, parent, axis, cursor}
    // (k_test_new) + one flag per wall.  Earlier phases borrow what is still dead: the sorted runs live in parent + axis, the sorted
    // keys in `left`, the ordered wall cells in `right`; a wall's point and the link it falls off ARE its x / y / cursor entries until
    // the compaction moves the new walls to the front (position o <= i, every thread reads its own entries before the barrier and
    // writes behind it).
    extern __shared__ uint32_t s_dyn[];
    float *lx = (float *)s_dyn, *ly = lx + cap, *lz = ly + cap;
    uint32_t *ll = (uint32_t *)(lz + cap), *lr = ll + cap;
    int *lpar = (int *)(lr + cap), *lax = lpar + cap, *lcur = lax + cap;
    int *wnew = lcur + cap;
    uint32_t *runs = (uint32_t *)lpar, *keys = ll;
    int *wcell = (int *)lr;
    __shared__ int swave[16];
    __shared__ int sbase;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float ps[3], st[3];
    frame_pose(src, st, ps);
    const float px = ps[0], py = ps[1], pt = ps[2];
    if (threadIdx.x == 0 && PART != 3) { // the frame's pose for everybody behind this kernel; the other ticket parity's keys start over
        for (int k = 0; k < 3; k++) { start_out[k] = st[k]; pose_out[k] = ps[k]; }
        start_out[3] = 0.0f;
        pose_out[3] = 0.0f;
        stats_next[0] = LLONG_MIN;
        stats_next[1] = LLONG_MIN;
    }
    const pf::AngleParts T = pf::angle_parts(pt);
    const int n_runs = sort_n >> 6; // sort_n = cap: whole waves
    int n = 0;
    const float cellDiag = pf::fsqrt(resx * resx + resy * resy), minDist = cellDiag / 2.0f;
    if (PART != 3) {
    // 1. the wall cell of every beam (k_get_walls), 2a. sorted inside its run of 64 (a wave's own bitonic network: no barrier)
    for (int r = wave; r < n_runs; r += 16) {
        const int j = r * 64 + lane;
        uint32_t key = 0xFFFFFFFFu;
        if (j < nb) {
            float wx, wy;
            beam_end_point_rt(beams, j, scan[j], pt, T, wx, wy, trig); // (= pf::clean_lidar_scan: the beam's parts from the table)
            if (fabsf(wx) < PF_LIDAR_RANGE && fabsf(wy) < PF_LIDAR_RANGE) {
                wx = roundf(pf::fdiv(wx, resx));
                wy = roundf(pf::fdiv(wy, resy));
                wx += (float)cx;
                wy += (float)cy;
                if (wx >= 0 && wx < dimx && wy >= 0 && wy < dimy) key = (uint32_t)(int)(wx * dimx + wy);
            }
        }
#pragma unroll
        for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
            for (int q = k >> 1; q > 0; q >>= 1) {
                const uint32_t other = (uint32_t)__shfl_xor((int)key, q, 64);
                const bool asc = (lane & k) == 0, lower = (lane & q) == 0;
                key = (lower == asc) ? min(key, other) : max(key, other);
            }
        runs[j] = key;
        keys[j] = 0xFFFFFFFFu;
    }
    __syncthreads();
    if (probe && threadIdx.x == 0) probe[PB_WALLS_KEYS - PB_WALLS] = wall_clock64();
    // 2b. a key's place among all of them: its place in its own run + what the other runs hold below it (binary searches; equal keys
    // are the same cell: any consistent order among them will do -- earlier runs count their equals, later ones do not)
    for (int i = threadIdx.x; i < sort_n; i += 1024) {
        const uint32_t key = runs[i];
        if (key == 0xFFFFFFFFu) continue;
        const int mine = i >> 6;
        int rank = i & 63;
        // (four runs' searches side by side: each is a chain of seven dependent LDS reads)
        for (int r0 = 0; r0 < n_runs; r0 += 4) {
            int lo[4] = {0, 0, 0, 0};
            uint32_t pk[4];
            bool on[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int r = r0 + u;
                on[u] = r < n_runs && r != mine && !(r > mine && key == 0u);
                pk[u] = r < mine ? key : key - 1u; // count of elements <= pk (a later run does not count its equals)
            }
#pragma unroll
            for (int step = 32; step >= 1; step >>= 1)
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (on[u]) lo[u] += (runs[(r0 + u) * 64 + lo[u] + step - 1] <= pk[u]) ? step : 0;
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (on[u]) rank += lo[u] + ((lo[u] == 63 && runs[(r0 + u) * 64 + 63] <= pk[u]) ? 1 : 0);
        }
        keys[rank] = key;
    }
    __syncthreads();
    // 3. duplicates dropped, order kept
    if (probe && threadIdx.x == 0) probe[PB_WALLS_SORTED - PB_WALLS] = wall_clock64();
    if (threadIdx.x == 0) sbase = 0;
    __syncthreads();
    for (int r0 = 0; r0 < sort_n; r0 += 1024) {
        const int i = r0 + threadIdx.x;
        const bool flag = i < sort_n && keys[i] != 0xFFFFFFFFu && (i == 0 || keys[i - 1] != keys[i]);
        const unsigned long long m = __ballot(flag);
        if (lane == 0) swave[wave] = __popcll(m);
        __syncthreads();
        int off = sbase;
        for (int k = 0; k < wave; k++) off += swave[k];
        if (flag) wcell[off + __popcll(m & ((1ull << lane) - 1ull))] = (int)keys[i];
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (int k = 0; k < 16; k++) tot += swave[k];
            sbase += tot;
        }
        __syncthreads();
    }
    n = sbase; // <= nb <= cap
    }
    // 4. every wall's traversal: nearest index (for the +4 pass and the test) and the link InsertNode would hang it on
    if (PART == 0) {
        for (int i = threadIdx.x; i < n; i += 1024) {
            const float4 p = cell_to_point(wcell[i], dimx, resx, resy, scalex, scaley, px, py);
            int leaf, b;
            if (tree.planar) b = pf::kd_resume<true, false, true>(tree, p.x, p.y, p.z, INFINITY, 0, 0, nullptr, &leaf);
            else b = pf::kd_resume<false, false, true>(tree, p.x, p.y, p.z, INFINITY, 0, 0, nullptr, &leaf);
            wall_c2[i] = b;
            const float d = node_dist(tree, b, p);
            lx[i] = p.x;
            ly[i] = p.y;
            lcur[i] = leaf;
            wnew[i] = d > minDist ? 1 : 0; // kernTestCorrespondance: a new wall
        }
    } else { // PART 3 behind k_walls_rank_traverse: the walls sit at their ranks, duplicates and beams without a wall are empty places
        if (threadIdx.x == 0) sbase = 0;
        __syncthreads();
        for (int r0 = 0; r0 < sort_n; r0 += 1024) {
            const int i = r0 + threadIdx.x;
            const bool flag = i < sort_n && keys_s[i] != 0xFFFFFFFFu;
            const float2 p = flag ? wall_xy2[i] : make_float2(0.0f, 0.0f);
            const int vleaf = flag ? wall_leaf2[i] : 0, vnew = flag ? wall_new2[i] : 0, vb = flag ? c2_s[i] : 0;
            const unsigned long long m = __ballot(flag);
            if (lane == 0) swave[wave] = __popcll(m);
            __syncthreads();
            int off = sbase;
            for (int k = 0; k < wave; k++) off += swave[k];
            if (flag) {
                const int o = off + __popcll(m & ((1ull << lane) - 1ull));
                lx[o] = p.x;
                ly[o] = p.y;
                lcur[o] = vleaf;
                wnew[o] = vnew;
                wall_c2[o] = vb; // (the +4 pass of the free-cell stream reads the list in this order)
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int tot = 0;
                for (int k = 0; k < 16; k++) tot += swave[k];
                sbase += tot;
            }
            __syncthreads();
        }
        n = sbase;
    }
    __syncthreads();
    if (probe && threadIdx.x == 0) probe[PB_WALLS_TRAV - PB_WALLS] = wall_clock64();
    // 5. the new walls to the front, order kept: from here on they are LDS-resident nodes
    if (threadIdx.x == 0) sbase = 0;
    __syncthreads();
    for (int r0 = 0; r0 < n; r0 += 1024) {
        const int i = r0 + threadIdx.x;
        const bool flag = i < n && wnew[i] != 0;
        const float vx = flag ? lx[i] : 0.0f, vy = flag ? ly[i] : 0.0f;
        const int vleaf = flag ? lcur[i] : 0;
        const unsigned long long m = __ballot(flag);
        if (lane == 0) swave[wave] = __popcll(m);
        __syncthreads();
        int off = sbase;
        for (int k = 0; k < wave; k++) off += swave[k];
        if (flag) {
            const int o = off + __popcll(m & ((1ull << lane) - 1ull));
            lx[o] = vx;
            ly[o] = vy;
            lz[o] = 0.0f;
            ll[o] = PF_KD_NULL;
            lr[o] = PF_KD_NULL;
            lcur[o] = vleaf;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (int k = 0; k < 16; k++) tot += swave[k];
            sbase += tot;
        }
        __syncthreads();
    }
    const int n_new = sbase, old = kd_state[0];
    const bool full = n_new > kd_cap - old;
    const int n_ins = full ? 0 : n_new;
    __shared__ int s_touched;
    if (threadIdx.x == 0) s_touched = 0;
    __syncthreads();
    if (n_ins > 0) { // block-uniform: KDTree::InsertNode for all of them (k_test_new has the argument)
        uint32_t *hw = (uint32_t *)hot;
        const bool planar = tree.planar != 0;
        for (int k = threadIdx.x; k < n_ins; k += 1024) { // round 1: the links of the existing tree
            const int at = lcur[k] >> 1, right = lcur[k] & 1;
            const uint32_t cand = (uint32_t)(old + k), axis = ld_agent(&hw[4 * at + 2]) >> 30;
            if (right) {
                atomicMin(&hw[4 * at + 3], cand);
                if (planar && axis == 2) atomicMin(&hw[4 * at + 2], cand | (2u << 30));
            } else {
                atomicMin(&hw[4 * at + 2], cand | (axis << 30));
            }
        }
        __threadfence();
        __syncthreads();
        int pend = 0;
        for (int k = threadIdx.x; k < n_ins; k += 1024) {
            const int at = lcur[k] >> 1, right = lcur[k] & 1;
            const uint32_t la = ld_agent(&hw[4 * at + 2]);
            const uint32_t link = right ? ld_agent(&hw[4 * at + 3]) : (la & 0x3fffffffu);
            if (link == (uint32_t)(old + k)) {
                if (touched) touched[1 + atomicAdd(&s_touched, 1)] = at * 2 + right;
                lpar[k] = at;
                lax[k] = (int)((la >> 30) + 1u) % 3;
                lcur[k] = -1;
            } else {
                lcur[k] = (int)link - old;
                pend = 1;
            }
        }
        pend = __syncthreads_or(pend);
        while (pend) { // rounds 2..: among the new nodes, in LDS
            for (int k = threadIdx.x; k < n_ins; k += 1024) {
                int a = lcur[k];
                if (a < 0) continue;
                uint32_t *lnk;
                for (;;) {
                    const int ax = lax[a];
                    const float key = ax == 0 ? lx[a] : ax == 1 ? ly[a] : lz[a];
                    const float pv = ax == 0 ? lx[k] : ax == 1 ? ly[k] : lz[k];
                    lnk = pv < key ? &ll[a] : &lr[a];
                    const uint32_t v = *(volatile uint32_t *)lnk;
                    if (v >= PF_KD_TAG) break;
                    a = (int)v;
                }
                atomicMin(lnk, (uint32_t)k | PF_KD_TAG);
                lcur[k] = a * 2 + (lnk == &lr[a] ? 1 : 0);
            }
            __syncthreads();
            pend = 0;
            for (int k = threadIdx.x; k < n_ins; k += 1024) {
                if (lcur[k] < 0) continue;
                const int a = lcur[k] >> 1;
                uint32_t *lnk = (lcur[k] & 1) ? &lr[a] : &ll[a];
                const uint32_t w = *(volatile uint32_t *)lnk & ~PF_KD_TAG;
                if (w == (uint32_t)k) {
                    *(volatile uint32_t *)lnk = (uint32_t)k;
                    lpar[k] = old + a;
                    lax[k] = (lax[a] + 1) % 3;
                    lcur[k] = -1;
                } else {
                    lcur[k] = (int)w;
                    pend = 1;
                }
            }
            pend = __syncthreads_or(pend);
        }
        for (int k = threadIdx.x; k < n_ins; k += 1024) {
            const int g = old + k, ax = lax[k];
            const int left = ll[k] == PF_KD_NULL ? -1 : old + (int)ll[k], right = lr[k] == PF_KD_NULL ? -1 : old + (int)lr[k];
            hot[g] = pf::pack_hot(lx[k], ly[k], ax, left, right, planar);
            parent[g] = lpar[k];
            kz[g] = (planar && ax == 2) ? __int_as_float(left) : lz[k];
            kw[g] = -100.0f; // kernel.cu:1514
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (touched) touched[0] = s_touched;
        const int cf = cell_state ? cell_state[PF_CS_FLAGS] : 0;
        const int cflag = ((cf & PF_CF_FAR) ? PF_HDR_CELLS_WIPE : 0) | ((cf & (PF_CF_LIST_FULL | PF_CF_POOL_FULL)) ? PF_HDR_CELLS_FULL : 0);
        wcounts[PF_WC_WALLS] = n;
        wcounts[PF_WC_NEW] = n_new;
        wcounts[PF_WC_FLAGS] = (full ? PF_HDR_KD_FULL : 0) | cflag;
        wcounts[PF_WC_SIZE] = old + n_ins;
        kd_state[0] = old + n_ins;
        *bound_next = old + n_ins; // what the NEXT frame's bounded passes may see
        if (probe) probe[PB_WALLS_END - PB_WALLS] = wall_clock64();
    }
}

// ---- the wall list over MANY compute units (round 5, second half) --------------------------------------------------------------------
// k_walls<0> ranks every wall cell among all of them on ONE compute unit: 1088 keys x 17 runs x 7 dependent LDS reads, sixteen waves
// on four SIMDs -- 12 us of instruction issue on the frame's critical chain.  The same work in three pieces:
//   k_wall_runs           one wave per run of 64 beams: the frame's pose, the beams' wall cells, the wave's own bitonic network; the
//                         sorted run goes to memory (4 bytes per beam).  Block 0 speaks for the frame (REDUCED, pose, key reset).
//   k_walls_rank_traverse one wave per run, on a compute unit of its own: all runs into LDS, its 64 keys ranked among all of them (the
//                         very searches of k_walls<0>: 17 waves side by side instead of in turns), duplicates flagged -- an equal key
//                         in an earlier run or at an earlier place of its own run: the instance k_walls<0>'s pass would have kept --,
//                         and the wall's whole traversal; everything is written at the key's RANK.
//   k_walls<3>            drops the flagged places while it loads the list (ordered compaction: the x-major unique list of the
//                         reference's double loop, kernel.cu:1435-1461) and goes on as before.
__global__ __launch_bounds__(64) void k_wall_runs(const float *__restrict__ scan, const pf::BeamParts *__restrict__ beams, int nb, PoseSrc src,
                                                  float *__restrict__ start_out, float *__restrict__ pose_out, long long *__restrict__ stats_next, int cx,
                                                  int cy, int dimx, int dimy, float resx, float resy, uint32_t *__restrict__ runs_g,
                                                  uint32_t *__restrict__ keys_s, unsigned long long *__restrict__ probe, int *__restrict__ flags, int ticket,
                                                  int *__restrict__ gate_err, int wait_poseg, int trig)
{
    pf_stamp(probe);
    const int lane = threadIdx.x;
    if (flags) { // stream gates: the reduce in front of this launch is done (block 0 says so); the ICP increment must be there (every wave waits)
        if (lane == 0) {
            if (blockIdx.x == 0) flag_store(flags + PF_FL_REDUCED, ticket);
            flag_wait(flags + PF_FL_ICP, ticket, gate_err);
            if (wait_poseg) flag_wait(flags + PF_FL_POSEG, ticket, gate_err); // (sharded: the best particle's pose is read out of the gathered blocks)
        }
        __syncthreads();
    }
    float ps[3], st[3];
    frame_pose(src, st, ps);
    if (blockIdx.x == 0 && lane == 0) { // the frame's pose for everybody behind this kernel; the other ticket parity's keys start over
        for (int k = 0; k < 3; k++) { start_out[k] = st[k]; pose_out[k] = ps[k]; }
        start_out[3] = 0.0f;
        pose_out[3] = 0.0f;
        stats_next[0] = LLONG_MIN;
        stats_next[1] = LLONG_MIN;
    }
    const float pt = ps[2];
    const pf::AngleParts T = pf::angle_parts(pt);
    const int j = blockIdx.x * 64 + lane;
    uint32_t key = 0xFFFFFFFFu;
    if (j < nb) {
        float wx, wy;
        beam_end_point_rt(beams, j, scan[j], pt, T, wx, wy, trig);
        if (fabsf(wx) < PF_LIDAR_RANGE && fabsf(wy) < PF_LIDAR_RANGE) {
            wx = roundf(pf::fdiv(wx, resx));
            wy = roundf(pf::fdiv(wy, resy));
            wx += (float)cx;
            wy += (float)cy;
            if (wx >= 0 && wx < dimx && wy >= 0 && wy < dimy) key = (uint32_t)(int)(wx * dimx + wy);
        }
    }
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
        for (int q = k >> 1; q > 0; q >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)key, q, 64);
            const bool asc = (lane & k) == 0, lower = (lane & q) == 0;
            key = (lower == asc) ? min(key, other) : max(key, other);
        }
    runs_g[j] = key;
    keys_s[j] = 0xFFFFFFFFu; // (a place no key's rank names stays empty)
    if (probe && blockIdx.x == 0 && lane == 0) probe[PB_WALLS_KEYS - PB_WALLS] = wall_clock64();
}

template <bool PLANAR>
__global__ __launch_bounds__(64) void k_walls_rank_traverse(const uint32_t *__restrict__ runs_g, int sort_n, const float *__restrict__ pose, int dimx, float resx,
                                                            float resy, float scalex, float scaley, pf::KdView tree, uint32_t *__restrict__ keys_s,
                                                            float2 *__restrict__ xy_s, int *__restrict__ c2_s, int *__restrict__ leaf_s,
                                                            int *__restrict__ new_s, unsigned long long *__restrict__ probe, int split)
{
    pf_stamp(probe);
    extern __shared__ uint32_t s_dyn[];
    uint32_t *runs = s_dyn;
    // split (1, 2, 4): a run's 64 keys over that many workgroups, 64 / split lanes of each at work.  A wave's traversals take as many rounds
    // (descent, parent test, re-descent) as its slowest lane's, every round as long as its deepest descent: fewer walls per wave, shorter waves.
    const int lane = threadIdx.x, n_runs = sort_n >> 6, mine = blockIdx.x / split, per = 64 / split, pos = (blockIdx.x % split) * per + lane;
    for (int i = lane; i < sort_n; i += 64) runs[i] = runs_g[i];
    __syncthreads();
    if (lane >= per) return;
    const int i = mine * 64 + pos;
    const uint32_t key = runs[i];
    if (key == 0xFFFFFFFFu) return; // no wall cell for this beam (the empty keys sort behind every real one: no rank counts them)
    int rank = pos;
    bool dup = pos > 0 && runs[i - 1] == key;
    for (int r0 = 0; r0 < n_runs; r0 += 4) { // (k_walls<0>'s searches, word for word: four runs side by side)
        int lo[4] = {0, 0, 0, 0};
        uint32_t pk[4];
        bool on[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int r = r0 + u;
            on[u] = r < n_runs && r != mine && !(r > mine && key == 0u);
            pk[u] = r < mine ? key : key - 1u; // count of elements <= pk (a later run does not count its equals)
        }
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1)
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (on[u]) lo[u] += (runs[(r0 + u) * 64 + lo[u] + step - 1] <= pk[u]) ? step : 0;
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (on[u]) {
                const int cnt = lo[u] + ((lo[u] == 63 && runs[(r0 + u) * 64 + 63] <= pk[u]) ? 1 : 0);
                rank += cnt;
                if (r0 + u < mine && cnt > 0 && runs[(r0 + u) * 64 + cnt - 1] == key) dup = true; // an earlier run holds this cell
            }
    }
    if (dup) return; // (its place stays empty)
    const float4 p = cell_to_point((int)key, dimx, resx, resy, scalex, scaley, pose[0], pose[1]);
    int leaf;
    const int b = pf::kd_resume<PLANAR, false, true>(tree, p.x, p.y, p.z, INFINITY, 0, 0, nullptr, &leaf);
    const float cellDiag = pf::fsqrt(resx * resx + resy * resy), minDist = cellDiag / 2.0f;
    keys_s[rank] = key;
    xy_s[rank] = make_float2(p.x, p.y);
    c2_s[rank] = b;
    leaf_s[rank] = leaf;
    new_s[rank] = node_dist(tree, b, p) > minDist ? 1 : 0;
}

// ---- F: the free cells' pass of kernUpdateMapKD on the tree as it was before the frame's insert --------------------------------------
template <bool PLANAR>
__global__ __launch_bounds__(256) void k_free_traverse(float4 *__restrict__ free_pts, int *__restrict__ free_idx, int free_cap, int wall_cap,
                                                       const int *__restrict__ counts, pf::KdView tree, int zero_tail, float *kw, float resx,
                                                       float resy, const int *__restrict__ bound_ptr, unsigned long long *__restrict__ probe)
{
    pf_stamp(probe);
    const int n_wall = min(counts[0], wall_cap), n_free = min(counts[1], free_cap);
    const int bound = *bound_ptr;
    const float cellDiag = pf::fsqrt(resx * resx + resy * resy);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_free; i += gridDim.x * 256) {
        float4 p = free_pts[i];
        if (zero_tail && i >= n_wall) {
            p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            free_pts[i] = p;
        }
        const int b = pf::kd_resume<PLANAR, false, false, true>(tree, p.x, p.y, p.z, INFINITY, 0, 0, nullptr, nullptr, bound);
        free_idx[i] = b;
        const bool hit = node_dist(tree, b, p) < cellDiag;
        if (zero_tail && i >= n_wall) { // H6: one compare-and-swap per wave (k_list_traverse has the argument)
            const unsigned long long m = __ballot(hit);
            if (hit && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) map_weight_add(kw, b, PF_FREE_WEIGHT, __popcll(m));
        } else if (hit) map_weight_add(kw, b, PF_FREE_WEIGHT);
    }
}

// ---- F: the walls' +4 (behind the free cells' -1, as in the reference) and the part of the frame's header the map update owns ----
__global__ __launch_bounds__(1024) void k_wall_weights(const float4 *__restrict__ wall_pts, const int *__restrict__ wall_cell, int wall_cap,
                                                      const int *__restrict__ wall_c2, const int *__restrict__ counts,
                                                      const int *__restrict__ wcounts, pf::KdView tree, float *kw, float resx, float resy,
                                                      const float *__restrict__ pose, HostHeader *__restrict__ hdr, int seq,
                                                      unsigned long long *__restrict__ probe)
{
    pf_stamp(probe);
    const int n_wall = min(counts[0], wall_cap);
    const float cellDiag = pf::fsqrt(resx * resx + resy * resy);
    for (int i = threadIdx.x; i < n_wall; i += 1024) {
        const int b = wall_c2[i];
        if (node_dist(tree, b, wall_pts[i]) < cellDiag) map_weight_add(kw, b, PF_OCCUPIED_WEIGHT);
    }
    if (threadIdx.x != 0 || !hdr) return;
    // the wall list of the mask (this stream) and the sorted one of k_walls are the same list by construction
    const int bad = counts[0] != wcounts[PF_WC_WALLS] ? PF_HDR_INTERNAL : 0;
    hdr->n_wall = counts[0];
    hdr->n_free = counts[1];
    hdr->n_new = wcounts[PF_WC_NEW];
    hdr->kd_size = wcounts[PF_WC_SIZE];
    hdr->flags = wcounts[PF_WC_FLAGS] | bad;
    for (int k = 0; k < 4; k++) hdr->pose[k] = pose[k];
    __threadfence_system();
    __hip_atomic_store(&hdr->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- P: kernUpdateWeights + the tile passes of the weight sums and of the resample scan, one launch ----------------------------------
// k_weights_apply<float> and k_weight_scan_tiles: the new weights of a 4096-particle tile stay in LDS, the tile's two canonical sums
// and its four scan-tile totals are taken from there (the same operations in the same order as the two kernels).
__global__ __launch_bounds__(256) void k_weights_tiles(float *__restrict__ w, float *__restrict__ wm, const float *__restrict__ fit, int n,
                                                       int mirror_count, const long long *__restrict__ stats, float *__restrict__ tile_r,
                                                       float *__restrict__ tile_r2, float *__restrict__ tile_tot,
                                                       unsigned long long *__restrict__ probe)
{
    pf_stamp(probe);
    __shared__ float s_w[PF_SUM_TILE];
    const int t0 = blockIdx.x * PF_SUM_TILE, cnt = min(PF_SUM_TILE, n - t0);
    const long long kmax = stats[0], kmin = stats[1];
    const float fmax = ordered_to_f32((int)(kmax >> 32));
    const float fmin = -ordered_to_f32((int)(kmin >> 32));
    const float rng = fmax - fmin;
    float c = 0.0f;
    int mint = 0;
    if (rng > 0.0f) {
        c = pf::fdiv(1.0f, rng);
        mint = (int)fmin;
    }
    for (int k = threadIdx.x; k < cnt; k += 256) {
        const int i = t0 + k;
        float wi = w[i];
        if (rng > 0.0f) wi = wi * (fit[i] - (float)mint) * c;
        w[i] = wi;
        if (i < mirror_count) wm[i] = wi;
        s_w[k] = wi;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = wave * PF_SCAN_TILE + lane * PF_SCAN_CHUNK; // tile-local
    if (wave * PF_SCAN_TILE < cnt) {
        float local[PF_SCAN_CHUNK];
        const float tot = (c0 < cnt) ? chunk_run(s_w, c0, cnt, local) : 0.0f;
        float total;
        chunk_offset_seq(tot, lane, total);
        if (lane == 0) tile_tot[blockIdx.x * (PF_SUM_TILE / PF_SCAN_TILE) + wave] = total;
    }
    if (wave != 0) return;
    float r = 0.0f, r2 = 0.0f;
#pragma unroll 8
    for (int i = lane; i < cnt; i += 64) {
        const float v = s_w[i];
        r = r + v;
        r2 = r2 + v * v;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        r = r + __shfl_xor(r, off, 64);
        r2 = r2 + __shfl_xor(r2, off, 64);
    }
    if (lane == 0) {
        tile_r[blockIdx.x] = r;
        tile_r2[blockIdx.x] = r2;
    }
}

// the part of the frame's header the particle chain owns (seq2 last; the host waits for both parts)
__device__ __forceinline__ void write_header_a(HostHeader *__restrict__ hdr, float r, float r2, float neff, const long long *__restrict__ stats,
                                               const float *__restrict__ sig, int seq, const float *__restrict__ gtheta = nullptr)
{
    hdr->r = r;
    hdr->r2 = r2;
    hdr->neff = neff;
    hdr->stats[0] = stats[0];
    hdr->stats[1] = stats[1];
    hdr->cloud_sigma = sig[0];
    float tm = 0.0f;
    for (int k = 0; k < 64; k++) tm = fmaxf(tm, sig[2 + k]);
    if (gtheta) tm = fmaxf(tm, *gtheta); // (sharded job: over every rank's pose block, k_theta_gmax)
    hdr->theta_max = tm;
    __threadfence_system();
    __hip_atomic_store(&hdr->seq2, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- P: k_weight_final_offsets + k_scan_apply in one launch ------------------------------------------------------------------------------
// Every workgroup forms the frame's sums itself (the canonical order gives every one of them the same bits: 25 tile sums at 100 k
// particles) and, when the frame resamples, its own tile offset: the strictly sequential sum of the tile totals in front of it (the
// canonical scan order; at most nt - 1 adds out of LDS).  Workgroup 0 publishes the sums and the particle chain's part of the header.
__global__ __launch_bounds__(64) void k_scan_apply2(const float *__restrict__ w, int n, const float *__restrict__ tile_r,
                                                    const float *__restrict__ tile_r2, int nt_sum, const float *__restrict__ tile_tot,
                                                    float *__restrict__ sums, float *__restrict__ cdf, float *__restrict__ chunk_max,
                                                    float *__restrict__ tile_max, double thr, HostHeader *__restrict__ hdr, int seq,
                                                    const long long *__restrict__ stats, const float *__restrict__ sig,
                                                    unsigned long long *__restrict__ probe, const float *__restrict__ gtheta = nullptr)
{
    pf_stamp(probe);
    float r, r2;
    if (n <= PF_SUM_TILE) {
        r = tile_r[0];
        r2 = tile_r2[0];
    } else {
        r = wave_sum_canonical(nt_sum, [&](int i) { return tile_r[i]; });
        r2 = wave_sum_canonical(nt_sum, [&](int i) { return tile_r2[i]; });
    }
    const float neff = pf::fdiv(r * r, r2); // kernel.cu:472
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sums[0] = r;
        sums[1] = r2;
        sums[2] = neff;
        if (hdr) write_header_a(hdr, r, r2, neff, stats, sig, seq, gtheta);
    }
    if (!((double)neff < thr)) return; // every lane of every workgroup holds the same bits
    __shared__ float buf[1024];
    float off = 0.0f;
    for (int t0 = 0; t0 < (int)blockIdx.x; t0 += 1024) {
        const int m = min(1024, (int)blockIdx.x - t0);
        for (int k = threadIdx.x; k < m; k += 64) buf[k] = tile_tot[t0 + k];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < m; k++) off = off + buf[k];
        __syncthreads();
    }
    off = __shfl(off, 0, 64);
    const int lane = threadIdx.x, c0 = blockIdx.x * PF_SCAN_TILE + lane * PF_SCAN_CHUNK;
    float local[PF_SCAN_CHUNK];
    const float tot = (c0 < n) ? chunk_run(w, c0, n, local) : 0.0f;
    float total;
    const float coff = chunk_offset_seq(tot, lane, total);
    float cmax = -INFINITY;
    if (c0 < n) {
        const float base = off + coff;
        for (int k = 0; k < PF_SCAN_CHUNK && c0 + k < n; k++) {
            const float v = base + local[k];
            cdf[c0 + k] = v;
            cmax = fmaxf(cmax, v);
        }
        chunk_max[c0 / PF_SCAN_CHUNK] = cmax;
    }
    const float tmax = wave_max_f32(cmax);
    if (lane == 0) tile_max[blockIdx.x] = tmax;
}
// header part A on its own (frames of up to one sum tile: k_weights_small has left the sums)
__global__ void k_header_a(const float *__restrict__ sums, const long long *__restrict__ stats, const float *__restrict__ sig,
                           HostHeader *__restrict__ hdr, int seq)
{
    if (threadIdx.x == 0) write_header_a(hdr, sums[0], sums[1], sums[2], stats, sig, seq);
}

// ---- P: dispersion + Hilbert cell of the lane order, one launch --------------------------------------------------------------------
// k_motion and k_cell_count, with the cloud statistics the cells are laid over taken from the PREVIOUS frame's launch (workgroup 0 of
// every launch leaves mean and spread of its own 256 particles, after their dispersion, for the next one; an odometry shift moves
// the stored mean along): the order only decides which lane scores which particle, and a cloud moves a fraction of its spread per
// frame -- but every workgroup re-deriving them from the first 1024 slots, and a launch boundary between the dispersion and the
// cells, were 15 of the particle chain's microseconds.  Also here: the frame's largest |heading| (what k_group_box used to reduce).
// cloud[0..3] = {mean x, mean y, mean heading, spread}.
__global__ __launch_bounds__(256) void k_motion_count(float *__restrict__ x, float *__restrict__ y, float *__restrict__ th, float *__restrict__ w,
                                                      const float *__restrict__ wm, int n, int frame, int goff, float reach, int bits,
                                                      unsigned *__restrict__ cell, int *__restrict__ hist, int *__restrict__ cs, CellGeom geo,
                                                      const float *__restrict__ cloud_in, float *__restrict__ cloud_out, float *__restrict__ sig,
                                                      float *__restrict__ sig_next, unsigned long long *__restrict__ probe, double2 *__restrict__ tparts = nullptr,
                                                      int trig = 0)
{
    pf_stamp(probe);
    __shared__ float red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    float xi = 0.0f, yi = 0.0f, ti = 0.0f;
    if (in) { // kernAddNoise (kernel.cu:375-397), k_motion
        w[i] = wm[i];
        uint32_t e2 = pf::engine_seed(frame, goff + i, 0);
        const float sx = 0.015, sy = 0.015, st = .01;
        const float nx = pf::normal(e2, 0.0f, sx, trig != 0);
        const float ny = pf::normal(e2, 0.0f, sy, trig != 0);
        const float nt = pf::normal(e2, 0.0f, st, trig != 0);
        xi = x[i] + nx;
        yi = y[i] + ny;
        ti = th[i] + nt;
        x[i] = xi;
        y[i] = yi;
        th[i] = ti;
        if (tparts) { // cos / sin of the dispersed heading, as doubles: the scan-match kernel's AngleParts of this particle (pf::angle_parts)
            double sd, cd;
            pf::sincos_d(ti, sd, cd);
            tparts[i] = make_double2(cd, sd);
        }
    }
    { // largest |heading| (non-negative floats order like their bit patterns; a NaN counts as infinity)
        float tm = in ? (ti == ti ? fabsf(ti) : INFINITY) : 0.0f;
        tm = wave_max_f32(tm);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = tm;
        __syncthreads();
        // (spread over 64 words: a thousand atomics on ONE word cost k_group_box 15 us; the header's writer takes their maximum)
        if (threadIdx.x == 0) atomicMax((int *)&sig[2 + (blockIdx.x & 63)], __float_as_int(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
        __syncthreads();
    }
    const float mx = cloud_in[0], my = cloud_in[1], mt = cloud_in[2], spread = cloud_in[3];
    if (blockIdx.x == 0 && threadIdx.x < 64) sig_next[2 + threadIdx.x] = 0.0f; // the next ticket's maxima start over (its launch is behind this one on the stream)
    if (blockIdx.x == 0) { // this cloud's statistics for the next launch; the cell window's bookkeeping (k_cell_count)
        const int ns = min(n, 256);
        const float inv = 1.0f / (float)ns;
        const bool s_in = (int)threadIdx.x < ns;
        const float nmx = block_sum_256(s_in ? xi : 0.0f, red) * inv, nmy = block_sum_256(s_in ? yi : 0.0f, red) * inv,
                    nmt = block_sum_256(s_in ? ti : 0.0f, red) * inv;
        const float a = s_in ? xi - nmx : 0.0f, b = s_in ? yi - nmy : 0.0f, c = s_in ? ti - nmt : 0.0f;
        const float dev_x = sqrtf(block_sum_256(a * a, red) * inv), dev_y = sqrtf(block_sum_256(b * b, red) * inv);
        const float dev_t = sqrtf(block_sum_256(c * c, red) * inv) * reach;
        if (threadIdx.x == 0) {
            const float sg = fmaxf(fmaxf(dev_x, dev_y), dev_t);
            cloud_out[0] = nmx; cloud_out[1] = nmy; cloud_out[2] = nmt; cloud_out[3] = sg;
            sig[0] = sg;          // -> header -> host (organisation of the next pass)
            if (cs) {
                const bool fin = fabsf(nmx) < 1e6f && fabsf(nmy) < 1e6f;
                const int kx = fin ? lattice_floor(nmx, geo.resx, geo.invx) : 0, ky = fin ? lattice_floor(nmy, geo.resy, geo.invy) : 0;
                if (cs[PF_CS_FLAGS] & PF_CF_NEED_ORIGIN) {
                    cs[PF_CS_OX] = PF_CELL_SUB * kx - PF_CELL_WIN / 2;
                    cs[PF_CS_OY] = PF_CELL_SUB * ky - PF_CELL_WIN / 2;
                    atomicAnd(&cs[PF_CS_FLAGS], ~PF_CF_NEED_ORIGIN);
                } else if (fin) {
                    const int dx = kx - (cs[PF_CS_OX] + PF_CELL_WIN / 2) / PF_CELL_SUB, dy = ky - (cs[PF_CS_OY] + PF_CELL_WIN / 2) / PF_CELL_SUB;
                    if (abs(dx) > PF_CELL_DRIFT_MAX || abs(dy) > PF_CELL_DRIFT_MAX) atomicOr(&cs[PF_CS_FLAGS], PF_CF_FAR);
                }
            }
        }
    }
    if (!in) return;
    const float D = (float)(1 << bits), half = 0.5f * D, top = D - 1.0f;
    const float e = fmaxf(6.4f / D * spread, 2.5e-4f);
    const float cx = 1.0f / e, cy = 1.0f / e, ct = reach / e;
    unsigned X[3] = {(unsigned)fminf(fmaxf((ti - mt) * ct + half, 0.0f), top),
                     (unsigned)fminf(fmaxf((xi - mx) * cx + half, 0.0f), top),
                     (unsigned)fminf(fmaxf((yi - my) * cy + half, 0.0f), top)};
    const unsigned M = 1u << (bits - 1); // Hilbert index, Skilling's axes-to-transpose (k_cell_count)
    for (unsigned Q = M; Q > 1; Q >>= 1) {
        const unsigned P = Q - 1;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (X[a] & Q) X[0] ^= P;
            else { const unsigned t = (X[0] ^ X[a]) & P; X[0] ^= t; X[a] ^= t; }
        }
    }
    X[1] ^= X[0]; X[2] ^= X[1];
    unsigned t = 0;
    for (unsigned Q = M; Q > 1; Q >>= 1) if (X[2] & Q) t ^= Q - 1;
    X[0] ^= t; X[1] ^= t; X[2] ^= t;
    const unsigned c = (spread3(X[0], bits) << 2) | (spread3(X[1], bits) << 1) | spread3(X[2], bits);
    cell[i] = c;
    atomicAdd(&hist[c], 1);
}
// PFSLAM_STABLE_ORDER=1 (tests): the counting sort places the particles of one Hilbert cell in atomic arrival order, so which of two
// cell-mates ends up in which wave -- hence the waves' pose boxes, hence WHICH lattice cells a frame claims (never a result) -- differs
// from run to run by a handful of cells.  This pass orders every cell's particles by index: the bookkeeping of two runs can then be
// compared to the last slot (tests/test_gpu_frame.py).
__global__ __launch_bounds__(256) void k_order_stable(const int *__restrict__ order, const unsigned *__restrict__ cell, int n, int *__restrict__ out)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const int i = order[s];
    const unsigned c = cell[i];
    int s0 = s, s1 = s + 1;
    while (s0 > 0 && cell[order[s0 - 1]] == c) s0--;
    while (s1 < n && cell[order[s1]] == c) s1++;
    int rank = 0;
    for (int t = s0; t < s1; t++) rank += order[t] < i;
    out[s0 + rank] = i;
}
// the statistics k_motion_count starts from when it has no predecessor (first frame of a run of pipelined frames, set_particles):
// mean and spread of the first min(n, 256) particles as they are; + the reset of the ticket's |heading| maximum
__global__ __launch_bounds__(256) void k_cloud_seed(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ th, int n,
                                                    float reach, float *__restrict__ cloud_out, float *__restrict__ sig)
{
    __shared__ float red[4];
    const int ns = min(n, 256);
    const bool s_in = (int)threadIdx.x < ns;
    const float inv = 1.0f / (float)ns;
    const float xi = s_in ? x[threadIdx.x] : 0.0f, yi = s_in ? y[threadIdx.x] : 0.0f, ti = s_in ? th[threadIdx.x] : 0.0f;
    const float mx = block_sum_256(xi, red) * inv, my = block_sum_256(yi, red) * inv, mt = block_sum_256(ti, red) * inv;
    const float a = s_in ? xi - mx : 0.0f, b = s_in ? yi - my : 0.0f, c = s_in ? ti - mt : 0.0f;
    const float dev_x = sqrtf(block_sum_256(a * a, red) * inv), dev_y = sqrtf(block_sum_256(b * b, red) * inv);
    const float dev_t = sqrtf(block_sum_256(c * c, red) * inv) * reach;
    if (threadIdx.x == 0) {
        // (the dispersion that follows widens the cloud by 1.5 cm / 0.01 rad: in quadrature, so that the cells do not start too narrow)
        const float sx = sqrtf(dev_x * dev_x + 0.015f * 0.015f), sy = sqrtf(dev_y * dev_y + 0.015f * 0.015f);
        const float stt = sqrtf(dev_t * dev_t + (0.01f * reach) * (0.01f * reach));
        cloud_out[0] = mx; cloud_out[1] = my; cloud_out[2] = mt; cloud_out[3] = fmaxf(fmaxf(sx, sy), stt);
    }
    if (threadIdx.x < 64) sig[2 + threadIdx.x] = 0.0f;
}

// ---- K: the single-step ICP (transformPointICP, kernel.cu:993-1093) in one launch ------------------------------------------------------
// k_icp_correspond on ceil(beams / 1024) workgroups; the one that arrives last (ticket behind an agent-scope fence: two or three
// workgroups) runs k_icp_solve's body.  One launch on the cells' stream, behind the insert of the previous frame.
template <bool PLANAR>
__global__ __launch_bounds__(1024) void k_icp_fused(const float *__restrict__ scan, int nb, const float *__restrict__ pose, pf::KdView tree,
                                                   float4 *tar, float4 *cor, float *__restrict__ dbg, int *__restrict__ ticket_word,
                                                   unsigned long long *__restrict__ probe, int *__restrict__ flags, int ticket, int trig)
{
    pf_stamp(probe);
    __shared__ float s_mu[6];
    __shared__ float s_A[9];
    __shared__ int s_last;
    const int i = blockIdx.x * 1024 + threadIdx.x;
    if (i < nb) {
        const float rx = pose[0], ry = pose[1], rt = pose[2];
        float wx, wy;
        pf::clean_lidar_scan(i, scan[i], rt, wx, wy, trig);
        float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (fabsf(wx) < PF_LIDAR_RANGE && fabsf(wy) < PF_LIDAR_RANGE) {
            t.x = rx + wx;
            t.y = ry + wy;
            t.z = 0.0f;
            t.w = PF_OCCUPIED_WEIGHT;
        }
        const int b = pf::kd_nearest_ref<PLANAR>(tree, t.x, t.y, t.z);
        const uint4 nd = tree.hot[b];
        tar[i] = t;
        // (the fourth component is not part of any sum; the node's weight, which the frame's map update may be changing, stays out)
        cor[i] = make_float4(__uint_as_float(nd.x), __uint_as_float(nd.y), PLANAR ? 0.0f : tree.z[b], 0.0f);
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(ticket_word, 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    if (threadIdx.x == 0) *ticket_word = 0;
    if (probe && threadIdx.x == 0) probe[PB_ICP_SOLVE - PB_ICP] = wall_clock64();
    icp_solve_block((const float4 *)tar, (const float4 *)cor, nb, nullptr, nullptr, dbg, s_mu, s_A);
    if (flags && threadIdx.x == 0) { // (thread 0 wrote the increment)
        __threadfence();
        flag_store(flags + PF_FL_ICP, ticket);
    }
}

// ==========================================================================================
// host side
// ==========================================================================================
__global__ void k_fs_init(int *__restrict__ fs, const int *__restrict__ kd_state, const int *__restrict__ cs, long long *__restrict__ fstats)
{
    const int t = threadIdx.x;
    if (t < PF_FRAME_RING) {
        fs[PF_FS_BOUND + t] = kd_state[0];
        fs[PF_FS_WALKED + t] = cs ? min(cs[PF_CS_COUNT], cs[PF_CS_LIST_CAP]) : 0;
    }
    if (t == 0) fs[PF_FS_TICKET] = fs[PF_FS_ICP] = 0;
    if (t < 8 && fstats) fstats[t] = (t & 3) < 2 ? LLONG_MIN : 0;
}
// the walked-up-to words after a synchronous pass (everything up to the counter is walked and published)
__global__ void k_fs_walked(int *__restrict__ fs, const int *__restrict__ cs)
{
    if (threadIdx.x < PF_FRAME_RING) fs[PF_FS_WALKED + threadIdx.x] = min(cs[PF_CS_COUNT], cs[PF_CS_LIST_CAP]);
}

// Do the handle's four streams make progress independently of one another?  For every ordered pair: a gate on the one, then the signal it
// waits for on the other.  Two streams that share a hardware queue would leave the signal queued behind the gate (the test gate gives up
// after 2 ms) or reach it only after 0.2 ms: then the frame's edges stay events.
static int gates_selftest(pfslam_handle *h, bool *ok)
{
    hipStream_t st[4] = {h->stream, h->aux, h->fstream, h->cstream};
    int *res = nullptr;
    CHK(dalloc(&res, 16));
    HIPCHK(hipMemset(res, 0, 64));
    int ticket = 0;
    for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++) {
            if (a == b) continue;
            ticket++;
            hipLaunchKernelGGL(k_gate_test, dim3(1), dim3(64), 0, st[a], (const int *)(h->flags + PF_FL_WORDS - 1), ticket, 200000ull, res + a * 4 + b);
            hipLaunchKernelGGL(k_signal, dim3(1), dim3(64), 0, st[b], h->flags + PF_FL_WORDS - 1, ticket);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st[a]));
            HIPCHK(hipStreamSynchronize(st[b]));
        }
    int host[16];
    HIPCHK(hipMemcpy(host, res, 64, hipMemcpyDeviceToHost));
    HIPCHK(hipFree(res));
    *ok = true;
    for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++)
            if (a != b && !host[a * 4 + b]) *ok = false;
    return 0;
}

static int frame_alloc(pfslam_handle *h)
{
    if (h->fs) return 0;
    CHK(dalloc(&h->fs, PF_FS_WORDS));
    HIPCHK(hipMemsetAsync(h->fs, 0, PF_FS_WORDS * 4, h->stream));
    CHK(dalloc(&h->wcounts, PF_WC_WORDS));
    HIPCHK(hipMemsetAsync(h->wcounts, 0, PF_WC_WORDS * 4, h->stream));
    CHK(dalloc(&h->wall_c2, (size_t)h->max_wall + 64));
    CHK(dalloc(&h->wall_xy2, (size_t)h->max_wall + 64));
    CHK(dalloc(&h->wall_leaf2, (size_t)h->max_wall + 64));
    CHK(dalloc(&h->wall_new2, (size_t)h->max_wall + 64));
    CHK(dalloc(&h->wall_runs, (size_t)h->max_wall + 64));
    CHK(dalloc(&h->wall_keys_s, (size_t)h->max_wall + 64));
    CHK(dalloc(&h->wall_c2s, (size_t)h->max_wall + 64));
    CHK(dalloc(&h->fstats, 8));
    CHK(dalloc(&h->flags, PF_FL_WORDS));
    HIPCHK(hipMemsetAsync(h->flags, 0, PF_FL_WORDS * 4, h->stream));
    HIPCHK(hipHostMalloc((void **)&h->gate_err, 64, hipHostMallocCoherent | hipHostMallocMapped));
    *h->gate_err = 0;
    {
        void *dp = nullptr;
        HIPCHK(hipHostGetDevicePointer(&dp, h->gate_err, 0));
        h->gate_err_dev = (int *)dp;
    }
    CHK(dalloc(&h->cloud, 8));
    HIPCHK(hipMemsetAsync(h->cloud, 0, 32, h->stream));
    CHK(dalloc(&h->sigr, (size_t)PF_FRAME_RING * 80));
    HIPCHK(hipMemsetAsync(h->sigr, 0, (size_t)PF_FRAME_RING * 80 * 4, h->stream));
    CHK(dalloc(&h->order_ring, (size_t)PF_FRAME_RING * h->n));
    hipEvent_t *evs[] = {&h->ev_reduced, &h->ev_tree2, &h->ev_order, &h->ev_icp, &h->ev_ftail, &h->ev_shift, &h->ev_poseg,
                         &h->ev_marked_r[0], &h->ev_marked_r[1], &h->ev_marked_r[2], &h->ev_marked_r[3],
                         &h->ev_walked_r[0], &h->ev_walked_r[1], &h->ev_walked_r[2], &h->ev_walked_r[3],
                         &h->ev_tail[0], &h->ev_tail[1], &h->ev_tail[2]};
    for (hipEvent_t *e : evs) HIPCHK(pf_event_create(e, hipEventDisableTiming));
    return 0;
}
// Gates or events for the frame about to be enqueued?  Gates when the handle asks for them (PFSLAM_GATES), it is the process's only
// handle (g_live_handles) and its four streams have passed the self-test since they last changed (pfslam_set_stream).  A change of
// mode between two frames drains the pipeline: the frames in flight signal their edges the old way.
static int gates_decide(pfslam_handle *h, bool *use)
{
    if (h->gates && !h->gates_tested) {
        if (h->pipe_live) CHK(settle_staged(h));
        hipStream_t st[4] = {h->stream, h->aux, h->fstream, h->cstream};
        for (hipStream_t q : st) HIPCHK(hipStreamSynchronize(q));
        bool ok = false;
        CHK(gates_selftest(h, &ok));
        h->gates_ok = ok;
        h->gates_tested = true;
        if (!ok && getenv("PFSLAM_VERBOSE")) fprintf(stderr, "pfslam: streams share a hardware queue: the frame's cross-stream edges stay events\n");
    }
    const bool want = h->gates && h->gates_ok && g_live_handles.load() == 1;
    if (h->pipe_live && want != h->gates_live) CHK(settle_staged(h));
    h->gates_live = want;
    *use = want;
    return 0;
}

static void frame_free(pfslam_handle *h)
{
    void *bufs[] = {h->fs, h->wcounts, h->flags, h->order_tmp, h->tparts, h->wall_c2, h->wall_xy2, h->wall_leaf2, h->wall_new2, h->wall_runs, h->wall_keys_s, h->wall_c2s, h->fstats, h->cloud, h->sigr, h->order_ring, h->pgroup, h->probe, h->plan_starts};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    hipEvent_t evs[] = {h->ev_reduced, h->ev_tree2, h->ev_order, h->ev_icp, h->ev_ftail, h->ev_shift, h->ev_poseg,
                        h->ev_marked_r[0], h->ev_marked_r[1], h->ev_marked_r[2], h->ev_marked_r[3],
                        h->ev_walked_r[0], h->ev_walked_r[1], h->ev_walked_r[2], h->ev_walked_r[3], h->ev_tail[0], h->ev_tail[1], h->ev_tail[2]};
    for (hipEvent_t e : evs)
        if (e) (void)hipEventDestroy(e);
    if (h->gate_err) (void)hipHostFree(h->gate_err);
}

// the tails of the chain, free-cell and cell streams -> the handle's stream (every entry point but pfslam_step starts with settle(), which
// calls this: whatever it then launches on the handle's stream is behind everything the frames in flight have enqueued anywhere)
static int join_all(pfslam_handle *h)
{
    if (!h->pipe_live || h->serial) return 0;
    hipStream_t tails[3] = {h->aux, h->fstream, h->cstream};
    for (int k = 0; k < 3; k++) {
        HIPCHK(hipEventRecord(h->ev_tail[k], tails[k]));
        HIPCHK(hipStreamWaitEvent(h->stream, h->ev_tail[k], 0));
    }
    return 0;
}

// can this frame run as a round-5 frame?  (everything else -- maps off the lattice, the plan, the plain traversal, non-integral map
// weights, per-phase timing, sharded handles -- takes the round-4 frame; a switch between the two drains the pipeline first)
static bool frame_v2_ok(pfslam_handle *h, int *chunks_out, int *bpc_out)
{
    if (h->timing >= 2 || h->kd_size <= 0 || !h->integral_w || h->nb > 4096) return false;
    if (!org_use_cells(h, nullptr, /*frame_loop=*/true)) return false;
    // the chunk plan (score_plan.h): uniform chunks, or -- long chunks -- last rows that shrink.  It changes with the particle count, the
    // beam count and the map's largest |weight| only
    if (h->plan_n != h->n || h->plan_nb != h->nb || h->plan_w != h->w_absmax) {
        h->chunk_plan = pf::score_plan(h->n, h->nb, h->w_absmax, h->integral_w != 0);
        h->plan_n = h->n;
        h->plan_nb = h->nb;
        h->plan_w = h->w_absmax;
        h->plan_uploaded = false;
    }
    const int used = h->chunk_plan.used, bpc = h->chunk_plan.bpc; // (bpc: the largest chunk)
    if (used < 2 || !((float)bpc * h->w_absmax <= 32767.0f)) return false; // 16-bit partials: a chunk's sum must fit
    if ((h->gn + PF_SCAN_TILE - 1) / PF_SCAN_TILE > 4096) return false; // k_scan_apply2 / k_sample_gather's LDS prefix maxima (a sharded job scans the GLOBAL weights)
    *chunks_out = used;
    *bpc_out = bpc;
    return true;
}

static int probe_slot_ptr(pfslam_handle *h, int id, unsigned long long **out)
{
    *out = (h->probe && h->probe_frames > 0) ? h->probe + (size_t)(h->cur_seq % h->probe_frames) * PF_PROBE_SLOTS + id : nullptr;
    return 0;
}
#define PB(id) (h->probe ? h->probe + (size_t)(seq % h->probe_frames) * PF_PROBE_SLOTS + (id) : (unsigned long long *)nullptr)

// One frame of particleFilter (kernel.cu:1702-1762) as a round-5 frame, enqueued in FOUR parts.  pfslam_step runs them back to back; the
// sharded frame (pfslam_shard_*) is the very same four parts with the caller's three all-gathers between them, each issued on the
// stream the part in front of it has prepared (pfslam_shard_stream) -- no stream of its own for the collectives: a fifth busy stream
// halves the frame rate on this runtime (tools/experiments/r04/README.md), and a collective launched straight into one of the frame's
// four streams needs no event on either side:
//   part 0 (disperse)  P: scan, dispersion, lane order, ORDER.   K: cells' passes.   F: ICP solve.
//                      [sharded, world > 1: all-gather of the pose blocks 16 -> 17 on P -- under the scan-match kernel; P has nothing to do until REDUCED]
//   part 1 (score)     P: k_theta_gmax (says POSEG: the gathered blocks are there).   C: scan-match, reduce.
//                      [all-gather of the 16-byte keys 14 -> 15 on C: the one collective on the frame's critical chain]
//   part 2 (chain)     C: walls (say REDUCED; wait for ICP and POSEG), traversals, insert, cell rows.   P: [gate REDUCED] weights.
//                      [all-gather of the weights 5 -> 10 on P]
//   part 3 (finish)    P: sums on the (gathered) weights, header part A, gated resample out of the (gathered) pose blocks.   F: [wait POSEG]
//                      free cells, weight passes, header part B.   Booking.
// What orders the readers of the gathered buffers (world > 1; tests/test_gpu_sharded_async.py holds each collective back for many frames):
//   17 pose blocks (collective 0, P)   P: k_theta_gmax, k_weights_apply_sharded, k_sample_gather by stream order.  C: k_wall_runs / k_walls<0>
//                                      wait for POSEG (k_theta_gmax's word, or ev_poseg).  F: k_get_walls and k_scatter_cells wait for POSEG
//                                      too -- REDUCED does not cover them: k_wall_runs says REDUCED before its own POSEG wait.
//   15 keys (collective 1, C; P in a one-stream frame)   C: k_wall_runs / k_walls by stream order.  P (k_weights_apply_sharded) and F
//                                      (k_get_walls, k_scatter_cells) wait for REDUCED, which C raises behind the collective.
//   10 weights (collective 2, P)       read on P only (k_weight_scan_tiles, k_scan_apply2, k_sample_gather).
//   next frame's collectives           0 and 2 ride P behind its FTAIL(f) wait (gate or ev_ftail), and FTAIL(f) lies behind every reader of
//                                      frame f on F and, through TREE(f), on C; 1 rides C behind ORDER(f + 1), which P raises behind that
//                                      wait.  A one-stream frame joins all four streams first (join_all).
//   staged chain                       every collective and reader on the handle's stream; its aux-stream map update starts behind an
//                                      event recorded there after k_weights_apply_sharded and reads the pose that kernel wrote, not 15 / 17.
// The caller has staged nothing yet: scan upload, re-balance and the first scan are handled here / by the caller as in frame_front.
struct FvCtx {
    hipStream_t P, C, F, K;
    int seq, s4, s2, lag, groups, world;
    bool gates, serial, sync_cells, sharded, multi, ftail_gate;
    CellGeom geo;
    pf::KdView tv;
    long long *stats, *stats_next;
    float *sig, *sig_next, *icp_dbg;
    int *order, *fl;
    HostHeader *hdr;
    PoseSrc psrc;
};
static FvCtx fv_ctx(pfslam_handle *h)
{
    FvCtx c;
    const auto &fv = h->fv;
    c.serial = fv.serial;
    c.sync_cells = fv.sync_cells;
    c.sharded = fv.sharded;
    c.world = h->world;
    c.multi = fv.sharded && h->world > 1;
    c.gates = fv.gates;
    c.ftail_gate = fv.ftail_gate;
    c.P = h->stream;
    c.C = c.serial ? c.P : h->aux;
    c.F = c.serial ? c.P : h->fstream;
    c.K = c.serial ? c.P : h->cstream;
    c.seq = h->cur_seq;
    c.s4 = c.seq & 3;
    c.s2 = c.seq & 1;
    c.lag = h->publish_lag;
    c.groups = (h->n + 63) / 64;
    c.geo = CellGeom{h->cfg.map_res_x, h->cfg.map_res_y, 1.0f / h->cfg.map_res_x, 1.0f / h->cfg.map_res_y};
    c.tv = kd_view(h);
    c.stats = h->fstats + 4 * c.s2;
    c.stats_next = h->fstats + 4 * (c.s2 ^ 1);
    c.sig = h->sigr + 80 * c.s4;
    c.sig_next = h->sigr + 80 * ((c.seq + 1) & 3);
    c.order = h->order_ring + (size_t)c.s4 * h->n;
    c.hdr = header_dev(h, c.seq);
    c.fl = h->flags;
    // (the ICP increment by ticket parity: the next frame's solve, two edges behind this frame's reduce, must not overwrite what k_walls reads)
    c.icp_dbg = h->icp_dbg + 32 * c.s2;
    c.psrc = PoseSrc{(const long long *)c.stats, h->x_frame, h->y_frame, h->th_frame, (const float *)c.icp_dbg, h->n,
                     c.multi ? (const long long *)h->gkeys : (const long long *)nullptr, c.multi ? (const float *)h->gpose : (const float *)nullptr, h->world, h->stride};
    return c;
}
#define FV_EDGE_WAIT(st, word, ev, back)                                                                                                      \
    do {                                                                                                                                      \
        if (c.gates) {                                                                                                                        \
            hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, st, (const int *)(c.fl + (word)), seq - (back), h->gate_err_dev);                \
            HIPCHK(hipGetLastError());                                                                                                        \
        } else HIPCHK(hipStreamWaitEvent(st, ev, 0));                                                                                         \
    } while (0)

// K: pose boxes, marking, the walk of the new cells.  Nothing in a frame waits for them (a cell claimed here gets its rows two
// frames on; until then its queries take the generic traversal: < 0.01 % of them).  They start with the lane order, beside the
// previous frame's k_cells_update, and the marking pass is mostly over when the scan-match kernel starts (behind the frame's reduce
// instead -- PFSLAM_MARK_EARLY=0 -- its 1081 four-wave workgroups ran beside the chain's latency-bound kernels and cost them 25 us).
// The walk is BOUNDED by the tree size before this frame's insert (it waits for the previous frame's; this frame's may run beside it:
// children it has not seen are ignored), and a publishing pass validates a walked record's links by reading them.
// Synchronous frame (wiped rows): marking and a publishing pass over everything, IN FRONT of the scan-match kernel.
static int fv_cells_passes(pfslam_handle *h, const FvCtx &c)
{
    const int seq = c.seq, s4 = c.s4, groups = c.groups;
    hipStream_t K = c.K;
    const bool mark_early = h->mark_early != 0; // 0 (A/B, PFSLAM_MARK_EARLY=0): behind the frame's reduce instead of the lane order
    if (!c.sync_cells) {
        if (mark_early) FV_EDGE_WAIT(K, PF_FL_ORDER, h->ev_order, 0);
        else FV_EDGE_WAIT(K, PF_FL_REDUCED, h->ev_reduced, 0);
    }
    hipLaunchKernelGGL(k_group_box, dim3(groups), dim3(64), 0, K, h->x_frame, h->y_frame, h->th_frame, h->n, (const int *)c.order, h->group_box, h->group_parts, h->d_sigma);
    const int per_block = PF_MARK_THREADS * PF_MARK_GROUPS;
    hipLaunchKernelGGL(k_cells_mark, dim3(h->nb, (groups + per_block - 1) / per_block), dim3(PF_MARK_THREADS), 0, K, (const pf::KdGroupBox *)h->group_box,
                       groups, (const float *)h->scan, h->nb, c.geo, h->cell_tab, h->cell_list, h->cell_state, (const pf::AngleParts *)h->group_parts,
                       (const pf::BeamParts *)h->beam_angle, PB(PB_MARK));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_marked_r[s4], K));
    // the walks read the tree as the previous frame's insert left it: a definite tree, whatever the timing (the bookkeeping -- which
    // records a walk already extends, which a publishing pass does -- is then the same in every run)
    if (!c.sync_cells && h->pipe_live) FV_EDGE_WAIT(K, PF_FL_TREE, h->ev_tree2, 1);
    if (c.sync_cells) {
        h->cells_passes++;
        hipLaunchKernelGGL(k_cells_update<true>, dim3(PF_CELLS_GRID), dim3(64), 0, K, c.tv, c.geo, h->cell_tab, (const int *)h->cell_list, h->cell_state, h->cell_pool,
                           h->cell_rec, h->cells_gen, (const int *)nullptr, 0, 0, 0, CellPass{nullptr, nullptr, nullptr, nullptr, 0}, PB(PB_WALK));
        hipLaunchKernelGGL(k_fs_walked, dim3(1), dim3(64), 0, K, h->fs, (const int *)h->cell_state);
    } else {
        // records [walked by the previous walk pass, counter) on the tree as the previous frame's insert left it
        hipLaunchKernelGGL(k_cells_update<false>, dim3(PF_CELLS_WALK_GRID), dim3(64), 0, K, c.tv, c.geo, h->cell_tab, (const int *)h->cell_list, h->cell_state,
                           h->cell_pool, h->cell_rec, h->cells_gen, (const int *)nullptr, 0, 0, 0,
                           CellPass{h->fs + PF_FS_WALKED + ((seq - 1) & 3), h->fs + PF_FS_WALKED + s4, nullptr, h->fs + PF_FS_BOUND + s4, 0}, PB(PB_WALK));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_walked_r[s4], K));
    return 0;
}

// ---- part 0: P front (scan, dispersion, lane order), K cells' passes, F ICP solve --------------------------------------------------------
static int frame_v2_begin(pfslam_handle *h, int frame, const float *scan_host, int used, int bpc, bool sharded)
{
    CHK(frame_alloc(h));
    if (!h->cell_tab) CHK(cells_alloc(h));
    const int groups = (h->n + 63) / 64;
    if (!h->group_box) CHK(dalloc(&h->group_box, (size_t)groups));
    if (!h->group_parts) CHK(dalloc(&h->group_parts, (size_t)groups));
    {
        const size_t need = (size_t)groups * used * 64;
        if (need > h->pgroup_elems) {
            if (h->pgroup) HIPCHK(hipFree(h->pgroup));
            h->pgroup = nullptr;
            CHK(dalloc(&h->pgroup, need));
            h->pgroup_elems = need;
        }
    }
    // The plan's chunk starts, where the chunks are not all of one size (frame_v2_ok has just made the plan these `used` chunks belong to).
    // A new plan is rare -- another map's weights, another particle count: the launches that read the old starts are waited for.
    if (h->chunk_plan.tapered && !h->plan_uploaded) {
        for (hipStream_t st : {h->stream, h->aux, h->cstream, h->istream}) HIPCHK(hipStreamSynchronize(st));
        if ((int)h->chunk_plan.starts.size() > h->plan_starts_cap) {
            if (h->plan_starts) HIPCHK(hipFree(h->plan_starts));
            h->plan_starts = nullptr;
            h->plan_starts_cap = 0;
            CHK(dalloc(&h->plan_starts, h->chunk_plan.starts.size()));
            h->plan_starts_cap = (int)h->chunk_plan.starts.size();
        }
        HIPCHK(hipMemcpy(h->plan_starts, h->chunk_plan.starts.data(), h->chunk_plan.starts.size() * 4, hipMemcpyHostToDevice));
        h->plan_uploaded = true;
    }
    bool gates = false;
    CHK(gates_decide(h, &gates)); // (may drain the pipeline: a change of mode, a self-test that has to run again)
    const bool sync_cells = h->cells_wipe_pending; // wiped rows: marked, walked and published in front of the scan-match kernel
    const bool serial = h->serial != 0 || sync_cells;
    if (!h->pipe_live) { // first round-5 frame behind anything else: nothing in flight, every ring slot and ticket word starts over
        CHK(settle(h));
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipStreamSynchronize(h->aux));
        HIPCHK(hipStreamSynchronize(h->cstream));
        HIPCHK(hipStreamSynchronize(h->istream));
        hipLaunchKernelGGL(k_fs_init, dim3(1), dim3(64), 0, h->stream, h->fs, (const int *)h->kd_state,
                           sync_cells ? (const int *)nullptr : (const int *)h->cell_state, h->fstats);
        HIPCHK(hipMemsetAsync(h->sigr, 0, (size_t)PF_FRAME_RING * 80 * 4, h->stream));
        HIPCHK(hipGetLastError());
        h->cloud_valid = false;
        h->shift_pending = false;
        h->icp_forked = h->map_forked = h->walk_pending = h->cells_snap = h->tree_event = h->mark_on_aux = false;
        HIPCHK(hipStreamSynchronize(h->stream)); // (the other streams' first launches of this frame read these words)
    } else if (serial) {
        CHK(join_all(h)); // everything the previous frames left on the other streams, in front of this frame's single stream
    }
    const int seq = ++h->seq;
    h->cur_seq = seq;
    h->cur_frame = frame;
    h->fv.used = used;
    h->fv.bpc = bpc;
    h->fv.starts = h->chunk_plan.tapered ? h->plan_starts : nullptr; // (null: uniform chunks of bpc beams)
    h->fv.frame = frame;
    h->fv.sync_cells = sync_cells;
    h->fv.serial = serial;
    h->fv.sharded = sharded;
    h->fv.gates = gates;
    h->fv.ftail_gate = gates && !serial;
    h->x_frame = h->x; h->y_frame = h->y; h->th_frame = h->th; // this frame's pose block (swap_pose_blocks moves h->x .. on before the cells' passes are enqueued)
    const FvCtx c = fv_ctx(h);
    hipStream_t P = c.P, F = c.F;
    int *fl = c.fl;
    const bool ftail_gate = c.ftail_gate;

    // ---- P: dispersion + lane order ----
    if (sync_cells) CHK(cells_wipe(h)); // (serial frame: P is every stream; in front of the window's new origin, which the cell count sets)
    {
        const int bits = h->n <= 400000 ? 6 : PF_CELL_BITS_MAX, ncell = 1 << (3 * bits);
        int *hist = h->cells, *cursor = h->cells + ncell, *tile_tot = h->cells + 2 * ncell;
        float *cloud_in = h->cloud + 4 * (c.s2 ^ 1), *cloud_out = h->cloud + 4 * c.s2;
        { // the frame's scan: every reader on the other streams takes it with the lane order (ev_order)
            float *hs = h->h_scan + (size_t)(seq % PF_HDR_SLOTS) * h->nb;
            h->scan = h->scan_base + (size_t)(seq % PF_HDR_SLOTS) * h->nb;
            memcpy(hs, scan_host, (size_t)h->nb * 4);
            scan_reach_of(h, hs);
            // (frame probe on: this ticket's row of stamps starts empty -- "0 = that launch did not run" also after the ring has wrapped.  Every
            // other stream's first launch of the frame sits behind SCAN(t) / ORDER(t), which this stream raises behind the memset.)
            if (h->probe && h->probe_frames > 0) {
                HIPCHK(hipMemsetAsync(h->probe + (size_t)(seq % h->probe_frames) * PF_PROBE_SLOTS, 0, (size_t)PF_PROBE_SLOTS * 8, P));
                HIPCHK(hipMemsetAsync(h->probe + (size_t)h->probe_frames * PF_PROBE_SLOTS + (size_t)(seq % h->probe_frames) * PF_PROBE_ENDS * PF_PROBE_END_STRIDE, 0,
                                      (size_t)PF_PROBE_ENDS * PF_PROBE_END_STRIDE * 8, P)); // (the ends of the scan-match launch's waves)
            }
            HIPCHK(hipMemcpyAsync(h->scan, hs, (size_t)h->nb * 4, hipMemcpyHostToDevice, P));
            // (gates) the scan is there: all the ICP solve waits for -- it then starts behind the previous frame's wall weights instead of behind
            // this frame's lane order, which matters when the scan-match kernel is too short to hide it (1000 particles: the wall kernel
            // waited for the increment)
            if (gates && !serial) hipLaunchKernelGGL(k_signal, dim3(1), dim3(64), 0, P, fl + PF_FL_SCAN, seq);
        }
        const float reach = h->scan_reach;
        h->tparts_cur = nullptr;
        if (!h->cloud_valid) {
            hipLaunchKernelGGL(k_cloud_seed, dim3(1), dim3(256), 0, P, (const float *)h->x, (const float *)h->y, (const float *)h->th, h->n, reach, cloud_in, c.sig);
            h->cloud_valid = true;
        }
        hipLaunchKernelGGL(k_motion_count, dim3((h->n + 255) / 256), dim3(256), 0, P, h->x, h->y, h->th, h->w, (const float *)h->wm, h->n, frame, h->goff,
                           reach, bits, h->mkey, hist, h->cell_state, c.geo, (const float *)cloud_in, cloud_out, c.sig, c.sig_next, PB(PB_MOTION), (double2 *)nullptr, h->trig);
        hipLaunchKernelGGL(k_cell_scan, dim3(ncell / 1024), dim3(256), 0, P, hist, cursor, tile_tot);
        hipLaunchKernelGGL(k_cell_scatter, dim3((h->n + 255) / 256), dim3(256), 0, P, h->mkey, h->n, cursor, tile_tot, ncell / 1024, c.order);
        if (h->stable_order) { // (tests)
            if (!h->order_tmp) CHK(dalloc(&h->order_tmp, (size_t)h->n));
            hipLaunchKernelGGL(k_order_stable, dim3((h->n + 255) / 256), dim3(256), 0, P, (const int *)c.order, (const unsigned *)h->mkey, h->n, h->order_tmp);
            HIPCHK(hipMemcpyAsync(c.order, h->order_tmp, (size_t)h->n * 4, hipMemcpyDeviceToDevice, P));
        }
        HIPCHK(hipGetLastError());
        // The lane order is the ONE thing the scan-match kernel waits for, so everything else it needs from another stream hangs on
        // it: the previous frame's free-cell chain (the -1 / +4 weight passes the kernel's scores read; the last reader of the previous
        // pose block's best particle) must be over before the order is announced -- it ended ~40 us ago.
        if (h->pipe_live && !serial) {
            if (ftail_gate) hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, P, (const int *)(fl + PF_FL_FTAIL), seq - 1, h->gate_err_dev); // (stored by this frame's first launch on F, below)
            else if (h->ftail_recorded) HIPCHK(hipStreamWaitEvent(P, h->ev_ftail, 0));
        }
        if (gates) hipLaunchKernelGGL(k_signal, dim3(1), dim3(64), 0, P, fl + PF_FL_ORDER, seq);
        else HIPCHK(hipEventRecord(h->ev_order, P));
        h->theta_bound += 0.1f;
    }
    // ---- K (see fv_cells_passes) ----
    if (sync_cells || h->mark_early != 0) CHK(fv_cells_passes(h, c));
    // ---- F: the ICP solve (transformPointICP, kernel.cu:993-1093: the scan at the PREVIOUS pose against the map as the previous frame's
    // insert left it -- this stream waited for that insert in front of k_wall_weights).  Behind the lane order (the scan comes with it):
    // beside the first microseconds of the scan-match kernel, on a high-priority stream (on the cells' low-priority stream its two
    // workgroups queued behind the scan-match kernel's 131 k); the chain takes its increment in front of the reduce. ----
    {
        if (ftail_gate) { // the gate for the scan, announcing first that the previous frame's free-cell chain (k_wall_weights) is over
            hipLaunchKernelGGL(k_gate_signal, dim3(1), dim3(64), 0, F, fl + PF_FL_FTAIL, seq - 1, (const int *)(fl + PF_FL_SCAN), seq, h->gate_err_dev);
            HIPCHK(hipGetLastError());
        } else FV_EDGE_WAIT(F, PF_FL_ORDER, h->ev_order, 0);
        if (h->shift_pending) HIPCHK(hipStreamWaitEvent(F, h->ev_shift, 0)); // (the solve starts from the shifted pose)
        h->shift_pending = false;
        const dim3 gi((h->nb + 1023) / 1024);
        if (h->planar)
            hipLaunchKernelGGL(k_icp_fused<true>, gi, dim3(1024), 0, F, (const float *)h->scan, h->nb, (const float *)h->pose, c.tv, (float4 *)h->icp_tar,
                               (float4 *)h->icp_cor, c.icp_dbg, h->fs + PF_FS_ICP, PB(PB_ICP), gates ? fl : (int *)nullptr, seq, h->trig);
        else
            hipLaunchKernelGGL(k_icp_fused<false>, gi, dim3(1024), 0, F, (const float *)h->scan, h->nb, (const float *)h->pose, c.tv, (float4 *)h->icp_tar,
                               (float4 *)h->icp_cor, c.icp_dbg, h->fs + PF_FS_ICP, PB(PB_ICP), gates ? fl : (int *)nullptr, seq, h->trig);
        HIPCHK(hipGetLastError());
        if (!gates) HIPCHK(hipEventRecord(h->ev_icp, F));
    }
    return 0;
}

// ---- part 1: (sharded: the gathered pose blocks are there) C: scan-match -> reduce ----------------------------------------------------------
static int frame_v2_score(pfslam_handle *h)
{
    const FvCtx c = fv_ctx(h);
    const int seq = c.seq, used = h->fv.used, bpc = h->fv.bpc, groups = c.groups;
    hipStream_t P = c.P, C = c.C;
    if (c.multi) {
        // the caller's all-gather of the pose blocks sits on P in front of this: the job-wide |heading| maximum for the header (the host's
        // choice of the next scan-match kernel's instantiation), and the word that says the gathered blocks are there
        hipLaunchKernelGGL(k_theta_gmax, dim3(std::min(256, (h->world * h->stride + 255) / 256)), dim3(256), 0, P, (const float *)h->gpose, h->world, h->stride, h->gtheta,
                           seq, c.gates ? c.fl + PF_FL_POSEG : (int *)nullptr);
        HIPCHK(hipGetLastError());
        if (!c.gates) HIPCHK(hipEventRecord(h->ev_poseg, P));
    }
    // ONE wait in front of the scan-match kernel: the lane order.  What else the kernel and the chain behind it need from other
    // streams -- the previous marking pass done with the particle block the resample overwrites, the walk pass whose records this
    // frame's publishing pass takes -- the particle chain waited for at the start of its previous branch (long satisfied there).
    FV_EDGE_WAIT(C, PF_FL_ORDER, h->ev_order, 0);
    hipEvent_t t_a = nullptr, t_b = nullptr;
    if (h->timing) {
        CHK(timer_event(h, &t_a));
        CHK(timer_event(h, &t_b));
        HIPCHK(hipEventRecord(t_a, C));
    }
    // a sharded job's resample imports particles from the other shards: unguarded only once a header with the job-wide |heading| maximum is booked
    const bool guard = !(h->theta_bound < 0.5f * PF_SUM_THETA_MAX) || (c.multi && !h->theta_global_known);
    const dim3 grid64(groups, used); // groups fastest: the plan's short chunks are the last to be dispatched
    const int *starts = h->fv.starts;
    unsigned long long *ends = h->probe ? h->probe + (size_t)h->probe_frames * PF_PROBE_SLOTS + (size_t)(seq % h->probe_frames) * PF_PROBE_ENDS * PF_PROBE_END_STRIDE : nullptr;
#define PF_CELLS_ARGS grid64, dim3(64), 0, C, h->x_frame, h->y_frame, h->th_frame, h->n, h->scan, (const pf::BeamParts *)h->beam_angle, h->nb, bpc, c.tv, c.geo, \
                      (const unsigned *)h->cell_tab, (const uint4 *)h->cell_pool, (const int *)h->cell_state, (const int *)c.order, 0
#define PF_CELLS_TAIL (float *)h->pgroup, 4, (pf::KdCensus *)nullptr, PB(PB_SCORE), (const double2 *)nullptr, starts, ends
    if (ends) { // frame probe on: the instantiations that also say when each wave ended
        if (h->trig) hipLaunchKernelGGL((k_score_kd_cells<false, PF_TRIG_DEVLIB, true>), PF_CELLS_ARGS, PF_CELLS_TAIL);
        else if (guard) hipLaunchKernelGGL((k_score_kd_cells<false, true, true>), PF_CELLS_ARGS, PF_CELLS_TAIL);
        else hipLaunchKernelGGL((k_score_kd_cells<false, false, true>), PF_CELLS_ARGS, PF_CELLS_TAIL);
    } else if (h->trig) hipLaunchKernelGGL((k_score_kd_cells<false, PF_TRIG_DEVLIB>), PF_CELLS_ARGS, PF_CELLS_TAIL);
    else if (guard) hipLaunchKernelGGL((k_score_kd_cells<false, true>), PF_CELLS_ARGS, PF_CELLS_TAIL);
    else hipLaunchKernelGGL((k_score_kd_cells<false, false>), PF_CELLS_ARGS, PF_CELLS_TAIL);
#undef PF_CELLS_TAIL
    HIPCHK(hipGetLastError());
    if (t_a) {
        HIPCHK(hipEventRecord(t_b, C));
        h->ev_pending.push_back(pfslam_handle::TimedSpan{t_a, t_b, PF_T_SCORE});
    }
    if (h->census_log && h->census_n < PF_CENSUS_LOG) { // the counting instantiation on the very same inputs, grid and chunk plan (no output: mode 2)
        if (h->trig) hipLaunchKernelGGL((k_score_kd_cells<true, PF_TRIG_DEVLIB>), PF_CELLS_ARGS, (float *)h->pgroup, 2, h->census_log + h->census_n++, (unsigned long long *)nullptr, (const double2 *)nullptr, starts);
        else hipLaunchKernelGGL((k_score_kd_cells<true, true>), PF_CELLS_ARGS, (float *)h->pgroup, 2, h->census_log + h->census_n++, (unsigned long long *)nullptr, (const double2 *)nullptr, starts);
        HIPCHK(hipGetLastError());
    }
#undef PF_CELLS_ARGS
    // the ICP increment (cells' stream, behind the previous frame's insert) goes into the pose the reduce's last workgroup forms: it has
    // had the whole scan-match kernel to finish -- waiting for it HERE keeps a 50 us solve out of the scan-match kernel's way
    if (!c.gates) HIPCHK(hipStreamWaitEvent(C, h->ev_icp, 0)); // (gates: k_walls waits for the increment itself)
    if (used >= 256) // few particles, up to one chunk per beam: the four waves of a workgroup share one group
        hipLaunchKernelGGL((k_reduce_groups<4>), dim3(groups), dim3(256), 0, C, (const short *)h->pgroup, h->n, groups, used, (const int *)c.order, h->fit, c.stats,
                           PB(PB_REDUCE), h->goff);
    else {
        hipLaunchKernelGGL((k_reduce_groups<1>), dim3(std::min((groups + 3) / 4, PF_REDUCE_WGS)), dim3(256), 0, C, (const short *)h->pgroup, h->n, groups, used,
                           (const int *)c.order, h->fit, c.stats, PB(PB_REDUCE), h->goff);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- part 2: (sharded: every rank's keys are there) C: walls + insert -> cell rows; P: weights ---------------------------------------------
static int frame_v2_chain(pfslam_handle *h)
{
    const FvCtx c = fv_ctx(h);
    const int seq = c.seq, s4 = c.s4, lag = c.lag;
    hipStream_t P = c.P, C = c.C;
    const bool gates = c.gates, serial = c.serial, sync_cells = c.sync_cells;
    int *fl = c.fl;
    {
        if (!gates) {
            HIPCHK(hipEventRecord(h->ev_reduced, C)); // (gates: k_walls says so in front of its own work)
            if (c.multi) HIPCHK(hipStreamWaitEvent(C, h->ev_poseg, 0));
        }
        if (!sync_cells && h->mark_early == 0) CHK(fv_cells_passes(h, c));
        const int sort_n = (h->nb + 63) / 64 * 64; // whole waves: also the stride of k_walls' LDS arrays
        const size_t lds = (size_t)sort_n * 9 * sizeof(uint32_t);
        if (!h->walls_attr_set) {
            HIPCHK(hipFuncSetAttribute((const void *)k_walls<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIPCHK(hipFuncSetAttribute((const void *)k_walls<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            h->walls_attr_set = true;
        }
        const int cx = (int)roundf(0.5f * h->dimx + h->cfg.map_res_x / 2), cy = (int)roundf(0.5f * h->dimy + h->cfg.map_res_y / 2);
        const int wait_poseg = c.multi ? 1 : 0;
#define PF_WALLS_ARGS dim3(1), dim3(1024), lds, C, (const float *)h->scan, (const pf::BeamParts *)h->beam_angle, h->nb, sort_n, c.psrc, h->start, h->pose, c.stats_next, \
                      cx, cy, h->dimx, h->dimy, h->cfg.map_res_x, h->cfg.map_res_y, h->cfg.map_scale_x, h->cfg.map_scale_y, c.tv, h->hot, h->parent, h->kz, h->kw,   \
                      h->kd_state, h->kd_cap, sort_n, h->wall_c2, h->wcounts, h->fs + PF_FS_BOUND + ((seq + 1) & 3), (const int *)h->cell_state, h->cell_touched
        if (h->planar == 0) {
            hipLaunchKernelGGL(k_walls<0>, PF_WALLS_ARGS, PB(PB_WALLS), h->wall_xy2, h->wall_leaf2, h->wall_new2, gates ? fl : (int *)nullptr, seq, h->gate_err_dev,
                               (const uint32_t *)nullptr, (const int *)nullptr, wait_poseg, h->trig);
        } else {
            hipLaunchKernelGGL(k_wall_runs, dim3(sort_n / 64), dim3(64), 0, C, (const float *)h->scan, (const pf::BeamParts *)h->beam_angle, h->nb, c.psrc, h->start, h->pose,
                               c.stats_next, cx, cy, h->dimx, h->dimy, h->cfg.map_res_x, h->cfg.map_res_y, h->wall_runs, h->wall_keys_s, PB(PB_WALLS),
                               gates ? fl : (int *)nullptr, seq, h->gate_err_dev, wait_poseg, h->trig);
            // (4 workgroups per run of 64 keys: ranks + traversals 34.4 -> 32.4 us, frame -2.5 us at 1000 and at 100 000 particles)
            const int walls_split = 4;
            hipLaunchKernelGGL(k_walls_rank_traverse<true>, dim3(sort_n / 64 * walls_split), dim3(64), (size_t)sort_n * 4, C, (const uint32_t *)h->wall_runs, sort_n,
                               (const float *)h->pose, h->dimx, h->cfg.map_res_x, h->cfg.map_res_y, h->cfg.map_scale_x, h->cfg.map_scale_y, c.tv, h->wall_keys_s,
                               h->wall_xy2, h->wall_c2s, h->wall_leaf2, h->wall_new2, PB(PB_WALLS_REP), walls_split);
            hipLaunchKernelGGL(k_walls<3>, PF_WALLS_ARGS, PB(PB_WALLS), h->wall_xy2, h->wall_leaf2, h->wall_new2, (int *)nullptr, seq, (int *)nullptr,
                               (const uint32_t *)h->wall_keys_s, (const int *)h->wall_c2s);
        }
#undef PF_WALLS_ARGS
        HIPCHK(hipGetLastError());
        if (!gates) HIPCHK(hipEventRecord(h->ev_tree2, C)); // (gates: k_cells_update says so in front of its own work)
        const int recut = h->cells_passes > 0 && h->cells_passes % PF_CELLS_RECUT_EVERY == 0 ? 1 : 0;
        if (recut) HIPCHK(hipMemsetAsync(h->cell_state + PF_CS_POOL, 0, 4, C));
        // the records a walk pass finished `lag` frames ago (the particle chain waited for it a frame ago); synchronous frame: everything (the walked words say so)
        hipLaunchKernelGGL(k_cells_update<true>, dim3(PF_CELLS_GRID), dim3(64), 0, C, c.tv, c.geo, h->cell_tab, (const int *)h->cell_list, h->cell_state, h->cell_pool,
                           h->cell_rec, h->cells_gen, (const int *)h->cell_touched, (int)(h->cells_passes & 15), recut, 0,
                           CellPass{nullptr, nullptr, h->fs + PF_FS_WALKED + ((seq - (sync_cells ? 0 : lag)) & 3), nullptr, h->fault}, PB(PB_UPDATE),
                           gates ? fl + PF_FL_TREE : (int *)nullptr, seq);
        HIPCHK(hipGetLastError());
        h->cells_passes++;
    }
    // ---- P: weights (a sharded frame: of this shard, from every rank's keys; the sums wait for the gathered weights: part 3) ----
    {
        FV_EDGE_WAIT(P, PF_FL_REDUCED, h->ev_reduced, 0);
        if (!serial) {
            // (both fired a frame ago) the previous frame's pose boxes are made: its pose block may be overwritten by this frame's resample;
            // the records the NEXT frame's publishing pass takes -- those of the walk pass `lag` - 1 frames back -- are written
            HIPCHK(hipStreamWaitEvent(P, h->ev_marked_r[(seq - 1) & 3], 0));
            HIPCHK(hipStreamWaitEvent(P, h->ev_walked_r[(seq + 1 - lag) & 3], 0));
        }
        if (c.sharded) {
            hipLaunchKernelGGL(k_weights_apply_sharded, dim3((h->n + 255) / 256), dim3(256), 0, P, h->w, h->wm, (const float *)h->fit, h->n, h->goff, mirror_count(h),
                               (const long long *)c.stats, c.multi ? (const long long *)h->gkeys : (const long long *)nullptr, h->world, (const float *)h->gpose, h->stride,
                               h->mkeys, (float *)nullptr, (const float *)nullptr, (float *)nullptr, PB(PB_WEIGHTS));
            HIPCHK(hipGetLastError());
        }
    }
    (void)s4;
    return 0;
}

// ---- part 3: (sharded: every rank's weights are there) P: sums, header part A, gated resample; F: free cells, weight passes, header part B ----
static int frame_v2_finish(pfslam_handle *h)
{
    const FvCtx c = fv_ctx(h);
    const int seq = c.seq, s4 = c.s4, frame = h->fv.frame;
    hipStream_t P = c.P, F = c.F;
    {
        const double thr = PF_EFFECTIVE_PARTICLES * h->gn;
        if (c.sharded) { // everything on the GLOBAL weights (gw aliases w on a one-rank job), sources out of the gathered pose blocks
            const int gn = h->gn, n = h->n;
            const int nts = (gn + PF_SUM_TILE - 1) / PF_SUM_TILE, nt = (gn + PF_SCAN_TILE - 1) / PF_SCAN_TILE;
            hipLaunchKernelGGL(k_weight_scan_tiles, dim3(nts), dim3(256), 0, P, (const float *)h->gw, gn, h->tile_r, h->tile_r2, h->tile_tot);
            hipLaunchKernelGGL(k_scan_apply2, dim3(nt), dim3(64), 0, P, (const float *)h->gw, gn, (const float *)h->tile_r, (const float *)h->tile_r2, nts,
                               (const float *)h->tile_tot, h->sums, h->cdf, h->chunk_max, h->tile_pmax, thr, c.hdr, seq, (const long long *)h->mkeys,
                               (const float *)c.sig, PB(PB_APPLY), c.multi ? (const float *)(h->gtheta + s4) : (const float *)nullptr);
            if (c.multi)
                hipLaunchKernelGGL((k_sample_gather<true, true>), dim3((n + 255) / 256), dim3(256), 0, P, (const float *)h->cdf, (const float *)h->chunk_max,
                                   (const float *)h->tile_pmax, gn, n, h->goff, frame, (const float *)h->sums, h->src, (const float *)h->gpose, h->pblk2, h->stride, h->w,
                                   h->wm, thr, h->resampler);
            else
                hipLaunchKernelGGL((k_sample_gather<true, false>), dim3((n + 255) / 256), dim3(256), 0, P, (const float *)h->cdf, (const float *)h->chunk_max,
                                   (const float *)h->tile_pmax, n, n, 0, frame, (const float *)h->sums, h->src, (const float *)h->pblk, h->pblk2, h->stride, h->w,
                                   h->wm, thr, h->resampler);
        } else {
            const int n = h->n;
            if (n <= PF_SUM_TILE) {
                hipLaunchKernelGGL(k_weights_small<float>, dim3(1), dim3(256), 0, P, h->w, h->wm, (const float *)h->fit, n, mirror_count(h), (const long long *)c.stats,
                                   h->x, h->y, h->th, (float *)nullptr, h->sums, (const float *)nullptr, h->pose);
                hipLaunchKernelGGL(k_header_a, dim3(1), dim3(64), 0, P, (const float *)h->sums, (const long long *)c.stats, (const float *)c.sig, c.hdr, seq);
                hipLaunchKernelGGL(k_resample_small, dim3(1), dim3(1024), 0, P, (const float *)h->w, n, h->cdf, h->chunk_max, h->tile_pmax, frame,
                                   (const float *)h->sums, h->src, (const float *)h->pblk, h->pblk2, h->stride, h->w, h->wm, thr, h->resampler);
            } else {
                const int nts = (n + PF_SUM_TILE - 1) / PF_SUM_TILE, nt = (n + PF_SCAN_TILE - 1) / PF_SCAN_TILE;
                hipLaunchKernelGGL(k_weights_tiles, dim3(nts), dim3(256), 0, P, h->w, h->wm, (const float *)h->fit, n, mirror_count(h), (const long long *)c.stats,
                                   h->tile_r, h->tile_r2, h->tile_tot, PB(PB_WEIGHTS));
                hipLaunchKernelGGL(k_scan_apply2, dim3(nt), dim3(64), 0, P, (const float *)h->w, n, (const float *)h->tile_r, (const float *)h->tile_r2, nts,
                                   (const float *)h->tile_tot, h->sums, h->cdf, h->chunk_max, h->tile_pmax, thr, c.hdr, seq, (const long long *)c.stats,
                                   (const float *)c.sig, PB(PB_APPLY));
                hipLaunchKernelGGL((k_sample_gather<true, false>), dim3((n + 255) / 256), dim3(256), 0, P, (const float *)h->cdf, (const float *)h->chunk_max,
                                   (const float *)h->tile_pmax, n, n, 0, frame, (const float *)h->sums, h->src, (const float *)h->pblk, h->pblk2, h->stride, h->w,
                                   h->wm, thr, h->resampler);
            }
        }
        HIPCHK(hipGetLastError());
        swap_pose_blocks(h);
    }
    // ---- F: the free cells (rays, lists, -1 pass on the tree before the insert), then the walls' +4 and header part B ----
    {
        FV_EDGE_WAIT(F, PF_FL_REDUCED, h->ev_reduced, 0);
        // (sharded: k_get_walls and k_scatter_cells read the best particle's pose out of the gathered pose blocks.  REDUCED does not cover
        // them -- k_wall_runs says REDUCED before it waits for POSEG, and ev_reduced is recorded in front of C's wait for ev_poseg -- so the
        // pose blocks' all-gather may still be running when the keys' has long finished)
        if (c.multi) FV_EDGE_WAIT(F, PF_FL_POSEG, h->ev_poseg, 0);
        const int cx = (int)roundf(0.5f * h->dimx + h->cfg.map_res_x / 2), cy = (int)roundf(0.5f * h->dimy + h->cfg.map_res_y / 2);
        const int M = h->dimx * h->dimy, nblk = (M + 4095) / 4096;
        if (!h->masks_cleared) HIPCHK(hipMemsetAsync(h->free_mask, 0, mask_bytes(h), F));
        hipLaunchKernelGGL(k_get_walls, dim3((h->nb + 3) / 4), dim3(256), 0, F, h->scan, h->nb, h->pose, cx, cy, h->free_mask, h->wall_mask, h->dimx, h->dimy,
                           h->cfg.map_res_x, h->cfg.map_res_y, 0, c.psrc, h->trig);
        hipLaunchKernelGGL(k_count_cells, dim3(nblk), dim3(256), 0, F, h->free_mask, h->wall_mask, M, h->blk_cnt);
        hipLaunchKernelGGL(k_scatter_cells, dim3(nblk), dim3(256), 0, F, h->free_mask, h->wall_mask, M, h->blk_cnt, h->counts, h->dimx, h->cfg.map_res_x,
                           h->cfg.map_res_y, h->cfg.map_scale_x, h->cfg.map_scale_y, h->pose, h->wall_cell, h->wall_pts, h->max_wall, h->free_cell,
                           h->free_pts, h->max_free, 1, c.psrc);
        h->masks_cleared = true;
        if (h->planar)
            hipLaunchKernelGGL(k_free_traverse<true>, dim3(1024), dim3(256), 0, F, h->free_pts, h->free_c, h->max_free, h->max_wall, (const int *)h->counts, c.tv,
                               h->cfg.free_upload_bug, h->kw, h->cfg.map_res_x, h->cfg.map_res_y, (const int *)(h->fs + PF_FS_BOUND + s4), PB(PB_FREE));
        else
            hipLaunchKernelGGL(k_free_traverse<false>, dim3(1024), dim3(256), 0, F, h->free_pts, h->free_c, h->max_free, h->max_wall, (const int *)h->counts, c.tv,
                               h->cfg.free_upload_bug, h->kw, h->cfg.map_res_x, h->cfg.map_res_y, (const int *)(h->fs + PF_FS_BOUND + s4), PB(PB_FREE));
        HIPCHK(hipGetLastError());
        FV_EDGE_WAIT(F, PF_FL_TREE, h->ev_tree2, 0);
        hipLaunchKernelGGL(k_wall_weights, dim3(1), dim3(1024), 0, F, (const float4 *)h->wall_pts, (const int *)h->wall_cell, h->max_wall, (const int *)h->wall_c2,
                           (const int *)h->counts, (const int *)h->wcounts, c.tv, h->kw, h->cfg.map_res_x, h->cfg.map_res_y, (const float *)h->pose, c.hdr, seq,
                           PB(PB_WALLW));
        HIPCHK(hipGetLastError());
        // (gates: the next frame's first launch on this stream says so instead -- k_gate_signal; whoever else needs the tail records the event then)
        h->ftail_recorded = !c.ftail_gate;
        if (!c.ftail_gate) HIPCHK(hipEventRecord(h->ev_ftail, F));
    }
    h->pipe_live = true;
    h->plan_valid = false;
    h->cells_valid = true;
    h->mirror_stale = true;
    h->stats_clean = false;
    h->icp_delta_ready = false;
    h->scan_front_done = false;
    pfslam_handle::Frame fr{seq, frame, 0, true, true};
    fr.gtheta = c.multi; // (its header carries the JOB-wide |heading| maximum: k_theta_gmax)
    h->in_flight.push_back(fr);
    while ((int)h->in_flight.size() > (h->topo_in_step == 1 ? 0 : h->lag)) CHK(consume_frame(h));
    if (h->topo_in_step == 1) CHK(frame_topology(h, nullptr));
    return 0;
}
#undef FV_EDGE_WAIT

static int frame_v2(pfslam_handle *h, int frame, const float *scan_host, int used, int bpc)
{
    CHK(frame_v2_begin(h, frame, scan_host, used, bpc, /*sharded=*/false));
    CHK(frame_v2_score(h));
    CHK(frame_v2_chain(h));
    return frame_v2_finish(h);
}
#undef PB
