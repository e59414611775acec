// kd_cells.hip.inc -- lattice-cell rows: the round-3 organisation of the scan-match kernel (planar maps on the map lattice).
//
// Every point the SLAM step puts into the map is a cell centre k * res (ROUND_FRAC, kernel.cu:52; cell_to_point below), so every
// split plane of the KD tree is a lattice plane, and the chain of `query < node` decisions that IS the first descent of the
// reference traversal (kernel.cu:1239-1259) comes out the same for every query inside one lattice cell
//     [fl(Kx res), fl((Kx + 1) res))  x  [fl(Ky res), fl((Ky + 1) res)).
// A frame's 10^8 queries (100 k particles x 1081 beams) fall into ~2 x 10^4 cells -- thousands of queries per cell.  So, per
// frame and per cell that can be hit:
//   k_cells_mark   the lattice cells under the beam-end boxes of the waves (the box W of the round-2 plan: every lane's end point
//                  lies inside it by construction), marked in a dense window table around the cloud and appended to a list;
//   k_cell_rows    one lane per listed cell walks the cell's first descent ONCE -- 42 nodes on the aged bench map, 25 of them
//                  inserted since the last re-balance -- and keeps only the nodes that can be nearest for some point of the cell
//                  (the interval pruning of the round-2 plan with W = one 2.5 cm cell), each with the split plane of its parent;
//                  then, for every candidate, the re-descent the traversal would make from it (sibling side of the parent, path
//                  decided by the cell again) and the nodes on it that could still beat the best distance (usually none); finally
//                  the rows of the cell's four SUB-cells (the cell halved in x and y: same descent, tighter bounds) are cut out
//                  of that set, minus the candidates the corner test rules out (PF_CORNER_F): 1.24 candidates per row on average;
//   k_score_kd_cells  a lane computes its beam end point, finds its sub-cell's row with one 4-byte gather, evaluates the candidates
//                  (16-byte gathers that the lanes of a wave largely share) with the very arithmetic of the per-node visit, does
//                  the parent-hyperplane test arithmetically, looks at the re-descent candidates of its winner, and only when
//                  one of THOSE wins (~5 % of the queries) continues with the generic traversal (kd_resume) -- which is also
//                  what a lane does whose sub-cell has no row (outside the window, too many candidates, pool exhausted, NaN).
// Nothing here changes what is computed: a dropped node is provably farther than a kept one for every query of the cell (1e-5
// relative margins on both bounds), order is kept, and the lanes run the visit's own float arithmetic including the guard band.
// The per-lane node visits of the round-2 kernel that grew with the age of the map (2.5 per query after a re-balance, 11.4
// twenty frames later) are gone; what a query costs no longer depends on how many walls were inserted since the re-balance.

#define PF_CELL_SUB 2              /* sub-cells per lattice cell and axis (a power of two): rows are per SUB-cell */
#define PF_CELL_WIN (2560 * PF_CELL_SUB) /* window side in sub-cells: 64 m at 0.025 m -- 20 sqrt(2) m of beam either side of the cloud */
#define PF_CELL_LIST_CAP (1 << 19) /* cells claimed between two wipes: one 256-byte record each (PF_REC_WORDS) */
#define PF_CELL_POOL_CAP (1 << 22) /* 16-byte row slots between two wipes (64 MB; bump-allocated, a re-cut cell abandons its old slots) */
#define PF_CELL_MAXC 12            /* first-descent candidates per row */
#define PF_CELL_RUN 32             /* ... and while the path is walked: the bound U tightens on the way down, early nodes drop out late */
#define PF_CELL_MAXR 14            /* re-descent candidates per row (all owners together) */
#define PF_CELL_MARK_MAX 4096      /* cells of ONE group's box beyond which it is not marked (a cloud wider than the host's estimate said: generic
                                      lanes for that group -- the plain traversal's cost --, instead of tens of milliseconds of claims; round 5) */
#define PF_CELL_PENDING 0xFFFFFFFFu
#define PF_CELL_FALLBACK 0xFFFFFFFEu
// table entry of a row: bits 0-3 n1 (1 .. 12 first-descent candidates), bits 4-7 n2 (0 .. 14 re-descent candidates, 15 = they
// did not fit: generic tail), bits 8-29 first slot in the pool; bits 30-31 zero
//
// Round 4: the rows PERSIST across frames.  Between two re-balances the tree is append-only (KDTree::InsertNode, kdtree.cpp:69-105)
// and a row stores node indices and coordinates, never weights, so the rows of a lattice cell stay valid until a node is hung on a
// link that the cell's first descent or one of its re-descent walks ENDS on.  Every claimed cell keeps a 256-byte record (its
// cell-level candidates, the terminal link of the first descent and of every candidate's re-descent walk, the re-descent
// candidates, the bound U); k_cells_update looks at those links after every insert (k_test_new) -- a handful of independent
// gathers per cell --, EXTENDS the walks of the cells whose links received a node (a few hops instead of the ~70 of a walk from
// the root) and re-cuts their rows.  New cells are found by k_cells_mark and walked from the root once; in the frame loops both
// run on the aux stream UNDER the scan-match kernel (their queries take the generic traversal for that one frame: ~0.1 % of the
// (wave, beam) rows on the bench workload, tools/experiments/r04/persist_sim.c), so neither is on the frame's critical path.
// Table, records and pool are wiped by the host (set_map, re-balance, overflow, cloud far from the window centre): cells_wipe.
// cell state (ints, PF_CS_*): [0] cells claimed since the wipe (= records; list[r] is record r's table index)  [1] pool slots used
//   [2] the list's length when the last walk pass (k_cells_update<false>) started: in the frame loops the NEXT frame's marking pass
//   appends to the list while k_cells_update<true> runs, and an entry whose slot is counted but not yet written must not be read
//   [4] [5] capacity of the list and of the pool in use (<= PF_CELL_LIST_CAP / PF_CELL_POOL_CAP: the allocations; smaller in tests of the
//   overflow paths, PFSLAM_CELL_LIST_CAP / PFSLAM_CELL_POOL_CAP)  [128] [129] lattice index (in sub-cells) of the window's corner  [6] flags (PF_CF_*)  [8] live rows  [9] sum n1  [10] sum n2 (without
//   the 15s)  [11] sub-cells without a row (too many candidates, pool exhausted, or the four of a cell the full list refused)  [12 .. 15] since the wipe: cells walked from the root / extensions / looks that found a
//   cell unchanged / cells claimed (the last three grow with every pass)
enum { PF_CS_COUNT = 0, PF_CS_POOL, PF_CS_SNAP, PF_CS_PAD3, PF_CS_LIST_CAP, PF_CS_POOL_CAP, PF_CS_FLAGS, PF_CS_PAD, PF_CS_ROWS, PF_CS_N1, PF_CS_N2,
       PF_CS_NONE, PF_CS_CUR_FRESH, PF_CS_CUR_EXT, PF_CS_CUR_REUSED, PF_CS_CUR_CLAIMED, PF_CS_WORDS = 32,
       // The window's corner lives 512 bytes away from the counters: every wave of the scan-match kernel reads it, and in the frame
       // loops the marking pass runs BESIDE that kernel, adding to the list counter -- on the same 128-byte line the 131 k reads
       // queued behind those atomics and the scan-match kernel lost 27 us (0.373 -> 0.400 ms; found by elimination, with the cell passes made synchronous)
       PF_CS_OX = 128, PF_CS_OY = 129, PF_CS_ALLOC = 256 };
#define PF_CF_LIST_FULL 1   /* more cells claimed than PF_CELL_LIST_CAP: the rest takes the generic traversal until the wipe */
#define PF_CF_POOL_FULL 2   /* row pool exhausted */
#define PF_CF_NEED_ORIGIN 4 /* wiped: the next k_cell_count puts the window around the cloud */
#define PF_CF_FAR 8         /* the cloud's mean has left the middle of the window (beam ends start to fall outside it) */
#define PF_CELL_DRIFT_MAX 120 /* ... by this many lattice cells (3 m at 2.5 cm; the window reaches 32 m, a beam 28.3 m) */
// record of a claimed cell (ints): [0] U  [1] terminal link of the first descent (node * 2 + side)  [2] m | nr << 8 | flags << 16
// [3] the wipe generation it was written in (anything else: the cell has not been walked yet -- no counter, no ticket, no fence)
// [4 .. 19] terminal link of each candidate's re-descent walk (-1: none to watch)  [20 .. 35] cell-level candidates (path order)
// [36 .. 51] each candidate's parent node (-1: the root)  [52 .. 75] re-descent candidates, node | owner << 27.  384 bytes = three
// 128-byte lines, and the look at the links (every record, every frame) reads the first 80 bytes only: one line per record.
#define PF_REC_WORDS 96
#define PF_REC_TERM 4
#define PF_REC_CAND 20
#define PF_REC_PAR 36
#define PF_REC_RC 52
#define PF_REC_POOL 76 /* [76] first pool slot of the cell's four rows, [77] slots allocated: an extension re-cuts IN PLACE while the rows fit */
#define PF_REC_LAST 80 /* [80 .. 83] the four table words this record published last: what the next publication replaces (its accounts are
                          closed from here -- the table words themselves are then plain stores, not exchanges whose answer the wave waits for) */
#define PF_ROW_HEADROOM 2 /* slots allocated beyond what the first cut needs (0 / 1 / 4: no difference beyond the run-to-run noise, ab_row_grow.sh) */
#define PF_RF_FRESH 1 /* walked under the scan-match kernel: rows not cut yet */
#define PF_RF_DEAD 2  /* no rows until the next wipe (too many candidates, a non-finite node on the path) */
#define PF_RF_ROVER 4 /* re-descent candidates did not fit: rows say n2 = 15 (generic tail), re-descent links are not watched */

struct CellGeom { float resx, resy, invx, invy; };

// frame probe (pfslam_set_probe): the first thread of a launch stores the 100 MHz wall clock -- where a frame's time goes, read off the
// frame's own kernels (no profiler attached, no extra launches, no events); nullptr: nothing
__device__ __forceinline__ void pf_stamp(unsigned long long *__restrict__ slot)
{
    if (slot && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *slot = wall_clock64();
}

// Rows are built per SUB-cell: the lattice cell halved in x and y (sub-cell index S = 2 K + [q >= mid], mid = fl(fl(K res) + res / 2)).
// The descent's decisions are still those of the lattice cell -- a sub-cell only tightens the bounds the candidates are pruned
// with: 2.1 candidates per row instead of 3.7 (CPU prototype; 1.24 once the corner test below has had its say -- the sub-cell
// edges are the bisectors of neighbouring lattice points), and a wave's maximum ~2 instead of ~6.5, which is what the scan-match
// kernel pays for; 3.7 x as many rows to build.
// RANGE for which everything below is exact: lattice indices |k| < PF_LATTICE_KMAX = 2^20 cells per axis, at ANY resolution
// pfslam_create accepts (res > 0, 2 .. 16384 cells per map side) -- 26 km either side of the origin at 2.5 cm.  upload_tree checks
// every map point against it (a map with a point beyond it, or off the lattice, is scored with the round-2 plan); a QUERY beyond
// it lies outside the table's window (2560 cells around the cloud) or fails the finite / |q| < 1e6 tests and takes the generic
// traversal.  Why 2^20: fl(q * fl(1 / res)) carries two roundings, |error| <= |k| 2^-23 < 1/8 of a cell, so floor() is within one of
// the true index and the two exact comparisons of lattice_floor settle it; sub_index_fast's margin 3e-7 |t| + 1e-6 > 4 u |t| needs
// |t| = 2 |k| < 2^23 only for v_fract to be exact.  (float)k * res and the map's own points are the same float product.
#define PF_LATTICE_KMAX (1 << 20)
// max k with fl(k * res) <= q.  inv ~ 1 / res; q must be finite.
__host__ __device__ __forceinline__ int lattice_floor(float q, float res, float inv)
{
    int k = (int)floorf(q * inv);
    if ((float)(k + 1) * res <= q) k++;
    else if (!((float)k * res <= q)) k--;
    return k;
}

// index of q's sub-cell on one axis (monotone in q); sub_edges: the closed interval of sub-cell S and the lower edge of ITS lattice cell
__host__ __device__ __forceinline__ int sub_index(float q, float res, float inv)
{
    const int k = lattice_floor(q, res, inv);
    const float mid = (float)k * res + 0.5f * res;
    return PF_CELL_SUB * k + (q >= mid ? 1 : 0);
}
// The same index without the exact comparisons, for a query that is not too near a sub-cell edge.  t = fl(q * inv2), inv2 = 2 fl(1 / res):
// two roundings put t within (2 u + u^2) |tau| of tau = 2 q / res (u = 2^-24); the edges sub_index compares with -- fl(k res)
// for S = 2 k, fl(fl(k res) + res / 2) for S = 2 k + 1 -- lie, in the same units, within (2 u + u^2) |S| of S.  So when t is
// farther than PF_SUB_MARGIN |t| + 1e-6 (> 4 u |t|, with a quarter to spare) from both neighbouring integers, floor(t) IS
// sub_index(q): `clear` > 0.  t - floor(t) is exact.  ~0.1 % of the queries are not safe and take sub_index itself
// (tests/test_gpu_score.py checks both against each other around every edge of the window).
#define PF_SUB_MARGIN 3e-7f
__device__ __forceinline__ int sub_index_fast(float q, float inv2, float &clear)
{
    const float t = q * inv2;
    int k;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(k) : "v"(t)); // (int)floorf(t) in one instruction (saturating; 0 for a NaN)
    const float fr = __builtin_amdgcn_fractf(t);         // t - floor(t), exact (clamped below 1)
    // clear > 0: min(fr, 1 - fr) > PF_SUB_MARGIN |t| + 1e-6 -- safe.  Not so for a NaN, an infinity and any |t| >= 2^23 (fr = 0).
    clear = __builtin_fmaf(fabsf(t), -PF_SUB_MARGIN, 0.5f - 1e-6f) - fabsf(fr - 0.5f);
    return k;
}
__host__ __device__ __forceinline__ void sub_edges(int S, float res, float &lo, float &hi, float &cell_lo)
{
    const int k = S >> 1; // floor(S / 2), also for negative S
    cell_lo = (float)k * res;
    const float mid = cell_lo + 0.5f * res;
    lo = (S & 1) ? mid : cell_lo;
    hi = (S & 1) ? (float)(k + 1) * res : mid;
}
static_assert(PF_CELL_SUB == 2, "sub_index / sub_edges halve the lattice cell");

// Beam-end box of a group of 64 lanes for beam j (shared by the round-2 plan and the cell marking): W = pose box (+) the
// end point's range over the group's headings.  Egocentric end point at the centre heading (the lanes' own formula); d/dphi of
// (r cos phi, r sin phi) is (-r sin phi, r cos phi), and |sin|, |cos| are 1-Lipschitz: over the group's headings the end point
// moves by at most (|cy| + |r| d) d in x and (|cx| + |r| d) d in y; eps covers the lanes' float rounding and the 1-ulp sincos
// many times over, and the rounding of rot = angle + theta itself, which grows with |theta| (headings are never normalised):
// the centre and every lane each round their own sum to 0.5 ulp(|rot|) <= 2^-24 (|theta| + 2.36).
// The box is the SPECIFICATION's in both arithmetic modes (pfslam_set_trig): the marking pass does not look at the mode, eps covers the
// last-place differences of the device library's cosf / sinf, and a lane whose end point lands in a cell nobody marked finds no row there
// and takes the generic traversal (tests/test_gpu_devlib_frames.py, test_marking_pass_does_not_look_at_the_mode: same bookkeeping in
// either mode; the frames and scores of that file hold the device-library lanes to the reference's kernel on those rows).
// false: no box (non-finite or absurd geometry, NaN poses, or a beam no heading can accept: |r| >= PF_RANGE_NEVER).
// T / beams: the centre heading's parts (k_group_box) and the beam table -- the same end point for 15 double operations instead of
// two argument reductions and polynomials (a marking thread computes one per (group, beam)); nullptr: from scratch.
__device__ __forceinline__ bool beam_box(const pf::KdGroupBox &b, int j, float r, float &wxlo, float &wxhi, float &wylo, float &wyhi,
                                         const pf::AngleParts *T = nullptr, const pf::BeamParts *beams = nullptr)
{
    const float tc = 0.5f * (b.tlo + b.thi), dth = 0.5f * (b.thi - b.tlo);
    float cx, cy;
    if (T) beam_end_point(beams, j, r, tc, *T, cx, cy);
    else pf::clean_lidar_scan(j, r, tc, cx, cy);
    const float dd = dth + 1e-6f;
    const float eps = 2e-4f + 1e-5f * fabsf(r) + fabsf(r) * 2.0f * 1.1920929e-7f * (fabsf(tc) + 2.4f + dd);
    const float hx = (fabsf(cy) + fabsf(r) * dd) * dd + eps, hy = (fabsf(cx) + fabsf(r) * dd) * dd + eps;
    wxlo = b.xlo + cx - hx; wxhi = b.xhi + cx + hx; wylo = b.ylo + cy - hy; wyhi = b.yhi + cy + hy;
    return (wxlo == wxlo) && (wxhi == wxhi) && (wylo == wylo) && (wyhi == wyhi) && fabsf(wxlo) < 1e6f && fabsf(wxhi) < 1e6f &&
           fabsf(wylo) < 1e6f && fabsf(wyhi) < 1e6f && (wxhi - wxlo) < 4.0f && (wyhi - wylo) < 4.0f && fabsf(r) < PF_RANGE_NEVER;
}

// One workgroup per (beam, 2048 groups): the beam-end boxes of up to 2048 waves of the score kernel along ONE beam cover a
// compact patch of the lattice (an arc a few cells thick), so the workgroup collects their cells in an LDS bitmap over the
// patch's bounding rectangle -- no global traffic at all --, and only the distinct cells of the patch (~60 per beam) go to the
// window table: a plain look, a CAS where it says "empty", an append for the winner.  Adjacent beams overlap, hence the CAS.
#define PF_MARK_THREADS 256
#define PF_MARK_GROUPS 8            /* groups per thread (512 x 4: 39.4 us, 384 x 6: 38.9, 256 x 8: 36.7) */
#define PF_MARK_CLAIMS 2048         /* new cells one workgroup collects before it appends them with ONE atomic on the list counter */
#define PF_MARK_WORDS 4096          /* bitmap words: patches up to 131072 cells (e.g. 362 x 362); larger: straight to the table */
__global__ __launch_bounds__(PF_MARK_THREADS) void k_cells_mark(const pf::KdGroupBox *__restrict__ box, int groups,
                                                                const float *__restrict__ scan, int nb, CellGeom geo, unsigned *tab,
                                                                int *__restrict__ list, int *cs, const pf::AngleParts *__restrict__ gparts,
                                                                const pf::BeamParts *__restrict__ beams, unsigned long long *__restrict__ probe = nullptr)
{
    pf_stamp(probe);
    __shared__ unsigned bm[PF_MARK_WORDS];
    __shared__ int s_red[4][PF_MARK_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, j = blockIdx.x;
    const int ox = cs[PF_CS_OX], oy = cs[PF_CS_OY];
    const float r = scan[j];
    int kx0[PF_MARK_GROUPS], kx1[PF_MARK_GROUPS], ky0[PF_MARK_GROUPS], ky1[PF_MARK_GROUPS];
    int ux0 = INT_MAX, ux1 = INT_MIN, uy0 = INT_MAX, uy1 = INT_MIN;
#pragma unroll
    for (int q = 0; q < PF_MARK_GROUPS; q++) {
        const int g = blockIdx.y * (PF_MARK_THREADS * PF_MARK_GROUPS) + q * PF_MARK_THREADS + t;
        kx0[q] = ky0[q] = INT_MAX;
        kx1[q] = ky1[q] = INT_MIN;
        if (g < groups) {
            float wxlo, wxhi, wylo, wyhi;
            const pf::AngleParts T = gparts[g];
            if (beam_box(box[g], j, r, wxlo, wxhi, wylo, wyhi, &T, beams)) {
                // marked per LATTICE cell (window coordinates in cells; the origin is a whole cell: even in sub-cell units)
                const int okx = ox >> 1, oky = oy >> 1, wk = PF_CELL_WIN / PF_CELL_SUB;
                const int a0 = max(lattice_floor(wxlo, geo.resx, geo.invx) - okx, 0), a1 = min(lattice_floor(wxhi, geo.resx, geo.invx) - okx, wk - 1);
                const int b0 = max(lattice_floor(wylo, geo.resy, geo.invy) - oky, 0), b1 = min(lattice_floor(wyhi, geo.resy, geo.invy) - oky, wk - 1);
                // (a box of more than PF_CELL_MARK_MAX cells is not marked at all: the gate that chose the cell rows -- the host's estimate of the
                // cloud's spread, one frame old or from the first 1024 particles of pfslam_set_particles -- was wrong about this group)
                if (a0 <= a1 && b0 <= b1 && (long long)(a1 - a0 + 1) * (b1 - b0 + 1) <= PF_CELL_MARK_MAX) { // not entirely outside the window
                    kx0[q] = a0; kx1[q] = a1; ky0[q] = b0; ky1[q] = b1;
                    ux0 = min(ux0, a0); ux1 = max(ux1, a1); uy0 = min(uy0, b0); uy1 = max(uy1, b1);
                }
            }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        ux0 = min(ux0, __shfl_xor(ux0, off, 64)); ux1 = max(ux1, __shfl_xor(ux1, off, 64));
        uy0 = min(uy0, __shfl_xor(uy0, off, 64)); uy1 = max(uy1, __shfl_xor(uy1, off, 64));
    }
    if (lane == 0) { s_red[0][wave] = ux0; s_red[1][wave] = ux1; s_red[2][wave] = uy0; s_red[3][wave] = uy1; }
    __syncthreads();
    for (int k = 0; k < PF_MARK_THREADS / 64; k++) {
        ux0 = min(ux0, s_red[0][k]); ux1 = max(ux1, s_red[1][k]); uy0 = min(uy0, s_red[2][k]); uy1 = max(uy1, s_red[3][k]);
    }
    if (ux0 > ux1) return; // no group of this workgroup has a box for this beam
    const int nx = ux1 - ux0 + 1;
    const long long bits = (long long)nx * (uy1 - uy0 + 1);
    // table word `idx` belongs to the pass: the first claimant appends it.  Appends are collected per workgroup (one atomic on the
    // list counter per workgroup: 25 k same-address atomics per pass cost more than everything else in this kernel)
    __shared__ int s_claim[PF_MARK_CLAIMS];
    __shared__ int s_nclaim, s_base;
    if (t == 0) s_nclaim = 0;
    __syncthreads();
    auto claim = [&](int idx) {
        // straight to the CAS (one trip to memory, not a look and then a CAS: the table is far larger than the L2).  The table
        // persists: a word that is not zero belongs to a cell claimed in an earlier pass (rows, pending or none) -- nothing to do
        if (atomicCAS(&tab[idx], 0u, PF_CELL_PENDING) == 0u) {
            const int k = atomicAdd(&s_nclaim, 1);
            if (k < PF_MARK_CLAIMS) s_claim[k] = idx;
            else { // more new cells than the workgroup can hold: append one by one
                const int pos = atomicAdd(&cs[PF_CS_COUNT], 1);
                // (booked like the collected ones: which workgroup wins a cell is a race, so a count that left these out differed from run
                // to run wherever a workgroup overflowed -- tests/test_gpu_observers.py compares it between runs)
                atomicAdd(&cs[PF_CS_CUR_CLAIMED], 1);
                if (pos < cs[PF_CS_LIST_CAP]) list[pos] = idx;
                else { // list full: the cell gets no row until the next wipe
                    atomicExch(&tab[idx], PF_CELL_FALLBACK);
                    atomicOr(&cs[PF_CS_FLAGS], PF_CF_LIST_FULL);
                    atomicAdd(&cs[PF_CS_NONE], PF_CELL_SUB * PF_CELL_SUB); // its sub-cells go without rows (no record: nobody unbooks them)
                }
            }
        }
    };
    auto flush = [&]() { // all threads
        __syncthreads();
        const int nc = min(s_nclaim, PF_MARK_CLAIMS);
        if (t == 0 && nc > 0) {
            s_base = atomicAdd(&cs[PF_CS_COUNT], nc);
            atomicAdd(&cs[PF_CS_CUR_CLAIMED], nc);
        }
        __syncthreads();
        for (int k = t; k < nc; k += PF_MARK_THREADS) {
            const int pos = s_base + k;
            if (pos < cs[PF_CS_LIST_CAP]) list[pos] = s_claim[k];
            else {
                atomicExch(&tab[s_claim[k]], PF_CELL_FALLBACK);
                atomicOr(&cs[PF_CS_FLAGS], PF_CF_LIST_FULL);
                atomicAdd(&cs[PF_CS_NONE], PF_CELL_SUB * PF_CELL_SUB);
            }
        }
    };
    if (bits > (long long)PF_MARK_WORDS * 32) { // a cloud this wide: every box straight to the table
#pragma unroll
        for (int q = 0; q < PF_MARK_GROUPS; q++) {
            if (kx0[q] > kx1[q] || (long long)(kx1[q] - kx0[q] + 1) * (ky1[q] - ky0[q] + 1) > PF_CELL_MARK_MAX) continue; // absurd: generic lanes
            for (int cy = ky0[q]; cy <= ky1[q]; cy++)
                for (int cx = kx0[q]; cx <= kx1[q]; cx++) claim(2 * cy * PF_CELL_WIN + 2 * cx);
        }
        flush();
        return;
    }
    const int words = (int)((bits + 31) >> 5);
    for (int w = t; w < words; w += PF_MARK_THREADS) bm[w] = 0u;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PF_MARK_GROUPS; q++)
        for (int cy = ky0[q]; cy <= ky1[q]; cy++) { // empty box: ky0 > ky1.  One row of the box = a run of bits: a word mask at a time
            const int b0 = (cy - uy0) * nx - ux0 + kx0[q], b1 = b0 + (kx1[q] - kx0[q]); // first and last bit of the run
            for (int w = b0 >> 5; w <= (b1 >> 5); w++) {
                const int lo = max(b0 - (w << 5), 0), hi = min(b1 - (w << 5), 31);
                const unsigned m = (0xFFFFFFFFu >> (31 - hi)) & (0xFFFFFFFFu << lo);
                if ((bm[w] & m) != m) atomicOr(&bm[w], m);
            }
        }
    __syncthreads();
    // one BIT per thread and round (not one word: the set bits of a word are neighbouring cells, and a claim is a chain of two
    // dependent trips to memory -- 32 of them in a row on one thread was the whole duration of this kernel)
    for (int bit = t; bit < (int)bits; bit += PF_MARK_THREADS)
        if ((bm[bit >> 5] >> (bit & 31)) & 1u) {
            const int cy = bit / nx;
            claim(2 * (uy0 + cy) * PF_CELL_WIN + 2 * (ux0 + (bit - cy * nx))); // the cell's claim word: its sub-cell (0, 0)
        }
    flush();
}

// One lane per claimed LATTICE cell: the rows of its four sub-cells.  The sub-cells share the cell's first descent and its
// re-descent paths -- only the bounds differ --, so the chain of dependent node reads is walked ONCE per lattice cell, pruning with
// the cell's own box (a superset of what any sub-cell keeps: lb_cell <= lb_sub, U_sub <= U_cell), and the four rows are cut out of
// that set at the end.
// The corner test.  Candidate a of a (sub-)cell is useless when ONE other candidate c is nearer for every query the row serves:
// |q - a|^2 - (1 + eps) |q - c|^2 is concave in q, so it is positive on a whole rectangle when it is at the four corners.  The
// rectangle is the (sub-)cell WITHOUT its edges -- [lo+, hi-] in x and y, lo+ / hi- the neighbouring floats: a query exactly on a
// low edge gets no row in the score kernel (it takes the generic traversal; the high edge belongs to the next cell) -- because the
// edges ARE the bisectors of neighbouring lattice points: on them two candidates tie, a float apart from them one is nearer by a
// relative 8 ulp(q) / res of the squared distance, 2e-5 and more.  Margins: the squared distances here and the lanes' own carry
// 4 u each (u = 2^-24: difference, two squares, sum); the lanes compare sqrt_rn's, which separates squares 2^-21 apart.  So the
// test D~c < D~a (1 - 4e-6) guarantees Dc (1 + 3.4e-6) < Da at the corners, hence everywhere, hence
// s~a > s~c (1 + 3.4e-6 - 8 u) > s~c (1 + 2^-21): c beats a in the lanes' own arithmetic wherever it is visited, a never ends as
// the best node, and neither a nor the re-descent candidates it owns are of any use to the row.
//
// Persistence (round 4).  What a record keeps is a SUPERSET argument: a row must list, in path order, every node that can end a
// query's first descent as its best node (and, per such node, every node of its re-descent walk that can still win); listing more is
// harmless -- the lanes evaluate every listed node with the visit's own arithmetic.  Appending to the tree only ever appends to
// those walks (a node hung on the link a walk ended on, and whatever hangs below it), and the bound U only tightens, so an
// EXTENSION keeps every candidate the record holds (its position too: the re-descent entries name their owner by position), walks on
// from the child of the terminal link, adds the new nodes that pass the interval test and the cell-level corner test, and re-cuts
// the four rows.  Which cells have to be extended is found by looking: the terminal links of every record are read after every
// insert (independent gathers; a link that still has no child has not changed).
#define PF_CORNER_F 0.999996f
#define PF_CELL_MAXU 16  /* candidates of a lattice cell = the union of its sub-cells' */
#define PF_CELL_MAXRU 24 /* re-descent candidates of a lattice cell */
static_assert(PF_REC_RC + PF_CELL_MAXRU <= PF_REC_POOL && PF_REC_POOL + 2 <= PF_REC_LAST && PF_REC_LAST + 4 <= PF_REC_WORDS && PF_REC_CAND == PF_REC_TERM + PF_CELL_MAXU && PF_REC_PAR == PF_REC_CAND + PF_CELL_MAXU && PF_REC_RC == PF_REC_PAR + PF_CELL_MAXU, "record layout");
// the child hanging on link = node * 2 + side (side 1 = right); -1: none.  A planar z level keeps its right child in both hot links
// and its true left child (which only a re-descent can reach, and which never gains a node: 0 < 0 is false) in the z array.
__device__ __forceinline__ int link_child(const pf::KdView &t, int link)
{
    const int a = link >> 1;
    const uint4 nd = t.hot[a];
    if ((link & 1) == 0 && t.planar && (nd.z >> 30) == 2u) return __float_as_int(t.z[a]);
    return (link & 1) ? (int)nd.w : pf::hot_left(nd.z);
}
#define PF_CELL_FILTER_WORDS 1024
__device__ __forceinline__ unsigned pf_link_hash(int link) { return ((unsigned)link * 2654435761u) >> 17; } // 15 bits
// the same for a WATCHED link: never the left link of a planar z level (that one cannot gain a node and is recorded as -1), so the
// child is in the hot record itself -- no dependent second read, and the 1 + m looks of a record are in flight together
__device__ __forceinline__ int watched_child(const pf::KdView &t, int link)
{
    const uint4 nd = t.hot[link >> 1];
    return (link & 1) ? (int)nd.w : pf::hot_left(nd.z);
}
// PUBLISH false: the claimed cells that have no record of this generation yet are walked from the root and their records written,
// flagged fresh; table and pool are not touched (the scan-match kernel may be running: frame loops, cell stream).
// PUBLISH true: every record is looked at.  No record yet: walked from the root.  Otherwise the terminal links are read; a cell
// one of whose links has gained a child is extended.  New, extended and fresh cells get their four rows cut and published.
// One wave per workgroup.  (A "last workgroup" ticket that kept a walked-up-to counter cost more than the whole look: its
// agent-scope fence is an L2 write-back + invalidate per workgroup, and a scan-match kernel running beside it lost 60 us to that.)
#ifdef PF_CELLS_PROFILE /* phase stamps of k_cells_update<true> (10 ns units): cs[64 + 2 p] sum over waves, cs[65 + 2 p] max; cs[63] waves */
#define PF_STAMP(p)                                                                      \
    do {                                                                                 \
        if (PUBLISH) {                                                                   \
            const long long now_ = (long long)wall_clock64();                            \
            if (lane == 0) {                                                             \
                atomicAdd(&cs[64 + 2 * (p)], (int)(now_ - t_prev_));                     \
                atomicMax(&cs[65 + 2 * (p)], (int)(now_ - t_prev_));                     \
            }                                                                            \
            t_prev_ = now_;                                                              \
        }                                                                                \
    } while (0)
#else
#define PF_STAMP(p)
#endif
// Round 5 (pfslam_frame.hip.inc): which records a pass may touch is a RANGE handed over through device words, never a guess from the
// list counter (the marking pass of the next frame bumps that counter before it writes the entries):
//   walk pass (PUBLISH false)   records [*lo, count) -- what the marking passes since the previous walk claimed --, walked on the tree AS
//                               IT WAS with *bound nodes (children >= *bound are ignored: the frame's insert may run beside the walk, so
//                               the insert does not have to wait for it); count is left in *w_out for the passes that follow;
//   publishing pass             records [0, *hi): walked by a walk pass that is ORDERED before this launch (an event chain, see the
//                               stream table in DESIGN.md), `lag` frames ago.  A record a walk left FRESH was made on an older tree: its
//                               links are validated by reading them (not through the filter of THIS frame's insert).
// all null: the round-4 behaviour (every record up to the counter / the snapshot; stage-level calls, the sharded frame).
// fault (tests only, PFSLAM_FAULT at creation): 1 = a publishing pass ignores *hi (the round-4 race: it then reads list slots the marking
// pass beside it has counted but not written, and records no walk pass has finished); 2 = it does not validate a FRESH record's links
// (rows of a bounded walk published as they were made: stale wherever the tree has grown since).  tests/test_gpu_frame.py shows that the
// bookkeeping comparison / pfslam_debug_check_cells catch both.
struct CellPass { const int *lo; int *w_out; const int *hi; const int *bound; int fault; };
template <bool PUBLISH>
__global__ __launch_bounds__(64) void k_cells_update(pf::KdView tree, CellGeom geo, unsigned *tab, const int *__restrict__ list, int *cs,
                                                     uint4 *__restrict__ pool, int *rec_base, int gen, const int *__restrict__ touched, int pass = 0, int recut = 0, int use_snap = 0,
                                                     CellPass cp = CellPass{nullptr, nullptr, nullptr, nullptr, 0}, unsigned long long *__restrict__ probe = nullptr,
                                                     int *__restrict__ signal_word = nullptr, int signal_ticket = 0)
{
    pf_stamp(probe);
    // stream gates (pfslam_frame.hip.inc): the insert in front of this launch is complete and visible -- say so for the other streams
    if (signal_word && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(signal_word, signal_ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    // LDS: 184 words per lane (47 KB per wave: three waves per CU).  The running list of a walk from the root (32 nodes + their
    // lower bounds) is dead once the final pruning has left at most 16 candidates in its first 16 places: the candidates' coordinates
    // and parent axes move in behind them.  (With every array on its own -- and 16 KB of corner distances, now recomputed -- a wave
    // took 78 KB and a CU held ONE: the 476 waves of a look at 30 k records ran in two rounds, 56 us.)
    __shared__ int lds[184][64];
#define S_IDX(k) lds[(k)][lane]                        /* [0, 32): running list / candidates (node indices) */
#define S_LB(k) (*(float *)&lds[32 + (k)][lane])       /* [32, 64): lower bounds of the running list */
#define S_CX(k) (*(float *)&lds[16 + (k)][lane])       /* after the final pruning: the candidates' coordinates ... */
#define S_CY(k) (*(float *)&lds[32 + (k)][lane])
#define S_PP(k) (*(uint32_t *)&lds[48 + (k)][lane])    /* ... parent axis << 30 of every candidate (3 = no parent) */
#define S_PC(k) (*(float *)&lds[64 + (k)][lane])       /* the parent's split coordinate */
#define S_CT(k) lds[80 + (k)][lane]                    /* terminal link of every candidate's re-descent walk; <= -2: -(child it has gained) - 2 */
#define S_PI(k) lds[96 + (k)][lane]                    /* every candidate's parent node */
#define S_R(k) lds[112 + (k)][lane]                    /* re-descent candidates: node | owning candidate << 27 */
#define S_RX(k) (*(float *)&lds[136 + (k)][lane])
#define S_RY(k) (*(float *)&lds[160 + (k)][lane])
    static_assert(PF_CELL_RUN == 32 && PF_CELL_MAXU == 16 && PF_CELL_MAXRU == 24, "LDS layout of k_cells_update");
    // The links that gained a node in the insert this update follows (k_test_new lists them: touched[0] entries from touched[1] on)
    // as a 32 k-bit filter in LDS: a record's 1 + m watched links are looked up THERE, and only a hit is confirmed by reading the
    // node -- reading every watched link's node instead (150 k scattered 16-byte gathers per frame, all waves at once, into an L2
    // the kernel boundary has just invalidated) was what the whole kernel waited for: 5 us of a wave's 23 on average, 30 at worst,
    // and every later phase queued behind that storm.  touched == nullptr: no insert since the last update -- nothing has changed.
    __shared__ unsigned s_filter[PF_CELL_FILTER_WORDS];
    const int n_touched = (PUBLISH && touched) ? touched[0] : 0;
    if (PUBLISH && n_touched > 0) {
        for (int w = threadIdx.x; w < PF_CELL_FILTER_WORDS; w += 64) s_filter[w] = 0u;
        __syncthreads();
        for (int k = threadIdx.x; k < n_touched; k += 64) {
            const unsigned hsh = pf_link_hash(touched[1 + k]);
            atomicOr(&s_filter[hsh >> 5], 1u << (hsh & 31));
        }
        __syncthreads();
    }
    auto maybe_touched = [&](int link) -> bool {
        const unsigned hsh = pf_link_hash(link);
        return (s_filter[hsh >> 5] >> (hsh & 31)) & 1u;
    };
    const int lane = threadIdx.x;
    // PUBLISH false runs between two marking passes (same stream): the list is complete up to the counter, which it leaves as a
    // snapshot.  PUBLISH true, in a frame loop, may run beside the next frame's marking pass, which bumps the counter BEFORE it writes
    // the entries: only records below the snapshot are looked at (the rest: next frame's walk pass).
    int count = min(cs[PF_CS_COUNT], cs[PF_CS_LIST_CAP]);
    // use_snap 2: a synchronous publishing pass (behind its marking pass on the same stream: the list is complete) leaves the snapshot too,
    // so that the publishing pass behind the frame's insert -- which may run beside the NEXT frame's marking pass -- always has one
    if ((!PUBLISH || use_snap == 2) && threadIdx.x == 0) cs[PF_CS_SNAP] = count; // (every workgroup stores the same value)
    if (PUBLISH && use_snap == 1) count = min(count, cs[PF_CS_SNAP]);
    if (PUBLISH && cp.hi && cp.fault != 1) count = min(count, *cp.hi);
    const int first = (!PUBLISH && cp.lo) ? min(*cp.lo, count) : 0;
    const int bound = cp.bound ? *cp.bound : 0x7fffffff;
    // (every workgroup stores the same value; *lo and *w_out are different words: a late workgroup still reads the old *lo)
    if (cp.w_out && threadIdx.x == 0) *cp.w_out = count;
    const int ox = cs[PF_CS_OX], oy = cs[PF_CS_OY];
    int st_rows = 0, st_n1 = 0, st_n2 = 0, st_none = 0, st_fresh = 0, st_ext = 0, st_reused = 0; // one atomic per wave and counter at the end
#ifdef PF_CELLS_PROFILE
    long long t_prev_ = (long long)wall_clock64();
    const long long t_start_ = t_prev_;
    if (PUBLISH && lane == 0 && blockIdx.x * 64 < count) atomicAdd(&cs[63], 1);
#endif
    // squared distance range of a box to a node (1e-5 relative margins, as in the round-2 plan)
    auto bounds = [](float xlo, float xhi, float ylo, float yhi, float nx, float ny, float &lb, float &ub) {
        const float dxn = fmaxf(fmaxf(xlo - nx, nx - xhi), 0.0f), dyn = fmaxf(fmaxf(ylo - ny, ny - yhi), 0.0f);
        const float dxf = fmaxf(fabsf(nx - xlo), fabsf(nx - xhi)), dyf = fmaxf(fabsf(ny - ylo), fabsf(ny - yhi));
        lb = (dxn * dxn + dyn * dyn) * 0.99999f;
        ub = (dxf * dxf + dyf * dyf) * 1.00001f;
    };
    // squared distances of a candidate to the four corners of a rectangle (the corner test; the very expressions the LDS copy held)
    auto corner4 = [](float px, float py, float ixlo, float ixhi, float iylo, float iyhi, float d[4]) {
        const float x0 = (px - ixlo) * (px - ixlo), x1 = (px - ixhi) * (px - ixhi), y0 = (py - iylo) * (py - iylo), y1 = (py - iyhi) * (py - iyhi);
        d[0] = x0 + y0; d[1] = x1 + y0; d[2] = x0 + y1; d[3] = x1 + y1;
    };
    // the accounts of a table word that is being replaced
    auto unbook = [&](unsigned old) {
        if (old == PF_CELL_FALLBACK) st_none--;
        else if (old != 0u && old < 0x40000000u) {
            st_rows--;
            st_n1 -= (int)(old & 15u);
            st_n2 -= ((old >> 4) & 15u) == 15u ? 0 : (int)((old >> 4) & 15u);
        }
    };
    // the loop is wave-uniform (lanes without work idle through an iteration): the pool allocation below is wave-aggregated
    for (int base = first + blockIdx.x * 64; base < count; base += gridDim.x * 64) {
        const int r = base + lane;
        const bool in = r < count;
        int *rec = rec_base + (size_t)(in ? r : 0) * PF_REC_WORDS;
        const int4 hd = in ? *(const int4 *)rec : make_int4(0, 0, 0, gen);
        // PUBLISH: the rest of the record and the cell's table index are requested WITH the header.  A touched record's look (links),
        // state (candidates, parents, re-descent list, slots) and cell were three dependent trips to memory -- header -> links, ballot ->
        // state, -> list entry -- on the frame's critical chain; they are one now (7 MB per pass of records nobody goes on to use: nothing
        // at this kernel's occupancy).  The walk pass keeps the lazy form: it runs beside the scan-match kernel, off the chain.
        int4 pre_ct[4], pre_cand[4], pre_par[4], pre_rc[6];
        int2 pre_pool = make_int2(0, 0);
        int4 pre_last = make_int4(0, 0, 0, 0);
        int pre_cell = 0;
        constexpr bool HOIST = PUBLISH;
        if (HOIST) {
#pragma unroll
            for (int q = 0; q < 4; q++) pre_ct[q] = pre_cand[q] = pre_par[q] = make_int4(-1, -1, -1, -1);
#pragma unroll
            for (int q = 0; q < 6; q++) pre_rc[q] = make_int4(0, 0, 0, 0);
            if (in) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    pre_ct[q] = *(const int4 *)(rec + PF_REC_TERM + 4 * q);
                    pre_cand[q] = *(const int4 *)(rec + PF_REC_CAND + 4 * q);
                    pre_par[q] = *(const int4 *)(rec + PF_REC_PAR + 4 * q);
                }
#pragma unroll
                for (int q = 0; q < 6; q++) pre_rc[q] = *(const int4 *)(rec + PF_REC_RC + 4 * q);
                pre_pool = *(const int2 *)(rec + PF_REC_POOL);
                pre_last = *(const int4 *)(rec + PF_REC_LAST);
                pre_cell = list[r];
            }
        }
        const bool scratch = in && hd.w != gen; // never walked: from the root
        bool work = scratch;
        int m_old = 0, nr = 0, rflags = 0, term0 = -1, child0 = -1;
        float U = INFINITY; // upper bound (with margin) of the final minimum for every point of the cell
        if (PUBLISH && in && !scratch) {
            U = __int_as_float(hd.x);
            term0 = hd.y;
            m_old = hd.z & 0xff;
            nr = (hd.z >> 8) & 0xff;
            rflags = hd.z >> 16;
            if (!(rflags & PF_RF_DEAD)) {
                // has one of the walks been appended to?  its terminal link then has a child (1 + m independent gathers)
                int ct[PF_CELL_MAXU];
#pragma unroll
                for (int q = 0; q < PF_CELL_MAXU / 4; q++) {
                    const int4 v = HOIST ? pre_ct[q] : *(const int4 *)(rec + PF_REC_TERM + 4 * q);
                    ct[4 * q] = v.x; ct[4 * q + 1] = v.y; ct[4 * q + 2] = v.z; ct[4 * q + 3] = v.w;
                }
                // (a first descent never ends on a z level's left link: it always goes right there)
                // (a FRESH record of a bounded walk was made on an older tree than the one this frame's insert touched: read its links)
                const bool direct = (rflags & PF_RF_FRESH) != 0 && cp.fault != 2;
                bool changed = false;
                if (direct || n_touched > 0) {
                    if (direct || maybe_touched(term0)) child0 = watched_child(tree, term0);
                    changed = child0 >= 0;
                }
#pragma unroll
                for (int k = 0; k < PF_CELL_MAXU; k++)
                    if (k < m_old) {
                        int c = -1;
                        if (ct[k] >= 0 && (direct || (n_touched > 0 && maybe_touched(ct[k])))) c = watched_child(tree, ct[k]);
                        S_CT(k) = c >= 0 ? -c - 2 : ct[k]; // the walk goes on from the child: the old link is not needed then
                        changed |= c >= 0;
                    }
                work = changed || (rflags & PF_RF_FRESH) != 0 || recut != 0; // (recut: every cell's rows are cut again, compactly)
                if (changed && !(rflags & PF_RF_FRESH)) st_ext++;
                if (!work) st_reused++;
            }
        }
        PF_STAMP(0); // the look at the links
        if (__builtin_amdgcn_ballot_w64(work) == 0ull) continue; // nothing to do for this wave's 64 cells
        const bool active = in && work;
        if (!active) m_old = nr = 0; // an idle lane's loops below must not run on what it read of its record
        if (active && scratch) st_fresh++; // walked from the root (counted once: a fresh record that is only cut here was counted then)
        const int cell = HOIST ? pre_cell : (in ? list[r] : 0); // table index of the cell's sub-cell (0, 0): even coordinates
        const int cyw = cell / PF_CELL_WIN, cxw = cell - cyw * PF_CELL_WIN;
        const int Kx = (ox + cxw) >> 1, Ky = (oy + cyw) >> 1;
        const float cxlo = (float)Kx * geo.resx, cxhi = (float)(Kx + 1) * geo.resx, xmid = cxlo + 0.5f * geo.resx;
        const float cylo = (float)Ky * geo.resy, cyhi = (float)(Ky + 1) * geo.resy, ymid = cylo + 0.5f * geo.resy;
        // the record's state: its candidates keep their places (lower bound 0: never dropped), the walks go on where they ended
        int n = 0, old_off = 0, old_len = 0;
        if (active && !scratch) {
            old_off = HOIST ? pre_pool.x : rec[PF_REC_POOL];
            old_len = recut ? 0 : (HOIST ? pre_pool.y : rec[PF_REC_POOL + 1]); // (a compaction pass: the pool starts over, nothing stays in place)
#pragma unroll
            for (int g4 = 0; g4 < PF_CELL_MAXU / 4; g4++) { // (the terminal links: by the look at the links above)
                const int k0 = 4 * g4;
                if (k0 < m_old) {
                    const int4 ci = HOIST ? pre_cand[g4] : *(const int4 *)(rec + PF_REC_CAND + k0);
                    const int4 pi = HOIST ? pre_par[g4] : *(const int4 *)(rec + PF_REC_PAR + k0);
                    const int cv[4] = {ci.x, ci.y, ci.z, ci.w}, pv[4] = {pi.x, pi.y, pi.z, pi.w};
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (k0 + q < m_old) {
                            S_IDX(k0 + q) = cv[q];
                            S_LB(k0 + q) = 0.0f;
                            S_PI(k0 + q) = pv[q];
                        }
                }
            }
#pragma unroll
            for (int g4 = 0; g4 < PF_CELL_MAXRU / 4; g4++) {
                const int k0 = 4 * g4;
                if (k0 < nr) {
                    const int4 rv = HOIST ? pre_rc[g4] : *(const int4 *)(rec + PF_REC_RC + k0);
                    const int rw[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (k0 + q < nr) S_R(k0 + q) = rw[q];
                }
            }
            n = m_old;
        }
        // query < node on a lattice plane, for every query of the lattice cell: the cell's lower edge decides (fl(k res) is monotone in k)
        int head = !active ? -1 : scratch ? 0 : child0;
        bool give_up = false;
        uint4 nd = tree.hot[max(head, 0)];
        while (head >= 0) {
            // both children are requested before this node is worked on: the kernel is one chain of dependent reads per lane, and
            // the node's own arithmetic (bounds, list) now runs under the next read instead of in front of it
            int cl = pf::hot_left(nd.z), cr = (int)nd.w;
            if (cl >= bound) cl = -1; // (a bounded walk: the tree as it was with `bound` nodes)
            if (cr >= bound) cr = -1;
            uint4 ndl = nd, ndr = nd;
            if (cl >= 0) ndl = tree.hot[cl]; // (a leaf -- where every extension ends -- requests nothing: one trip to memory less)
            if (cr >= 0) ndr = tree.hot[cr];
            const float nx = __uint_as_float(nd.x), ny = __uint_as_float(nd.y);
            const uint32_t axis = nd.z >> 30;
            if (!(fabsf(nx) < 1e6f && fabsf(ny) < 1e6f)) { give_up = true; break; } // a non-finite node (uploaded, or inserted under an infinite pose; a NaN pose inserts none): no rows
            float lb, ub;
            bounds(cxlo, cxhi, cylo, cyhi, nx, ny, lb, ub);
            U = fminf(U, ub);
            if (lb <= U) { // may be the nearest for some query of the cell
                if (n == PF_CELL_RUN) { // full: drop what the tighter U has ruled out meanwhile
                    int m = 0;
                    for (int k = 0; k < PF_CELL_RUN; k++) {
                        const int ci = S_IDX(k);
                        const float cl = S_LB(k);
                        if (cl <= U) {
                            S_IDX(m) = ci;
                            S_LB(m) = cl;
                            m++;
                        }
                    }
                    n = m;
                    if (n == PF_CELL_RUN) { give_up = true; break; }
                }
                S_IDX(n) = head;
                S_LB(n) = lb;
                n++;
            }
            const bool lt = axis == 0 ? cxlo < nx : (axis == 1 ? cylo < ny : false); // planar z levels: both links hold the right child
            term0 = head * 2 + (lt ? 0 : 1);
            head = lt ? cl : cr;
            nd = lt ? ndl : ndr;
        }
        PF_STAMP(1); // record state + first descent
        int m = 0; // final pruning with the final U (the record's candidates stay: lower bound 0, and they come first)
        if (!give_up)
            for (int k = 0; k < n; k++)
                if (S_LB(k) <= U) S_IDX(m++) = S_IDX(k);
        bool dead = active && (give_up || m == 0 || m > PF_CELL_MAXU);
        if (dead || !active) m = 0; // the loops below idle
        if (dead) m_old = nr = 0;
        // One round of reads, four entries of each kind in flight: the candidates' coordinates (the new ones' parent links with
        // them), the recorded candidates' parents (their split planes go into the rows: the lanes' parent-hyperplane test), the
        // recorded re-descent candidates' coordinates
        auto parent_plane = [&](int k, const uint4 pn) {
            const uint32_t paxis = pn.z >> 30;
            const bool none = S_PI(k) < 0; // no parent (H1: the search stops)
            S_PP(k) = none ? 3u << 30 : paxis << 30;
            S_PC(k) = none ? 0.0f : __uint_as_float(paxis == 0 ? pn.x : pn.y); // unused for a z level (hyperplane distance 0)
        };
        for (int k0 = 0; k0 < max(m, nr); k0 += 4) {
            uint4 cn[4], pn[4], rn[4];
            int par[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int k = k0 + q;
                if (k < m) {
                    const int ci = S_IDX(k);
                    cn[q] = tree.hot[ci];
                    if (k >= m_old) par[q] = tree.parent[ci];
                    else pn[q] = tree.hot[max(S_PI(k), 0)];
                }
                if (k < nr) rn[q] = tree.hot[S_R(k) & 0x7ffffff];
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int k = k0 + q;
                if (k < m) {
                    S_CX(k) = __uint_as_float(cn[q].x);
                    S_CY(k) = __uint_as_float(cn[q].y);
                    if (k >= m_old) S_PI(k) = par[q];
                    else parent_plane(k, pn[q]);
                }
                if (k < nr) {
                    S_RX(k) = __uint_as_float(rn[q].x);
                    S_RY(k) = __uint_as_float(rn[q].y);
                }
            }
        }
        PF_STAMP(2); // the round of reads
        // ... then the pruning of the whole set: the record's candidates against the bound U (it may have tightened: their lower bounds
        // are not kept, the coordinates just read give them again), and the corner test on the whole lattice cell (see the sub-cells
        // below): a candidate another one beats at the cell's four corners is of no use to any sub-cell -- a new one's parent and
        // re-descent path need not be read at all, a recorded one's link need not be watched any longer.  Without this a record
        // only ever grew: cells next to a wall that gains points every frame reached 16 candidates, and what the corner tests of
        // the cut cost grows with the square of that -- the slowest wave of the kernel took 50-90 us for a mean of 23.
        if (m > 0 && (m > 1 || m_old > 0)) {
            const uint32_t mask = (1u << m) - 1u; // m <= 16
            uint32_t kept = mask;
            for (int k = 0; k < m_old; k++) {
                float lb, ub;
                bounds(cxlo, cxhi, cylo, cyhi, S_CX(k), S_CY(k), lb, ub);
                if (!(lb <= U)) kept &= ~(1u << k);
            }
            if (m > 1) {
                const float ixlo = nextafterf(cxlo, INFINITY), ixhi = nextafterf(cxhi, -INFINITY), iylo = nextafterf(cylo, INFINITY),
                            iyhi = nextafterf(cyhi, -INFINITY);
                for (int ka = 0; ka < m; ka++) {
                    float a[4];
                    corner4(S_CX(ka), S_CY(ka), ixlo, ixhi, iylo, iyhi, a);
                    for (uint32_t rc = mask & ~(1u << ka); rc; rc &= rc - 1u) {
                        const int kc = __ffs(rc) - 1;
                        float c[4];
                        corner4(S_CX(kc), S_CY(kc), ixlo, ixhi, iylo, iyhi, c);
                        if (c[0] < a[0] * PF_CORNER_F && c[1] < a[1] * PF_CORNER_F && c[2] < a[2] * PF_CORNER_F && c[3] < a[3] * PF_CORNER_F) {
                            kept &= ~(1u << ka);
                            break;
                        }
                    }
                }
            }
            if (kept == 0u) kept = 1u; // (cannot happen: the node that set U passes both tests against everything else; belt and braces)
            if (kept != mask) { // close the gaps, path order kept; the re-descent entries name their owner by position
                unsigned long long newpos = 0ull;
                int w = 0;
                for (int k = 0; k < m; k++)
                    if ((kept >> k) & 1u) {
                        newpos |= (unsigned long long)w << (4 * k);
                        S_IDX(w) = S_IDX(k);
                        S_CX(w) = S_CX(k);
                        S_CY(w) = S_CY(k);
                        S_PI(w) = S_PI(k);
                        if (k < m_old) { // a recorded candidate: its link, and the parent plane the round of reads has just set
                            S_CT(w) = S_CT(k);
                            S_PP(w) = S_PP(k);
                            S_PC(w) = S_PC(k);
                        }
                        w++;
                    }
                int v = 0;
                for (int k = 0; k < nr; k++) {
                    const int e = S_R(k), ow = (e >> 27) & 15;
                    if ((kept >> ow) & 1u) {
                        S_R(v) = (e & 0x7ffffff) | ((int)((newpos >> (4 * ow)) & 15ull) << 27);
                        S_RX(v) = S_RX(k);
                        S_RY(v) = S_RY(k);
                        v++;
                    }
                }
                nr = v;
                m_old = __popc(kept & ((1u << m_old) - 1u));
                m = w;
            }
        }
        // the new candidates' parents (those that are left), and with them where each one's re-descent walk starts: from candidate k the
        // traversal looks at the parent's hyperplane and, if it is nearer than the best distance, walks the side of the parent the
        // query is NOT on (kernel.cu:1261-1274).  S_CT(k) <= -2: the walk starts at node -S_CT(k) - 2 (the very form the look at the
        // links leaves for a recorded candidate whose terminal link has gained a child); otherwise: the link to watch, no walk.
        for (int k0 = m_old; k0 < m; k0 += 4) {
            uint4 pn[4];
            float zl[4];
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (k0 + q < m) {
                    const int pi = max(S_PI(k0 + q), 0);
                    pn[q] = tree.hot[pi];
                    zl[q] = tree.z[pi]; // true left child of a planar z-level node, as int bits (the query is on its right)
                }
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (k0 + q < m) {
                    const int k = k0 + q, pi = S_PI(k);
                    parent_plane(k, pn[q]);
                    int start = -1, link = -1;
                    if (pi >= 0) {
                        const uint32_t paxis = pn[q].z >> 30;
                        if (paxis == 2) start = __float_as_int(zl[q]); // that link never gains a node (0 < 0 is false): not watched
                        else {
                            const bool plt = (paxis == 0 ? cxlo : cylo) < S_PC(k);
                            link = pi * 2 + (plt ? 1 : 0); // the side the query is NOT on
                            start = plt ? (int)pn[q].w : pf::hot_left(pn[q].z);
                        }
                        if (start >= bound) start = -1; // (bounded walk: that child did not exist yet -- the link is watched instead)
                    }
                    S_CT(k) = start >= 0 ? -start - 2 : link;
                }
        }
        PF_STAMP(3); // pruning + new parents
        // The walks, all of a lane's one after the other and every lane at its own pace: a trip of this loop is ONE hop of every
        // lane that still has one to make (with a loop over the candidates around a loop over the walk, a wave paid the longest walk
        // of its 64 lanes once per candidate position).  A node on a walk can only replace the best one if it is nearer than the
        // best distance <= sqrt(U).
        bool r_over = (rflags & PF_RF_ROVER) != 0;
#ifdef PF_CELLS_PROFILE
        const int nr_before_walks_ = nr;
#endif
        {
            int k = -1, h2 = -1, link = -1;
            uint4 nd = make_uint4(0u, 0u, 0u, 0u);
            for (;;) {
                if (h2 < 0 && k < m) { // this lane's next walk
                    if (k >= 0) S_CT(k) = link; // (of the walk just finished; k only ever stops on a candidate that had one)
                    for (k++; k < m && !r_over; k++) {
                        const int c = S_CT(k);
                        if (c <= -2) {
                            h2 = -c - 2;
                            break;
                        }
                    }
                    if (r_over) k = m;
                    if (k < m) nd = tree.hot[h2];
                }
                if (__builtin_amdgcn_ballot_w64(k < m) == 0ull) break;
                if (k < m) { // one hop
                    int cl = pf::hot_left(nd.z), cr = (int)nd.w;
                    if (cl >= bound) cl = -1;
                    if (cr >= bound) cr = -1;
                    uint4 ndl = nd, ndr = nd; // as in the first descent
                    if (cl >= 0) ndl = tree.hot[cl];
                    if (cr >= 0) ndr = tree.hot[cr];
                    const float nx = __uint_as_float(nd.x), ny = __uint_as_float(nd.y);
                    const uint32_t axis = nd.z >> 30;
                    float lb, ub;
                    bounds(cxlo, cxhi, cylo, cyhi, nx, ny, lb, ub);
                    if (lb <= U || !(fabsf(nx) < 1e6f && fabsf(ny) < 1e6f)) { // (a non-finite node: to the lanes, which know what to do with it)
                        if (nr == PF_CELL_MAXRU) r_over = true; // the rows send such queries down the generic tail: no list, no link to watch
                        else {
                            S_R(nr) = h2 | (k << 27);
                            S_RX(nr) = nx;
                            S_RY(nr) = ny;
                            nr++;
                        }
                    }
                    const bool lt = axis == 0 ? cxlo < nx : (axis == 1 ? cylo < ny : false);
                    link = h2 * 2 + (lt ? 0 : 1);
                    h2 = lt ? cl : cr;
                    nd = lt ? ndl : ndr;
                    if (r_over) { h2 = -1; k = m; }
                }
            }
        }
        PF_STAMP(4); // re-descent walks
#ifdef PF_CELLS_PROFILE /* cs[60]: extensions (no recut pass, not fresh)  cs[61]: ... that added neither a candidate nor a re-descent candidate */
        if (PUBLISH && active && !scratch && !(rflags & PF_RF_FRESH) && !recut) {
            atomicAdd(&cs[60], 1);
            if (m == m_old && nr == nr_before_walks_) atomicAdd(&cs[61], 1);
        }
#endif
        // the record
        if (active) {
            const int fl = (dead ? PF_RF_DEAD : 0) | (r_over ? PF_RF_ROVER : 0) | (PUBLISH ? 0 : PF_RF_FRESH);
            *(int4 *)rec = make_int4(__float_as_int(U), term0, m | (nr << 8) | (fl << 16), gen);
            for (int k = 0; k < m; k++) {
                rec[PF_REC_CAND + k] = S_IDX(k);
                rec[PF_REC_TERM + k] = r_over ? -1 : S_CT(k);
                rec[PF_REC_PAR + k] = S_PI(k);
            }
            for (int k = 0; k < nr; k++) rec[PF_REC_RC + k] = S_R(k);
            if (!PUBLISH) rec[PF_REC_POOL] = rec[PF_REC_POOL + 1] = 0; // no rows yet (a record of an older generation may have left its own here)
        }
        PF_STAMP(5); // record written
        if (!PUBLISH) continue;
        // the four sub-cells: their own bound U_b, their candidates (lb_b <= U_b, path order) and re-descent candidates.
        // A candidate a is also dropped when ONE other candidate c is nearer for every query of the sub-cell (the corner test, see
        // PF_CORNER_F above).  2.14 -> 1.26 candidates per query on the aged bench map (CPU prototype): three queries in four are
        // left with ONE candidate.
        // (candidate in the outer loop, the four sub-cells inside: every LDS entry is read once per pass, not four times -- this
        // arithmetic was 6 of the kernel's ~25 us per wave)
        float Ub[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
        uint32_t keep[4] = {0u, 0u, 0u, 0u};
        int mb[4], rb[4] = {0, 0, 0, 0}, total = 0;
        const float bxlo[4] = {cxlo, xmid, cxlo, xmid}, bxhi[4] = {xmid, cxhi, xmid, cxhi}, bylo[4] = {cylo, cylo, ymid, ymid}, byhi[4] = {ymid, ymid, cyhi, cyhi};
        for (int k = 0; k < m; k++) {
            const float px = S_CX(k), py = S_CY(k);
#pragma unroll
            for (int b4 = 0; b4 < 4; b4++) {
                float lb, ub;
                bounds(bxlo[b4], bxhi[b4], bylo[b4], byhi[b4], px, py, lb, ub);
                Ub[b4] = fminf(Ub[b4], ub);
            }
        }
        for (int k = 0; k < m; k++) {
            const float px = S_CX(k), py = S_CY(k);
#pragma unroll
            for (int b4 = 0; b4 < 4; b4++) {
                float lb, ub;
                bounds(bxlo[b4], bxhi[b4], bylo[b4], byhi[b4], px, py, lb, ub);
                if (lb <= Ub[b4]) keep[b4] |= 1u << k;
            }
        }
#pragma unroll
        for (int b4 = 0; b4 < 4; b4++) {
            const uint32_t mask = keep[b4];
            uint32_t kept = mask;
            if (mask & (mask - 1u)) { // two or more: squared distances to the sub-cell's four corners, once per candidate
                const float ixlo = nextafterf(bxlo[b4], INFINITY), ixhi = nextafterf(bxhi[b4], -INFINITY), iylo = nextafterf(bylo[b4], INFINITY),
                            iyhi = nextafterf(byhi[b4], -INFINITY);
                for (uint32_t ra = mask; ra; ra &= ra - 1u) {
                    const int ka = __ffs(ra) - 1;
                    float a[4];
                    corner4(S_CX(ka), S_CY(ka), ixlo, ixhi, iylo, iyhi, a);
                    for (uint32_t rc = mask & ~(1u << ka); rc; rc &= rc - 1u) {
                        const int kc = __ffs(rc) - 1;
                        float c[4];
                        corner4(S_CX(kc), S_CY(kc), ixlo, ixhi, iylo, iyhi, c);
                        if (c[0] < a[0] * PF_CORNER_F && c[1] < a[1] * PF_CORNER_F && c[2] < a[2] * PF_CORNER_F && c[3] < a[3] * PF_CORNER_F) {
                            kept &= ~(1u << ka);
                            break;
                        }
                    }
                }
            }
            keep[b4] = kept;
        }
        for (int k = 0; k < nr; k++) {
            const float rx = S_RX(k), ry = S_RY(k);
            const int ow = (S_R(k) >> 27) & 15;
#pragma unroll
            for (int b4 = 0; b4 < 4; b4++) {
                float lb, ub;
                bounds(bxlo[b4], bxhi[b4], bylo[b4], byhi[b4], rx, ry, lb, ub);
                rb[b4] += (lb <= Ub[b4] || !(lb == lb)) && ((keep[b4] >> ow) & 1u); // its owner is a candidate of this sub-cell too
            }
        }
#pragma unroll
        for (int b4 = 0; b4 < 4; b4++) {
            int mm = __popc(keep[b4]);
            if (r_over || rb[b4] > PF_CELL_MAXR) rb[b4] = 15; // lists did not fit: generic tail
            if (mm > PF_CELL_MAXC) mm = 0;                    // too many candidates: this sub-cell gets no row
            mb[b4] = mm;
            total += mm ? mm + (rb[b4] == 15 ? 0 : rb[b4]) : 0;
        }
        PF_STAMP(6); // rows cut (arithmetic)
        // Slots: an extended cell's rows go where they were while they fit (a few spare slots are allocated with the first cut) -- with
        // every re-cut at the end of the pool, 25 frames spread 144 k live slots over 610 k, and the scan-match kernel, whose waves
        // gather the slots of neighbouring cells, lost 5 % to that (0.388 vs 0.369 ms against the round-3 build on one box).
        const bool in_place = active && total <= old_len;
        const int alloc = (!active || in_place || total == 0) ? 0 : total + PF_ROW_HEADROOM;
        int incl = alloc; // wave prefix sum: one atomic on the pool counter per wave
        for (int off = 1; off < 64; off <<= 1) {
            const int u = __shfl_up(incl, off, 64);
            if (lane >= off) incl += u;
        }
        const int wave_total = __shfl(incl, 63, 64);
        int wave_base = 0;
        if (lane == 0 && wave_total > 0) wave_base = atomicAdd(&cs[PF_CS_POOL], wave_total);
        wave_base = __shfl(wave_base, 0, 64);
        int off = in_place ? old_off : wave_base + incl - alloc;
        PF_STAMP(7); // pool allocation
        if (!active) continue;
        const bool pool_full = !in_place && off + alloc > cs[PF_CS_POOL_CAP];
        if (pool_full && total > 0) atomicOr(&cs[PF_CS_FLAGS], PF_CF_POOL_FULL);
        rec[PF_REC_POOL] = pool_full ? 0 : off;
        rec[PF_REC_POOL + 1] = pool_full ? 0 : (in_place ? old_len : alloc);
        unsigned word[4]; // the four table words: the slots first, then the four exchanges in flight together
#pragma unroll
        for (int b4 = 0; b4 < 4; b4++) {
            if (mb[b4] == 0 || pool_full) {
                word[b4] = PF_CELL_FALLBACK;
                st_none++;
                continue;
            }
            const float xlo = bxlo[b4], xhi = bxhi[b4], ylo = bylo[b4], yhi = byhi[b4];
            const float u = Ub[b4];
            const uint32_t kept = keep[b4];
            int w = off;
            for (int k = 0; k < m; k++)
                if ((kept >> k) & 1u)
                    pool[w++] = make_uint4(__float_as_uint(S_CX(k)), __float_as_uint(S_CY(k)), (uint32_t)S_IDX(k) | S_PP(k),
                                           __float_as_uint(S_PC(k)));
            if (rb[b4] != 15)
                for (int k = 0; k < nr; k++) {
                    float lb, ub;
                    const int e = S_R(k), ow = (e >> 27) & 15;
                    bounds(xlo, xhi, ylo, yhi, S_RX(k), S_RY(k), lb, ub);
                    if ((lb <= u || !(lb == lb)) && ((kept >> ow) & 1u))
                        pool[w++] = make_uint4(__float_as_uint(S_RX(k)), __float_as_uint(S_RY(k)), (uint32_t)(e & 0x7ffffff),
                                               (uint32_t)S_IDX(ow)); // w: the owner's node
                }
            word[b4] = ((uint32_t)off << 8) | ((uint32_t)rb[b4] << 4) | (uint32_t)mb[b4];
            off = w;
            st_rows++;
            st_n1 += mb[b4];
            st_n2 += rb[b4] == 15 ? 0 : rb[b4];
        }
        // What the four words replace: nothing that counts at a record's first publication (the claim word is PENDING, the others zero: only
        // this record's publications ever write a claimed cell's words), afterwards what the record itself published last -- kept in the
        // record, so the table words are plain stores and the wave does not wait for four exchanges to come back.
        const int4 last_words = HOIST ? pre_last : *(const int4 *)(rec + PF_REC_LAST);
        *(int4 *)(rec + PF_REC_LAST) = make_int4((int)word[0], (int)word[1], (int)word[2], (int)word[3]);
        if (!(scratch || (rflags & PF_RF_FRESH))) {
            const int4 last = last_words;
            unbook((unsigned)last.x); unbook((unsigned)last.y); unbook((unsigned)last.z); unbook((unsigned)last.w);
        }
#pragma unroll
        for (int b4 = 0; b4 < 4; b4++) __hip_atomic_store(&tab[cell + (b4 & 1) + ((b4 & 2) ? PF_CELL_WIN : 0)], word[b4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        PF_STAMP(8); // slots + table words
    }
#ifdef PF_CELLS_PROFILE
    if (PUBLISH && lane == 0) { // whole-wave time of this pass (slot = pass & 15): max, and how many waves took more than 20 / 40 us
        const int dt = (int)((long long)wall_clock64() - t_start_);
        atomicMax(&cs[96 + (pass & 15)], dt);
        if (dt > 2000) atomicAdd(&cs[112 + (pass & 15)], 1);
    }
#endif
    for (int off = 32; off >= 1; off >>= 1) {
        st_rows += __shfl_xor(st_rows, off, 64); st_n1 += __shfl_xor(st_n1, off, 64);
        st_n2 += __shfl_xor(st_n2, off, 64); st_none += __shfl_xor(st_none, off, 64);
        st_fresh += __shfl_xor(st_fresh, off, 64); st_ext += __shfl_xor(st_ext, off, 64); st_reused += __shfl_xor(st_reused, off, 64);
    }
    if (PUBLISH && probe && lane == 0) atomicMax(probe + (PB_UPDATE_END - PB_UPDATE), (unsigned long long)wall_clock64()); // (frame probe: when the last wave ended)
    if (lane == 0) {
        if (st_rows) atomicAdd(&cs[PF_CS_ROWS], st_rows);
        if (st_n1) atomicAdd(&cs[PF_CS_N1], st_n1);
        if (st_n2) atomicAdd(&cs[PF_CS_N2], st_n2);
        if (st_none) atomicAdd(&cs[PF_CS_NONE], st_none);
        if (st_fresh) atomicAdd(&cs[PF_CS_CUR_FRESH], st_fresh);
        if (st_ext) atomicAdd(&cs[PF_CS_CUR_EXT], st_ext);
        if (st_reused) atomicAdd(&cs[PF_CS_CUR_REUSED], st_reused);
    }
}

#undef S_IDX
#undef S_LB
#undef S_CX
#undef S_CY
#undef S_PP
#undef S_PC
#undef S_CT
#undef S_PI
#undef S_R
#undef S_RX
#undef S_RY
// one visit of a row candidate: the arithmetic of kd_resume's visit (packed sub / mul, guard band)
__device__ __forceinline__ float cell_dist2(const uint4 cd, float wx, float wy)
{
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 nxy = {__uint_as_float(cd.x), __uint_as_float(cd.y)};
    const f32x2 pxy = {wx, wy};
    const f32x2 d = nxy - pxy;
    const f32x2 dd = d * d;
    return dd.x + dd.y;
}
__device__ __forceinline__ bool cell_visit(const uint4 cd, float wx, float wy, float &sBest)
{
    const float s = cell_dist2(cd, wx, wy);
    const float sGuard = sBest * PF_GUARD_K;
    bool take = s < sGuard;
    const bool inBand = (s < sBest) != take;
    if (__builtin_amdgcn_ballot_w64(inBand) != 0ull) {
        float sb = sBest;
        asm volatile("" : "+v"(sb));
        take = take | (inBand && pf::fsqrt(s) < pf::fsqrt(sb));
    }
    sBest = take ? s : sBest;
    return take;
}

// CENSUS counters of this kernel: trips = wave-level 16-byte gathers (row slots + node records of the generic tail), lanes = active
// lanes in them, tests / test_lanes = parent-hyperplane tests of the generic tail (one 4-byte + one 16-byte wave gather each),
// uniform = wave-level 4-byte gathers of the cell table, prefix = lanes that found a row, redesc = lanes that ran the generic
// traversal (no row: whole traversal; re-descent winner: tail), redesc_noop = generic re-descents that changed nothing + lanes
// whose cell had no row
//
// The kernel is bound by VALU issue (PMC: 4 cycles x VALU wave-instructions / SIMDs = the kernel's cycles), and a wave's beam
// is a chain of dependent trips to memory, so the loop is organised by hand:
//   * software pipeline: the end point and the table word of beam j + 1 are requested before beam j's row is worked on, a row's
//     slots are requested four at a time (immediate offsets off one address; slots behind the row's end are read and ignored),
//     a node's weight is added one iteration after it was requested;
//   * the beam's angle and its cos / sin come from a per-beam table (wave-uniform scalars), the heading's cos / sin are computed once
//     per lane: an end point is 14 double operations (sincos_sum_spec) instead of an argument reduction and two polynomials;
//   * the parent-hyperplane test needs no square root: hd < sqrt_rn(s) is decided on hd^2 against s with a 2^-21 guard band
//     (sqrt_rn is within 2^-24 of the root and halves relative gaps), the exact comparison runs only inside the band;
//   * a row without re-descent candidates ends the query at once (no test at all: no re-descent could change the best node).
// (Parking the ~9 % of queries that do look at re-descent candidates in their lane and resolving them a few beams later, many
// lanes at once, was measured: same kernel time -- the generic tail runs in 15 % of the (wave, beam) rows, not in most.)
#define PF_ROW_SLACK 4 /* pool slots behind the last row that a four-slot request may touch */
template <bool CENSUS = false, int GUARD = 1, bool ENDS = false>
__global__ __launch_bounds__(64) void k_score_kd_cells(const float *__restrict__ px, const float *__restrict__ py,
                                                       const float *__restrict__ pth, int n, const float *__restrict__ scan,
                                                       const pf::BeamParts *__restrict__ beams, int nb, int beams_per_chunk, pf::KdView tree,
                                                       CellGeom geo, const unsigned *__restrict__ tab, const uint4 *__restrict__ pool,
                                                       const int *__restrict__ cs, const int *__restrict__ order, int direct,
                                                       float *__restrict__ out, int out_mode, pf::KdCensus *__restrict__ census = nullptr,
                                                       unsigned long long *__restrict__ probe = nullptr, const double2 *__restrict__ tparts = nullptr,
                                                       const int *__restrict__ starts = nullptr, unsigned long long *__restrict__ probe_ends = nullptr)
{
    pf_stamp(probe);
    // (frame probe: when the last-indexed wave starts -- with groups fastest and the shortest chunks last, the launch's tail begins here)
    if (probe && blockIdx.x == gridDim.x - 1 && blockIdx.y == gridDim.y - 1 && threadIdx.x == 0) probe[PB_SCORE_LAST - PB_SCORE] = wall_clock64();
    const int g = blockIdx.x, slot = g * 64 + threadIdx.x;
    // this wave's beams: chunk blockIdx.y of the plan (score_plan.h: the round-5 frame's chunks are not all of one size; wave-uniform,
    // two scalar loads), or of the uniform cut
    const int j0 = starts ? starts[blockIdx.y] : blockIdx.y * beams_per_chunk;
    const int j1 = starts ? starts[blockIdx.y + 1] : min(nb, j0 + beams_per_chunk);
    // every lane of the last wave stays in the loop (clamped to the last particle, its result dropped): the wave-level decisions
    // below (ballots) then always see 64 lanes
    const bool real = slot < n;
    const int i = order ? order[min(slot, n - 1)] : min(slot, n - 1);
    const float x = px[i], y = py[i], th = pth[i];
    // the heading's part of every end point of this lane: cos / sin of the heading as doubles.  The frame loop's dispersion kernel leaves
    // them per particle (tparts: the same function of the same float), so that a particle's 42 beam-chunk workgroups do not each run the
    // argument reduction and the two degree-6 polynomials again
    pf::AngleParts T;
    if (tparts) {
        const double2 tp = tparts[i];
        T.c = tp.x;
        T.s = tp.y;
        T.a = (double)th;
    } else T = pf::angle_parts(th);
    const int ox = cs[PF_CS_OX], oy = cs[PF_CS_OY];
    const float inv2x = 2.0f * geo.invx, inv2y = 2.0f * geo.invy;
    const pf::kd_rsrc_t tab_rsrc = pf::kd_rsrc(tab), pool_rsrc = pf::kd_rsrc(pool);
    float acc = 0.0f, wpend = 0.0f; // wpend: the weight requested in the previous iteration (added in beam order, one step late)
    pf::KdCensusLocal cl = {0, 0, 0, 0, 0, 0, 0, 0};
    // stage A of beam j: end point and the table word of its cell.  false: the beam does not score for this lane.
    auto stage_a = [&](int j, float &wx, float &wy, unsigned &e) -> bool {
        const float r = scan[j]; // wave-uniform: scalar loads
        // a beam of 28.4 m or more fails the +-20 m test below for every heading (20 * sqrt(2) = 28.28) -- and so does a NaN range
        if (!(fabsf(r) < PF_RANGE_NEVER)) return false;
        beam_end_point<GUARD>(beams, j, r, th, T, wx, wy);
        if (!(fabsf(wx) < PF_LIDAR_RANGE && fabsf(wy) < PF_LIDAR_RANGE)) return false;
        wx += x;
        wy += y;
        e = 0u;
        float gx, gy;
        int cx = sub_index_fast(wx, inv2x, gx), cy = sub_index_fast(wy, inv2y, gy);
        const float g = fminf(gx, gy);
        bool ok = g > 0.0f; // both axes clear of the sub-cell edges (implies finite)
        if (__builtin_amdgcn_fcmpf(g, 0.0f, 2 /* ordered > */) != __builtin_amdgcn_ballot_w64(true)) { // some lane is not
            if (!ok && fabsf(wx) < 1e6f && fabsf(wy) < 1e6f) { // (a NaN pose fails both: no row, the generic traversal)
                cx = sub_index(wx, geo.resx, geo.invx);
                cy = sub_index(wy, geo.resy, geo.invy);
                float lox, loy, hi, cell_lo;
                sub_edges(cx, geo.resx, lox, hi, cell_lo);
                sub_edges(cy, geo.resy, loy, hi, cell_lo);
                ok = wx != lox && wy != loy; // exactly on a low edge: the rows are not built for that (corner test, PF_CORNER_F)
            }
        }
        cx -= ox;
        cy -= oy;
        if (ok && (unsigned)cx < (unsigned)PF_CELL_WIN && (unsigned)cy < (unsigned)PF_CELL_WIN) {
            if (CENSUS) { unsigned dummy = 0; pf::census_add(cl.uniform, dummy); }
            int off; // byte offset of the cell's word: 24-bit multiply-add (cy < 5120)
            asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(off) : "v"(cy), "s"(PF_CELL_WIN * 4), "v"(cx << 2));
            e = (unsigned)pf::kd_load_i32_bytes(tab_rsrc, off);
        }
        return true;
    };
    // the re-descent of a query whose winner's parent hyperplane is nearer than the best distance: only the nodes the row lists
    // for that winner can matter; if one of them wins (or the lists did not fit), the traversal goes on from the new best node,
    // generically -- kd_resume starts with the parent-hyperplane test of the CURRENT best node, the reference's next step
    auto resolve = [&](float wx, float wy, float sBest, int b, int roff, int n2) -> int {
        bool changed = n2 == 15; // lists did not fit: let the generic tail redo the test and walk
        if (n2 != 15) {
            const uint32_t owner = (uint32_t)b;
            for (int k0 = 0; k0 < n2; k0 += 2) {
                uint4 cd[2];
                const int base = (roff + k0) << 4;
#pragma unroll
                for (int q = 0; q < 2; q++) cd[q] = pf::kd_load_hot_at(pool_rsrc, base, q * 16);
                if (CENSUS) for (int q = 0; q < 2; q++) pf::census_add(cl.trips, cl.lanes);
#pragma unroll
                for (int q = 0; q < 2; q++)
                    if (k0 + q < n2 && cd[q].w == owner && cell_visit(cd[q], wx, wy, sBest)) {
                        b = (int)cd[q].z;
                        changed = true;
                    }
            }
        }
        if (changed) {
            if (CENSUS) cl.redesc++;
            b = pf::kd_resume<true, CENSUS>(tree, wx, wy, 0.0f, sBest, b, -1, &cl);
        }
        return b;
    };
    float cwx = 0.0f, cwy = 0.0f;
    unsigned ce = 0u;
    bool cok = j0 < j1 && stage_a(j0, cwx, cwy, ce);
    for (int j = j0; j < j1; j++) {
        float nwx = 0.0f, nwy = 0.0f;
        unsigned ne = 0u;
        const bool nok = j + 1 < j1 && stage_a(j + 1, nwx, nwy, ne); // in flight while this beam's row is worked on
        if (cok) {
            const float wx = cwx, wy = cwy;
            const unsigned e = ce;
            int b;
            if (e == 0u || e >= 0x40000000u) { // no row for this cell: the whole traversal, per lane
                if (CENSUS) { cl.redesc++; cl.redesc_noop++; }
                b = pf::kd_nearest_ref<true, CENSUS>(tree, wx, wy, 0.0f, &cl);
            } else {
                const int n1 = (int)(e & 15u), n2 = (int)((e >> 4) & 15u), off = (int)(e >> 8);
                if (CENSUS) cl.prefix++;
                // four slots per trip.  A slot no lane of the wave needs is not requested (the texture addresser is as busy as the
                // VALUs here); it then stays undefined -- and unread: the visits are predicated the same way.  Slot 0 always exists,
                // and the first node a search visits becomes its best node whatever the distance (bestDist starts at infinity).
                uint4 cd[4];
                const int base = off << 4;
                cd[0] = pf::kd_load_hot_at(pool_rsrc, base, 0);
                if (CENSUS) pf::census_add(cl.trips, cl.lanes);
#pragma unroll
                for (int q = 1; q < 4; q++)
                    if (__builtin_amdgcn_ballot_w64(q < n1) != 0ull) {
                        cd[q] = pf::kd_load_hot_at(pool_rsrc, base, q * 16);
                        if (CENSUS) pf::census_add(cl.trips, cl.lanes);
                    }
                float sBest = cell_dist2(cd[0], wx, wy);
                uint32_t pk = cd[0].z; // node | parent axis << 30 of the best candidate
                float pcoord = __uint_as_float(cd[0].w);
#pragma unroll
                for (int q = 1; q < 4; q++)
                    if (q < n1) {
                        const bool take = cell_visit(cd[q], wx, wy, sBest);
                        pk = take ? cd[q].z : pk;
                        pcoord = take ? __uint_as_float(cd[q].w) : pcoord;
                    }
                for (int k0 = 4; k0 < n1; k0 += 4) { // rows of more than four candidates: rare
                    const int basek = (off + k0) << 4;
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (__builtin_amdgcn_ballot_w64(k0 + q < n1) != 0ull) {
                            cd[q] = pf::kd_load_hot_at(pool_rsrc, basek, q * 16);
                            if (CENSUS) pf::census_add(cl.trips, cl.lanes);
                        }
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (k0 + q < n1) {
                            const bool take = cell_visit(cd[q], wx, wy, sBest);
                            pk = take ? cd[q].z : pk;
                            pcoord = take ? __uint_as_float(cd[q].w) : pcoord;
                        }
                }
                b = (int)(pk & 0x3fffffffu);
                // parent axis = pk >> 30 (3: no parent -- H1, the search stops); tested on pk itself
                if (pk < 0xC0000000u && n2 != 0) { // the best node has a parent and the row lists re-descent candidates (none: no
                                                   // re-descent can change the best node -- done)
                    // hd < bestDist = sqrt_rn(sBest), without the root: outside a 2^-21 band around sBest, hd^2 decides.  A z-level
                    // parent has hyperplane distance 0 (0 < sqrt_rn(s) exactly when s > 0).  hd^2 may underflow -- harmless while
                    // sBest is an ordinary number (the comparison still comes out right); a best distance below 1e-15 m goes the
                    // exact way.
                    float hd = (pk < 0x40000000u ? wx : wy) - pcoord;
                    hd = (int)pk < 0 ? 0.0f : hd;
                    const float h2 = hd * hd;
                    bool pass = h2 < sBest * PF_GUARD_K;
                    const bool inBand = (!pass && h2 * PF_GUARD_K <= sBest) || sBest < 1e-30f;
                    if (__builtin_amdgcn_ballot_w64(inBand) != 0ull) { // wave-uniform, almost never taken
                        float sb = sBest;
                        asm volatile("" : "+v"(sb));
                        pass = inBand ? fabsf(hd) < pf::fsqrt(sb) : pass;
                    }
                    if (pass) b = resolve(wx, wy, sBest, b, off + n1, n2); // re-descent of the parent's other side
                }
            }
            acc += wpend;
            wpend = tree.w[b];
        }
        cok = nok; cwx = nwx; cwy = nwy; ce = ne;
    }
    acc += wpend;
    if (CENSUS) pf::census_flush(cl, census);
    // out_mode 0: this chunk's partial sum as a float (reduced by the next kernel); 2: nothing (census replay of a pass)
    if (real && out_mode == 0) out[(size_t)blockIdx.y * n + (direct ? i : slot)] = acc;
    // 3: the partial as a 16-bit integer (integer map weights and beams per chunk x largest |weight| <= 32767: exact) -- half the bytes
    // written here and read back by the reduce kernel (33.6 -> 16.8 MB each way per frame at 100 k particles)
    if (real && out_mode == 3) ((short *)out)[(size_t)blockIdx.y * n + slot] = (short)(int)acc;
    // 4: the same 16-bit partial, GROUP-major -- [group][chunk][lane]: the reduce kernel of the frame loop (k_reduce_groups) then reads a
    // group's chunks as 16-byte pieces of one contiguous run instead of one strided 2-byte load per chunk (a lane beyond n stores 0)
    // (as non-temporal stores: measured neutral, tools/experiments/r05/README.md)
    if (out_mode == 4) ((short *)out)[((size_t)g * gridDim.y + blockIdx.y) * 64 + threadIdx.x] = real ? (short)(int)acc : (short)0;
    // (frame probe: when the last wave ended -- a maximum over the launch's waves, spread over PF_PROBE_ENDS words: see there.  An
    // instantiation of its own, launched only while the probe is on: these two lines behind a null test cost the kernel 20 us of its 398
    // at 100 k particles with the probe OFF -- profiles/chunk_taper_ab.txt, "what the end stamp costs")
    if (ENDS && probe_ends && threadIdx.x == 0) atomicMax(probe_ends + (blockIdx.x & (PF_PROBE_ENDS - 1)) * PF_PROBE_END_STRIDE, (unsigned long long)wall_clock64());
}
