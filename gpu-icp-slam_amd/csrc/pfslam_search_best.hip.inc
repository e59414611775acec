// pfslam_search_best.hip.inc -- pfslam_search_best (the best candidate of each of the N best cells of a search window: pfslam_search_wide's
// branch and bound with one key per cell instead of one per call); the specification is in include/pfslam.h.  Included by pfslam_hip.hip
// behind pfslam_search_wide.hip.inc (same translation unit): k_search_ends, k_search_field, k_wide_pyramid and k_wide_top are launched as
// they are, and the field levels, the end points, the in-range counts, the frontier and the lower bounds are pfslam_search_wide's buffers
// (scratch that either function rewrites from the start of every call).  The shared refusals are search_plan's (pfslam_search.hip.inc) and
// the descent is pfslam_search_wide's wide_descend; this file brings its scoring, its threshold and expansion, and the selection behind.
// tests/test_search_best_kernel_text.py cuts the text between the two SEARCH-BEST-KERNEL-TEXT marks out and runs it on the CPU.
//   Measured on one MI355X, 1081 beams (profiles/search_best.txt): the whole map, 1601 x 1601 x 503 candidates in 2 545 263 cells, eight rows:
//   15.2 ms on the 4000-point map and 19.0 ms on the 100 000-point map, 1.16 and 1.31 times pfslam_search_wide; count = 1: 1.01 and 1.02 times.
//   Kernel resources (VGPRs / LDS bytes per workgroup / waves per SIMD): scoring 59 / 0 / 8 (44 at level 0), threshold 26 / 34 944 / 4 (one
//   workgroup a launch), expansion 19 / 0 / 8, compaction 5 / 0 / 8, rows 16 / 0 / 8.

#define PF_BEST_MAX_COUNT 64       /* rows of one call */
#define PF_BEST_MAX_CELLS (1 << 22) /* cells of one call: the table of representatives stays within 32 MB */
#define PF_BEST_STATE (4 + PF_BEST_MAX_COUNT + PF_BEST_MAX_COUNT * PF_SEARCH_OUT / 2) /* threshold, box, child count; the rows' keys; the rows */

// SEARCH-BEST-KERNEL-TEXT-BEGIN
#define PF_BEST_SLICES 4096 /* cell c belongs to slice c mod 4096; the threshold is selected among the slices' minima */

// pfslam_best_opts and what the host derives from them, by value
struct BestParams {
    int ls, g;  // tile_log2, group_theta
    int tx, ty; // tiles of a heading's window in x and y
    int cells;  // tx * ty * ceil(na / g); tab holds `cells` representatives and, behind them, the PF_BEST_SLICES slice minima
};

// The cell of candidate k.
__device__ __forceinline__ int best_cell(int k, const SearchParams &p, const BestParams &q)
{
    const int nx = 2 * p.hx + 1, row = nx * (2 * p.hy + 1);
    const int a = k / row, c = k % row;
    return ((a / q.g) * q.ty + ((c / nx) >> q.ls)) * q.tx + ((c % nx) >> q.ls); // below q.cells <= 2^22
}

// The hot path: k_wide_score's wave per node and its beam loop (coalesced 8-byte end points, two 2-byte gathers per beam at the same index,
// no branch in the loop, integer sums, an xor butterfly).  Instead of the call's one key, lane 0 offers the origin's exact key S << 32 | k0
// to the representative of the origin's cell and to the minimum of that cell's slice, each behind the stale-read guard: both words only
// fall, so a stale read costs an atomic, never a result.
template <bool LEAF>
__global__ __launch_bounds__(64) void k_best_score(const int *__restrict__ nodes, const int2 *__restrict__ ends, const int *__restrict__ nin,
                                                   const int *__restrict__ box, const uint16_t *__restrict__ f0, const uint16_t *__restrict__ fL,
                                                   SearchParams p, BestParams q, int *__restrict__ lb, unsigned long long *tab)
{
    const int w = blockIdx.x; // (the launch has one workgroup per node)
    const int k0 = nodes[w];
    const int nx = 2 * p.hx + 1, row = nx * (2 * p.hy + 1);
    const int a = k0 / row, c = k0 % row;
    if (nin[a] == 0) { // (the whole wave) a heading without an in-range beam takes no part: the node is dropped
        if (threadIdx.x == 0) lb[w] = -1;
        return;
    }
    const SearchBox B = search_box(box, p);
    // the origin's shift, as in k_wide_score: the origin is a candidate of the window, so every index below is inside the box
    const int off = (c / nx - p.hy) * p.stride * B.W + (c % nx - p.hx) * p.stride;
    const int2 *__restrict__ e = ends + (size_t)a * p.nb;
    int lo = 0, S = 0;
#pragma unroll 4
    for (int b0 = 0; b0 < p.nb; b0 += 64) {
        const int b = b0 + (int)threadIdx.x;
        const int2 v = e[min(b, p.nb - 1)];
        const bool mine = b < p.nb, cell = mine && v.x != PF_SEARCH_BAD;
        const int lin = cell ? (v.y - B.y0) * B.W + (v.x - B.x0) + off : (!mine || v.y == PF_SEARCH_SKIP ? p.cap : p.cap + 1);
        S += (int)f0[lin];
        if (!LEAF) lo += (int)fL[lin];
    }
    for (int o = 32; o >= 1; o >>= 1) {
        S += __shfl_xor(S, o, 64);
        if (!LEAF) lo += __shfl_xor(lo, o, 64);
    }
    if (LEAF) lo = S;
    if (threadIdx.x == 0) {
        lb[w] = lo;
        const unsigned long long m = ((unsigned long long)(unsigned)S << 32) | (unsigned)k0;
        const int id = ((a / q.g) * q.ty + ((c / nx) >> q.ls)) * q.tx + ((c % nx) >> q.ls); // best_cell(k0)
        unsigned long long *rep = tab + id, *slice = tab + q.cells + (id & (PF_BEST_SLICES - 1));
        if (m < *(volatile unsigned long long *)rep) atomicMin(rep, m);
        if (m < *(volatile unsigned long long *)slice) atomicMin(slice, m);
    }
}

// After a scoring launch has finished: the threshold, the `count`-th smallest of the slice minima (all ones while fewer than `count`
// slices hold a key).  A slice's minimum is the representative so far of ONE of its cells, the minima of different slices belong to
// different cells, and a representative only falls: `count` cells end at or below the threshold, so the final `count`-th smallest
// representative does.  One workgroup; the 4096 minima are staged in LDS and round r takes the smallest above round r - 1's (the keys of
// different candidates are distinct), reduced through LDS in two steps of 16.
__global__ __launch_bounds__(256) void k_best_thr(const unsigned long long *__restrict__ slices, int count, unsigned long long *__restrict__ thr)
{
    __shared__ unsigned long long s_v[PF_BEST_SLICES], s_p[256], s_q[16];
    const int t = threadIdx.x;
    for (int n = t; n < PF_BEST_SLICES; n += 256) s_v[n] = slices[n];
    __syncthreads();
    unsigned long long prev = 0;
    for (int r = 0; r < count; r++) {
        unsigned long long m = ~0ull;
        for (int n = 0; n < PF_BEST_SLICES / 256; n++) {
            const unsigned long long v = s_v[n * 256 + t];
            if ((r == 0 || v > prev) && v < m) m = v;
        }
        s_p[t] = m;
        __syncthreads();
        if (t < 16) {
            m = s_p[t * 16];
            for (int n = 1; n < 16; n++) m = s_p[t * 16 + n] < m ? s_p[t * 16 + n] : m;
            s_q[t] = m;
        }
        __syncthreads(); // (a thread writes s_p or s_q again only behind a barrier that every reader of this round has reached)
        prev = s_q[0];
        for (int n = 1; n < 16; n++) prev = s_q[n] < prev ? s_q[n] : prev;
        if (prev == ~0ull) break; // (the whole workgroup) fewer than `count` slices hold a key
    }
    if (t == 0) *thr = prev;
}

// After the threshold: a node with key nk = LB << 32 | k0 leaves (1) if nk > the threshold -- no candidate of its block can be the
// representative of one of the `count` best cells -- or (2) if its block lies inside one cell (L <= tile_log2; a block is one heading) and
// nk > that cell's representative, which the block then cannot improve.  Equality never drops a node: k0 is the block's lowest k, and the
// lowest-k tie would be lost.  Children and the wave's one atomicAdd are k_wide_expand's.  `out` holds 4 n nodes.
__global__ __launch_bounds__(256) void k_best_expand(const int *__restrict__ nodes, const int *__restrict__ lb, int n, int L, SearchParams p, BestParams q,
                                                     const unsigned long long *__restrict__ thr, const unsigned long long *__restrict__ tab,
                                                     int *__restrict__ out, int *count)
{
    const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const int nx = 2 * p.hx + 1, ny = 2 * p.hy + 1, half = 1 << (L - 1);
    int k0 = 0, kids = 0;
    bool right = false, down = false;
    if (t < n) {
        k0 = nodes[t];
        const int v = lb[t];
        const unsigned long long nk = ((unsigned long long)(unsigned)v << 32) | (unsigned)k0;
        bool keep = v >= 0 && nk <= *thr;
        if (keep && L <= q.ls) keep = nk <= tab[best_cell(k0, p, q)];
        if (keep) {
            const int c = k0 % (nx * ny);
            right = c % nx + half < nx;
            down = c / nx + half < ny;
            kids = 1 + (right ? 1 : 0) + (down ? 1 : 0) + (right && down ? 1 : 0);
        }
    }
    // the wave's exclusive prefix and total of `kids`, then the base from lane 0's atomicAdd
    int sum = kids, before = 0;
    for (int o = 1; o <= 32; o <<= 1) {
        const int other = __shfl_xor(sum, o, 64);
        if (lane & o) before += other;
        sum += other;
    }
    int base = 0;
    if (lane == 0 && sum) base = atomicAdd(count, sum);
    for (int o = 32; o >= 1; o >>= 1) base += __shfl_xor(base, o, 64);
    if (!kids) return;
    int *__restrict__ w = out + base + before;
    *w++ = k0;
    if (right) *w++ = k0 + half;
    if (down) { // (half * nx is below the candidate count here)
        *w++ = k0 + half * nx;
        if (right) *w++ = k0 + half * nx + half;
    }
}

// After the descent, one thread per cell: the representatives at or below the threshold, in any order, behind their number in the low half
// of list[0].  The list has room for every cell, so a long list costs a long copy, never the result.
__global__ __launch_bounds__(256) void k_best_compact(const unsigned long long *__restrict__ tab, int cells, const unsigned long long *__restrict__ thr,
                                                      unsigned long long *__restrict__ list)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cells) return;
    const unsigned long long v = tab[c];
    if (v == ~0ull || v > *thr) return;
    list[1 + atomicAdd((int *)list, 1)] = v; // (fewer than `cells` hits before this one)
}

// Row r from its key, one thread a row: k_search_result's arithmetic for that candidate.
__global__ __launch_bounds__(64) void k_best_rows(const unsigned long long *__restrict__ keys, int n, const int *__restrict__ nin, SearchParams p,
                                                  float *__restrict__ rows)
{
    const int r = threadIdx.x;
    if (blockIdx.x != 0 || r >= n) return;
    const int nx = 2 * p.hx + 1, ny = 2 * p.hy + 1, row = nx * ny;
    const unsigned long long kk = keys[r];
    const int S = (int)(kk >> 32), k = (int)(kk & 0xffffffffull);
    const int a = k / row, j = (k % row) / nx, i = k % nx;
    float *out = rows + (size_t)r * PF_SEARCH_OUT;
    out[0] = p.cx + (float)((i - p.hx) * p.stride) * p.res;
    out[1] = p.cy + (float)((j - p.hy) * p.stride) * p.res;
    out[2] = p.ct + (float)(a - p.ht) * p.step_theta;
    out[3] = 0.0f;
    out[4] = 0.0f;
    out[5] = (float)k;
    out[6] = (float)nin[a];
    out[7] = pf::fdiv((float)S * p.u, (float)nin[a]);
    out[8] = (float)S;
    out[9] = (float)(row * (2 * p.ht + 1));
    out[10] = (float)p.qcap;
    out[11] = 0.0f;
}
// SEARCH-BEST-KERNEL-TEXT-END

extern "C" void pfslam_search_best_default_opts(pfslam_best_opts *o)
{
    if (!o) return;
    o->count = 8;
    o->tile_log2 = 3;
    o->group_theta = 8;
    o->reserved_ = 0;
}

extern "C" int pfslam_search_best(pfslam_handle *h, const float centre[3], const pfslam_search_opts *opts, const pfslam_best_opts *best,
                                  float *poses_out, float *info, int64_t *index, int *found, int64_t stats[8])
{
    // pfslam_search_wide's refusals, in its order
    if (!h || !opts) return fail("pfslam_search_best: bad argument");
    SearchPlan s;
    CHK(search_plan(h, "pfslam_search_best", PF_FORM_WIDE, nullptr, centre, opts, &s));
    const SearchParams &p = s.p;
    const long long nx = s.nx, ny = s.ny, na = s.na;
    // then this function's own
    if (!best || !poses_out || !info || !index || !found) return fail("pfslam_search_best: bad argument");
    if (best->count < 1 || best->count > PF_BEST_MAX_COUNT) return fail("pfslam_search_best: count must be 1 .. 64");
    if (best->tile_log2 < 0 || best->tile_log2 > PF_WIDE_MAX_LEVEL) return fail("pfslam_search_best: tile_log2 must be 0 .. 7");
    if (best->group_theta < 1) return fail("pfslam_search_best: group_theta must be >= 1");
    if (best->reserved_) return fail("pfslam_search_best: reserved_ must be 0");
    BestParams q;
    q.ls = best->tile_log2;
    q.g = best->group_theta;
    q.tx = (int)(((nx - 1) >> q.ls) + 1);
    q.ty = (int)(((ny - 1) >> q.ls) + 1);
    const long long cells = (long long)q.tx * q.ty * ((na - 1) / q.g + 1);
    if (cells > PF_BEST_MAX_CELLS) {
        char msg[200];
        snprintf(msg, sizeof(msg), "pfslam_search_best: more than 2^22 cells (%d x %d tiles x %lld heading groups)", q.tx, q.ty, (na - 1) / q.g + 1);
        return fail(msg);
    }
    q.cells = (int)cells;
    const int want = best->count;
    // this function's own buffers: the table (representatives, then slice minima), the list (its length, then up to every cell) and
    // threshold + box words + child count + the rows' keys + the rows; they grow when a call needs more
    CHK(search_grow(&h->best_tab, &h->best_tab_cap, (size_t)cells + PF_BEST_SLICES));
    CHK(search_grow(&h->best_list, &h->best_list_cap, (size_t)cells + 1));
    if (!h->best_state) CHK(dalloc(&h->best_state, (size_t)PF_BEST_STATE));
    unsigned long long *thr = h->best_state, *tab = h->best_tab, *keys = h->best_state + 4;
    int *box = (int *)(h->best_state + 1);
    int *count = (int *)(h->best_state + 3);
    float *rows = (float *)(h->best_state + 4 + PF_BEST_MAX_COUNT);
    HIPCHK(hipMemsetAsync(h->best_state, 0xff, 24, h->stream));
    HIPCHK(hipMemsetAsync(tab, 0xff, ((size_t)cells + PF_BEST_SLICES) * 8, h->stream));
    HIPCHK(hipMemsetAsync(h->best_list, 0, 8, h->stream));
    // pfslam_search_wide's descent through its scratch; between a batch's scoring and its expansion the threshold is selected anew
    WideDescent d;
    CHK(wide_descend(
        h, "pfslam_search_best", s, box, count,
        [&](auto leaf, int n, const int *nodes, const uint16_t *fL) {
            hipLaunchKernelGGL(k_best_score<decltype(leaf)::value>, dim3((unsigned)n), dim3(64), 0, h->stream, nodes, (const int2 *)h->wide_ends,
                               (const int *)h->wide_nin, (const int *)box, (const uint16_t *)h->wide_field, fL, p, q, h->wide_lb, tab);
        },
        [&](int L, int n, const int *nodes, int *next) {
            hipLaunchKernelGGL(k_best_thr, dim3(1), dim3(256), 0, h->stream, (const unsigned long long *)(tab + cells), want, thr);
            hipLaunchKernelGGL(k_best_expand, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, nodes, (const int *)h->wide_lb, n, L, p, q,
                               (const unsigned long long *)thr, (const unsigned long long *)tab, next, count);
        },
        &d));
    // The selection: the last threshold, the cells at or below it (at least `count` of them, or every cell that has a representative),
    // their exact order on the host.  The first copy takes the list's head, which is the whole list unless many cells share a slice.
    hipLaunchKernelGGL(k_best_thr, dim3(1), dim3(256), 0, h->stream, (const unsigned long long *)(tab + cells), want, thr);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_best_compact, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, h->stream, (const unsigned long long *)tab, (int)cells,
                       (const unsigned long long *)thr, h->best_list);
    HIPCHK(hipGetLastError());
    const size_t head = (size_t)std::min<long long>(cells, 1023);
    std::vector<unsigned long long> list(1 + head);
    int bw[4];
    HIPCHK(hipMemcpyAsync(list.data(), h->best_list, (1 + head) * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(bw, box, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const long long n_list = (long long)(list[0] & 0xffffffffull);
    if (n_list > cells) return fail("pfslam_search_best: internal: more representatives than cells");
    if ((size_t)n_list > head) {
        list.resize(1 + (size_t)n_list);
        HIPCHK(hipMemcpyAsync(list.data() + 1 + head, h->best_list + 1 + head, ((size_t)n_list - head) * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    const int n_rows = (int)std::min<long long>(n_list, want);
    std::partial_sort(list.begin() + 1, list.begin() + 1 + n_rows, list.begin() + 1 + n_list);
    float r[PF_BEST_MAX_COUNT * PF_SEARCH_OUT];
    if (n_rows) {
        HIPCHK(hipMemcpyAsync(keys, list.data() + 1, (size_t)n_rows * 8, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_best_rows, dim3(1), dim3(64), 0, h->stream, (const unsigned long long *)keys, n_rows, (const int *)h->wide_nin, p, rows);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(r, rows, (size_t)n_rows * PF_SEARCH_OUT * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    for (int n = 0; n < n_rows; n++) {
        memcpy(poses_out + 3 * n, r + PF_SEARCH_OUT * n, 12);
        memcpy(info + 8 * n, r + PF_SEARCH_OUT * n + 4, 32);
        index[n] = (int64_t)(list[1 + n] & 0xffffffffull);
    }
    *found = n_rows;
    if (stats) {
        stats[0] = n_rows ? (int64_t)(list[1] & 0xffffffffull) : -1;
        wide_stats(s, d, bw, stats);
        stats[7] = cells;
    }
    return 0;
}
