// pfslam_search_wide.hip.inc -- pfslam_search_wide (pfslam_search's winner over windows of up to 2^31 - 1 candidates, found by branch and
// bound over min-pooled copies of the field); the specification is in include/pfslam.h.  Included by pfslam_hip.hip behind
// pfslam_search.hip.inc (same translation unit): k_search_ends, k_search_field and k_search_result are launched as they are.
// tests/test_search_wide_kernel_text.py cuts the text between the two SEARCH-WIDE-KERNEL-TEXT marks out and runs it on the CPU.
// The refusals are search_plan's (pfslam_search.hip.inc; the candidate limits PF_WIDE_MAX_CAND and PF_WIDE_MAX_ROW stand there too).  The
// descent, wide_descend, is here once for this entry point and for pfslam_search_best, which bring their own scoring and expansion.

#define PF_WIDE_FRONTIER (1 << 22)    /* nodes a frontier buffer holds unless pfslam_debug_search_frontier says otherwise: 16 MB a level */

// SEARCH-WIDE-KERNEL-TEXT-BEGIN
#define PF_WIDE_MAX_LEVEL 7 /* blocks of up to 128 x 128 candidates; a call holds up to 8 fields */

// A node is a block of 2^L x 2^L translations of one heading, named by its origin candidate k0 = (a * ny + J) * nx + I: the lowest k of
// the block and a candidate itself.  The level is the same for every node of a launch.

// Level L of the pyramid from level L - 1, one thread per cell of the box, every level at full resolution:
// M_L[x, y] = min of M_{L-1} at (x, y), (x + shift, y), (x, y + shift), (x + shift, y + shift), shift = 2^(L-1) stride; terms outside the
// box are skipped.  M_L[x, y] is then the smallest q of the 2^L x 2^L lattice block (step `stride`) whose origin is (x, y), cut at the box.
__global__ __launch_bounds__(256) void k_wide_pyramid(const int *__restrict__ box, SearchParams p, int shift, const uint16_t *__restrict__ prev,
                                                      uint16_t *__restrict__ next)
{
    const SearchBox B = search_box(box, p);
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id == 0) { // the two spare cells behind every level, as behind the field (k_search_field)
        next[p.cap] = 0;
        next[p.cap + 1] = (uint16_t)p.qcap;
    }
    if (id >= B.W * B.H || id >= p.cap) return;
    const int x = id % B.W, y = id / B.W;
    const bool right = x + shift < B.W, down = y + shift < B.H; // (shift <= 2^12, W and H <= 2^26: no overflow)
    int m = prev[id];
    if (right) m = min(m, (int)prev[id + shift]);
    if (down) {
        const int below = (y + shift) * B.W + x; // < W * H
        m = min(m, (int)prev[below]);
        if (right) m = min(m, (int)prev[below + shift]);
    }
    next[id] = (uint16_t)m;
}

// The top level's nodes first .. first + n - 1 of the na * by * bx blocks that tile the window, by stands for ceil(ny / 2^L).
__global__ __launch_bounds__(256) void k_wide_top(SearchParams p, int L, long long first, int n, int *__restrict__ nodes)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int nx = 2 * p.hx + 1, ny = 2 * p.hy + 1;
    const int bx = ((nx - 1) >> L) + 1, by = ((ny - 1) >> L) + 1;
    const long long id = first + t;
    const int a = (int)(id / ((long long)bx * by)), r = (int)(id % ((long long)bx * by));
    nodes[t] = (a * ny + ((r / bx) << L)) * nx + ((r % bx) << L); // a candidate: below 2^31
}

// The hot path.  A workgroup is one wave and scores one node, the beams across the lanes: each lane loads the 8-byte end point of its
// beams (coalesced) and gathers two bytes of M_L and two of M_0 at the same index.  LB, the sum over M_L, is <= S of every candidate of
// the block; S, the sum over M_0, is the exact score of the block's origin and goes into the call's key with the 64-bit atomicMin.
// Both are integer sums: exact in any order.  At level 0 (LEAF) the two are one.  As in k_search_score there is no branch in the loop, so
// that the gathers of several beams are in flight at once: a beam that is out of range, or behind the scan's last, reads the spare cell
// `cap` (0), an in-range beam without a cell the spare cell `cap + 1` (qcap).  The frontier needs no order: the nodes of a wave's
// neighbours are 2^L stride cells apart or belong to other headings.
template <bool LEAF>
__global__ __launch_bounds__(64) void k_wide_score(const int *__restrict__ nodes, const int2 *__restrict__ ends, const int *__restrict__ nin,
                                                   const int *__restrict__ box, const uint16_t *__restrict__ f0, const uint16_t *__restrict__ fL,
                                                   SearchParams p, int *__restrict__ lb, unsigned long long *key)
{
    const int w = blockIdx.x; // (the launch has one workgroup per node)
    const int k0 = nodes[w];
    const int nx = 2 * p.hx + 1, row = nx * (2 * p.hy + 1);
    const int a = k0 / row, c = k0 % row;
    if (nin[a] == 0) { // (the whole wave) a heading without an in-range beam takes no part in the pick: the node is dropped
        if (threadIdx.x == 0) lb[w] = -1;
        return;
    }
    const SearchBox B = search_box(box, p);
    // the origin's shift, as in k_search_score: the origin is a candidate of the window, so every index below is inside the box
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
        if (m < *(volatile unsigned long long *)key) atomicMin(key, m); // (the key only falls: a stale read costs an atomic, never a result)
    }
}

// After a level's scoring launch has finished: a node leaves only if (LB << 32 | k0) > the key -- no candidate of its block can then take
// the key, not even by the tie rule, as k0 is the block's lowest k.  Equality of LB alone never drops a node.  A survivor's children are
// the up to four blocks of level L - 1 inside the window; a wave books their places with one atomicAdd.  `out` holds 4 n nodes.
__global__ __launch_bounds__(256) void k_wide_expand(const int *__restrict__ nodes, const int *__restrict__ lb, int n, int L, SearchParams p,
                                                     const unsigned long long *__restrict__ key, int *__restrict__ out, int *count)
{
    const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const int nx = 2 * p.hx + 1, ny = 2 * p.hy + 1, half = 1 << (L - 1);
    int k0 = 0, kids = 0;
    bool right = false, down = false;
    if (t < n) {
        k0 = nodes[t];
        const int v = lb[t];
        if (v >= 0 && (((unsigned long long)(unsigned)v << 32) | (unsigned)k0) <= *key) {
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
    int *__restrict__ q = out + base + before;
    *q++ = k0;
    if (right) *q++ = k0 + half;
    if (down) { // (half * nx is below the candidate count here)
        *q++ = k0 + half * nx;
        if (right) *q++ = k0 + half * nx + half;
    }
}
// SEARCH-WIDE-KERNEL-TEXT-END

extern "C" int pfslam_debug_search_frontier(pfslam_handle *h, int nodes)
{
    if (!h || nodes < 0) return fail("pfslam_debug_search_frontier: bad argument");
    h->wide_frontier = nodes == 0 ? PF_WIDE_FRONTIER : std::max(nodes, 4);
    return 0;
}

static long long search_box_cells(const int bw[4], const SearchParams &p)
{
    return bw[0] < 0 ? 0 : ((long long)bw[1] + bw[0] - 2LL * PF_SEARCH_BIAS + 1 + 2LL * p.hx * p.stride) *
                               ((long long)bw[3] + bw[2] - 2LL * PF_SEARCH_BIAS + 1 + 2LL * p.hy * p.stride);
}

// The branch and bound of pfslam_search_wide and pfslam_search_best: end points, the field and its pyramid into the wide_* buffers, then
// the descent.  `box` and `count` are words of the caller's state row, which it has memset; the caller brings its launches (checked here):
//   score(leaf, n, nodes, fL) scores the batch's n nodes (fL: their level of the pyramid; leaf: std::true_type at level 0, the scoring
//                             kernels' template argument) into wide_lb and into its own keys;
//   expand(L, n, nodes, next) books the survivors' children in `next`, the buffer of level L - 1, and their number in *count.
struct WideDescent { int top; long long bounded, scored, batches; }; // the top level; nodes scored above and at level 0; launches of `score`

// stats[1 .. 6] of either entry point; stats[6]: the cells of the box as search_box computes it, none when no beam of any heading has a cell
static void wide_stats(const SearchPlan &s, const WideDescent &d, const int bw[4], int64_t stats[8])
{
    stats[1] = (int64_t)s.cand;
    stats[2] = d.bounded;
    stats[3] = d.scored;
    stats[4] = d.top;
    stats[5] = d.batches;
    stats[6] = search_box_cells(bw, s.p);
}
template <typename Score, typename Expand>
static int wide_descend(pfslam_handle *h, const char *fn, const SearchPlan &s, int *box, int *count, Score score, Expand expand, WideDescent *d)
{
    const SearchParams &p = s.p;
    int top = 0;
    while (top < PF_WIDE_MAX_LEVEL && (1LL << top) < std::max(s.nx, s.ny)) top++;
    const long long n_top = s.na * (((s.nx - 1) >> top) + 1) * (((s.ny - 1) >> top) + 1);
    const int room = h->wide_frontier ? h->wide_frontier : PF_WIDE_FRONTIER; // nodes of one frontier buffer
    const size_t level = (size_t)p.cap + 2;                                  // cells of one level (+ the two spare cells of k_search_field)
    // scratch that either caller rewrites from the start of every call; it grows when a call needs more
    CHK(search_grow(&h->wide_field, &h->wide_field_cap, level * (size_t)(top + 1)));
    CHK(search_grow(&h->wide_ends, &h->wide_ends_cap, (size_t)s.na * h->nb));
    CHK(search_grow(&h->wide_nin, &h->wide_nin_cap, (size_t)s.na));
    CHK(search_grow(&h->wide_nodes, &h->wide_nodes_cap, (size_t)room * (size_t)(top + 1)));
    CHK(search_grow(&h->wide_lb, &h->wide_lb_cap, (size_t)room));
    hipLaunchKernelGGL(k_search_ends, dim3((unsigned)s.na), dim3(256), 0, h->stream, (const float *)h->scan, p, h->trig, h->wide_ends, h->wide_nin, box);
    HIPCHK(hipGetLastError());
    const unsigned cell_blocks = (unsigned)((p.cap + 255) / 256);
    hipLaunchKernelGGL(k_search_field, dim3(cell_blocks), dim3(256), 0, h->stream, kd_view(h), p, (const int *)box, h->wide_field);
    HIPCHK(hipGetLastError());
    for (int L = 1; L <= top; L++) {
        hipLaunchKernelGGL(k_wide_pyramid, dim3(cell_blocks), dim3(256), 0, h->stream, (const int *)box, p, (1 << (L - 1)) * p.stride,
                           (const uint16_t *)(h->wide_field + level * (size_t)(L - 1)), h->wide_field + level * (size_t)L);
        HIPCHK(hipGetLastError());
    }
    // The descent, depth first over batches: a batch is at most room / 4 nodes of one level (room at level 0), so that its children fit
    // the next level's buffer whatever the pruning does.  With room to spare a level is one batch and the descent is level by level.
    // One wait per batch above level 0: the host reads how many children it left.
    long long have[PF_WIDE_MAX_LEVEL + 1] = {0}, done[PF_WIDE_MAX_LEVEL + 1] = {0};
    *d = WideDescent{top, 0, 0, 0};
    have[top] = n_top;
    for (int L = top;;) {
        if (done[L] >= have[L]) {
            if (L == top) break;
            L++;
            continue;
        }
        const int n = (int)std::min<long long>(have[L] - done[L], L ? std::max(room / 4, 1) : room);
        int *nodes = h->wide_nodes + (size_t)room * (size_t)L;
        if (L == top) {
            hipLaunchKernelGGL(k_wide_top, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, p, L, done[L], n, nodes);
            HIPCHK(hipGetLastError());
        } else {
            nodes += done[L];
        }
        done[L] += n;
        d->batches++;
        (L ? d->bounded : d->scored) += n;
        const uint16_t *fL = h->wide_field + level * (size_t)L;
        L ? score(std::false_type{}, n, (const int *)nodes, fL) : score(std::true_type{}, n, (const int *)nodes, fL);
        HIPCHK(hipGetLastError());
        if (L == 0) continue;
        HIPCHK(hipMemsetAsync(count, 0, 4, h->stream));
        expand(L, n, (const int *)nodes, h->wide_nodes + (size_t)room * (size_t)(L - 1));
        HIPCHK(hipGetLastError());
        int kids = 0;
        HIPCHK(hipMemcpyAsync(&kids, count, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (kids < 0 || kids > 4 * n) return fail(std::string(fn) + ": internal: a batch left more children than four a node");
        if (kids) {
            L--;
            have[L] = kids;
            done[L] = 0;
        }
    }
    return 0;
}

extern "C" int pfslam_search_wide(pfslam_handle *h, const float centre[3], const pfslam_search_opts *opts, float pose_out[3], float info[8],
                                  int64_t stats[8])
{
    if (!h || !opts || !pose_out || !info) return fail("pfslam_search_wide: bad argument");
    SearchPlan s;
    CHK(search_plan(h, "pfslam_search_wide", PF_FORM_WIDE, nullptr, centre, opts, &s));
    const SearchParams &p = s.p;
    if (!h->wide_state) CHK(dalloc(&h->wide_state, (size_t)4 + PF_SEARCH_OUT / 2)); // key, the four box words, the child count, the result row
    unsigned long long *key = h->wide_state;
    int *box = (int *)(h->wide_state + 1);
    int *count = (int *)(h->wide_state + 3);
    float *out = (float *)(h->wide_state + 4);
    HIPCHK(hipMemsetAsync(h->wide_state, 0xff, 24, h->stream));
    WideDescent d;
    CHK(wide_descend(
        h, "pfslam_search_wide", s, box, count,
        [&](auto leaf, int n, const int *nodes, const uint16_t *fL) {
            hipLaunchKernelGGL(k_wide_score<decltype(leaf)::value>, dim3((unsigned)n), dim3(64), 0, h->stream, nodes, (const int2 *)h->wide_ends,
                               (const int *)h->wide_nin, (const int *)box, (const uint16_t *)h->wide_field, fL, p, h->wide_lb, key);
        },
        [&](int L, int n, const int *nodes, int *next) {
            hipLaunchKernelGGL(k_wide_expand, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, nodes, (const int *)h->wide_lb, n, L, p,
                               (const unsigned long long *)key, next, count);
        },
        &d));
    hipLaunchKernelGGL(k_search_result, dim3(1), dim3(1), 0, h->stream, (const unsigned long long *)key, (const int *)h->wide_nin, p, out);
    HIPCHK(hipGetLastError());
    unsigned long long st[4 + PF_SEARCH_OUT / 2];
    HIPCHK(hipMemcpyAsync(st, h->wide_state, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(pose_out, st + 4, 12);
    memcpy(info, (const float *)(st + 4) + 4, 32);
    if (stats) {
        int bw[4];
        memcpy(bw, st + 1, 16);
        stats[0] = st[0] == ~0ull ? -1 : (int64_t)(st[0] & 0xffffffffull);
        wide_stats(s, d, bw, stats);
        stats[7] = 0;
    }
    return 0;
}
