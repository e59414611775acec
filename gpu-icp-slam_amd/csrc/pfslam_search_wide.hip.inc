// pfslam_search_wide.hip.inc -- pfslam_search_wide (pfslam_search's winner over windows of up to 2^31 - 1 candidates, found by branch and
// bound over min-pooled copies of the field); the specification is in include/pfslam.h.  Included by pfslam_hip.hip behind
// pfslam_search.hip.inc (same translation unit): k_search_ends, k_search_field and k_search_result are launched as they are.
// tests/test_search_wide_kernel_text.py cuts the text between the two SEARCH-WIDE-KERNEL-TEXT marks out and runs it on the CPU.

#define PF_WIDE_MAX_CAND 2147483647LL /* candidates of one call: k stays a non-negative int32, the key stays S << 32 | k */
#define PF_WIDE_MAX_ROW (1 << 24)     /* (2 half_x + 1)(2 half_y + 1): the candidates of one heading */
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

extern "C" int pfslam_search_wide(pfslam_handle *h, const float centre[3], const pfslam_search_opts *opts, float pose_out[3], float info[8],
                                  int64_t stats[8])
{
    if (!h || !opts || !pose_out || !info) return fail("pfslam_search_wide: bad argument");
    if (opts->half_x < 0 || opts->half_y < 0 || opts->half_theta < 0) return fail("pfslam_search_wide: half_x, half_y and half_theta must be >= 0");
    if (opts->stride < 1 || opts->stride > 64) return fail("pfslam_search_wide: stride must be 1 .. 64");
    if (!std::isfinite(opts->step_theta) || (opts->half_theta > 0 && !(opts->step_theta > 0.0f)))
        return fail("pfslam_search_wide: step_theta must be finite, and > 0 unless half_theta is 0");
    if (!std::isfinite(opts->max_dist) || !(opts->max_dist > 0.0f)) return fail("pfslam_search_wide: max_dist must be finite and > 0");
    if (opts->reserved_[0] || opts->reserved_[1]) return fail("pfslam_search_wide: reserved_ must be 0");
    if (centre && !(std::isfinite(centre[0]) && std::isfinite(centre[1]) && std::isfinite(centre[2]))) return fail("pfslam_search_wide: the centre must be finite");
    const long long nx = 2LL * opts->half_x + 1, ny = 2LL * opts->half_y + 1, na = 2LL * opts->half_theta + 1;
    if (nx > PF_WIDE_MAX_ROW || ny > PF_WIDE_MAX_ROW || nx * ny > PF_WIDE_MAX_ROW || nx * ny * na > PF_WIDE_MAX_CAND)
        return fail("pfslam_search_wide: more than 2^31 - 1 candidates, or more than 2^24 of one heading ((2 half_x + 1)(2 half_y + 1))");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    if (h->kd_size <= 0) return fail("pfslam_search_wide: no map loaded");
    if (h->nb > PF_SUM_TILE) return fail("pfslam_search_wide: n_beams > 4096 not supported");
    if (h->cfg.map_res_x != h->cfg.map_res_y) return fail("pfslam_search_wide: map_res_x != map_res_y not supported");
    SearchParams p;
    p.res = h->cfg.map_res_x;
    p.u = (p.res * p.res) * 0.0625f;
    const float qf = rintf(pf::fdiv(opts->max_dist * opts->max_dist, p.u));
    if (!(qf >= 1.0f && qf <= 65535.0f)) {
        char msg[200];
        snprintf(msg, sizeof(msg), "pfslam_search_wide: max_dist %g gives qcap %g in units of res^2 / 16; it must be 1 .. 65535", (double)opts->max_dist, (double)qf);
        return fail(msg);
    }
    if (na * h->nb > PF_SEARCH_MAX_ENDS) return fail("pfslam_search_wide: more than 2^24 end points ((2 half_theta + 1) * n_beams)");
    float c3[4] = {0, 0, 0, 0};
    if (centre) {
        memcpy(c3, centre, 12);
    } else { // the handle's pose, as pfslam_get_pose reads it
        HIPCHK(hipMemcpyAsync(c3, h->pose, 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (!(std::isfinite(c3[0]) && std::isfinite(c3[1]) && std::isfinite(c3[2]))) return fail("pfslam_search_wide: the centre (the handle's pose) must be finite");
    }
    p.cx = c3[0]; p.cy = c3[1]; p.ct = c3[2];
    p.step_theta = opts->step_theta;
    p.hx = opts->half_x; p.hy = opts->half_y; p.ht = opts->half_theta;
    p.stride = opts->stride;
    p.qcap = (int)qf;
    p.nb = h->nb;
    auto cell_bound = [&](float c, float d) { // rint((c + d) / res) as k_search_ends computes it, inside +-2^20
        const float f = rintf(pf::fdiv(c + d, p.res));
        return (int)std::min(std::max(f, -(float)PF_SEARCH_CELL_MAX), (float)PF_SEARCH_CELL_MAX);
    };
    p.lox = cell_bound(p.cx, -PF_LIDAR_RANGE); p.hix = cell_bound(p.cx, PF_LIDAR_RANGE);
    p.loy = cell_bound(p.cy, -PF_LIDAR_RANGE); p.hiy = cell_bound(p.cy, PF_LIDAR_RANGE);
    const long long W = (long long)p.hix - p.lox + 1 + 2LL * p.hx * p.stride, H = (long long)p.hiy - p.loy + 1 + 2LL * p.hy * p.stride;
    if (W > PF_SEARCH_MAX_FIELD || H > PF_SEARCH_MAX_FIELD || W * H > PF_SEARCH_MAX_FIELD) {
        char msg[200];
        snprintf(msg, sizeof(msg), "pfslam_search_wide: the field would have %lld x %lld cells (40 m / res + 1 + 2 half stride a side); at most 2^26 cells", W, H);
        return fail(msg);
    }
    p.cap = (int)(W * H);
    // the top level: the smallest whose one block covers a heading's window, at most PF_WIDE_MAX_LEVEL
    int top = 0;
    while (top < PF_WIDE_MAX_LEVEL && (1LL << top) < std::max(nx, ny)) top++;
    const long long n_top = na * (((nx - 1) >> top) + 1) * (((ny - 1) >> top) + 1);
    const int room = h->wide_frontier ? h->wide_frontier : PF_WIDE_FRONTIER; // nodes of one frontier buffer
    const size_t level = (size_t)p.cap + 2;                                  // cells of one level (+ the two spare cells of k_search_field)
    // the feature's own device buffers; they grow when a call needs more
    CHK(search_grow(&h->wide_field, &h->wide_field_cap, level * (size_t)(top + 1)));
    CHK(search_grow(&h->wide_ends, &h->wide_ends_cap, (size_t)na * h->nb));
    CHK(search_grow(&h->wide_nin, &h->wide_nin_cap, (size_t)na));
    CHK(search_grow(&h->wide_nodes, &h->wide_nodes_cap, (size_t)room * (size_t)(top + 1)));
    CHK(search_grow(&h->wide_lb, &h->wide_lb_cap, (size_t)room));
    if (!h->wide_state) CHK(dalloc(&h->wide_state, (size_t)4 + PF_SEARCH_OUT / 2)); // key, the four box words, the child count, the result row
    unsigned long long *key = h->wide_state;
    int *box = (int *)(h->wide_state + 1);
    int *count = (int *)(h->wide_state + 3);
    float *out = (float *)(h->wide_state + 4);
    HIPCHK(hipMemsetAsync(h->wide_state, 0xff, 24, h->stream));
    hipLaunchKernelGGL(k_search_ends, dim3((unsigned)na), dim3(256), 0, h->stream, (const float *)h->scan, p, h->trig, h->wide_ends, h->wide_nin, box);
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
    long long bounded = 0, scored = 0, batches = 0;
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
        batches++;
        (L ? bounded : scored) += n;
        const uint16_t *fL = h->wide_field + level * (size_t)L;
        if (L)
            hipLaunchKernelGGL(k_wide_score<false>, dim3((unsigned)n), dim3(64), 0, h->stream, (const int *)nodes, (const int2 *)h->wide_ends,
                               (const int *)h->wide_nin, (const int *)box, (const uint16_t *)h->wide_field, fL, p, h->wide_lb, key);
        else
            hipLaunchKernelGGL(k_wide_score<true>, dim3((unsigned)n), dim3(64), 0, h->stream, (const int *)nodes, (const int2 *)h->wide_ends,
                               (const int *)h->wide_nin, (const int *)box, (const uint16_t *)h->wide_field, fL, p, h->wide_lb, key);
        HIPCHK(hipGetLastError());
        if (L == 0) continue;
        HIPCHK(hipMemsetAsync(count, 0, 4, h->stream));
        hipLaunchKernelGGL(k_wide_expand, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const int *)nodes, (const int *)h->wide_lb, n, L, p,
                           (const unsigned long long *)key, h->wide_nodes + (size_t)room * (size_t)(L - 1), count);
        HIPCHK(hipGetLastError());
        int kids = 0;
        HIPCHK(hipMemcpyAsync(&kids, count, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (kids < 0 || kids > 4 * n) return fail("pfslam_search_wide: internal: a batch left more children than four a node");
        if (kids) {
            L--;
            have[L] = kids;
            done[L] = 0;
        }
    }
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
        // the box as search_box computes it: empty when no beam of any heading has a cell
        const long long cells = bw[0] < 0 ? 0 : ((long long)bw[1] + bw[0] - 2LL * PF_SEARCH_BIAS + 1 + 2LL * p.hx * p.stride) *
                                                    ((long long)bw[3] + bw[2] - 2LL * PF_SEARCH_BIAS + 1 + 2LL * p.hy * p.stride);
        stats[0] = st[0] == ~0ull ? -1 : (int64_t)(st[0] & 0xffffffffull);
        stats[1] = nx * ny * na;
        stats[2] = bounded;
        stats[3] = scored;
        stats[4] = top;
        stats[5] = batches;
        stats[6] = cells;
        stats[7] = 0;
    }
    return 0;
}
