// pfslam_search.hip.inc -- pfslam_search (windowed correlative scan-to-map search: every pose of a window scored against a distance field
// of the map); the specification is in include/pfslam.h.  Included by pfslam_hip.hip behind pfslam_register_batch.hip.inc (same
// translation unit): it reuses pf::kd_nearest_exact, pf::clean_lidar_scan and pf::fdiv as they are.
// tests/test_search_kernel_text.py cuts the text between the two SEARCH-KERNEL-TEXT marks out and runs it on the CPU.
// What the search family shares on the host is here: search_derive (SearchParams from a call's arguments; inside the marks, so the CPU
// emulators run it too), search_plan (the common refusals, in their one order, under the caller's name) and search_grow.  The one
// volume runner, search_volume, is declared here and defined in pfslam_search_cov.hip.inc, behind the kernels of both field forms.

#define PF_SEARCH_MAX_CAND (1 << 24)   /* candidates of one call: 16.8e6 candidates of 1081 beams on a 100 000-point map: 9.0 ms measured (profiles/search.txt) */
#define PF_SEARCH_MAX_ENDS (1 << 24)   /* (2 half_theta + 1) * n_beams end points of one call: 128 MB */
#define PF_WIDE_MAX_CAND 2147483647LL  /* candidates of one branch-and-bound call: k stays a non-negative int32, the key stays S << 32 | k */
#define PF_WIDE_MAX_ROW (1 << 24)      /* (2 half_x + 1)(2 half_y + 1): the candidates of one heading of such a call */

// SEARCH-KERNEL-TEXT-BEGIN
#define PF_SEARCH_MAX_FIELD (1 << 26) /* field cells of one call: 128 MB */
#define PF_SEARCH_CELL_MAX 1048576 /* 2^20: an end point farther out counts as qcap */
#define PF_SEARCH_BIAS (1 << 21)
#define PF_SEARCH_SKIP (-2147483647 - 1) /* ends[].y: the beam is out of range and takes no part */
#define PF_SEARCH_BAD (-2147483647 - 1)  /* ends[].x: no cell -- the beam is out of range, or in range and counts as qcap for every candidate */
#define PF_SEARCH_NONE 2147483647  /* the score of a heading without an in-range beam */
#define PF_SEARCH_OUT 12           /* out: pose[3], 0, info[8] */

// pfslam_search_opts and what the host derives from them, by value
struct SearchParams {
    float cx, cy, ct, step_theta, res, u;
    int hx, hy, ht, stride, qcap, nb;
    int lox, hix, loy, hiy; // the host's bounds of the end-point cells: rint((c -+ 20) / res), inside +-2^20
    int cap;                // cells the field buffer holds: (hix - lox + 1 + 2 hx stride) * (hiy - loy + 1 + 2 hy stride), + 2 spare cells
};

// SearchParams from a call's arguments: the part of every entry point's prologue that needs neither the handle nor the device (a plain
// host function).  *out is complete when the call fits; a refusal brings its message's figures; SEARCH_QCAP does not depend on the centre.
enum SearchRefusal { SEARCH_FITS = 0, SEARCH_QCAP, SEARCH_FIELD };
struct SearchWhy { float qf; long long W, H; };
static inline SearchRefusal search_derive(float res, int nb, const float centre[3], int hx, int hy, int ht, int stride, float step_theta, float max_dist,
                                          SearchParams *out, SearchWhy *why)
{
    SearchParams &p = *out;
    p.res = res;
    p.u = (p.res * p.res) * 0.0625f;
    why->qf = rintf(pf::fdiv(max_dist * max_dist, p.u));
    if (!(why->qf >= 1.0f && why->qf <= 65535.0f)) return SEARCH_QCAP;
    p.cx = centre[0]; p.cy = centre[1]; p.ct = centre[2];
    p.step_theta = step_theta;
    p.hx = hx; p.hy = hy; p.ht = ht;
    p.stride = stride;
    p.qcap = (int)why->qf;
    p.nb = nb;
    auto cell_bound = [&](float c, float d) { // rint((c + d) / res) as k_search_ends computes it, inside +-2^20
        const float f = rintf(pf::fdiv(c + d, p.res));
        return (int)std::min(std::max(f, -(float)PF_SEARCH_CELL_MAX), (float)PF_SEARCH_CELL_MAX);
    };
    p.lox = cell_bound(p.cx, -PF_LIDAR_RANGE); p.hix = cell_bound(p.cx, PF_LIDAR_RANGE);
    p.loy = cell_bound(p.cy, -PF_LIDAR_RANGE); p.hiy = cell_bound(p.cy, PF_LIDAR_RANGE);
    const long long W = why->W = (long long)p.hix - p.lox + 1 + 2LL * p.hx * p.stride, H = why->H = (long long)p.hiy - p.loy + 1 + 2LL * p.hy * p.stride;
    if (W > PF_SEARCH_MAX_FIELD || H > PF_SEARCH_MAX_FIELD || W * H > PF_SEARCH_MAX_FIELD) return SEARCH_FIELD;
    p.cap = (int)(W * H);
    return SEARCH_FITS;
}

// The field of a call is the bounding box of the end-point cells of every heading, grown by the window: its extent is known only on
// the device, where k_search_ends merges it into four words that a memset of 0xff leaves "empty" (-1) and that only grow:
// box[0] = max(BIAS - ex), [1] = max(ex + BIAS), [2] and [3] the same in y; a valid ex lies in +-2^20, so the biased values are positive.
struct SearchBox { int x0, y0, W, H; };
__device__ __forceinline__ SearchBox search_box(const int *box, const SearchParams &p)
{
    if (box[0] < 0) return SearchBox{0, 0, 0, 0}; // no heading has a beam with a cell
    const int minx = PF_SEARCH_BIAS - box[0], maxx = box[1] - PF_SEARCH_BIAS, miny = PF_SEARCH_BIAS - box[2], maxy = box[3] - PF_SEARCH_BIAS;
    const int gx = p.hx * p.stride, gy = p.hy * p.stride;
    return SearchBox{minx - gx, miny - gy, maxx - minx + 1 + 2 * gx, maxy - miny + 1 + 2 * gy};
}

// One workgroup per heading, the beams strided over its 256 threads: the packed end-point cells of the heading, its in-range count and
// its share of the box.  (ex, ey) depend on the heading only; a translation of the window is an index shift.
__global__ __launch_bounds__(256) void k_search_ends(const float *__restrict__ scan, SearchParams p, int trig, int2 *__restrict__ ends,
                                                     int *__restrict__ nin, int *box)
{
    __shared__ int s_red[4][5];
    const int a = blockIdx.x;
    const float theta = p.ct + (float)(a - p.ht) * p.step_theta;
    int acc[5] = {0, -1, -1, -1, -1}; // in-range beams; the four box words
    for (int b = threadIdx.x; b < p.nb; b += 256) {
        float wx, wy;
        pf::clean_lidar_scan(b, scan[b], theta, wx, wy, trig);
        int2 e;
        e.x = PF_SEARCH_BAD;
        e.y = PF_SEARCH_SKIP;
        if (fabsf(wx) < PF_LIDAR_RANGE && fabsf(wy) < PF_LIDAR_RANGE) {
            acc[0]++;
            const float fx = rintf(pf::fdiv(p.cx + wx, p.res)), fy = rintf(pf::fdiv(p.cy + wy, p.res));
            e.y = 0;
            if (fabsf(fx) <= (float)PF_SEARCH_CELL_MAX && fabsf(fy) <= (float)PF_SEARCH_CELL_MAX) { // (false for a NaN)
                const int ex = (int)fx, ey = (int)fy;
                // The host's bounds hold for every such cell: |wx| < 20 and the sum, the division and rintf are monotone.  The test
                // is what keeps the field's loads and stores inside its buffer whatever the arithmetic does.
                if (ex >= p.lox && ex <= p.hix && ey >= p.loy && ey <= p.hiy) {
                    e.x = ex;
                    e.y = ey;
                    acc[1] = max(acc[1], PF_SEARCH_BIAS - ex);
                    acc[2] = max(acc[2], ex + PF_SEARCH_BIAS);
                    acc[3] = max(acc[3], PF_SEARCH_BIAS - ey);
                    acc[4] = max(acc[4], ey + PF_SEARCH_BIAS);
                }
            }
        }
        ends[(size_t)a * p.nb + b] = e;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        acc[0] += __shfl_xor(acc[0], off, 64);
        for (int k = 1; k < 5; k++) acc[k] = max(acc[k], __shfl_xor(acc[k], off, 64));
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 5; k++) s_red[threadIdx.x >> 6][k] = acc[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) {
            acc[0] += s_red[w][0];
            for (int k = 1; k < 5; k++) acc[k] = max(acc[k], s_red[w][k]);
        }
        nin[a] = acc[0];
        if (acc[1] >= 0)
            for (int k = 0; k < 4; k++) atomicMax(&box[k], acc[k + 1]);
    }
}

// One thread per cell of the box: q = min(rint(d2 / u), qcap) of the exact nearest node of the cell's lattice point.  The launch covers
// the `cap` cells the host bounds the box by; the threads behind the box leave at once.
__global__ __launch_bounds__(256) void k_search_field(pf::KdView tree, SearchParams p, const int *__restrict__ box, uint16_t *__restrict__ field)
{
    const SearchBox B = search_box(box, p);
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id == 0) { // the two spare cells behind the field (k_search_score)
        field[p.cap] = 0;
        field[p.cap + 1] = (uint16_t)p.qcap;
    }
    if (id >= B.W * B.H || id >= p.cap) return;
    const int kx = B.x0 + id % B.W, ky = B.y0 + id / B.W;
    float d2;
    pf::kd_nearest_exact(tree, (float)kx * p.res, (float)ky * p.res, 0.0f, &d2); // (no nearest node: d2 = +inf, the cell saturates)
    const float r = rintf(pf::fdiv(d2, p.u));
    field[id] = (uint16_t)(r >= (float)p.qcap ? p.qcap : (int)r);
}

// The hot path.  A workgroup is one wave: 64 adjacent candidates (i fastest, then j) of ONE heading, so every lane walks the same beam
// list -- the end-point cell of a beam is wave-uniform, read through the scalar path and shared by the 64 lanes -- and a wave's 64
// loads of a beam fall into the one or two lines of a field row per window row the wave spans (stride 1).  S is an integer sum: exact in
// any order.  The wave's smallest key (S << 32 | k) goes to the call's one 64-bit word with a vector atomicMin.
__global__ __launch_bounds__(64) void k_search_score(const int2 *__restrict__ ends, const int *__restrict__ nin, const int *__restrict__ box,
                                                     const uint16_t *__restrict__ field, SearchParams p, int chunks, int *__restrict__ scores,
                                                     unsigned long long *key)
{
    const int a = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int nx = 2 * p.hx + 1, row = nx * (2 * p.hy + 1);
    const int c = chunk * 64 + threadIdx.x;
    const bool live = c < row;
    const int k = a * row + c;
    if (nin[a] == 0) { // (the whole workgroup) a heading without an in-range beam takes no part in the pick
        if (live && scores) scores[k] = PF_SEARCH_NONE;
        return;
    }
    const SearchBox B = search_box(box, p);
    const int i = live ? c % nx : 0, j = live ? c / nx : 0;
    const int off = (j - p.hy) * p.stride * B.W + (i - p.hx) * p.stride; // the candidate's shift; |off| and every index below are bounded by cap
    const int2 *__restrict__ e = ends + (size_t)a * p.nb;
    int S = 0;
    // No branch in the loop, so that the loads of several beams are in flight at once: a beam that is out of range reads the field's
    // spare cell `cap` (0), an in-range beam without a cell the spare cell `cap + 1` (qcap); both choices are wave-uniform.
#pragma unroll 8
    for (int b = 0; b < p.nb; b++) {
        const int2 v = e[b];
        const bool cell = v.x != PF_SEARCH_BAD;
        const int lin = cell ? (v.y - B.y0) * B.W + (v.x - B.x0) : (v.y == PF_SEARCH_SKIP ? p.cap : p.cap + 1);
        S += (int)field[lin + (cell ? off : 0)];
    }
    if (live && scores) scores[k] = S;
    unsigned long long m = live ? ((unsigned long long)(unsigned)S << 32) | (unsigned)k : ~0ull;
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long t = __shfl_xor(m, o, 64);
        m = t < m ? t : m;
    }
    if (threadIdx.x == 0) atomicMin(key, m);
}

// The winner's pose and info from the key, on the device: the arithmetic of the specification under the library's compile flags.
__global__ void k_search_result(const unsigned long long *__restrict__ key, const int *__restrict__ nin, SearchParams p, float *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int nx = 2 * p.hx + 1, ny = 2 * p.hy + 1, row = nx * ny;
    const float cand = (float)(row * (2 * p.ht + 1));
    const unsigned long long kk = *key;
    out[3] = 0.0f;
    out[9] = cand;
    out[10] = (float)p.qcap;
    out[11] = 0.0f;
    if (kk == ~0ull) { // no heading has an in-range beam
        out[0] = p.cx; out[1] = p.cy; out[2] = p.ct;
        out[4] = 2.0f; out[5] = -1.0f; out[6] = out[7] = out[8] = 0.0f;
        return;
    }
    const int S = (int)(kk >> 32), k = (int)(kk & 0xffffffffull);
    const int a = k / row, j = (k % row) / nx, i = k % nx;
    out[0] = p.cx + (float)((i - p.hx) * p.stride) * p.res;
    out[1] = p.cy + (float)((j - p.hy) * p.stride) * p.res;
    out[2] = p.ct + (float)(a - p.ht) * p.step_theta;
    out[4] = 0.0f;
    out[5] = (float)k;
    out[6] = (float)nin[a];
    out[7] = pf::fdiv((float)S * p.u, (float)nin[a]);
    out[8] = (float)S;
}
// SEARCH-KERNEL-TEXT-END

extern "C" void pfslam_search_default_opts(pfslam_search_opts *o)
{
    if (!o) return;
    o->half_x = o->half_y = 20;
    o->half_theta = 16;
    o->stride = 1;
    o->step_theta = 0.0125f;
    o->max_dist = 0.2f;
    o->reserved_[0] = o->reserved_[1] = 0;
}

// grow one of the feature's own device buffers to `count` elements
template <typename T>
static int search_grow(T **buf, size_t *have, size_t count)
{
    if (count <= *have) return 0;
    if (*buf) HIPCHK(hipFree(*buf));
    *buf = nullptr;
    *have = 0;
    CHK(dalloc(buf, count));
    *have = count;
    return 0;
}

// What search_plan derives for every entry point: the kernels' parameters and the window's extent.  Then the forms of a call, or-ed.
struct SearchPlan { SearchParams p; long long nx, ny, na; size_t cand; };
#define PF_FORM_NO_MAP 1 /* the field comes from a reference scan: no map is needed, and a call without a centre takes ref_pose, not the handle's pose */
#define PF_FORM_WIDE 2   /* branch and bound: up to 2^31 - 1 candidates, 2^24 of one heading */

// The refusals every entry point shares, in their one order, worded under the caller's name `fn`; on success the device is current, the
// handle settled and *out filled.  An entry point checks its own arguments before and behind this call.
static int search_plan(pfslam_handle *h, const char *fn, int form, const float *ref_pose, const float centre[3], const pfslam_search_opts *opts, SearchPlan *out)
{
    const std::string name = std::string(fn) + ": ";
    auto finite3 = [](const float *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); };
    if (opts->half_x < 0 || opts->half_y < 0 || opts->half_theta < 0) return fail(name + "half_x, half_y and half_theta must be >= 0");
    if (opts->stride < 1 || opts->stride > 64) return fail(name + "stride must be 1 .. 64");
    if (!std::isfinite(opts->step_theta) || (opts->half_theta > 0 && !(opts->step_theta > 0.0f)))
        return fail(name + "step_theta must be finite, and > 0 unless half_theta is 0");
    if (!std::isfinite(opts->max_dist) || !(opts->max_dist > 0.0f)) return fail(name + "max_dist must be finite and > 0");
    if (opts->reserved_[0] || opts->reserved_[1]) return fail(name + "reserved_ must be 0");
    if (ref_pose && !finite3(ref_pose)) return fail(name + "the ref_pose must be finite");
    if (centre && !finite3(centre)) return fail(name + "the centre must be finite");
    const long long nx = 2LL * opts->half_x + 1, ny = 2LL * opts->half_y + 1, na = 2LL * opts->half_theta + 1;
    const bool wide = (form & PF_FORM_WIDE) != 0;
    if (wide && (nx > PF_WIDE_MAX_ROW || ny > PF_WIDE_MAX_ROW || nx * ny > PF_WIDE_MAX_ROW || nx * ny * na > PF_WIDE_MAX_CAND))
        return fail(name + "more than 2^31 - 1 candidates, or more than 2^24 of one heading ((2 half_x + 1)(2 half_y + 1))");
    if (!wide && (nx > PF_SEARCH_MAX_CAND || ny > PF_SEARCH_MAX_CAND || na > PF_SEARCH_MAX_CAND || nx * ny > PF_SEARCH_MAX_CAND || nx * ny * na > PF_SEARCH_MAX_CAND))
        return fail(name + "more than 2^24 candidates");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    if (!(form & PF_FORM_NO_MAP) && h->kd_size <= 0) return fail(name + "no map loaded");
    if (h->nb > PF_SUM_TILE) return fail(name + "n_beams > 4096 not supported");
    if (h->cfg.map_res_x != h->cfg.map_res_y) return fail(name + "map_res_x != map_res_y not supported");
    // the centre: given, the reference pose, or the handle's pose -- which is read only behind the two refusals that do not depend on it
    float c3[4] = {0, 0, 0, 0};
    const float *given = centre ? centre : ((form & PF_FORM_NO_MAP) ? ref_pose : nullptr);
    if (given) memcpy(c3, given, 12);
    SearchWhy why;
    char msg[240];
    auto derive = [&] {
        return search_derive(h->cfg.map_res_x, h->nb, c3, opts->half_x, opts->half_y, opts->half_theta, opts->stride, opts->step_theta, opts->max_dist, &out->p, &why);
    };
    SearchRefusal no = derive();
    if (no == SEARCH_QCAP) {
        snprintf(msg, sizeof(msg), "%s: max_dist %g gives qcap %g in units of res^2 / 16; it must be 1 .. 65535", fn, (double)opts->max_dist, (double)why.qf);
        return fail(msg);
    }
    if (na * h->nb > PF_SEARCH_MAX_ENDS) return fail(name + "more than 2^24 end points ((2 half_theta + 1) * n_beams)");
    if (!given) { // as pfslam_get_pose reads it (the one case with a second copy and wait: the field's bounds need it here)
        HIPCHK(hipMemcpyAsync(c3, h->pose, 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (!finite3(c3)) return fail(name + "the centre (the handle's pose) must be finite");
        no = derive();
    }
    if (no == SEARCH_FIELD) {
        snprintf(msg, sizeof(msg), "%s: the field would have %lld x %lld cells (40 m / res + 1 + 2 half stride a side); at most 2^26 cells", fn, why.W, why.H);
        return fail(msg);
    }
    out->nx = nx; out->ny = ny; out->na = na;
    out->cand = (size_t)(nx * ny * na);
    return 0;
}

// The one volume runner of the four windowed entry points, defined in pfslam_search_cov.hip.inc (`cov` NULL: no reduction).
static int search_volume(pfslam_handle *h, const char *fn, int form, const float *ref_scan_host, const float ref_pose[3], const float *scan_host, const float centre[3],
                         const pfslam_search_opts *opts, const pfslam_cov_opts *cov, float pose_out[3], float info[8], float cov_out[16], int32_t *scores);

extern "C" int pfslam_search(pfslam_handle *h, const float centre[3], const pfslam_search_opts *opts, float pose_out[3], float info[8],
                             int32_t *scores)
{
    if (!h || !opts || !pose_out || !info) return fail("pfslam_search: bad argument");
    return search_volume(h, "pfslam_search", 0, nullptr, nullptr, nullptr, centre, opts, nullptr, pose_out, info, nullptr, scores);
}
