// pfslam_cast.hip.inc -- pfslam_cast (the scan the point-cloud map predicts from a pose: every beam walked through a raster of the map's
// nodes until it meets an occupied cell) and pfslam_map_raster (that raster, for export); the specification is in include/pfslam.h.
// Included by pfslam_hip.hip behind pfslam_search_best.hip.inc (same translation unit): it reuses pf::clean_lidar_scan, pf::fdiv,
// pf::fsqrt and search_grow as they are and shares no buffer with another entry point.
// tests/test_cast_kernel_text.py cuts the text between the two CAST-KERNEL-TEXT marks out and runs it on the CPU.

#define PF_CAST_MAX_POSES 65536
#define PF_CAST_MAX_RAYS (1 << 24)  /* m * n_beams of one call: 64 MB of ranges, 128 MB of cells */
#define PF_CAST_MAX_CELLS (1 << 28) /* W * H of the raster: 32 MB of tiles, 256 MB of pfslam_map_raster's bytes */
#define PF_CAST_MAX_STEPS 16384.0f  /* max_range / res: 2 t |d| + n of the walk stays below 2^31 */

// CAST-KERNEL-TEXT-BEGIN
#define PF_CAST_CELL_MAX 1048576 /* 2^20: a node or a ray end farther out takes no part */
#define PF_CAST_BIAS (1 << 21)
#define PF_CAST_MISS (-2147483647 - 1) /* both cell words of a ray that hits nothing */
#define PF_CAST_STATE 8 /* ints: the four box words (k_search_ends' scheme), qualifying nodes, |O|, hits, spare */

// pfslam_cast_opts and what the host derives from the handle, by value
struct CastParams {
    float res_x, res_y, max_range, w_min, no_hit;
    int inflate, skip, nb, trig;
};
// The raster of a call: the box of the specification, cut into tiles of 8 x 8 cells.  A tile is one 64-bit word, bit (lx * 8 + ly) the
// cell (x0 + 8 tx + lx, y0 + 8 ty + ly); the tiles lie column by column, word tx * TH + ty.  The host reads the box words after
// k_cast_box (the call's one extra wait: the raster's size follows from them) and hands the box to the kernels behind it by value.
struct CastBox { int x0, y0, W, H, TH; };

// the cell of a node and whether it qualifies: every test is false for a NaN
__device__ __forceinline__ bool cast_node_cell(const uint4 nd, float w, const CastParams &p, int &nx, int &ny)
{
    const float fx = rintf(pf::fdiv(__uint_as_float(nd.x), p.res_x)), fy = rintf(pf::fdiv(__uint_as_float(nd.y), p.res_y));
    if (!(w >= p.w_min && fabsf(fx) <= (float)PF_CAST_CELL_MAX && fabsf(fy) <= (float)PF_CAST_CELL_MAX)) return false;
    nx = (int)fx;
    ny = (int)fy;
    return true;
}

// One thread per node: the bounding box of the qualifying cells and their number.  A wave merges its lanes with shuffles and adds one
// set of atomics; the box words are k_search_ends': a memset of 0xff leaves them "empty" (-1), they only grow, and a cell inside +-2^20
// keeps the biased values positive.
__global__ __launch_bounds__(256) void k_cast_box(const uint4 *__restrict__ hot, const float *__restrict__ w, int n, CastParams p, int *st)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    int acc[5] = {0, -1, -1, -1, -1};
    int nx, ny;
    if (i < n && cast_node_cell(hot[i], w[i], p, nx, ny)) {
        acc[0] = 1;
        acc[1] = PF_CAST_BIAS - nx;
        acc[2] = nx + PF_CAST_BIAS;
        acc[3] = PF_CAST_BIAS - ny;
        acc[4] = ny + PF_CAST_BIAS;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        acc[0] += __shfl_xor(acc[0], off, 64);
        for (int k = 1; k < 5; k++) acc[k] = max(acc[k], __shfl_xor(acc[k], off, 64));
    }
    if ((threadIdx.x & 63) == 0 && acc[0] > 0) {
        for (int k = 0; k < 4; k++) atomicMax(&st[k], acc[k + 1]);
        atomicAdd(&st[4], acc[0]);
    }
}

// One thread per node: a qualifying node sets the (2 inflate + 1)^2 cells around its own, at most 17 x 17 cells in 3 x 3 tiles, with one
// 64-bit OR per tile.  An OR is exact in any order.  The box holds every such cell by construction; the clip against it is what keeps
// the stores inside the buffer whatever the arithmetic does.
__global__ __launch_bounds__(256) void k_cast_splat(const uint4 *__restrict__ hot, const float *__restrict__ w, int n, CastParams p, CastBox B,
                                                    unsigned long long *tiles)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    int nx, ny;
    if (i >= n || !cast_node_cell(hot[i], w[i], p, nx, ny)) return;
    const int xlo = max(nx - p.inflate - B.x0, 0), xhi = min(nx + p.inflate - B.x0, B.W - 1);
    const int ylo = max(ny - p.inflate - B.y0, 0), yhi = min(ny + p.inflate - B.y0, B.H - 1);
    if (xlo > xhi || ylo > yhi) return;
    for (int tx = xlo >> 3; tx <= xhi >> 3; tx++) {
        const int a = max(xlo - 8 * tx, 0), b = min(xhi - 8 * tx, 7);
        const unsigned long long cols = (~0ull >> (64 - 8 * (b - a + 1))) << (8 * a);
        for (int ty = ylo >> 3; ty <= yhi >> 3; ty++) {
            const int c = max(ylo - 8 * ty, 0), d = min(yhi - 8 * ty, 7);
            const unsigned long long rows = (unsigned long long)(((1u << (d - c + 1)) - 1u) << c) * 0x0101010101010101ull;
            atomicOr(&tiles[(size_t)tx * B.TH + ty], cols & rows);
        }
    }
}

// One thread per tile: |O|.  (A tile's bits outside the box are never set.)
__global__ __launch_bounds__(256) void k_cast_count(const unsigned long long *__restrict__ tiles, int ntiles, int *st)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    int c = i < ntiles ? __popcll(tiles[i]) : 0;
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c > 0) atomicAdd(&st[5], c);
}

// The smallest t whose minor offset (2 t adm + n) div (2 n) reaches q; n + 1 when no t of the walk does (the offset ends at adm).
// (2 q - 1) n stays below 2^31: q <= adm <= n here, and n is bounded by max_range / res + 2.
__device__ __forceinline__ int cast_reach(int q, int adm, int n)
{
    if (q <= 0) return 0;
    if (q > adm) return n + 1;
    return ((2 * q - 1) * n + 2 * adm - 1) / (2 * adm);
}

// The walk of one ray, for k_cast_rays and for k_cast_score (pfslam_cast_score.hip.inc): from the pose (x, y) towards (x + wx, y + wy); 1
// and the hit's cell and range, or 0 and the three left as they were.  The walk's cell is a closed form of its index t (the
// specification), which lets a ray jump:
//   * the t for which the ray is inside the box form one interval, found up front -- a ray that starts outside enters by it;
//   * an empty tile is left at once, for the first t that leaves it along either axis (SKIP).
// Inside a tile that holds something the walk steps cell by cell; between two jumps the minor offset is carried with its remainder
// (o, rem: 2 t adm + n == o * 2 n + rem), which is the closed form without its division.  !SKIP is the plain walk: every cell of
// t = skip .. n is tested against the box and the raster.  The test against the box stays in both forms: it keeps the loads inside the
// buffer whatever the arithmetic does.
template <bool SKIP>
__device__ __forceinline__ int cast_walk(float x, float y, float wx, float wy, const CastParams &p, const CastBox &B,
                                         const unsigned long long *__restrict__ tiles, int &hx, int &hy, float &range)
{
    const float fsx = rintf(pf::fdiv(x, p.res_x)), fex = rintf(pf::fdiv(x + wx, p.res_x));
    const float fsy = rintf(pf::fdiv(y, p.res_y)), fey = rintf(pf::fdiv(y + wy, p.res_y));
    const float lim = (float)PF_CAST_CELL_MAX;
    int hit = 0;
    if (fabsf(fsx) <= lim && fabsf(fex) <= lim && fabsf(fsy) <= lim && fabsf(fey) <= lim) { // (false for a NaN and for an infinity)
        const int sx = (int)fsx, sy = (int)fsy, dx = (int)fex - sx, dy = (int)fey - sy;
        const int adx = abs(dx), ady = abs(dy), n = max(adx, ady);
        const bool xmajor = adx >= ady;
        // M: the axis that moves one cell per step; m: the other one
        const int sM = xmajor ? sx : sy, sm = xmajor ? sy : sx, adm = xmajor ? ady : adx;
        const int dM = xmajor ? dx : dy, dm = xmajor ? dy : dx;
        const int gM = dM > 0 ? 1 : -1, gm = dm > 0 ? 1 : (dm < 0 ? -1 : 0);
        const int M0 = xmajor ? B.x0 : B.y0, ML = xmajor ? B.W : B.H, m0 = xmajor ? B.y0 : B.x0, mL = xmajor ? B.H : B.W;
        int t = p.skip, tend = n > 0 ? n : -1;
        if (SKIP && n > 0) {
            // inside the box along M for t in [lo, hi]; along m while the offset lies in [qlo, qhi]
            const int lo = gM > 0 ? M0 - sM : sM - (M0 + ML - 1), hi = gM > 0 ? M0 + ML - 1 - sM : sM - M0;
            const int qlo = gm >= 0 ? m0 - sm : sm - (m0 + mL - 1), qhi = gm >= 0 ? m0 + mL - 1 - sm : sm - m0;
            t = max(t, max(lo, cast_reach(qlo, adm, n)));
            tend = min(tend, hi);
            if (qhi < 0) tend = -1;
            else tend = min(tend, cast_reach(qhi + 1, adm, n) - 1);
        }
        const int n2 = 2 * n;
        int o = 0, rem = 0, tile_at = -1;
        unsigned long long word = 0;
        bool fresh = true; // (o, rem) must be set from t
        while (t <= tend) {
            if (fresh) {
                const int num = 2 * t * adm + n;
                o = num / n2;
                rem = num - o * n2;
                fresh = false;
            }
            const int kM = sM + gM * t, km = sm + gm * o;
            const int kx = xmajor ? kM : km, ky = xmajor ? km : kM;
            const int cx = kx - B.x0, cy = ky - B.y0;
            if ((unsigned)cx < (unsigned)B.W && (unsigned)cy < (unsigned)B.H) {
                const int tile = (cx >> 3) * B.TH + (cy >> 3);
                if (tile != tile_at) {
                    word = tiles[tile];
                    tile_at = tile;
                }
                if (SKIP && word == 0ull) {
                    // the first t outside this tile: kM passes its far edge, or the offset reaches the edge along m
                    const int cM = xmajor ? cx : cy, cm = xmajor ? cy : cx;
                    const int eM = M0 + (cM & ~7), em = m0 + (cm & ~7);
                    const int tM = gM > 0 ? eM + 8 - sM : sM - eM + 1;
                    const int tm = gm >= 0 ? cast_reach(em + 8 - sm, adm, n) : cast_reach(sm - em + 1, adm, n);
                    t = max(t + 1, min(tM, tm)); // (both lie behind t: the cell of t is in the tile)
                    fresh = true;
                    continue;
                }
                if ((word >> ((cx & 7) * 8 + (cy & 7))) & 1ull) {
                    hx = kx;
                    hy = ky;
                    const float ddx = (float)kx * p.res_x - x, ddy = (float)ky * p.res_y - y;
                    range = pf::fsqrt(ddx * ddx + ddy * ddy);
                    hit = 1;
                    break;
                }
            }
            t++;
            rem += 2 * adm;
            if (rem >= n2) {
                rem -= n2;
                o++;
            }
        }
    }
    return hit;
}

// The cast.  One lane per ray, adjacent lanes the adjacent beams of one pose: their walks start in the same cell and fan out, so a wave's
// loads fall into few tiles.
template <bool SKIP>
__global__ __launch_bounds__(256) void k_cast_rays(const float *__restrict__ poses, int rays, CastParams p, CastBox B,
                                                   const unsigned long long *__restrict__ tiles, float *__restrict__ ranges,
                                                   int *__restrict__ cells, int *st)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    const bool live = id < rays; // (a lane behind the last ray stays for the wave's count of the hits; it casts nothing)
    const int r = live ? id / p.nb : 0, b = live ? id - r * p.nb : 0;
    const float x = poses[3 * r], y = poses[3 * r + 1], theta = poses[3 * r + 2];
    float wx, wy;
    pf::clean_lidar_scan(b, p.max_range, theta, wx, wy, p.trig);
    int hx = PF_CAST_MISS, hy = PF_CAST_MISS;
    float range = p.no_hit;
    int hit = live ? cast_walk<SKIP>(x, y, wx, wy, p, B, tiles, hx, hy, range) : 0;
    for (int off = 32; off >= 1; off >>= 1) hit += __shfl_xor(hit, off, 64);
    if ((threadIdx.x & 63) == 0 && hit > 0) atomicAdd(&st[6], hit); // one add per wave
    if (!live) return;
    ranges[id] = range;
    if (cells) {
        int2 c;
        c.x = hx;
        c.y = hy;
        ((int2 *)cells)[id] = c; // (the buffer is an allocation of its own: 8-byte aligned)
    }
}

// pfslam_map_raster's bytes: one thread per cell, occ[(kx - x0) * H + (ky - y0)]
__global__ __launch_bounds__(256) void k_cast_expand(const unsigned long long *__restrict__ tiles, CastBox B, uint8_t *__restrict__ occ)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= B.W * B.H) return; // (W * H <= 2^28)
    const int cx = id / B.H, cy = id - cx * B.H;
    occ[id] = (uint8_t)((tiles[(size_t)(cx >> 3) * B.TH + (cy >> 3)] >> ((cx & 7) * 8 + (cy & 7))) & 1ull);
}
// CAST-KERNEL-TEXT-END

extern "C" void pfslam_cast_default_opts(pfslam_cast_opts *o)
{
    if (!o) return;
    o->max_range = 30.0f;
    o->w_min = 1.0f;
    o->no_hit = 30.0f;
    o->inflate = 1;
    o->skip_cells = 1;
    o->reserved_[0] = o->reserved_[1] = o->reserved_[2] = 0;
}

// the options' ranges, for both entry points; `who` is the function's name
static int cast_check_opts(const pfslam_handle *h, const pfslam_cast_opts *o, const char *who)
{
    const std::string f = std::string(who) + ": ";
    if (!std::isfinite(o->max_range) || !(o->max_range > 0.0f)) return fail(f + "max_range must be finite and > 0");
    if (!std::isfinite(o->w_min)) return fail(f + "w_min must be finite");
    if (o->inflate < 0 || o->inflate > 8) return fail(f + "inflate must be 0 .. 8");
    if (o->skip_cells < 0) return fail(f + "skip_cells must be >= 0");
    if (o->reserved_[0] || o->reserved_[1] || o->reserved_[2]) return fail(f + "reserved_ must be 0");
    if (!(pf::fdiv(o->max_range, h->cfg.map_res_x) <= PF_CAST_MAX_STEPS && pf::fdiv(o->max_range, h->cfg.map_res_y) <= PF_CAST_MAX_STEPS))
        return fail(f + "max_range / map_res_x and max_range / map_res_y must be <= 16384");
    return 0;
}

// The raster of a call, for both entry points: the box pass, the call's extra wait (the box and with it the raster's size are known on the
// device only), then the clear, the splat and the count.  Leaves the box in B, the state words on the device.
static int cast_build_raster(pfslam_handle *h, const CastParams &p, const char *who, CastBox &B, int &nq)
{
    if (!h->cast_state) CHK(dalloc(&h->cast_state, (size_t)PF_CAST_STATE));
    HIPCHK(hipMemsetAsync(h->cast_state, 0xff, 16, h->stream));
    HIPCHK(hipMemsetAsync(h->cast_state + 4, 0, 16, h->stream));
    const unsigned nblk = (unsigned)((h->kd_size + 255) / 256);
    hipLaunchKernelGGL(k_cast_box, dim3(nblk), dim3(256), 0, h->stream, (const uint4 *)h->hot, (const float *)h->kw, h->kd_size, p, h->cast_state);
    HIPCHK(hipGetLastError());
    int st[5];
    HIPCHK(hipMemcpyAsync(st, h->cast_state, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    nq = st[4];
    B = CastBox{0, 0, 0, 0, 0};
    if (st[0] < 0) return 0; // no qualifying node
    const int minx = PF_CAST_BIAS - st[0], maxx = st[1] - PF_CAST_BIAS, miny = PF_CAST_BIAS - st[2], maxy = st[3] - PF_CAST_BIAS;
    B.x0 = minx - p.inflate;
    B.y0 = miny - p.inflate;
    B.W = maxx - minx + 1 + 2 * p.inflate;
    B.H = maxy - miny + 1 + 2 * p.inflate;
    B.TH = (B.H + 7) / 8;
    if ((long long)B.W * B.H > PF_CAST_MAX_CELLS) {
        char msg[200];
        snprintf(msg, sizeof(msg), "%s: the raster would have %d x %d cells; at most 2^28 cells", who, B.W, B.H);
        return fail(msg);
    }
    const size_t ntiles = (size_t)((B.W + 7) / 8) * B.TH;
    CHK(search_grow(&h->cast_tiles, &h->cast_tiles_cap, ntiles));
    HIPCHK(hipMemsetAsync(h->cast_tiles, 0, ntiles * 8, h->stream));
    hipLaunchKernelGGL(k_cast_splat, dim3(nblk), dim3(256), 0, h->stream, (const uint4 *)h->hot, (const float *)h->kw, h->kd_size, p, B, h->cast_tiles);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_cast_count, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, h->stream, (const unsigned long long *)h->cast_tiles, (int)ntiles,
                       h->cast_state);
    HIPCHK(hipGetLastError());
    return 0;
}

static CastParams cast_params(const pfslam_handle *h, const pfslam_cast_opts *o)
{
    CastParams p;
    p.res_x = h->cfg.map_res_x; p.res_y = h->cfg.map_res_y;
    p.max_range = o->max_range; p.w_min = o->w_min; p.no_hit = o->no_hit;
    p.inflate = o->inflate; p.skip = o->skip_cells;
    p.nb = h->nb; p.trig = h->trig;
    return p;
}

static void cast_stats(int64_t stats[8], int64_t rays, const int st[PF_CAST_STATE], const CastBox &B)
{
    stats[0] = rays; stats[1] = rays ? st[6] : 0; stats[2] = st[4]; stats[3] = st[5];
    stats[4] = B.x0; stats[5] = B.y0; stats[6] = B.W; stats[7] = B.H;
}

extern "C" int pfslam_cast(pfslam_handle *h, const float *poses, int m, const pfslam_cast_opts *opts, float *ranges_out, int32_t *cells_out,
                           int64_t stats[8])
{
    if (!h || !opts || !ranges_out) return fail("pfslam_cast: bad argument");
    if (m < 1 || m > PF_CAST_MAX_POSES) return fail("pfslam_cast: m must be 1 .. 65536");
    if ((long long)m * h->nb > PF_CAST_MAX_RAYS) return fail("pfslam_cast: more than 2^24 rays (m * n_beams)");
    if (!poses && m != 1) return fail("pfslam_cast: poses NULL (the handle's pose) needs m == 1");
    CHK(cast_check_opts(h, opts, "pfslam_cast"));
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    if (h->kd_size <= 0) return fail("pfslam_cast: no map loaded");
    const CastParams p = cast_params(h, opts);
    const int rays = m * h->nb;
    CastBox B;
    int nq;
    CHK(cast_build_raster(h, p, "pfslam_cast", B, nq));
    CHK(search_grow(&h->cast_ranges, &h->cast_ranges_cap, (size_t)rays));
    if (cells_out) CHK(search_grow(&h->cast_cells, &h->cast_cells_cap, (size_t)2 * rays));
    const float *from = h->pose; // read on the device
    if (poses) {
        CHK(search_grow(&h->cast_poses, &h->cast_poses_cap, (size_t)3 * m));
        // (the caller's array is pageable: it is consumed before the call returns, behind its last wait)
        HIPCHK(hipMemcpyAsync(h->cast_poses, poses, (size_t)m * 12, hipMemcpyHostToDevice, h->stream));
        from = h->cast_poses;
    }
    hipLaunchKernelGGL(k_cast_rays<true>, dim3((unsigned)((rays + 255) / 256)), dim3(256), 0, h->stream, from, rays, p, B,
                       (const unsigned long long *)h->cast_tiles, h->cast_ranges, cells_out ? h->cast_cells : nullptr, h->cast_state);
    HIPCHK(hipGetLastError());
    // (the caller's arrays are written only when the whole call has succeeded)
    std::vector<float> rg((size_t)rays);
    std::vector<int32_t> ce(cells_out ? (size_t)2 * rays : 0);
    int st[PF_CAST_STATE];
    HIPCHK(hipMemcpyAsync(rg.data(), h->cast_ranges, (size_t)rays * 4, hipMemcpyDeviceToHost, h->stream));
    if (cells_out) HIPCHK(hipMemcpyAsync(ce.data(), h->cast_cells, (size_t)rays * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(st, h->cast_state, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(ranges_out, rg.data(), (size_t)rays * 4);
    if (cells_out) memcpy(cells_out, ce.data(), (size_t)rays * 8);
    if (stats) cast_stats(stats, rays, st, B);
    return 0;
}

extern "C" int pfslam_map_raster(pfslam_handle *h, const pfslam_cast_opts *opts, int64_t stats[8], uint8_t *occ, size_t cap)
{
    if (!h || !opts || !stats) return fail("pfslam_map_raster: bad argument");
    CHK(cast_check_opts(h, opts, "pfslam_map_raster"));
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    if (h->kd_size <= 0) return fail("pfslam_map_raster: no map loaded");
    const CastParams p = cast_params(h, opts);
    CastBox B;
    int nq;
    CHK(cast_build_raster(h, p, "pfslam_map_raster", B, nq));
    const size_t ncell = (size_t)B.W * B.H;
    if (occ && cap < ncell) {
        char msg[200];
        snprintf(msg, sizeof(msg), "pfslam_map_raster: cap %zu is less than the raster's %d x %d cells", cap, B.W, B.H);
        return fail(msg);
    }
    if (occ && ncell) {
        CHK(search_grow(&h->cast_occ, &h->cast_occ_cap, ncell));
        hipLaunchKernelGGL(k_cast_expand, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, h->stream, (const unsigned long long *)h->cast_tiles, B, h->cast_occ);
        HIPCHK(hipGetLastError());
    }
    int st[PF_CAST_STATE];
    std::vector<uint8_t> bytes(occ ? ncell : 0);
    if (occ && ncell) HIPCHK(hipMemcpyAsync(bytes.data(), h->cast_occ, ncell, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(st, h->cast_state, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (occ && ncell) memcpy(occ, bytes.data(), ncell);
    cast_stats(stats, 0, st, B);
    return 0;
}
