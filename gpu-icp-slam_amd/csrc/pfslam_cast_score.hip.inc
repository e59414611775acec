// pfslam_cast_score.hip.inc -- pfslam_cast_score: the beam-model comparison of a measured scan with the scan pfslam_cast expects from each
// pose of a list, of the handle's pose or of the handle's own particles, fused into the cast and reduced to eight integers per pose on the
// device; the specification is in include/pfslam.h.  Included by pfslam_hip.hip behind pfslam_cast.hip.inc (same translation unit): the
// raster, its buffers, cast_walk, cast_check_opts, cast_build_raster, cast_params and cast_stats are the cast's as they are.
// tests/test_cast_score_kernel_text.py cuts the text between the two CAST-SCORE-KERNEL-TEXT marks out and runs it on the CPU.

#define PF_CAST_SCORE_MAX_BEAMS 4096

// CAST-SCORE-KERNEL-TEXT-BEGIN
#define PF_CAST_SCORE_ROW 8 /* ints of a row: valid, agree, through, short, valid misses, Q1, Q2, cost (on the device: the pose's hits) */

// pfslam_cast_score_opts as the kernel needs them, by value: u = tol / 16, qcap = rint(clip / u)
struct CastScoreParams {
    float tol, u, z_min, z_max;
    int qcap, count_miss;
};

// One lane per ray, adjacent lanes the adjacent beams of one pose, as in the cast; the rays of a wave run across pose boundaries (a wave
// of 64 rays holds up to 64 poses when n_beams is 1).  The pose r is (px[r * ps], py[r * ps], pth[r * ps]): a list of (x, y, theta) rows is
// (base, base + 1, base + 2) with ps = 3, the particle block its three arrays with ps = 1.  A lane has the seven counters of its one beam
// and its hit in registers; a wave adds them up by pose with a segmented reduction (the lanes of a pose are contiguous: after the step
// `off` a lane holds the sum of the up to 2 * off lanes from itself on that share its pose), and the first lane of every pose in the wave
// adds what is not zero to the pose's row.  The rows are cleared before the launch.  Every sum is an integer below 2^31 (4096 beams x
// qcap <= 32767): exact in any order.  On the device a row's last word is the pose's hits, valid or not; the host sums them into
// stats[1] and puts the cost there (pfslam_cast_score below), so no two waves of different poses ever add to one address.
// (Measured against one 256-thread workgroup per pose with the beams strided over its threads and the rows stored, not added:
// profiles/cast_score.txt.)
template <bool SKIP>
__global__ __launch_bounds__(256) void k_cast_score(const float *__restrict__ px, const float *__restrict__ py, const float *__restrict__ pth,
                                                    int ps, const float *__restrict__ scan, int rays, CastParams p, CastScoreParams s, CastBox B,
                                                    const unsigned long long *__restrict__ tiles, int *rows, uint8_t *__restrict__ classes)
{
    const int id = blockIdx.x * 256 + threadIdx.x; // (rays <= 2^28)
    const bool live = id < rays;                    // (a lane behind the last ray stays for the wave's shuffles; it casts nothing)
    const int r = live ? id / p.nb : -1, b = live ? id - r * p.nb : 0;
    int acc[PF_CAST_SCORE_ROW] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
        const float x = px[(size_t)r * ps], y = py[(size_t)r * ps], theta = pth[(size_t)r * ps];
        float wx, wy;
        pf::clean_lidar_scan(b, p.max_range, theta, wx, wy, p.trig);
        int hx = 0, hy = 0;
        float e = 0.0f;
        const int hit = cast_walk<SKIP>(x, y, wx, wy, p, B, tiles, hx, hy, e);
        acc[7] = hit;
        const float z = scan[b];
        int cls = 0;
        if (z >= s.z_min && z <= s.z_max) { // (false for a NaN)
            acc[0] = 1;
            if (!hit) {
                cls = 1;
                acc[4] = 1;
            } else {
                const float d = z - e, a = fabsf(d);
                const float fq = rintf(pf::fdiv(a, s.u));
                const int q = fq >= (float)s.qcap ? s.qcap : (int)fq; // (the compare first: a huge a has a defined result)
                cls = a <= s.tol ? 2 : (d > s.tol ? 3 : 4);
                acc[1] = cls == 2;
                acc[2] = cls == 3;
                acc[3] = cls == 4;
                acc[5] = q;
                if (cls == 2) acc[6] = q * q; // (q <= 16 here)
            }
        }
        if (classes) classes[id] = (uint8_t)cls;
    }
    const int lane = threadIdx.x & 63;
    for (int off = 1; off <= 32; off <<= 1) {
        const bool same = __shfl_down(r, off, 64) == r && lane + off < 64;
        for (int k = 0; k < PF_CAST_SCORE_ROW; k++) {
            const int other = __shfl_down(acc[k], off, 64);
            if (same) acc[k] += other;
        }
    }
    if (live && (lane == 0 || b == 0)) // the first lane of its pose in this wave
        for (int k = 0; k < PF_CAST_SCORE_ROW; k++)
            if (acc[k]) atomicAdd(&rows[(size_t)r * PF_CAST_SCORE_ROW + k], acc[k]);
}
// CAST-SCORE-KERNEL-TEXT-END

extern "C" void pfslam_cast_score_default_opts(pfslam_cast_score_opts *o)
{
    if (!o) return;
    o->tol = 0.1f;
    o->clip = 1.0f;
    o->z_min = 0.1f;
    o->z_max = 20.0f;
    o->count_miss = 1;
    o->source = 0;
    o->reserved_[0] = o->reserved_[1] = 0;
}

extern "C" int pfslam_cast_score(pfslam_handle *h, const float *poses, int m, const float *scan_host, const pfslam_cast_opts *cast,
                                 const pfslam_cast_score_opts *opts, int32_t *rows_out, uint8_t *classes_out, int *best, int64_t stats[8])
{
    if (!h || !cast || !opts || !rows_out) return fail("pfslam_cast_score: bad argument");
    if (m < 1 || m > PF_CAST_MAX_POSES) return fail("pfslam_cast_score: m must be 1 .. 65536");
    if (h->nb > PF_CAST_SCORE_MAX_BEAMS) return fail("pfslam_cast_score: n_beams must be <= 4096");
    if (opts->source < 0 || opts->source > 1) return fail("pfslam_cast_score: source must be 0 .. 1");
    if (opts->source == 0 && !poses && m != 1) return fail("pfslam_cast_score: poses NULL (the handle's pose) needs m == 1");
    if (opts->source == 1 && (poses || m != h->n)) return fail("pfslam_cast_score: source 1 (the handle's particles) needs poses NULL and m == n_particles");
    if (classes_out && (long long)m * h->nb > PF_CAST_MAX_RAYS) return fail("pfslam_cast_score: classes_out with more than 2^24 rays (m * n_beams)");
    CHK(cast_check_opts(h, cast, "pfslam_cast_score"));
    if (!std::isfinite(opts->tol) || !(opts->tol >= 1e-4f)) return fail("pfslam_cast_score: tol must be finite and >= 1e-4");
    if (!std::isfinite(opts->clip)) return fail("pfslam_cast_score: clip must be finite");
    if (!std::isfinite(opts->z_min) || !std::isfinite(opts->z_max) || !(opts->z_min <= opts->z_max))
        return fail("pfslam_cast_score: z_min and z_max must be finite, z_min <= z_max");
    if (opts->count_miss < 0 || opts->count_miss > 1) return fail("pfslam_cast_score: count_miss must be 0 or 1");
    if (opts->reserved_[0] || opts->reserved_[1]) return fail("pfslam_cast_score: reserved_ must be 0");
    CastScoreParams s;
    s.tol = opts->tol;
    s.u = opts->tol * 0.0625f;
    s.z_min = opts->z_min;
    s.z_max = opts->z_max;
    s.count_miss = opts->count_miss;
    const float fcap = rintf(pf::fdiv(opts->clip, s.u));
    if (!(fcap >= 16.0f && fcap <= 32767.0f)) return fail("pfslam_cast_score: qcap = rint(clip / (tol / 16)) must be 16 .. 32767");
    s.qcap = (int)fcap;
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    if (h->kd_size <= 0) return fail("pfslam_cast_score: no map loaded");
    const CastParams p = cast_params(h, cast);
    CastBox B;
    int nq;
    CHK(cast_build_raster(h, p, "pfslam_cast_score", B, nq));
    const size_t rays = (size_t)m * h->nb;
    CHK(search_grow(&h->cscore_rows, &h->cscore_rows_cap, (size_t)m * PF_CAST_SCORE_ROW));
    if (classes_out) CHK(search_grow(&h->cscore_classes, &h->cscore_classes_cap, rays));
    const float *scan = h->scan; // read on the device
    if (scan_host) {
        CHK(search_grow(&h->cscore_scan, &h->cscore_scan_cap, (size_t)h->nb));
        // (the caller's arrays are pageable: they are consumed before the call returns, behind its last wait)
        HIPCHK(hipMemcpyAsync(h->cscore_scan, scan_host, (size_t)h->nb * 4, hipMemcpyHostToDevice, h->stream));
        scan = h->cscore_scan;
    }
    const float *px = h->pose, *py = h->pose + 1, *pth = h->pose + 2; // read on the device
    int ps = 3;
    if (opts->source == 1) {
        px = h->x; py = h->y; pth = h->th;
        ps = 1;
    } else if (poses) {
        CHK(search_grow(&h->cast_poses, &h->cast_poses_cap, (size_t)3 * m));
        HIPCHK(hipMemcpyAsync(h->cast_poses, poses, (size_t)m * 12, hipMemcpyHostToDevice, h->stream));
        px = h->cast_poses; py = px + 1; pth = px + 2;
    }
    HIPCHK(hipMemsetAsync(h->cscore_rows, 0, (size_t)m * PF_CAST_SCORE_ROW * 4, h->stream));
    hipLaunchKernelGGL(k_cast_score<true>, dim3((unsigned)((rays + 255) / 256)), dim3(256), 0, h->stream, px, py, pth, ps, scan, (int)rays, p, s, B,
                       (const unsigned long long *)h->cast_tiles, h->cscore_rows, classes_out ? h->cscore_classes : nullptr);
    HIPCHK(hipGetLastError());
    // (the caller's arrays are written only when the whole call has succeeded)
    std::vector<int32_t> rw((size_t)m * PF_CAST_SCORE_ROW);
    std::vector<uint8_t> cl(classes_out ? rays : 0);
    int st[PF_CAST_STATE];
    HIPCHK(hipMemcpyAsync(rw.data(), h->cscore_rows, rw.size() * 4, hipMemcpyDeviceToHost, h->stream));
    if (classes_out) HIPCHK(hipMemcpyAsync(cl.data(), h->cscore_classes, rays, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(st, h->cast_state, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    // the device's rows end with the pose's hits: they go into stats[1], and the cost takes their place
    long long hits = 0;
    for (int r = 0; r < m; r++) {
        int32_t *row = &rw[(size_t)r * PF_CAST_SCORE_ROW];
        hits += row[7];
        row[7] = row[5] + (s.count_miss ? s.qcap * row[4] : 0);
    }
    st[6] = (int)hits; // (at most 2^28 rays)
    memcpy(rows_out, rw.data(), rw.size() * 4);
    if (classes_out) memcpy(classes_out, cl.data(), rays);
    if (best) {
        // among the rows with an agreeing beam: the smallest cost, then the larger agree, then the lowest row
        int at = -1;
        for (int r = 0; r < m; r++) {
            const int32_t *row = &rw[(size_t)r * PF_CAST_SCORE_ROW];
            if (row[1] <= 0) continue;
            const int32_t *win = at < 0 ? nullptr : &rw[(size_t)at * PF_CAST_SCORE_ROW];
            if (!win || row[7] < win[7] || (row[7] == win[7] && row[1] > win[1])) at = r;
        }
        *best = at;
    }
    if (stats) cast_stats(stats, (int64_t)rays, st, B);
    return 0;
}
