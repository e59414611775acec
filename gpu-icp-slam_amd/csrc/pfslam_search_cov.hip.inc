// pfslam_search_cov.hip.inc -- pfslam_search_cov and pfslam_search_scan_cov (pfslam_search's / pfslam_search_scan's call, and on top of
// its score volume the weighted mean pose, the 3x3 covariance, the effective number of candidates and the share of the weight on the
// window's border); the specification is in include/pfslam.h.  Included by pfslam_hip.hip behind pfslam_search_scan.hip.inc (same
// translation unit): the volume comes from k_search_ends, k_search_field / the scan splat, k_search_score and k_search_result as they
// are, the sums from pfslam_estimate's device functions (est_moments, est_means, est_centred, est_finish, wave_sum_canonical) as they
// are.  What is new is how a tile of 4096 candidates gets into LDS: a score becomes a weight (pf::exp2m), an index becomes a pose.
// Behind the kernels stands search_volume, the one volume runner of pfslam_search, pfslam_search_scan and this file's two entry points.
// tests/test_search_cov_kernel_text.py cuts the text between the two SEARCH-COV-KERNEL-TEXT marks out and runs it on the CPU.

// SEARCH-COV-KERNEL-TEXT-BEGIN
#define PF_COV_OUT 16 /* the floats of cov_out */

// A step of n candidates through k = (a * ny + j) * nx + i as three digits: n = (da * ny + dj) * nx + di, di < nx, dj < ny (the host).
struct CovStep { int di, dj, da; };
// pfslam_cov_opts and what the host derives from them, by value
struct CovParams {
    float hs;     // the scale of the specification
    int cand;     // candidates of the call, <= 2^24
    CovStep wg;   // PF_EST_WAVES * 64 candidates: a thread's stride while it stages a tile
    CovStep wave; // 64 candidates: a lane's stride in a canonical sum
};
struct CovIdx { int a, j, i; };
__device__ __forceinline__ CovIdx cov_idx(int k, int nx, int ny) // (the two divisions a thread makes)
{
    const int row = nx * ny, a = k / row, c = k - a * row, j = c / nx;
    return CovIdx{a, j, c - j * nx};
}
__device__ __forceinline__ void cov_step(CovIdx &c, const CovStep &s, int nx, int ny) // i + di < 2 nx and j + dj + 1 < 2 ny: one carry each
{
    c.i += s.di;
    int carry = c.i >= nx ? 1 : 0;
    c.i -= carry ? nx : 0;
    c.j += s.dj + carry;
    carry = c.j >= ny ? 1 : 0;
    c.j -= carry ? ny : 0;
    c.a += s.da + carry;
}
// e_k: on the first or last index of a dimension that has more than one candidate
__device__ __forceinline__ bool cov_edge(const CovIdx &c, int nx, int ny, int na)
{
    return (nx > 1 && (c.i == 0 || c.i == nx - 1)) || (ny > 1 && (c.j == 0 || c.j == ny - 1)) || (na > 1 && (c.a == 0 || c.a == na - 1));
}

// The tile [k0, k0 + cnt) as est_moments / est_centred read it: s[0] the weights, s[1 .. 3] x, y, theta.  One coalesced load per
// candidate; the weight is recomputed in every pass (the same function of the same bits), the pose comes from the index.
__device__ __forceinline__ void cov_stage(float (*s)[PF_SUM_TILE], const int *__restrict__ scores, const SearchParams &p, const CovParams &q,
                                          int smin, int k0, int cnt)
{
    const int nx = 2 * p.hx + 1, ny = 2 * p.hy + 1;
    CovIdx c = cov_idx(k0 + threadIdx.x, nx, ny);
    for (int i = threadIdx.x; i < cnt; i += PF_EST_WAVES * 64) {
        const int S = scores[k0 + i];
        s[0][i] = S == PF_SEARCH_NONE ? 0.0f : pf::exp2m((float)(S - smin) * q.hs); // (a heading that takes no part)
        s[1][i] = p.cx + (float)((c.i - p.hx) * p.stride) * p.res;
        s[2][i] = p.cy + (float)((c.j - p.hy) * p.stride) * p.res;
        s[3][i] = p.ct + (float)(c.a - p.ht) * p.step_theta;
        cov_step(c, q.wg, nx, ny);
    }
}
// the sixth wave, idle in est_moments: the canonical sum of the border's weights -> edge[t]
__device__ __forceinline__ void cov_border(const float (*s)[PF_SUM_TILE], int cnt, const SearchParams &p, const CovParams &q, int k0,
                                           float *edge, int t)
{
    if ((threadIdx.x >> 6) != 5) return;
    const int nx = 2 * p.hx + 1, ny = 2 * p.hy + 1, na = 2 * p.ht + 1;
    CovIdx c = cov_idx(k0 + (threadIdx.x & 63), nx, ny);
    const float v = wave_sum_canonical(cnt, [&](int i) {
        const float w = cov_edge(c, nx, ny, na) ? s[0][i] : 0.0f;
        cov_step(c, q.wave, nx, ny);
        return w;
    });
    if ((threadIdx.x & 63) == 0) edge[t] = v;
}
// cov_out from the tile sums (first wave of the workgroup): est_finish's 13 floats, the border share and hs.  `none`: status 2.
__device__ __forceinline__ void cov_finish(const float *part, int nt, const CovParams &q, bool none, float *out)
{
    if (threadIdx.x >= 64) return;
    if (none) {
        if (threadIdx.x == 0) {
            for (int k = 0; k < PF_COV_OUT; k++) out[k] = 0.0f;
            out[12] = (float)q.cand;
            out[14] = q.hs;
        }
        return;
    }
    est_finish(part, nt, q.cand, out);
    const float s0 = wave_sum_canonical(nt, [&](int i) { return part[i]; });
    const float e = wave_sum_canonical(nt, [&](int i) { return part[11 * nt + i]; });
    if (threadIdx.x == 0) {
        out[13] = pf::fdiv(e, s0);
        out[14] = q.hs;
    }
}

// part[q * nt + t]: q = 0 .. 10 as in pfslam_estimate, 11 the border's weights.  One workgroup per tile; 64 KB of LDS: two per CU.
__global__ __launch_bounds__(PF_EST_WAVES * 64) void k_cov_moments(const int *__restrict__ scores, const unsigned long long *__restrict__ key,
                                                                   SearchParams p, CovParams q, float *__restrict__ part, int nt)
{
    __shared__ float s[4][PF_SUM_TILE];
    const unsigned long long kk = *key;
    if (kk == ~0ull) return; // no heading takes part: k_cov_final writes the zeros
    const int t = blockIdx.x, cnt = min(PF_SUM_TILE, q.cand - t * PF_SUM_TILE);
    cov_stage(s, scores, p, q, (int)(kk >> 32), t * PF_SUM_TILE, cnt);
    __syncthreads();
    est_moments(s, cnt, part, nt, t);
    cov_border(s, cnt, p, q, t * PF_SUM_TILE, part + (size_t)11 * nt, t);
}
// the moments are complete (stream order): `mom` = part[0 .. 5 nt) is read-only here, `cen` = part + 5 nt is written
__global__ __launch_bounds__(PF_EST_WAVES * 64) void k_cov_centred(const int *__restrict__ scores, const unsigned long long *__restrict__ key,
                                                                   SearchParams p, CovParams q, const float *__restrict__ mom,
                                                                   float *__restrict__ cen, int nt)
{
    __shared__ float s[4][PF_SUM_TILE];
    const unsigned long long kk = *key;
    if (kk == ~0ull) return;
    const int t = blockIdx.x, cnt = min(PF_SUM_TILE, q.cand - t * PF_SUM_TILE);
    cov_stage(s, scores, p, q, (int)(kk >> 32), t * PF_SUM_TILE, cnt);
    float s0, m[3];
    est_means(mom, nt, &s0, m);
    __syncthreads();
    est_centred(s, cnt, m, cen, nt, t);
}
__global__ __launch_bounds__(64) void k_cov_final(const float *__restrict__ part, const unsigned long long *__restrict__ key, CovParams q,
                                                  int nt, float *__restrict__ out)
{
    cov_finish(part, nt, q, *key == ~0ull, out);
}
// up to one tile: the three passes as one workgroup, the tile sums crossing from wave to wave through `part` as in k_estimate_small
__global__ __launch_bounds__(PF_EST_WAVES * 64) void k_cov_small(const int *__restrict__ scores, const unsigned long long *__restrict__ key,
                                                                 SearchParams p, CovParams q, float *part, float *out)
{
    __shared__ float s[4][PF_SUM_TILE];
    const unsigned long long kk = *key;
    const bool none = kk == ~0ull; // (the whole workgroup)
    if (!none) {
        cov_stage(s, scores, p, q, (int)(kk >> 32), 0, q.cand);
        __syncthreads();
        est_moments(s, q.cand, part, 1, 0);
        cov_border(s, q.cand, p, q, 0, part + 11, 0);
        __syncthreads();
        float s0, m[3];
        est_means(part, 1, &s0, m);
        est_centred(s, q.cand, m, part + 5, 1, 0);
        __syncthreads();
    }
    cov_finish(part, 1, q, none, out);
}
// SEARCH-COV-KERNEL-TEXT-END

extern "C" void pfslam_search_cov_default_opts(pfslam_cov_opts *o)
{
    if (!o) return;
    o->sigma = 0.2f;
    o->reserved_[0] = o->reserved_[1] = o->reserved_[2] = 0;
}

static CovStep cov_step_of(long long n, long long nx, long long ny)
{
    const long long t = n / nx;
    return CovStep{(int)(n % nx), (int)(t % ny), (int)(t / ny)};
}

// The family's one volume runner (declared in pfslam_search.hip.inc): search_plan, then end points, field (the map's tree, or under
// PF_FORM_NO_MAP the points of ref_scan_host), scores and result into the srch_* buffers, with `cov` the reduction, one copy, one wait, and
// the caller's arrays only on success.  The state row srch_state serves all four entry points: key, the four box words, then one row of
// floats -- the result row, the point count (scan forms), three spare words, cov_out.  Every call memsets it, runs on the handle's stream
// and waits before it returns, so no call reads what another left.
#define PF_SEARCH_ROW (PF_SEARCH_OUT + 4 + PF_COV_OUT)
static int search_volume(pfslam_handle *h, const char *fn, int form, const float *ref_scan_host, const float ref_pose[3], const float *scan_host, const float centre[3],
                         const pfslam_search_opts *opts, const pfslam_cov_opts *cov, float pose_out[3], float info[8], float cov_out[16], int32_t *scores)
{
    const std::string name = std::string(fn) + ": ";
    const bool scan_form = (form & PF_FORM_NO_MAP) != 0;
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const float *rp = scan_form ? (ref_pose ? ref_pose : zero) : nullptr;
    SearchPlan s;
    CHK(search_plan(h, fn, form, rp, centre, opts, &s));
    const SearchParams &p = s.p;
    const size_t cand = s.cand;
    CovParams q;
    int nt = 0;
    if (cov) { // behind the search's own checks, before any launch: the options of the covariance
        if (!std::isfinite(cov->sigma) || !(cov->sigma > 0.0f)) return fail(name + "sigma must be finite and > 0");
        if (cov->reserved_[0] || cov->reserved_[1] || cov->reserved_[2]) return fail(name + "the reserved_ of pfslam_cov_opts must be 0");
        q.hs = pf::fdiv(p.u * 1.442695f, (2.0f * cov->sigma) * cov->sigma);
        if (!std::isfinite(q.hs) || !(q.hs > 0.0f)) {
            char msg[200];
            snprintf(msg, sizeof(msg), "%s: sigma %g gives the scale hs = %g; it must be finite and > 0", fn, (double)cov->sigma, (double)q.hs);
            return fail(msg);
        }
        q.cand = (int)cand;
        q.wg = cov_step_of(PF_EST_WAVES * 64, s.nx, s.ny);
        q.wave = cov_step_of(64, s.nx, s.ny);
        nt = (int)((cand + PF_SUM_TILE - 1) / PF_SUM_TILE); // <= 4096: the tile sums fit one tile
    }
    // the feature's own device buffers; they grow when a call needs more.  The volume is built when the caller asks for it, and always
    // for the reduction; the scans and the points are the scan forms', the tile sums the reduction's
    const bool volume = scores || cov;
    CHK(search_grow(&h->srch_field, &h->srch_field_cap, (size_t)p.cap + 2)); // (+ the two spare cells)
    CHK(search_grow(&h->srch_ends, &h->srch_ends_cap, (size_t)s.na * h->nb));
    CHK(search_grow(&h->srch_nin, &h->srch_nin_cap, (size_t)s.na));
    if (volume) CHK(search_grow(&h->srch_scores, &h->srch_scores_cap, cand));
    if (cov) CHK(search_grow(&h->cov_part, &h->cov_part_cap, (size_t)12 * nt));
    if (scan_form && !h->scan_in) CHK(dalloc(&h->scan_in, (size_t)2 * h->nb));
    if (scan_form && !h->scan_pts) CHK(dalloc(&h->scan_pts, (size_t)h->nb));
    if (!h->srch_state) CHK(dalloc(&h->srch_state, (size_t)3 + PF_SEARCH_ROW / 2));
    unsigned long long *key = h->srch_state;
    int *box = (int *)(h->srch_state + 1);
    float *out = (float *)(h->srch_state + 3);
    int *count = (int *)(out + PF_SEARCH_OUT);
    float *dcov = out + PF_SEARCH_OUT + 4;
    int *vol = volume ? h->srch_scores : nullptr;
    HIPCHK(hipMemsetAsync(h->srch_state, 0xff, 24, h->stream));
    const float *scan = h->scan;
    if (scan_form) { // the reference scan's points, before the end points as ever
        HIPCHK(hipMemsetAsync(count, 0, 4, h->stream));
        // (the callers' arrays are pageable: they are consumed before the call returns, behind its one wait)
        HIPCHK(hipMemcpyAsync(h->scan_in, ref_scan_host, (size_t)h->nb * 4, hipMemcpyHostToDevice, h->stream));
        if (scan_host) {
            HIPCHK(hipMemcpyAsync(h->scan_in + h->nb, scan_host, (size_t)h->nb * 4, hipMemcpyHostToDevice, h->stream));
            scan = h->scan_in + h->nb;
        }
        hipLaunchKernelGGL(k_scan_points, dim3((unsigned)((h->nb + 255) / 256)), dim3(256), 0, h->stream, (const float *)h->scan_in, rp[0], rp[1], rp[2],
                           h->nb, h->trig, h->scan_pts, count);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_search_ends, dim3((unsigned)s.na), dim3(256), 0, h->stream, scan, p, h->trig, h->srch_ends, h->srch_nin, box);
    HIPCHK(hipGetLastError());
    if (scan_form) {
        CHK(scan_field_from_points(h, h->scan_pts, h->nb, p, opts->max_dist, box, h->srch_field));
    } else {
        hipLaunchKernelGGL(k_search_field, dim3((unsigned)((p.cap + 255) / 256)), dim3(256), 0, h->stream, kd_view(h), p, (const int *)box, h->srch_field);
        HIPCHK(hipGetLastError());
    }
    const int chunks = (int)((s.nx * s.ny + 63) / 64);
    hipLaunchKernelGGL(k_search_score, dim3((unsigned)(s.na * chunks)), dim3(64), 0, h->stream, (const int2 *)h->srch_ends, (const int *)h->srch_nin,
                       (const int *)box, (const uint16_t *)h->srch_field, p, chunks, vol, key);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_search_result, dim3(1), dim3(1), 0, h->stream, (const unsigned long long *)key, (const int *)h->srch_nin, p, out);
    HIPCHK(hipGetLastError());
    if (cov) { // the reduction over the volume: moments, centred moments, the final sums (one workgroup does all three up to one tile)
        const dim3 wg(PF_EST_WAVES * 64);
        float *part = h->cov_part;
        if (nt == 1) {
            hipLaunchKernelGGL(k_cov_small, dim3(1), wg, 0, h->stream, (const int *)vol, (const unsigned long long *)key, p, q, part, dcov);
        } else {
            hipLaunchKernelGGL(k_cov_moments, dim3(nt), wg, 0, h->stream, (const int *)vol, (const unsigned long long *)key, p, q, part, nt);
            hipLaunchKernelGGL(k_cov_centred, dim3(nt), wg, 0, h->stream, (const int *)vol, (const unsigned long long *)key, p, q,
                               (const float *)part, part + (size_t)5 * nt, nt);
            hipLaunchKernelGGL(k_cov_final, dim3(1), dim3(64), 0, h->stream, (const float *)part, (const unsigned long long *)key, q, nt, dcov);
        }
        HIPCHK(hipGetLastError());
    }
    float r[PF_SEARCH_ROW];
    std::vector<int32_t> sc(scores ? cand : 0); // (the caller's array is written only when the whole call has succeeded)
    HIPCHK(hipMemcpyAsync(r, out, sizeof(r), hipMemcpyDeviceToHost, h->stream));
    if (scores) HIPCHK(hipMemcpyAsync(sc.data(), h->srch_scores, cand * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (scan_form) {
        int npts;
        memcpy(&npts, r + PF_SEARCH_OUT, 4);
        r[4 + 7] = (float)npts;
    }
    memcpy(pose_out, r, 12);
    memcpy(info, r + 4, 32);
    if (cov) memcpy(cov_out, r + PF_SEARCH_OUT + 4, PF_COV_OUT * 4);
    if (scores) memcpy(scores, sc.data(), cand * 4);
    return 0;
}

extern "C" int pfslam_search_cov(pfslam_handle *h, const float centre[3], const pfslam_search_opts *opts, const pfslam_cov_opts *cov,
                                 float pose_out[3], float info[8], float cov_out[16], int32_t *scores)
{
    if (!h || !opts || !pose_out || !info || !cov || !cov_out) return fail("pfslam_search_cov: bad argument");
    return search_volume(h, "pfslam_search_cov", 0, nullptr, nullptr, nullptr, centre, opts, cov, pose_out, info, cov_out, scores);
}

extern "C" int pfslam_search_scan_cov(pfslam_handle *h, const float *ref_scan_host, const float ref_pose[3], const float *scan_host,
                                      const float centre[3], const pfslam_search_opts *opts, const pfslam_cov_opts *cov, float pose_out[3],
                                      float info[8], float cov_out[16], int32_t *scores)
{
    if (!h || !opts || !pose_out || !info || !cov || !cov_out) return fail("pfslam_search_scan_cov: bad argument");
    if (!ref_scan_host) return fail("pfslam_search_scan_cov: ref_scan_host must not be NULL");
    return search_volume(h, "pfslam_search_scan_cov", PF_FORM_NO_MAP, ref_scan_host, ref_pose, scan_host, centre, opts, cov, pose_out, info, cov_out, scores);
}
