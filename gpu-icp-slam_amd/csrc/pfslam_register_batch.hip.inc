// pfslam_register_batch.hip.inc -- pfslam_register_batch (m independent runs of pfslam_register's iteration in one launch); the
// specification is in include/pfslam.h.  Included by pfslam_hip.hip behind pfslam_register.hip.inc (same translation unit): it reuses
// RegOpts, pf::kd_nearest_exact, pf::exact_d2, pf::kd_nearest_ref, pf::clean_lidar_scan, wave_sum_canonical, pf::svd3 and pf::asinf_spec
// as they are and restates k_register's iteration with the per-run scratch in LDS.
// tests/test_register_batch_kernel_text.py cuts the text between the two REGISTER-BATCH-KERNEL-TEXT marks out and runs it on the CPU.

#define PF_REGB_MAX_RUNS 4096             /* a full launch of 40 iterations on a 100 000-point map: 0.41 s measured (profiles/register_batch.txt) */
#define PF_REGB_LDS_PER_CU (160 * 1024)   /* gfx950 */

// REGISTER-BATCH-KERNEL-TEXT-BEGIN
#define PF_REGB_OUT 12 /* out row: pose[3], 0, info[8] */

// One workgroup per run (blockIdx.x = row of starts / out), nothing between workgroups: a run that stops early retires its workgroup and
// the next row takes its place.  The iteration is k_register's, phase for phase and operation for operation, with two differences that
// cannot change a bit: the per-beam scratch is eight arrays of nb floats in dynamic LDS (target x y z, valid, node x y z, d2; arrays,
// not float4 records: lane l of a canonical sum reads elements l, l + 64, ... and at a 16-byte stride that is a four-way bank
// conflict), and the eight masked sums and nine entries of A are looped over the NT / 64 waves there are -- every sum is the canonical
// one of a single wave whichever wave computes it.  There is no trace.
// NT: 1024 or 256 threads, chosen by the host from m and the LDS a run needs (pfslam_register_batch below); the result does not
// depend on it.
template <bool PLANAR, int NT>
__global__ __launch_bounds__(NT) void k_register_batch(const float *__restrict__ scan, int nb, const float *__restrict__ starts, pf::KdView tree,
                                                       RegOpts o, int trig, float *__restrict__ out)
{
    HIP_DYNAMIC_SHARED(float, s_beam) // 8 * nb floats
    __shared__ float s_sum[8];        // raw masked sums: target x y z, node x y z, pair count, residual
    __shared__ float s_A[9];
    __shared__ float s_pose[3];
    __shared__ int s_status;          // -1: go on
    constexpr int NW = NT / 64;
    const int wave = threadIdx.x >> 6;
    const int row = blockIdx.x;
    float *s_t = s_beam;                                     // s_t[r * nb + i]: component r of target i
    float *s_v = s_beam + 3 * (size_t)nb;                    // 1 / 0
    float *s_c = s_beam + 4 * (size_t)nb;                    // s_c[j * nb + i]: component j of node i; j == 3: d2
    if (threadIdx.x == 0) {
        s_pose[0] = starts[3 * (size_t)row];
        s_pose[1] = starts[3 * (size_t)row + 1];
        s_pose[2] = starts[3 * (size_t)row + 2];
        s_status = -1;
    }
    __syncthreads();
    const float gate2 = o.max_dist * o.max_dist;
    const int need = o.min_pairs > 1 ? o.min_pairs : 1;
    int it = 0, status = 0;
    float last_pairs = 0.0f, last_e = 0.0f;
    for (; it < o.max_iters; it++) {
        const float x = s_pose[0], y = s_pose[1], th = s_pose[2];
        for (int i = threadIdx.x; i < nb; i += NT) {
            float wx, wy;
            pf::clean_lidar_scan(i, scan[i], th, wx, wy, trig);
            const bool in = fabsf(wx) < PF_LIDAR_RANGE && fabsf(wy) < PF_LIDAR_RANGE;
            const float tx = in ? x + wx : 0.0f, ty = in ? y + wy : 0.0f;
            float cx = 0.0f, cy = 0.0f, cz = 0.0f, cw = 0.0f;
            bool v = true;
            if (o.select == 1 && !in) {
                v = false; // a rejected beam takes no part: no search either
            } else {
                int b;
                if (o.match == 0) b = pf::kd_nearest_ref<PLANAR>(tree, tx, ty, 0.0f);
                else b = pf::kd_nearest_exact(tree, tx, ty, 0.0f, &cw);
                if (b >= 0) {
                    const uint4 nd = tree.hot[b];
                    cx = __uint_as_float(nd.x);
                    cy = __uint_as_float(nd.y);
                    cz = PLANAR ? 0.0f : tree.z[b];
                    cw = pf::exact_d2(cx, cy, cz, tx, ty, 0.0f);
                } else { // a target that is not finite has no nearest node: the fit turns non-finite and the run ends with status 3
                    cx = cy = cz = cw = NAN;
                }
                if (o.select == 1) v = !(o.max_dist > 0.0f) || cw <= gate2;
            }
            s_t[i] = tx;
            s_t[nb + i] = ty;
            s_t[2 * nb + i] = 0.0f;
            s_v[i] = v ? 1.0f : 0.0f;
            s_c[i] = cx;
            s_c[nb + i] = cy;
            s_c[2 * nb + i] = cz;
            s_c[3 * nb + i] = cw;
        }
        __syncthreads();
        for (int k = wave; k < 8; k += NW) {
            const float *src = k < 3 ? s_t + k * nb : s_c + (k == 7 ? 3 : k - 3) * nb;
            const float s = k == 6 ? wave_sum_canonical(nb, [&](int i) { return s_v[i]; })
                                   : wave_sum_canonical(nb, [&](int i) { return s_v[i] != 0.0f ? src[i] : 0.0f; });
            if ((threadIdx.x & 63) == 0) s_sum[k] = s;
        }
        __syncthreads();
        const float nvf = s_sum[6]; // (a count of at most 4096: exact)
        if (o.select == 1 && nvf < (float)need) {
            status = 2;
            last_pairs = nvf;
            break;
        }
        for (int k = wave; k < 9; k += NW) { // A[j * 3 + r] = sum (tar_r - mu) * (cor_j - mu), as icp_solve_block
            const int j = k / 3, r = k % 3;
            const float mt = pf::fdiv(s_sum[r], nvf), mc = pf::fdiv(s_sum[3 + j], nvf);
            const float *tr = s_t + r * nb, *cj = s_c + j * nb;
            const float s = wave_sum_canonical(nb, [&](int i) {
                const float t = tr[i] + (-mt);
                const float c = cj[i] + (-mc);
                return s_v[i] != 0.0f ? t * c : 0.0f;
            });
            if ((threadIdx.x & 63) == 0) s_A[k] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float A[9], mu_t[3], mu_c[3];
            for (int e = 0; e < 9; e++) A[e] = s_A[e];
            for (int k = 0; k < 3; k++) {
                mu_t[k] = pf::fdiv(s_sum[k], nvf);
                mu_c[k] = pf::fdiv(s_sum[3 + k], nvf);
            }
            float U[9], S[9], V[9];
            pf::svd3(A, U, S, V);
            float R[9]; // R = U * V^T with glm's column-major evaluation order, t = mu_c - R mu_t (icp_solve_block)
            for (int j = 0; j < 3; j++)
                for (int i = 0; i < 3; i++)
                    R[j * 3 + i] = U[i * 3 + 0] * V[j * 3 + 0] + U[i * 3 + 1] * V[j * 3 + 1] + U[i * 3 + 2] * V[j * 3 + 2];
            float t[3];
            for (int i = 0; i < 3; i++)
                t[i] = mu_c[i] - (R[0 * 3 + i] * mu_t[0] + R[1 * 3 + i] * mu_t[1] + R[2 * 3 + i] * mu_t[2]);
            const float theta = pf::asinf_spec(R[0 * 3 + 1]);
            const float e = pf::fdiv(s_sum[7], nvf);
            float xn, yn;
            if (o.update == 0) {
                xn = x + t[0];
                yn = y + t[1];
            } else {
                xn = (R[0] * x + R[3] * y) + t[0];
                yn = (R[1] * x + R[4] * y) + t[1];
            }
            const float tn = th + theta;
            if (!(fabsf(xn) < INFINITY && fabsf(yn) < INFINITY && fabsf(tn) < INFINITY)) {
                s_status = 3;
            } else {
                const float dx = xn - x, dy = yn - y, dt = tn - th;
                s_pose[0] = xn; s_pose[1] = yn; s_pose[2] = tn;
                if (fabsf(dx) < o.eps_xy && fabsf(dy) < o.eps_xy && fabsf(dt) < o.eps_theta) s_status = 1;
                s_sum[7] = e; // (read back below by every thread: the residual of the last completed iteration)
            }
        }
        __syncthreads();
        const int stop = s_status;
        if (stop == 3) {
            status = 3;
            break;
        }
        last_pairs = nvf;
        last_e = s_sum[7];
        if (stop == 1) {
            status = 1;
            it++;
            break;
        }
        // (no barrier here: s_sum, s_A and the beam arrays are rewritten by threads that have all passed the barrier above, and read
        //  again only behind the next one)
    }
    if (threadIdx.x == 0) {
        float *r = out + PF_REGB_OUT * (size_t)row;
        r[0] = s_pose[0]; r[1] = s_pose[1]; r[2] = s_pose[2]; r[3] = 0.0f;
        r[4] = (float)status;
        r[5] = (float)it;
        r[6] = last_pairs;
        r[7] = last_e;
        r[8] = r[9] = r[10] = r[11] = 0.0f;
    }
}
// REGISTER-BATCH-KERNEL-TEXT-END

// *best of pfslam_register_batch from info alone (include/pfslam.h)
static int regb_pick_best(const float *info, int m)
{
    auto eligible = [&](int r) {
        const float *f = info + 8 * (size_t)r;
        return (f[0] == 0.0f || f[0] == 1.0f) && f[1] >= 1.0f && std::isfinite(f[3]);
    };
    float P = -1.0f;
    for (int r = 0; r < m; r++)
        if (eligible(r) && info[8 * (size_t)r + 2] > P) P = info[8 * (size_t)r + 2];
    int best = -1;
    for (int r = 0; r < m; r++) {
        if (!eligible(r)) continue;
        const float pairs = info[8 * (size_t)r + 2], e = info[8 * (size_t)r + 3];
        if (!(2.0f * pairs >= P)) continue; // (pair counts are integers of at most 4096: exact)
        if (best < 0 || e < info[8 * (size_t)best + 3] || (e == info[8 * (size_t)best + 3] && pairs > info[8 * (size_t)best + 2])) best = r;
    }
    return best;
}

template <bool PLANAR, int NT>
static int regb_launch(pfslam_handle *h, int m, size_t lds, const RegOpts &o)
{
    // above the 64 KB a kernel may have without asking (set whenever it is needed: the limit belongs to the function, not the handle)
    if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void *)k_register_batch<PLANAR, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_register_batch<PLANAR, NT>), dim3(m), dim3(NT), lds, h->stream, (const float *)h->scan, h->nb, (const float *)h->regb_in,
                       kd_view(h), o, h->trig, h->regb_out);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int pfslam_register_batch(pfslam_handle *h, const float *starts, int m, const pfslam_register_opts *opts, float *poses_out, float *info,
                                     int *best)
{
    if (!h || !starts || !opts || !poses_out || !info) return fail("pfslam_register_batch: bad argument");
    if (m < 1 || m > PF_REGB_MAX_RUNS) return fail("pfslam_register_batch: m must be 1 .. 4096");
    if (opts->max_iters < 1 || opts->max_iters > 64) return fail("pfslam_register_batch: max_iters must be 1 .. 64");
    if (opts->match < 0 || opts->match > 1) return fail("pfslam_register_batch: match must be 0 (the reference's traversal) or 1 (exact nearest neighbour)");
    if (opts->select < 0 || opts->select > 1) return fail("pfslam_register_batch: select must be 0 (every beam) or 1 (in-range beams inside the gate)");
    if (opts->update < 0 || opts->update > 1) return fail("pfslam_register_batch: update must be 0 (the reference's increment) or 1 (rigid)");
    if (!std::isfinite(opts->max_dist)) return fail("pfslam_register_batch: max_dist must be finite (<= 0: no gate)");
    if (!(opts->eps_xy >= 0.0f) || !(opts->eps_theta >= 0.0f) || !std::isfinite(opts->eps_xy) || !std::isfinite(opts->eps_theta))
        return fail("pfslam_register_batch: eps_xy and eps_theta must be finite and >= 0 (0: never stop early)");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    if (h->kd_size <= 0) return fail("pfslam_register_batch: no map loaded");
    if (h->nb > PF_SUM_TILE) return fail("pfslam_register_batch: n_beams > 4096 not supported");
    if (m > h->regb_cap) { // the feature's own device buffers: starts and result rows; they grow when a call needs more
        if (h->regb_in) HIPCHK(hipFree(h->regb_in));
        if (h->regb_out) HIPCHK(hipFree(h->regb_out));
        h->regb_in = h->regb_out = nullptr;
        h->regb_cap = 0;
        CHK(dalloc(&h->regb_in, (size_t)m * 3));
        CHK(dalloc(&h->regb_out, (size_t)m * PF_REGB_OUT));
        h->regb_cap = m;
    }
    const RegOpts o{opts->max_iters, opts->match, opts->select, opts->update, opts->max_dist, opts->eps_xy, opts->eps_theta, opts->min_pairs};
    const size_t lds = (size_t)h->nb * 8 * sizeof(float);
    // Workgroup size (profiles/register_batch.txt): a run that has a compute unit to itself -- no more rows than compute units, or so
    // much LDS that only one workgroup fits -- is fastest with the 1024 threads of k_register; otherwise four 256-thread runs share a
    // compute unit and one run's serial phases (the sums, the SVD) are hidden behind the others' searches.
    if (!h->regb_cus) HIPCHK(hipDeviceGetAttribute(&h->regb_cus, hipDeviceAttributeMultiprocessorCount, h->cfg.device));
    const bool wide = m <= h->regb_cus || 2 * (lds + 256) > PF_REGB_LDS_PER_CU;
    HIPCHK(hipMemcpyAsync(h->regb_in, starts, (size_t)m * 12, hipMemcpyHostToDevice, h->stream));
    if (h->planar) CHK((wide ? regb_launch<true, 1024>(h, m, lds, o) : regb_launch<true, 256>(h, m, lds, o)));
    else CHK((wide ? regb_launch<false, 1024>(h, m, lds, o) : regb_launch<false, 256>(h, m, lds, o)));
    std::vector<float> r((size_t)m * PF_REGB_OUT);
    HIPCHK(hipMemcpyAsync(r.data(), h->regb_out, r.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int k = 0; k < m; k++) {
        memcpy(poses_out + 3 * (size_t)k, r.data() + PF_REGB_OUT * (size_t)k, 12);
        memcpy(info + 8 * (size_t)k, r.data() + PF_REGB_OUT * (size_t)k + 4, 32);
    }
    if (best) *best = regb_pick_best(info, m);
    return 0;
}
