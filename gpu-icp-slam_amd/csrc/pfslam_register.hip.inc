// pfslam_register.hip.inc -- pfslam_nearest (exact nearest map node) and pfslam_register (iterated ICP on the device); the specification
// of both is in include/pfslam.h.  Included by pfslam_hip.hip behind pfslam_stages.hip.inc (same translation unit): it reuses
// pf::clean_lidar_scan, pf::kd_nearest_ref, wave_sum_canonical, pf::svd3 and pf::asinf_spec as they are.
// tests/test_register_kernel_text.py cuts the text between the two REGISTER-KERNEL-TEXT marks out and runs it on the CPU.

// REGISTER-KERNEL-TEXT-BEGIN
namespace pf {

// squared distance node - query: ((dx dx + dy dy) + dz dz), one rounding per operation, in this order
__device__ __forceinline__ float exact_d2(float nx, float ny, float nz, float qx, float qy, float qz)
{
    const float dx = nx - qx, dy = ny - qy, dz = nz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// The exact nearest node of the tree: smallest exact_d2, the lowest node index among equal ones; -1 for a query with a non-finite
// coordinate.  Branch and bound without a stack: the walk goes down into the side the query is on, and on the way back up -- through
// the parent links -- into the other side unless its half space is farther than the best node so far.  `from` tells a node how it was
// reached: from its parent (-2: it is visited now), or back from one of its children.  No depth limit: between two re-balances the
// tree only grows at its leaves (KDTree::InsertNode) and can be deep.
//   Pruning: a node n behind the split plane of s has |n_a - q_a| >= |s_a - q_a| on the split axis (left sub-trees hold coordinates
//   <= the split's, right ones >=: KDTree::InsertList sorts, InsertNode sends "query < node" left), float subtraction, squaring and the
//   sums of non-negative terms in exact_d2 are monotone, so exact_d2(n) >= fl((s_a - q_a)^2) =: pd2 AS COMPUTED.  A side is skipped only
//   when pd2 > best; at pd2 == best it is entered, because it may hold an equal distance at a lower index.
//   A z-level node of a PLANAR map keeps its true left child in the z array (kd_device.h); its plane distance to a z = 0 query is 0, so
//   both of its sides are always walked.
// visits (COUNT only): node evaluations, for profiles/register.txt.
template <bool COUNT = false>
__device__ __forceinline__ int kd_nearest_exact(const KdView &t, float qx, float qy, float qz, float *d2_out, unsigned *visits = nullptr)
{
    float best = INFINITY;
    int bi = -1;
    if (!(fabsf(qx) < INFINITY && fabsf(qy) < INFINITY && fabsf(qz) < INFINITY)) { // (NaN too)
        *d2_out = best;
        return bi;
    }
    int cur = 0, from = -2;
    for (;;) {
        const uint4 nd = t.hot[cur];
        const uint32_t axis = nd.z >> 30;
        const float nx = __uint_as_float(nd.x), ny = __uint_as_float(nd.y);
        float nz = 0.0f;
        int left = hot_left(nd.z);
        if (!t.planar) nz = t.z[cur];
        else if (axis == 2) left = __float_as_int(t.z[cur]); // the hot record of a planar z level holds its right child twice
        const int right = (int)nd.w;
        const float qa = axis == 0 ? qx : (axis == 1 ? qy : qz), na = axis == 0 ? nx : (axis == 1 ? ny : nz);
        const bool lt = qa < na;
        const int near = lt ? left : right, far = lt ? right : left;
        if (from == -2) {
            if (COUNT) (*visits)++;
            const float d2 = exact_d2(nx, ny, nz, qx, qy, qz);
            if (d2 < best || (d2 == best && (bi < 0 || cur < bi))) {
                best = d2;
                bi = cur;
            }
            if (near >= 0) {
                cur = near;
                continue;
            }
        }
        if ((from == -2 || from == near) && far >= 0) { // the near side is done (or empty): the far side, unless the plane rules it out
            const float pd = na - qa;
            if (pd * pd <= best) {
                cur = far;
                from = -2;
                continue;
            }
        }
        const int p = t.parent[cur];
        if (p < 0) break;
        from = cur;
        cur = p;
    }
    *d2_out = best;
    return bi;
}

} // namespace pf

__global__ __launch_bounds__(256) void k_nearest(const float *__restrict__ xyz, int n, pf::KdView tree, int *__restrict__ best,
                                                 float *__restrict__ d2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float d;
    best[i] = pf::kd_nearest_exact(tree, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &d);
    d2[i] = d;
}

// pfslam_register_opts by value (the header's struct, field for field)
struct RegOpts {
    int max_iters, match, select, update;
    float max_dist, eps_xy, eps_theta;
    int min_pairs;
};
#define PF_REG_OUT_HEAD 12 /* out: pose[4], info[8], then the trace rows */

// pfslam_register: every iteration in ONE persistent 1024-thread workgroup -- no host wait, no second launch, nothing between
// workgroups.  Per iteration: (1) targets and correspondences, beams strided over the threads, into the feature's own scratch
// tar / cor (float4 per beam: target x, y, 0, valid; node x, y, z, d2); (2) a wave per masked sum (six components, the pair count,
// the residual); (3) a wave per entry of A; (4) thread 0: SVD, update, stopping test, trace row.  The scratch crosses from phase to
// phase through global memory with a barrier in between (not __restrict__: the loads must not be taken for loads of kernel-invariant
// memory).  use_start == 0: the start is the handle's pose, read here.
template <bool PLANAR>
__global__ __launch_bounds__(1024) void k_register(const float *__restrict__ scan, int nb, const float *__restrict__ pose, float sx, float sy,
                                                   float st, int use_start, pf::KdView tree, RegOpts o, int trig, float4 *tar, float4 *cor,
                                                   float *out)
{
    __shared__ float s_sum[8]; // raw masked sums: target x y z, node x y z, pair count, residual
    __shared__ float s_A[9];
    __shared__ float s_pose[3];
    __shared__ int s_status;   // -1: go on
    const int wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        s_pose[0] = use_start ? sx : pose[0];
        s_pose[1] = use_start ? sy : pose[1];
        s_pose[2] = use_start ? st : pose[2];
        s_status = -1;
    }
    __syncthreads();
    const float gate2 = o.max_dist * o.max_dist;
    const int need = o.min_pairs > 1 ? o.min_pairs : 1;
    const float *tf = (const float *)tar, *cf = (const float *)cor;
    int it = 0, status = 0;
    float last_pairs = 0.0f, last_e = 0.0f;
    for (; it < o.max_iters; it++) {
        const float x = s_pose[0], y = s_pose[1], th = s_pose[2];
        for (int i = threadIdx.x; i < nb; i += 1024) {
            float wx, wy;
            pf::clean_lidar_scan(i, scan[i], th, wx, wy, trig);
            const bool in = fabsf(wx) < PF_LIDAR_RANGE && fabsf(wy) < PF_LIDAR_RANGE;
            const float tx = in ? x + wx : 0.0f, ty = in ? y + wy : 0.0f;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            bool v = true;
            if (o.select == 1 && !in) {
                v = false; // a rejected beam takes no part: no search either
            } else {
                int b;
                if (o.match == 0) b = pf::kd_nearest_ref<PLANAR>(tree, tx, ty, 0.0f);
                else b = pf::kd_nearest_exact(tree, tx, ty, 0.0f, &c.w);
                if (b >= 0) {
                    const uint4 nd = tree.hot[b];
                    c.x = __uint_as_float(nd.x);
                    c.y = __uint_as_float(nd.y);
                    c.z = PLANAR ? 0.0f : tree.z[b];
                    c.w = pf::exact_d2(c.x, c.y, c.z, tx, ty, 0.0f);
                } else { // a target that is not finite has no nearest node: the fit turns non-finite and the run ends with status 3
                    c = make_float4(NAN, NAN, NAN, NAN);
                }
                if (o.select == 1) v = !(o.max_dist > 0.0f) || c.w <= gate2;
            }
            tar[i] = make_float4(tx, ty, 0.0f, v ? 1.0f : 0.0f);
            cor[i] = c;
        }
        __syncthreads();
        if (wave < 8) {
            const float *src = wave < 3 ? tf + wave : cf + (wave == 7 ? 3 : wave - 3);
            const float s = wave == 6 ? wave_sum_canonical(nb, [&](int i) { return tf[4 * i + 3]; })
                                      : wave_sum_canonical(nb, [&](int i) { return tf[4 * i + 3] != 0.0f ? src[4 * i] : 0.0f; });
            if ((threadIdx.x & 63) == 0) s_sum[wave] = s;
        }
        __syncthreads();
        const float nvf = s_sum[6]; // (a count of at most 4096: exact)
        if (o.select == 1 && nvf < (float)need) {
            status = 2;
            last_pairs = nvf;
            break;
        }
        if (wave < 9) { // A[j * 3 + r] = sum (tar_r - mu) * (cor_j - mu), as icp_solve_block
            const int j = wave / 3, r = wave % 3;
            const float mt = pf::fdiv(s_sum[r], nvf), mc = pf::fdiv(s_sum[3 + j], nvf);
            const float s = wave_sum_canonical(nb, [&](int i) {
                const float t = tf[4 * i + r] + (-mt);
                const float c = cf[4 * i + j] + (-mc);
                return tf[4 * i + 3] != 0.0f ? t * c : 0.0f;
            });
            if ((threadIdx.x & 63) == 0) s_A[wave] = s;
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
                float *row = out + PF_REG_OUT_HEAD + 8 * it;
                row[0] = xn; row[1] = yn; row[2] = tn;
                row[3] = dx; row[4] = dy; row[5] = dt;
                row[6] = nvf; row[7] = e;
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
        // (no barrier here: s_sum and s_A are rewritten only behind the next iteration's first barrier)
    }
    if (threadIdx.x == 0) {
        out[0] = s_pose[0]; out[1] = s_pose[1]; out[2] = s_pose[2]; out[3] = 0.0f;
        out[4] = (float)status;
        out[5] = (float)it;
        out[6] = last_pairs;
        out[7] = last_e;
        out[8] = out[9] = out[10] = out[11] = 0.0f;
    }
}
// REGISTER-KERNEL-TEXT-END

extern "C" void pfslam_register_default_opts(pfslam_register_opts *o)
{
    if (!o) return;
    o->max_iters = 40;
    o->match = 1;
    o->select = 1;
    o->update = 1;
    o->max_dist = 0.5f;
    o->eps_xy = 1e-4f;
    o->eps_theta = 1e-5f;
    o->min_pairs = 3;
}

extern "C" int pfslam_nearest(pfslam_handle *h, const float *xyz_host, int n, int32_t *best_host, float *d2_host)
{
    if (!h || !xyz_host || !best_host || n < 0) return fail("pfslam_nearest: bad argument");
    if (h->kd_size <= 0) return fail("pfslam_nearest: no map loaded");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    float *d_xyz = nullptr, *d_d2 = nullptr;
    int *d_best = nullptr;
    CHK(dalloc(&d_xyz, (size_t)n * 3));
    CHK(dalloc(&d_best, (size_t)n));
    CHK(dalloc(&d_d2, (size_t)n));
    HIPCHK(hipMemcpyAsync(d_xyz, xyz_host, (size_t)n * 12, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_nearest, dim3((n + 255) / 256), dim3(256), 0, h->stream, (const float *)d_xyz, n, kd_view(h), d_best, d_d2);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(best_host, d_best, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    if (d2_host) HIPCHK(hipMemcpyAsync(d2_host, d_d2, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipFree(d_xyz));
    HIPCHK(hipFree(d_best));
    HIPCHK(hipFree(d_d2));
    return 0;
}

extern "C" int pfslam_register(pfslam_handle *h, const float start[3], const pfslam_register_opts *opts, float pose_out[3], float info[8],
                               float *trace)
{
    if (!h || !opts || !pose_out || !info) return fail("pfslam_register: bad argument");
    if (opts->max_iters < 1 || opts->max_iters > 64) return fail("pfslam_register: max_iters must be 1 .. 64");
    if (opts->match < 0 || opts->match > 1) return fail("pfslam_register: match must be 0 (the reference's traversal) or 1 (exact nearest neighbour)");
    if (opts->select < 0 || opts->select > 1) return fail("pfslam_register: select must be 0 (every beam) or 1 (in-range beams inside the gate)");
    if (opts->update < 0 || opts->update > 1) return fail("pfslam_register: update must be 0 (the reference's increment) or 1 (rigid)");
    if (!std::isfinite(opts->max_dist)) return fail("pfslam_register: max_dist must be finite (<= 0: no gate)");
    if (!(opts->eps_xy >= 0.0f) || !(opts->eps_theta >= 0.0f) || !std::isfinite(opts->eps_xy) || !std::isfinite(opts->eps_theta))
        return fail("pfslam_register: eps_xy and eps_theta must be finite and >= 0 (0: never stop early)");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    if (h->kd_size <= 0) return fail("pfslam_register: no map loaded");
    if (h->nb > PF_SUM_TILE) return fail("pfslam_register: n_beams > 4096 not supported");
    if (!h->reg_tar) { // the feature's own scratch, on first use: targets, correspondences, pose + info + trace
        CHK(dalloc(&h->reg_tar, (size_t)h->nb * 4));
        CHK(dalloc(&h->reg_cor, (size_t)h->nb * 4));
        CHK(dalloc(&h->reg_out, (size_t)PF_REG_OUT_HEAD + 64 * 8));
    }
    const RegOpts o{opts->max_iters, opts->match, opts->select, opts->update, opts->max_dist, opts->eps_xy, opts->eps_theta, opts->min_pairs};
    const float sx = start ? start[0] : 0.0f, sy = start ? start[1] : 0.0f, st = start ? start[2] : 0.0f;
    if (h->planar)
        hipLaunchKernelGGL(k_register<true>, dim3(1), dim3(1024), 0, h->stream, (const float *)h->scan, h->nb, (const float *)h->pose, sx, sy, st,
                           start ? 1 : 0, kd_view(h), o, h->trig, (float4 *)h->reg_tar, (float4 *)h->reg_cor, h->reg_out);
    else
        hipLaunchKernelGGL(k_register<false>, dim3(1), dim3(1024), 0, h->stream, (const float *)h->scan, h->nb, (const float *)h->pose, sx, sy, st,
                           start ? 1 : 0, kd_view(h), o, h->trig, (float4 *)h->reg_tar, (float4 *)h->reg_cor, h->reg_out);
    HIPCHK(hipGetLastError());
    float r[PF_REG_OUT_HEAD + 64 * 8];
    HIPCHK(hipMemcpyAsync(r, h->reg_out, sizeof(float) * (PF_REG_OUT_HEAD + 8 * (size_t)opts->max_iters), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(pose_out, r, 12);
    memcpy(info, r + 4, 32);
    const int done = (int)r[5];
    if (trace && done > 0) memcpy(trace, r + PF_REG_OUT_HEAD, sizeof(float) * 8 * (size_t)done);
    return 0;
}
