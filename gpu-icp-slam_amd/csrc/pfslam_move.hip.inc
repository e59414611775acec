// pfslam_move.hip.inc -- pfslam_move_particles (the odometry motion model: every particle moves by the increment rotated into its own frame,
// plus correlated Gaussian noise drawn from a 3 x 3 covariance; no reference counterpart).  The specification is in include/pfslam.h.
// Included by pfslam_hip.hip (same translation unit): the entry point shares enqueue_odometry with pfslam_shift_particles.
// tests/test_move_kernel_text.py cuts the text between the two MOVE-KERNEL-TEXT marks out and runs it on the CPU.

// MOVE-KERNEL-TEXT-BEGIN
// The call's constants: the lower Cholesky factor of the noise covariance (host, once per call), the increment and the heading of the
// frame both are expressed in.
struct MoveParams {
    float l00, l10, l11, l20, l21, l22;
    float dx, dy, dt, ref_theta;
};
// One pose through the motion model with the standard normal draws z1, z2, z3 (the robot's pose: all three 0).  Float, one rounding per
// operation, in the order of the header; trig 1 takes the device library's sinf / cosf.
__device__ __forceinline__ void move_pose(float &x, float &y, float &th, float z1, float z2, float z3, const MoveParams &m, int trig)
{
    const float mx = m.dx + m.l00 * z1;
    const float my = m.dy + (m.l10 * z1 + m.l11 * z2);
    const float mt = m.dt + ((m.l20 * z1 + m.l21 * z2) + m.l22 * z3);
    const float phi = th - m.ref_theta;
    float s, c;
    if (trig) {
        s = ::sinf(phi);
        c = ::cosf(phi);
    } else {
        pf::sincosf_spec(phi, s, c);
    }
    x = x + ((c * mx) - (s * my));
    y = y + ((s * mx) + (c * my));
    th = th + mt;
}
// One thread per particle, coalesced SoA, like k_motion: three erfcinv evaluations and one sincos in fp64, no LDS, no atomics.  The draw is
// keyed by the GLOBAL index goff + i at depth 1 (the dispersion's stream is depth 0), so any sharding gives the unsharded bits.  Thread 0
// moves the robot's pose without noise and the cloud statistics of both ticket parities by the pose's increment (performance only), as
// k_shift does.
__global__ __launch_bounds__(256) void k_move(float *__restrict__ x, float *__restrict__ y, float *__restrict__ th, int n, MoveParams m, int frame,
                                              int goff, int trig, float *__restrict__ pose, float *__restrict__ cloud)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        float px = pose[0], py = pose[1], pt = pose[2];
        move_pose(px, py, pt, 0.0f, 0.0f, 0.0f, m, trig);
        const float ix = px - pose[0], iy = py - pose[1], it = pt - pose[2];
        pose[0] = px; pose[1] = py; pose[2] = pt;
        if (cloud)
            for (int k = 0; k < 2; k++) {
                cloud[4 * k] += ix; cloud[4 * k + 1] += iy; cloud[4 * k + 2] += it;
            }
    }
    if (i >= n) return;
    uint32_t e = pf::engine_seed(frame, goff + i, 1);
    const float z1 = pf::normal(e, 0.0f, 1.0f, trig != 0);
    const float z2 = pf::normal(e, 0.0f, 1.0f, trig != 0);
    const float z3 = pf::normal(e, 0.0f, 1.0f, trig != 0);
    float xi = x[i], yi = y[i], ti = th[i];
    move_pose(xi, yi, ti, z1, z2, z3, m, trig);
    x[i] = xi;
    y[i] = yi;
    th[i] = ti;
}
// MOVE-KERNEL-TEXT-END

// The largest |pf::normal(., 0, 1)| the generator can return is the u = 0 draw, p = 2^-32: 6.2303 in the specification's form and in the
// device library's (evaluated on the CPU: tests/test_move_spec.py holds both below this constant).  The next integer:
#define PF_MOVE_Z 7.0f

extern "C" void pfslam_move_default_opts(pfslam_move_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->ref_theta = 0.0f;
    o->cov_scale = 1.0f;
    o->sigma_xy_min = 0.0f;
    o->sigma_theta_min = 0.0f;
}

// The noise factor of the header: a = cov_scale * cov + floors, lower Cholesky in float with a fixed order.  0 = ok, 1 = a pivot that is
// negative or not finite.
static int move_factor(const float c[6], const pfslam_move_opts &o, MoveParams &m)
{
    const float fxy = o.sigma_xy_min * o.sigma_xy_min, ft = o.sigma_theta_min * o.sigma_theta_min;
    const float a00 = o.cov_scale * c[0] + fxy;
    const float a10 = o.cov_scale * c[1];
    const float a20 = o.cov_scale * c[2];
    const float a11 = o.cov_scale * c[3] + fxy;
    const float a21 = o.cov_scale * c[4];
    const float a22 = o.cov_scale * c[5] + ft;
    const auto bad = [](float p) { return !(p >= 0.0f) || std::isinf(p); };
    m.l00 = m.l10 = m.l20 = m.l11 = m.l21 = m.l22 = 0.0f;
    const float p0 = a00;
    if (bad(p0)) return 1;
    if (p0 != 0.0f) { // (a pivot that is exactly 0: its whole column stays 0, no division)
        m.l00 = pf::fsqrt(p0);
        m.l10 = pf::fdiv(a10, m.l00);
        m.l20 = pf::fdiv(a20, m.l00);
    }
    const float p1 = a11 - m.l10 * m.l10;
    if (bad(p1)) return 1;
    if (p1 != 0.0f) {
        m.l11 = pf::fsqrt(p1);
        m.l21 = pf::fdiv(a21 - m.l20 * m.l10, m.l11);
    }
    const float p2 = a22 - (m.l20 * m.l20 + m.l21 * m.l21);
    if (bad(p2)) return 1;
    if (p2 != 0.0f) m.l22 = pf::fsqrt(p2);
    return 0; // (an entry that overflowed over a tiny pivot has made the next pivot -inf or NaN: refused above)
}

extern "C" int pfslam_move_particles(pfslam_handle *h, int frame, const float delta[3], const float cov[6], const pfslam_move_opts *opts)
{
    if (!h || !delta || !opts) return fail("pfslam_move_particles: bad argument");
    const float zero[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const float *c = cov ? cov : zero;
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(delta[k])) return fail("pfslam_move_particles: delta is not finite");
    for (int k = 0; k < 6; k++)
        if (!std::isfinite(c[k])) return fail("pfslam_move_particles: cov is not finite");
    if (!std::isfinite(opts->ref_theta)) return fail("pfslam_move_particles: ref_theta is not finite");
    if (!std::isfinite(opts->cov_scale)) return fail("pfslam_move_particles: cov_scale is not finite");
    if (!std::isfinite(opts->sigma_xy_min) || !std::isfinite(opts->sigma_theta_min)) return fail("pfslam_move_particles: a floor is not finite");
    if (opts->cov_scale < 0.0f) return fail("pfslam_move_particles: cov_scale is negative");
    if (opts->sigma_xy_min < 0.0f || opts->sigma_theta_min < 0.0f) return fail("pfslam_move_particles: a floor is negative");
    for (int k = 0; k < 4; k++)
        if (opts->reserved_[k] != 0) return fail("pfslam_move_particles: reserved_ must be 0");
    MoveParams m;
    if (move_factor(c, *opts, m)) return fail("pfslam_move_particles: covariance is not positive semi-definite");
    m.dx = delta[0]; m.dy = delta[1]; m.dt = delta[2]; m.ref_theta = opts->ref_theta;
    // every heading moves by at most this much: the host's bound decides which scan-match instantiation runs
    const float ad = fabsf(delta[2]) + PF_MOVE_Z * (fabsf(m.l20) + fabsf(m.l21) + fabsf(m.l22));
    return enqueue_odometry(h, ad, [&] {
        hipLaunchKernelGGL(k_move, dim3((h->n + 255) / 256), dim3(256), 0, h->stream, h->x, h->y, h->th, h->n, m, frame, h->goff, h->trig, h->pose,
                           h->cloud_valid ? h->cloud : (float *)nullptr);
    });
}
