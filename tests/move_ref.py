"""pfslam_move_particles restated from the CPU oracle's primitives.

TEST INFRASTRUCTURE (helper module, not a test).  The CPU oracle is frozen and has no motion model; this restates the specification of
include/pfslam.h with numpy float32 element-wise operations (one rounding each, in the order written; numpy's float32 sqrt and divide are
correctly rounded) and takes the generator and the trigonometry from the oracle: orc_engine_seed, orc_normal, orc_sincosf.

    a   = cov_scale * cov + floors,  L = its lower Cholesky factor (a zero pivot: a zero column)
    e   = engine_seed(frame, g, 1);  z1, z2, z3 = normal(e, 0, 1)
    m   = delta + L z                (mx, my, mt; the sums in the header's order)
    phi = theta - ref_theta;  x' = x + (c mx - s my),  y' = y + (s mx + c my),  theta' = theta + mt

tests/test_move_spec.py holds it against the header's claims; tests/test_move_kernel_text.py and tests/test_gpu_move.py hold the kernel to
it bit for bit."""
import ctypes as C

import numpy as np

import oracle_lib as O

F = np.float32
MINSTD_M = 2147483647
# the state whose next minstd output is 1, i.e. u = 0: the generator's most extreme normal draw
STATE_U0 = pow(48271, -1, MINSTD_M)
# a full covariance of corridor shape (include/pfslam.h: 0.106 m along, 0.003 m across, 0.00037 rad), every pair correlated
SD = (0.106, 0.003, 0.00037)
CORRIDOR_COV = np.array([SD[0] * SD[0], 0.3 * SD[0] * SD[1], -0.2 * SD[0] * SD[2], SD[1] * SD[1], 0.4 * SD[1] * SD[2], SD[2] * SD[2]], F)
STAT_N, STAT_FRAME, STAT_DELTA = 65536, 7, np.array([0.5, -0.03, 0.02], F)


class NotPsd(ValueError):
    pass


def factor(cov=None, cov_scale=1.0, sigma_xy_min=0.0, sigma_theta_min=0.0):
    """(L, a): L = (L00, L10, L11, L20, L21, L22) and a = (a00, a10, a20, a11, a21, a22) as float32; NotPsd for a bad pivot."""
    c = np.zeros(6, F) if cov is None else np.ascontiguousarray(cov, F).reshape(6)
    s, fxy, ft = F(cov_scale), F(sigma_xy_min) * F(sigma_xy_min), F(sigma_theta_min) * F(sigma_theta_min)
    with np.errstate(all="ignore"):
        a00, a10, a20 = F(s * c[0]) + fxy, F(s * c[1]), F(s * c[2])
        a11, a21, a22 = F(s * c[3]) + fxy, F(s * c[4]), F(s * c[5]) + ft
        bad = lambda p: not (p >= 0) or np.isinf(p)
        l00 = l10 = l20 = l11 = l21 = l22 = F(0)
        p0 = a00
        if bad(p0):
            raise NotPsd("covariance is not positive semi-definite")
        if p0 != 0:
            l00 = np.sqrt(p0)
            l10, l20 = F(a10 / l00), F(a20 / l00)
        p1 = F(a11 - F(l10 * l10))
        if bad(p1):
            raise NotPsd("covariance is not positive semi-definite")
        if p1 != 0:
            l11 = np.sqrt(p1)
            l21 = F(F(a21 - F(l20 * l10)) / l11)
        p2 = F(a22 - F(F(l20 * l20) + F(l21 * l21)))
        if bad(p2):
            raise NotPsd("covariance is not positive semi-definite")
        if p2 != 0:
            l22 = np.sqrt(p2)
    return np.array([l00, l10, l11, l20, l21, l22], F), np.array([a00, a10, a20, a11, a21, a22], F)


def draws(frame, g):
    """z[len(g), 3]: the three successive normal(e, 0, 1) of engine_seed(frame, g, 1) for every global index in g."""
    L = O.lib()
    z = np.empty((len(g), 3), F)
    st = C.c_uint32()
    for r, gi in enumerate(g):
        st.value = L.orc_engine_seed(int(frame), int(gi), 1)
        z[r, 0] = L.orc_normal(C.byref(st), 0.0, 1.0)
        z[r, 1] = L.orc_normal(C.byref(st), 0.0, 1.0)
        z[r, 2] = L.orc_normal(C.byref(st), 0.0, 1.0)
    return z


def z_max():
    """|normal(., 0, 1)| of the u = 0 draw: the largest the generator can return."""
    st = C.c_uint32(STATE_U0)
    return abs(float(O.lib().orc_normal(C.byref(st), 0.0, 1.0)))


def increments(z, delta, L):
    """(mx, my, mt) of every row of z."""
    d = np.ascontiguousarray(delta, F)
    z1, z2, z3 = z[:, 0], z[:, 1], z[:, 2]
    mx = d[0] + L[0] * z1
    my = d[1] + (L[1] * z1 + L[2] * z2)
    mt = d[2] + ((L[3] * z1 + L[4] * z2) + L[5] * z3)
    return mx, my, mt


def apply(x, y, th, mx, my, mt, ref_theta):
    x, y, th = (np.ascontiguousarray(v, F) for v in (x, y, th))
    s, c = O.sincosf(th - F(ref_theta))
    return x + ((c * mx) - (s * my)), y + ((s * mx) + (c * my)), th + mt


def move(x, y, th, frame, delta, cov=None, ref_theta=0.0, cov_scale=1.0, sigma_xy_min=0.0, sigma_theta_min=0.0, goff=0):
    """The particles after pfslam_move_particles: (x', y', theta') as float32 arrays."""
    L, _ = factor(cov, cov_scale, sigma_xy_min, sigma_theta_min)
    z = draws(frame, goff + np.arange(len(x)))
    return apply(x, y, th, *increments(z, delta, L), ref_theta)


def move_pose(pose, delta, cov=None, ref_theta=0.0, cov_scale=1.0, sigma_xy_min=0.0, sigma_theta_min=0.0):
    """The robot's pose after the call: the same formulas with z = 0."""
    L, _ = factor(cov, cov_scale, sigma_xy_min, sigma_theta_min)
    p = np.ascontiguousarray(pose, F).reshape(1, 3)
    x, y, t = apply(p[:, 0], p[:, 1], p[:, 2], *increments(np.zeros((1, 3), F), delta, L), ref_theta)
    return np.array([x[0], y[0], t[0]], F)


def move_oracle(o, frame, delta, cov=None, **opts):
    """pfslam_move_particles on a whole-step oracle (oracle_lib.Slam): its particles and pose go through move / move_pose and back through
    the oracle's pose hook, which writes both particle copies and robotPos and no weight."""
    p = o.particles()
    x, y, th = move(p["x"], p["y"], p["theta"], frame, delta, cov, **opts)
    o.replace_poses(x, y, th, move_pose(o.pose, delta, cov, **opts))


def theta_growth(delta, L, z=7.0):
    """What the host's heading bound grows by."""
    return F(abs(F(delta[2]))) + F(z) * F(F(abs(L[3]) + abs(L[4])) + abs(L[5]))


def cloud(n, ref_theta=0.0, spread=0.2, seed=0, lo=8.0, hi=16.0):
    """n poses with positions in [lo, hi) and headings ref_theta +- spread, and weights in (0, 1)."""
    rng = np.random.RandomState(7919 * seed + n)
    x = rng.uniform(lo, hi, n).astype(F)
    y = rng.uniform(lo, hi, n).astype(F)
    th = (ref_theta + rng.uniform(-spread, spread, n)).astype(F)
    w = rng.uniform(0.1, 1.0, n).astype(F)
    return x, y, th, w


def particles_of(x, y, th, w):
    p = np.zeros(len(x), O.PARTICLE_DTYPE)
    p["x"], p["y"], p["theta"], p["w"] = x, y, th, w
    return p


# ---- the stage's inputs at their edges: one set for the GPU (tests/test_gpu_move.py) and for the kernel text on the CPU
# (tests/test_move_kernel_text.py), so that a disagreement on the device is split between arithmetic and indexing
EDGE_N, EDGE_FRAME, EDGE_REF = 257, 9, 0.7
EDGE_DELTA = np.array([0.31, -0.07, 0.045], F)
EDGE_OPTS = dict(cov_scale=1.5, sigma_xy_min=0.007, sigma_theta_min=0.0036)
EDGE_POSE = np.array([11.5, 9.25, EDGE_REF + 0.13], F)
# the shard whose global indices cross 2^24: rank 4097 of stride 4095 (2^24 - 1 = 4095 * 4097), the job's last, 65 particles
EDGE_SHARD = dict(global_offset=(1 << 24) - 1, global_n=(1 << 24) - 1 + 65, shard_stride=4095)
NAN_AT, INF_AT = 70, 200


def edge_cases():
    """name -> dict(n, x, y, th, w, pose, frame, delta, cov, ref_theta, opts, goff): what the issue's list of edges asks for, each a
    variation of the stage test's case (a full covariance, a scale, both floors, frame 9, headings ref_theta +- 0.2, positions in [8, 16))."""
    def case(seed, n=EDGE_N, ref=EDGE_REF, spread=0.2, centre=None, lo=8.0, hi=16.0, pose=None, frame=EDGE_FRAME, delta=EDGE_DELTA,
             cov=CORRIDOR_COV, opts=EDGE_OPTS, goff=0):
        x, y, th, w = cloud(n, ref if centre is None else centre, spread, seed, lo, hi)
        pose = np.array([0.5 * (lo + hi), 0.25 * lo + 0.75 * hi, (ref if centre is None else centre) + 0.13], F) if pose is None else pose
        return dict(n=n, x=x, y=y, th=th, w=w, pose=pose, frame=frame, delta=delta, cov=cov, ref_theta=float(ref), opts=dict(opts), goff=goff)

    c = {
        "headings all round": case(11, spread=np.pi),
        "phi near +100": case(12, ref=-50.0, centre=50.0, spread=0.5),
        "phi near -100": case(13, ref=50.0, centre=-50.0, spread=0.5),
        "phi near +1100": case(14, ref=-550.0, centre=550.0, spread=0.5),
        "phi near -1100": case(15, ref=550.0, centre=-550.0, spread=0.5),
        "ref_theta +1000": case(16, ref=1000.0),
        "ref_theta -1000": case(17, ref=-1000.0),
        "positions to 2000": case(18, lo=-2000.0, hi=2000.0),
        "positions below 1e-3": case(19, lo=-1e-3, hi=1e-3),
        "first pivot 0": case(20, cov=np.array([0, 0, 0, 0.01, 0.001, 0.0004], F), opts={}),
        "rank 1": case(21, cov=np.array([4, 2, 1, 1, 0.5, 0.25], F) * F(0.0009765625), opts={}),
        "scale 0": case(22, opts=dict(cov_scale=0.0, sigma_theta_min=0.01)),
        "frame 0": case(23, frame=0),
        "frame 1": case(24, frame=1),
        "frame 4194303": case(25, frame=4194303),
        "indices across 2^24": case(26, n=65, goff=EDGE_SHARD["global_offset"]),
    }
    L, _ = factor(c["first pivot 0"]["cov"])
    assert (L[[0, 1, 3]] == 0).all() and (L[[2, 4, 5]] != 0).all()
    L, _ = factor(c["rank 1"]["cov"])
    assert L[0] != 0 and L[1] != 0 and L[3] != 0 and (L[[2, 4, 5]] == 0).all()           # p1 and p2 are exactly 0
    L, _ = factor(c["scale 0"]["cov"], **c["scale 0"]["opts"])
    assert (L[:5] == 0).all() and L[5] == F(0.01)
    for name, least in (("phi near +100", 99), ("phi near -100", 99), ("phi near +1100", 1099), ("phi near -1100", 1099)):
        k = c[name]
        assert (np.sign(k["th"]) == -np.sign(k["ref_theta"])).all() and np.abs(k["th"] - F(k["ref_theta"])).min() > least
    return c


def edge_want(k):
    """(x', y', theta', pose') of an edge case by the restatement."""
    x, y, th = move(k["x"], k["y"], k["th"], k["frame"], k["delta"], k["cov"], k["ref_theta"], goff=k["goff"], **k["opts"])
    return x, y, th, move_pose(k["pose"], k["delta"], k["cov"], k["ref_theta"], **k["opts"])


_STAT = {}


def stat_case():
    """The statistics case, computed once and left unchanged: STAT_N particles at the origin with heading 0 = ref_theta, so that the moved
    particles ARE (mx, my, mt).  Returns (L, a, mx, my, mt)."""
    if not _STAT:
        L, a = factor(CORRIDOR_COV)
        mx, my, mt = increments(draws(STAT_FRAME, np.arange(STAT_N)), STAT_DELTA, L)
        for v in (L, a, mx, my, mt):
            v.setflags(write=False)
        _STAT["v"] = (L, a, mx, my, mt)
    return _STAT["v"]
