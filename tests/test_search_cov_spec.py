"""The specification of pfslam_search_cov / pfslam_search_scan_cov (include/pfslam.h), without a GPU: header, binding and library carry the
entry points, and tests/search_cov_ref.py -- the restatement the kernel text and the GPU are held to bit for bit -- computes what it
claims to compute:
  * (a) exp2m: the polynomial within 2e-15 relative of 2^-f (measured 4.5e-16), w(0) = 1, non-increasing, 0 from t = 64 on;
  * (b) the restatement against a float64 computation of the same weights, within tests/test_estimate_spec.py's bounds;
  * (c) adding a constant to every score changes no bit;
  * (d) with sigma = 1000 the weights are flat and C is the lattice's own variance: C_xx within 1e-3 relative of
        ((nx^2 - 1) / 12) (stride res)^2, likewise for y and theta;
  * (e) the two scenarios the covariance was made for, scan to scan, 1081 beams, window 21 x 21 x 9 at stride 1, the reference scan at
        (0, 0, 0), the searched scan cast from (0.1, 0.05, 0.0125) and the window centred there (with the window centred on the
        reference pose the corridor gives sd_x 0.070 m, Neff 10.4 and a border share of 0.002 instead of 0.106 m, 11.9 and 0.040),
        sigma 0.2: between two walls y = +-1 the winner is 0.1 m off along the corridor and C_xx >= 100 C_yy (measured 1290) with a
        border share > 0.01 (0.040); in a closed 6 m x 4 m room C_xx <= 0.05 of the corridor's (measured 0.018) and the border share
        < 1e-6 (2e-17);
  * (f) the refusals and their order."""
import ctypes as C
import math

import numpy as np
import pytest

import estimate_ref as E
import search_cov_ref as SC
import search_ref as S
import search_scan_ref as SS

F = np.float32
WINDOW = dict(half_x=10, half_y=10, half_theta=4)                       # 21 x 21 x 9 at stride 1 and the default 0.0125 rad
REF_POSE = np.zeros(3, np.float32)
POSE = (0.1, 0.05, 0.0125)
CENTRE = np.array(POSE, np.float32)                                     # the window's centre: the pose the searched scan was cast from
CORRIDOR = np.array([[-30.0, 1.0, 30.0, 1.0], [-30.0, -1.0, 30.0, -1.0]])
ROOM = np.array([[-3.0, 2.0, 3.0, 2.0], [-3.0, -2.0, 3.0, -2.0], [-3.0, -2.0, -3.0, 2.0], [3.0, -2.0, 3.0, 2.0]])
_SCENE = {}


def scene(pkg, name):
    """(reference scan, searched scan, the search's result with its volume), computed once and left unchanged."""
    if name not in _SCENE:
        segs = CORRIDOR if name == "corridor" else ROOM
        ref, scan = pkg.synth.make_scan(segs, tuple(REF_POSE), seed=7), pkg.synth.make_scan(segs, POSE, seed=8)
        _SCENE[name] = (ref, scan, SS.search(ref, REF_POSE, scan, CENTRE, **WINDOW))
    return _SCENE[name]


def cov_of(pkg, name, sigma=0.2, shift=0):
    found = scene(pkg, name)[2]
    return SC.reduce(found["scores"] + np.int32(shift), CENTRE, 0.025, sigma, **WINDOW)


def test_header_binding_classes_and_library_carry_the_entry_points(pkg):
    L = pkg.load()
    for name in ("pfslam_search_cov", "pfslam_search_scan_cov", "pfslam_search_cov_default_opts"):
        assert hasattr(L, name) and name in pkg.binding.SYMBOLS, name
    assert callable(pkg.PfSlam.search_cov) and callable(pkg.PfSlam.search_scan_cov)
    from importlib import import_module
    sh = import_module("gpu-icp-slam_amd.sharded").ShardedSlam
    assert callable(sh.search_cov) and callable(sh.search_scan_cov)
    q = pkg.binding.CovOpts()
    assert C.sizeof(q) == 16
    q.sigma, q.reserved_[2] = 7.0, 5
    L.pfslam_search_cov_default_opts(C.byref(q))
    assert q.sigma == F(0.2) and list(q.reserved_) == [0, 0, 0]
    L.pfslam_search_cov_default_opts(None)                              # (a NULL is left alone)
    # a NULL handle is refused before anything touches a device
    assert L.pfslam_search_cov(None, None, None, None, None, None, None, None) != 0
    assert L.pfslam_last_error().decode() == "pfslam_search_cov: bad argument"
    assert L.pfslam_search_scan_cov(None, None, None, None, None, None, None, None, None, None, None) != 0
    assert L.pfslam_last_error().decode() == "pfslam_search_scan_cov: bad argument"


def test_the_binding_unpacks_the_sixteen_floats(pkg):
    d = pkg.PfSlam._cov_dict({}, np.arange(16, dtype=np.float32))
    assert d["mean"].tolist() == [0, 1, 2] and d["cov"].dtype == np.float32
    assert d["cov"].tolist() == [[3, 4, 5], [4, 6, 7], [5, 7, 8]]
    assert (d["neff"], d["edge"]) == (9.0, 13.0) and d["raw"].tolist() == list(range(16))


# ---- (a) exp2m ---------------------------------------------------------------------------------------------------------------------------
def test_exp2m_the_polynomial_is_within_2e_15_of_exp2():
    rng = np.random.RandomState(24)
    t = np.concatenate([rng.uniform(0, 1, 100000), rng.uniform(0, 64, 100000), [0.0, 0.5, 1.0 - 2.0 ** -24, 63.999996]]).astype(np.float32)
    p, n, live = SC.exp2m_parts(t)
    assert live.all()
    f = t.astype(np.float64) - n
    assert (f >= 0).all() and (f < 1).all()
    exp2 = getattr(math, "exp2", lambda v: math.pow(2.0, v))           # (math.exp2 is new in Python 3.11; pow(2, v) is the same libm quality)
    want = np.array([exp2(-v) for v in f])
    rel = np.abs(p - want) / want
    print("exp2m: the polynomial's largest relative error over %d arguments: %.3g" % (len(t), rel.max()))
    assert rel.max() <= 2e-15
    w = SC.exp2m(t)
    assert (np.abs(w.astype(np.float64) - np.exp2(-t.astype(np.float64))) <= 6.0e-8 * np.exp2(-t.astype(np.float64))).all()      # (half an ulp of a float)


def test_exp2m_is_1_at_0_does_not_increase_and_ends_at_64():
    assert SC.exp2m(np.zeros(1, np.float32)).view(np.int32)[0] == F(1.0).view(np.int32)
    rng = np.random.RandomState(25)
    t = np.sort(np.concatenate([rng.uniform(0, 70, 200000), np.arange(0, 66), np.arange(1, 65) - 2.0 ** -19]).astype(np.float32))
    w = SC.exp2m(t)
    assert (np.diff(w) <= 0).all() and (w >= 0).all() and (w <= 1).all()
    below = np.nextafter(F(64.0), F(0.0))
    edge = SC.exp2m(np.array([below, 64.0, 64.5, 1e30, np.inf, np.nan], np.float32))
    assert edge[0] > 0 and abs(float(edge[0]) - 2.0 ** -float(below)) <= 6.0e-8 * 2.0 ** -64 and (edge[1:].view(np.int32) == 0).all()
    # integer arguments are exact powers of two
    k = np.arange(0, 64)
    assert (SC.exp2m(k.astype(np.float32)).astype(np.float64) == np.ldexp(1.0, -k)).all()


def test_the_scale_and_the_weights_follow_the_header():
    u, _ = S.unit_cap(0.025, 0.2)
    hs = SC.scale(u, 0.2)
    assert abs(float(hs) - float(u) * 1.442695 / 0.08) <= 1e-6 * float(hs) and SC.LOG2E.view(np.uint32) == 0x3fb8aa3b
    vol = np.array([[[700, 712, S.NONE, 700 + (1 << 25) + 1]]], np.int32)
    w = SC.weights(vol, 700, hs)
    assert w[0] == 1 and w[2] == 0 and 0 < w[1] < 1 and w[3] == 0
    assert w[1] == SC.exp2m(np.array([F(12.0) * hs], np.float32))[0]
    # above 2^24 the difference rounds to nearest even on its way to float
    slow = SC.scale(u, 50.0)
    d = (1 << 24) + 1
    assert SC.weights(np.array([0, d], np.int32), 0, slow)[1] == SC.exp2m(np.array([F(1 << 24) * slow], np.float32))[0]


# ---- (b) against float64 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", (0.2, 1000.0))
@pytest.mark.parametrize("name", ("corridor", "room"))
def test_restatement_against_float64(pkg, name, sigma):
    """At sigma 0.2 and 1000 the posterior is spread over the lattice, as the clouds of tests/test_estimate_spec.py are spread, and that
    file's bounds apply.  (At sigma 0.05 it collapses onto one row of the lattice: C_yy is then the square of the mean's own rounding
    error, 1e-17 and less, and a bound relative to C says nothing; the kernel text and the GPU are still held to those bits.)"""
    found = scene(pkg, name)[2]
    raw = cov_of(pkg, name, sigma)
    w = SC.weights(found["scores"], int(found["scores"].min()), raw[14])
    x, y, t, edge = SC.poses(CENTRE, dict(S.DEFAULTS, **WINDOW), 0.025)
    m64, c64, neff64 = E.estimate_f64(x, y, t, w)
    err_m = np.abs(raw[0:3].astype(np.float64) - m64)
    print("%s sigma %g: mean error %s" % (name, sigma, err_m))
    assert (err_m <= 4e-6).all(), err_m
    diag = {0: c64[0], 1: c64[3], 2: c64[5]}
    for q, (k, l) in enumerate(E.PAIRS):
        err, scale = abs(float(raw[3 + q]) - c64[q]), np.sqrt(diag[k] * diag[l])
        print("  C[%d%d] %.6g error %.3g, relative %.3g" % (k, l, c64[q], err, err / scale if scale > 0 else 0.0))
        assert err <= 1e-6 * scale, (k, l, err, scale)
    assert abs(float(raw[9]) - neff64) <= 3e-5 * neff64
    share64 = w.astype(np.float64)[edge].sum() / w.astype(np.float64).sum()
    assert abs(float(raw[13]) - share64) <= 3e-5 * share64 + 1e-30
    assert raw[12] == 21 * 21 * 9 and raw[15] == 0 and raw[10] >= 1
    # the weights themselves against exp in float64: the likelihood of the header's model
    d = (found["scores"].astype(np.float64) - found["scores"].min()).ravel()
    want = np.exp(-d * float(S.unit_cap(0.025, 0.2)[0]) / (2.0 * sigma * sigma))
    keep = want > 1e-12
    assert (np.abs(w[keep] - want[keep]) <= 2e-5 * want[keep]).all()


# ---- (c) a constant ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", (1, 1000, 1 << 20))
def test_adding_a_constant_to_every_score_changes_no_bit(pkg, shift):
    for name in ("corridor", "room"):
        assert SC.same_cov(cov_of(pkg, name, 0.2, shift), cov_of(pkg, name)) is None


# ---- (d) flat weights --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", (1, 3))
def test_with_sigma_1000_the_covariance_is_the_lattice_s(pkg, stride):
    found = scene(pkg, "corridor")[2]
    opts = dict(WINDOW, stride=stride, half_x=10, half_y=7, half_theta=4, step_theta=0.01)
    vol = found["scores"][:, 3:18, :]                                   # (any scores do: the weights are flat)
    raw = SC.reduce(vol, np.array([0.3, -0.2, 0.1], np.float32), 0.025, 1000.0, **opts)
    for q, n, step in ((3, 21, stride * 0.025), (6, 15, stride * 0.025), (8, 9, 0.01)):
        want = (n * n - 1) / 12.0 * step * step
        print("C[%d] %.6g, the lattice's %.6g" % (q, raw[q], want))
        assert abs(float(raw[q]) - want) <= 1e-3 * want
    assert abs(float(raw[9]) - vol.size) <= 1e-3 * vol.size


# ---- (e) the scenarios -------------------------------------------------------------------------------------------------------------------
def test_the_corridor_is_undetermined_along_it_and_the_room_is_not(pkg):
    cor, room = scene(pkg, "corridor")[2], scene(pkg, "room")[2]
    c, r = cov_of(pkg, "corridor"), cov_of(pkg, "room")
    for name, found, raw in (("corridor", cor, c), ("room", room, r)):
        print("%s: winner %s, sd %.4g m / %.4g m / %.4g rad, Neff %.3g, border share %.3g" % (name, found["pose"].tolist(), raw[3] ** 0.5, raw[6] ** 0.5,
                                                                                            raw[8] ** 0.5, raw[9], raw[13]))
    assert cor["status"] == 0 and room["status"] == 0
    assert np.abs(room["pose"].astype(np.float64) - np.array(POSE)).max() <= 1e-6 and abs(float(cor["pose"][0])) <= 1e-6                   # the room's winner is the pose itself
    assert abs(float(cor["pose"][1]) - 0.05) <= 1e-6 and abs(float(cor["pose"][2]) - 0.0125) <= 1e-6   # the corridor's: right across, arbitrary along
    assert c[3] >= 100 * c[6] and c[13] > 0.01
    assert r[3] <= 0.05 * c[3] and r[13] < 1e-6
    # the figures the header quotes, to the digits it quotes: sd_x 0.106, Neff 11.9, share 0.040; sd 0.014 / 0.0049 / 0.0050, Neff 2.9
    for got, want in ((c[3] ** 0.5, 0.106), (c[9], 11.9), (c[13], 0.040), (r[3] ** 0.5, 0.014), (r[6] ** 0.5, 0.0049), (r[8] ** 0.5, 0.0050), (r[9], 2.9)):
        assert abs(float(got) - want) <= 0.04 * want, (float(got), want)


# ---- (f) refusals ------------------------------------------------------------------------------------------------------------------------
def test_the_order_of_the_refusals():
    nan3, ok3 = (0.0, np.nan, 0.0), (0.0, 0.0, 0.0)
    for scan_form in (True, False):
        kw = dict(scan_form=scan_form, centre=ok3)
        assert SC.refusal(1081, **kw) is None
        assert SC.refusal(1081, cov=False, half_x=-1, **kw) == "bad argument" and SC.refusal(1081, cov_out=False, sigma=-1.0, **kw) == "bad argument"
        # everything of the search comes first
        assert "must be >= 0" in SC.refusal(1081, sigma=0.0, half_y=-1, **kw)
        assert "stride" in SC.refusal(1081, sigma=np.nan, stride=65, **kw)
        assert "1 .. 65535" in SC.refusal(1081, sigma=0.0, max_dist=1.6, **kw)
        assert "2^24 candidates" in SC.refusal(1081, reserved=(0, 1, 0), half_x=2048, half_y=2048, half_theta=0, **kw)
        assert "2^26 cells" in SC.refusal(1081, sigma=0.0, half_x=1000, half_y=0, half_theta=0, stride=64, **kw)
        assert "centre must be finite" in SC.refusal(1081, scan_form=scan_form, centre=nan3, sigma=0.0)
        # then sigma, reserved_, hs
        for bad in (0.0, -0.2, np.inf, np.nan):
            assert SC.refusal(1081, sigma=bad, reserved=(1, 0, 0), **kw) == "sigma must be finite and > 0"
        for r in ((1, 0, 0), (0, 1, 0), (0, 0, -1)):
            assert "reserved_ of pfslam_cov_opts" in SC.refusal(1081, reserved=r, sigma=1e30, **kw)
        assert "it must be finite and > 0" in SC.refusal(1081, sigma=1e30, **kw)      # sigma * sigma overflows: hs = 0
        assert "it must be finite and > 0" in SC.refusal(1081, sigma=1e-22, **kw)     # sigma * sigma underflows to a denormal: hs = inf
        assert SC.refusal(1081, sigma=1000.0, **kw) is None and SC.refusal(1081, sigma=1e-3, **kw) is None
    assert SC.refusal(1081, scan_form=False, centre=ok3, have_map=False, sigma=0.0) == "no map loaded"
    assert "ref_scan_host" in SC.refusal(1081, ref_scan=False, sigma=0.0) and "ref_pose must be finite" in SC.refusal(1081, ref_pose=nan3, sigma=0.0)
