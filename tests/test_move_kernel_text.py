"""pfslam_move_particles' kernel text, run on the CPU (no GPU needed): tests/move_emu.cpp compiles the kernel cut out of
csrc/pfslam_move.hip.inc behind tests/simt_shim.h with -ffp-contract=off like the library, under AddressSanitizer and UBSan with every
buffer at its exact size.  Particles and the robot's pose must equal the restatement (tests/move_ref.py) bit for bit with trig 0, at sizes
around the wave and the workgroup and at two global offsets, which also shows that no index leaves a buffer.  What it cannot show is the
GPU's arithmetic: tests/test_gpu_move.py does."""
import numpy as np
import pytest

import kernel_text as KT
import move_ref as M

KT.SECTIONS["move"] = ("pfslam_move.hip.inc", "MOVE", ())

FRAME, REF_THETA = 11, 0.7
DELTA = np.array([0.31, -0.07, 0.045], np.float32)
OPTS = dict(cov_scale=1.5, sigma_xy_min=0.007, sigma_theta_min=0.0036)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return KT.build(tmp_path_factory, "move", ("k_move", "move_pose"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("goff", (0, 1000))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_kernel_text_on_the_cpu_equals_the_restatement(emu, n, goff):
    d, exe = emu
    x, y, th, _ = M.cloud(n, REF_THETA, seed=goff)
    pose = np.array([11.5, 9.25, REF_THETA + 0.13], np.float32)
    cloud = np.arange(8, dtype=np.float32)
    L, _ = M.factor(M.CORRIDOR_COV, **OPTS)
    params = np.concatenate([L, DELTA, [np.float32(REF_THETA)]]).astype(np.float32)
    fin, fout = str(d / ("in_%d_%d.bin" % (n, goff))), str(d / ("out_%d_%d.bin" % (n, goff)))
    with open(fin, "wb") as f:
        for a in (params, pose, cloud, x, y, th):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    KT.run(exe, n, goff, FRAME, 0, fin, fout)
    got = np.fromfile(fout, np.float32)
    assert len(got) == 11 + 3 * n
    wx, wy, wt = M.move(x, y, th, FRAME, DELTA, M.CORRIDOR_COV, REF_THETA, goff=goff, **OPTS)
    want_pose = M.move_pose(pose, DELTA, M.CORRIDOR_COV, REF_THETA, **OPTS)
    assert (bits(got[0:3]) == bits(want_pose)).all(), (got[0:3], want_pose)
    for name, g, w in (("x", got[11:11 + n], wx), ("y", got[11 + n:11 + 2 * n], wy), ("theta", got[11 + 2 * n:], wt)):
        assert (bits(g) == bits(w)).all(), (name, np.flatnonzero(bits(g) != bits(w))[:8])
    assert not (bits(got[11:11 + n]) == bits(x)).any()          # (every particle did move)
    # the cloud statistics of both ticket parities move by the pose's increment (performance only: its spread, [3] and [7], stays)
    inc = want_pose - pose
    want_cloud = cloud.copy()
    want_cloud[0:3] += inc
    want_cloud[4:7] += inc
    assert (bits(got[3:11]) == bits(want_cloud)).all()


def run_text(emu, tag, k, x=None, y=None, th=None):
    """The kernel text on one case of move_ref.edge_cases(): (pose', x', y', theta')."""
    d, exe = emu
    n = k["n"]
    L, _ = M.factor(k["cov"], **k["opts"])
    params = np.concatenate([L, k["delta"], [np.float32(k["ref_theta"])]]).astype(np.float32)
    fin, fout = str(d / ("in_%s.bin" % tag)), str(d / ("out_%s.bin" % tag))
    with open(fin, "wb") as f:
        for a in (params, k["pose"], np.zeros(8, np.float32), k["x"] if x is None else x, k["y"] if y is None else y, k["th"] if th is None else th):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    KT.run(exe, n, k["goff"], k["frame"], 0, fin, fout)
    got = np.fromfile(fout, np.float32)
    assert len(got) == 11 + 3 * n
    return got[0:3], got[11:11 + n], got[11 + n:11 + 2 * n], got[11 + 2 * n:]


EDGES = M.edge_cases()


@pytest.mark.parametrize("name", sorted(EDGES))
def test_kernel_text_at_the_edges_of_its_inputs(emu, name):
    """The input set tests/test_gpu_move.py runs on the device (move_ref.edge_cases): headings all round, |phi| near 100 and 1100 rad,
    ref_theta of +-1000, positions to 2000 m and below a millimetre, zero pivots, frames 0, 1 and 2^22 - 1, global indices across 2^24."""
    k = EDGES[name]
    pose, x, y, th = run_text(emu, "edge_%d" % sorted(EDGES).index(name), k)
    wx, wy, wt, wpose = M.edge_want(k)
    assert (bits(pose) == bits(wpose)).all(), (pose, wpose)
    for fld, g, w in (("x", x, wx), ("y", y, wy), ("theta", th, wt)):
        assert (bits(g) == bits(w)).all(), (name, fld, np.flatnonzero(bits(g) != bits(w))[:8])


def test_kernel_text_keeps_a_particle_that_is_not_finite_to_itself(emu):
    """x = +inf stays +inf, the rest of that particle is the restatement's, and nobody else notices.  The NaN heading of the device test is
    left out here: pf::sincos_core converts the quadrant, a NaN then, to int, which the device defines (and every field the heading enters
    is NaN whatever the quadrant) and C++ on the host does not -- the sanitizer build stops there."""
    k = dict(EDGES["headings all round"])
    x = k["x"].copy()
    x[M.INF_AT] = np.inf
    pose, gx, gy, gt = run_text(emu, "nonfinite", k, x=x)
    wx, wy, wt, wpose = M.edge_want(k)
    assert np.isinf(gx[M.INF_AT]) and gx[M.INF_AT] > 0
    assert (bits(gy) == bits(wy)).all() and (bits(gt) == bits(wt)).all()
    rest = np.ones(k["n"], bool)
    rest[M.INF_AT] = False
    assert (bits(gx[rest]) == bits(wx[rest])).all()
    assert (bits(pose) == bits(wpose)).all()


def test_the_largest_draw_is_below_the_bound_constant_in_both_forms(emu):
    """The heading bound's Z (PF_MOVE_Z in csrc/pfslam_move.hip.inc, 7) must be at or above the largest |normal(., 0, 1)|: the u = 0 draw,
    evaluated here by pf::normal itself in the specification's form and in the device library's (the CPU's log for the GPU's)."""
    d, exe = emu
    out = str(d / "zmax.bin")
    KT.run(exe, "zmax", M.STATE_U0, out)
    z = np.fromfile(out, np.float32)
    print("u = 0 draw: specification %.6f, device-library form %.6f" % (z[0], z[1]))
    assert bits(z[0]) == bits(np.float32(-M.z_max())) or bits(z[0]) == bits(np.float32(M.z_max()))
    assert 6.0 < abs(z[0]) < 7.0 and 6.0 < abs(z[1]) < 7.0
    src = open(KT.os.path.join(KT.CSRC, "pfslam_move.hip.inc")).read()
    assert "#define PF_MOVE_Z 7.0f" in src
