"""pfslam_nearest and pfslam_register on the GPU: both against tests/register_ref.py (the specification restated from the oracle's primitives,
pinned to orc_icp and held to its convergence by tests/test_register_spec.py), register against the existing stage pfslam_icp iterated
from the host, behind frames in flight (it must read and change nothing), on sharded handles, through the replay binary, and its refusals.

Every comparison is bit for bit; there is no tolerance anywhere in this file."""
import ctypes as C
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import register_ref as R
from test_gpu_sharded import _VirtualRanks
from test_host_layer import HOST, SCENE_TXT, build_host

pytestmark = pytest.mark.gpu
START = np.array([0.6, 0.22, 0.13], np.float32)     # 0.10 m / 0.03 rad off the pose the scan was cast from


@pytest.fixture(scope="module")
def world(pkg):
    tree, segs, _ = R.planar_tree(4000, seed=1)
    return {"p4000": tree, "np300": R.nonplanar_tree(300), "grown4500": R.grown_tree(4000, 500, seed=1)[0],
            "scan": pkg.synth.make_scan(segs, (0.5, 0.3, 0.1), seed=7), "segs": segs}


def truncated(want, k):
    """What a run of at most k iterations returns, from a longer run `want` of the same options."""
    if want["iterations"] < k or (want["iterations"] == k and want["status"] in (0, 1)):
        return want
    t = want["trace"][:k]                              # the longer run went on (or failed in a later iteration): k rows, none passed eps
    return {"pose": t[-1, 0:3].copy(), "status": 0, "iterations": k, "pairs": int(t[-1, 6]), "residual": float(t[-1, 7]), "trace": t.copy()}


# ---- 1. nearest --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p4000", "np300", "grown4500"])
def test_nearest_equals_brute_force_on_every_kind_of_tree(pkg, world, name):
    tree = world[name]
    q = R.tie_queries(tree, 2000)
    q[7] = [np.nan, 0.0, 0.0]
    q[8] = [0.0, -np.inf, 0.0]
    h = pkg.PfSlam(64, kd_capacity=1 << 16)
    h.set_map(tree)
    best, d2 = h.nearest(q)
    wb, wd = R.nearest(tree, q)
    assert (best == wb).all(), np.nonzero(best != wb)[0][:10]
    assert (R.bits(d2) == R.bits(wd)).all()
    assert best[7] == -1 and best[8] == -1
    # the reference's traversal is NOT this: the two differ on this very set
    assert (h.traverse(q[9:]) != best[9:]).any()
    h.close()


def test_nearest_on_a_map_replaced_after_a_frame_has_run(pkg, world):
    h = pkg.PfSlam(300, kd_capacity=1 << 16)
    _, frames = pkg.synth.corridor_sequence(3, seed=5)
    for f, (_, scan) in enumerate(frames, start=1):
        h.step(f, scan)
    grown = h.map()                                   # the map the frames built: Create + device-side InsertNode
    q = R.tie_queries(grown, 600)
    best, d2 = h.nearest(q)
    wb, wd = R.nearest(grown, q)
    assert (best == wb).all() and (R.bits(d2) == R.bits(wd)).all()
    h.set_map(world["np300"])
    q = R.tie_queries(world["np300"], 600)
    best, d2 = h.nearest(q)
    wb, wd = R.nearest(world["np300"], q)
    assert (best == wb).all() and (R.bits(d2) == R.bits(wd)).all()
    h.close()


# ---- 2. register against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 65, 1025, 1081])
def test_register_equals_the_restatement_for_every_option_combination(pkg, world, nb):
    """Every (match, select, update), max_iters 1, 2 and 7 (the shorter runs are prefixes of the restatement's 7), with set_trig(0)."""
    tree = world["p4000"]
    scan = np.resize(world["scan"], nb) if nb != 1081 else world["scan"]
    h = pkg.PfSlam(64, n_beams=nb, kd_capacity=1 << 16)
    h.set_map(tree)
    h.set_scan(scan)
    h.set_trig(0)
    for match, select, update in itertools.product((0, 1), repeat=3):
        opts = dict(match=match, select=select, update=update, max_dist=0.5 if nb > 1 else 0.0, min_pairs=1)
        want7 = R.register(tree, scan, START, max_iters=7, **opts)
        for k in (1, 2, 7):
            got = h.register(START, max_iters=k, **opts)
            diff = R.same_result(got, truncated(want7, k))
            assert diff is None, "beams %d, match %d select %d update %d, max_iters %d: %s" % (nb, match, select, update, k, diff)
    h.close()


def test_register_defaults_converge_on_the_device_as_in_the_restatement(pkg, world):
    tree, scan = world["p4000"], world["scan"]
    h = pkg.PfSlam(64, kd_capacity=1 << 16)
    h.set_map(tree)
    h.set_scan(scan)
    h.set_pose(START)
    got = h.register()                                 # start = the handle's pose, every option at its default
    want = R.register(tree, scan, START)
    assert R.same_result(got, want) is None, R.same_result(got, want)
    assert got["status"] == 1 and 1 < got["iterations"] < 40
    err = np.abs(got["pose"].astype(np.float64) - np.array([0.5, 0.3, 0.1]))
    assert err[0] <= 0.025 and err[1] <= 0.025 and err[2] <= np.deg2rad(0.25)
    for name in ("np300", "grown4500"):
        h.set_map(world[name])
        opts = dict(max_iters=4, max_dist=0.5 if name == "grown4500" else 0.0)
        got, want = h.register(START, **opts), R.register(world[name], scan, START, **opts)
        assert R.same_result(got, want) is None, (name, R.same_result(got, want))
    far = np.full(1081, 1000.0, np.float32)
    h.set_scan(far)
    got = h.register(START)
    assert got["status"] == 2 and got["iterations"] == 0 and (R.bits(got["pose"]) == R.bits(START)).all() and got["trace"].shape == (0, 8)
    h.close()


# ---- 3. register against the existing stage ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trig", [0, 1])
def test_reference_options_equal_the_icp_stage_iterated_from_the_host(pkg, world, trig):
    """match 0, select 0, update 0: trace row k is set_pose(p_k); icp(start = p_k) on the same handle, in either arithmetic mode; status 3
    exactly where the stage's pose turns non-finite."""
    tree, scan = world["p4000"], world["scan"]
    h = pkg.PfSlam(64, kd_capacity=1 << 16)
    h.set_map(tree)
    h.set_scan(scan)
    h.set_trig(trig)
    ref = dict(match=0, select=0, update=0, eps_xy=0.0, eps_theta=0.0)
    for start, iters in ((START, 7), (np.array([3.0e38, 3.0e38, 0.1], np.float32), 3)):
        got = h.register(start, max_iters=iters, **ref)
        p, rows = np.array(start, np.float32), []
        for _ in range(iters):
            h.set_pose(p)
            nxt, _ = h.icp(start=p)
            if not np.isfinite(nxt).all():
                break
            rows.append(nxt.copy())
            p = nxt
        assert got["iterations"] == len(rows) and got["status"] == (0 if len(rows) == iters else 3)
        assert (R.bits(got["pose"]) == R.bits(p)).all()
        if rows:
            assert (R.bits(got["trace"][:, 0:3]) == R.bits(np.stack(rows))).all()
    assert got["status"] == 3, "the overflowing start was meant to end with status 3"
    h.close()


# ---- 4. read-only ------------------------------------------------------------------------------------------------------------------------
def test_register_behind_frames_in_flight_reads_and_changes_nothing(pkg):
    torch = pytest.importorskip("torch")
    sharded = importlib.import_module("gpu-icp-slam_amd.sharded")

    def buffers(e):
        out = []
        for which in (11, 12):
            ptr, nbytes = e.device_ptr(which)
            t = torch.as_tensor(sharded._DevView(ptr, nbytes, "<i4", 4), device=torch.device("cuda", 0))
            out.append(t.cpu().numpy().tobytes())
        return out

    n = 1000
    _, frames = pkg.synth.corridor_sequence(9, seed=5)
    h, twin = pkg.PfSlam(n, kd_capacity=1 << 16), pkg.PfSlam(n, kd_capacity=1 << 16)
    seen = []
    for f, (_, scan) in enumerate(frames, start=1):
        h.step(f, scan)
        twin.step(f, scan)
        if f in (4, 7):                                  # a frame is in flight (default lag): register books it first
            for opts in (dict(max_iters=4), dict(match=0, select=0, update=0, max_iters=3)):
                got = h.register(**opts)
                want = R.register(h.map(), scan, h.pose, **opts)
                assert R.same_result(got, want) is None, (f, opts, R.same_result(got, want))
                seen.append(got)
            assert (R.bits(h.pose) == R.bits(twin.pose)).all()
            assert buffers(h) == buffers(twin), "buffers 11 / 12 after frame %d" % f
            assert h.check_cells()["violations"] == 0
    assert seen[0]["iterations"] >= 1
    assert (R.bits(h.pose) == R.bits(twin.pose)).all()
    ph, pt = h.particles(), twin.particles()
    for fld in ("x", "y", "theta", "w"):
        assert (R.bits(ph[fld]) == R.bits(pt[fld])).all(), fld
    assert h.map().tobytes() == twin.map().tobytes()
    assert buffers(h) == buffers(twin)
    assert h.check_cells()["violations"] == 0 and twin.check_cells()["violations"] == 0
    h.close(); twin.close()


# ---- 5. wrappers -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_every_rank_of_a_sharded_job_gets_the_unsharded_bits(pkg, nranks):
    torch = pytest.importorskip("torch")
    n = 1000
    kw = dict(kd_capacity=1 << 16)
    one = pkg.PfSlam(n, **kw)
    v = _VirtualRanks(pkg, torch, n, nranks, **kw)
    _, frames = pkg.synth.corridor_sequence(5, seed=5)
    for f, (_, scan) in enumerate(frames, start=1):
        one.step(f, scan)
        v.step(f, scan)
    v._sync()
    for opts in (dict(), dict(match=0, select=0, update=0, max_iters=3)):
        want = one.register(**opts)
        assert want["iterations"] >= 1
        for r, e in enumerate(v.engs):
            diff = R.same_result(e.register(**opts), want)
            assert diff is None, "rank %d of %d: %s" % (r, nranks, diff)
    assert R.same_result(want, R.register(one.map(), frames[-1][1], one.pose, **opts)) is None
    v.close(); one.close()


def test_sharded_wrapper_passes_register_through(pkg):
    torch = pytest.importorskip("torch")
    sharded = importlib.import_module("gpu-icp-slam_amd.sharded")
    a = pkg.PfSlam(500, kd_capacity=1 << 16)
    s = sharded.ShardedSlam(pkg, 500, 0, 1, device=0, torch=torch, kd_capacity=1 << 16)
    _, frames = pkg.synth.corridor_sequence(4, seed=7)
    for f, (_, scan) in enumerate(frames, start=1):
        a.step(f, scan)
        s.step(f, scan)
    issued = s.collectives
    assert R.same_result(s.register(max_iters=5), a.register(max_iters=5)) is None and s.collectives == issued
    a.close(); s.eng.close()


def test_replay_binary_with_register_5_prints_the_handle_s_registration(tmp_path, pkg):
    """pfslamRegister (host/kernel.h) through `pfslam_replay ... register=5`: one line per frame whose float bits are the C-ABI's."""
    build_host(pkg)
    _, frames = pkg.synth.corridor_sequence(6, seed=5)
    scene = tmp_path / "scene.txt"
    scene.write_text(SCENE_TXT)
    scans = np.stack([np.zeros(1081, np.float32)] + [s for _, s in frames])  # scans[0] is never used (frame starts at 1)
    lidar = tmp_path / "lidar.f32"
    scans.astype(np.float32).tofile(str(lidar))
    env = dict(os.environ, PFSLAM_PARTICLES="300", PFSLAM_KD_CAPACITY=str(1 << 16))
    out = subprocess.check_output([os.path.join(HOST, "pfslam_replay"), str(scene), str(lidar), "register=5"], env=env).decode()
    lines = [l for l in out.splitlines() if l.startswith("register ")]
    assert len(lines) == len(frames)
    h = pkg.PfSlam(300, kd_capacity=1 << 16)
    for f, ((_, scan), line) in enumerate(zip(frames, lines), start=1):
        h.step(f, scan)
        got = h.register(h.pose, max_iters=5)
        tok = line.split()
        assert tok[1] == str(f) and tok[2] == "pose" and tok[6] == "status" and tok[8] == "iterations" and tok[10] == "bits" and len(tok) == 14, line
        assert [int(v, 16) for v in tok[11:14]] == got["pose"].view(np.uint32).tolist(), line
        assert int(tok[7]) == got["status"] and int(tok[9]) == got["iterations"], line
    h.close()
    out = subprocess.check_output([os.path.join(HOST, "pfslam_replay"), str(scene), str(lidar)], env=env).decode()
    assert not [l for l in out.splitlines() if l.startswith("register ")]


def test_refusals_name_their_cause_and_the_handle_goes_on(pkg, world):
    h = pkg.PfSlam(64, kd_capacity=1 << 16)
    with pytest.raises(pkg.PfSlamError, match="pfslam_register: no map loaded"):
        h.register(START)
    with pytest.raises(pkg.PfSlamError, match="pfslam_nearest: no map loaded"):
        h.nearest(np.zeros((3, 3), np.float32))
    h.set_map(world["p4000"])
    h.set_scan(world["scan"])
    for bad, cause in ((dict(max_iters=0), "max_iters"), (dict(max_iters=65), "max_iters"), (dict(match=2), "match"), (dict(select=-1), "select"),
                       (dict(update=2), "update"), (dict(max_dist=float("nan")), "max_dist"), (dict(eps_xy=-1.0), "eps"),
                       (dict(eps_theta=float("inf")), "eps")):
        with pytest.raises(pkg.PfSlamError, match="pfslam_register: .*%s" % cause):
            h.register(START, **bad)
    o = pkg.binding.RegisterOpts()
    h.L.pfslam_register_default_opts(C.byref(o))
    o.match = 7
    pose, info, trace = np.full(3, 7.5, np.float32), np.full(8, 7.5, np.float32), np.full((40, 8), 7.5, np.float32)
    assert h.L.pfslam_register(h._h, START.ctypes.data_as(C.c_void_p), C.byref(o), pose.ctypes.data_as(C.c_void_p),
                               info.ctypes.data_as(C.c_void_p), trace.ctypes.data_as(C.c_void_p)) != 0
    assert (pose == 7.5).all() and (info == 7.5).all() and (trace == 7.5).all(), "an output was written"
    with pytest.raises(pkg.PfSlamError, match="at most 4096 beams"):   # (no handle can hold more: pfslam_register's own refusal of
        pkg.PfSlam(64, n_beams=4097, kd_capacity=1 << 16)             #  n_beams > 4096 cannot be reached through pfslam_create)
    got = h.register(START, max_iters=3)
    assert R.same_result(got, R.register(world["p4000"], world["scan"], START, max_iters=3)) is None
    h.close()
