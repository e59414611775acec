"""pfslam_register_batch on the GPU.  Its definition is pfslam_register: every row is compared with that call on the same handle, pose and
all eight info floats, through the C-ABI -- for one row, two, and one more than the device has compute units; for scans of 1 to 4096
beams (the 128 KB LDS launch); on every kind of tree; for all eight option combinations; in both trigonometry modes; in batches whose
rows stop at different iterations or fail.  Then against the restatement (tests/register_batch_ref.py), behind frames in flight (it must
read and change nothing), after its buffers grew and the map was replaced, on sharded handles, through the replay binary, and its
refusals.  *best is held to the restated rule and, in the scenario of tests/test_register_batch_spec.py, to the pose the scan was cast from.

Every comparison is bit for bit; there is no tolerance anywhere in this file but the scenario's one map cell and one beam step."""
import ctypes as C
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest

import register_batch_ref as B
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


def starts_of(m, seed=3):
    """m starts: START, then offsets of up to 0.3 m and 0.1 rad around it."""
    rng = np.random.RandomState(seed)
    d = rng.uniform(-1.0, 1.0, (m, 3)) * np.array([0.3, 0.3, 0.1])
    d[0] = 0.0
    return (START.astype(np.float64) + d).astype(np.float32)


def options(pkg, h, **opts):
    o = pkg.binding.RegisterOpts()
    h.L.pfslam_register_default_opts(C.byref(o))
    for k, v in opts.items():
        setattr(o, k, v)
    return o


def rows_of_register(pkg, h, starts, **opts):
    """poses (m, 3) and info (m, 8) of one pfslam_register call per start, through the C-ABI (no trace)."""
    o = options(pkg, h, **opts)
    starts = np.ascontiguousarray(starts, np.float32).reshape(-1, 3)
    poses, info = np.zeros((len(starts), 3), np.float32), np.zeros((len(starts), 8), np.float32)
    for r in range(len(starts)):
        p, f = np.zeros(3, np.float32), np.zeros(8, np.float32)
        rc = h.L.pfslam_register(h._h, starts[r].ctypes.data_as(C.c_void_p), C.byref(o), p.ctypes.data_as(C.c_void_p),
                                 f.ctypes.data_as(C.c_void_p), None)
        assert rc == 0, h.L.pfslam_last_error()
        poses[r], info[r] = p, f
    return {"poses": poses, "info": info, "best": B.pick_best(info)}


def assert_rows_are_register(pkg, h, starts, what="", **opts):
    got = h.register_batch(starts, **opts)
    want = rows_of_register(pkg, h, starts, **opts)
    diff = B.same_rows(got, want)
    assert diff is None, "%s %r: %s" % (what, opts, diff)
    return got


# ---- 1. rows equal pfslam_register ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 65, 1025, 1081, 4096])
def test_rows_equal_register_for_one_two_and_257_rows_in_both_trig_modes(pkg, world, nb):
    """257 rows: one more than the compute units, so at least one compute unit takes a second workgroup; 4096 beams: the 128 KB launch."""
    scan = np.resize(world["scan"], nb) if nb != 1081 else world["scan"]
    h = pkg.PfSlam(64, n_beams=nb, kd_capacity=1 << 16)
    h.set_map(world["p4000"])
    h.set_scan(scan)
    for trig in (0, 1):
        h.set_trig(trig)
        for m in (1, 2, 257):
            got = assert_rows_are_register(pkg, h, starts_of(m), "beams %d trig %d rows %d" % (nb, trig, m),
                                           max_iters=2 if m == 257 else 3, max_dist=0.5 if nb > 1 else 0.0, min_pairs=1)
            assert got["poses"].shape == (m, 3) and (got["iterations"] >= 1).any()
    h.close()


@pytest.mark.parametrize("name", ["p4000", "np300", "grown4500"])
def test_rows_equal_register_on_every_kind_of_tree(pkg, world, name):
    h = pkg.PfSlam(64, kd_capacity=1 << 16)
    h.set_map(world[name])
    h.set_scan(world["scan"])
    for m in (2, 257):
        got = assert_rows_are_register(pkg, h, starts_of(m), name, max_iters=3 if m == 2 else 2, max_dist=0.0 if name == "np300" else 0.5)
        assert (got["iterations"] >= 1).any()
    h.close()


def test_rows_equal_register_for_all_eight_option_combinations(pkg, world):
    h = pkg.PfSlam(64, kd_capacity=1 << 16)
    h.set_map(world["p4000"])
    h.set_scan(world["scan"])
    for match, select, update in itertools.product((0, 1), repeat=3):
        got = assert_rows_are_register(pkg, h, starts_of(2), "combination", match=match, select=select, update=update, max_iters=3)
        assert (got["iterations"] == 3).all() or (got["status"] != 0).any()
    h.close()


@pytest.mark.parametrize("p", B.SCENARIO_POSES)
def test_the_scenario_rows_are_register_and_best_is_the_rule_s_and_meets_the_bound(pkg, world, p):
    """The 26 starts of tests/test_register_batch_spec.py, 20 iterations each: the one long run of this file."""
    scan = pkg.synth.make_scan(world["segs"], p, seed=7)
    h = pkg.PfSlam(64, kd_capacity=1 << 16)
    h.set_map(world["p4000"])
    h.set_scan(scan)
    got = assert_rows_are_register(pkg, h, B.scenario_starts(p), "scenario", max_iters=20)
    assert got["best"] == B.pick_best(got["info"]) and got["best"] >= 0
    inside, err = B.within_bounds(got["poses"][got["best"]], p)
    ok = sum(B.within_bounds(got["poses"][r], p)[0] for r in range(26))
    print("pose %s: best row %d, |error| = %.5f m %.5f m %.6f rad; %d of 26 rows meet the bound" % (p, got["best"], err[0], err[1], err[2], ok))
    assert inside, err
    h.close()


# ---- 2. rows equal the restatement -----------------------------------------------------------------------------------------------------------
def test_rows_equal_the_restatement(pkg, world):
    """6 rows x 3 iterations with the defaults and with the reference's options, 2 x 3 on the non-planar map: 42 row-iterations."""
    h = pkg.PfSlam(64, kd_capacity=1 << 16)
    h.set_scan(world["scan"])
    h.set_trig(0)
    for name, m, opts in (("p4000", 6, dict(max_iters=3)), ("p4000", 6, dict(match=0, select=0, update=0, max_iters=3)),
                          ("np300", 2, dict(max_iters=3, max_dist=0.0))):
        h.set_map(world[name])
        starts = starts_of(m)
        got, want = h.register_batch(starts, **opts), B.register_batch(world[name], world["scan"], starts, **opts)
        assert B.same_rows(got, want) is None, (name, opts, B.same_rows(got, want))
        for k in ("status", "iterations", "pairs"):
            assert (got[k] == want[k]).all()
        assert (R.bits(got["residual"]) == R.bits(want["residual"])).all()
    h.close()


# ---- 3. rows that stop early or fail -----------------------------------------------------------------------------------------------------------
def test_a_mixed_batch_of_early_stops_failures_and_a_nan_start(pkg, world):
    """No gate, so that a start whose targets overflow reaches the fit (status 3); a NaN heading puts no beam in range (status 2); the
    other rows stop on a coarse eps after different numbers of iterations.  Each row is still its own pfslam_register."""
    h = pkg.PfSlam(64, kd_capacity=1 << 16)
    h.set_map(world["p4000"])
    h.set_scan(world["scan"])
    starts = np.concatenate([np.array([[0.6, 0.22, np.nan], [3.0e38, 3.0e38, 0.1], [np.nan, 0.3, 0.1], [0.5, 0.3, 0.1]], np.float32), starts_of(40),
                             np.array([[np.inf, 0.0, 0.0], [0.5, 0.3, 0.1]], np.float32)])
    got = assert_rows_are_register(pkg, h, starts, "mixed", max_dist=0.0, max_iters=12, eps_xy=5e-3, eps_theta=1e-3)
    print("mixed batch: status %s iterations %s best %d" % (got["status"].tolist(), got["iterations"].tolist(), got["best"]))
    assert got["status"][0] == 2 and got["status"][1] == 3 and got["status"][2] in (2, 3) and got["status"][44] in (2, 3)
    assert (got["status"] == 1).any() and len(set(got["iterations"][got["status"] == 1].tolist())) >= 2, "the rows were meant to stop at different iterations"
    assert (R.bits(got["poses"][3]) == R.bits(got["poses"][45])).all() and (R.bits(got["info"][3]) == R.bits(got["info"][45])).all()
    assert got["best"] == B.pick_best(got["info"]) and got["status"][got["best"]] in (0, 1)
    # with the gate every failing start has too few pairs
    got = assert_rows_are_register(pkg, h, starts[:6], "mixed, gated", max_iters=3)
    assert (got["status"][:3] == 2).all()
    # no row eligible: best is -1 (and *best may be NULL)
    h.set_scan(np.full(1081, 1000.0, np.float32))
    got = assert_rows_are_register(pkg, h, starts_of(3), "rejected ranges")
    assert (got["status"] == 2).all() and got["best"] == -1 and (R.bits(got["poses"]) == R.bits(starts_of(3))).all()
    poses, info = np.zeros((3, 3), np.float32), np.zeros((3, 8), np.float32)
    o = options(pkg, h)
    assert h.L.pfslam_register_batch(h._h, starts_of(3).ctypes.data_as(C.c_void_p), 3, C.byref(o), poses.ctypes.data_as(C.c_void_p),
                                     info.ctypes.data_as(C.c_void_p), None) == 0
    assert (R.bits(info) == R.bits(got["info"])).all()
    h.close()


# ---- 4. its buffers and the map ----------------------------------------------------------------------------------------------------------------
def test_buffers_grow_from_4_rows_to_300_and_a_replaced_map_is_the_one_read(pkg, world):
    h = pkg.PfSlam(64, kd_capacity=1 << 16)
    h.set_map(world["p4000"])
    h.set_scan(world["scan"])
    assert_rows_are_register(pkg, h, starts_of(4), "4 rows", max_iters=2)
    assert_rows_are_register(pkg, h, starts_of(300, seed=5), "300 rows", max_iters=2)
    small = assert_rows_are_register(pkg, h, starts_of(4), "4 rows again", max_iters=2)      # (the larger buffers serve a smaller call)
    h.set_map(world["np300"])
    other = assert_rows_are_register(pkg, h, starts_of(4), "replaced map", max_iters=2, max_dist=0.0)
    assert not (R.bits(other["poses"]) == R.bits(small["poses"])).all()
    want = B.register_batch(world["np300"], world["scan"], starts_of(4), max_iters=2, max_dist=0.0)
    assert B.same_rows(other, want) is None, B.same_rows(other, want)
    h.close()


# ---- 5. read-only --------------------------------------------------------------------------------------------------------------------------------
def test_register_batch_behind_frames_in_flight_reads_and_changes_nothing(pkg):
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
        if f in (4, 7):                                  # a frame is in flight (default lag): register_batch books it first
            off = np.array([[0, 0, 0], [0.1, 0, 0], [0, -0.1, 0.02], [-0.05, 0.05, -0.02]], np.float32)
            first = h.register_batch(off, max_iters=1)   # (books the frame: h.pose below is the frame's)
            assert B.same_rows(first, rows_of_register(pkg, h, off, max_iters=1)) is None
            starts = (h.pose[None, :].astype(np.float64) + off).astype(np.float32)
            for opts in (dict(max_iters=4), dict(match=0, select=0, update=0, max_iters=3)):
                seen.append(assert_rows_are_register(pkg, h, starts, "frame %d" % f, **opts))
            want = B.register_batch(h.map(), scan, starts[:2], max_iters=2)                 # 2 x 2 row-iterations per frame
            got = h.register_batch(starts[:2], max_iters=2)
            assert B.same_rows(got, want) is None, (f, B.same_rows(got, want))
            assert (R.bits(h.pose) == R.bits(twin.pose)).all()
            assert buffers(h) == buffers(twin), "buffers 11 / 12 after frame %d" % f
            assert h.check_cells()["violations"] == 0
    assert (seen[0]["iterations"] >= 1).all()
    assert (R.bits(h.pose) == R.bits(twin.pose)).all()
    ph, pt = h.particles(), twin.particles()
    for fld in ("x", "y", "theta", "w"):
        assert (R.bits(ph[fld]) == R.bits(pt[fld])).all(), fld
    assert h.map().tobytes() == twin.map().tobytes()
    assert buffers(h) == buffers(twin)
    assert h.check_cells()["violations"] == 0 and twin.check_cells()["violations"] == 0
    h.close(); twin.close()


def test_the_first_call_behind_a_frame_in_flight_books_that_frame(pkg):
    """register_batch as the FIRST call after step: the rows are the registrations against the map and scan of the frame just enqueued,
    and the next frame equals that of a handle that never called it."""
    n = 1000
    _, frames = pkg.synth.corridor_sequence(6, seed=5)
    h, twin = pkg.PfSlam(n, kd_capacity=1 << 16), pkg.PfSlam(n, kd_capacity=1 << 16)
    starts = None
    for f, (_, scan) in enumerate(frames, start=1):
        h.step(f, scan)
        twin.step(f, scan)
        if f == 4:
            starts = (np.array(twin.pose, np.float64)[None, :] + np.array([[0, 0, 0], [0.1, -0.1, 0.01]])).astype(np.float32)   # (twin.pose books twin's frame)
            got = h.register_batch(starts, max_iters=2)                                                                  # h's frame is still in flight
            want = B.register_batch(twin.map(), scan, starts, max_iters=2)
            assert B.same_rows(got, want) is None, B.same_rows(got, want)
    assert starts is not None and (R.bits(h.pose) == R.bits(twin.pose)).all() and h.map().tobytes() == twin.map().tobytes()
    h.close(); twin.close()


# ---- 6. wrappers -----------------------------------------------------------------------------------------------------------------------------------
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
    starts = (np.array(one.pose, np.float64)[None, :] + (starts_of(5).astype(np.float64) - START)).astype(np.float32)
    for opts in (dict(max_iters=4), dict(match=0, select=0, update=0, max_iters=3)):
        want = one.register_batch(starts, **opts)
        assert (want["iterations"] >= 1).any()
        for r, e in enumerate(v.engs):
            diff = B.same_rows(e.register_batch(starts, **opts), want)
            assert diff is None, "rank %d of %d: %s" % (r, nranks, diff)
    assert B.same_rows(want, rows_of_register(pkg, one, starts, **opts)) is None
    v.close(); one.close()


def test_sharded_wrapper_passes_register_batch_through(pkg):
    torch = pytest.importorskip("torch")
    sharded = importlib.import_module("gpu-icp-slam_amd.sharded")
    a = pkg.PfSlam(500, kd_capacity=1 << 16)
    s = sharded.ShardedSlam(pkg, 500, 0, 1, device=0, torch=torch, kd_capacity=1 << 16)
    _, frames = pkg.synth.corridor_sequence(4, seed=7)
    for f, (_, scan) in enumerate(frames, start=1):
        a.step(f, scan)
        s.step(f, scan)
    issued = s.collectives
    starts = (np.array(a.pose, np.float64)[None, :] + (starts_of(3).astype(np.float64) - START)).astype(np.float32)
    assert B.same_rows(s.register_batch(starts, max_iters=4), a.register_batch(starts, max_iters=4)) is None and s.collectives == issued
    a.close(); s.eng.close()


def test_replay_binary_with_multistart_3_prints_the_handle_s_batch(tmp_path, pkg):
    """pfslamRegisterBatch (host/kernel.h) through `pfslam_replay ... multistart=3`: one line per frame with the row the library picks and
    that row's pose, whose float bits are the C-ABI's."""
    build_host(pkg)
    _, frames = pkg.synth.corridor_sequence(6, seed=5)
    scene = tmp_path / "scene.txt"
    scene.write_text(SCENE_TXT)
    scans = np.stack([np.zeros(1081, np.float32)] + [s for _, s in frames])  # scans[0] is never used (frame starts at 1)
    lidar = tmp_path / "lidar.f32"
    scans.astype(np.float32).tofile(str(lidar))
    env = dict(os.environ, PFSLAM_PARTICLES="300", PFSLAM_KD_CAPACITY=str(1 << 16))
    out = subprocess.check_output([os.path.join(HOST, "pfslam_replay"), str(scene), str(lidar), "multistart=3"], env=env).decode()
    lines = [l for l in out.splitlines() if l.startswith("multistart ")]
    assert len(lines) == len(frames)
    h = pkg.PfSlam(300, kd_capacity=1 << 16)
    off = np.float32([-0.1, 0.0, 0.1])
    picked = 0
    for f, ((_, scan), line) in enumerate(zip(frames, lines), start=1):
        h.step(f, scan)
        p = h.pose
        starts = np.array([[p[0] + off[a], p[1] + off[b], p[2]] for a in range(3) for b in range(3)], np.float32)   # row-major in dx
        got = h.register_batch(starts, max_iters=3)
        tok = line.split()
        assert tok[1] == str(f) and tok[2] == "best" and int(tok[3]) == got["best"], line
        if got["best"] >= 0:
            picked += 1
            assert tok[4] == "pose" and tok[8] == "bits" and len(tok) == 12, line
            assert [int(v, 16) for v in tok[9:12]] == got["poses"][got["best"]].view(np.uint32).tolist(), line
        else:
            assert len(tok) == 4, line
    assert picked >= 3
    h.close()
    out = subprocess.check_output([os.path.join(HOST, "pfslam_replay"), str(scene), str(lidar)], env=env).decode()
    assert not [l for l in out.splitlines() if l.startswith("multistart ")]


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_leave_the_outputs_and_the_handle_goes_on(pkg, world):
    h = pkg.PfSlam(64, kd_capacity=1 << 16)
    with pytest.raises(pkg.PfSlamError, match="pfslam_register_batch: no map loaded"):
        h.register_batch(starts_of(2))
    h.set_map(world["p4000"])
    h.set_scan(world["scan"])
    for bad, cause in ((dict(max_iters=0), "max_iters"), (dict(max_iters=65), "max_iters"), (dict(match=2), "match"), (dict(select=-1), "select"),
                       (dict(update=2), "update"), (dict(max_dist=float("nan")), "max_dist"), (dict(eps_xy=-1.0), "eps"),
                       (dict(eps_theta=float("inf")), "eps")):
        with pytest.raises(pkg.PfSlamError, match="pfslam_register_batch: .*%s" % cause):
            h.register_batch(starts_of(2), **bad)
    with pytest.raises(pkg.PfSlamError, match="pfslam_register_batch: m must be 1 .. 4096"):
        h.register_batch(np.zeros((0, 3), np.float32))
    with pytest.raises(pkg.PfSlamError, match="pfslam_register_batch: m must be 1 .. 4096"):
        h.register_batch(np.zeros((4097, 3), np.float32))

    # through the C-ABI: every refusal returns non-zero and writes no output
    m = 3
    starts = starts_of(m)
    poses, info, best = np.full((m, 3), 7.5, np.float32), np.full((m, 8), 7.5, np.float32), C.c_int(77)
    good = options(pkg, h, max_iters=2)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(st=starts, rows=m, o=good, p=poses, i=info, handle=None):
        return h.L.pfslam_register_batch(h._h if handle is None else handle, None if st is None else vp(st), rows, None if o is None else C.byref(o),
                                         None if p is None else vp(p), None if i is None else vp(i), C.byref(best))

    def untouched():
        return (poses == 7.5).all() and (info == 7.5).all() and best.value == 77

    for kw, cause in ((dict(st=None), "bad argument"), (dict(o=None), "bad argument"), (dict(p=None), "bad argument"), (dict(i=None), "bad argument"),
                      (dict(rows=0), "m must be"), (dict(rows=-1), "m must be"), (dict(rows=4097), "m must be"),
                      (dict(o=options(pkg, h, match=7)), "match"), (dict(o=options(pkg, h, max_iters=65)), "max_iters"),
                      (dict(o=options(pkg, h, eps_xy=float("nan"))), "eps")):
        assert call(**kw) != 0, kw
        assert cause in h.L.pfslam_last_error().decode(), (kw, h.L.pfslam_last_error())
        assert untouched(), "an output was written: %r" % (kw,)
    empty = pkg.PfSlam(64, kd_capacity=1 << 16)
    assert h.L.pfslam_register_batch(empty._h, vp(starts), m, C.byref(good), vp(poses), vp(info), C.byref(best)) != 0
    assert "no map loaded" in h.L.pfslam_last_error().decode() and untouched()
    empty.close()
    with pytest.raises(pkg.PfSlamError, match="at most 4096 beams"):   # (no handle can hold more: the refusal of n_beams > 4096 cannot
        pkg.PfSlam(64, n_beams=4097, kd_capacity=1 << 16)             #  be reached through pfslam_create)
    assert call() == 0 and not untouched() and best.value == B.pick_best(info)
    assert_rows_are_register(pkg, h, starts, "after the refusals", max_iters=2)
    h.close()
