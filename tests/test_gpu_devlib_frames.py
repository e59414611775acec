"""Whole frames in device-library mode (pfslam_set_trig(h, 1): the device library's cosf / sinf / erfcinvf, the mode in which the product's
kernels equal the reference's own kernel.cu compiled for gfx950).

The CPU oracle cannot follow that mode, so the oracle here is tests/stage_shadow.py: a second handle driven STAGE BY STAGE through the
public entry points, each of which tests/test_gpu_ref_kernels.py pins to the reference's kernel with zero mismatches.  The chain:

  1. the composition is proven in the default mode, where the CPU oracle exists: shadow == oracle == pfslam_step, every frame;
  2. pfslam_step / pfslam_step_grid / the sharded frame against the shadow, both in device-library mode: small counts from an empty
     map, the 100 000-point world of test_gpu_frame.py with frames in flight, one stream / events / lag 0 / lag 2, a mode switch in flight;
  3. the frame's own scan-match launch (k_score_kd_cells as the frame launches it, k_reduce_groups) and its ICP arrays (k_icp_fused)
     against the reference's kernEvaluateParticlesKD / kernGetWallsKD / findCorrespondenceKD;
  4. the ICP stage (k_icp_correspond) in device-library mode against the same two kernels;
  5. tests/fuzz_step.py --devlib: the differential fuzz with the shadow as comparator.

Everything is bit for bit; there is no tolerance anywhere in this file.

What a run on one MI355X compares (every line is also printed by report() of test_gpu_ref_kernels.py), differing: 0 throughout:
  composition, default mode      6 cases, 86 frames, shadow == oracle == frame
  frames from an empty map       10 cases, 144 frames, 15.8 M occupancy-cell indices, two 1600 x 1600 grids
  100 k world, frames in flight  n 20 000 x 30 and n 100 000 x 24 frames, looked at once and every third frame; n 128 x 2000 frames (200 looks)
  one stream / events / lags     5 runs of n 100 000 x 12 frames, cell-row bookkeeping equal where test_gpu_frame.py asserts it
  sharded                        (1000, world 2), (1001, world 3) x 12 frames; n 20 000, world 2, x 12 round-5 frames
  mode switch in flight          n 20 000 x 18 frames, modes 0 / 1 / 0
  frame's own scan-match launch  310 000 scores against kernEvaluateParticlesKD (70 000 against orc_score_kd for the read-back's calibration);
                                 98 371 words of k_icp_fused's arrays against kernGetWallsKD / findCorrespondenceKD
  ICP stage                      3 x 8 648 words
  fuzz --devlib                  2 x 60 s: about 5 000 cases, 43 000 frames
Mutations this file was checked against (each once, on a scratch copy): the frame launching the specification's scan-match instantiation in
device-library mode fails nine tests here (frames in flight and the reference-kernel comparison among them); k_wall_runs given trig = 0 in
device-library mode fails the 2000-frame run in its frame 431 (k_walls<0>'s own trig argument cannot be reached: round-5 frames need a planar
map, which takes the k_wall_runs branch); the shadow calling icp before measurement_update fails all five KD cases of the composition test."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from ref_kernels import PARTICLE_COUNT, LIDAR_SIZE, ptr, i32, ivec2, vec3, patch
from stage_shadow import StageShadow
from test_gpu_frame import BOOK, CHECK, run_frames, world          # noqa: F401  (world: a fixture)
from test_gpu_ref_kernels import report, rk                        # noqa: F401  (rk: a fixture)
from test_gpu_sharded import _VirtualRanks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("x", "y", "theta", "w")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def look(e):
    """one row of run_frames: trace + pose bits"""
    t = e.trace()
    return [t["best"], t["resampled"], t["n_wall"], t["n_free"], t["n_insert"], t["kd_size"]] + bits(e.pose).tolist()


def same_trace(a, b):
    a, b = dict(a), dict(b)
    return bits(a.pop("neff")) == bits(b.pop("neff")) and a == b


def assert_same_particles(got, want, what=""):
    for fld in FIELDS:
        bad = int((bits(got[fld]) != bits(want[fld])).sum())
        assert bad == 0, "%s: %d of %d particles differ in %s" % (what, bad, len(want), fld)


def map_bytes(e):
    return (e.map() if hasattr(e, "map") else e.tree()).tobytes()


@contextlib.contextmanager
def environ(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def compare_per_frame(engines, frames, grid=False, first=1):
    """Step `frames` through every engine of `engines` (the first is the one under test); after every frame all must show the same trace,
    pose bits and occupancy-cell lists; at the end the same particles and map.  Returns (frames, cells, particles) compared."""
    n_cells = 0
    ref = engines[0]
    for f, scan in enumerate(frames, start=first):
        for e in engines:
            (e.step_grid if grid else e.step)(f, scan)
        t = ref.trace()
        for k, e in enumerate(engines[1:], start=1):
            assert same_trace(e.trace(), t), "frame %d, engine %d: trace %s vs %s" % (f, k, e.trace(), t)
            assert (bits(e.pose) == bits(ref.pose)).all(), "frame %d, engine %d: pose %s vs %s" % (f, k, e.pose, ref.pose)
            if not grid:
                for which in (0, 1):
                    a, b = e.cells(which), ref.cells(which)
                    assert len(a) == len(b) and (a == b).all(), "frame %d, engine %d: %s cells differ" % (f, k, ("wall", "free")[which])
                    n_cells += len(b)
    want = ref.particles()
    for k, e in enumerate(engines[1:], start=1):
        assert_same_particles(e.particles(), want, "engine %d" % k)
        if grid:
            ga = e.grid if not callable(e.grid) else e.grid()
            gb = ref.grid if not callable(ref.grid) else ref.grid()
            assert (ga == gb).all(), "engine %d: occupancy grids differ in %d cells" % (k, (ga != gb).sum())
            n_cells += gb.size
        else:
            assert map_bytes(e) == map_bytes(ref), "engine %d: maps differ" % k
    return len(frames), n_cells, len(want)


def corridor(pkg, n_frames, nb=LIDAR_SIZE):
    _, seq = pkg.synth.corridor_sequence(n_frames, seed=5)
    return [np.ascontiguousarray(s[:nb], np.float32) for _, s in seq]


# ---- 1. the composition, proven where the CPU oracle exists ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant,bug,grid,n_frames", [(50, 0, 0, False, 14), (1000, 0, 0, False, 14), (300, 3, 0, False, 14),
                                                         (50, 0, 1, False, 14), (1000, 0, 1, False, 14), (50, 0, 0, True, 16)])
def test_stage_composition_equals_oracle_and_frame_in_default_mode(pkg, monkeypatch, n, variant, bug, grid, n_frames):
    """pfslam_set_trig(0): the frame composed of stage calls == the CPU oracle's orc_slam_step == pfslam_step, every frame (trace, pose
    bits, wall and free cells), particles and map bytes at the end; the frame-5 re-balance is inside.  This licenses the shadow as an
    oracle -- and checks GPU stages composed == GPU frame directly rather than through the oracle."""
    monkeypatch.setenv("ORC_THREADS", "16")
    frames = corridor(pkg, n_frames)
    kw = dict(kd_capacity=1 << 16, free_upload_bug=bug)
    o = O.Slam(n, **kw)
    s = StageShadow(n, pkg=pkg, variant=variant or None, **kw)
    h = pkg.PfSlam(n, **kw)
    if variant:
        h.set_variant(variant)
    got = compare_per_frame([o, s, h], frames, grid=grid)
    if not grid:
        assert o.kd_size > 100
        if variant:
            assert h.frame_mode()["round5_frame"] and h.cell_stats()["rows"] > 0
    report("default mode, n %d variant %d free_upload_bug %d %s: shadow == oracle == frame over %d frames, %d cells, %d particles" % ((n, variant, bug, "2-D" if grid else "KD") + got))
    for e in (o, s, h):
        e.close()


# ---- 2a. device-library frames from an empty map ----------------------------------------------------------------------------------------
SMALL = [dict(n=50), dict(n=1000), dict(n=1025), dict(n=300, variant=3), dict(n=3000, variant=3), dict(n=1000, bug=1), dict(n=300, variant=3, bug=1),
         dict(n=300, nb=721, scale=30.0, res=0.05), dict(n=50, grid=True), dict(n=10000, grid=True)]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "-".join("%s%s" % kv for kv in sorted(c.items())))
def test_devlib_frames_from_an_empty_map_equal_the_shadow(pkg, case):
    """pfslam_step / pfslam_step_grid against the shadow, both with pfslam_set_trig(1), frame by frame."""
    n, variant, bug, grid = case["n"], case.get("variant", 0), case.get("bug", 0), case.get("grid", False)
    nb = case.get("nb", LIDAR_SIZE)
    frames = corridor(pkg, 16 if grid else 14, nb)
    kw = dict(kd_capacity=1 << 16, free_upload_bug=bug, n_beams=nb)
    if "scale" in case:
        kw.update(map_scale=(case["scale"],) * 2, map_res=(case["res"],) * 2)
    s = StageShadow(n, pkg=pkg, trig=1, variant=variant or None, **kw)
    h = pkg.PfSlam(n, **kw)
    h.set_trig(1)
    if variant:
        h.set_variant(variant)
    got = compare_per_frame([s, h], frames, grid=grid)
    if not grid:
        assert h.kd_size > 100
        if variant:
            assert h.frame_mode()["round5_frame"] and h.cell_stats()["rows"] > 0
    report("device library, %s: frame == shadow over %d frames, %d cells, %d particles; differing: 0" % ((case,) + got))
    s.close(); h.close()


# ---- the shadow on the 100 000-point world (stepped once per configuration, kept for the tests below) -----------------------------------
_SHADOWS = {}


def shadow_on_world(pkg, tree, scans, n, n_frames, switch=None, snaps=()):
    """The shadow through run_frames' recipe (map, five dispersions, frames 6 ...) in device-library mode (switch: {frame index: mode},
    default {0: 1}): a row per frame, particles and map bytes behind the frames of `snaps` and behind the last."""
    switch = switch or {0: 1}
    key = (n, n_frames, tuple(sorted(switch.items())), tuple(snaps))
    if key in _SHADOWS:
        return _SHADOWS[key]
    s = StageShadow(n, pkg=pkg, kd_capacity=len(tree) + (1 << 18), trig=switch[0])   # (the five dispersions are in the first mode too)
    s.set_map(tree)
    for f in range(1, 6):
        s.motion_update(f)
    rows, snap = [], {}
    for i in range(n_frames):
        if i and i in switch:
            s.set_trig(switch[i])
        s.step(6 + i, scans[i])
        rows.append(look(s))
        if i + 1 in snaps or i + 1 == n_frames:
            snap[i + 1] = (s.particles().copy(), s.map().tobytes())
    s.close()
    _SHADOWS[key] = (rows, snap)
    return _SHADOWS[key]


def assert_run_equals_shadow(run, shadow, n_frames, look_every, what):
    rows, snap = shadow
    looked = [i for i in range(n_frames) if look_every and (i + 1) % look_every == 0] + [n_frames - 1]
    assert len(run[0]) == len(looked)
    for got, i in zip(run[0], looked):
        assert got == rows[i], "%s: frame %d: %s vs the shadow's %s" % (what, 6 + i, got, rows[i])
    assert_same_particles(run[1], snap[n_frames][0], what)
    assert run[2] == snap[n_frames][1], "%s: maps differ" % what
    assert run[4]["violations"] == 0, run[4]
    return len(looked)


def devlib(h):
    h.set_trig(1)


def seen(h):
    return h.frame_mode(), h.cell_stats()


# ---- 2b. frames in flight on the 100 000-point world ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_frames", [(20000, 30), (100000, 24)])
def test_devlib_frames_in_flight_equal_the_shadow(pkg, world, n, n_frames):
    """Round-5 frames on persistent cell rows that live through inserts and extensions, compared only at the end (frames really in flight)
    and, in a second run, every third frame (a getter drains the pipeline)."""
    tree, scans = world
    sh = shadow_on_world(pkg, tree, scans, n, n_frames, snaps=(12,))
    rows = sh[0]
    assert sum(r[1] for r in rows) >= 2, "fewer than 2 resamples"
    assert rows[-1][5] > len(tree) and sum(r[4] for r in rows) > 0, "the map did not grow"
    for every in (0, 3):
        run = run_frames(pkg, tree, scans[:n_frames], n, serial=False, look_every=every, prepare=devlib, inspect=seen)
        looked = assert_run_equals_shadow(run, sh, n_frames, every, "n %d, look every %d" % (n, every))
        mode, st = run[5]
        assert mode["round5_frame"] and st["rows"] > 0 and st["flags"] == 0 and run[3]["flags"] == 0
        report("device library, 100 k world, n %d x %d frames, looked at %d: frame == shadow in %d rows, %d particles, %d map bytes; differing: 0 (cell rows %d)"
               % (n, n_frames, looked, looked, n, len(run[2]), st["rows"]))


def test_devlib_long_run_places_every_wall_where_the_shadow_does(pkg, world):
    """The two modes place a wall's end point in different occupancy cells about once in 400 frames (measured: k_wall_runs given the
    specification's end points in device-library mode first disagrees with k_get_walls' list in frame 431 of this run -- the frames of
    the cases above, some 400 round-5 frames in all, do not reach such a beam).  2000 round-5 frames at n = 128 with cell rows, the 30
    scans of the world in turn, looked at every tenth frame: the insert chain's wall list (k_wall_runs, k_walls_rank_traverse, k_walls),
    the free-cell chain's (k_get_walls) and the shadow's stage (k_get_walls alone) must name the same cells throughout -- a disagreement
    is a loud pfslam_step error or another map."""
    tree, scans = world
    n, n_frames = 128, 2000
    cap = len(tree) + (1 << 19)
    s = StageShadow(n, pkg=pkg, kd_capacity=cap, trig=1, variant=3)
    h = pkg.PfSlam(n, kd_capacity=cap)
    h.set_trig(1)
    h.set_variant(3)
    for e in (s, h):
        e.set_map(tree)
        for f in range(1, 6):
            e.motion_update(f)
    looks = 0
    for i in range(n_frames):
        s.step(6 + i, scans[i % len(scans)])
        h.step(6 + i, scans[i % len(scans)])
        if (i + 1) % 10 == 0:
            assert look(h) == look(s), "frame %d: %s vs the shadow's %s" % (6 + i, look(h), look(s))
            looks += 1
        if (i + 1) % 500 == 0:
            assert h.map().tobytes() == s.map().tobytes(), "maps differ by frame %d" % (6 + i)
    assert h.frame_mode()["round5_frame"] and h.cell_stats()["rows"] > 0 and h.check_cells()["violations"] == 0
    assert_same_particles(h.particles(), s.particles(), "long run")
    report("device library, long run, n %d x %d round-5 frames: frame == shadow at %d looks, %d map nodes; differing: 0" % (n, n_frames, looks, h.kd_size))
    h.close(); s.close()


# ---- 2c. one stream, events, lag 0 / 2 ---------------------------------------------------------------------------------------------------
def test_devlib_one_stream_events_and_lags_equal_the_shadow(pkg, world):
    tree, scans = world
    n, n_frames = 100000, 12
    rows, snap = shadow_on_world(pkg, tree, scans, n, 24, snaps=(12,))
    sh = (rows[:n_frames], snap)
    kw = dict(look_every=0, inspect=seen)
    base = run_frames(pkg, tree, scans[:n_frames], n, serial=False, prepare=devlib, **kw)
    serial = run_frames(pkg, tree, scans[:n_frames], n, serial=True, prepare=devlib, **kw)
    events = run_frames(pkg, tree, scans[:n_frames], n, serial=False, prepare=devlib, env={"PFSLAM_GATES": "0"}, **kw)
    lag0 = run_frames(pkg, tree, scans[:n_frames], n, serial=False, prepare=lambda h: (h.set_trig(1), h.set_lag(0)), **kw)
    lag2 = run_frames(pkg, tree, scans[:n_frames], n, serial=False, prepare=lambda h: (h.set_trig(1), h.set_lag(2)), **kw)
    for name, run in (("four streams", base), ("one stream", serial), ("events", events), ("lag 0", lag0), ("lag 2", lag2)):
        assert_run_equals_shadow(run, sh, n_frames, 0, name)
        assert run[5][0]["round5_frame"] and run[5][1]["rows"] > 0 and run[3]["flags"] == 0, name
    assert serial[5][0]["serial"] and not base[5][0]["serial"] and not events[5][0]["gates"]
    # the cell rows' bookkeeping, wherever test_gpu_frame.py asserts it in the default mode: one stream vs four, gates vs events
    assert base[3] == serial[3], (base[3], serial[3])
    assert {k: base[4][k] for k in CHECK} == {k: serial[4][k] for k in CHECK}, (base[4], serial[4])
    assert base[3] == events[3], (base[3], events[3])
    assert base[3]["cells"] > 1000
    report("device library, n %d x %d frames: four streams / one stream / events / lag 0 / lag 2 == shadow (5 runs, %d particles each); bookkeeping equal: %s"
           % (n, n_frames, n, base[3]))


# ---- 2d. the sharded frame ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,world_size", [(1000, 2), (1001, 3)])
def test_devlib_sharded_frames_from_an_empty_map_equal_the_single_handle(pkg, n, world_size):
    torch = pytest.importorskip("torch")
    frames = corridor(pkg, 12)
    v = _VirtualRanks(pkg, torch, n, world_size, kd_capacity=1 << 16)
    one = pkg.PfSlam(n, kd_capacity=1 << 16)
    s = StageShadow(n, pkg=pkg, trig=1, kd_capacity=1 << 16)
    one.set_trig(1)
    for e in v.engs:
        e.set_trig(1)
    for f, scan in enumerate(frames, start=1):
        one.step(f, scan); v.step(f, scan); s.step(f, scan)
        t = one.trace()
        assert same_trace(v.trace(), t) and same_trace(s.trace(), t), (f, v.trace(), s.trace(), t)   # (every rank's: _VirtualRanks checks them against rank 0's)
        assert (bits(v.pose) == bits(one.pose)).all() and (bits(s.pose) == bits(one.pose)).all(), f
    want = one.particles()
    got = [e.particles() for e in v.engs]
    assert_same_particles({fld: np.concatenate([g[fld] for g in got]) for fld in FIELDS}, want, "ranks")
    assert_same_particles(s.particles(), want, "shadow")
    for e in v.engs:
        assert e.map().tobytes() == one.map().tobytes()
    assert s.map().tobytes() == one.map().tobytes() and one.kd_size > 100
    report("device library, sharded %d / world %d: every rank == single handle == shadow over %d frames, %d particles; differing: 0" % (n, world_size, len(frames), n))
    v.close(); one.close(); s.close()


def test_devlib_sharded_round5_frames_equal_the_single_handle(pkg, world):
    """n = 20 000 on two virtual ranks, on the 100 000-point world: the sharded round-5 frame with the device library's trigonometry on every rank."""
    torch = pytest.importorskip("torch")
    tree, scans = world
    n, n_frames = 20000, 12
    rows, _ = shadow_on_world(pkg, tree, scans, n, 30, snaps=(12,))
    one = run_frames(pkg, tree, scans[:n_frames], n, serial=False, look_every=1, prepare=devlib)
    v = _VirtualRanks(pkg, torch, n, 2, kd_capacity=len(tree) + (1 << 18))
    for e in v.engs:
        e.set_map(tree)
        e.set_trig(1)
        for f in range(1, 6):
            e.motion_update(f)
    v2_frames = 0
    for i in range(n_frames):
        v.step(6 + i, scans[i])
        got = look(v)
        assert got == one[0][i] == rows[i], "frame %d: ranks %s, single handle %s, shadow %s" % (6 + i, got, one[0][i], rows[i])
        v2_frames += all(e.frame_mode()["round5_frame"] for e in v.engs)
    # (a shard whose cloud has grown too wide for its size goes back to the staged chain for a frame: test_gpu_sharded.py)
    assert v2_frames >= n_frames - 3, v2_frames
    for e in v.engs:
        e.synchronize()
        assert e.map().tobytes() == one[2]
    parts = [e.particles() for e in v.engs]
    assert_same_particles({fld: np.concatenate([g[fld] for g in parts]) for fld in FIELDS}, one[1], "ranks")
    report("device library, sharded round-5 frames, n %d / world 2 x %d frames: every rank == single handle == shadow; differing: 0" % (n, n_frames))
    v.close()


# ---- 2e. the mode switched in flight ------------------------------------------------------------------------------------------------------
def test_mode_switch_in_flight_equals_a_shadow_switched_at_the_same_frames(pkg, world):
    """6 frames in the default mode, 6 with the device library, 6 in the default mode again, at n = 20 000: pfslam_set_trig settles the
    frames in flight; the cell rows made in one mode are used in the other -- legitimately, rows depend on the map only -- and this is
    the test that says so."""
    tree, scans = world
    n, n_frames, switch = 20000, 18, {0: 0, 6: 1, 12: 0}
    rows, snap = shadow_on_world(pkg, tree, scans, n, n_frames, switch=switch)
    plain, _ = shadow_on_world(pkg, tree, scans, n, 30, snaps=(12,))
    assert rows != plain[:n_frames], "the switch changed nothing: the case does not tell the modes apart"
    h = pkg.PfSlam(n, kd_capacity=len(tree) + (1 << 18))
    h.set_map(tree)
    h.set_trig(switch[0])
    for f in range(1, 6):
        h.motion_update(f)
    wipes = None
    for i in range(n_frames):
        if i and i in switch:
            h.set_trig(switch[i])
        h.step(6 + i, scans[i])
        if (i + 1) % 3 == 0:   # (in between, frames are in flight)
            assert look(h) == rows[i], "frame %d: %s vs the shadow's %s" % (6 + i, look(h), rows[i])
            st = h.cell_stats()
            assert st["rows"] > 0 and st["flags"] == 0
            assert wipes is None or st["wipes"] == wipes, "the rows were wiped at a mode switch"
            wipes = st["wipes"]
    h.synchronize()
    assert h.frame_mode()["round5_frame"] and h.check_cells()["violations"] == 0
    assert_same_particles(h.particles(), snap[n_frames][0], "switched")
    assert h.map().tobytes() == snap[n_frames][1]
    report("mode switch in flight, n %d x %d frames (modes %s): frame == shadow at %d looks, %d particles; differing: 0" % (n, n_frames, switch, n_frames // 3, n))
    h.close()


# ---- 3. the frame's own scan-match launch and ICP arrays against the reference's kernels -------------------------------------------------
def d2h(rk, h, which, dtype, shape):
    addr, nbytes = h.device_ptr(which)
    out = np.empty(shape, dtype)
    assert out.nbytes <= nbytes
    assert rk.L.ref_d2h(O.P(out), C.c_void_p(addr), out.nbytes) == 0
    return out


def ref_scores(rk, tree, p, scan):
    """kernEvaluateParticlesKD on every particle of p, in batches of PARTICLE_COUNT (compiled into the reference's kernel)"""
    N = PARTICLE_COUNT
    assert len(p) % N == 0
    tb, t0 = rk.tree_dev(tree)
    ds = rk.dev(np.ascontiguousarray(scan, np.float32))
    out = np.empty(len(p), np.float32)
    for s in range(0, len(p), N):
        dp, df = rk.dev(np.ascontiguousarray(p[s:s + N])), rk.zeros(N, np.float32)
        rk.launch("kernEvaluateParticlesKD", N, 128, ptr(0), ivec2(1600, 1600), patch(), ptr(dp), vec3(0, 0, 0), ptr(ds), ptr(df), ptr(t0), i32(len(tree)))
        out[s:s + N] = df.get()
        dp.free(); df.free()
    tb.free(); ds.free()
    return out


def ref_icp_arrays(rk, tree, scan, pose):
    """kernGetWallsKD's targets at `pose` and findCorrespondenceKD's matched nodes of those targets"""
    nb = len(scan)
    tb, t0 = rk.tree_dev(tree)
    ds, tar, cor = rk.dev(np.ascontiguousarray(scan, np.float32)), rk.zeros((nb, 4), np.float32), rk.zeros((nb, 4), np.float32)
    rk.launch("kernGetWallsKD", nb, 128, ptr(ds), vec3(float(pose[0]), float(pose[1]), float(pose[2])), ptr(tar), patch())
    rk.launch("findCorrespondenceKD", nb, 128, i32(nb), ptr(cor), ptr(tar), ptr(t0))
    out = tar.get(), cor.get()
    for b in (tb, ds, tar, cor):
        b.free()
    return out


def frames_against_reference_kernel(pkg, rk, tree, scans, n, variant, trig, pick):
    """Product and shadow in lockstep; for every frame `pick` chooses: the map before the frame, ONE frame, synchronize, the frame's score
    buffer (pfslam_device_ptr 1, particle order) against the scores of `tree before` x `scan` x the frame's dispersed particles (the
    shadow's, behind its motion_update): the reference kernel's in device-library mode, the CPU oracle's in the default mode (the
    calibration of the read-back).  Behind the frame the ICP arrays k_icp_fused left (buffers 11 / 12) against the reference's kernels too."""
    h = pkg.PfSlam(n, kd_capacity=len(tree) + (1 << 18))
    s = StageShadow(n, pkg=pkg, kd_capacity=len(tree) + (1 << 18), trig=trig, variant=variant or None)
    h.set_trig(trig)
    if variant:
        h.set_variant(variant)
    for e in (h, s):
        e.set_map(tree)
        for f in range(1, 6):
            e.motion_update(f)
    scores = diff = icp_words = icp_diff = 0
    kinds, after_resample = [], False
    for i, scan in enumerate(scans):
        kind = pick(i, after_resample, len(scans))
        if kind:
            before, pose = h.map().copy(), np.asarray(h.pose, np.float32).copy()
        s.step(6 + i, scan, keep_dispersed=bool(kind))
        h.step(6 + i, scan)
        if kind:
            h.synchronize()
            got = d2h(rk, h, 1, np.float32, n)
            assert h.frame_mode()["round5_frame"], "frame %d did not run as a round-5 frame" % (6 + i)
            want = ref_scores(rk, before, s.dispersed, scan) if trig else O.score_kd(before, s.dispersed, scan, threads=16)
            bad = int((bits(got) != bits(want)).sum())
            scores += n; diff += bad
            assert bad == 0, "frame %d (%s): %d of %d scores of the frame's own scan-match launch differ" % (6 + i, kind, bad, n)
            if trig:
                tar, cor = ref_icp_arrays(rk, before, scan, pose)
                gt, gc = d2h(rk, h, 11, np.float32, (len(scan), 4)), d2h(rk, h, 12, np.float32, (len(scan), 4))
                bad = int((bits(gt) != bits(tar)).sum() + (bits(gc[:, :3]) != bits(cor[:, :3])).sum())
                icp_words += 7 * len(scan); icp_diff += bad
                assert bad == 0, "frame %d: %d words of the ICP targets / correspondences differ from kernGetWallsKD / findCorrespondenceKD" % (6 + i, bad)
            kinds.append(kind)
        assert look(h) == look(s), "frame %d: %s vs the shadow's %s" % (6 + i, look(h), look(s))
        after_resample = bool(h.trace()["resampled"])
    assert h.cell_stats()["rows"] > 0
    h.close(); s.close()
    return scores, diff, icp_words, icp_diff, kinds


def pick_three():
    """a picker with a memory of its own: one frame right behind a resample, one not, the last"""
    taken = {}

    def pick(i, after_resample, n_frames):
        if i == 0:
            return None
        if i == n_frames - 1:
            return "last"
        kind = "behind a resample" if after_resample else "not behind a resample"
        if kind in taken:
            return None
        taken[kind] = i
        return kind
    return pick


def pick_every(i, after_resample, n_frames):
    return "every"


def test_read_back_of_the_frames_scores_is_calibrated_in_default_mode(pkg, rk, world):
    """The frame leaves its scores in buffer 1 in particle order: in the default mode they equal the CPU oracle's orc_score_kd on the map
    before the frame and the dispersed particles -- every frame of an n = 1000 run with cell rows, and three frames at n = 20 000."""
    tree, scans = world
    a = frames_against_reference_kernel(pkg, rk, tree, scans[:10], 1000, 3, 0, pick_every)
    b = frames_against_reference_kernel(pkg, rk, tree, scans[:24], 20000, 0, 0, pick_three())
    assert len(b[4]) >= 2 and b[4][-1] == "last", b[4]
    report("default mode: the frame's score buffer == orc_score_kd in %d of %d scores (n 1000 every frame, n 20 000 %s)" % (a[0] + b[0] - a[1] - b[1], a[0] + b[0], b[4]))


@pytest.mark.parametrize("n,variant,n_frames", [(1000, 3, 10), (100000, 0, 24)])
def test_devlib_frames_own_scan_match_equals_kernEvaluateParticlesKD(pkg, rk, world, n, variant, n_frames):
    """k_score_kd_cells<false, PF_TRIG_DEVLIB> as the FRAME launches it (group-major 16-bit partials, k_reduce_groups, persistent cell rows) and
    the arrays k_icp_fused leaves, against the reference's own kernels: every frame at n = 1000 with cell rows, three frames of the
    n = 100 000 run (one right behind a resample, one not, the last); zero tolerance."""
    tree, scans = world
    pick = pick_every if n == 1000 else pick_three()
    sc, diff, words, wdiff, kinds = frames_against_reference_kernel(pkg, rk, tree, scans[:n_frames], n, variant, 1, pick)
    if n != 1000:
        assert len(kinds) == 3 and "behind a resample" in kinds and "not behind a resample" in kinds, kinds
    report("device library, n %d: the frame's own scan-match launch vs kernEvaluateParticlesKD: %d of %d scores differ (%d frames: %s); ICP arrays of k_icp_fused: %d of %d words differ"
           % (n, diff, sc, len(kinds), sorted(set(kinds)), wdiff, words))


# ---- 4. the ICP stage in device-library mode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,start,weird", [((0.1, -0.2, 0.3), (0.12, -0.19, 0.31), False), ((0, 0, 0), (0.01, 0.02, -0.01), False),
                                               ((0.3, 0.2, -0.4), (0.31, 0.22, -0.41), True)])
def test_devlib_icp_stage_equals_kernGetWallsKD_and_findCorrespondenceKD(pkg, rk, small_world, robot, start, weird):
    """k_icp_correspond with trig = 1: targets against kernGetWallsKD, correspondences against findCorrespondenceKD fed with those targets,
    bit for bit (the solve behind them does no trigonometry and is bit-pinned to the oracle: the pose must be the oracle's ICP of the
    product's own arrays, which the default-mode tests cover).  Poses of test_icp_matches_oracle_bitwise, scan of ..._uses_zero_fill."""
    tree = small_world["tree"]
    scan = (pkg.synth.make_weird_scan(9) if weird else pkg.synth.make_scan(small_world["segs"], robot, seed=77)).astype(np.float32)
    h = pkg.PfSlam(64)
    h.set_trig(1)
    h.set_map(tree); h.set_scan(scan); h.set_pose(robot)
    pose, _ = h.icp(start)
    gt, gc = d2h(rk, h, 11, np.float32, (len(scan), 4)), d2h(rk, h, 12, np.float32, (len(scan), 4))
    h.close()
    tar, cor = ref_icp_arrays(rk, tree, scan, np.asarray(robot, np.float32))
    bad_t, bad_c = int((bits(gt) != bits(tar)).sum()), int((bits(gc) != bits(cor)).sum())
    report("device library, ICP stage at %s: targets differing from kernGetWallsKD %d of %d words, correspondences differing from findCorrespondenceKD %d of %d words (rejected beams: %d)"
           % (robot, bad_t, gt.size, bad_c, gc.size, int((gt[:, 3] == 0).sum())))
    assert bad_t == 0 and bad_c == 0
    assert np.isfinite(pose).all()
    if weird:
        assert (gt[:, 3] == 0).sum() > 0   # the zero-filled slots of H2 are in the comparison


# ---- 5. differential fuzz with the shadow as comparator -----------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,seed", [({}, "201"), ({"PFSLAM_PLAN_MIN_N": "1", "PFSLAM_VARIANT": "3"}, "202")], ids=["plain", "rows-at-every-count"])
def test_devlib_differential_fuzz(extra, seed):
    """60 s of tests/fuzz_step.py --devlib (comparator: the shadow; pfslam_set_trig(1) on both), plain and with the cell rows at every count."""
    env = dict(os.environ, **extra)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_step.py"), "--devlib", "60", seed], capture_output=True, text=True, timeout=60 + 240, env=env)
    assert out.returncode == 0 and "fuzz ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    report("device library, fuzz (%s): %s" % (extra or "plain", out.stdout.strip().splitlines()[-1]))


# ---- 6. the marking pass does not look at the mode ----------------------------------------------------------------------------------------
def test_marking_pass_does_not_look_at_the_mode(pkg, world):
    """beam_box (csrc/kd_cells.hip.inc) computes its box from the SPECIFICATION's end point in either mode: two fresh handles, the aged map,
    the 100 000 particles and the next scan of the device-library run above, one pfslam_score_kd each in mode 0 and mode 1 -- the same cells
    claimed, walked, rows, pool slots, the invariants intact.  (Mode 1's scores: test_devlib_frames_own_scan_match_... and test_gpu_ref_kernels.py.)"""
    tree, scans = world
    n = 100000
    _, snap = shadow_on_world(pkg, tree, scans, n, 24, snaps=(12,))
    p, aged = snap[24][0], np.frombuffer(snap[24][1], dtype=O.NODE_DTYPE)
    assert len(aged) > len(tree)
    out = []
    for mode in (0, 1):
        with environ(PFSLAM_STABLE_ORDER="1"):
            h = pkg.PfSlam(n, kd_capacity=len(aged) + (1 << 18))
        h.set_variant(0)
        h.set_trig(mode)
        h.set_map(aged); h.set_particles(p); h.set_scan(scans[24])
        fit = h.score_kd()
        st, chk = h.cell_stats(), h.check_cells()
        h.close()
        assert chk["violations"] == 0 and st["rows"] > 0 and st["flags"] == 0, (mode, st, chk)
        out.append(({k: st[k] for k in BOOK}, {k: chk[k] for k in CHECK}, fit))
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    assert out[0][1] == out[1][1], (out[0][1], out[1][1])
    report("marking pass in mode 0 and mode 1: same bookkeeping %s; scores differing between the modes: %d of %d" % (out[0][0], int((bits(out[0][2]) != bits(out[1][2])).sum()), n))
