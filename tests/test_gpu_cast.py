"""pfslam_cast and pfslam_map_raster on the GPU against their restatement (tests/cast_ref.py): ranges bit for bit, cells and stats integer
for integer, the raster byte for byte -- for 1 to 1081 beams and 1 to 300 poses (a partial wave, a partial workgroup, several
workgroups), at the ends of max_range, on maps of one node and of none that qualifies, for poses outside the box and poses that are not
finite, behind frames in flight (it must read the booked map and change nothing), in the device-library trigonometry mode, on a sharded
handle, and its refusals.  There is no tolerance anywhere in this file.

(A NaN weight cannot reach the device -- pfslam_set_map refuses it -- so that rule is held on the CPU: tests/test_cast_spec.py.)"""
import ctypes as C
import importlib

import numpy as np
import pytest

import cast_ref as CR
import oracle_lib as O
import register_ref as R
import search_ref as S
from test_gpu_search import device_targets

pytestmark = pytest.mark.gpu
RES = (0.025, 0.025)


@pytest.fixture(scope="module")
def world(pkg):
    tree, segs, pts = R.planar_tree(4000, seed=1)
    return {"tree": tree, "segs": segs, "pts": pts, "rasters": {}}


def raster(world, w_min=1.0, inflate=1):
    key = (float(w_min), int(inflate))
    if key not in world["rasters"]:
        world["rasters"][key] = CR.Raster(world["tree"], RES, w_min, inflate)
    return world["rasters"][key]


def handle(pkg, tree, nb=1081, **kw):
    h = pkg.PfSlam(64, n_beams=nb, kd_capacity=1 << 16, **kw)
    h.set_map(tree)
    return h


def poses_of(m, seed=3):
    rng = np.random.RandomState(seed)
    p = np.concatenate([rng.uniform(-15, 15, (m, 2)), rng.uniform(-3.2, 3.2, (m, 1))], axis=1).astype(np.float32)
    p[0] = (0.5, 0.3, 0.1)
    return p


def assert_cast(h, ras, poses, what="", ends=None, **opts):
    got = h.cast(poses, cells=True, **opts)
    want = CR.cast(ras, h.pose if poses is None else poses, h.nb, ends, **opts)
    assert CR.same(got, want) is None, "%s %r: %s" % (what, opts, CR.same(got, want))
    flat = h.cast(poses, **opts)                       # without the cells
    assert flat["cells"] is None and CR.same(flat, want, cells=False) is None
    return got


def tree_of(cells, w=4.0, res=RES):
    a = np.zeros((len(cells), 4), np.float32)
    a[:, 0] = np.array([c[0] for c in cells], np.float32) * np.float32(res[0])
    a[:, 1] = np.array([c[1] for c in cells], np.float32) * np.float32(res[1])
    a[:, 3] = w
    return O.kd_create(a)


# ---- 1. shapes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 65, 1081])
def test_ranges_cells_and_stats_equal_the_restatement(pkg, world, nb):
    h = handle(pkg, world["tree"], nb)
    for m in (1, 3, 65, 300):
        got = assert_cast(h, raster(world), poses_of(m, seed=m), "beams %d poses %d" % (nb, m))
        assert got["stats"][0] == m * nb and (m * nb < 1081 or 0 < got["stats"][1] < m * nb)
    h.close()


@pytest.mark.parametrize("max_range", [30.0, 5.0, float(np.float32(16384) * np.float32(0.025))])
def test_the_ends_of_max_range(pkg, world, max_range):
    h = handle(pkg, world["tree"])
    got = assert_cast(h, raster(world), poses_of(3), max_range=max_range, no_hit=-2.5)
    assert 0 < got["stats"][1] < 3 * 1081 and (got["ranges"][got["cells"][..., 0] == CR.MISS] == -2.5).all()
    h.close()


@pytest.mark.parametrize("opts", [dict(inflate=0), dict(inflate=3), dict(inflate=8, skip_cells=0), dict(w_min=-113.0, inflate=0), dict(skip_cells=40),
                                  dict(w_min=100.0), dict(no_hit=float("nan"), max_range=2.0)], ids=str)
def test_options(pkg, world, opts):
    h = handle(pkg, world["tree"])
    assert_cast(h, raster(world, opts.get("w_min", 1.0), opts.get("inflate", 1)), poses_of(5), **opts)
    h.close()


# ---- 2. edges --------------------------------------------------------------------------------------------------------------------------
def test_poses_outside_the_box_rows_that_are_not_finite_and_the_handle_s_pose(pkg, world):
    h = handle(pkg, world["tree"])
    poses = np.array([[0.5, 0.3, 0.1], [30.0, 0.0, 3.1], [np.nan, 0.0, 0.0], [-25.0, -25.0, 0.8], [0.0, np.inf, 0.0], [0.0, 45.0, -1.6], [0.0, 0.0, np.nan],
                      [21.0, 21.0, -2.4], [0.0, 0.0, -np.inf], [3000.0, 0.0, 0.0], [2.0e7, 0.0, 0.0], [10.0, -8.0, 0.3]], np.float32)
    got = assert_cast(h, raster(world), poses)
    hit = (got["cells"][..., 0] != CR.MISS).any(axis=1)
    assert hit.tolist() == [True, True, False, True, False, True, False, True, False, False, False, True]
    h.set_pose(np.array([10.0, -8.0, 0.3], np.float32))
    own = assert_cast(h, raster(world), None)
    assert (R.bits(own["ranges"][0]) == R.bits(got["ranges"][11])).all()
    h.close()


def test_a_map_of_one_node_a_start_on_it_and_a_walk_of_no_cells(pkg):
    tree = tree_of([(12, -7)])
    h = handle(pkg, tree)
    for inflate in (0, 1, 8):
        ras = CR.Raster(tree, RES, 1.0, inflate)
        poses = np.array([[0.0, 0.0, 0.0], [0.3, -0.175, 1.0], [0.31, -0.17, -2.0], [5.0, 5.0, -2.3]], np.float32)
        g1 = assert_cast(h, ras, poses, inflate=inflate)
        g0 = assert_cast(h, ras, poses, inflate=inflate, skip_cells=0)
        side = 2 * inflate + 1
        assert list(g1["stats"][2:]) == [1, side * side, 12 - inflate, -7 - inflate, side, side]
        assert (g0["cells"][1] == (12, -7)).all() and g0["stats"][1] >= g1["stats"][1] > 0
        assert inflate or not (g1["cells"][1:3, :, 0] != CR.MISS).any(), "from the only occupied cell, skipping it, nothing is hit"
        # n == 0: from the middle of a cell a beam of 0.4 cells ends in it
        none = assert_cast(h, ras, poses[[0, 1, 3]], inflate=inflate, skip_cells=0, max_range=0.01)
        assert none["stats"][1] == 0
    h.close()


def test_nodes_off_the_lattice_below_w_min_and_beyond_2_20_cells(pkg, world):
    extra = np.array([[0.26, 0.1137, 0.0, 4.0], [0.3, 0.3, 0.0, 0.5], [3.0e4, 0.0, 0.0, 4.0], [0.0, -2.7e4, 0.0, 4.0]], np.float32)
    tree = O.kd_create(np.concatenate([world["pts"], extra]))
    h = handle(pkg, tree)
    ras = CR.Raster(tree, RES, 1.0, 1)
    assert ras.qualifying == raster(world).qualifying + 1 and ras.box == raster(world).box
    assert_cast(h, ras, poses_of(3))
    h.close()


def test_oblong_cells(pkg, world):
    res = (0.025, 0.05)
    h = handle(pkg, world["tree"], map_scale=(40.0, 80.0), map_res=res)
    got = assert_cast(h, CR.Raster(world["tree"], res, 1.0, 1), poses_of(3))
    assert got["stats"][1] > 0
    box, occ = h.map_raster()
    assert box == CR.Raster(world["tree"], res, 1.0, 1).box
    h.close()


# ---- 3. the raster ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(), dict(inflate=0, w_min=-113.0), dict(inflate=8), dict(w_min=1000.0)], ids=str)
def test_map_raster_equals_the_restatement(pkg, world, opts):
    h = handle(pkg, world["tree"])
    ras = raster(world, opts.get("w_min", 1.0), opts.get("inflate", 1))
    box, occ = h.map_raster(**opts)
    assert box == ras.box and occ.shape == ras.dense().shape and occ.tobytes() == ras.dense().tobytes()
    o = h._cast_opts("map_raster", opts)
    stats = np.full(8, -5, np.int64)
    assert h.L.pfslam_map_raster(h._h, C.byref(o), stats.ctypes.data_as(C.c_void_p), None, 0) == 0        # the stats alone
    assert list(stats) == list(ras.stats())
    h.close()


# ---- 4. behind frames, and what it leaves alone ---------------------------------------------------------------------------------------------
def test_cast_behind_frames_in_flight_reads_the_booked_map_and_changes_nothing(pkg):
    torch = pytest.importorskip("torch")
    sharded = importlib.import_module("gpu-icp-slam_amd.sharded")

    def buffers(e):
        out = []
        for which in (11, 12):
            ptr, nbytes = e.device_ptr(which)
            out.append(torch.as_tensor(sharded._DevView(ptr, nbytes, "<i4", 4), device=torch.device("cuda", 0)).cpu().numpy().tobytes())
        return out

    n = 1000
    _, frames = pkg.synth.corridor_sequence(3, seed=5)
    h, twin = pkg.PfSlam(n, kd_capacity=1 << 16), pkg.PfSlam(n, kd_capacity=1 << 16)
    for f, (_, scan) in enumerate(frames, start=1):         # no synchronize in between: the cast books the frames first
        h.step(f, scan)
        twin.step(f, scan)
    poses = np.array([[0.04, 0.02, 0.008], [0.5, -0.2, 1.0], [-1.0, 0.3, -2.0]], np.float32)
    got = h.cast(poses, cells=True)
    own = h.cast(None, cells=True)
    every = h.cast(poses, cells=True, w_min=-113.0, inflate=0)       # (a young map's weights are low: every node)
    box, occ = h.map_raster()
    ras = CR.Raster(h.map(), RES, 1.0, 1)
    dense = CR.Raster(h.map(), RES, -113.0, 0)
    assert dense.qualifying == len(h.map()) > 100 and every["stats"][1] > 100
    assert CR.same(every, CR.cast(dense, poses, 1081, w_min=-113.0, inflate=0)) is None
    assert CR.same(got, CR.cast(ras, poses, 1081)) is None, CR.same(got, CR.cast(ras, poses, 1081))
    assert CR.same(own, CR.cast(ras, h.pose, 1081)) is None
    assert box == ras.box and occ.tobytes() == ras.dense().tobytes()
    assert (R.bits(h.pose) == R.bits(twin.pose)).all()
    ph, pt = h.particles(), twin.particles()
    for fld in ("x", "y", "theta", "w"):
        assert (R.bits(ph[fld]) == R.bits(pt[fld])).all(), fld
    assert h.map().tobytes() == twin.map().tobytes()
    assert np.asarray(h.grid()).tobytes() == np.asarray(twin.grid()).tobytes()
    assert buffers(h) == buffers(twin)
    centre = (h.pose.astype(np.float64) + (0.05, -0.05, 0.02)).astype(np.float32)
    small = dict(half_x=3, half_y=2, half_theta=1)
    assert S.same_result(h.search(centre, scores=True, **small), twin.search(centre, scores=True, **small)) is None
    assert h.check_cells()["violations"] == 0
    h.close(); twin.close()


# ---- 5. the trigonometry mode and the sharded wrapper ---------------------------------------------------------------------------------------
def test_the_device_library_trigonometry_mode(pkg, world):
    """pfslam_set_trig(1): the end points are the device's own, taken from the ICP stage of a second handle in the same mode (buffer 11
    after pfslam_icp, as tests/test_gpu_search.py does) on a scan of max_range everywhere -- 8 m, so that every beam is in the stage's range."""
    max_range = 8.0
    h, h2 = handle(pkg, world["tree"]), handle(pkg, world["tree"])
    h.set_trig(1)
    h2.set_trig(1)
    scan = np.full(1081, max_range, np.float32)
    h2.set_scan(scan)
    targets = device_targets(h2)

    def ends(pose, nb, rng):
        t, inr = targets(scan, pose)
        assert inr.all() and nb == 1081 and rng == max_range
        return t[:, 0], t[:, 1]

    poses = poses_of(3)
    got = assert_cast(h, raster(world), poses, "trig 1", ends, max_range=max_range)
    h.set_trig(0)
    spec = assert_cast(h, raster(world), poses, "trig 0", max_range=max_range)
    assert got["stats"][1] > 0 and spec["stats"][1] > 0
    h.close(); h2.close()


def test_a_handle_driven_through_the_shard_calls_with_world_1_gives_the_same_bits(pkg):
    torch = pytest.importorskip("torch")
    sharded = importlib.import_module("gpu-icp-slam_amd.sharded")
    a = pkg.PfSlam(500, kd_capacity=1 << 16)
    s = sharded.ShardedSlam(pkg, 500, 0, 1, device=0, torch=torch, kd_capacity=1 << 16)
    _, frames = pkg.synth.corridor_sequence(4, seed=7)
    for f, (_, scan) in enumerate(frames, start=1):
        a.step(f, scan)
        s.step(f, scan)
    issued = s.collectives
    poses = np.array([[0.05, 0.02, 0.01], [0.5, -0.2, 1.0]], np.float32)
    want = a.cast(poses, cells=True)
    assert want["stats"][1] > 0
    assert CR.same(s.cast(poses, cells=True), want) is None and CR.same(s.cast(None, cells=True), a.cast(None, cells=True)) is None
    (bs, os_), (ba, oa) = s.map_raster(), a.map_raster()
    assert bs == ba and os_.tobytes() == oa.tobytes() and s.collectives == issued
    a.close(); s.eng.close()


def test_replay_binary_with_cast_1_prints_the_handle_s_hits_and_agreement(tmp_path, pkg):
    """pfslamCastScan (host/kernel.h) through `pfslam_replay ... cast=1`: one line per frame with the hits of the default cast from the
    frame's pose and the beams whose cast range is within 0.1 m of the scan's, both the C-ABI's."""
    import os
    import subprocess
    from test_host_layer import HOST, SCENE_TXT, build_host
    build_host(pkg)
    _, frames = pkg.synth.corridor_sequence(4, seed=5)
    scene = tmp_path / "scene.txt"
    scene.write_text(SCENE_TXT)
    scans = np.stack([np.zeros(1081, np.float32)] + [s for _, s in frames])  # scans[0] is never used (frame starts at 1)
    lidar = tmp_path / "lidar.f32"
    scans.astype(np.float32).tofile(str(lidar))
    env = dict(os.environ, PFSLAM_PARTICLES="300", PFSLAM_KD_CAPACITY=str(1 << 16))
    out = subprocess.check_output([os.path.join(HOST, "pfslam_replay"), str(scene), str(lidar), "cast=1"], env=env).decode()
    lines = [l for l in out.splitlines() if l.startswith("cast ")]
    assert len(lines) == len(frames)
    h = pkg.PfSlam(300, kd_capacity=1 << 16)
    for f, ((_, scan), line) in enumerate(zip(frames, lines), start=1):
        h.step(f, scan)
        got = h.cast(h.pose)
        agree = int((np.abs(got["ranges"][0] - scan) <= np.float32(0.1)).sum())
        assert line.split() == ["cast", str(f), "hits", str(int(got["stats"][1])), "agree", str(agree)], line
    assert int(lines[-1].split()[3]) > 0
    h.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_leave_the_outputs_and_the_handle_goes_on(pkg, world):
    h = pkg.PfSlam(64, kd_capacity=1 << 16)
    with pytest.raises(pkg.PfSlamError, match="pfslam_cast: no map loaded"):
        h.cast(poses_of(1))
    with pytest.raises(pkg.PfSlamError, match="pfslam_map_raster: no map loaded"):
        h.map_raster()
    h.set_map(world["tree"])
    bad_opts = (dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=float("inf")), dict(max_range=float("nan")), dict(max_range=409.7),
                dict(w_min=float("nan")), dict(w_min=float("inf")), dict(inflate=-1), dict(inflate=9), dict(skip_cells=-1))
    esc = lambda s: s.replace("^", r"\^").replace("(", r"\(").replace(")", r"\)")
    for bad in bad_opts:
        cause = CR.refusal(1081, **bad)
        assert cause is not None, bad
        with pytest.raises(pkg.PfSlamError, match="pfslam_cast: .*%s" % esc(cause)):
            h.cast(poses_of(1), **bad)
        with pytest.raises(pkg.PfSlamError, match="pfslam_map_raster: .*%s" % esc(cause)):
            h.map_raster(**bad)
    with pytest.raises(TypeError):
        h.cast(poses_of(1), reserved_=1)
    with pytest.raises(ValueError, match="poses must be"):
        h.cast(np.zeros((2, 4), np.float32))

    # through the C-ABI: every refusal returns non-zero and writes no output
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    poses = poses_of(2)
    ranges, cells, stats = np.full(2 * 1081, 7.5, np.float32), np.full(4 * 1081, 77, np.int32), np.full(8, -5, np.int64)
    occ = np.full(16, 9, np.uint8)

    def options(**kw):
        o = h._cast_opts("cast", {k: v for k, v in kw.items() if k != "reserved_"})
        if "reserved_" in kw:
            o.reserved_[2] = kw["reserved_"]
        return o

    good = options()

    def call(p=poses, m=2, o=good, r=ranges, handle=None):
        return h.L.pfslam_cast(h._h if handle is None else handle, None if p is None else vp(p), m, None if o is None else C.byref(o),
                               None if r is None else vp(r), vp(cells), vp(stats))

    def untouched():
        return (ranges == 7.5).all() and (cells == 77).all() and (stats == -5).all() and (occ == 9).all()

    err = lambda: h.L.pfslam_last_error().decode()
    assert h.L.pfslam_cast(None, vp(poses), 2, C.byref(good), vp(ranges), vp(cells), vp(stats)) != 0 and "pfslam_cast: bad argument" in err()
    for kw, cause in ((dict(o=None), "bad argument"), (dict(r=None), "bad argument"), (dict(m=0), "m must be 1 .. 65536"), (dict(m=65537), "m must be 1 .. 65536"),
                      (dict(m=15521), "2^24 rays"), (dict(p=None), "needs m == 1"), (dict(o=options(reserved_=1)), "reserved_ must be 0"),
                      (dict(o=options(inflate=9)), "inflate must be 0 .. 8"), (dict(o=options(max_range=409.7)), "<= 16384")):
        assert call(**kw) != 0, kw
        assert "pfslam_cast: " in err() and cause in err(), (kw, err())
        assert untouched(), "an output was written: %r" % (kw,)
    empty = pkg.PfSlam(64, kd_capacity=1 << 16)
    assert call(handle=empty._h) != 0 and "pfslam_cast: no map loaded" in err() and untouched()
    empty.close()
    assert h.L.pfslam_map_raster(h._h, C.byref(good), None, vp(occ), 16) != 0 and "pfslam_map_raster: bad argument" in err()
    assert h.L.pfslam_map_raster(h._h, None, vp(stats), vp(occ), 16) != 0 and "pfslam_map_raster: bad argument" in err()
    assert h.L.pfslam_map_raster(h._h, C.byref(options(reserved_=1)), vp(stats), vp(occ), 16) != 0 and "pfslam_map_raster: reserved_ must be 0" in err()
    assert h.L.pfslam_map_raster(h._h, C.byref(good), vp(stats), vp(occ), 16) != 0 and "pfslam_map_raster: cap 16 is less" in err() and untouched()
    # a raster above 2^28 cells: found on the device
    wide = handle(pkg, tree_of([(0, 0), (1 << 19, 1 << 10), (-(1 << 10), -(1 << 19))]))
    assert call(handle=wide._h) != 0 and "pfslam_cast: the raster would have" in err() and "2^28" in err() and untouched()
    assert h.L.pfslam_map_raster(wide._h, C.byref(good), vp(stats), None, 0) != 0 and "pfslam_map_raster: the raster would have" in err() and untouched()
    wide.close()
    assert call() == 0 and not untouched()
    want = CR.cast(raster(world), poses, 1081)
    got = {"ranges": ranges.reshape(2, 1081), "cells": cells.reshape(2, 1081, 2), "stats": stats}
    assert CR.same(got, want) is None, CR.same(got, want)
    h.close()
