"""GPU parity on maps with oblong cells (map_res_x != map_res_y; tests/oblong_cases.py): every stage that carries both cell sizes --
k_get_walls, cell_to_point / k_scatter_cells, the wall keys and k_walls_rank_traverse, the cellDiag gates of the map update,
k_score_grid, find_walls, the per-axis lattice test of pfslam_set_map, the persistent cell rows (CellGeom) and the plan's box estimate
-- against the oracle, which follows the reference's resolution.x / resolution.y, and against the reference's own kernels.  Every
comparison is on bits; there is no tolerance anywhere.  tests/test_oblong_spec.py shows, without a GPU, that these inputs tell the two
axes apart: a kernel that takes one axis' cell size for the other cannot pass here."""
import ctypes as C
import time

import numpy as np
import pytest

import oblong_cases as B
import oracle_lib as O
import ref_kernels as R
from ref_kernels import f32, i32, ivec2, ptr, vec3
from test_gpu_map_geometry import FIELDS, same_cells, same_grid, same_trace
from test_gpu_ref_kernels import rk  # noqa: F401  (fixture)
from test_topology import loop_trajectory, walled_grid

pytestmark = pytest.mark.gpu

NAMES = sorted(B.GEOMETRIES)
N, CAP = B.N_PARTICLES, B.KD_CAP
PLAN_MIN = 4608            # tests/test_gpu_size_edges.py: from here on the default organisation scores with cell rows
bits = B.bits


@pytest.fixture(autouse=True)
def duration(request):
    t0 = time.perf_counter()
    yield
    print("[oblong cells] %s: %.2f s" % (request.node.name, time.perf_counter() - t0))


_RUNS = {}


def oracle_frames(g, frames, n=N, **cfg):
    """B.kd_run once per (geometry, frames, particles, configuration)."""
    key = (B.geom(g), frames, n, tuple(sorted(cfg.items())))
    if key not in _RUNS:
        _RUNS[key] = B.kd_run(g, frames, n=n, **cfg)
    return _RUNS[key]


def look(h, want, i, what):
    assert same_trace(h.trace(), want["trace"][i]), "%s frame %d: trace %s vs the oracle's %s" % (what, i + 1, h.trace(), want["trace"][i])
    assert (bits(h.pose) == want["pose"][i]).all(), "%s frame %d: pose %s" % (what, i + 1, h.pose)
    same_cells(h.cells(0), want["wall"][i], "%s frame %d, wall" % (what, i + 1))
    same_cells(h.cells(1), want["free"][i], "%s frame %d, free" % (what, i + 1))


def same_particles(got, want, what):
    for fld in FIELDS:
        assert (bits(got[fld]) == bits(want[fld])).all(), "%s: particles differ in %s" % (what, fld)


def at_end(h, want, what):
    m = h.map()
    assert len(m) == len(want["map"]) and m.tobytes() == want["map"].tobytes(), "%s: maps differ" % what
    same_particles(h.particles(), want["particles"], what)


def same_fits(got, want, what):
    bad = np.flatnonzero(bits(got) != bits(want))
    assert len(bad) == 0, "%s: %d of %d fits differ, the first at %d: %r vs the oracle's %r" % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


# ---- 1. KD frames, every organisation -----------------------------------------------------------------------------------------------------------
ORGANISATIONS = ["default", "variant2", "variant3_serial", "variant3", "variant4"]
KD_CASES = [(g, o, {}) for g in NAMES for o in ORGANISATIONS] + [
    ("G1", "variant3", {"lag": 0}), ("G3", "default", {"lag": 0}),
    ("G2", "variant3", {"strict_host_mirror": 0, "free_upload_bug": 1}), ("G1", "default", {"strict_host_mirror": 0, "free_upload_bug": 1})]


@pytest.mark.parametrize("name,organisation,extra", KD_CASES, ids=lambda v: ("-".join("%s%s" % kv for kv in sorted(v.items())) or "plain") if isinstance(v, dict) else v)
def test_kd_frames_in_every_organisation(pkg, name, organisation, extra):
    """Eight frames of pfslam_step against O.Slam.step: trace, pose bits and the ordered wall and free lists after every frame, map and
    particles at the end.  variant 3: frames 2 .. 8 are round-5 frames scored from the persistent cell rows, whose invariants hold."""
    frames = 8
    cfg = {k: v for k, v in extra.items() if k != "lag"}
    want = oracle_frames(name, frames, **cfg)
    what = "%s, %s %s" % (name, organisation, extra or "")
    h = pkg.PfSlam(N, kd_capacity=CAP, **cfg, **B.handle_kw(name))
    try:
        if organisation != "default":
            h.set_variant(int(organisation[7]))
        if organisation == "variant3_serial":
            h.set_serial(1)
        if "lag" in extra:
            h.set_lag(extra["lag"])
        rows = organisation.startswith("variant3")
        for i, s in enumerate(B.scans(frames)):
            h.step(i + 1, s)
            look(h, want, i, what)
            if rows and i >= 1:
                assert h.frame_mode()["round5_frame"], "%s: frame %d did not run as a round-5 frame" % (what, i + 1)
        if rows:
            st = h.cell_stats()
            assert st["rows"] > 100 and st["flags"] == 0, (what, st)
        at_end(h, want, what)
        if rows:
            chk = h.check_cells()
            assert chk["violations"] == 0 and chk["records"] > 0, (what, chk)
    finally:
        h.close()


# ---- 2. cell rows by default -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["G1", "G3"])
def test_cell_rows_by_default_at_4608_particles(pkg, monkeypatch, name):
    """4608 particles, the default organisation, five frames with the per-frame checks; then pfslam_score_kd on the handle's own state
    in variants 0, 2, 3 and 4 against O.score_kd."""
    monkeypatch.setenv("ORC_THREADS", "16")
    frames = 5
    want = oracle_frames(name, frames, n=PLAN_MIN)
    h = pkg.PfSlam(PLAN_MIN, kd_capacity=CAP, **B.handle_kw(name))
    try:
        for i, s in enumerate(B.scans(frames)):
            h.step(i + 1, s)
            look(h, want, i, "%s, 4608 particles" % name)
        st = h.cell_stats()
        assert h.frame_mode()["round5_frame"] and st["rows"] > 100 and st["flags"] == 0, (name, h.frame_mode(), st)
        at_end(h, want, "%s, 4608 particles" % name)
        assert h.check_cells()["violations"] == 0
        scan = B.scans(frames + 1)[-1]
        p, tree = want["particles"], want["map"]
        fit = O.score_kd(tree, p, scan, threads=16)
        h.set_particles(p); h.set_scan(scan)
        for variant in (0, 2, 3, 4):
            h.set_variant(variant)
            same_fits(h.score_kd(), fit, "%s, score_kd in variant %d" % (name, variant))
            rows, plan = h.cell_stats()["rows"] > 0, h.plan_stats()["rows"] > 0
            assert (rows, plan) == {0: (True, False), 2: (False, False), 3: (True, False), 4: (False, True)}[variant], (name, variant, rows, plan)
    finally:
        h.close()


# ---- 3. the lattice test is per axis --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["G1", "G3"])
def test_lattice_test_of_set_map_is_per_axis(pkg, name):
    """The oracle's final map of a geometry uploaded to a handle of that geometry (every point is on its lattice: cell rows) and to a
    handle of the transposed geometry (the x coordinates are off a lattice of the other cell size: no rows, the shared-prefix plan).
    The score does not depend on the resolution: both give O.score_kd's bits."""
    want = oracle_frames(name, 8)
    tree, p, scan = want["map"], want["particles"], B.scans(9)[-1]
    rx, ry = B.res_xy(name)
    kx = tree["x"].astype(np.float64) / ry                                     # the premise: some x is no multiple of the OTHER cell size
    assert (np.abs(kx - np.round(kx)) > 0.2).any()
    fit = O.score_kd(tree, p, scan)
    assert len(np.unique(fit)) > 10
    for g, on_lattice in ((name, True), (B.transposed(name), False)):
        h = pkg.PfSlam(N, kd_capacity=CAP, **B.handle_kw(g))
        try:
            h.set_variant(3)
            h.set_map(tree); h.set_particles(p); h.set_scan(scan)
            same_fits(h.score_kd(), fit, "%s map on %s" % (name, g))
            rows, plan = h.cell_stats()["rows"], h.plan_stats()["rows"]
            if on_lattice:
                assert rows > 0, (name, g, rows, plan)
            else:
                assert rows == 0 and plan > 0, (name, g, rows, plan)
        finally:
            h.close()


# ---- 4. stage calls --------------------------------------------------------------------------------------------------------------------------------------
def oracle_map_update(name, tree_in, robot, scan, cap):
    """The oracle's map update in its pieces (tests/test_gpu_stages.py's _oracle_map_update) on an oblong patch."""
    L = O.lib()
    pa = B.patch(name)
    cx, cy = B.kd_centre(name)
    fm, wm = B.masks(name, scan, cx, cy, robot[2])
    wall, free = B.masks_to_points(name, fm, wm, robot)
    nw, nf = len(wall), len(free)
    tree = np.zeros(cap, O.NODE_DTYPE); tree[:len(tree_in)] = tree_in
    size = len(tree_in)
    fc, _ = O.traverse_batch(tree, free[:, :3]); wc, _ = O.traverse_batch(tree, wall[:, :3])
    L.orc_update_map_kd(O.P(tree), O.P(free), O.P(fc), nf, -1, C.byref(pa))
    L.orc_update_map_kd(O.P(tree), O.P(wall), O.P(wc), nw, 4, C.byref(pa))
    create = np.zeros(max(nw, 1), np.uint8)
    L.orc_test_correspondence(O.P(tree), O.P(wall), O.P(wc), nw, O.P(create), C.byref(pa))
    for i in range(nw):
        if create[i]:
            O.kd_insert(tree, size, np.array([wall[i, 0], wall[i, 1], wall[i, 2], -100], np.float32)); size += 1
    return tree[:size], np.flatnonzero(wm).astype(np.int32), np.flatnonzero(fm).astype(np.int32)


STAGE_POSES = [(0.0, 0.0, 0.0), (0.37, -0.21, 0.8), (-1.2, 0.9, -2.9)]


@pytest.mark.parametrize("name", NAMES)
def test_map_update_and_icp_stages(pkg, name):
    """pfslam_update_map_kd at three poses on the oracle's map of the geometry (tree bytes, both cell lists), and pfslam_icp once."""
    tree = oracle_frames(name, 8)["map"]
    cap = len(tree) + 4000
    scan = B.scans(10)[-1]
    h = pkg.PfSlam(64, kd_capacity=cap, **B.handle_kw(name))
    try:
        for robot in STAGE_POSES:
            want_tree, want_wall, want_free = oracle_map_update(name, tree, robot, scan, cap)
            assert len(want_tree) > len(tree) and len(want_wall) > 100
            h.set_map(tree); h.set_scan(scan); h.set_pose(robot)
            h.update_map_kd()
            same_cells(h.cells(0), want_wall, "%s at %s, wall" % (name, robot))
            same_cells(h.cells(1), want_free, "%s at %s, free" % (name, robot))
            got = h.map()
            assert len(got) == len(want_tree) and got.tobytes() == want_tree.tobytes(), (name, robot)
        robot, start = (0.02, 0.01, 0.004), (0.03, 0.0, 0.01)
        h.set_map(tree); h.set_scan(scan); h.set_pose(robot)
        pose, dbg = h.icp(start)
        want, wdbg = O.icp(tree, robot, start, scan)
        assert (bits(dbg[:28]) == bits(wdbg[:28])).all() and (bits(pose) == bits(want)).all(), (name, pose, want)
    finally:
        h.close()


def mask_places(name):
    d = B.CELLS[name]
    rx, ry = B.res_xy(name)
    out = [("centre", np.array([0.013, -0.021, 0.3], np.float32)), ("corner", B.pose_on(name, d - 1, d - 2, -2.0)),
           ("corner00", B.pose_on(name, 0, 1, 1.0))]
    if name == "G2":
        out.append(("y edge", np.array([0.3, 0.5 * B.GEOMETRIES[name][1] - 0.5, 0.7], np.float32)))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_masks_of_the_grid_update(pkg, name):
    """pfslam_update_map_grid into an empty grid leaves -1 on a free cell, 4 on a wall cell and 3 on a cell that is both: the two masks,
    against O.get_walls with (res_x, res_y) from the robot's cell as the reference's expression gives it per axis."""
    d = B.CELLS[name]
    scan = B.scans(4)[-1]
    h = pkg.PfSlam(8, **B.handle_kw(name))
    try:
        for what, pose in mask_places(name):
            cx, cy = B.centre_cell(name, pose)
            fm, wm = O.get_walls(scan, cx, cy, pose[2], d, d, B.res_xy(name))
            assert wm.sum() > (100 if what in ("centre", "y edge") else 0) and fm.sum() > 100, (name, what, wm.sum(), fm.sum())
            h.set_grid(np.zeros((d, d), np.int8)); h.set_pose(pose); h.set_scan(scan)
            h.update_map_grid()
            g = h.grid().reshape(-1)
            assert np.isin(g, (-1, 0, 3, 4)).all()
            same_cells(np.flatnonzero((g == -1) | (g == 3)), np.flatnonzero(fm), "%s, %s: free mask" % (name, what))
            same_cells(np.flatnonzero(g >= 3), np.flatnonzero(wm), "%s, %s: wall mask" % (name, what))
    finally:
        h.close()


# ---- 5. the 2-D path ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_grid_frames_and_grid_score(pkg, name):
    """Six frames of pfslam_step_grid from a seeded random grid against O.Slam.step_grid, then one pfslam_score_grid."""
    frames = 6
    want = B.grid_run(name, frames)
    h = pkg.PfSlam(N, kd_capacity=CAP, **B.handle_kw(name))
    try:
        h.set_grid(want["grid0"])
        for i, s in enumerate(B.scans(frames)):
            h.step_grid(i + 1, s)
            assert same_trace(h.trace(), want["trace"][i]), (name, i + 1, h.trace(), want["trace"][i])
            assert (bits(h.pose) == want["pose"][i]).all(), (name, i + 1)
        same_grid(h.grid(), want["grid"], name)
        same_particles(h.particles(), want["particles"], name)
        scan = B.scans(frames + 1)[-1]
        fit = B.score_grid(name, want["grid"], want["particles"], scan)
        assert len(np.unique(fit)) > 10
        h.set_grid(want["grid"]); h.set_particles(want["particles"]); h.set_scan(scan)
        got = h.score_grid()
        bad = np.flatnonzero(got != fit)
        assert len(bad) == 0, "%s: %d grid scores differ, the first at %d: %d vs %d" % (name, len(bad), bad[0], got[bad[0]], fit[bad[0]])
    finally:
        h.close()


# ---- 6. rays and the graph ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_find_walls_on_random_segments(pkg, name):
    """200 random segments, ends beyond every side of the map included, on a grid with a few hundred confident walls."""
    grid = B.wall_grid(name, 4)
    a, b = B.segments(name, 200, 9)
    pa = B.patch(name)
    h = pkg.PfSlam(8, n_beams=1, **B.handle_kw(name))
    try:
        h.set_grid(grid)
        total, sides = 0, set()
        for p, q in zip(a, b):
            want = O.find_walls(grid, p, q, pa)
            assert h.find_walls(p, q) == want, (name, p, q, want)
            total += want
            sides |= {B.side_of(name, p), B.side_of(name, q)}
        assert total > 50 and sides >= {"", "x-", "x+", "y-", "y+"}, (total, sides)
    finally:
        h.close()


def test_topology_and_loop_closure_on_g1(pkg):
    """tests/test_topology.py's loop through set_pose / topology_update / check_loop_closure on a G1 handle, against O.Topology with
    G1's patch: the graph is in metres, the walls between two nodes are counted in oblong cells."""
    name = "G1"
    grid, pa = walled_grid(), B.patch(name)
    h = pkg.PfSlam(64, **B.handle_kw(name))
    try:
        h.set_grid(grid)
        t = O.Topology()
        rng = np.random.RandomState(0)
        proposed, differs = 0, 0
        for p in loop_trajectory():
            p = (p + np.array([rng.normal(0, 0.01), rng.normal(0, 0.01), 0], np.float32)).astype(np.float32)
            h.set_pose(p)
            t.update(p)
            assert h.topology_update() == t.n_nodes
            want = t.loop_closure(grid, p, patch=pa)
            assert h.check_loop_closure().tolist() == want.tolist(), p
            proposed += len(want)
            differs += want.tolist() != t.loop_closure(grid, p).tolist()
        nodes, idx = h.topology()
        assert idx == t.node_idx and (bits(nodes) == bits(t.nodes())).all()
        assert proposed > 0, "the oracle never proposes a pair"
        print("[oblong cells] loop on G1: %d pairs proposed, %d poses whose pairs differ from the square patch's" % (proposed, differs))
    finally:
        h.close()


def test_kd_frames_with_topology_on_g1(pkg):
    """Six KD frames with UpdateTopology + CheckLoopClosure inside the frame: closures per frame and the final graph."""
    name, frames = "G1", 6
    key = ("topology", name, frames)
    if key not in _RUNS:
        _RUNS[key] = B.kd_run(name, frames, topology=True)
    want = _RUNS[key]
    h = pkg.PfSlam(N, kd_capacity=CAP, **B.handle_kw(name))
    try:
        h.set_topology(1)
        for i, s in enumerate(B.scans(frames)):
            h.step(i + 1, s)
            look(h, want, i, "G1 with topology")
            assert h.closures().tolist() == want["closures"][i], i + 1
        nodes, idx = h.topology()
        assert idx == want["graph"][1] and (bits(nodes) == bits(want["graph"][0])).all()
        at_end(h, want, "G1 with topology")
    finally:
        h.close()


# ---- 7. the sub-cell shortcut at these resolutions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [0.03, 0.04, 0.05, 0.1])
def test_sub_cell_index_shortcut_at_other_resolutions(pkg, res):
    """tests/test_gpu_score.py's test_sub_cell_index_shortcut_agrees_with_the_exact_index on the lattices of the oblong geometries
    (selector 8 of pfslam_debug_math takes the resolution from its first input): +-40 ulps around every sub-cell edge with |k| <= 4200
    and 10^6 random queries.  The exact index is numpy's, from the sorted float edge list; the shortcut, wherever it applies, is the
    exact index; a query on an edge never takes it; and it applies to more than half of the random queries (a guard against a vacuous
    test -- the share itself is printed, not bounded)."""
    h = pkg.PfSlam(64)
    try:
        r = np.float32(res)
        k = np.arange(-4200, 4201)
        lo = k.astype(np.float32) * r
        mid = lo + np.float32(0.5) * r
        edges = np.empty(2 * len(k), np.float32)
        edges[0::2], edges[1::2] = lo, mid
        assert (np.diff(edges) > 0).all()
        near = [edges]
        a = b = edges
        for _ in range(40):
            a = np.nextafter(a, np.float32(np.inf)); b = np.nextafter(b, np.float32(-np.inf))
            near += [a, b]
        rnd = np.random.RandomState(3).uniform(-4199.0 * res, 4199.0 * res, 1000000).astype(np.float32)
        q = np.concatenate(near + [rnd]).astype(np.float32)
        got = h.debug_math(8, np.concatenate([[r], q]).astype(np.float32))[1:]
        want = np.searchsorted(edges, q, side="right") - 1 + 2 * int(k[0])
        inside = (q >= edges[0]) & (q < edges[-1])
        assert inside[-len(rnd):].all() and inside.sum() > 2 * len(rnd)
        assert (got[inside, 0] == want[inside]).all()
        safe = got[:, 1] != np.int32(-2 ** 31)
        assert (got[safe, 1] == got[safe, 0]).all()
        assert not safe[: len(edges)].any()
        share = float(safe[-len(rnd):].mean())
        print("[oblong cells] sub-cell shortcut at res %g: applies to %.4f %% of 10^6 random queries (%.4f %% take the exact index)"
              % (res, 100.0 * share, 100.0 * (1.0 - share)))
        assert share > 0.5, share
    finally:
        h.close()


# ---- 8. sharded -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_replicate_the_map_update_on_g1(pkg):
    """Two virtual ranks of one GPU through four frames on G1: every rank's replica of the map update."""
    torch = pytest.importorskip("torch")
    from test_gpu_sharded import _VirtualRanks
    name, frames = "G1", 4
    want = oracle_frames(name, frames)
    v = _VirtualRanks(pkg, torch, N, 2, kd_capacity=CAP, **B.handle_kw(name))
    try:
        for i, s in enumerate(B.scans(frames)):
            v.step(i + 1, s)
            assert same_trace(v.trace(), want["trace"][i]), (i + 1, v.trace(), want["trace"][i])
            assert (bits(v.pose) == want["pose"][i]).all(), i + 1
            for e in v.engs:
                same_cells(e.cells(0), want["wall"][i], "frame %d, wall" % (i + 1))
                same_cells(e.cells(1), want["free"][i], "frame %d, free" % (i + 1))
        for e in v.engs:
            assert e.map().tobytes() == want["map"].tobytes()
    finally:
        v.close()


# ---- 9. the reference's own kernels, device-library trigonometry: zero mismatches ----------------------------------------------------------------------------------------
NB = R.LIDAR_SIZE


def ref_patch(name):
    sx, sy, rx, ry = B.GEOMETRIES[name]
    return R.patch(scale=(sx, sy, 0.0), res=(rx, ry, 0.0))


@pytest.mark.parametrize("theta", [0.3, -2.0])
@pytest.mark.parametrize("name", ["G1", "G3"])
def test_devlib_masks_equal_kernGetWalls_on_oblong_cells(pkg, rk, name, theta):  # noqa: F811
    """k_get_walls and the ordered cell lists with the device library's trigonometry against the reference's kernGetWalls launched with
    the oblong patch, at the KD path's centre: wall and free cells, cell for cell."""
    d = B.CELLS[name]
    centre = B.kd_centre(name)
    scan = B.scans(10)[-1].copy()
    scan[3], scan[500] = 40.0, 0.0
    fm, wm = rk.zeros(d * d, np.uint8), rk.zeros(d * d, np.uint8)
    rk.launch("kernGetWalls", NB, 128, ptr(rk.dev(scan)), ivec2(*centre), f32(theta), ptr(fm), ptr(wm), ivec2(d, d), ref_patch(name))
    want_f, want_w = np.flatnonzero(fm.get()), np.flatnonzero(wm.get())
    assert len(want_w) > 100 and len(want_f) > 1000
    tree = oracle_frames(name, 8)["map"]
    h = pkg.PfSlam(64, kd_capacity=len(tree) + 4000, **B.handle_kw(name))
    try:
        h.set_trig(1)
        h.set_map(tree); h.set_scan(scan); h.set_pose((0.1, -0.2, theta))
        h.update_map_kd()
        same_cells(h.cells(0), want_w.astype(np.int32), "%s theta %.1f, wall" % (name, theta))
        same_cells(h.cells(1), want_f.astype(np.int32), "%s theta %.1f, free" % (name, theta))
    finally:
        h.close()


@pytest.mark.parametrize("name", ["G1", "G3"])
def test_devlib_grid_score_equals_kernEvaluateParticles_on_oblong_cells(pkg, rk, name):  # noqa: F811
    """k_score_grid with the device library's trigonometry against kernEvaluateParticles launched with the oblong patch: every one of
    the 1000 scores, particles whose end points leave the grid on either axis included."""
    d, n = B.CELLS[name], R.PARTICLE_COUNT
    sx, sy, rx, ry = B.GEOMETRIES[name]
    rng = np.random.RandomState(16)
    grid = rng.randint(-100, 100, d * d).astype(np.int8)
    p = O.make_particles(n)
    p["x"] = rng.normal(0.2, 0.05, n).astype(np.float32)
    p["y"] = rng.normal(-0.1, 0.05, n).astype(np.float32)
    p["theta"] = rng.normal(0.3, 0.02, n).astype(np.float32)
    p["x"][0], p["y"][1], p["x"][2], p["y"][3] = 0.5 * sx - 0.5, -0.5 * sy + 0.1, -0.5 * sx + 0.3, 0.5 * sy - 0.2
    scan = B.scans(10)[-1]
    fit = rk.zeros(n, np.int32)
    rk.launch("kernEvaluateParticles", n, 128, ptr(rk.dev(grid)), ivec2(d, d), ref_patch(name), ptr(rk.dev(p)), vec3(0, 0, 0), ptr(rk.dev(scan)), ptr(fit))
    want = fit.get()
    assert len(np.unique(want)) > 100
    h = pkg.PfSlam(n, **B.handle_kw(name))
    try:
        h.set_trig(1)
        h.set_grid(grid.reshape(d, d)); h.set_particles(p); h.set_scan(scan)
        got = h.score_grid()
    finally:
        h.close()
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s: %d grid scores differ from the reference kernel, the first at %d: %d vs %d" % (name, len(bad), bad[0], got[bad[0]], want[bad[0]])


def distinct_batches(idx, near):
    """Split a list of (point, node) pairs into launches in which no node occurs twice among the pairs that can write (`near`): the
    reference's read-modify-write is not atomic (H4); pair order per node is kept, which is what the clamps depend on."""
    occ = np.zeros(len(idx), np.int64)
    seen = {}
    for i in np.flatnonzero(near):
        occ[i] = seen.get(int(idx[i]), 0)
        seen[int(idx[i])] = occ[i] + 1
    return [np.flatnonzero((occ == k) & (near | (k == 0))) for k in range(int(occ.max()) + 1)]


@pytest.mark.parametrize("name", ["G1", "G3"])
def test_devlib_map_update_equals_kernUpdateMapKD_on_oblong_cells(pkg, rk, name):  # noqa: F811
    """The product's map update (device-library trigonometry) against the reference's kernUpdateMapKD and kernTestCorrespondance
    launched with the oblong patch on the product's own cell lists: the updated weights, the inserts and so the whole tree, byte for
    byte.  The points of the cells and the nearest nodes are the oracle's (cell_to_point and the traversal are checked elsewhere); which
    pairs are close enough to move a weight or to insert a node -- the cell diagonal of BOTH cell sizes -- is the reference kernels'."""
    tree = oracle_frames(name, 8)["map"].copy()
    tree["w"][::7] = 112.0                                                      # the clamps at +-113
    tree["w"][3::7] = -113.0
    cap = len(tree) + 4000
    d = B.CELLS[name]
    robot = (0.37, -0.21, 0.8)
    scan = B.scans(10)[-1]
    h = pkg.PfSlam(64, kd_capacity=cap, **B.handle_kw(name))
    try:
        h.set_trig(1)
        h.set_map(tree); h.set_scan(scan); h.set_pose(robot)
        h.update_map_kd()
        wall_cells, free_cells, got = h.cells(0), h.cells(1), h.map()
    finally:
        h.close()
    fm = np.zeros(d * d, np.uint8); wm = np.zeros(d * d, np.uint8)
    fm[free_cells], wm[wall_cells] = 1, 1
    wall, free = B.masks_to_points(name, fm, wm, robot)
    assert len(wall) > 100 and len(free) > 1000
    rx, ry = B.res_xy(name)
    diag = float(np.hypot(rx, ry))
    tb, t0 = rk.tree_dev(tree)
    for pts, val in ((free, -1), (wall, 4)):
        idx, _ = O.traverse_batch(tree, pts[:, :3])
        dist = np.hypot(pts[:, 0].astype(np.float64) - tree["x"][idx], pts[:, 1].astype(np.float64) - tree["y"][idx])
        for sel in distinct_batches(idx, dist < 2.0 * diag):                    # (farther pairs write nothing, whatever the rounding)
            if len(sel):
                rk.launch("kernUpdateMapKD", len(sel), 128, i32(len(sel)), ptr(t0), ptr(rk.dev(pts[sel])), ptr(rk.dev(idx[sel].astype(np.int32))), i32(val),
                          ref_patch(name))
    want = tb.get()[1:].copy()
    assert (want["w"] != tree["w"]).sum() > 100
    wc, _ = O.traverse_batch(want, wall[:, :3])
    dd = rk.zeros(len(wall), np.uint8)
    tb2, t2 = rk.tree_dev(want)
    rk.launch("kernTestCorrespondance", len(wall), 128, i32(len(wall)), ptr(t2), ptr(rk.dev(wall)), ptr(rk.dev(wc.astype(np.int32))), ptr(dd), ref_patch(name))
    create = dd.get() != 0
    assert 0 < create.sum() < len(wall)
    full = np.zeros(cap, O.NODE_DTYPE); full[:len(want)] = want
    size = len(want)
    for i in np.flatnonzero(create):
        O.kd_insert(full, size, np.array([wall[i, 0], wall[i, 1], wall[i, 2], -100], np.float32)); size += 1
    assert len(got) == size, "%s: the product inserted %d nodes, the reference's kernels ask for %d" % (name, len(got) - len(tree), size - len(tree))
    bad = np.flatnonzero(bits(got["w"]) != bits(full[:size]["w"]))
    assert len(bad) == 0, "%s: %d weights differ from the reference kernels', the first at node %d" % (name, len(bad), bad[0])
    assert got.tobytes() == full[:size].tobytes(), name
