"""GPU parity of the three pieces of device code that turn a scan into map cells -- the mask path (k_get_walls -> trace_ray_wave ->
k_count_cells / k_scatter_cells), the wall keys of the round-5 frame and k_find_walls -- on the scenarios of
tests/map_geometry_cases.py: map sizes that are odd, tiny, no multiple of a 16-cell chunk or a 4096-cell block, or above 4096 cells
per side; one ray per mask in every octant and at the lengths around the 64-lane and 256-thread strides; robot cells outside the
grid; grids at the clamps; and the caps of the three topology getters.  Everything is bit for bit against the oracle
(tests/oracle_lib.py): there is no tolerance anywhere.  tests/test_map_geometry_spec.py shows, without a GPU, that every scenario
reaches the edge it was built for."""
import ctypes as C
import time

import numpy as np
import pytest

import map_geometry_cases as G
import oracle_lib as O
from test_gpu_stages import _oracle_map_update
from test_topology import loop_trajectory

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "theta", "w")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(autouse=True)
def duration(request):
    t0 = time.perf_counter()
    yield
    print("[map geometry] %s: %.2f s" % (request.node.name, time.perf_counter() - t0))


def same_grid(got, want, what):
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d cells differ, the first at %s: %d vs the oracle's %d" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def same_cells(got, want, what):
    assert len(got) == len(want), "%s: %d cells, the oracle has %d" % (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s: %d of %d cells differ, the first at place %d: %d vs the oracle's %d" % (
        what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


def same_trace(a, b):
    if a == b:
        return True
    rest = lambda t: {k: v for k, v in t.items() if k != "neff"}
    return bool(np.isnan(a["neff"]) and np.isnan(b["neff"]) and rest(a) == rest(b))


def pose_on(dim, cx, cy, theta):
    return np.array([G.coord_of(dim, cx), G.coord_of(dim, cy), theta], np.float32)


# ---- 1. one ray per call, 2-D path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centre", ["middle", "corner00", "corner11"])
def test_every_short_ray_alone_in_its_mask(pkg, centre):
    """The 67-cell map, one beam: each of the 625 offsets of [-12, 12]^2 traced by itself from the middle cell and from two corner
    cells (where most rays leave the grid) into a fresh random grid."""
    dim, res = 67, G.res_of(67)
    cx, cy = {"middle": (33, 33), "corner00": (0, 0), "corner11": (dim - 1, dim - 1)}[centre]
    grid0 = G.random_grid(dim, 3)
    h = pkg.PfSlam(8, n_beams=1, **G.handle_kw(dim))
    try:
        for dx, dy in G.short_offsets():
            theta, scan = G.one_beam(dx, dy, res)
            pose = pose_on(dim, cx, cy, theta)
            h.set_grid(grid0); h.set_pose(pose); h.set_scan(scan)
            h.update_map_grid()
            want = G.update_grid(grid0.copy(), dim, pose, scan)
            same_grid(h.grid(), want, "ray (%d, %d) from cell (%d, %d)" % (dx, dy, cx, cy))
    finally:
        h.close()


# ---- 2. the same rays through the ordered lists ------------------------------------------------------------------------------------------
def kd_list_offsets():
    """The zero ray, every axis, diagonal and octant (shallow and steep) at 1, 2, 7 and 12 cells, and six rays to and through the far
    corner of the 67-cell map, whose cells lie in the masks' 9-cell tail: (32, 32) ends on the very last cell, (35, 35) frees it."""
    out = [(0, 0)]
    for L in (1, 2, 7, 12):
        out += [o for o in G.long_offsets(L) if o not in out]
    return out + [(32, 31), (32, 24), (36, 35), (40, 38), (32, 32), (35, 35)]


def test_single_rays_through_the_cell_lists(pkg, small_world):
    """update_map_kd with a one-beam scan on a loaded map, 67 cells per side: the ordered wall and free lists and the updated map
    against the oracle's stages."""
    dim, res = 67, G.res_of(67)
    pa = G.patch(dim)
    keep = small_world["pts"][(np.abs(small_world["pts"][:, :2]) < 3.0).all(axis=1)][:400]
    tree = pkg.kd_create(keep)
    cap = len(tree) + 64
    c = G.roundf(np.float32(0.5) * np.float32(dim) + np.float32(res) / np.float32(2))
    M, groups, tail_w, tail_f, last_w, last_f = dim * dim, set(), 0, 0, 0, 0
    h = pkg.PfSlam(8, n_beams=1, kd_capacity=cap, **G.handle_kw(dim))
    try:
        for dx, dy in kd_list_offsets():
            theta, scan = G.one_beam(dx, dy, res)
            robot = (0.02, -0.03, float(theta))
            want_tree, want_wall, want_free = oracle_map_update(tree, robot, scan, cap, dim, pa, c)
            h.set_map(tree); h.set_scan(scan); h.set_pose(robot)
            h.update_map_kd()
            same_cells(h.cells(0), want_wall, "ray (%d, %d), wall" % (dx, dy))
            same_cells(h.cells(1), want_free, "ray (%d, %d), free" % (dx, dy))
            got = h.map()
            assert len(got) == len(want_tree) and got.tobytes() == want_tree.tobytes(), (dx, dy)
            groups.add(G.classify(dx, dy))
            tail_w += int((want_wall >= M - M % 16).sum()); tail_f += int((want_free >= M - M % 16).sum())
            last_w += int((want_wall == M - 1).sum()); last_f += int((want_free == M - 1).sum())
    finally:
        h.close()
    assert groups == set(G.ALL_GROUPS) | {"zero"} and tail_w > 1 and tail_f > 1 and last_w > 0 and last_f > 0, (tail_w, tail_f, last_w, last_f)


def oracle_map_update(tree_in, robot, scan, cap, dim, pa, c):
    """tests/test_gpu_stages.py's _oracle_map_update at another map size (that one is tied to 1600 cells)."""
    if dim == 1600:
        return _oracle_map_update(tree_in, robot, scan, cap)
    L = O.lib()
    fm, wm = G.masks(dim, scan, c, c, robot[2])
    wall = np.zeros((dim * dim, 4), np.float32); free = np.zeros((dim * dim, 4), np.float32)
    nw, nf = C.c_int(), C.c_int()
    rb = np.asarray(robot, np.float32)
    L.orc_masks_to_points(O.P(fm), O.P(wm), dim, dim, C.byref(pa), O.P(rb), O.P(wall), C.byref(nw), O.P(free), C.byref(nf))
    nw, nf = nw.value, nf.value
    tree = np.zeros(cap, O.NODE_DTYPE); tree[:len(tree_in)] = tree_in
    size = len(tree_in)
    fc, _ = O.traverse_batch(tree, free[:nf, :3]); wc, _ = O.traverse_batch(tree, wall[:nw, :3])
    L.orc_update_map_kd(O.P(tree), O.P(free), O.P(fc), nf, -1, C.byref(pa))
    L.orc_update_map_kd(O.P(tree), O.P(wall), O.P(wc), nw, 4, C.byref(pa))
    create = np.zeros(max(nw, 1), np.uint8)
    L.orc_test_correspondence(O.P(tree), O.P(wall), O.P(wc), nw, O.P(create), C.byref(pa))
    for i in range(nw):
        if create[i]:
            O.kd_insert(tree, size, np.array([wall[i, 0], wall[i, 1], wall[i, 2], -100], np.float32)); size += 1
    return tree[:size], np.flatnonzero(wm).astype(np.int32), np.flatnonzero(fm).astype(np.int32)


# ---- 3. long rays and clipping, 1333 cells ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h1333(pkg):
    h = pkg.PfSlam(8, n_beams=1, **G.handle_kw(1333))
    yield h
    h.close()


@pytest.mark.parametrize("length", G.MASK_LENGTHS)
def test_long_rays_around_the_wave_stride(h1333, length):
    """24 rays whose longer side is `length` cells (axes, diagonals, a shallow and a steep ray per octant) from the middle of the
    1333-cell map, one per update; the grid carries over from ray to ray on both sides."""
    dim, res = 1333, G.res_of(1333)
    want = G.random_grid(dim, length)
    h1333.set_grid(want)
    for dx, dy in G.long_offsets(length):
        theta, scan = G.one_beam(dx, dy, res)
        pose = pose_on(dim, dim // 2, dim // 2, theta)
        h1333.set_pose(pose); h1333.set_scan(scan)
        h1333.update_map_grid()
        G.update_grid(want, dim, pose, scan)
        same_grid(h1333.grid(), want, "ray (%d, %d)" % (dx, dy))


@pytest.mark.parametrize("part", range(4))
def test_rays_clipped_at_every_side(h1333, part):
    """Robot cells -40, -1, 0, dim - 1, dim and dim + 40 on either axis and 100-cell rays in twelve directions: rays that leave the grid,
    enter it, cross a corner or miss it altogether."""
    dim, res = 1333, G.res_of(1333)
    cases = G.clip_cases(dim)[part::4]
    want = G.random_grid(dim, 50 + part)
    h1333.set_grid(want)
    for cx, cy, dx, dy in cases:
        theta, scan = G.one_beam(dx, dy, res)
        pose = pose_on(dim, cx, cy, theta)
        h1333.set_pose(pose); h1333.set_scan(scan)
        h1333.update_map_grid()
        G.update_grid(want, dim, pose, scan)
        same_grid(h1333.grid(), want, "ray (%d, %d) from cell (%d, %d)" % (dx, dy, cx, cy))


# ---- 4. every size: 2-D update at the clamps, 2-D score at the edges ----------------------------------------------------------------------------
@pytest.mark.parametrize("dim", sorted(G.SIZES))
def test_grid_update_and_score_at_every_size(pkg, dim):
    """A 1081-beam update from the middle and from the far corner of the map (cells in the masks' last chunk) into grids that hold the
    clamp values under the rays; then the 2-D score of 64, 65 and 300 particles standing on cells -1, 0, dim - 1 and dim."""
    for corner in (False, True):
        sc = G.size_scenario(dim, corner=corner)
        h = pkg.PfSlam(8, **G.handle_kw(dim))
        try:
            h.set_grid(sc["grid"]); h.set_pose(sc["pose"]); h.set_scan(sc["scan"])
            h.update_map_grid()
            want = G.update_grid(sc["grid"].copy(), dim, sc["pose"], sc["scan"])
            same_grid(h.grid(), want, "%d cells, corner=%s" % (dim, corner))
            h.update_map_grid()                                            # once more: the masks were cleared by the full memset path
            G.update_grid(want, dim, sc["pose"], sc["scan"])
            same_grid(h.grid(), want, "%d cells, corner=%s, second update" % (dim, corner))
        finally:
            h.close()
    for n in (64, 65, 300):
        sc = G.score_scenario(dim, n)
        h = pkg.PfSlam(n, **G.handle_kw(dim))
        try:
            h.set_grid(sc["grid"]); h.set_particles(sc["particles"]); h.set_scan(sc["scan"])
            got = h.score_grid()
            want = G.score_grid(sc)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, "%d cells, %d particles: %d scores differ, the first at %d: %d vs %d" % (
                dim, n, len(bad), bad[0], got[bad[0]], want[bad[0]])
        finally:
            h.close()


# ---- 5. whole frames -------------------------------------------------------------------------------------------------------------------------------
N_FRAME_PARTICLES = 96
KD_CAP = 1 << 16
_FRAMES = {}


def oracle_frames(dim):
    """O.Slam.step through four room scans, once per size: per frame the trace, the pose bits and both cell lists; at the end the map
    and the particles."""
    if dim not in _FRAMES:
        o = O.Slam(N_FRAME_PARTICLES, kd_capacity=KD_CAP, patch=G.patch(dim))
        rec = {"trace": [], "pose": [], "wall": [], "free": []}
        for f, s in enumerate(G.frame_scans(dim), start=1):
            o.step(f, s)
            rec["trace"].append(o.trace()); rec["pose"].append(bits(o.pose).copy())
            rec["wall"].append(o.cells(0)); rec["free"].append(o.cells(1))
        rec["map"], rec["particles"] = o.tree(), o.particles()
        o.close()
        _FRAMES[dim] = rec
    return _FRAMES[dim]


def look(h, want, i, what):
    assert same_trace(h.trace(), want["trace"][i]), "%s frame %d: trace %s vs the oracle's %s" % (what, i + 1, h.trace(), want["trace"][i])
    assert (bits(h.pose) == want["pose"][i]).all(), "%s frame %d: pose %s" % (what, i + 1, h.pose)
    same_cells(h.cells(0), want["wall"][i], "%s frame %d, wall" % (what, i + 1))
    same_cells(h.cells(1), want["free"][i], "%s frame %d, free" % (what, i + 1))


def at_end(h, want, what):
    m = h.map()
    assert len(m) == len(want["map"]) and m.tobytes() == want["map"].tobytes(), "%s: maps differ" % what
    got = h.particles()
    for fld in FIELDS:
        assert (bits(got[fld]) == bits(want["particles"][fld])).all(), "%s: particles differ in %s" % (what, fld)


@pytest.mark.parametrize("organisation", ["default", "variant3_serial"])
@pytest.mark.parametrize("dim", [151, 250, 1333, 4800])
def test_kd_frames_at_odd_and_large_sizes(pkg, dim, organisation):
    """Four frames of pfslam_step against O.Slam.step: trace, pose bits and the ordered wall and free lists after every frame, map and
    particles at the end.  variant 3 + serial: frames 2 .. 4 are round-5 frames, whose wall keys replace the wall mask."""
    want = oracle_frames(dim)
    assert want["trace"][0]["kd_size"] > 100 and all(t["n_wall"] > 100 and t["n_free"] > 1000 for t in want["trace"])
    h = pkg.PfSlam(N_FRAME_PARTICLES, kd_capacity=KD_CAP, **G.handle_kw(dim))
    try:
        if organisation == "variant3_serial":
            h.set_variant(3); h.set_serial(1)
        for i, s in enumerate(G.frame_scans(dim)):
            h.step(i + 1, s)
            look(h, want, i, "%d cells, %s" % (dim, organisation))
            if organisation == "variant3_serial" and i >= 1:
                assert h.frame_mode()["round5_frame"], "%d cells: frame %d did not run as a round-5 frame" % (dim, i + 1)
        at_end(h, want, "%d cells, %s" % (dim, organisation))
    finally:
        h.close()


@pytest.mark.parametrize("dim", sorted(G.SIZES))
def test_grid_frames_at_every_size(pkg, dim):
    """Four frames of pfslam_step_grid against O.Slam.step_grid at every size, from a random grid."""
    o = O.Slam(N_FRAME_PARTICLES, kd_capacity=KD_CAP, patch=G.patch(dim))
    h = pkg.PfSlam(N_FRAME_PARTICLES, kd_capacity=KD_CAP, **G.handle_kw(dim))
    try:
        g0 = G.random_grid(dim, 77)
        o.set_grid(g0); h.set_grid(g0)
        for f, s in enumerate(G.frame_scans(dim), start=1):
            o.step_grid(f, s); h.step_grid(f, s)
            assert same_trace(h.trace(), o.trace()), (dim, f, h.trace(), o.trace())
            assert (bits(h.pose) == bits(o.pose)).all(), (dim, f)
        same_grid(h.grid(), o.grid, "%d cells" % dim)
        got, want = h.particles(), o.particles()
        for fld in FIELDS:
            assert (bits(got[fld]) == bits(want[fld])).all(), (dim, fld)
    finally:
        h.close(); o.close()


def test_two_ranks_replicate_the_map_update_at_151_cells(pkg):
    """Two virtual ranks of one GPU through the same four frames at 151 cells: every rank's replica of the map update."""
    torch = pytest.importorskip("torch")
    from test_gpu_sharded import _VirtualRanks
    dim = 151
    want = oracle_frames(dim)
    v = _VirtualRanks(pkg, torch, N_FRAME_PARTICLES, 2, kd_capacity=KD_CAP, **G.handle_kw(dim))
    try:
        for i, s in enumerate(G.frame_scans(dim)):
            v.step(i + 1, s)
            assert same_trace(v.trace(), want["trace"][i]), (i + 1, v.trace(), want["trace"][i])
            assert (bits(v.pose) == want["pose"][i]).all(), i + 1
            for e in v.engs:
                same_cells(e.cells(0), want["wall"][i], "frame %d, wall" % (i + 1))
                same_cells(e.cells(1), want["free"][i], "frame %d, free" % (i + 1))
        for e in v.engs:
            m = e.map()
            assert m.tobytes() == want["map"].tobytes()
    finally:
        v.close()


# ---- 6. find_walls -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["middle", "corner", "outside"])
def test_find_walls_every_short_ray_both_ways(pkg, start):
    """The 67-cell map, a grid dense in 30 and 31: every ray between a start cell and the cells of [-9, 9]^2 around it, in both
    directions (the end point left out differs)."""
    dim = 67
    sx, sy = {"middle": (33, 33), "corner": (0, dim - 1), "outside": (-1, 20)}[start]
    grid = G.walls_30_31(dim, 6)
    h = pkg.PfSlam(8, n_beams=1, **G.handle_kw(dim))
    try:
        h.set_grid(grid)
        total = 0
        for dx, dy in G.short_offsets(9):
            a = (G.coord_of(dim, sx), G.coord_of(dim, sy))
            b = (G.coord_of(dim, sx + dx), G.coord_of(dim, sy + dy))
            for p, q in ((a, b), (b, a)):
                want = G.find_walls(grid, dim, p, q)
                assert h.find_walls(p, q) == want, (sx, sy, dx, dy, p is b)
                total += want
        assert total > 0
    finally:
        h.close()


@pytest.mark.parametrize("length", G.FIND_LENGTHS)
def test_find_walls_around_the_block_stride(h1333, length):
    dim = 1333
    grid = G.walls_30_31(dim, length)
    h1333.set_grid(grid)
    c = dim // 2
    a = (G.coord_of(dim, c), G.coord_of(dim, c))
    for dx, dy in G.long_offsets(length):
        b = (G.coord_of(dim, c + dx), G.coord_of(dim, c + dy))
        for p, q in ((a, b), (b, a)):
            assert h1333.find_walls(p, q) == G.find_walls(grid, dim, p, q), (dx, dy, p is b)


def test_find_walls_with_ends_outside_each_side(h1333):
    dim = 1333
    grid = G.walls_30_31(dim, 8)
    h1333.set_grid(grid)
    n = 0
    for cx, cy, dx, dy in G.clip_cases(dim)[::2]:
        a = (G.coord_of(dim, cx), G.coord_of(dim, cy))
        for k in (1, 15):                                                   # 100 cells (one end outside), 1500 cells (both ends outside)
            b = (G.coord_of(dim, cx + k * dx), G.coord_of(dim, cy + k * dy))
            want = G.find_walls(grid, dim, a, b)
            assert h1333.find_walls(a, b) == want, (cx, cy, dx, dy, k)
            n += want > 0
    assert n > 0


# ---- 7. caps ---------------------------------------------------------------------------------------------------------------------------------------------
def loop_grid(dim):
    grid = np.full((dim, dim), -100, np.int8)
    c = dim // 2
    grid[c - 10:c + 10, c] = 113
    grid[c + 25, c - 20:c + 40] = 31
    grid[c + 35, c - 20:c + 40] = 30
    return grid


def capped(fn, cap, count_slot=True):
    """Call a (pairs, cap, n) getter of the C-ABI on a sentinel-filled buffer of 64 pairs; returns (count, buffer)."""
    buf = np.full((64, 2), -7, np.int32)
    n = C.c_int(-1)
    rc = fn(None if cap == 0 else buf.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    assert rc == 0
    return n.value, buf


def test_caps_of_the_topology_getters(pkg):
    """pfslam_check_loop_closure, pfslam_get_closures and pfslam_get_topology with a cap below the count: the count is the full count,
    exactly min(count, cap) entries are written and the words behind them are untouched (include/pfslam.h: "pairs beyond cap are
    counted, not written").  The loop of tests/test_topology.py on the 151-cell map, until the oracle proposes at least four pairs."""
    dim = 151
    L = pkg.load()
    pa = G.patch(dim)
    grid = loop_grid(dim)
    n_p = 32
    h = pkg.PfSlam(n_p, **G.handle_kw(dim))
    o = O.Slam(n_p, patch=pa)
    try:
        h.set_grid(grid)
        t = O.Topology()
        want = None
        for p in loop_trajectory():
            h.set_pose(p)
            t.update(p)
            assert h.topology_update() == t.n_nodes
            pairs = np.zeros((4096, 2), np.int32)
            r = np.ascontiguousarray(p, np.float32)
            cnt = O.lib().orc_check_loop_closure(C.byref(t), O.P(grid), dim, dim, C.byref(pa), O.P(r), O.P(pairs), 4096)
            if cnt >= 4:
                want = pairs[:cnt].copy()
                break
        assert want is not None, "the oracle never proposes four pairs"
        count = len(want)
        assert 4 <= count <= 64
        # check_loop_closure
        for cap in (0, 1, count):
            got_n, buf = capped(lambda b, c, n: L.pfslam_check_loop_closure(h._h, b, c, n), cap)
            assert got_n == count, (cap, got_n, count)
            assert (buf[:min(count, cap)] == want[:min(count, cap)]).all() and (buf[min(count, cap):] == -7).all(), cap
        # get_topology below the node count
        assert t.n_nodes >= 4
        for cap in (0, 2, t.n_nodes):
            nodes = np.full((64, 3), -7.0, np.float32)
            n, idx = C.c_int(-1), C.c_int(-1)
            assert L.pfslam_get_topology(h._h, None if cap == 0 else nodes.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(idx)) == 0
            assert n.value == t.n_nodes and idx.value == t.node_idx
            assert (bits(nodes[:cap]) == bits(t.nodes()[:cap])).all() and (nodes[cap:] == -7.0).all(), cap
        # get_closures of a frame (mode 1): one 2-D frame at the same pose, the oracle's engine carrying the same graph and grid
        o.set_topology(True); o.set_grid(grid)
        C.memmove(O.lib().orc_slam_topology(o.h), C.byref(t), C.sizeof(O.Topology))
        h.set_topology(1)
        cloud = O.make_particles(n_p, float(p[0]), float(p[1]), 0.0)
        scan = G.room(dim, 1081, 0)
        o.set_particles(cloud); h.set_particles(cloud)
        o.step_grid(7, scan); h.step_grid(7, scan)
        fw = o.closures()
        fcount = len(fw)
        assert 4 <= fcount <= 64
        for cap in (0, 1, fcount):
            got_n, buf = capped(lambda b, c, n: L.pfslam_get_closures(h._h, b, c, n), cap)
            assert got_n == fcount, (cap, got_n, fcount)
            assert (buf[:min(fcount, cap)] == fw[:min(fcount, cap)]).all() and (buf[min(fcount, cap):] == -7).all(), cap
    finally:
        h.close(); o.close()


# ---- 5, continued: the KD frames on the two tiny maps, where the oracle seeds a map at all ----------------------------------------------------------
@pytest.mark.parametrize("organisation", ["default", "variant3_serial"])
@pytest.mark.parametrize("dim", [3, 67])
def test_kd_frames_on_the_tiny_maps(pkg, dim, organisation):
    """pfslam_step at 3 and 67 cells runs only where the oracle's first KD frame seeds a map (a frame without a map only seeds again);
    which of the two ran is printed.  The rooms are scaled with the map, so both sizes seed one: two nodes at 3 cells, where the
    robot's own cell is the last cell of the masks' 9-cell tail."""
    want = oracle_frames(dim)
    seeded = want["trace"][0]["kd_size"] > 0
    print("[map geometry] %d cells: the oracle's first KD frame seeds %d nodes: pfslam_step %s" % (
        dim, want["trace"][0]["kd_size"], "runs" if seeded else "is left out (step_grid only, test_grid_frames_at_every_size)"))
    if not seeded:
        return
    h = pkg.PfSlam(N_FRAME_PARTICLES, kd_capacity=KD_CAP, **G.handle_kw(dim))
    try:
        if organisation == "variant3_serial":
            h.set_variant(3); h.set_serial(1)
        for i, s in enumerate(G.frame_scans(dim)):
            h.step(i + 1, s)
            look(h, want, i, "%d cells, %s" % (dim, organisation))
        print("[map geometry] %d cells, %s: frame mode %s" % (dim, organisation, h.frame_mode()))
        at_end(h, want, "%d cells, %s" % (dim, organisation))
    finally:
        h.close()
