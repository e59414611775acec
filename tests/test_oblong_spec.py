"""Maps with oblong cells on the CPU oracle alone (tests/oblong_cases.py): the three geometries have the properties they were chosen
for, their runs tell the two axes apart (so that a kernel which uses one axis' cell size for the other cannot pass
tests/test_gpu_oblong_cells.py), and the oracle's per-axis arithmetic is the reference's, re-derived here in plain float32 numpy
from the reference's expressions (kernel.cu:536-537, 553-554, 1389-1392).  No GPU needed."""
import numpy as np
import pytest

import oblong_cases as B
import oracle_lib as O

NAMES = sorted(B.GEOMETRIES)


@pytest.fixture(scope="module")
def orc(oracle):
    return oracle


_RUNS = {}


def run12(g):
    key = B.geom(g)
    if key not in _RUNS:
        _RUNS[key] = B.kd_run(g, 12)
    return _RUNS[key]


# ---- 1. the inputs test what they claim ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_geometry_has_equal_cell_counts_and_a_living_map(orc, name):
    sx, sy, rx, ry = B.GEOMETRIES[name]
    assert rx != ry and B.dims(name) == (B.CELLS[name], B.CELLS[name])
    assert B.dims(B.transposed(name)) == (B.CELLS[name], B.CELLS[name])          # test_gpu_oblong_cells.py creates that handle too
    rec = run12(name)
    assert rec["trace"][0]["kd_size"] > 100
    assert all(t["n_wall"] > 100 and t["n_free"] > 1000 for t in rec["trace"]), [B.brief(t) for t in rec["trace"]]
    sizes = [0] + [t["kd_size"] for t in rec["trace"]]                           # frame 1 seeds the map, every later frame inserts
    assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    assert all(t["n_insert"] == b - a > 0 for t, a, b in zip(rec["trace"][1:], sizes[1:], sizes[2:])), rec["trace"]
    assert (rec["trace"][-1]["kd_size"], rec["trace"][-1]["n_insert"]) == B.TABLE[name], rec["trace"][-1]
    assert len(rec["map"]) == B.TABLE[name][0]


@pytest.mark.parametrize("other", ["transposed", "square_x", "square_y"])
@pytest.mark.parametrize("name", NAMES)
def test_kd_run_differs_from_the_run_with_the_axes_mixed(orc, name, other):
    """The run on the transposed patch and on either square patch differs from the oblong run in frame 1's (n_wall, n_free, kd_size)
    and in the final tree."""
    a, b = run12(name), run12(getattr(B, other)(name))
    assert B.brief(a["trace"][0]) != B.brief(b["trace"][0]), (name, other, B.brief(a["trace"][0]))
    assert a["map"].tobytes() != b["map"].tobytes(), (name, other)


@pytest.mark.parametrize("name", NAMES)
def test_grid_run_differs_from_the_transposed_run(orc, name):
    a, b = B.grid_run(name, 6), B.grid_run(B.transposed(name), 6)
    assert (a["grid0"] == b["grid0"]).all()
    assert (a["grid"] != b["grid"]).any(), name
    assert (a["grid"] != b["grid"].T).any(), name                                   # ... nor is it the transposed grid


# ---- 2. the oracle's per-axis arithmetic is the reference's ------------------------------------------------------------------------------
POSES = [(0.0, 0.0), (0.0125, 0.0125), (-0.0125, 0.0125), (0.37, -0.21), (-1.2, 0.9), (3.03, 3.03), (-3.03, -3.03), (0.06, 0.06),
         (0.075, 0.075), (-0.075, 0.075), (7.49, -7.49), (0.02, 0.015)]


@pytest.mark.parametrize("name", NAMES)
def test_centre_cell_per_axis(orc, name):
    """round(0.5 dim + p / res + res / 2) with each axis' own cell size: a zero-range beam marks the robot's own cell, and only it."""
    dim = B.CELLS[name]
    rx, ry = B.res_xy(name)
    apart = 0
    for px, py in POSES:
        pose = np.array([px, py, 0.3], np.float32)
        grid = np.zeros((dim, dim), np.int8)
        B.update_grid(name, grid, pose, np.zeros(1, np.float32))
        want = (B.cell_of(dim, px, rx), B.cell_of(dim, py, ry))
        assert np.argwhere(grid != 0).tolist() == [list(want)], (name, px, py, want)
        apart += want != (B.cell_of(dim, px, ry), B.cell_of(dim, py, rx))
    assert apart >= 8, apart                                                     # the poses tell the axes apart


def edge_values(coarse, fine):
    """Float32 values v with fl(v / coarse) = k + 1/2 exactly (a cell edge of the coarse axis: roundf goes away from zero) and
    fl(v / fine) an integer (the middle of a cell of the fine axis)."""
    out = []
    c, f = np.float32(coarse), np.float32(fine)
    for k in range(0, 300):
        v = np.float32((k + 0.5) * coarse)
        qc, qf = v / c, v / f
        if float(qc) == k + 0.5 and float(qf) == round(float(qf)):
            out.append(float(v))
    return out


BEAMS = [(540, 0.0, 1.0), (900, 0.0, 2.5), (180, 0.0, 0.77), (0, 0.0, 3.3), (1080, 0.0, 3.3), (333, 0.3, 5.123), (700, -2.0, 9.87),
         (100, 1.0, 14.2), (1000, 0.1, 19.5), (540, 0.785, 12.0), (20, 3.0, 0.26), (777, -0.4, 7.001)]


@pytest.mark.parametrize("name", NAMES)
def test_wall_cell_of_a_beam_per_axis(orc, name):
    """round(w / res) per axis on a dozen beams, and on end points that sit exactly on a cell edge of the coarse axis while they are
    mid-cell on the fine one: the same distance along x (beam 540) and along y (beam 900) then gives different offsets."""
    dim = B.CELLS[name]
    rx, ry = B.res_xy(name)
    cx, cy = dim // 2, dim // 2 + 3
    cases = list(BEAMS)
    coarse, fine = max(rx, ry), min(rx, ry)
    edges = edge_values(coarse, fine)[:6]
    assert len(edges) >= 2, (name, edges)
    cases += [(b, 0.0, v) for v in edges for b in (540, 900)]
    apart = 0
    for beam, theta, rng in cases:
        scan = np.full(1081, 1000.0, np.float32)                                  # every other beam is out of range
        scan[beam] = rng
        wx, wy = B.end_point(beam, rng, theta)
        assert abs(wx) < B.LIDAR_RANGE and abs(wy) < B.LIDAR_RANGE
        X, Y = cx + B.wall_offset(wx, rx), cy + B.wall_offset(wy, ry)
        fm, wm = B.masks(name, scan, cx, cy, theta)
        want = [X * dim + Y] if 0 <= X < dim and 0 <= Y < dim else []
        assert np.flatnonzero(wm).tolist() == want, (name, beam, theta, rng, X, Y)
        apart += (X, Y) != (cx + B.wall_offset(wx, ry), cy + B.wall_offset(wy, rx))
    assert apart >= 12, apart
    for v in edges:                                                              # on the coarse axis the edge rounds away from zero
        ex, _ = B.end_point(540, v, 0.0)
        _, ey = B.end_point(900, v, 0.0)
        assert float(ex) == v and float(ey) == v
        k = int(v / coarse)
        assert B.wall_offset(v, coarse) == k + 1 and float(np.float32(v) / np.float32(coarse)) == k + 0.5
        assert B.wall_offset(v, fine) == round(v / fine)


@pytest.mark.parametrize("name", NAMES)
def test_cell_to_point_rounds_to_each_axis_own_lattice(orc, name):
    """ROUND_FRAC(cell * res - scale / 2 + p, res) per axis: the points the map update looks up and inserts."""
    dim = B.CELLS[name]
    sx, sy, rx, ry = B.GEOMETRIES[name]
    rng = np.random.RandomState(5)
    cells = [(0, 0), (dim - 1, dim - 1), (0, dim - 1), (dim // 2, dim // 2), (dim // 2 + 1, dim // 2 - 1)]
    cells += [tuple(int(v) for v in rng.randint(0, dim, 2)) for _ in range(7)]
    for robot in ((0.0, 0.0, 0.0), (0.37, -0.21, 0.8), (-1.2, 0.9, -2.9), (0.0125, 0.02, 0.1)):
        fm = np.zeros(dim * dim, np.uint8); wm = np.zeros(dim * dim, np.uint8)
        order = sorted(cells)
        for i, (x, y) in enumerate(order):
            (wm if i % 2 else fm)[x * dim + y] = 1
        wall, free = B.masks_to_points(name, fm, wm, robot)
        assert len(wall) == len(order) // 2 and len(free) == len(order) - len(order) // 2
        for pts, sel in ((free, order[0::2]), (wall, order[1::2])):
            want = np.array([[B.cell_point(x, rx, sx, robot[0]), B.cell_point(y, ry, sy, robot[1]), 0, 0] for x, y in sel], np.float32)
            assert (B.bits(pts) == B.bits(want)).all(), (name, robot)
            mixed = np.array([[B.cell_point(x, ry, sx, robot[0]), B.cell_point(y, rx, sy, robot[1])] for x, y in sel], np.float32)
            assert (B.bits(mixed) != B.bits(want[:, :2])).any(), (name, robot)


def test_widened_helpers_keep_their_defaults(orc):
    """get_walls with one number or a pair, find_walls / loop_closure with or without a patch: the square default is unchanged."""
    scan = B.scans(1)[0]
    a = O.get_walls(scan, 800, 800, 0.3)
    b = O.get_walls(scan, 800, 800, 0.3, res=(0.025, 0.025))
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    c = O.get_walls(scan, 800, 800, 0.3, res=(0.025, 0.05))
    assert (a[1] != c[1]).any()
    grid = B.wall_grid("G1", 4)
    sa, sb = B.segments("G1", 50, 9)
    d = [O.find_walls(grid, p, q) for p, q in zip(sa, sb)]
    assert d == [O.find_walls(grid, p, q, O.default_patch()) for p, q in zip(sa, sb)]
    assert d != [O.find_walls(grid, p, q, B.patch("G1")) for p, q in zip(sa, sb)]
