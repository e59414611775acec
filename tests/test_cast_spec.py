"""The restatement of pfslam_cast (tests/cast_ref.py, vectorised over t) pinned against an independent cell-by-cell Python loop on small
cases, then what the feature is for: the scan cast through a map of wall points against the scan cast from the walls themselves
(synth.make_scan), on dense and on sparse walls.  No GPU needed."""
import math

import numpy as np
import pytest

import cast_ref as CR

F = np.float32
RES = (0.025, 0.025)


def loop_cast(nodes, poses, nb, res=RES, **opts):
    """pfslam_cast cell by cell: Python integers, a set of occupied cells, one ray and one cell at a time."""
    o = CR.options(**opts)
    rx, ry = F(res[0]), F(res[1])
    occupied, own = set(), []
    with np.errstate(all="ignore"):
        for x, y, _, w in np.ascontiguousarray(nodes, np.float32).reshape(-1, 4):
            nx, ny = np.rint(x / rx), np.rint(y / ry)
            if not (w >= F(o["w_min"]) and abs(nx) <= 2**20 and abs(ny) <= 2**20):
                continue
            own.append((int(nx), int(ny)))
            for ox in range(-o["inflate"], o["inflate"] + 1):
                for oy in range(-o["inflate"], o["inflate"] + 1):
                    occupied.add((int(nx) + ox, int(ny) + oy))
    box = (0, 0, 0, 0)
    if own:
        xs, ys = [c[0] for c in own], [c[1] for c in own]
        box = (min(xs) - o["inflate"], min(ys) - o["inflate"], max(xs) - min(xs) + 1 + 2 * o["inflate"], max(ys) - min(ys) + 1 + 2 * o["inflate"])
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 3)
    ranges = np.full((len(poses), nb), F(o["no_hit"]), np.float32)
    cells = np.full((len(poses), nb, 2), -2**31, np.int64)
    hits = 0
    sgn = lambda v: (v > 0) - (v < 0)
    for r, (x, y, th) in enumerate(poses):
        X, Y = CR.oracle_ends((x, y, th), nb, o["max_range"])
        for b in range(nb):
            with np.errstate(all="ignore"):
                ends = [float(np.rint(x / rx)), float(np.rint(X[b] / rx)), float(np.rint(y / ry)), float(np.rint(Y[b] / ry))]
            if not all(math.isfinite(v) and abs(v) <= 2**20 for v in ends):
                continue
            sx, ex, sy, ey = [int(v) for v in ends]
            dx, dy = ex - sx, ey - sy
            n = max(abs(dx), abs(dy))
            for t in range(o["skip_cells"], n + 1 if n else 0):
                if abs(dx) >= abs(dy):
                    kx, ky = sx + sgn(dx) * t, sy + sgn(dy) * ((2 * t * abs(dy) + n) // (2 * n))
                else:
                    ky, kx = sy + sgn(dy) * t, sx + sgn(dx) * ((2 * t * abs(dx) + n) // (2 * n))
                if (kx, ky) in occupied:
                    ddx, ddy = F(kx) * rx - x, F(ky) * ry - y
                    ranges[r, b] = np.sqrt(ddx * ddx + ddy * ddy)
                    cells[r, b] = kx, ky
                    hits += 1
                    break
    return {"ranges": ranges, "cells": cells.astype(np.int32), "stats": np.array([len(poses) * nb, hits, len(own), len(occupied)] + list(box), np.int64),
            "occupied": occupied}


def nodes_of(cells, w=4.0, res=RES):
    a = np.zeros((len(cells), 4), np.float32)
    a[:, 0] = np.array([c[0] for c in cells], np.float32) * F(res[0])
    a[:, 1] = np.array([c[1] for c in cells], np.float32) * F(res[1])
    a[:, 3] = w
    return a


def ring(radius, step=1):
    """The cells of a square ring around the origin (every `step`-th one): something to hit in every direction."""
    out = []
    for k in range(-radius, radius + 1, step):
        out += [(k, -radius), (k, radius), (-radius, k), (radius, k)]
    return sorted(set(out))


def agree(nodes, poses, nb, res=RES, **opts):
    want = loop_cast(nodes, poses, nb, res, **opts)
    o = CR.options(**opts)
    ras = CR.Raster(nodes, res, o["w_min"], o["inflate"])
    got = CR.cast(ras, poses, nb, **opts)
    assert CR.same(got, want) is None, CR.same(got, want)
    occ = ras.dense()
    x0, y0, W, H = ras.box
    assert occ.shape == (W, H) and int(occ.sum()) == len(want["occupied"]) == ras.occupied
    assert all(occ[kx - x0, ky - y0] for kx, ky in want["occupied"])
    return got


def test_every_octant_the_diagonals_and_the_axes():
    nodes = nodes_of(ring(60))
    poses = np.array([[0.0, 0.0, 0.0], [0.1, -0.05, 0.1], [0.0, 0.0, math.pi], [-0.3, 0.2, 2.0]], np.float32)
    got = agree(nodes, poses, 1081, max_range=3.0)
    c = got["cells"].astype(np.int64)
    hit = c[..., 0] != CR.MISS
    assert hit[0].all(), "a ring around the robot is hit by every beam"
    dx, dy = c[..., 0][hit], c[..., 1][hit]
    octants = set(zip((dx > 0).tolist(), (dy > 0).tolist(), (abs(dx) > abs(dy)).tolist()))
    assert len(octants) == 8
    s = c[0] - 0                                   # pose 0 stands in cell (0, 0): the hit cell is the offset
    assert (abs(s[:, 0]) == abs(s[:, 1])).any(), "no beam ends on a diagonal"
    assert (s[:, 1] == 0).any() and (s[:, 0] == 0).any(), "no beam runs along an axis"
    # the same with every cell of the walk tested from the robot's own cell on
    agree(nodes, poses, 1081, max_range=3.0, skip_cells=0)


def test_a_walk_of_no_cells_and_a_skip_beyond_the_walk():
    nodes = nodes_of(ring(2) + [(0, 0)])
    got = agree(nodes, [[0.0, 0.0, 0.3]], 1081, max_range=0.01, skip_cells=0, no_hit=-1.0)       # n == 0: the own cell is occupied and still no hit
    assert got["stats"][1] == 0 and (got["ranges"] == -1.0).all() and (got["cells"] == CR.MISS).all()
    got = agree(nodes, [[0.0, 0.0, 0.3]], 1081, max_range=1.0, skip_cells=41)                    # n <= 40 + 1
    assert got["stats"][1] == 0
    got = agree(nodes, [[0.0, 0.0, 0.3]], 1081, max_range=1.0, skip_cells=2)
    assert got["stats"][1] == 1081


def test_a_start_outside_the_box_and_on_an_occupied_cell():
    nodes = nodes_of(ring(20, 1))
    outside = np.array([[2.0, 0.1, math.pi], [-1.5, -1.5, 0.8], [0.0, 3.0, -1.6], [40.0, 40.0, 0.0]], np.float32)
    got = agree(nodes, outside, 1081, max_range=5.0)
    assert (got["cells"][3] == CR.MISS).all()
    for r in range(3):      # (seen from outside the 1 m ring fills 20 to 40 degrees of the fan)
        assert 80 < (got["cells"][r, :, 0] != CR.MISS).sum() < 400
    on = np.array([[0.5, 0.1, 0.0]], np.float32)                                                 # the cell (20, 4) of the ring
    g0, g1 = agree(nodes, on, 1081, max_range=2.0, skip_cells=0), agree(nodes, on, 1081, max_range=2.0, skip_cells=1)
    assert (g0["cells"][0] == (20, 4)).all(), "with skip_cells 0 every beam hits the robot's own cell"
    assert not (g1["cells"][0] == (20, 4)).all(axis=1).any() and g1["stats"][1] > 0


@pytest.mark.parametrize("inflate", [0, 1, 3])
def test_inflated_nodes_at_the_box_s_corners(inflate):
    nodes = nodes_of([(-30, -20), (30, 25), (-30, 25), (30, -20), (7, 7)])
    got = agree(nodes, [[0.0, 0.0, 0.0], [0.7, 0.6, 3.0]], 1081, max_range=2.0, inflate=inflate)
    side = 2 * inflate + 1
    assert list(got["stats"][2:]) == [5, 5 * side * side, -30 - inflate, -20 - inflate, 61 + 2 * inflate, 46 + 2 * inflate]


def test_nodes_that_do_not_qualify_and_a_node_off_the_lattice():
    nodes = nodes_of(ring(30, 3))
    extra = np.array([[0.2, 0.2, 0.0, np.nan], [np.nan, 0.1, 0.0, 4.0], [0.1, np.inf, 0.0, 4.0], [3.0e4, 0.0, 0.0, 4.0], [0.0, -2.7e4, 0.0, 4.0],
                      [0.26, 0.1137, 5.0, 4.0], [0.3, 0.3, 0.0, 0.5]], np.float32)
    all_nodes = np.concatenate([nodes, extra])
    got = agree(all_nodes, [[0.0, 0.0, 0.2]], 1081, max_range=2.0, inflate=0)
    assert got["stats"][2] == len(nodes) + 1, "only the node off the lattice (z = 5 is ignored) joins the ring"
    assert (got["cells"][0] == (10, 5)).all(axis=1).any(), "the node off the lattice lies in the cell (10, 5)"
    assert list(got["stats"][4:]) == [-30, -30, 61, 61]
    # exactly 2^20 cells out still qualifies (the raster is a key list: the box is 2^20 wide)
    far = np.concatenate([nodes, nodes_of([(1 << 20, 0)])])
    ras = CR.Raster(far, RES, 1.0, 0)
    assert ras.box == (-30, -30, (1 << 20) + 31, 61) and not ras.too_large()
    assert CR.Raster(np.concatenate([far, nodes_of([(0, 1 << 20)])]), RES, 1.0, 0).too_large()


def test_an_empty_raster_and_poses_that_are_not_finite():
    nodes = nodes_of(ring(10))
    got = agree(nodes, [[0.0, 0.0, 0.0]], 65, w_min=5.0, no_hit=np.nan)
    assert list(got["stats"]) == [65, 0, 0, 0, 0, 0, 0, 0] and np.isnan(got["ranges"]).all()
    poses = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, np.nan], [0.0, 0.0, -np.inf], [0.01, 0.0, 0.5]], np.float32)
    got = agree(nodes, poses, 65, max_range=1.0)
    assert (got["cells"][1:5] == CR.MISS).all() and (got["cells"][0] != CR.MISS).all() and (got["cells"][5] != CR.MISS).all()


def test_oblong_cells():
    res = (0.025, 0.05)
    nodes = nodes_of(ring(40), res=res)
    got = agree(nodes, [[0.0, 0.0, 0.0], [0.3, -0.7, 1.0], [1.5, 0.0, 3.0]], 1081, res=res, max_range=4.0)
    assert got["stats"][1] > 2000
    hit = got["cells"][0, :, 0] != CR.MISS
    assert hit.all() and got["ranges"][0].max() > 1.9, "the ring is 1 m away in x and 2 m in y"
    assert CR.refusal(1081, res=res) is None and "16384" in CR.refusal(1081, res=(0.001, 0.05))


# ---- what the feature is for --------------------------------------------------------------------------------------------------------------
POSES = [(0.5, 0.3, 0.1), (10.0, -8.0, 0.3)]


@pytest.fixture(scope="module", params=[4000, 100000])
def world(request, pkg):
    pts, segs = pkg.synth.make_map_points(request.param)
    truth = [pkg.synth.make_scan(segs, p, noise=0) for p in POSES]
    return {"n": request.param, "pts": pts, "truth": truth}


def measure(world, w_min, inflate):
    """(missed truth hits, truth hits, median |cast - truth| over the beams both hit) per pose."""
    out = []
    got = CR.cast_map(world["pts"], np.array(POSES, np.float32), 1081, max_range=30.0, w_min=w_min, inflate=inflate)
    for r, truth in enumerate(world["truth"]):
        t_hit = truth < 29.9
        c_hit = got["cells"][r, :, 0] != CR.MISS
        both = t_hit & c_hit
        out.append((int((t_hit & ~c_hit).sum()), int(t_hit.sum()), float(np.median(np.abs(got["ranges"][r][both].astype(np.float64) - truth[both])))))
    return out


def test_dense_walls_are_never_crossed_and_the_range_is_within_a_cell(world):
    for r, (missed, hits, med) in enumerate(measure(world, -113.0, 0)):
        print("dense %d points pose %d: missed %d of %d truth hits, median |cast - truth| %.4f m" % (world["n"], r, missed, hits, med))
        assert hits > 500 and missed == 0
        assert med <= 0.025 * math.sqrt(2.0)


def test_sparse_walls_need_inflate_1(pkg):
    """On the 4000-point map, where a beam that slips through a wall of which half the nodes qualify meets nothing behind it.  (On the
    100 000-point map it meets the next wall, so no beam counts as missed there: profiles/cast.txt.)"""
    pts, segs = pkg.synth.make_map_points(4000)
    small = {"n": 4000, "pts": pts, "truth": [pkg.synth.make_scan(segs, p, noise=0) for p in POSES]}
    m0, m1 = measure(small, 1.0, 0), measure(small, 1.0, 1)
    for r in range(len(POSES)):
        print("sparse 4000 points pose %d: inflate 0 missed %d of %d, inflate 1 missed %d of %d, median error at inflate 1 %.4f m"
              % (r, m0[r][0], m0[r][1], m1[r][0], m1[r][1], m1[r][2]))
        assert m0[r][0] > 0.20 * m0[r][1]
        assert m1[r][0] < 0.05 * m1[r][1]
