"""The restatement of pfslam_cast_score (tests/cast_score_ref.py) pinned against an independent beam-by-beam Python loop on the ring maps of
tests/test_cast_spec.py, with scans that land on every edge of the specification; then what the feature is for: on the synthetic map the
beam model picks the true pose among displaced ones, on dense and on sparse walls.  No GPU needed."""
import math

import numpy as np
import pytest

import cast_ref as CR
import cast_score_ref as SR
from test_cast_spec import RES, loop_cast, nodes_of, ring

F = np.float32


def loop_score(nodes, poses, scan, nb, res=RES, cast=None, **opts):
    """pfslam_cast_score beam by beam: one float32 operation at a time on scalars, Python integers for the sums."""
    o = SR.options(**opts)
    c = loop_cast(nodes, poses, nb, res, **(cast or {}))
    tol, zmin, zmax = F(o["tol"]), F(o["z_min"]), F(o["z_max"])
    u = tol * F(0.0625)
    qcap = int(np.rint(F(o["clip"]) / u))
    assert 16 <= qcap <= 32767
    rows, classes = [], []
    for r in range(len(c["ranges"])):
        n = [0] * 8
        cl = []
        for b in range(nb):
            z, e = F(scan[b]), c["ranges"][r, b]
            hit = c["cells"][r, b, 0] != CR.MISS
            if not (z >= zmin and z <= zmax):
                cl.append(0)
                continue
            n[0] += 1
            if not hit:
                n[4] += 1
                cl.append(1)
                continue
            with np.errstate(all="ignore"):
                d = z - e
                a = np.abs(d)
                fq = float(np.rint(a / u))
            q = qcap if fq >= float(qcap) else int(fq)
            k = 2 if a <= tol else (3 if d > tol else 4)
            cl.append(k)
            n[k - 1] += 1
            n[5] += q
            if k == 2:
                assert q <= 16
                n[6] += q * q
        n[7] = n[5] + (qcap * n[4] if o["count_miss"] else 0)
        rows.append(n)
        classes.append(cl)
    best = -1
    for r, n in enumerate(rows):
        if n[1] > 0 and (best < 0 or n[7] < rows[best][7] or (n[7] == rows[best][7] and n[1] > rows[best][1])):
            best = r
    return {"rows": np.array(rows, np.int64), "classes": np.array(classes, np.uint8), "best": best, "stats": c["stats"], "ranges": c["ranges"],
            "cells": c["cells"]}


def agree(nodes, poses, scan, nb, res=RES, cast=None, **opts):
    want = loop_score(nodes, poses, scan, nb, res, cast, **opts)
    got = SR.score_map(nodes, poses, scan, nb, res, cast=cast, **opts)
    assert SR.same(got, want) is None, SR.same(got, want)
    return got, want


RING = dict(max_range=3.0)


def expected(nodes, pose, nb):
    return loop_cast(nodes, [pose], nb, **RING)["ranges"][0]


def test_the_tolerance_is_closed_and_one_ulp_above_it_is_outside():
    nodes = nodes_of(ring(60))
    pose = [0.05, -0.02, 0.3]
    e = expected(nodes, pose, 65)
    scan = e.copy()
    scan[10], scan[20] = e[10] + F(0.1), e[20] - F(0.1)
    # z lies within a factor of two of e, so z - e is exact: a tolerance of exactly that residual, and the float below it
    a10, a20 = F(scan[10] - e[10]), F(e[20] - scan[20])
    assert a10 > 0 and a20 > 0
    got, _ = agree(nodes, [pose], scan, 65, cast=RING, tol=float(a10))
    assert got["classes"][0, 10] == 2
    got, _ = agree(nodes, [pose], scan, 65, cast=RING, tol=float(np.nextafter(a10, F(0))))
    assert got["classes"][0, 10] == 3, "one ulp above the tolerance, behind the wall: through"
    got, _ = agree(nodes, [pose], scan, 65, cast=RING, tol=float(a20))
    assert got["classes"][0, 20] == 2
    got, _ = agree(nodes, [pose], scan, 65, cast=RING, tol=float(np.nextafter(a20, F(0))))
    assert got["classes"][0, 20] == 4, "one ulp above the tolerance, in front of the wall: short"
    assert got["rows"][0, 0] == 65 and got["rows"][0, 1] >= 63
    # a == tol is 16 units exactly: Q2 counts 256 for it
    got, _ = agree(nodes, [pose], np.where(np.arange(65) == 10, scan, e), 65, cast=RING, tol=float(a10))
    assert got["rows"][0].tolist() == [65, 65, 0, 0, 0, 16, 256, 16]


def test_the_ends_of_the_valid_interval_and_ranges_that_are_no_numbers():
    nodes = nodes_of(ring(60))
    pose = [0.0, 0.0, 0.0]
    e = expected(nodes, pose, 65)
    scan = e.copy()
    zmin, zmax = F(1.2), F(1.9)
    scan[0], scan[1] = zmin, np.nextafter(zmin, F(0))
    scan[2], scan[3] = zmax, np.nextafter(zmax, F(9))
    scan[4], scan[5], scan[6], scan[7] = np.nan, np.inf, -np.inf, -1.5
    got, _ = agree(nodes, [pose], scan, 65, cast=RING, z_min=float(zmin), z_max=float(zmax))
    cl = got["classes"][0]
    assert cl[0] != 0 and cl[1] == 0 and cl[2] != 0 and cl[3] == 0 and (cl[4:8] == 0).all()
    assert got["rows"][0, 0] == int((cl != 0).sum()) and got["rows"][0, 0] < 65


def test_a_residual_that_saturates_and_one_beyond_every_integer():
    nodes = nodes_of(ring(60))
    pose = [0.0, 0.0, 0.0]
    e = expected(nodes, pose, 65)
    scan = e.copy()
    scan[5] = e[5] + F(0.99)                 # below clip: 158 units
    scan[6] = e[6] + F(1.01)                 # above clip: saturates at qcap = 160
    scan[7] = F(5.0e8)                       # a / u is 8e10, beyond 2^31: the compare comes before the conversion
    scan[8] = F(3.0e38)                      # a / u overflows to infinity
    scan[9] = F(0.2)                         # short of the wall by more than clip
    got, want = agree(nodes, [pose], scan, 65, cast=RING, z_max=3.3e38)
    assert got["qcap"] == 160
    assert F(5.0e8) / got["u"] > 2.0**31
    assert got["classes"][0, 5:10].tolist() == [3, 3, 3, 3, 4]
    assert got["rows"][0].tolist() == [65, 60, 4, 1, 0, 158 + 4 * 160, 0, 158 + 4 * 160]
    # the largest qcap and the smallest tolerance
    got, _ = agree(nodes, [pose], scan, 65, cast=RING, z_max=3.3e38, tol=1e-4, clip=0.2)
    assert got["qcap"] == 32000
    assert SR.refusal(65, tol=1e-4, clip=0.21) == "must be 16 .. 32767" and SR.refusal(65, clip=0.09) == "must be 16 .. 32767"
    assert SR.refusal(65, tol=0.5, clip=0.5) is None and SR.unit(0.5, 0.5)[1] == 16


def test_rays_that_miss_with_and_without_their_cost_and_a_pose_that_is_not_finite():
    nodes = nodes_of(ring(20))
    poses = np.array([[0.0, 0.0, 0.0], [2.0, 0.1, math.pi], [np.nan, 0.0, 0.0], [0.0, 0.0, np.inf], [40.0, 40.0, 0.0]], np.float32)
    scan = np.full(1081, 0.5, np.float32)
    scan[::7] = np.nan
    valid = int(np.isfinite(scan).sum())
    g1, _ = agree(nodes, poses, scan, 1081, cast=dict(max_range=5.0), count_miss=1)
    g0, _ = agree(nodes, poses, scan, 1081, cast=dict(max_range=5.0), count_miss=0)
    assert (g1["rows"][:, 0] == valid).all()
    assert 0 < g1["rows"][1, 4] < valid, "seen from outside the ring fills a part of the fan"
    for r in (2, 3, 4):
        assert g1["rows"][r].tolist() == [valid, 0, 0, 0, valid, 0, 0, 160 * valid] and g0["rows"][r].tolist() == [valid, 0, 0, 0, valid, 0, 0, 0]
        assert set(g1["classes"][r].tolist()) == {0, 1}
    assert (g1["rows"][:, :7] == g0["rows"][:, :7]).all() and (g0["rows"][:, 7] == g0["rows"][:, 5]).all()
    assert (g1["rows"][:, 7] == g1["rows"][:, 5] + 160 * g1["rows"][:, 4]).all()
    assert g1["stats"][1] == (g1["classes"][:, ~np.isnan(scan)] > 1).sum() + (CR.cast_map(nodes, poses, 1081, max_range=5.0)["cells"][:, np.isnan(scan), 0] != CR.MISS).sum()
    assert g1["best"] == 0 and g0["best"] == 0


def test_no_valid_beam_no_pick_and_ties_go_to_agree_and_then_to_the_row():
    nodes = nodes_of(ring(60))
    pose = [0.0, 0.0, 0.0]
    e = expected(nodes, pose, 65)
    got, _ = agree(nodes, [pose, pose], np.full(65, np.nan, np.float32), 65, cast=RING)
    assert got["best"] == -1 and not got["rows"].any() and not got["classes"].any()
    got, _ = agree(nodes, [pose, pose], np.full(65, 2.9, np.float32), 65, cast=RING)
    assert got["best"] == -1 and (got["rows"][:, 0] == 65).all() and (got["rows"][:, 1] == 0).all(), "valid beams, none agrees: no row is eligible"
    # equal poses tie on everything: the lowest row
    got, _ = agree(nodes, [[9.0, 9.0, 0.0], pose, pose], e, 65, cast=RING)
    assert got["best"] == 1
    # the pick from rows alone: cost first, then agree, then the row
    rows = np.zeros((5, 8), np.int64)
    rows[:, 1], rows[:, 7] = [0, 3, 5, 5, 9], [0, 7, 7, 7, 8]
    assert SR.best_of(rows) == 2
    rows[0, 1] = 1
    assert SR.best_of(rows) == 0
    rows[:, 1] = 0
    assert SR.best_of(rows) == -1


def test_oblong_cells_and_the_cast_s_options():
    res = (0.025, 0.05)
    nodes = nodes_of(ring(40), res=res)
    poses = [[0.0, 0.0, 0.0], [0.3, -0.7, 1.0]]
    e = loop_cast(nodes, [poses[0]], 257, res, max_range=4.0)["ranges"][0]
    got, _ = agree(nodes, poses, e, 257, res=res, cast=dict(max_range=4.0))
    assert got["rows"][0].tolist() == [257, 257, 0, 0, 0, 0, 0, 0] and got["best"] == 0 and got["rows"][1, 1] < 257
    got, _ = agree(nodes, poses, e, 257, res=res, cast=dict(max_range=4.0, inflate=2, skip_cells=0, w_min=5.0))
    assert (got["rows"][:, 4] == 257).all(), "no node qualifies: every valid beam misses"


def test_the_refusals_in_their_order():
    R = SR.refusal
    assert R(65, m=0) == R(65, m=65537, source=7) == "m must be 1 .. 65536"
    assert R(4097, source=7) == "n_beams must be <= 4096" and R(4096) is None
    assert R(65, source=2, poses=False, m=3) == R(65, source=-1) == "source must be 0 .. 1"
    assert R(65, m=2, poses=False, classes=True, tol=0.0) == "needs m == 1" and R(65, m=1, poses=False) is None
    assert R(65, m=300, source=1, n_particles=300) == "needs poses NULL and m == n_particles"
    assert R(65, m=299, source=1, poses=False, n_particles=300) == "needs poses NULL and m == n_particles"
    assert R(65, m=300, source=1, poses=False, n_particles=300) is None
    assert R(1081, m=65536, classes=True, cast=dict(inflate=9)) == "more than 2^24 rays" and R(1081, m=65536) is None
    assert R(65, cast=dict(inflate=9), tol=0.0) == "inflate must be 0 .. 8" and R(65, cast_reserved=1, tol=0.0) == "reserved_ must be 0"
    assert R(65, tol=0.0, clip=np.inf) == R(65, tol=np.nan) == R(65, tol=9.9e-5) == "tol must be finite and >= 1e-4"
    assert R(65, clip=np.inf, z_min=np.nan) == "clip must be finite"
    assert R(65, z_min=2.0, z_max=1.0, count_miss=2) == R(65, z_max=np.inf) == "z_min and z_max must be finite, z_min <= z_max"
    assert R(65, z_min=1.0, z_max=1.0) is None
    assert R(65, count_miss=2, reserved=1) == "count_miss must be 0 or 1" and R(65, reserved=1, clip=0.0) == "reserved_ must be 0"
    assert R(65, clip=0.0, have_map=False) == R(65, clip=-1.0) == "must be 16 .. 32767"
    assert R(65, have_map=False) == "no map loaded"
    with pytest.raises(TypeError):
        R(65, no_hit=1.0)


# ---- what the feature is for --------------------------------------------------------------------------------------------------------------
TRUE = (0.5, 0.3, 0.1)
POSES = [TRUE, (0.8, 0.3, 0.1), (0.5, -0.2, 0.1), (0.5, 0.3, 0.15), (3.5, 0.3, 0.1), (10.0, -8.0, 0.3)]


@pytest.mark.parametrize("walls,cast,share", [("dense", dict(w_min=-113.0, inflate=0), 0.95), ("sparse", {}, 0.90)])
def test_the_beam_model_picks_the_true_pose_among_displaced_ones(pkg, walls, cast, share):
    pts, segs = pkg.synth.make_map_points(4000)
    scan = pkg.synth.make_scan(segs, TRUE, noise=0)
    got = SR.score_map(pts, np.array(POSES, np.float32), scan, 1081, cast=cast)
    rows = got["rows"]
    others = rows[1:]
    print("%s walls: agree at the true pose %d of %d, through %d, cost %d; costs of the other five %d .. %d, fewest through among them %d"
          % (walls, rows[0, 1], rows[0, 0], rows[0, 2], rows[0, 7], others[:, 7].min(), others[:, 7].max(), others[:, 2].min()))
    for r, p in enumerate(POSES):
        print("   %-18r %s" % (p, " ".join("%s %d" % (k, v) for k, v in zip(SR.COLUMNS, rows[r]))))
    assert rows[0, 0] == 805 and (rows[:, 0] == 805).all()
    assert got["best"] == 0
    assert rows[0, 1] >= share * rows[0, 0]
    assert (others[:, 2] > rows[0, 2]).all()
