"""Scoring, the measurement stages and whole frames on UPLOADED maps and clouds at the limits of what pfslam_set_map and
pfslam_set_particles accept: map weights far above the +-113 the SLAM step produces, particle poses that are NaN, infinite or huge,
map nodes with such coordinates.

Every comparison is bit for bit against the CPU oracle (tests/oracle_lib.py; tests/resampler_ref.py for the resampler modes,
tests/estimate_ref.py for pfslam_estimate, tests/register_ref.py's brute force for pfslam_nearest).  No tolerance, never a second
product handle.  The one relaxation is same_bits_nan: where both sides hold a NaN its position must agree, its payload and sign need
not (x86 and gfx950 generate different default NaNs).  Integer outputs -- best, traces, sources, node indices -- are always exact.

Two tests of this file are not GPU tests and run with the CPU suite (hence a mark per test instead of a module-wide pytestmark):
test_the_inputs_test_what_they_claim evaluates on the oracle alone the condition that makes each case test what it says, and
test_the_thresholds_are_the_ones_the_code_has reads the thresholds back out of csrc/.

The edges (csrc/):
  A1  beams per chunk x largest |weight| <= 32767: 16-bit beam-chunk partials of the cell-row kernel (launch_score: p16; frame_v2_ok: the
      round-5 frame) | float partials, the staged chain.  5825 particles x 1081 beams score in chunks of 5 beams: 5 x 6553 | 5 x 6554
  A2  integral weights with |w| x n_beams <= 2^24 are summed chunk-wise, everything else in ONE chunk, the reference's beam order
      (upload_tree, score_chunks): 15520 | 15521 at 1081 beams, 8192 and 8193 (the older bound), 100.5
  A3  the same class across beam counts: weights up to 8191 are integral at 2048 beams and not at 2049, 3000 and 4096, where a
      particle's score passes 2^24 and a float32 sum of integers depends on its order
  A4  a map with a NaN or infinite weight is refused (pfslam_set_map names the node and keeps the loaded map): kernUpdateWeights
      converts the smallest fit to int (kernel.cu:297-304), which is undefined for a fit of -inf or NaN, and thrust::minmax_element's
      `<` never selects a NaN fit while the packed keys of k_minmax order NaN above +inf
  B   particles with NaN / +-inf / >= 1e6 coordinates, inside the first 1024 slots (cloud statistics, window origin: k_cell_count) and
      only beyond them; one slot, a whole wave (k_group_box: no plan, no box), all but one, all.  The map's root gets the map's lowest
      weight: a query that is NaN or infinite ends at the root, so such a particle scores low and is never the best
  C   map nodes (leaves, links untouched) with NaN / +-inf / 1e6 / 3e38 coordinates: no lattice rows, the shared-prefix plan; and a tree
      that GAINED non-finite nodes while the cell rows were live (kd_cells.hip.inc: dead records).  Under a pose that is +inf in x the
      frame's walls are inserted at (+inf, y); under a NaN pose none is: kernTestCorrespondance creates a node where
      `distance > minDist` (kernel.cu:1367-1379), false for a NaN distance, so no frame grows a NaN node.  Both are run

Mutations this file was checked against (each once, on a scratch copy of the library):
  the 16-bit bound raised to 65535 (launch_score and frame_v2_ok): the four A1 frame cases at +-6554 fail in their first frame (another
      best particle, hence another pose and wall list), and the four at +-6553 still pass; the stage calls pass on either side -- a
      stage call has no fused min / max and never takes 16-bit partials
  the `bad` ballot of k_group_box removed (bad = 0): NOT caught, by any B or C case.  fminf / fmaxf drop a NaN, so the group's box is
      that of its other lanes and the group gets its plan or its marked cells after all -- and the NaN lane loses nothing by it: every
      comparison of its query is false, the traversal never leaves the root whichever nodes a row offers it, and a NaN heading rejects
      every beam before the map is read.  An infinite pose makes the box infinite with or without the ballot (beam_box refuses it).  The
      ballot also raises the cloud's max |heading| to infinity (the guarded sine / cosine form); the lane it is raised for scores nothing.
      And the ballot stands inside `if (threadIdx.x == 0)`: only lane 0 is active there, so it has only ever seen lane 0's pose -- a NaN
      in lanes 1 .. 63 never withheld the plan, and for the reasons above never needed to
  the parent commit's class of integral weights (|w| <= 8192 whatever the beam count): A3 fails at 3000 and 4096 beams with 1100
      particles in variants 0, 2 and 3 -- every one of the 1100 fits, the first at particle 0 (24435848 for the oracle's 24435956 at 3000
      beams, 33363348 for 33363416 at 4096) -- and passes at 130 particles, where a chunk is one beam and chunk order is beam order;
      with it the three A4 cases (that library accepts the maps)
"""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import estimate_ref as E
import oracle_lib as O
import register_ref as G
import resampler_ref as R
from test_gpu_devlib_frames import environ
from test_gpu_frame import run_frames
from test_gpu_size_edges import oracle_measurement, score_chunks
from test_resampler_spec import skewed

gpu = pytest.mark.gpu          # (every test but the first two)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-icp-slam_amd", "csrc")
FIELDS = ("x", "y", "theta", "w")
NB = 1081
P16_MAX, SUM_EXACT, SPAN_MAX, STAT_SLOTS = 32767, 1 << 24, 1e6, 1024


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits_nan(a, b):
    """element-wise: the same bits, or a NaN on both sides (payload and sign of a NaN are the machine's)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


def assert_particles(got, want, what):
    for fld in FIELDS:
        bad = np.flatnonzero(~same_bits_nan(got[fld], want[fld]))
        assert len(bad) == 0, "%s: %d of %d particles differ in %s, first at %d" % (what, len(bad), len(want), fld, bad[0])


def assert_maps(got, want, what):
    """two node arrays (or their bytes): links and axes exactly, coordinates and weights with same_bits_nan"""
    got, want = [np.frombuffer(m, O.NODE_DTYPE) if isinstance(m, bytes) else m for m in (got, want)]
    assert len(got) == len(want), "%s: %d nodes, the oracle has %d" % (what, len(got), len(want))
    for fld in ("axis", "left", "right", "parent"):
        assert (got[fld] == want[fld]).all(), "%s: %s differs" % (what, fld)
    for fld in ("x", "y", "z", "w"):
        bad = np.flatnonzero(~same_bits_nan(got[fld], want[fld]))
        assert len(bad) == 0, "%s: %d nodes differ in %s, first at %d" % (what, len(bad), fld, bad[0])


def integral_class(w, nb):
    """upload_tree's class of a map, restated: every weight an integer and nb x largest |w| (at least the map update's clamp, 113) <= 2^24"""
    w = np.asarray(w, np.float64)
    return bool(np.isfinite(w).all() and (w == np.rint(w)).all() and max(np.abs(w).max(), 113.0) * nb <= SUM_EXACT)


def measured(h, p, fit, what):
    """pfslam_measurement_update behind a score against orc_minmax_first_f32 / orc_update_weights_f32"""
    imin, imax, fmin, fmax, want = oracle_measurement(p, fit)
    best, gmin, gmax = h.measurement_update()
    print("%s: best %d (oracle %d), fmin %r (%r), fmax %r (%r)" % (what, best, imax, gmin, float(fmin), gmax, float(fmax)))
    assert best == imax and bits(gmin) == bits(fmin) and bits(gmax) == bits(fmax), what
    bad = np.flatnonzero(~same_bits_nan(h.particles()["w"], want["w"]))
    assert len(bad) == 0, "%s: %d weights differ, first at %d" % (what, len(bad), bad[0])


def scored(h, fit, what):
    got = h.score_kd()
    bad = np.flatnonzero(~same_bits_nan(got, fit))
    print("%s: %d of %d fits differ%s" % (what, len(bad), len(fit), "" if not len(bad) else ", first at %d: %r vs the oracle's %r" % (bad[0], got[bad[0]], fit[bad[0]])))
    assert len(bad) == 0, "%s: %d of %d fits differ from the oracle's, first at particle %d: %r vs %r" % (what, len(bad), len(fit), bad[0], got[bad[0]], fit[bad[0]])


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        with environ(ORC_THREADS="16"):
            _CACHE[key] = make()
    return _CACHE[key]


def row_of(e):
    """run_frames' row of an engine: trace without Neff, then the pose bits"""
    t = e.trace()
    return [t["best"], t["resampled"], t["n_wall"], t["n_free"], t["n_insert"], t["kd_size"]] + bits(e.pose).tolist()


# ---- A. map weights ----------------------------------------------------------------------------------------------------------------------
A1_N = 5825
A1_W = (6553, 6554, -6553, -6554)
A2_EDGE = SUM_EXACT // NB                                   # 15520: the largest integral weight at 1081 beams
A2_W = (8192, -8192, 8193, A2_EDGE, -A2_EDGE, A2_EDGE + 1, 100.5)
A2_SIZES = ((65, 3), (300, 0), (A1_N, 0))                    # (particles, variant)
A3_BEAMS = (2048, 2049, 3000, 4096)
A3_NS = (130, 1100)     # 130 particles score one beam per chunk -- chunk partials added in chunk order ARE the beam order --, 1100 two or three
A3_GUARD = 12           # particles whose beams the guard adds up by hand (at 3000 and 4096 beams nearly every fit is inexact)


def a_scan(nb, seed=5):
    """ranges in [1, 15] m: |r cos|, |r sin| < 20, every beam is accepted whatever the heading"""
    return np.random.RandomState(seed).uniform(1.0, 15.0, nb).astype(np.float32)


def a_cloud(n):
    return O.add_noise(O.make_particles(n), 3)              # a few centimetres around the origin


def a_tree(world, W):
    """the 4000-point map with every weight W, a random tenth one smaller in magnitude (so that W is the largest magnitude)"""
    tree = world["tree"].copy()
    w = np.full(len(tree), W, np.float32)
    w[np.random.RandomState(7).uniform(size=len(tree)) < 0.1] = np.float32(W - np.sign(W))
    tree["w"] = w
    return tree


def a3_tree(world):
    """odd-heavy integers in [8100, 8191]"""
    tree = world["tree"].copy()
    rng = np.random.RandomState(9)
    w = rng.randint(8100, 8192, len(tree))
    odd = rng.uniform(size=len(tree)) < 0.75
    tree["w"] = np.where(odd, w | 1, w).astype(np.float32)
    return tree


def a_stage(world, W, n, nb=NB):
    def make():
        tree, p, scan = (a3_tree(world) if W == "a3" else a_tree(world, W)), a_cloud(n), a_scan(nb)
        p["w"] = np.random.RandomState(n).uniform(0.1, 1.0, n).astype(np.float32)
        return tree, p, scan, O.score_kd(tree, p, scan, threads=16)
    return cached(("a", W, n, nb), make)


def beam_weights(tree, p1, scan):
    """the map weight every accepted beam of one particle adds, in beam order (float64), through orc_traverse_batch on the oracle's end points"""
    L, x, y = O.lib(), C.c_float(), C.c_float()
    q = []
    for j, r in enumerate(scan):
        L.orc_clean_lidar_scan(j, float(r), float(p1["theta"]), C.byref(x), C.byref(y))
        if abs(x.value) < 20.0 and abs(y.value) < 20.0:
            q.append((np.float32(x.value) + np.float32(p1["x"]), np.float32(y.value) + np.float32(p1["y"]), 0.0))
    best, _ = O.traverse_batch(tree, np.array(q, np.float32))
    return tree["w"][best].astype(np.float64)


def a1_frames(world, W):
    def make():
        # a smooth closed room, ranges in [3, 13] m: neighbouring beams end in neighbouring cells, as a real scan's do (1081 independent
        # ranges put every beam's box into lattice cells of its own, the cell list fills up and the frames leave the rows for that reason)
        ang = np.radians(-135.0 + 0.25 * np.arange(NB))
        scans = [(8.0 + 5.0 * np.cos(3.0 * ang + 0.05 * f)).astype(np.float32) for f in range(6)]
        tree = a_tree(world, W)
        o = O.Slam(A1_N, kd_capacity=len(tree) + (1 << 16))
        o.set_map(tree)
        rows = []
        for i, s in enumerate(scans):
            o.step(6 + i, s)
            rows.append(row_of(o))
        out = {"tree": tree, "scans": scans, "rows": rows, "particles": o.particles().copy(), "map": o.tree().copy()}
        o.close()
        return out
    return cached(("a1f", W), make)


# ---- B. particle poses -------------------------------------------------------------------------------------------------------------------
NAN, INF = np.float32(np.nan), np.float32(np.inf)
B_SETS = ("P1", "P2", "P3", "P4", "P5", "P6", "P7", "P8")
B_STAGE = [(65, False), (130, False), (1100, False), (1100, True), (4700, False), (4700, True)]     # (particles, poison only beyond slot 1024)
B_FRAMES = [(130, 3, False), (1100, 3, False), (1100, 3, True), (4700, 0, False), (4700, 0, True)]   # (particles, variant, beyond)
B_FRAME_SETS = ("P1", "P2", "P3", "P4", "P6")
B_POSE = (0.1, -0.2, 0.3)                                   # where small_world's scan was taken


def poison(p, pset, beyond):
    """the poison sets of the module docstring, written into p; returns the poisoned slots"""
    n = len(p)
    base = STAT_SLOTS if beyond else 0
    assert not beyond or n > STAT_SLOTS + 64
    if pset == "P1":
        s = [base]; p["x"][s] = NAN
    elif pset == "P2":
        s = [n - 1 if (beyond or n <= STAT_SLOTS) else STAT_SLOTS - 1]; p["theta"][s] = NAN
    elif pset == "P3":
        s = [base + 64]; p["y"][s] = INF
    elif pset == "P4":
        s = [base + 5]; p["x"][s] = -INF; p["theta"][s] = INF
    elif pset == "P5":
        s = [base + 1, base + 2, base + 3]
        p["x"][s] = [np.nextafter(np.float32(1e6), np.float32(0)), 1e6, 3e38]
    elif pset == "P6":          # one whole wave
        s = list(range(base + 64, min(base + 128, n))) if not beyond else list(range(base, base + 64))
        p["x"][s] = NAN
    else:                       # P7: all (beyond: all behind slot 1024) but one, P8: all of them
        s = [k for k in range(base, n) if pset == "P8" or k != base + (n - base) // 2]
        p["x"][s] = NAN
    return np.array(s)


def b_tree(world):
    """the 4000-point map; the root -- where a NaN or infinite query ends -- and the nodes at the map's edge that queries from x >= 1e6
    end at (P5) hold the map's lowest weight"""
    def make():
        tree = world["tree"].copy()
        y = np.arange(-25.0, 25.0, 0.0125, dtype=np.float32)
        far = [O.traverse_batch(tree, np.stack([np.full_like(y, X), y, np.zeros_like(y)], axis=1))[0] for X in (1e6, 3e38)]
        tree["w"][np.concatenate([[0]] + far)] = tree["w"].min()
        return tree
    return cached("btree", make)


def b_cloud(n, pset, beyond):
    p = O.add_noise(O.make_particles(n, *B_POSE), 3)
    p["w"] = np.random.RandomState(n + 1).uniform(0.1, 1.0, n).astype(np.float32)
    slots = poison(p, pset, beyond)
    return p, slots


def b_grid(world):
    def make():
        grid = np.full((1600, 1600), -100, np.int8)
        pts = world["pts"]
        gx = np.round(0.5 * 40 / 0.025 + pts[:, 0] / 0.025).astype(int); gy = np.round(0.5 * 40 / 0.025 + pts[:, 1] / 0.025).astype(int)
        grid[gx, gy] = np.random.RandomState(4).randint(-113, 114, len(pts))
        return grid
    return cached("bgrid", make)


def b_stage(world, n, pset, beyond):
    def make():
        tree, scan = b_tree(world), world["scan"]
        p, slots = b_cloud(n, pset, beyond)
        fit = O.score_kd(tree, p, scan, threads=16)
        gfit = np.zeros(n, np.int32)
        patch = O.default_patch()
        O.lib().orc_score_grid(O.P(b_grid(world)), 1600, 1600, C.byref(patch), O.P(p), n, O.P(scan), NB, O.P(gfit))
        return {"tree": tree, "scan": scan, "p": p, "slots": slots, "fit": fit, "gfit": gfit}
    return cached(("b", n, pset, beyond), make)


def resample_cloud(n, pset, beyond):
    """skewed weights (Neff far below 0.7 n) on the poisoned cloud; the slot's own index in a coordinate the set leaves alone"""
    q, _ = b_cloud(n, pset, beyond)
    idx = "x" if pset == "P3" else "y"
    q[idx] = np.arange(n)
    q["w"] = skewed(n)["w"]
    return q, idx


def b_scans(world):
    return cached("bscans", lambda: [importlib.import_module("gpu-icp-slam_amd").synth.make_scan(
        world["segs"], (B_POSE[0] + 0.002 * i, B_POSE[1] + 0.001 * i, B_POSE[2] + 0.0004 * i), seed=3000 + i) for i in range(8)])


def dispersed(p):
    """run_frames disperses the uploaded cloud through frames 1 .. 5 before it steps"""
    p = p.copy()
    for f in range(1, 6):
        O.add_noise(p, f)
    return p


def b_frames(world, n, pset, beyond):
    def make():
        tree, scans = b_tree(world), b_scans(world)
        p, _ = b_cloud(n, pset, beyond)
        o = O.Slam(n, kd_capacity=len(tree) + (1 << 18))
        o.set_map(tree)
        o.set_particles(dispersed(p))
        rows, finite = [], True
        for i, s in enumerate(scans):
            o.step(6 + i, s)
            rows.append(row_of(o))
            finite = finite and bool(np.isfinite(o.pose).all())
        out = {"tree": tree, "scans": scans, "p": p, "rows": rows, "particles": o.particles().copy(), "map": o.tree().copy(), "finite": finite}
        o.close()
        return out
    return cached(("bf", n, pset, beyond), make)


def b_best_is_finite(world, n, pset, beyond):
    """the first frame's best particle, restated from the stage functions: finite (run_frames' rows carry the pose, not the particle)"""
    tree, scans = b_tree(world), b_scans(world)
    p = O.add_noise(dispersed(b_cloud(n, pset, beyond)[0]), 6)
    fit = O.score_kd(tree, p, scans[0], threads=16)
    best = oracle_measurement(p, fit)[1]
    return bool(np.isfinite([p[f][best] for f in ("x", "y", "theta")]).all()), best


# ---- C. map nodes ------------------------------------------------------------------------------------------------------------------------
C_KINDS = {"nan": [NAN], "+inf": [INF], "-inf": [-INF], "1e6": [np.float32(1e6)], "3e38": [np.float32(3e38)],
           "mixed": [NAN, INF, -INF, np.float32(1e6), np.float32(3e38), np.float32(-3e38)]}


def c_world(kind):
    def make():
        pkg = importlib.import_module("gpu-icp-slam_amd")
        pts, segs = pkg.synth.make_map_points(3000, seed=21)
        tree = pkg.kd_create(pts)
        clean = tree.copy()
        leaves = np.flatnonzero((tree["left"] < 0) & (tree["right"] < 0) & (tree["axis"] != 2))
        take = leaves[np.random.RandomState(3).choice(len(leaves), 12, replace=False)]
        vals = C_KINDS[kind]
        for k, i in enumerate(take):
            tree["x" if k % 2 == 0 else "y"][i] = vals[k % len(vals)]
        scan = pkg.synth.make_scan(segs, (0.0, 0.0, 0.0), seed=22)
        rng = np.random.RandomState(23)
        q = np.zeros((1500 + 4 * len(take), 3), np.float32)
        q[:1500, :2] = rng.uniform(-19, 19, (1500, 2))
        for k, i in enumerate(take):      # queries around the places the poisoned leaves were sorted to
            q[1500 + 4 * k:1504 + 4 * k, 0] = clean["x"][i] + rng.uniform(-0.05, 0.05, 4)
            q[1500 + 4 * k:1504 + 4 * k, 1] = clean["y"][i] + rng.uniform(-0.05, 0.05, 4)
        p = O.add_noise(O.make_particles(130), 3)
        start = np.array([0.01, -0.02, 0.005], np.float32)
        pose, dbg = O.icp(tree, np.zeros(3, np.float32), start, scan)
        return {"tree": tree, "take": take, "scan": scan, "q": q, "trav": O.traverse_batch(tree, q)[0], "p": p,
                "fit": O.score_kd(tree, p, scan, threads=16), "start": start, "icp": pose, "near": G.nearest(tree, q)}
    return cached(("c", kind), make)


C2_N = 1100


def c2_cloud(f):
    return O.add_noise(O.make_particles(C2_N), f)


C2_KINDS = {"nan": NAN, "+inf": INF}


def c2_run(eng, scans, kind):
    """three healthy frames, every x = NaN or +inf for one frame, a healthy cloud and five more frames; yields behind every frame"""
    for i, s in enumerate(scans):
        if i == 3:
            p = c2_cloud(3); p["x"] = C2_KINDS[kind]
            eng.set_particles(p)
        if i == 4:
            eng.set_particles(c2_cloud(4))
        eng.step(6 + i, s)
        yield i


def c2_oracle(kind):
    def make():
        pkg = importlib.import_module("gpu-icp-slam_amd")
        pts, segs = pkg.synth.make_map_points(2000, seed=1)
        tree = pkg.kd_create(pts)
        scans = [pkg.synth.make_scan(segs, (0.002 * i, 0.001 * i, 0.0004 * i), seed=2000 + i) for i in range(9)]
        o = O.Slam(C2_N, kd_capacity=len(tree) + (1 << 16), balance_period=0)
        o.set_map(tree)
        rows, nan_nodes = [], []
        for i in c2_run(o, scans, kind):
            t = o.trace()
            rows.append(([t["best"], t["resampled"], t["n_wall"], t["n_free"], t["n_insert"], t["kd_size"]], o.pose.copy(), np.float32(t["neff"])))
            nan_nodes.append(int((~np.isfinite(o.tree()["x"])).sum()))
        out = {"tree": tree, "scans": scans, "rows": rows, "nan_nodes": nan_nodes, "particles": o.particles().copy(), "map": o.tree().copy()}
        o.close()
        return out
    return cached(("c2", kind), make)


# ---- the two CPU tests -------------------------------------------------------------------------------------------------------------------
def test_the_thresholds_are_the_ones_the_code_has():
    """The constants the cases above sit on, read out of the sources: a threshold that moves takes this test with it."""
    hip = open(os.path.join(CSRC, "pfslam_hip.hip")).read()
    frame = open(os.path.join(CSRC, "pfslam_frame.hip.inc")).read()
    stages = open(os.path.join(CSRC, "pfslam_stages.hip.inc")).read()
    cells = open(os.path.join(CSRC, "kd_cells.hip.inc")).read()
    math = open(os.path.join(CSRC, "pf_math.h")).read()
    assert "(float)bpc * h->w_absmax <= %d.0f" % P16_MAX in hip and "(float)bpc * h->w_absmax <= %d.0f" % P16_MAX in frame
    assert len(re.findall(r"w_absmax <= (\d+)", hip + frame)) == 2
    assert "#define PF_SUM_EXACT %d.0f" % SUM_EXACT in hip
    assert "(double)wabs * (double)h->nb <= (double)PF_SUM_EXACT" in hip and "(double)st[2] * (double)h->nb <= (double)PF_SUM_EXACT" in stages
    assert "8192.0f" not in hip                                # (the bound that held for 1081 beams only)
    assert "if (!h->integral_w) chunks = 1;" in hip
    assert set(re.findall(r"< (1e6f)", hip + frame + cells)) == {"1e6f"} and float(SPAN_MAX) == 1e6
    assert "fabsf(mx) < 1e6f && fabsf(my) < 1e6f" in hip and "fabsf(wx) < 1e6f && fabsf(wy) < 1e6f" in cells and "fabsf(wxlo) < 1e6f" in cells
    assert "const int ns = min(n, %d); // cloud statistics" % STAT_SLOTS in hip
    assert "#define PF_SUM_THETA_MAX 1024.0f" in math and "!(fabs(T.a) < (double)PF_SUM_THETA_MAX)" in math
    assert "#define PF_LATTICE_KMAX (1 << 20)" in cells and "rx * (float)PF_LATTICE_KMAX" in hip
    assert "c.nb < 1 || c.nb > 4096" in hip or re.search(r"n_beams[^;\n]*4096", hip)      # the largest handle: A3's 4096 beams
    # the cases sit on both sides of each
    assert score_chunks(A1_N, NB) == (5, 217) and 217 < 256 and A1_N >= 4608
    assert 5 * 6553 <= P16_MAX < 5 * 6554
    assert A2_EDGE * NB <= SUM_EXACT < (A2_EDGE + 1) * NB and A2_EDGE == 15520
    assert 2048 * 8191 <= SUM_EXACT < 2049 * 8191


def test_the_inputs_test_what_they_claim(small_world):
    """Each case's condition, evaluated on the oracle alone (no GPU): if one cannot be met the INPUT changes, never the condition."""
    world = small_world
    # A1: whole chunks reach bpc x |W|, and W is the largest magnitude on either side of the 16-bit edge
    for W in A1_W:
        tree, p, scan, fit = a_stage(world, W, A1_N)
        assert np.abs(tree["w"]).max() == abs(W) and integral_class(tree["w"], NB)
        assert np.abs(fit).max() >= 0.9 * NB * abs(W), (W, np.abs(fit).max())
        assert (5 * abs(W) <= P16_MAX) == (abs(W) == 6553)
    # A2: the class the upload gives each map
    for W in A2_W:
        assert integral_class(a_tree(world, W)["w"], NB) == (float(W) == int(W) and abs(W) <= A2_EDGE), W
    # A3: the float32 fit differs from the exact sum of its beams for some particle at 3000 and 4096 beams, for none at 2048
    # -- and, at 1100 particles, from the sum of chunk partials the integral class would add up (130 particles: one beam per chunk)
    assert [score_chunks(130, nb)[0] for nb in A3_BEAMS] == [1, 1, 1, 1] and [score_chunks(1100, nb)[0] for nb in A3_BEAMS] == [2, 2, 3, 3]
    for nb in A3_BEAMS:
        for n in A3_NS:
            tree, p, scan, fit = a_stage(world, "a3", n, nb)
            assert tree["w"].min() >= 8100 and tree["w"].max() == 8191 and (tree["w"] % 2 == 1).mean() > 0.7
            assert integral_class(tree["w"], nb) == (nb == 2048), nb
            bpc = score_chunks(n, nb)[0]
            inexact = chunked = 0
            for i in range(A3_GUARD):
                w = beam_weights(tree, p[i], scan)
                assert len(w) == nb                                                      # every beam is accepted
                f32 = w.astype(np.float32)
                assert bits(np.cumsum(f32)[-1:]) == bits(fit[i:i + 1])                   # (the helper restates the oracle's sum)
                inexact += float(fit[i]) != w.sum()
                parts = np.array([np.cumsum(f32[c:c + bpc])[-1] for c in range(0, nb, bpc)], np.float32)
                chunked += int(bits(np.cumsum(parts)[-1:])[0] != bits(fit[i:i + 1])[0])
            print("A3, %d beams, %d particles: of the first %d oracle fits %d are not the exact sum, %d not the sum of %d-beam chunks"
                  % (nb, n, A3_GUARD, inexact, chunked, bpc))
            if nb == 2048:
                assert inexact == 0 and chunked == 0 and nb * tree["w"].max() <= SUM_EXACT     # (no partial sum of any particle can round)
            elif nb >= 3000:
                assert inexact >= 1, nb
                assert n == 130 or chunked >= 1, (nb, n)
    # B, stage calls: a poisoned particle is never the best (P8 has no other), and the resampling cloud resamples
    tree = b_tree(world)
    assert tree["w"][0] == tree["w"].min() and tree["parent"][0] == -1
    for n, beyond in B_STAGE:
        for pset in B_SETS:
            d = b_stage(world, n, pset, beyond)
            assert (d["slots"] >= STAT_SLOTS).all() if beyond else (d["slots"] < STAT_SLOTS).any(), (n, pset, d["slots"])
            assert np.isfinite(d["fit"]).all()
            if pset != "P8":
                imin, imax = oracle_measurement(d["p"], d["fit"])[:2]
                assert imax not in set(d["slots"].tolist()), (n, pset, beyond, imax)
                q, _ = resample_cloud(n, pset, beyond)
                assert R.sums_and_cdf(q["w"])[0] < 0.7 * n
    # B, frames: the best particle of the first frame and the pose of every frame are finite
    for n, variant, beyond in B_FRAMES:
        for pset in B_FRAME_SETS:
            ok, best = b_best_is_finite(world, n, pset, beyond)
            d = b_frames(world, n, pset, beyond)
            assert ok and best == d["rows"][0][0] and d["finite"], (n, pset, beyond)
            assert np.isfinite([d["particles"][f][r[0]] for r in d["rows"][-1:] for f in ("x", "y", "theta")]).all()
    # C1: leaves only, links untouched
    for kind in C_KINDS:
        d = c_world(kind)
        t = d["tree"]
        assert (t["left"][d["take"]] == -1).all() and (t["right"][d["take"]] == -1).all()
        assert (~np.isfinite(t["x"]) | ~np.isfinite(t["y"]) | (np.abs(t["x"]) >= 1e6) | (np.abs(t["y"]) >= 1e6)).sum() == len(d["take"])
    # C2: under the +inf cloud the poisoned frame inserts, and the oracle's tree holds non-finite nodes from it on.  Under the NaN cloud
    # it has walls and inserts none: kernTestCorrespondance creates a node where `distance > minDist` (kernel.cu:1367-1379), which a NaN
    # distance never is -- no input grows a NaN node, an infinite one is the only non-finite node a frame can insert
    d = c2_oracle("+inf")
    assert d["rows"][3][0][4] > 0 and d["nan_nodes"][2] == 0 and d["nan_nodes"][3] >= 1, (d["rows"][3], d["nan_nodes"])
    assert np.isposinf(d["rows"][3][1][0]) and np.isposinf(d["map"]["x"]).sum() == d["nan_nodes"][-1]
    d = c2_oracle("nan")
    assert np.isnan(d["rows"][3][1][0]) and d["rows"][3][0][2] > 0 and d["rows"][3][0][4] == 0 and d["nan_nodes"][-1] == 0, d["rows"][3]


# ---- A on the GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", A1_W)
@gpu
def test_a1_stage_calls_on_either_side_of_the_16_bit_partials(pkg, small_world, W):
    """5825 particles x 1081 beams, chunks of 5 beams, the cell rows: 5 x 6553 fits a 16-bit partial, 5 x 6554 does not."""
    tree, p, scan, fit = a_stage(small_world, W, A1_N)
    h = pkg.PfSlam(A1_N, kd_capacity=len(tree) + 4096)
    h.set_map(tree); h.set_particles(p); h.set_scan(scan)
    scored(h, fit, "A1 W %d" % W)
    assert h.cell_stats()["rows"] > 0
    measured(h, p, fit, "A1 W %d" % W)
    h.close()


@pytest.mark.parametrize("serial", [False, True], ids=["concurrent", "serial"])
@pytest.mark.parametrize("W", A1_W)
@gpu
def test_a1_frames_on_either_side_of_the_16_bit_partials(pkg, small_world, W, serial):
    """6 frames of pfslam_step with the cell rows forced (variant 3) against O.Slam: round-5 frames at +-6553, the staged chain at +-6554."""
    d = a1_frames(small_world, W)
    h = pkg.PfSlam(A1_N, kd_capacity=len(d["tree"]) + (1 << 16))
    h.set_map(d["tree"]); h.set_variant(3)
    if serial:
        h.set_serial(1)
    for i, s in enumerate(d["scans"]):
        h.step(6 + i, s)
        assert row_of(h) == d["rows"][i], "W %d frame %d: %s vs the oracle's %s" % (W, 6 + i, row_of(h), d["rows"][i])
        assert h.frame_mode()["round5_frame"] == (abs(W) == 6553), (W, i, h.frame_mode(), h.cell_stats())
    assert_particles(h.particles(), d["particles"], "A1 frames W %d" % W)
    assert_maps(h.map(), d["map"], "A1 frames W %d" % W)
    h.close()


@pytest.mark.parametrize("n,variant", A2_SIZES)
@gpu
def test_a2_integral_and_other_weights(pkg, small_world, n, variant):
    """+-8192 and +-15520 are summed chunk-wise, 15521 and 100.5 in one chunk; 8193 was the older bound's first non-integral weight."""
    for W in A2_W:
        tree, p, scan, fit = a_stage(small_world, W, n)
        h = pkg.PfSlam(n, kd_capacity=len(tree) + 4096)
        h.set_variant(variant)
        h.set_map(tree); h.set_particles(p); h.set_scan(scan)
        scored(h, fit, "A2 n %d W %s" % (n, W))
        measured(h, p, fit, "A2 n %d W %s" % (n, W))
        h.close()


def a3_check(pkg, world, variants):
    failed = []
    for nb in A3_BEAMS:
        for n in A3_NS:
            tree, p, scan, fit = a_stage(world, "a3", n, nb)
            for variant in variants:
                h = pkg.PfSlam(n, n_beams=nb, kd_capacity=len(tree) + 4096)
                h.set_variant(variant)
                h.set_map(tree); h.set_particles(p); h.set_scan(scan)
                what = "A3 %d beams %d particles variant %d" % (nb, n, variant)
                try:
                    scored(h, fit, what)
                    measured(h, p, fit, what)
                except AssertionError as e:
                    failed.append(str(e).splitlines()[0])
                h.close()
    assert not failed, "\n".join(failed)


@gpu
def test_a3_beam_count_times_weight_against_2_to_the_24(pkg, small_world):
    """130 and 1100 particles, weights in [8100, 8191], 2048 | 2049 | 3000 | 4096 beams, variants 0, 2 and 3: from 2049 beams on a score can
    pass 2^24 and only the reference's own beam order gives the reference's float32 sum."""
    a3_check(pkg, small_world, (0, 2, 3))


@gpu
def test_a3_with_the_organisation_forced_at_every_count():
    """The same under PFSLAM_PLAN_MIN_N=1 (read once per process, hence a child): variant 0 is organised at 130 particles too."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PFSLAM_PLAN_MIN_N="1"))
    assert out.returncode == 0 and "a3 ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.parametrize("kind", ["nan", "+inf", "+-inf"])
@gpu
def test_a4_a_map_with_a_non_finite_weight_is_refused(pkg, small_world, kind):
    """pfslam_set_map names the node and leaves the handle as it was (tests/test_gpu_edges.py: refused maps)."""
    tree, scan = small_world["tree"], small_world["scan"]
    h = pkg.PfSlam(32, kd_capacity=len(tree) + 8)
    h.set_map(tree)
    p = O.make_particles(32, 0.1, 0.1, 0.1)
    h.set_particles(p); h.set_scan(scan)
    before = h.score_kd()
    assert (bits(before) == bits(O.score_kd(tree, p, scan))).all()
    bad = tree.copy()
    at = len(bad) // 3
    bad["w"][at] = {"nan": NAN, "+inf": INF, "+-inf": -INF}[kind]
    if kind == "+-inf":
        bad["w"][at + 7] = INF
    with pytest.raises(pkg.PfSlamError, match=r"node %d\b.*weight" % at):
        h.set_map(bad)
    assert h.kd_size == len(tree) and h.map().tobytes() == tree.tobytes()
    assert (bits(h.score_kd()) == bits(before)).all()
    h.close()


# ---- B on the GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,beyond", B_STAGE, ids=lambda v: str(v))
@gpu
def test_b_stage_calls_on_poisoned_clouds(pkg, small_world, n, beyond):
    """Every poison set: pfslam_score_kd in variants 0, 2, 3, 4 (variant 0 alone at 4700), pfslam_measurement_update, the 2-D measurement,
    pfslam_motion_update, pfslam_resample in modes 0 .. 2 (sources exact) and pfslam_estimate."""
    patch = O.default_patch()
    for pset in B_SETS:
        d = b_stage(small_world, n, pset, beyond)
        tree, scan, p, fit = d["tree"], d["scan"], d["p"], d["fit"]
        what = "B %s n %d%s" % (pset, n, " beyond" if beyond else "")
        for variant in ((0, 2, 3, 4) if n <= 1100 else (0,)):
            h = pkg.PfSlam(n, kd_capacity=len(tree) + 4096)
            h.set_variant(variant)
            h.set_map(tree); h.set_particles(p); h.set_scan(scan)
            scored(h, fit, "%s variant %d" % (what, variant))
            if h.cell_stats()["rows"] > 0:
                assert pset in ("P7", "P8") or h.check_cells()["violations"] == 0, (what, variant, h.check_cells())
            measured(h, p, fit, "%s variant %d" % (what, variant))    # (P8 inside: every fit is the same, a range of zero)
            h.close()
        h = pkg.PfSlam(n, kd_capacity=4096)
        # the 2-D measurement: score, int min / max / first argmax, weights
        h.set_grid(b_grid(small_world)); h.set_particles(p); h.set_scan(scan)
        gfit = d["gfit"]
        assert (h.score_grid() == gfit).all(), what
        imin, imax = C.c_int(), C.c_int()
        O.lib().orc_minmax_first_i32(O.P(gfit), n, C.byref(imin), C.byref(imax))
        rng = int(gfit[imax.value]) - int(gfit[imin.value])
        wp = p.copy()
        if rng > 0:
            O.lib().orc_update_weights_i32(O.P(wp), n, O.P(gfit), float(np.float32(1) / np.float32(rng)), int(gfit[imin.value]))
        assert_particles(h.particles(), wp, what + " 2-D weights")
        # dispersion
        h.set_particles(p)
        h.motion_update(7)
        assert_particles(h.particles(), O.add_noise(p.copy(), 7), what + " motion")
        # resampling and the estimate
        q, idx = resample_cloud(n, pset, beyond)
        h.set_particles(q)
        got16, want16 = h.estimate_raw(), E.estimate_particles(q)
        assert same_bits_nan(got16, want16).all(), "%s estimate: %s vs %s" % (what, got16.tolist(), want16.tolist())
        for mode in (0, 1, 2):
            did, neff, src = R.resample_ref(q, 17, mode)
            h.set_resampler(mode)
            h.set_particles(q)
            did_g, neff_g = h.resample(17)
            assert did == 1 and did_g == 1 and bits(neff_g) == bits(neff), (what, mode, did_g, neff_g, neff)
            got = h.particles()
            bad = int((got[idx] != src.astype(np.float32)).sum())
            assert bad == 0, "%s mode %d: %d sources differ from the restatement" % (what, mode, bad)
            for fld in ("x", "y", "theta"):
                assert same_bits_nan(got[fld], q[fld][src]).all(), (what, mode, fld)
            assert (got["w"] == 1).all()
        h.close()


@pytest.mark.parametrize("pset", B_FRAME_SETS)
@pytest.mark.parametrize("n,variant,beyond", B_FRAMES, ids=lambda v: str(v))
@gpu
def test_b_frames_on_poisoned_clouds(pkg, small_world, n, variant, beyond, pset):
    """8 KD frames (run_frames: the uploaded cloud dispersed through frames 1 .. 5, then frames 6 .. 13) against O.Slam, four streams and
    one: trace and pose of every frame, particles, map, and the cell rows' invariants."""
    d = b_frames(small_world, n, pset, beyond)
    for serial in (False, True):
        rows, p, m, book, chk = run_frames(pkg, d["tree"], d["scans"], n, serial, variant=variant, look_every=1,
                                           prepare=lambda h: h.set_particles(d["p"]))
        rows = rows[:len(d["rows"])]       # (run_frames appends the last frame's row once more)
        for i, (g, w) in enumerate(zip(rows, d["rows"])):
            assert g == w, "B frames %s n %d serial %d frame %d: %s vs the oracle's %s" % (pset, n, serial, 6 + i, g, w)
        what = "B frames %s n %d%s serial %d" % (pset, n, " beyond" if beyond else "", serial)
        assert_particles(p, d["particles"], what)
        assert_maps(m, d["map"], what)
        assert chk["violations"] == 0, (what, chk)


# ---- C on the GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(C_KINDS))
@gpu
def test_c1_stage_calls_on_a_map_with_poisoned_leaves(pkg, kind):
    """pfslam_traverse, pfslam_score_kd in variants 0, 2, 3, 4, pfslam_icp and pfslam_nearest on a tree twelve of whose leaves hold a NaN,
    an infinity, 1e6 or 3e38 in x or y."""
    d = c_world(kind)
    tree = d["tree"]
    for variant in (0, 2, 3, 4):
        h = pkg.PfSlam(len(d["p"]), kd_capacity=len(tree) + 4096)
        h.set_variant(variant)
        h.set_map(tree); h.set_particles(d["p"]); h.set_scan(d["scan"])
        scored(h, d["fit"], "C1 %s variant %d" % (kind, variant))
        assert h.cell_stats()["rows"] == 0                    # (off the lattice: never the cell rows)
        if variant == 0:
            assert (h.traverse(d["q"]) == d["trav"]).all(), kind
            pose, _ = h.icp(d["start"])
            assert same_bits_nan(pose, d["icp"]).all(), (kind, pose, d["icp"])
            best, d2 = h.nearest(d["q"])
            assert (best == d["near"][0]).all() and (bits(d2) == bits(d["near"][1])).all(), kind
            assert not set(best.tolist()) & set(d["take"].tolist()) or kind in ("1e6", "3e38")
        h.close()


@pytest.mark.parametrize("serial", [False, True], ids=["concurrent", "serial"])
@pytest.mark.parametrize("kind", list(C2_KINDS))
@gpu
def test_c2_cell_rows_over_a_tree_that_gained_non_finite_nodes(pkg, kind, serial):
    """1100 particles, cell rows forced, no re-balance: three healthy frames, one frame from a cloud whose every x is +inf (its pose is
    +inf in x, its walls are inserted at (+inf, y)) or NaN (walls at (NaN, y), none inserted: the reference's `distance > minDist`), five
    frames from a healthy cloud -- against O.Slam frame by frame."""
    d = c2_oracle(kind)
    h = pkg.PfSlam(C2_N, kd_capacity=len(d["tree"]) + (1 << 16), balance_period=0)
    h.set_map(d["tree"]); h.set_variant(3)
    if serial:
        h.set_serial(1)
    for i in c2_run(h, d["scans"], kind):
        t = h.trace()
        got = [t["best"], t["resampled"], t["n_wall"], t["n_free"], t["n_insert"], t["kd_size"]]
        want, pose, neff = d["rows"][i]
        assert got == want, "C2 frame %d: %s vs the oracle's %s" % (6 + i, got, want)
        assert same_bits_nan(h.pose, pose).all(), (i, h.pose, pose)
        assert same_bits_nan(np.float32(t["neff"]), neff).all(), (i, t["neff"], neff)
    assert_particles(h.particles(), d["particles"], "C2")
    assert_maps(h.map(), d["map"], "C2")
    chk = h.check_cells()
    assert chk["violations"] == 0, chk
    h.close()


if __name__ == "__main__":     # test_a3_with_the_organisation_forced_at_every_count's child
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    _pkg = importlib.import_module("gpu-icp-slam_amd")
    _pts, _segs = _pkg.synth.make_map_points(4000, seed=11)     # tests/conftest.py: small_world
    a3_check(_pkg, {"tree": _pkg.kd_create(_pts)}, (0, 3))
    print("a3 ok")
