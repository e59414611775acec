"""The round-5 frame's wall list -- k_wall_runs -> k_walls_rank_traverse<true> -> k_walls<3> (csrc/pfslam_frame.hip.inc) -- at its sort,
duplicate and beam-count edges, through whole frames of pfslam_step against the CPU oracle (tests/oracle_lib.py, O.Slam.step).

Everything is bit for bit; there is no tolerance anywhere in this file.  After EVERY frame: the trace, the pose bits and the ORDERED wall
and free cell lists (pfslam_get_cells), and from frame 2 on that the frame ran as a round-5 frame; after the last one: map bytes,
particles, pfslam_debug_check_cells.  The oracle runs once per scenario and is shared by every handle that replays it.  Every scenario
asserts, on the oracle's output alone, that it still reaches the edge it was built for.

  A  one cell        1081 beams of range 0.005: all 17 runs hold the same key; every later run is wholly `<= pk` (the lo == 63 fix-up),
                     every key but one is a duplicate of an earlier run; then a room scan again (more than 1000 walls)
  B  few cells       1081 beams over five ranges, scattered by 7919 j mod 5: every run holds every cell
  C  key 0           20 m / 0.1 m patch, eight beams of 14.142 m at -135 degrees: the far corner of the local grid, cell index 0
                     (`!(r > mine && key == 0u)`, `pk = key - 1u`)
  D  beam counts     64 .. 4096: n_runs % 4 = 1, 2, 3, 0; sort_n 1024 | 1088; a last run of one beam | full; the 1024-strides of
                     k_walls<3>'s passes; 147 456 bytes of dynamic LDS at 4096 beams, more than 3072 new walls in one frame
  E  coinciding laps 4096 beams, beam j and j + 1440 in the same cell: duplicates in runs 22 apart, more than 1024 new walls
  F  clamp order     70 frames of one scan without re-balance: the map weights reach -113 and +113 (the walls' +4 behind the free cells' -1)
  G  larger cloud    A and E at 5000 particles: k_reduce_groups<1> and the tiled weights in front of the chain

Every handle runs with pfslam_set_variant(3).  The frame loop keeps the lattice-cell rows -- and with them round-5 frames -- only while the
cloud is narrow (org_use_cells: a wave's beam-end box of at most 24 cells per side; at 96 particles and 0.025 m cells that is a spread
of 0.054 m), and variant 3 differs from the default organisation in nothing but that test.  Without it D at 64 beams and E leave
round-5 frames in their frame 3 (two dispersions without a resample in between), and the chain would see one frame of each.

Preconditions as the oracle gave them, on the MI355X machine's build and on a CPU-only one alike (96 particles unless noted):
  A  n_wall 1, 1, 1 in frames 2-4 (n_free 0, 0, 0), 1042 in frame 5; at 5000 particles 1, 1, 1 and 1046
  B  n_wall 54, 54, 54
  C  cell 0 heads the wall list in frames 2, 3, 4, 6, 7 of 7 at 96 particles, in 2, 4, 6, 7 at 1000
  D  4096 beams: n_wall 4038, 4049, 4049 in frames 2-4, n_insert 4029, 3979, 3709; 1088 beams: n_wall 1057, 1050, 1056
  E  n_wall 1385, 1385, 1390, 1390, n_insert 1364 in frame 2; at 5000 particles 1385, 1385, 1391, 1387 and 1364, 1370, 1115
  F  map weights from -113 to 113
Every case ran as round-5 frames from frame 2 on (variant 3).  4096 beams launch: 147 456 bytes of dynamic LDS are within a workgroup's 160 KiB.

Mutations this file was checked against, on a scratch copy of csrc/:
  `dup = true` for an equal key in an earlier run dropped (k_walls_rank_traverse; memory-safe by inspection: a surviving duplicate's rank
      is its place among the at most nb real keys, and every list it lengthens holds nb entries): 18 of 25 cases fail, each on the
      header's internal-consistency error in the first frame that holds a cell in two runs: A, B, C, E, F, all of G, D at 1024, 1025, 4033,
      4095, 4096 beams; D at 64 .. 320 and 1088 beams passes (neighbouring runs of these scans share no cell)
  the `lo[u] == 63` fix-up term dropped: NOT run.  Two keys then share a rank and a wall is lost, so k_walls<3>'s list is shorter than the
      mask's; k_wall_weights reads wall_c2 up to the MASK's count, and on a fresh handle the places behind the chain's count were never
      written (hipMalloc does not clear them): an index read from there may leave the map's arrays.  Not memory-safe by inspection.
  the key-0 guard's removal: NOT run.  It makes `pk` wrap and sends ranks past sort_n.
"""
import time

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_devlib_frames import environ

pytestmark = pytest.mark.gpu
FIELDS = ("x", "y", "theta", "w")
KD_CAP = 1 << 17       # (70 frames of 1081 beams, 4 frames of 4096: never reached)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_trace(a, b):
    """tests/fuzz_step.py's comparison: equal, or both neff NaN and everything else equal"""
    if a == b:
        return True
    rest = lambda t: {k: v for k, v in t.items() if k != "neff"}
    return bool(np.isnan(a["neff"]) and np.isnan(b["neff"]) and rest(a) == rest(b))


# ---- scans ---------------------------------------------------------------------------------------------------------------------------------
def room(nb, f=0, lapstep=0.0, noise=0.0):
    """A closed, three-lobed room around the robot; beam j looks along -135 + 0.25 j degrees, so beams 1440 apart look the same way:
    lapstep moves every further lap outwards (distinct cells), noise takes neighbours apart."""
    j = np.arange(nb)
    ang = np.radians(-135.0 + 0.25 * j)
    r = 6.0 + 1.5 * np.cos(3.0 * ang + 0.05 * f) + lapstep * (j // 1440)
    r = r + np.random.RandomState(4 + f).uniform(-noise, noise, nb)
    return r.astype(np.float32)


def scans_one_cell():
    return [room(1081)] + [np.full(1081, 0.005, np.float32)] * 3 + [room(1081, 1)]


def scans_few_cells():
    j = np.arange(1081)
    return [room(1081)] + [(0.02 * (1 + (7919 * j + k) % 5)).astype(np.float32) for k in range(3)]


def scans_key0():
    s = room(1081)
    t = s.copy()
    t[:8] = 14.142
    return [s] + [t] * 6


def scans_beams(nb):
    return [room(nb, f, lapstep=1.7, noise=0.01) for f in range(4)]


def scans_laps():
    return [room(4096, f) for f in range(4)]


def scans_clamp():
    return [room(1081)] * 70


# ---- the oracle, once per scenario -----------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_frames(key, n, nb, scans, scale=40.0, res=0.025, balance_period=100):
    """O.Slam through the scans (frame numbers from 1): per frame the trace, the pose bits and both cell lists; at the end the map and the
    particles.  Computed once per key and never changed afterwards."""
    if key not in _ORACLE:
        with environ(ORC_THREADS="16"):
            o = O.Slam(n, n_beams=nb, kd_capacity=KD_CAP, balance_period=balance_period, patch=O.Patch(scale, scale, res, res))
            rec = {"trace": [], "pose": [], "wall": [], "free": []}
            for f, s in enumerate(scans, start=1):
                o.step(f, s)
                rec["trace"].append(o.trace())
                rec["pose"].append(bits(o.pose).copy())
                rec["wall"].append(o.cells(0))
                rec["free"].append(o.cells(1))
            rec["map"] = o.tree()
            rec["particles"] = o.particles()
            o.close()
        for v in rec.values():
            for a in (v if isinstance(v, list) else [v]):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _ORACLE[key] = rec
    return _ORACLE[key]


# ---- the common harness ----------------------------------------------------------------------------------------------------------------------
def same_cells(got, want, what):
    assert len(got) == len(want), "%s: %d cells, the oracle has %d" % (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s: %d of %d cells differ, the first at place %d: %d vs the oracle's %d" % (
        what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


def look(h, want, i, what):
    """frame i + 1 of the handle against the oracle's: trace, pose bits, the ordered wall and free cell lists; a round-5 frame from frame 2 on"""
    f = i + 1
    got = h.trace()
    assert same_trace(got, want["trace"][i]), "%s frame %d: trace %s vs the oracle's %s" % (what, f, got, want["trace"][i])
    assert (bits(h.pose) == want["pose"][i]).all(), "%s frame %d: pose %s" % (what, f, h.pose)
    same_cells(h.cells(0), want["wall"][i], "%s frame %d, wall" % (what, f))
    same_cells(h.cells(1), want["free"][i], "%s frame %d, free" % (what, f))
    if f >= 2:
        assert h.frame_mode()["round5_frame"], "%s frame %d did not run as a round-5 frame" % (what, f)


def run_case(pkg, want, n, nb, scans, what, serial=0, every_frame=True, scale=40.0, res=0.025, balance_period=100):
    """A fresh handle (default lag: frames in flight; variant 3: see the module's text) through the scans against the oracle's record:
    after every frame (every_frame) or after the last one only, so that the frames really overlap; then map, particles and the cell
    rows' invariants."""
    t0 = time.perf_counter()
    h = pkg.PfSlam(n, n_beams=nb, kd_capacity=KD_CAP, balance_period=balance_period, map_scale=(scale, scale), map_res=(res, res))
    try:
        h.set_variant(3)
        if serial:
            h.set_serial(1)
        for i, s in enumerate(scans):
            h.step(i + 1, s)
            if every_frame or i == len(scans) - 1:
                look(h, want, i, what)
        assert h.frame_mode()["serial"] == bool(serial), what
        m = h.map()
        assert len(m) == len(want["map"]) and m.tobytes() == want["map"].tobytes(), "%s: maps differ" % what
        got = h.particles()
        for fld in FIELDS:
            bad = int((bits(got[fld]) != bits(want["particles"][fld])).sum())
            assert bad == 0, "%s: %d of %d particles differ in %s" % (what, bad, n, fld)
        chk = h.check_cells()
        assert chk["violations"] == 0, "%s: %s" % (what, chk)
    finally:
        h.close()
    print("[wall] %s: %d frames in %.2f s" % (what, len(scans), time.perf_counter() - t0))


def n_wall(want, frames):
    return [want["trace"][f - 1]["n_wall"] for f in frames]


def n_insert(want, frames):
    return [want["trace"][f - 1]["n_insert"] for f in frames]


# ---- A, G: one cell ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("serial", (0, 1))
@pytest.mark.parametrize("n", (96, 5000))
def test_a_whole_scan_in_one_cell(pkg, n, serial):
    """A (and G at 5000 particles): three frames whose 1081 beams all end in the robot's own cell -- seventeen runs of one key: a rank per
    run, every instance but the first a duplicate of an earlier run, every other run wholly `<= pk` -- then a room scan again."""
    scans = scans_one_cell()
    want = oracle_frames(("A", n), n, 1081, scans)
    print("A, n %d: n_wall %s, n_free %s" % (n, n_wall(want, range(1, 6)), [t["n_free"] for t in want["trace"]]))
    assert n_wall(want, (2, 3, 4)) == [1, 1, 1], n_wall(want, (2, 3, 4))
    assert n_wall(want, (5,))[0] > 1000, n_wall(want, (5,))
    run_case(pkg, want, n, 1081, scans, "A n %d serial %d" % (n, serial), serial=serial)


# ---- B: few cells -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("serial", (0, 1))
def test_b_few_cells_shared_by_every_run(pkg, serial):
    """B: five ranges scattered over the beams by 7919 j mod 5 -- neighbours never share a range, every run holds every cell many times."""
    scans = scans_few_cells()
    want = oracle_frames("B", 96, 1081, scans)
    print("B: n_wall %s" % n_wall(want, range(1, 5)))
    assert all(2 <= v <= 60 for v in n_wall(want, (2, 3, 4))), n_wall(want, (2, 3, 4))
    run_case(pkg, want, 96, 1081, scans, "B serial %d" % serial, serial=serial)


# ---- C: key 0 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("serial", (0, 1))
@pytest.mark.parametrize("n", (96, 1000))
def test_c_the_wall_cell_with_index_zero(pkg, n, serial):
    """C: a 200 x 200 patch of 0.1 m cells and eight beams of 14.142 m along -135 degrees: the local grid's cell (0, 0), key 0 -- the one
    key whose `key - 1u` wraps, kept out of the later runs' searches by its own guard."""
    scans = scans_key0()
    want = oracle_frames(("C", n), n, 1081, scans, scale=20.0, res=0.1)
    heads = [f for f in range(1, 8) if len(want["wall"][f - 1]) and want["wall"][f - 1][0] == 0]
    print("C, n %d: cell 0 heads the wall list in frames %s" % (n, heads))
    assert any(f >= 2 for f in heads), heads
    run_case(pkg, want, n, 1081, scans, "C n %d serial %d" % (n, serial), serial=serial, scale=20.0, res=0.1)


# ---- D: beam counts ---------------------------------------------------------------------------------------------------------------------------
BEAMS = (64, 65, 128, 192, 256, 320, 1024, 1025, 1088, 4033, 4095, 4096)


@pytest.mark.parametrize("nb", BEAMS)
def test_d_beam_counts_where_the_loops_change_shape(pkg, nb):
    """D: sort_n = the beams rounded up to whole runs of 64; the rank searches take four runs side by side; k_walls<3>'s passes step by
    1024.  Laps 1.7 m apart and 1 cm of noise: nearly every beam its own cell, nearly every cell a new wall."""
    scans = scans_beams(nb)
    want = oracle_frames(("D", nb), 96, nb, scans)
    print("D, %d beams: n_wall %s, n_insert %s" % (nb, n_wall(want, range(1, 5)), n_insert(want, range(1, 5))))
    if nb == 4096:
        assert min(n_wall(want, (2, 3, 4))) > 3900, n_wall(want, (2, 3, 4))
        assert max(n_insert(want, (2, 3, 4))) > 3072, n_insert(want, (2, 3, 4))
    if nb == 1088:
        assert min(n_wall(want, (2, 3, 4))) > 1024, n_wall(want, (2, 3, 4))
    run_case(pkg, want, 96, nb, scans, "D %d beams" % nb)
    if nb == 4096:
        run_case(pkg, want, 96, nb, scans, "D %d beams, looked at once" % nb, every_frame=False)


# ---- E, G: coinciding laps --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (96, 5000))
def test_e_laps_that_coincide(pkg, n):
    """E (and G at 5000 particles): 4096 beams are 2.8 laps of the same room: beam j and beam j + 1440 end in the same cell, in runs 22 or
    23 apart, and the first frame on the seeded map still inserts more than 1024 walls."""
    scans = scans_laps()
    want = oracle_frames(("E", n), n, 4096, scans)
    print("E, n %d: n_wall %s, n_insert %s" % (n, n_wall(want, range(1, 5)), n_insert(want, range(1, 5))))
    assert max(n_wall(want, (1, 2, 3, 4))) < 1500, n_wall(want, (1, 2, 3, 4))
    assert max(n_insert(want, (2, 3, 4))) > 1024, n_insert(want, (2, 3, 4))
    run_case(pkg, want, n, 4096, scans, "E n %d" % n)
    run_case(pkg, want, n, 4096, scans, "E n %d, looked at once" % n, every_frame=False)


# ---- F: clamp order ---------------------------------------------------------------------------------------------------------------------------
def test_f_weights_reach_both_clamps(pkg):
    """F: the same scan 70 times, no re-balance: walls climb by +4 to the clamp at 113, free cells sink by -1 to -113, and a cell that is both
    takes its -1 first (k_free_traverse in front of k_wall_weights on the free-cell stream)."""
    scans = scans_clamp()
    want = oracle_frames("F", 96, 1081, scans, balance_period=0)
    w = want["map"]["w"]
    print("F: map weights %g .. %g over %d nodes" % (w.min(), w.max(), len(w)))
    assert w.min() == -113 and w.max() == 113, (w.min(), w.max())
    try:
        run_case(pkg, want, 96, 1081, scans, "F", balance_period=0)
    finally:
        del _ORACLE["F"]        # (70 frames of free cells: nobody else replays them)
