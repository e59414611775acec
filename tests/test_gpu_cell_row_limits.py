"""The persistent lattice-cell rows (csrc/kd_cells.hip.inc) where they overflow, move and suspend.

Three recovery paths sit under the rows, and an oracle comparison alone sees none of them -- a window that is never re-centred gives
the same bits through the generic traversal, a wipe that never happens scores from rows that are right most of the time:
  * the window MOVES when the cloud's mean has left its middle by more than PF_CELL_DRIFT_MAX = 120 lattice cells (PF_CF_FAR ->
    PF_HDR_CELLS_WIPE -> a wipe in front of the next scoring pass, which puts the window around the cloud again);
  * a full LIST or POOL (PF_CF_LIST_FULL / PF_CF_POOL_FULL -> PF_HDR_CELLS_FULL) leaves the other cells without rows and wipes the table;
  * a second overflow whose frame number is 1 .. 16 above the first one's SUSPENDS the rows (the round-2 plan scores, staged frames)
    until the map is uploaded again (pfslam_set_map, a re-balance).
Each path is forced here and its bookkeeping (pfslam_cell_stats: wipes, window corner, flags, suspended; pfslam_frame_mode;
pfslam_plan_stats) is asserted, next to the one reference used everywhere: the CPU oracle stepping the same frames with the same
shifts, compared bit for bit (trace, pose, the four particle fields, the map bytes), and pfslam_debug_check_cells == no violation
wherever the rows are looked at.

The window moves run in this process with the real capacities.  The capacities are read once per process (cells_wipe), so the
overflow cases run in tests/cell_row_limits_case.py, ONE child process per capacity setting: the first runs the scenario uncapped and
measures what it needs, the list cap / the pool cap of the other two are a quarter of that (the library's floor is 64) -- a cap that
turned out too generous fails its cases ("the flag was never raised") instead of passing them vacuously.  The first test of a
capacity setting pays for its child; the others read what it printed.

Measured on an MI355X (300 particles, rows forced on, 20 000 map points, frames 6 .. 16): 211 201 claimed cells and 2 567 596 pool
slots at most, hence a list cap of 52 800 and a pool cap of 641 899; either flag first appears in frame 6, the second overflow and
the suspension follow in frame 7, the re-balance of frame 15 lifts it.  Case f found that pfslam_cell_stats' "sub-cells without a
row" left out the cells a full list refuses (k_cells_mark counts them now).  The whole module: 22 s."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cell_row_limits_case as K
import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 300
FRAMES = 14                       # frames 6 .. 19
SHIFT_CELLS = 80                  # one odometry shift: 2.0 m at 0.025 m
SLACK = 8                         # cells: 20 cm is far above the cloud's own drift in these frames (1.5 cm of diffusion each), far below 40


# ---- 1. window moves -----------------------------------------------------------------------------------------------------------
def move_plan(vec, cells, at):
    """Shift by `cells` lattice cells along vec in front of every scan index in `at`: (delta, the offset every scan is cast from)."""
    d = np.array([vec[0] * cells * K.RES, vec[1] * cells * K.RES, 0.0], np.float32)
    offsets = [(float(d[0]) * sum(i >= a for a in at), float(d[1]) * sum(i >= a for a in at)) for i in range(FRAMES)]
    return d, offsets


class OracleRun:
    """The oracle stepped once through a scenario: every frame's trace + pose bits, the particles and the map at the end."""

    def __init__(self, pkg, vec, cells, at, patch=None):
        self.delta, offsets = move_plan(vec, cells, at)
        self.at = at
        self.world = K.World(pkg, FRAMES, offsets)
        o = K.make_oracle(self.world, N, patch=patch)
        self.rows = []
        for i, s in enumerate(self.world.scans):
            if i in at:
                o.shift_particles(self.delta)
            o.step(K.FIRST + i, s)
            self.rows.append(K.frame_row(o))
        self.particles, self.tree = o.particles(), o.tree().tobytes()
        o.close()

    def check_end(self, h):
        assert K.frame_row(h) == self.rows[-1]
        K.same_particles(h.particles(), self.particles, "end")
        assert h.map().tobytes() == self.tree


@pytest.fixture(scope="module")
def oracle_runs(pkg):
    """Oracle runs, one per shift vector, shared by the lags."""
    cache = {}

    def get(vec):
        if vec not in cache:
            cache[vec] = OracleRun(pkg, vec, SHIFT_CELLS, (3, 6))
        return cache[vec]
    return get


def corner(st):
    """Window corner in lattice cells (cell_stats gives sub-cells)."""
    sub = K.cell_sub()
    return st["window_kx"] / sub, st["window_ky"] / sub


def check_moved(before, st, vec, cells):
    (x0, y0), (x1, y1) = corner(before), corner(st)
    print("window corner %s -> %s (cells), wipes %d -> %d" % ((x0, y0), (x1, y1), before["wipes"], st["wipes"]))
    assert st["wipes"] == before["wipes"] + 1, (before, st)
    for moved, axis in ((x1 - x0, vec[0]), (y1 - y0, vec[1])):
        assert abs(moved - axis * cells) <= SLACK, (moved, axis * cells)      # (an unshifted axis: axis == 0)
    assert st["flags"] == 0 and st["suspended"] == 0 and st["rows"] > 0, st


@pytest.mark.parametrize("lag", [0, 1, 2])
@pytest.mark.parametrize("vec", [(1, 0), (0, -1), (1, -1)], ids=["+x", "-y", "+x-y"])
def test_window_follows_a_cloud_that_leaves_its_middle(pkg, oracle_runs, vec, lag):
    """80 cells of odometry leave the window where it is (40 cells short of PF_CELL_DRIFT_MAX); 80 more raise PF_CF_FAR in frames that
    are in flight: ONE wipe, the window re-centred 160 cells further on the shifted axes and nowhere else, rows live, no flag left."""
    ref = oracle_runs(vec)
    h = K.make_handle(pkg, ref.world, N, variant=3, lag=lag)
    base = None
    for i, s in enumerate(ref.world.scans):
        if i in ref.at:
            h.shift_particles(ref.delta)
        h.step(K.FIRST + i, s)
        if i >= 6:                # behind the second shift: no look, the frames really are in flight
            continue
        h.synchronize()
        st = K.look(h, "frame %d" % (K.FIRST + i))
        assert K.frame_row(h) == ref.rows[i], "frame %d" % (K.FIRST + i)
        assert st["flags"] == 0 and st["suspended"] == 0 and st["rows"] > 0 and st["round5"], st
        if i == 2:
            base = st
        if i > 2:                 # shifted by 80 cells: nothing moves, nothing is wiped
            assert st["wipes"] == base["wipes"] and corner(st) == corner(base), (base, st)
    h.synchronize()
    st = K.look(h, "end")
    check_moved(base, st, vec, 2 * SHIFT_CELLS)
    ref.check_end(h)
    h.close()


def test_beam_ends_outside_the_window_until_it_moves(pkg):
    """A 120 m map and ONE shift of 25 m: the cloud stays inside the old window's 32 m reach, most beam ends fall outside it -- the frames
    in flight in front of the wipe take the bounds test of k_score_kd_cells and the generic traversal.  Then the window moves 1000 cells."""
    cells = 1000
    ref = OracleRun(pkg, (1, 0), cells, (3,), patch=O.Patch(120.0, 120.0, K.RES, K.RES))
    h = K.make_handle(pkg, ref.world, N, variant=3, lag=2, map_scale=(120.0, 120.0))
    base = None
    for i, s in enumerate(ref.world.scans):
        if i in ref.at:
            h.shift_particles(ref.delta)
        h.step(K.FIRST + i, s)
        if i >= 3:
            continue
        h.synchronize()
        base = K.look(h, "frame %d" % (K.FIRST + i))
        assert K.frame_row(h) == ref.rows[i], "frame %d" % (K.FIRST + i)
        assert base["flags"] == 0 and base["suspended"] == 0 and base["rows"] > 0 and base["round5"], base
    h.synchronize()
    st = K.look(h, "end")
    check_moved(base, st, (1, 0), cells)
    ref.check_end(h)
    h.close()


# ---- 2. capacities ---------------------------------------------------------------------------------------------------------------
LIST_CASES = ("a", "b", "c", "d", "e", "f", "g")
POOL_CASES = ("a", "b", "c", "d", "e")


def run_child(cases, env_extra):
    """One child, all its cases: {case: its JSON line}.  A child that stopped at a library error leaves the later cases out."""
    env = dict(os.environ, **env_extra)
    for k in ("PFSLAM_CELL_LIST_CAP", "PFSLAM_CELL_POOL_CAP"):
        if k not in env_extra:
            env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cell_row_limits_case.py")] + list(cases), capture_output=True, text=True,
                         timeout=600, env=env)
    res = {}
    for line in out.stdout.splitlines():
        if line.startswith("{"):
            d = json.loads(line)
            res[d["case"]] = d
    res["_exit"] = out.returncode
    res["_tail"] = out.stdout[-1500:] + out.stderr[-2500:]
    return res


@pytest.fixture(scope="module")
def children():
    """kind -> results of that capacity setting's child (started on first use, one at a time); "need" is the uncapped measurement."""
    cache = {}

    def get(kind):
        if "need" not in cache:
            cache["need"] = run_child(["measure"], {})
        need = cache["need"].get("measure")
        assert need and need["ok"], cache["need"]
        if kind == "need":
            return cache["need"]
        if kind not in cache:
            list_cap, pool_cap = max(64, need["cells"] // 4), max(64, need["pool_slots"] // 4)
            print("measured need: %d cells, %d pool slots -> list cap %d, pool cap %d" % (need["cells"], need["pool_slots"], list_cap, pool_cap))
            if kind == "list":
                cache[kind] = run_child(LIST_CASES, {"PFSLAM_CELL_LIST_CAP": str(list_cap)})
            else:
                cache[kind] = run_child(POOL_CASES, {"PFSLAM_CELL_POOL_CAP": str(pool_cap)})
        return cache[kind]
    return get


def test_uncapped_scenario_needs_more_than_the_floor_of_the_caps(children):
    """The measurement the caps are derived from: no flag, no suspension, rows and round-5 frames throughout (asserted by the child), at
    least 256 claimed cells -- a quarter of that is still the library's floor of 64 or more."""
    need = children("need")["measure"]
    print("uncapped, 300 particles, frames 6 .. 16: %d cells, %d pool slots at most" % (need["cells"], need["pool_slots"]))
    assert need["ok"], need["error"]
    assert need["cells"] >= 256, need


def case_result(children, kind, case):
    res = children(kind)
    assert case in res, "case %s did not run: the child ended with status %s\n%s" % (case, res["_exit"], res["_tail"])
    r = res[case]
    print(json.dumps(r))
    assert r["ok"], "%s cap, case %s: %s" % (kind, case, r["error"])
    assert r["cap"] == kind
    return r


@pytest.mark.parametrize("kind,case", [("list", c) for c in LIST_CASES] + [("pool", c) for c in POOL_CASES])
def test_overflow_wipe_suspension_and_lift(children, kind, case):
    """tests/cell_row_limits_case.py, cases a .. g (their docstrings): the flag of this cap is seen, the cells beyond it go without rows,
    the frame behind an overflow runs on a wiped table, the second overflow suspends, a re-balance and pfslam_set_map lift the
    suspension, frame numbers 20 apart never suspend, the same with frames in flight, on the staged chain, at stage level and on two
    virtual ranks -- bit-identical to the oracle throughout."""
    r = case_result(children, kind, case)
    if case in ("a", "e"):        # the sequence the child asserted, restated on what it printed
        A, B, L = r["A"], r["B"], r["L"]
        print("%s cap: first overflow in frame %d, second in frame %d, lifted in frame %d" % (kind, A, B, L))
        by = {s["frame"]: s for s in r["seen"]}
        assert by[A]["flags"] & K.BIT[kind] and by[A]["cells_without_row"] > 0
        assert by[A + 1]["wipes"] == by[A]["wipes"] + 1
        assert by[B]["suspended"] == 1 and by[L]["suspended"] == 0
        assert all(by[f]["rows"] == 0 and by[f]["plan_rows"] > 0 and not by[f]["round5"] and by[f]["wipes"] == by[B]["wipes"] for f in range(B + 1, L))
        assert L > B + 1
    if case == "c":
        assert [s["suspended"] for s in r["seen"]] == [0] * 5 and [s["wipes"] - r["seen"][0]["wipes"] for s in r["seen"]] == [0, 1, 2, 3, 4]
    if case == "d":
        assert [s["lag"] for s in r["seen"]] == [1, 2] and all(s["suspended"] == 1 and s["wipes"] >= 1 for s in r["seen"])
