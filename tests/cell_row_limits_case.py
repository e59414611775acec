"""Child-process driver of tests/test_gpu_cell_row_limits.py: the lattice-cell rows (csrc/kd_cells.hip.inc) with their list or pool cut
short.  cells_wipe reads PFSLAM_CELL_LIST_CAP / PFSLAM_CELL_POOL_CAP once per process, so every capacity setting needs a process
of its own: the test sets the environment and runs
    python tests/cell_row_limits_case.py CASE [CASE ...]
Every case steps a handle and the CPU oracle through the same frames, compares them bit for bit (trace, pose, at the end the four
particle fields and the map bytes), asks pfslam_debug_check_cells for violations wherever it looks, and asserts the bookkeeping of
the overflow path it is about.  One JSON line per case goes to stdout: {"case", "ok", "error", ...what the case saw}.  Exit status 1
when a case failed; a library error (PfSlamError: a HIP error, a stream gate that gave up) ends the process at once with status 2 --
nothing more is started on the device behind it.
The world and the helpers are shared with the in-process tests of that module."""
import importlib
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import oracle_lib as O  # noqa: E402

N_MAP = 20000          # map points (the issue: 20 000 .. 100 000, as few as give >= 256 claimed cells -- `measure` asserts that)
N_BEAMS = 1081
RES = 0.025
FIRST = 6              # frames 1 .. 5 only disperse the cloud (pfslam_motion_update), as tests/test_gpu_frame.py does
BIT = {"list": 1, "pool": 2}   # PF_CF_LIST_FULL, PF_CF_POOL_FULL
FIELDS = ("x", "y", "theta", "w")


def cell_sub():
    """PF_CELL_SUB: cell_stats()'s window corner is in SUB-cells."""
    with open(os.path.join(ROOT, "gpu-icp-slam_amd", "csrc", "kd_cells.hip.inc")) as f:
        return int(re.search(r"#define PF_CELL_SUB (\d+)", f.read()).group(1))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


class World:
    """The uploaded map and a scan per frame; offsets[i] = the odometry shift the cloud has seen before scan i is taken."""

    def __init__(self, pkg, n_scans, offsets=None, n_map=N_MAP):
        pts, self.segs = pkg.synth.make_map_points(n_map, seed=1)
        self.tree = pkg.kd_create(pts)
        offsets = offsets if offsets is not None else [(0.0, 0.0)] * n_scans
        self.scans = [pkg.synth.make_scan(self.segs, (0.002 * i + offsets[i][0], 0.001 * i + offsets[i][1], 0.0004 * i), seed=2000 + i)
                      for i in range(n_scans)]
        assert all(len(s) == N_BEAMS for s in self.scans)
        self.cap = len(self.tree) + (1 << 18)


def start_cloud(n):
    """What five pfslam_motion_update calls make of n particles at the origin."""
    p = O.make_particles(n)
    for f in range(1, FIRST):
        O.add_noise(p, f)
    return p


def same_particles(got, want, what):
    for fld in FIELDS:
        assert (bits(got[fld]) == bits(want[fld])).all(), "%s: particles differ in %s" % (what, fld)


def make_oracle(world, n, balance_period=100, patch=None):
    o = O.Slam(n, n_beams=N_BEAMS, kd_capacity=world.cap, balance_period=balance_period, patch=patch)
    o.set_map(world.tree)
    o.set_particles(start_cloud(n))
    return o


def make_handle(pkg, world, n, variant=0, lag=None, timing=0, balance_period=100, **kw):
    h = pkg.PfSlam(n, n_beams=N_BEAMS, kd_capacity=world.cap, balance_period=balance_period, **kw)
    h.set_map(world.tree)
    if variant:
        h.set_variant(variant)
    if timing:
        h.set_timing(timing)
    if lag is not None:
        h.set_lag(lag)
    for f in range(1, FIRST):
        h.motion_update(f)
    return h


def frame_row(e):
    """Trace and pose bits of the last booked frame (handle, oracle or a set of virtual ranks)."""
    t = e.trace()
    return [t["best"], t["resampled"], t["n_wall"], t["n_free"], t["n_insert"], int(np.float32(t["neff"]).view(np.int32)), t["kd_size"]] + bits(e.pose).tolist()


def parity(h, o, what):
    got, want = frame_row(h), frame_row(o)
    assert got == want, "%s: trace / pose differ from the oracle: %s != %s" % (what, got, want)


def parity_at_end(h, o, what):
    parity(h, o, what)
    same_particles(h.particles(), o.particles(), what)
    assert h.map().tobytes() == o.tree().tobytes(), "%s: map bytes differ from the oracle" % what


def look(h, what):
    """cell_stats + frame mode + plan rows; the rows' invariants must hold wherever they are looked at."""
    st = h.cell_stats()
    chk = h.check_cells()
    assert chk["violations"] == 0, "%s: check_cells %s" % (what, chk)
    st["flags"] = int(st["flags"])
    st["round5"] = h.frame_mode()["round5_frame"]
    st["plan_rows"] = h.plan_stats()["rows"]
    st["published"] = chk["published"]
    return st


KEEP = ("cells", "rows", "pool_slots", "cells_without_row", "flags", "wipes", "suspended", "round5", "plan_rows", "window_kx", "window_ky")


def brief(frame, st):
    d = {k: (st[k] if isinstance(st[k], bool) else int(st[k])) for k in KEEP}
    d["frame"] = frame
    return d


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def case_measure(pkg, out):
    """Uncapped: what the scenario of case a needs -- the largest list and pool use over its frames."""
    n = 300
    w = World(pkg, 11)
    h, o = make_handle(pkg, w, n, variant=3, balance_period=10), make_oracle(w, n, balance_period=10)
    cells = pool = 0
    for i, s in enumerate(w.scans):
        o.step(FIRST + i, s); h.step(FIRST + i, s); h.synchronize()
        st = look(h, "measure frame %d" % (FIRST + i))
        parity(h, o, "measure frame %d" % (FIRST + i))
        assert st["flags"] == 0 and st["suspended"] == 0 and st["rows"] > 0 and st["round5"], st
        cells, pool = max(cells, int(st["cells"])), max(pool, int(st["pool_slots"]))
        out.setdefault("seen", []).append(brief(FIRST + i, st))
    parity_at_end(h, o, "measure")
    h.close(); o.close()
    out["cells"], out["pool_slots"] = cells, pool
    assert cells >= 256, "the scenario claims only %d cells: raise N_MAP" % cells


def sequence(pkg, out, bit, timing):
    """Cases a, b (first half) and e: consecutive frames, looked at after each.  A = first frame whose flags carry `bit`, B = the second
    overflowing frame, L = the re-balance frame (frame % 10 == 5) behind the suspension."""
    n = 300
    w = World(pkg, 11)                                    # frames 6 .. 16: the re-balance of frame 15 lifts the suspension
    h, o = make_handle(pkg, w, n, variant=3, timing=timing, balance_period=10), make_oracle(w, n, balance_period=10)
    A = B = L = None
    seen = out.setdefault("seen", [])
    for i, s in enumerate(w.scans):
        f = FIRST + i
        what = "frame %d" % f
        o.step(f, s); h.step(f, s); h.synchronize()
        st = look(h, what)
        seen.append(brief(f, st))
        parity(h, o, what)
        prev = seen[-2] if len(seen) > 1 else None
        if B is not None and L is None and f % 10 != 5:   # suspended: the round-2 plan scores, staged frames, no wipe
            assert st["suspended"] == 1, (what, st)
            assert st["rows"] == 0 and st["plan_rows"] > 0 and not st["round5"], (what, st)
            assert st["wipes"] == out["wipes_at_B"], (what, "a suspended handle wiped", st)
        elif B is not None and L is None:                 # the re-balance (upload_tree) lifts the suspension
            L = f
            assert st["suspended"] == 0, (what, "the re-balance did not lift the suspension", st)
        elif L is not None:                               # (the same caps: the rows overflow again, which is not this part's business)
            if f == L + 1:
                assert prev["rows"] > 0 or st["rows"] > 0, (what, "the rows are not in use again", prev, st)
                assert st["wipes"] > out["wipes_at_B"], (what, "rows of the re-balanced map start wiped", st)
        elif A is None:
            assert st["suspended"] == 0 and st["rows"] > 0 and st["round5"] == (timing < 2), (what, st)
            if st["flags"] & bit:
                A = f
                assert st["cells_without_row"] > 0, (what, "overflow, and no cell without a row", st)
            else:
                assert st["flags"] == 0, (what, st)
        else:                                             # behind A, in front of B
            if f == A + 1:
                assert st["wipes"] == prev["wipes"] + 1, (what, "the frame behind the overflow did not run on a wiped table", prev, st)
            assert st["rows"] > 0, (what, st)
            if st["flags"] & bit:
                B = f
                assert B - A <= 16
                assert st["suspended"] == 1, (what, "second overflow within 16 frames, not suspended", st)
                out["wipes_at_B"] = int(st["wipes"])
            else:
                assert st["suspended"] == 0, (what, st)
    out["A"], out["B"], out["L"] = A, B, L
    assert A is not None, "flag bit %d was never raised: the cap is too generous (or ignored)" % bit
    assert B is not None, "no second overflow behind frame %d" % A
    assert L is not None and B < L < FIRST + len(w.scans) - 1, "no re-balance frame behind the suspension"
    parity_at_end(h, o, "end")
    h.close(); o.close()


def case_a(pkg, out, bit):
    sequence(pkg, out, bit, timing=0)


def case_e(pkg, out, bit):
    """Per-phase timing: frame_v2_ok refuses, the staged chain runs -- the other copy of the flag logic (pfslam_stages.hip.inc)."""
    sequence(pkg, out, bit, timing=2)


def case_b(pkg, out, bit):
    """pfslam_set_map of the very same tree lifts a suspension too."""
    n = 300
    w = World(pkg, 8)
    h, o = make_handle(pkg, w, n, variant=3), make_oracle(w, n)
    seen = out.setdefault("seen", [])
    i = 0
    while i < 5:
        o.step(FIRST + i, w.scans[i]); h.step(FIRST + i, w.scans[i]); h.synchronize()
        st = look(h, "frame %d" % (FIRST + i))
        seen.append(brief(FIRST + i, st))
        parity(h, o, "frame %d" % (FIRST + i))
        i += 1
        if st["suspended"] == 1:
            break
    assert st["suspended"] == 1 and st["flags"] & bit, ("not suspended within five frames", seen)
    wipes = st["wipes"]
    m = h.map()
    assert m.tobytes() == o.tree().tobytes()
    h.set_map(m); o.set_map(m)
    assert h.cell_stats()["suspended"] == 0, "set_map did not lift the suspension"
    rows = []
    for k in range(2):
        o.step(FIRST + i, w.scans[i]); h.step(FIRST + i, w.scans[i]); h.synchronize()
        st = look(h, "frame %d" % (FIRST + i))
        seen.append(brief(FIRST + i, st))
        parity(h, o, "frame %d" % (FIRST + i))
        rows.append(st["rows"])
        if k == 0:
            assert st["suspended"] == 0 and st["wipes"] == wipes + 1, (seen[-1], wipes)
        i += 1
    assert max(rows) > 0, ("the rows are not in use again behind set_map", seen)
    parity_at_end(h, o, "end")
    h.close(); o.close()


def case_c(pkg, out, bit):
    """Frame numbers 20 apart: every frame overflows and is wiped behind, none suspends (the test is on FRAME NUMBERS, 1 .. 16 apart)."""
    n = 300
    frames = (6, 26, 46, 66, 86)                          # none is 5 mod 100: no re-balance
    w = World(pkg, len(frames))
    h, o = make_handle(pkg, w, n, variant=3), make_oracle(w, n)
    seen = out.setdefault("seen", [])
    for i, f in enumerate(frames):
        o.step(f, w.scans[i]); h.step(f, w.scans[i]); h.synchronize()
        st = look(h, "frame %d" % f)
        seen.append(brief(f, st))
        parity(h, o, "frame %d" % f)
        assert st["flags"] & bit, ("frame %d did not overflow" % f, st)
        assert st["suspended"] == 0 and st["rows"] > 0 and st["round5"], ("frame %d" % f, st)
        assert st["wipes"] == seen[0]["wipes"] + i, ("one wipe per frame behind the first", seen)
    parity_at_end(h, o, "end")
    h.close(); o.close()


def case_d(pkg, out, bit):
    """1000 particles, default variant (round-5 frames with rows from 65 particles on, while the cloud's spread allows them), frames in
    flight and no look until the end: the overflow is booked `lag` steps late, the frames enqueued meanwhile carry the flag again, the
    switch to staged frames happens with frames enqueued, and header flags of frames enqueued before a wipe are dropped."""
    n = 1000
    w = World(pkg, 9)
    for lag in (1, 2):
        h, o = make_handle(pkg, w, n, lag=lag), make_oracle(w, n)
        for i, s in enumerate(w.scans):
            o.step(FIRST + i, s); h.step(FIRST + i, s)
        h.synchronize()
        st = look(h, "lag %d" % lag)
        out.setdefault("seen", []).append(dict(brief(FIRST + len(w.scans) - 1, st), lag=lag))
        assert st["suspended"] == 1, ("lag %d: not suspended" % lag, st)
        assert st["wipes"] >= 1, ("lag %d" % lag, st)
        assert st["rows"] == 0 and not st["round5"], ("lag %d: a suspended handle still runs round-5 frames" % lag, st)
        parity_at_end(h, o, "lag %d" % lag)
        h.close(); o.close()


def case_f(pkg, out, bit):
    """Stage-level call: pfslam_score_kd under the list cap."""
    n = 300
    w = World(pkg, 1)
    p = start_cloud(n)
    h = pkg.PfSlam(n, n_beams=N_BEAMS, kd_capacity=w.cap)
    h.set_map(w.tree); h.set_variant(3)
    h.set_particles(p); h.set_scan(w.scans[0])
    want = O.score_kd(w.tree, p, w.scans[0])
    fits = []
    for k in range(2):
        fits.append(h.score_kd())
        st = look(h, "call %d" % k)
        out.setdefault("seen", []).append(brief(k, st))
        assert st["flags"] & bit and st["cells_without_row"] > 0 and st["rows"] > 0, ("call %d" % k, st)
        assert (bits(fits[k]) == bits(want)).all(), "call %d: fits differ from the oracle" % k
    assert (bits(fits[0]) == bits(fits[1])).all()
    h.close()


def case_g(pkg, out, bit):
    """Two virtual ranks of 300 particles each against ONE capped handle of 600 and the oracle."""
    import torch
    from test_gpu_sharded import _VirtualRanks
    n, world = 600, 2
    w = World(pkg, 6)
    one, o = make_handle(pkg, w, n, variant=3), make_oracle(w, n)
    v = _VirtualRanks(pkg, torch, n, world, n_beams=N_BEAMS, kd_capacity=w.cap)
    for e in v.engs:
        e.set_map(w.tree); e.set_variant(3)
        for f in range(1, FIRST):
            e.motion_update(f)
    flagged = [False] * world
    seen = out.setdefault("seen", [])
    for i, s in enumerate(w.scans):
        f = FIRST + i
        o.step(f, s); one.step(f, s); one.synchronize()
        v.step(f, s)
        for e in v.engs:
            e.synchronize()
        want = frame_row(o)
        assert frame_row(one) == want, "frame %d: the single handle differs from the oracle" % f
        for r, e in enumerate(v.engs):
            assert frame_row(e) == want, "frame %d: rank %d differs from the oracle: %s != %s" % (f, r, frame_row(e), want)
            st = look(e, "frame %d rank %d" % (f, r))
            flagged[r] = flagged[r] or bool(st["flags"] & bit)
            seen.append(dict(brief(f, st), rank=r))
    assert all(flagged), ("a rank never raised the flag", flagged)
    assert one.cell_stats()["suspended"] == 1
    for r, e in enumerate(v.engs):
        assert e.cell_stats()["suspended"] == 1, "rank %d did not end suspended" % r
        assert e.map().tobytes() == o.tree().tobytes(), "rank %d: map bytes" % r
    got = [e.particles() for e in v.engs]
    same_particles({fld: np.concatenate([g[fld] for g in got]) for fld in FIELDS}, o.particles(), "ranks")
    parity_at_end(one, o, "single handle")
    v.close(); one.close(); o.close()


CASES = {"measure": case_measure, "a": case_a, "b": case_b, "c": case_c, "d": case_d, "e": case_e, "f": case_f, "g": case_g}


def main(argv):
    pkg = importlib.import_module("gpu-icp-slam_amd")
    os.environ.setdefault("ORC_THREADS", str(min(16, os.cpu_count() or 1)))
    kinds = [k for k, v in (("list", "PFSLAM_CELL_LIST_CAP"), ("pool", "PFSLAM_CELL_POOL_CAP")) if os.environ.get(v)]
    failed = 0
    for name in argv:
        out = {"case": name, "ok": False, "error": None}
        try:
            if name == "measure":
                assert not kinds, "measure runs uncapped"
                case_measure(pkg, out)
            else:
                assert len(kinds) == 1, "set exactly one of PFSLAM_CELL_LIST_CAP / PFSLAM_CELL_POOL_CAP"
                out["cap"] = kinds[0]
                CASES[name](pkg, out, BIT[kinds[0]])
            out["ok"] = True
        except pkg.PfSlamError as e:      # the device may be in any state: nothing more is started on it
            out["error"] = "PfSlamError: %s" % e
            print(json.dumps(out), flush=True)
            return 2
        except AssertionError as e:
            out["error"] = "AssertionError: %s" % (e,)
            failed += 1
        print(json.dumps(out), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
