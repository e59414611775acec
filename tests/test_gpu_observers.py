"""The switches that only OBSERVE a handle -- pfslam_set_timing, pfslam_set_census, pfslam_set_probe, the timing helpers -- and
pfslam_set_stream, which only says where its launches go: none of them may change a result.  The caller-stream cases run in a child
process (tests/caller_stream_case.py says why), started by the last test of this module.

The baseline is the unobserved run of tests/test_gpu_frame.py's run_frames: per-frame rows (trace + pose bits), the final particles, the
map's bytes, the cell rows' bookkeeping (BOOK, and the counts pfslam_debug_check_cells returns) and no violated invariant.  Every
observed run is compared with it bit for bit.  The world is small: a 4000-point map, 12 scans, and
  r5           192 particles, pfslam_set_variant(3): cell rows at any particle count -- the round-5 frame
  default100k  100 000 particles, default organisation -- the round-5 frame as pfslam_step chooses it by itself
  default      4672 particles, the first multiple of 64 above PFSLAM_PLAN_MIN_N's default of 4608, default organisation.  Here that is
               the round-5 frame for TWO frames only: the host learns the cloud's spread from the first booked frame's header, and the
               cloud five dispersions leave (heading spread x beam reach: ~0.4 m) gives 73 waves beam-end boxes of ~50 lattice cells,
               wider than the 24 the cell rows take (org_use_cells) -- from frame 3 on the frames are round-4 frames with the
               shared-prefix plan.  So this case switches between the two frame loops by itself, with a frame in flight; 100 000
               particles is the round count at which the same cloud's boxes are narrow enough for the round-5 frame to stay
  r4           192 particles, variant 2: the plain traversal -- the round-4 frame, nothing planned
  r4plan       192 particles, variant 4: the shared-prefix plan forced -- the round-4 frame with planning launches
and every case asserts the frame it ran as (pfslam_frame_mode), so that a moved threshold cannot quietly turn one into the other.
Per-phase timing (pfslam_set_timing 2) moves a frame from the round-5 to the round-4 code path ON PURPOSE; the results must not notice.

The census counters are held to tests/census_ref.py, a numpy count of the same traversal (pinned to the CPU oracle in
tests/test_census_ref.py).  Timer values are only asked to be finite, >= 0, and > 0 where something was counted."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import census_ref
import oracle_lib as O
from test_gpu_frame import CHECK, bits, run_frames

pytestmark = pytest.mark.gpu
FIELDS = ("x", "y", "theta", "w")
FRAMES = 12
# n, variant, round-5 frame (of the last frame), how the last scan-match pass is organised
CASES = {"r5": (192, 3, True, "cells"), "default100k": (100000, 0, True, "cells"), "default": (4672, 0, False, "plan"),
         "r4": (192, 2, False, "plain"), "r4plan": (192, 4, False, "plan")}
ROUND5_FRAMES = {"r5": FRAMES, "default100k": FRAMES, "default": 2, "r4": 0, "r4plan": 0}   # the first so many frames are round-5 frames
CENSUS_KEYS = ("trips", "visits", "tests", "test_lanes", "uniform_trips", "prefix_trips", "redescents", "redescents_noop")


def make_world(pkg):
    pts, segs = pkg.synth.make_map_points(4000, seed=1)
    tree = pkg.kd_create(pts)
    scans = [pkg.synth.make_scan(segs, (0.002 * i, 0.001 * i, 0.0004 * i), seed=2000 + i) for i in range(FRAMES)]
    return {"pts": pts, "tree": tree, "scans": scans, "base": {}}


@pytest.fixture(scope="module")
def world(pkg):
    import torch
    assert pkg.device_count() > 0 and torch.cuda.is_available()
    torch.cuda.init()                 # (the compute-unit count comes from torch: its start-up is paid here, once)
    return make_world(pkg)


def mode_of(h):
    return dict(h.frame_mode(), plan_rows=h.plan_stats()["rows"])


def hooks(setup=None, after=None, modes=None):
    """A `prepare` for run_frames: setup(h) at once, and after(h, i) right behind the i-th pfslam_step (0-based) -- that frame is still in
    flight then: run_frames looks at it only afterwards.  modes collects pfslam_frame_mode()[0] behind every step."""
    def prepare(h):
        if setup:
            setup(h)
        step, count = h.step, [0]

        def hooked(frame, scan):
            step(frame, scan)
            i = count[0]
            count[0] += 1
            if modes is not None:
                modes.append(h.frame_mode()["round5_frame"])
            if after:
                after(h, i)
        h.step = hooked
    return prepare


def run(pkg, world, case, look=0, prepare=None, inspect=mode_of, frames=FRAMES):
    n, variant = CASES[case][:2]
    return run_frames(pkg, world["tree"], world["scans"][:frames], n, serial=False, variant=variant, look_every=look, prepare=prepare, inspect=inspect)


def baseline(pkg, world, case, look=0):
    """the unobserved run, once per (case, look)"""
    key = (case, look)
    if key not in world["base"]:
        modes = []
        b = run(pkg, world, case, look, prepare=hooks(modes=modes))       # (pfslam_frame_mode reads host state only)
        assert modes == [True] * ROUND5_FRAMES[case] + [False] * (FRAMES - ROUND5_FRAMES[case]) and b[5]["round5_frame"] == CASES[case][2], (case, modes, b[5])
        assert (b[5]["plan_rows"] > 0) == (CASES[case][3] == "plan") and (b[3]["cells"] > 0) == (CASES[case][3] == "cells"), (case, b[5], b[3])
        assert b[4]["violations"] == 0, b[4]
        assert len(b[0]) == (FRAMES + 1 if look == 1 else 1) and b[0][-1][5] > len(world["tree"])   # (a row per look and the last one; walls were inserted)
        assert b[3]["flags"] == 0 and b[3]["claimed"] == b[3]["cells"], b[3]
        world["base"][key] = b
    return world["base"][key]


def assert_same(got, want, book=True, what=""):
    assert got[0] == want[0], what
    for fld in FIELDS:
        assert (bits(got[1][fld]) == bits(want[1][fld])).all(), (what, fld)
    assert got[2] == want[2], what
    assert got[4]["violations"] == 0, (what, got[4])
    if book:
        assert got[3] == want[3], (what, got[3], want[3])
        assert {k: got[4][k] for k in CHECK} == {k: want[4][k] for k in CHECK}, (what, got[4], want[4])


def check_timers(t, counts):
    """counts: name -> expected count (None: not specified).  Values: finite and >= 0; > 0 where something was counted."""
    for name, want in counts.items():
        ms, cnt = t[name + "_ms"], t["score_launches" if name == "score" else name + "_count"]
        assert math.isfinite(ms) and ms >= 0.0, (name, t)
        if want is not None:
            assert cnt == want, (name, t)
        if cnt > 0:
            assert ms > 0.0, (name, t)


# ---- 1. timing 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_timing_1_changes_nothing_and_counts_every_scan_match(pkg, world, case):
    def look(h):
        mode, first = h.frame_mode(), h.timers()
        h.set_timing(1)
        return mode, first, h.timers()
    got = run(pkg, world, case, prepare=lambda h: h.set_timing(1), inspect=look)
    want = baseline(pkg, world, case)
    assert_same(got, want, what=case)
    mode, t, again = got[5]
    assert mode["round5_frame"] == CASES[case][2], mode        # events on the cells' stream do not cost the round-5 frame
    # the map is uploaded, so no frame only seeds it: every frame scores once.  Phases are timed in mode 2 only.  The planning launches
    # are timed where the round-4 frame has any (the plan); variant 2 has none
    plan = None if ROUND5_FRAMES[case] == FRAMES else FRAMES - ROUND5_FRAMES[case] if CASES[case][3] == "plan" else 0
    check_timers(t, {"score": FRAMES, "motion": 0, "measurement": 0, "map": 0, "resample": 0, "plan": plan})
    assert all(v == 0 for v in again.values()), again          # pfslam_set_timing resets the accumulators


# ---- 2. timing 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["r5", "default100k", "default", "r4"])
def test_timing_2_leaves_the_round_5_frame_and_changes_no_result(pkg, world, case):
    """The bookkeeping of the cell rows is left out of this comparison -- and only where frames leave the round-5 loop or start it over
    (here, and in the test that switches the timing with a frame in flight): with the phases timed the rows' passes run synchronously in front of
    the scan-match kernel (launch_score: cells_sync), so cells are walked and published in other frames than in the asynchronous
    baseline -- legitimately.  The invariants still hold."""
    got = run(pkg, world, case, prepare=lambda h: h.set_timing(2), inspect=lambda h: (h.frame_mode(), h.timers()))
    assert_same(got, baseline(pkg, world, case), book=False, what=case)
    mode, t = got[5]
    assert mode["round5_frame"] is False, mode
    # cell rows and the plan are made in front of the scan-match kernel of the round-4 frame: one planning span per scoring pass
    check_timers(t, {"score": FRAMES, "motion": FRAMES, "measurement": FRAMES, "map": FRAMES, "resample": FRAMES,
                     "plan": 0 if case == "r4" else FRAMES})


def test_shard_disperse_refuses_per_phase_timing(pkg, world):
    h = pkg.PfSlam(192, kd_capacity=len(world["tree"]) + 4096)
    h.set_map(world["tree"])
    h.set_timing(2)
    with pytest.raises(pkg.PfSlamError, match="pfslam_set_timing"):
        h.shard_disperse(6, world["scans"][0])
    h.set_timing(1)                                           # a world-1 handle goes through the sharded calls otherwise
    assert h.shard_disperse(6, world["scans"][0]) is False
    h.shard_score(); h.shard_weights(); h.shard_finish()
    h.synchronize()
    assert h.trace()["best"] >= 0
    h.close()


# ---- 3. switching with frames in flight -----------------------------------------------------------------------------------------------
def test_switching_the_timing_between_frames_in_flight_drains_the_pipeline(pkg, world):
    """lag 1, a look behind every frame.  0 -> 2 behind frame 4 (frames 5 .. 8 are round-4 frames: the round-5 frames in flight are booked
    first), 2 -> 0 behind frame 8 (the frame ring starts over), 0 -> 1 behind frame 10 -- each switch while the frame just enqueued is
    still in flight."""
    switch = {3: 2, 7: 0, 9: 1}
    modes = []
    prepare = hooks(setup=lambda h: h.set_lag(1), after=lambda h, i: h.set_timing(switch[i]) if i in switch else None, modes=modes)
    got = run(pkg, world, "r5", look=1, prepare=prepare, inspect=lambda h: h.timers())
    want = baseline(pkg, world, "r5", look=1)
    for f, (a, b) in enumerate(zip(got[0], want[0])):
        assert a == b, "frame %d" % (f + 1)
    assert_same(got, want, book=False, what="switched")          # (frames 5 .. 8 ran their cell passes synchronously: see timing 2)
    assert modes == [True] * 4 + [False] * 4 + [True] * 4, modes
    check_timers(got[5], {"score": 2, "motion": 0, "measurement": 0, "map": 0, "resample": 0, "plan": None})   # what mode 1 saw: frames 11, 12
    # The bookkeeping up to the first switch: the same run cut off behind frame 4 -- the switch to mode 2 still falls on a frame in flight,
    # and booking it must leave the cell rows' counts, and what pfslam_debug_check_cells counts, where the unobserved four frames leave them.
    modes4 = []
    cut = run(pkg, world, "r5", look=1, prepare=hooks(setup=lambda h: h.set_lag(1), after=lambda h, i: h.set_timing(2) if i == 3 else None, modes=modes4),
              frames=4)
    plain = run(pkg, world, "r5", look=1, prepare=lambda h: h.set_lag(1), frames=4)
    assert modes4 == [True] * 4 and plain[3]["cells"] > 0 and cut[0] == got[0][:4] + got[0][3:4]
    assert_same(cut, plain, what="cut off behind frame 4")


# ---- 4. census log in the frames --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["r5", "default100k", "default", "r4"])
def test_census_log_changes_nothing_and_logs_every_pass(pkg, world, case):
    def look(h):
        mode, log = h.frame_mode(), h.census_log()
        h.set_census(False)                                   # keeps the records readable and stops logging
        h.step(6 + FRAMES, world["scans"][0])
        h.synchronize()
        off = h.census_log()
        h.set_census(True)                                    # ... and switching it on again empties the log
        return mode, log, off, h.census_log()
    got = run(pkg, world, case, prepare=lambda h: h.set_census(True), inspect=look)
    assert_same(got, baseline(pkg, world, case), what=case)
    mode, log, off, emptied = got[5]
    assert mode["round5_frame"] == CASES[case][2], mode
    assert len(log) == FRAMES and off == log and emptied == []
    for rec in log:
        assert rec["trips"] * 64 >= rec["visits"] >= rec["trips"] > 0 and rec["tests"] * 64 >= rec["test_lanes"] >= rec["tests"], rec
    if case == "r4":   # the plain traversal: every in-range beam of every particle tests a parent at least once
        assert all(rec["test_lanes"] >= 192 for rec in log)


# ---- 5. census on the stage path ---------------------------------------------------------------------------------------------------------
def clouds(n, k):
    p = O.make_particles(n)
    out = []
    for f in range(1, k + 1):
        O.add_noise(p, f)
        out.append(p.copy())
    return out


PER_LANE = ("visits", "test_lanes", "redescents", "redescents_noop")


@pytest.mark.parametrize("n,variant", [(192, 1), (192, 2), (192, 3), (192, 4), (64, 2), (64, 3), (64, 4)])
def test_census_replay_on_the_stage_path_leaves_the_fits_alone(pkg, world, n, variant):
    """pfslam_score_kd with the log on launches the counting instantiation behind the scan-match kernel, and that one writes the partial
    sums a second time: the fits must be those of a handle without the log (and the oracle's), one record per pass.
    Record k against pfslam_score_census on the same handle behind the pass: the record counts the logged launch itself -- same lane
    order buffer --, while pfslam_score_census is a launch of its own, and from 65 particles on a launch's lane order is the counting
    sort's: arrival order inside a Hilbert cell, so two launches may put cell-mates into different waves (PFSLAM_STABLE_ORDER
    canonicalises the round-5 frame's order only).  What two launches must agree on is therefore:
      64 particles, every variant: up to 64 particles the lane order is the identity (launch_score), so the launch is the same launch --
                all eight counters.  Variants 3 and 4 score with the shared-prefix plan there (cell rows need more than one wave, and
                with it the sorted lane order: no stage-level pass runs them with a fixed order);
      192 particles, variant 1 (identity lane order, plain traversal): all eight counters;
      192 particles, variant 2 (plain traversal): the per-lane counters, which no lane order can change; the wave-level ones (trips,
                tests, uniform and prefix trips) depend on who shares a wave and are held to their bounds;
      192 particles, variants 3 and 4: a lane's visits depend on its wave's rows / plan too, so only the bounds -- the next test holds
                the counters themselves to an independent count."""
    logged, plain = [pkg.PfSlam(n, kd_capacity=len(world["tree"]) + 4096) for _ in range(2)]
    for h in (logged, plain):
        h.set_map(world["tree"]); h.set_variant(variant); h.set_scan(world["scans"][3])
    logged.set_census(True)
    behind = []
    for p in clouds(n, 3):
        for h in (logged, plain):
            h.set_particles(p)
        fits = [logged.score_kd(), plain.score_kd()]
        assert (bits(fits[0]) == bits(fits[1])).all() and (bits(fits[0]) == bits(O.score_kd(world["tree"], p, world["scans"][3]))).all()
        behind.append(logged.score_census())
        organised = {"plan": logged.plan_stats()["rows"] > 0, "cells": logged.cell_stats()["rows"] > 0}
        assert organised == {"plan": variant == 4 or (n, variant) == (64, 3), "cells": (n, variant) == (192, 3)}, organised
    log = logged.census_log()
    assert len(log) == 3, len(log)                             # one record per pfslam_score_kd; pfslam_score_census itself logs nothing
    for k, (rec, c) in enumerate(zip(log, behind)):
        for r in (rec, c):
            assert r["trips"] * 64 >= r["visits"] >= r["trips"] > 0 and r["tests"] * 64 >= r["test_lanes"] >= r["tests"] > 0, (k, r)
            assert r["redescents_noop"] <= r["redescents"], (k, r)
            if variant in (1, 2):   # (the plan and the cell rows book the queries that found a plan / a row as prefix trips: no descent-loop trips)
                assert r["prefix_trips"] <= r["uniform_trips"] <= r["trips"], (k, r)
        if n == 64 or variant == 1:
            assert rec == c, (k, rec, c)
        if variant == 2:
            assert {key: rec[key] for key in PER_LANE} == {key: c[key] for key in PER_LANE}, (k, rec, c)
    for h in (logged, plain):
        h.close()


# ---- 6. the counters against an independent count -----------------------------------------------------------------------------------------
def test_census_counters_equal_an_independent_count_of_the_plain_traversal(pkg):
    """variant 2, the plain per-lane traversal: the four per-lane counters are exactly the sums census_ref counts over the in-range
    (particle, beam) pairs.  The plain traversal skips nothing of what kd_resume's text does: the "skipped no-op re-descents" of
    tests/test_gpu_score.py's comment are the cell-row kernel's (k_score_kd_cells books them as re-descents that changed nothing without
    walking them), which is why variants 3 and 4 are only asked for 0 < lanes <= the plain count.  Two things the count has to follow
    the kernel's text in: a test is booked BEFORE the parent index is loaded, so the test that ends at the root (H1) counts; and a
    re-descent is booked when the hyperplane test passes, also where the far side is empty (zero visits, and a no-op)."""
    tree, p, scan = census_ref.small_case(pkg)
    ref = census_ref.census(tree, p, scan)
    want_fit = O.score_kd(tree, p, scan)
    h = pkg.PfSlam(len(p), n_beams=len(scan), kd_capacity=len(tree) + 64)
    h.set_map(tree); h.set_particles(p); h.set_scan(scan)
    h.set_variant(2)
    assert (bits(h.score_kd()) == bits(want_fit)).all()
    c = h.score_census()
    got = {"visits": c["visits"], "tests": c["test_lanes"], "redescents": c["redescents"], "redescents_noop": c["redescents_noop"]}
    assert got == {k: ref[k] for k in census_ref.KEYS}, (got, {k: ref[k] for k in census_ref.KEYS})
    # wave-level counters depend on how the hardware reconverges: bounds only
    assert c["trips"] * 64 >= c["visits"] >= c["trips"] and c["tests"] * 64 >= c["test_lanes"] >= c["tests"]
    assert c["prefix_trips"] <= c["uniform_trips"] <= c["trips"]
    for v in (3, 4):
        h.set_variant(v)
        assert (bits(h.score_kd()) == bits(want_fit)).all(), v
        assert 0 < h.score_census()["visits"] <= ref["visits"], v
    h.close()


# ---- 7. log capacity ------------------------------------------------------------------------------------------------------------------
def census_raw(h, cap):
    out = np.zeros((max(cap, 1), 8), np.uint64)
    n = C.c_int(-1)
    assert h.L.pfslam_get_census_log(h._h, out.ctypes.data_as(C.c_void_p), cap, C.byref(n)) == 0
    return out, n.value


def test_census_log_stops_at_its_capacity(pkg):
    tree, _, _ = census_ref.small_case(pkg)
    n, nb = 64, 8
    p = clouds(n, 2)[-1]
    scan = np.array([3.0, 5.5, 1000.0, 7.25, 0.0, 9.0, 12.5, 4.0], np.float32)
    h = pkg.PfSlam(n, n_beams=nb, kd_capacity=len(tree) + 64)
    h.set_map(tree); h.set_particles(p); h.set_scan(scan)
    h.set_census(True)
    for _ in range(1030):
        h.score_kd(fetch=False)
    log = h.census_log(cap=2048)
    assert len(log) == 1024
    assert all(rec == log[0] for rec in log) and log[0]["visits"] > 0      # the same pass 1024 times
    assert (bits(h.score_kd()) == bits(O.score_kd(tree, p, scan))).all()
    out, count = census_raw(h, 4)
    assert count == 1024
    assert [dict(zip(CENSUS_KEYS, (int(v) for v in row))) for row in out] == log[:4]
    guard = np.full((6, 8), 0xABCD, np.uint64)                               # nothing behind row cap - 1 is written
    count = C.c_int(-1)
    assert h.L.pfslam_get_census_log(h._h, guard.ctypes.data_as(C.c_void_p), 4, C.byref(count)) == 0
    assert (guard[4:] == 0xABCD).all() and count.value == 1024
    h.close()


# ---- 8. frame probe -----------------------------------------------------------------------------------------------------------------------
def test_probe_changes_nothing(pkg, world):
    """pfslam_set_probe switches the round-5 frame to the instantiations of the scan-match kernel that also stamp when each wave ended."""
    got = run(pkg, world, "r5", prepare=lambda h: h.set_probe(8), inspect=lambda h: (h.frame_mode(), h.probe(8)))
    assert_same(got, baseline(pkg, world, "r5"), what="probe")
    mode, (names, t, last) = got[5]
    assert mode["round5_frame"] is True
    assert t.shape[0] == 8 and last >= FRAMES and (t[:, names.index("C scan-match")] > 0).all(), (last, t[:, names.index("C scan-match")])


# ---- 9. the timing helpers --------------------------------------------------------------------------------------------------------------
def test_timing_helpers_leave_the_state_alone(pkg, world):
    """pfslam_time_score_kd, pfslam_ubench_gather and pfslam_time_score_grid between two scoring calls of each kind, against a handle that
    makes the same calls without them: fits, particles (the weights pfslam_score_grid updates included), their mirror -- read behind a
    dispersion, which restores the weights from it --, pose, map and grid.  pfslam_time_score_grid's passes end in the weight update; the
    call has to put the weights back."""
    torch = pytest.importorskip("torch")
    n = 192
    p = clouds(n, 3)[-1]
    p["w"] = (1.0 + 0.25 * (np.arange(n) % 5)).astype(np.float32)
    grid = np.full((1600, 1600), -100, np.int8)
    gx = np.round(800 + world["pts"][:, 0] / 0.025).astype(int)
    gy = np.round(800 + world["pts"][:, 1] / 0.025).astype(int)
    grid[gx, gy] = np.random.RandomState(4).randint(-113, 114, len(gx))
    seen = []
    for helpers in (True, False):
        h = pkg.PfSlam(n, kd_capacity=len(world["tree"]) + 4096)
        h.set_map(world["tree"]); h.set_particles(p); h.set_scan(world["scans"][2]); h.set_grid(grid); h.set_pose((0.01, 0.02, 0.03))
        rec = {"kd": [h.score_kd()]}
        if helpers:
            ms = h.time_score_kd(3)
            ub = h.ubench_gather()
            assert math.isfinite(ms) and ms > 0.0
            assert all(math.isfinite(v) and v > 0.0 for v in ub.values()), ub
            assert ub["cus"] == torch.cuda.get_device_properties(0).multi_processor_count, ub
        rec["kd"].append(h.score_kd())
        rec["p kd"] = h.particles()
        rec["grid"] = [h.score_grid()]
        rec["p grid"] = h.particles()
        if helpers:
            k_ms, pass_ms = h.time_score_grid(3)
            assert math.isfinite(k_ms) and math.isfinite(pass_ms) and k_ms > 0.0 and pass_ms > 0.0
            after = h.particles()
            for fld in FIELDS:
                assert (bits(after[fld]) == bits(rec["p grid"][fld])).all(), fld
        rec["grid"].append(h.score_grid())
        rec["p end"] = h.particles()
        h.motion_update(9)
        rec["p mirror"] = h.particles()
        rec["pose"], rec["map"], rec["grid bytes"] = bits(h.pose).tolist(), h.map().tobytes(), h.grid().tobytes()
        h.close()
        seen.append(rec)
    a, b = seen
    assert (bits(a["kd"][0]) == bits(a["kd"][1])).all() and (a["grid"][0] == a["grid"][1]).all()
    assert len(set(a["grid"][0].tolist())) > 1                   # the grid fits differ, so every weight update changes the weights
    assert bits(a["p grid"]["w"]).tolist() != bits(a["p kd"]["w"]).tolist()
    for k in (0, 1):
        assert (bits(a["kd"][k]) == bits(b["kd"][k])).all() and (a["grid"][k] == b["grid"][k]).all()
    for key in ("p kd", "p grid", "p end", "p mirror"):
        for fld in FIELDS:
            assert (bits(a[key][fld]) == bits(b[key][fld])).all(), (key, fld)
    assert a["pose"] == b["pose"] and a["map"] == b["map"] and a["grid bytes"] == b["grid bytes"]


# ---- Part C: caller streams, in a process of their own ------------------------------------------------------------------------------------
def test_callers_streams_change_nothing():
    """tests/caller_stream_case.py: stage calls and frames on a stream the library did not create, and a change of the stream with a frame in
    flight, each against a handle on its own stream or the baseline -- computed in the child, so that no torch stream ever exists in this
    process.  Whether the frames' edges were gates or events on the caller's stream is reported in the message, not required."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "caller_stream_case.py")], capture_output=True, text=True, timeout=240)
    recs = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    seen = {r["case"]: r for r in recs}
    assert out.returncode == 0 and sorted(seen) == ["change", "frames-r4", "frames-r5", "stage-0", "stage-3"], \
        "exit %d\n%s\n%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    assert all(r["ok"] for r in recs), recs
