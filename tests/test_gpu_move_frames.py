"""Frames with pfslam_move_particles between them, held to the CPU oracle (oracle_lib.Slam moved by move_ref.move_oracle, itself held to
the oracle's shift by tests/test_move_frames_spec.py) in every frame mode.  Every comparison is bit for bit: after a frame the pose bits and
the trace (best, resampled, n_wall, n_free, n_insert, kd_size), at the end the particles in all four fields and the map bytes.

The drive (tests/move_frames.py) is corridor_sequence(12, seed=5) from an empty map with the commanded motion before every frame from the
second on, under three noise settings: "small" (CORRIDOR_COV scaled to a centimetre, floors), "wide" (standard deviations of 0.05 m,
0.03 m and 0.02 rad, CORRIDOR_COV's correlations, no scale) and "floors" (cov NULL).  Every drive's oracle rows must show a resample behind
a move and inserts in every frame from the second on, so that no case passes on frames that do nothing.

Where the instantiations switch (tests/test_gpu_size_edges.py): the frame loop takes lattice-cell rows, and with them round-5 frames, from
65 particles on while the cloud is narrow enough for its size; set_variant(3) forces the rows at any count above 64, set_variant(2) the
staged chain with the plain traversal and set_variant(4) the staged chain with the shared-prefix plan, which the default handle's staged
frames take only from PLAN_MIN = 4608 particles on.  300 and 3000 are below PLAN_MIN and below the 4096 of k_resample_small; 4608 and 5000
(the heading bound) are above both; 30001 / 3 ranks is the sharded round-5 size.

Where a second handle is the reference (the shadow in device-library and resampler modes, the single handle at 30001 particles) the
docstring says why the oracle cannot be.

Seconds on one MI355X, the slowest case of each test (the first test of a session that imports torch pays some 11 s for it once):
modes and variants 0.47, frames in flight 0.04, staged chain's plan 0.47, smallest round-5 size 0.17, widening turn 0.42, two moves and a
getter 0.22, re-balance frame 0.23, first frame 0.23, heading bound 0.56, resampler modes 0.04, shadow == oracle == frame 0.71, device
library 0.04, virtual ranks 1001 0.26, virtual ranks 30001 0.18, asynchronous ranks 0.75, queries 0.10; tests/test_gpu_move.py's new
cases 0.03 or less each."""
import numpy as np
import pytest

import move_frames as MF
import move_ref as M
import oracle_lib as O
from stage_shadow import StageShadow
from test_gpu_sharded import _VirtualRanks, _bench_like

pytestmark = pytest.mark.gpu
F = np.float32
bits = MF.bits
PLAN_MIN = 4608                      # tests/test_gpu_size_edges.py
R5_MIN = 65                          # the smallest count that runs round-5 frames without a forced variant
KD = dict(kd_capacity=1 << 16)

HANDLES = {
    "default": lambda h: None,
    "serial": lambda h: h.set_serial(1),
    "lag0": lambda h: h.set_lag(0),
    "variant2": lambda h: h.set_variant(2),
    "variant3": lambda h: h.set_variant(3),
}


def gpu_run(pkg, n, frames, sched, prepare=None, look=True, before=None, **kw):
    """A fresh handle through MF.run: (rows, end state, frame mode, cell statistics)."""
    h = pkg.PfSlam(n, **dict(KD, **kw))
    if prepare:
        prepare(h)
    rows = MF.run(h, frames, sched, look=look, before=before)
    fm = h.frame_mode()
    end = MF.final(h)
    cs = h.cell_stats()
    h.close()
    return rows, end, fm, cs


def assert_rows(got, want, what):
    bad = [i + 1 for i in range(len(want)) if got[i] != want[i]]
    assert not bad, "%s: frames %s differ from the oracle; first: %s against %s" % (what, bad, got[bad[0] - 1], want[bad[0] - 1])


# ---- 1. modes and variants ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", sorted(MF.SETTINGS))
@pytest.mark.parametrize("n", [300, 3000])
def test_frames_with_moves_equal_the_oracle_in_every_mode_and_variant(pkg, n, setting):
    """The default handle (a frame in flight when the move is enqueued), one stream, every frame booked, the staged chain and forced cell
    rows: each equals the oracle after every frame and at the end.  With set_variant(3) the last frame was a round-5 frame on cell rows,
    with set_variant(2) it was not."""
    frames = MF.corridor(pkg)
    sched = MF.schedule(MF.commanded(frames, setting))
    want = MF.oracle_drive(pkg, n, setting)
    MF.assert_conditions(want["rows"], "%d particles, %s" % (n, setting))
    for name in sorted(HANDLES):
        rows, end, fm, cs = gpu_run(pkg, n, frames, sched, HANDLES[name])
        what = "%d particles, %s, %s" % (n, setting, name)
        assert_rows(rows, want["rows"], what)
        MF.assert_same_end(end, want, what)
        if name == "variant3":
            assert fm["round5_frame"] and cs["rows"] > 0, (what, fm, cs)
        if name == "variant2":
            assert not fm["round5_frame"] and cs["rows"] == 0, (what, fm, cs)
        if name == "serial":
            assert fm["serial"], (what, fm)


@pytest.mark.parametrize("setting", sorted(MF.SETTINGS))
def test_frames_in_flight_with_moves_equal_the_oracle(pkg, setting):
    """No getter between the first frame and the last at 3000 particles: the moves are enqueued behind frames really in flight, on forced
    cell rows and in the default organisation; only the end is compared."""
    n = 3000
    frames = MF.corridor(pkg)
    sched = MF.schedule(MF.commanded(frames, setting))
    want = MF.oracle_drive(pkg, n, setting)
    for name in ("default", "variant3"):
        _, end, fm, cs = gpu_run(pkg, n, frames, sched, HANDLES[name], look=False)
        MF.assert_same_end(end, want, "%s, %s, in flight" % (setting, name))
        if name == "variant3":
            assert fm["round5_frame"] and cs["rows"] > 0, (fm, cs)


def test_frames_with_moves_on_the_staged_chains_plan_equal_the_oracle(pkg):
    """PLAN_MIN = 4608 particles (above the 4096 of k_resample_small: the tiled resample), "wide" moves, every frame against the oracle:
    set_variant(4) runs the staged chain with the shared-prefix plan, set_variant(2) with the plain traversal, and the default handle takes
    cell rows while the cloud's spread allows and otherwise the staged chain, which has the plan from this count on."""
    n = PLAN_MIN
    frames = MF.corridor(pkg)
    sched = MF.schedule(MF.commanded(frames, "wide"))
    want = MF.oracle_drive(pkg, n, "wide")
    MF.assert_conditions(want["rows"], "%d particles" % n)
    for name, prepare in (("variant4", lambda h: h.set_variant(4)), ("variant2", HANDLES["variant2"]), ("default", None)):
        h = pkg.PfSlam(n, **KD)
        if prepare:
            prepare(h)
        ran = []
        for f, (_, scan) in enumerate(frames, start=1):
            MF.apply_moves(h, sched.get(f, ()))
            h.step(f, scan)
            assert MF.row_of(h) == want["rows"][f - 1], (name, f)
            ran.append((h.frame_mode()["round5_frame"], h.cell_stats()["rows"] > 0, h.plan_stats()["rows"] > 0))
        MF.assert_same_end(MF.final(h), want, name)
        h.close()
        print("%d particles, %s: (round-5 frame, cell rows, plan rows) per frame: %s" % (n, name, ran))
        if name == "variant4":
            assert all(r == (False, False, True) for r in ran[1:]), ran
        elif name == "variant2":
            assert all(r == (False, False, False) for r in ran[1:]), ran
        else:
            assert ran[1][:2] == (True, True), ran
            assert all(r[1:] == ((True, False) if r[0] else (False, True)) for r in ran[1:]), ran


def test_the_smallest_round5_size_without_a_forced_variant(pkg):
    """65 particles, the default handle, "small" moves: the first stepped frame, a move in front of it, is a round-5 frame on cell rows
    (the frame loop's own threshold).  So few particles leave the rows once the corridor's cloud has spread (measured: every later frame
    of this drive took the staged chain, as the 125-particle shards of tests/test_gpu_sharded_async.py do), and every frame equals the
    oracle whichever organisation it took."""
    n = R5_MIN
    frames = MF.corridor(pkg)
    sched = MF.schedule(MF.commanded(frames, "small"))
    want = MF.oracle_drive(pkg, n, "small")
    MF.assert_conditions(want["rows"], "65 particles")
    h = pkg.PfSlam(n, **KD)
    seen = []
    for f, (_, scan) in enumerate(frames, start=1):
        MF.apply_moves(h, sched.get(f, ()))
        h.step(f, scan)
        assert MF.row_of(h) == want["rows"][f - 1], f
        seen.append((h.frame_mode()["round5_frame"], h.cell_stats()["rows"] > 0))
    print("65 particles: (round-5 frame, cell rows) per frame: %s" % seen)
    assert seen[1] == (True, True), seen
    MF.assert_same_end(MF.final(h), want, "65 particles")
    h.close()


# ---- 2. a move that widens and turns the cloud between two round-5 frames ------------------------------------------------------------------
TURN_N, TURN_AT = 3000, 6
TURN_SD = (0.5, 0.5, 0.1)
TURN_COV = np.array([TURN_SD[0] ** 2, 0, 0, TURN_SD[1] ** 2, 0, TURN_SD[2] ** 2], F)
TURN_DELTA = np.array([0.3, -0.2, 2.5], F)
_TURN = {}


def turn_drive(pkg):
    """The oracle first: the move's ref_theta is one radian away from the heading its pose has behind frame 5."""
    if not _TURN:
        frames = MF.corridor(pkg)
        sched = MF.schedule(MF.commanded(frames, "small"))
        with MF.oracle_threads():
            o = O.Slam(TURN_N, **KD)
            rows = MF.run(o, frames[:TURN_AT - 1], sched, oracle=True)
            ref = float(o.pose[2]) + 1.0
            sched[TURN_AT] = [(TURN_AT, TURN_DELTA, TURN_COV, dict(ref_theta=ref))]
            for f in range(TURN_AT, len(frames) + 1):
                MF.apply_moves(o, sched.get(f, ()), oracle=True)
                o.step(f, frames[f - 1][1])
                rows.append(MF.row_of(o))
            want = MF.final(o)
            o.close()
        want["rows"] = rows
        _TURN.update(frames=frames, sched=sched, want=want)
    return _TURN["frames"], _TURN["sched"], _TURN["want"]


@pytest.mark.parametrize("look", [False, True], ids=["in flight", "booked"])
def test_a_move_that_widens_and_turns_the_cloud_between_two_round5_frames(pkg, look):
    """set_variant(3) at 3000 particles; before frame 6 one move with standard deviations of 0.5 m, 0.5 m and 0.1 rad, delta (0.3, -0.2,
    2.5) and ref_theta a radian off the pose's heading.  The header says the cloud statistics the next lane order starts from move by the
    pose's increment only and keep their spread ("performance only"): here the spread they keep is wrong by a factor of fifty and the
    turn moves every particle off the pose's increment, so a result that leaned on them would differ.  The rows may be wiped or groups go
    unmarked; every following frame equals the oracle.  In flight: no getter between frame 1 and the end."""
    frames, sched, want = turn_drive(pkg)
    MF.assert_conditions(want["rows"], "the turn", resample_from=TURN_AT)
    rows, end, fm, cs = gpu_run(pkg, TURN_N, frames, sched, HANDLES["variant3"], look=look)
    print("cell statistics behind the turn (%s): %s" % ("booked" if look else "in flight", {k: cs[k] for k in ("rows", "wipes", "suspended", "cells_without_row")}))
    if look:
        assert_rows(rows, want["rows"], "the turn")
    MF.assert_same_end(end, want, "the turn")
    assert fm["round5_frame"] and cs["rows"] > 0, (fm, cs)


# ---- 3. moves back to back, a getter behind a move, the re-balance frame, the first frame ------------------------------------------------
_BEHIND = {}


@pytest.mark.parametrize("name", ["default", "variant3", "lag0"])
def test_two_moves_before_one_frame_and_a_getter_right_behind_a_move(pkg, name):
    """1000 particles.  Frame 4 has two moves in front of it (the second draws under frame number 104, so that the two draws differ);
    behind the move in front of frame 7 the pose and the particles are read -- the getter books the frames in flight and must show the
    moved cloud -- and checked against the oracle before the frame runs; then further frames."""
    n = 1000
    frames = MF.corridor(pkg)
    moves = MF.commanded(frames, "wide")
    sched = MF.schedule(moves)
    sched[4] = sched[4] + [(104,) + tuple(MF.commanded(frames, "small")[4])]
    seen = _BEHIND                                            # (filled once: the oracle's run is shared between the cases)

    def oracle_look(o):
        seen["pose"], seen["particles"] = np.array(o.pose, F), o.particles().copy()

    want = MF.oracle_run(pkg, ("back to back", n), n, frames, sched, before={7: oracle_look})
    assert not (bits(seen["pose"]) == bits(want["rows"][5][6:9])).any()      # (the pose behind the move is not the one frame 6 left)
    MF.assert_conditions(want["rows"], "back to back")

    def look(h):
        assert (bits(h.pose) == bits(seen["pose"])).all(), (h.pose, seen["pose"])
        MF.assert_same_particles(h.particles(), seen["particles"], "behind the move in front of frame 7")

    rows, end, _, _ = gpu_run(pkg, n, frames, sched, HANDLES[name], before={7: look})
    assert_rows(rows, want["rows"], name)
    MF.assert_same_end(end, want, name)


def test_a_move_in_front_of_the_rebalance_frame(pkg):
    """balance_period = 10: frame 5 rebuilds the tree on the host, with a "wide" move enqueued in front of it and frames in flight around
    it (set_variant(3), no getter before the end), and once more with every frame read."""
    n = 1000
    frames = MF.corridor(pkg)
    sched = MF.schedule(MF.commanded(frames, "wide"))
    want = MF.oracle_run(pkg, ("rebalance", n), n, frames, sched, balance_period=10)
    MF.assert_conditions(want["rows"], "re-balance")
    for look in (False, True):
        rows, end, fm, cs = gpu_run(pkg, n, frames, sched, HANDLES["variant3"], look=look, balance_period=10)
        if look:
            assert_rows(rows, want["rows"], "re-balance")
        MF.assert_same_end(end, want, "re-balance, look %s" % look)
        assert fm["round5_frame"] and cs["rows"] > 0


def test_a_move_in_front_of_the_very_first_frame(pkg):
    """The map is empty: the seed frame puts the pose at 0 whatever the move made of it, and the particles are what the oracle says --
    moved, with noise, before anything was dispersed.  Default handle and forced cell rows."""
    n = 1000
    frames = MF.corridor(pkg)
    sched = MF.schedule(MF.commanded(frames, "wide", first=1))
    assert 1 in sched
    want = MF.oracle_run(pkg, ("first frame", n), n, frames, sched)
    MF.assert_conditions(want["rows"], "first frame")
    assert want["rows"][0][6:9] == (0, 0, 0)                  # (the seed frame's pose: +0.0 three times)
    for name in ("default", "variant3"):
        rows, end, _, _ = gpu_run(pkg, n, frames, sched, HANDLES[name])
        assert_rows(rows, want["rows"], name)
        MF.assert_same_end(end, want, name)


# ---- 4. the heading bound ----------------------------------------------------------------------------------------------------------------
TURNS = [164, 1 << 18]


@pytest.mark.parametrize("look", [False, True], ids=["in flight", "booked"])
@pytest.mark.parametrize("turns", TURNS)
def test_the_heading_bound_against_the_oracle(pkg, turns, look):
    """tests/test_gpu_move.py's drive -- one move of 164 full turns between two frames in flight, 5000 particles on cell rows -- against
    the oracle instead of a second handle, with no getter before the end and with every frame read.  At 1030 rad the scan-match kernel's
    angle-sum form without the guard still gives the direct form's results, so a bound that did not move with the call is not seen there:
    the library with `theta_bound += ad` taken out of enqueue_odometry passes the 164 turns (and 32 768 turns, 2.06e5 rad: the end points
    move by micrometres and no score changes).  The second drive turns 2^18 times, to 1.65e6 rad, where a float heading resolves 0.125 rad
    and the unguarded form is wrong by millimetres: that library fails it, in flight and booked (a booked header rebuilds the bound from
    theta_shift, but not before the next frame has chosen its kernel)."""
    n, nframes = 5000, 14
    frames = MF.corridor(pkg, nframes, seed=13)
    sched = {6: [(6, np.array([0.0, 0.0, turns * 2 * np.pi], F), M.CORRIDOR_COV, dict(ref_theta=0.0, **MF.SMALL))]}
    want = MF.oracle_run(pkg, ("heading bound", n, turns), n, frames, sched)
    assert any(r[1] for r in want["rows"][5:]) and all(r[4] > 0 for r in want["rows"][1:])
    assert float(want["pose"][2]) > 1024.0 * turns / 164
    rows, end, fm, cs = gpu_run(pkg, n, frames, sched, HANDLES["variant3"], look=look)
    if look:
        assert_rows(rows, want["rows"], "booked")
    MF.assert_same_end(end, want, "%d turns" % turns)
    assert fm["round5_frame"] and cs["rows"] > 0


# ---- 5. resampler modes 1 and 2 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_resampler_modes_with_moves_equal_the_shadow(pkg, mode):
    """The oracle has the reference's resampler only; the shadow (the frame composed of stage calls, as tests/test_gpu_resampler.py uses
    it for these modes) is given the same "small" moves at 1000 particles.  Default handle and forced cell rows."""
    n = 1000
    frames = MF.corridor(pkg)
    sched = MF.schedule(MF.commanded(frames, "small"))
    s = StageShadow(n, pkg=pkg, **KD)
    s.h.set_resampler(mode)
    want_rows = MF.run(s, frames, sched)
    want = MF.final(s)
    s.close()
    MF.assert_conditions(want_rows, "resampler %d" % mode)
    for name in ("default", "variant3"):
        def prepare(h):
            h.set_resampler(mode)
            HANDLES[name](h)
        rows, end, _, _ = gpu_run(pkg, n, frames, sched, prepare)
        assert_rows(rows, want_rows, "resampler %d, %s" % (mode, name))
        MF.assert_same_end(end, want, "resampler %d, %s" % (mode, name))


# ---- 6. device-library mode --------------------------------------------------------------------------------------------------------------
def test_the_shadow_with_moves_is_the_oracle_and_the_frame_in_the_default_mode(pkg):
    """What licenses the shadow as the reference of the next test: at 1000 particles StageShadow with moves == O.Slam with move_oracle ==
    pfslam_step with moves, every frame, under all three settings."""
    n = 1000
    frames = MF.corridor(pkg)
    for setting in sorted(MF.SETTINGS):
        sched = MF.schedule(MF.commanded(frames, setting))
        want = MF.oracle_drive(pkg, n, setting)
        MF.assert_conditions(want["rows"], setting)
        s = StageShadow(n, pkg=pkg, **KD)
        assert_rows(MF.run(s, frames, sched), want["rows"], "shadow, %s" % setting)
        MF.assert_same_end(MF.final(s), want, "shadow, %s" % setting)
        s.close()
        rows, end, _, _ = gpu_run(pkg, n, frames, sched)
        assert_rows(rows, want["rows"], "frame, %s" % setting)
        MF.assert_same_end(end, want, "frame, %s" % setting)


@pytest.mark.parametrize("setting", ["small", "wide"])
def test_device_library_frames_with_moves_equal_the_shadow(pkg, setting):
    """pfslam_set_trig(1) at 3000 particles, where the CPU oracle cannot follow: pfslam_step with moves == StageShadow(trig=1) with the
    same moves, bit for bit, in the default organisation and on forced cell rows."""
    n = 3000
    frames = MF.corridor(pkg)
    sched = MF.schedule(MF.commanded(frames, setting))
    s = StageShadow(n, pkg=pkg, trig=1, **KD)
    want_rows = MF.run(s, frames, sched)
    want = MF.final(s)
    s.close()
    MF.assert_conditions(want_rows, "device library, %s" % setting)
    for variant in (0, 3):
        def prepare(h):
            h.set_trig(1)
            if variant:
                h.set_variant(variant)
        rows, end, fm, cs = gpu_run(pkg, n, frames, sched, prepare)
        assert_rows(rows, want_rows, "device library, variant %d" % variant)
        MF.assert_same_end(end, want, "device library, variant %d" % variant)
        if variant == 3:
            assert fm["round5_frame"] and cs["rows"] > 0


# ---- 7. sharded frames -------------------------------------------------------------------------------------------------------------------
def ranks_end(v):
    for e in v.engs:
        e.synchronize()
    got = [e.particles() for e in v.engs]
    maps = {e.map().tobytes() for e in v.engs}
    assert len(maps) == 1
    return dict(pose=np.array(v.pose, F), particles={fld: np.concatenate([g[fld] for g in got]) for fld in MF.FIELDS}, map=maps.pop())


@pytest.mark.parametrize("setting", ["small", "wide"])
def test_virtual_ranks_with_moves_equal_the_oracle_and_the_single_handle(pkg, setting):
    """1001 particles on 3 ranks (334 + 334 + 333), a move on every rank before every frame from the second on: every rank's pose and
    trace equal the oracle's in every frame, the concatenated shards and every rank's map at the end; the single handle equals the oracle
    too."""
    torch = pytest.importorskip("torch")
    n = 1001
    frames = MF.corridor(pkg)
    sched = MF.schedule(MF.commanded(frames, setting))
    want = MF.oracle_drive(pkg, n, setting)
    MF.assert_conditions(want["rows"], "1001 particles, %s" % setting)
    v = _VirtualRanks(pkg, torch, n, 3, **KD)
    assert [cnt for _, _, cnt in v.lay] == [334, 334, 333]
    assert_rows(MF.run(v, frames, sched), want["rows"], "3 ranks, %s" % setting)
    MF.assert_same_end(ranks_end(v), want, "3 ranks, %s" % setting)
    v.close()
    rows, end, _, _ = gpu_run(pkg, n, frames, sched)
    assert_rows(rows, want["rows"], "one handle, %s" % setting)
    MF.assert_same_end(end, want, "one handle, %s" % setting)


BENCH_DELTA = np.array([0.002, 0.001, 0.0004], F)      # the motion between two scans of test_gpu_sharded._bench_like


def bench_sched(setting, first, count):
    cov, opts = MF.SETTINGS[setting]
    return {f: [(f, BENCH_DELTA, cov, dict(ref_theta=0.0004 * (f - first - 1), **opts))] for f in range(first + 1, first + count)}


def bench_run(e, tree, scans, sched, step, first=6, after=None):
    """test_gpu_sharded._run with moves: the map, five dispersions, frames 6 ... with the scheduled moves in front of them and no getter."""
    e.set_map(tree)
    for f in range(1, 6):
        e.motion_update(f)
    for i, s in enumerate(scans):
        MF.apply_moves(e, sched.get(first + i, ()))
        step(first + i, s)
        if after:
            after(i)


@pytest.mark.parametrize("setting,force", [("small", False), ("wide", True), ("wide", False)], ids=["small", "wide-variant3", "wide-default"])
def test_virtual_ranks_at_cell_row_sizes_with_moves_equal_the_single_handle(pkg, setting, force):
    """30001 particles on 3 ranks (10001 + 10001 + 9999) on the fixed 20 000-point map, too many for the CPU oracle in a test of seconds:
    the reference is ONE handle with the same moves (held to the oracle at the sizes above).  The sharded frames are round-5 frames on
    every rank, as test_virtual_ranks_run_round5_frames_at_cell_row_sizes asserts without moves.  Under "wide" moves the cloud grows too
    wide for its size and the default handle goes back to the staged chain (measured: the single handle's last frame was no round-5
    frame), so that setting runs with set_variant(3) on every handle, which keeps the cell rows whatever the spread -- and once more in
    the default organisation, where each rank falls back to the staged chain when its own shard says so: there only the equality with the
    single handle is asserted."""
    torch = pytest.importorskip("torch")
    n, world, nframes = 30001, 3, 12
    tree, scans = _bench_like(pkg, n, n_frames=nframes)
    sched = bench_sched(setting, 6, nframes)
    cap = len(tree) + (1 << 18)
    rows_meant = setting == "small" or force
    one = pkg.PfSlam(n, kd_capacity=cap)
    if force:
        one.set_variant(3)
    poses_one = []
    bench_run(one, tree, scans, sched, one.step, after=lambda i: poses_one.append(bits(one.pose).tolist()))
    assert one.frame_mode()["round5_frame"] or not rows_meant
    want = MF.final(one)
    flags_one = one.trace()["resampled"]
    one.close()
    v = _VirtualRanks(pkg, torch, n, world, kd_capacity=cap)
    if force:
        for e in v.engs:
            e.set_variant(3)
    poses, r5 = [], []

    class Both:                                           # (bench_run's engine: the calls go to every rank)
        def set_map(self, t):
            for e in v.engs:
                e.set_map(t)

        def motion_update(self, f):
            for e in v.engs:
                e.motion_update(f)

        def move_particles(self, *a, **kw):
            v.move_particles(*a, **kw)

    def after(i):
        r5.append(all(e.frame_mode()["round5_frame"] for e in v.engs))
        poses.append(bits(v.pose).tolist())

    bench_run(Both(), tree, scans, sched, v.step, after=after)
    print("round-5 frames on every rank: %s" % r5)
    assert sum(r5) >= nframes - 3 or not rows_meant, r5
    assert poses == poses_one
    assert v.trace()["resampled"] == flags_one
    MF.assert_same_end(ranks_end(v), want, "3 ranks of 30001, %s" % setting)
    v.close()


def test_async_ranks_with_moves_under_delayed_gathers_equal_the_single_handle(pkg):
    """tests/test_gpu_sharded_async.py's w3_ragged job (30001 particles, 3 ranks, asynchronous all-gathers on the frame's own streams, no
    host wait inside a frame) with a "small" move enqueued on every rank between frames while the delayed gather of the frame before is
    still outstanding: the pose blocks' gather delayed, then the weights'.  The result equals the single handle with the same moves."""
    torch = pytest.importorskip("torch")
    import test_gpu_sharded_async as A
    wl = A._Workload(pkg, "w3_ragged")
    sched = bench_sched("small", wl.first, len(wl.scans))
    ms_per_frame = min(A._single(pkg, wl, read=False)["ms_per_frame"] for _ in range(2))    # (undelayed frames, as that module times them)
    one = pkg.PfSlam(wl.n, kd_capacity=wl.cap)
    bench_run(one, wl.tree, wl.scans, sched, one.step, first=wl.first)
    want = MF.final(one)
    want_trace = {k: v for k, v in one.trace().items() if k in A.TRACE}
    one.close()
    for delay_k in (0, 2):
        job = A._AsyncJob(pkg, torch, wl, "concurrent")                    # (prepares every rank: the map and the five dispersions)
        cycles = A._delay_cycles(A._calibrate_sleep(torch, job.engs[0].shard_stream(0)), ms_per_frame)
        modes = []
        for i, (f, s) in enumerate(zip(wl.frame_ids(), wl.scans)):
            for e in job.engs:
                MF.apply_moves(e, sched.get(f, ()))
            job.step(f, s, delay_k, cycles if i >= A.FIRST_DELAYED else 0)
            modes.append([e.frame_mode()["round5_frame"] for e in job.engs])    # (host state: books nothing)
        ms = A._check_spans(torch, job.coll.spans, delay_k, len(wl.scans) - A.FIRST_DELAYED, wl.world, ms_per_frame)
        print("delay %d: %d delays of %.2f .. %.2f ms, an undelayed frame %.3f ms" % (delay_k, len(ms), min(ms), max(ms), ms_per_frame))
        for e in job.engs:
            e.synchronize()
        for r in range(wl.world):
            assert sum(row[r] for row in modes) >= len(wl.scans) - 3, (delay_k, r, [row[r] for row in modes])
        for r, e in enumerate(job.engs):
            assert {k: v for k, v in e.trace().items() if k in A.TRACE} == want_trace, (delay_k, r)
            assert (bits(e.pose) == bits(want["pose"])).all(), (delay_k, r)
            assert e.map().tobytes() == want["map"], (delay_k, r)
            assert e.check_cells()["violations"] == 0, (delay_k, r)
        got = [e.particles() for e in job.engs]
        MF.assert_same_particles({fld: np.concatenate([g[fld] for g in got]) for fld in MF.FIELDS}, want["particles"], "delay %d" % delay_k)
        job.close()


# ---- 8. query calls behind a move --------------------------------------------------------------------------------------------------------
QUERY_N, QUERY_AT = 1000, 6
_QUERY = {}


def query_state(pkg):
    """The oracle behind frame 5 and the move in front of frame 6: (frames, schedule, particles, pose, tree)."""
    if not _QUERY:
        frames = MF.corridor(pkg)
        sched = MF.schedule(MF.commanded(frames, "wide"))
        with MF.oracle_threads():
            o = O.Slam(QUERY_N, **KD)
            MF.run(o, frames[:QUERY_AT - 1], sched, oracle=True)
            _QUERY.update(before=(o.particles().copy(), np.array(o.pose, F)))
            MF.apply_moves(o, sched[QUERY_AT], oracle=True)
            _QUERY.update(frames=frames, sched=sched, particles=o.particles().copy(), pose=np.array(o.pose, F), tree=o.tree().copy())
            o.close()
    return _QUERY


def query_fresh(pkg, q, query, particles, pose):
    fresh = pkg.PfSlam(QUERY_N, **KD)
    fresh.set_map(q["tree"])
    fresh.set_scan(q["frames"][QUERY_AT - 2][1])
    fresh.set_particles(particles)
    fresh.set_pose(pose)
    out = QUERIES[query](fresh)
    fresh.close()
    return out


QUERIES = {
    "search": lambda h: (lambda r: (bits(r["pose"]).tolist(), bits(r["info"]).tolist()))(h.search(None, half_x=6, half_y=6, half_theta=6)),
    "cast_score": lambda h: (lambda r: (r["rows"].tolist(), r["best"], r["stats"].tolist()))(h.cast_score(particles=True)),
    "estimate": lambda h: bits(h.estimate_raw()).tolist(),
}


@pytest.mark.parametrize("variant", [0, 3])
@pytest.mark.parametrize("query", sorted(QUERIES))
def test_a_query_right_behind_a_move_sees_the_moved_pose_and_cloud(pkg, query, variant):
    """Five frames with moves and no getter, the move in front of frame 6, then -- with nothing in between -- search(None, ...) around the
    handle's pose, cast_score on the handle's own particles, or estimate(): each equals the same call on a fresh handle that was uploaded
    the oracle's map, scan, moved particles and moved pose.  A query that read the cloud or the pose of before the move would differ: the
    answer on the cloud and pose of before the move is computed as well, and is another one."""
    q = query_state(pkg)
    h = pkg.PfSlam(QUERY_N, **KD)
    if variant:
        h.set_variant(variant)
    MF.run(h, q["frames"][:QUERY_AT - 1], q["sched"], look=False)
    MF.apply_moves(h, q["sched"][QUERY_AT])
    got = QUERIES[query](h)
    MF.assert_same_particles(h.particles(), q["particles"], "behind the query")
    h.close()
    want = query_fresh(pkg, q, query, q["particles"], q["pose"])
    stale = query_fresh(pkg, q, query, *q["before"])
    assert want != stale, "%s cannot tell the moved state from the one before" % query
    assert got == want, query
