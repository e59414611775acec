"""Frames with odometry moves: the drives tests/test_move_frames_spec.py (CPU) and tests/test_gpu_move_frames.py (GPU) share.

TEST INFRASTRUCTURE (helper module, not a test).  A drive is pkg.synth.corridor_sequence(12, seed=5) from an empty map with a
pfslam_move_particles before every frame from the second on: the commanded motion between the sequence's poses in the frame of the earlier
one, with one of three noise settings.  The CPU oracle (oracle_lib.Slam moved by move_ref.move_oracle) goes through each (size, setting)
once; its rows, particles and map are left unchanged and shared."""
import contextlib
import os

import numpy as np

import move_ref as M
import oracle_lib as O

F = np.float32
FIELDS = ("x", "y", "theta", "w")
N_FRAMES, SEED = 12, 5
# a full covariance of a centimetre, so that the filter keeps its track
SMALL = dict(cov_scale=0.01, sigma_xy_min=0.002, sigma_theta_min=0.0005)
# standard deviations of 0.05 m, 0.03 m and 0.02 rad with CORRIDOR_COV's correlations (0.3, -0.2, 0.4) and no scale
WSD = (0.05, 0.03, 0.02)
WIDE_COV = np.array([WSD[0] * WSD[0], 0.3 * WSD[0] * WSD[1], -0.2 * WSD[0] * WSD[2], WSD[1] * WSD[1], 0.4 * WSD[1] * WSD[2], WSD[2] * WSD[2]], F)
# setting -> (cov, options besides ref_theta)
SETTINGS = {
    "small": (M.CORRIDOR_COV, SMALL),
    "wide": (WIDE_COV, {}),
    "floors": (None, dict(sigma_xy_min=0.002, sigma_theta_min=0.0005)),
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@contextlib.contextmanager
def oracle_threads(k=16):
    old = os.environ.get("ORC_THREADS")
    os.environ["ORC_THREADS"] = str(k)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("ORC_THREADS", None)
        else:
            os.environ["ORC_THREADS"] = old


def corridor(pkg, n_frames=N_FRAMES, seed=SEED):
    _, frames = pkg.synth.corridor_sequence(n_frames, seed=seed)
    return frames


def commanded(frames, setting, first=2):
    """{frame: (delta, cov, opts)} for every frame from `first` on: the motion between the sequence's poses, in the earlier pose's frame of
    heading.  (Frame 1 has no earlier pose: first=1 commands a step of the same length as the second's there.)"""
    cov, opts = SETTINGS[setting]
    moves = {}
    for f in range(max(first, 2), len(frames) + 1):
        prev, cur = np.array(frames[f - 2][0], F), np.array(frames[f - 1][0], F)
        moves[f] = (cur - prev, cov, dict(ref_theta=float(prev[2]), **opts))
    if first < 2:
        moves[1] = moves[2]
    return moves


def row_of(e):
    """what is compared after every frame: the trace without Neff, and the pose bits"""
    t = e.trace()
    return (t["best"], t["resampled"], t["n_wall"], t["n_free"], t["n_insert"], t["kd_size"]) + tuple(bits(e.pose).tolist())


def apply_moves(e, mv, oracle=False):
    """mv: one (delta, cov, opts) or a list of them, applied in order with the frame number each carries"""
    for frame, delta, cov, opts in mv:
        if oracle:
            M.move_oracle(e, frame, delta, cov, **opts)
        else:
            e.move_particles(frame, delta, cov, **opts)


def schedule(moves):
    """{frame: (delta, cov, opts)} -> {frame: [(frame, delta, cov, opts)]}, the form run() takes (several moves before one frame, and a
    frame number of the draw that is not the frame's)"""
    return {f: [(f,) + tuple(m)] for f, m in moves.items()}


def run(e, frames, sched, oracle=False, look=True, before=None):
    """Step e through the frames with the scheduled moves in front of them.  look: read a row after every frame (a getter books the frames
    in flight; look=False leaves them in flight and returns no rows).  before: {frame: fn(e)} called between the moves and the frame."""
    rows = []
    for f, (_, scan) in enumerate(frames, start=1):
        apply_moves(e, sched.get(f, ()), oracle)
        if before and f in before:
            before[f](e)
        e.step(f, scan)
        if look:
            rows.append(row_of(e))
    return rows


def final(e):
    return dict(pose=np.array(e.pose, F), particles=e.particles().copy(), map=(e.map() if hasattr(e, "map") else e.tree()).tobytes())


_ORACLE = {}


def oracle_run(pkg, key, n, frames, sched, before=None, **kw):
    """The CPU oracle through a drive, once per key: rows, pose, particles, map; read-only."""
    if key not in _ORACLE:
        with oracle_threads():
            o = O.Slam(n, kd_capacity=1 << 16, **kw)
            rows = run(o, frames, sched, oracle=True, before=before)
            out = final(o)
            o.close()
        out["rows"] = rows
        out["particles"].setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def oracle_drive(pkg, n, setting):
    """The standard drive of a setting at n particles."""
    frames = corridor(pkg)
    return oracle_run(pkg, ("drive", n, setting), n, frames, schedule(commanded(frames, setting)))


def assert_conditions(rows, what, resample_from=2):
    """A drive cannot pass vacuously: at least one frame resamples behind a move, and every frame from the second on inserts nodes."""
    assert any(r[1] for r in rows[resample_from - 1:]), "%s: no frame resamples behind a move" % what
    assert all(r[4] > 0 for r in rows[1:]), "%s: a frame inserts nothing: %s" % (what, [r[4] for r in rows])


def assert_same_particles(got, want, what=""):
    for fld in FIELDS:
        bad = np.flatnonzero(bits(got[fld]) != bits(want[fld]))
        assert len(bad) == 0, "%s: %d of %d particles differ in %s, first %s" % (what, len(bad), len(want), fld, bad[:8])


def assert_same_end(got, want, what=""):
    assert (bits(got["pose"]) == bits(want["pose"])).all(), (what, got["pose"], want["pose"])
    assert_same_particles(got["particles"], want["particles"], what)
    assert got["map"] == want["map"], "%s: maps differ" % what
