"""Child-process driver of tests/test_gpu_observers.py's caller-stream test: pfslam_set_stream with a stream the library did not create.

A process of its own, because a torch stream takes one of the runtime's hardware queues for as long as the process lives: the stream
gates' self-test of every handle created afterwards may then find two of its streams on one queue and leave that handle's edges events
(gates_selftest, csrc/pfslam_frame.hip.inc) -- the documented fallback, but tests that assert gates must not run behind it.  So the
baselines AND the caller-stream runs are computed here, and torch's streams never exist in the pytest process.
    python tests/caller_stream_case.py
Cases (world, baseline and helpers are tests/test_gpu_observers.py's):
  stage-0, stage-3   pfslam_motion_update, pfslam_score_kd, pfslam_measurement_update, pfslam_icp, pfslam_update_map_kd and pfslam_resample --
                     a frame as tests/stage_shadow.py composes it -- on the caller's stream against a handle on its own stream, variants 0, 3
  frames-r5, -r4     12 frames with the handle's particle chain on the caller's stream (the other three streams of a round-5 frame stay the
                     handle's own) equal the baseline: rows, particles, map, bookkeeping, pfslam_debug_check_cells
  change             lag 1: the stream changes right behind the enqueueing of frame 5 of 12; pfslam_set_stream books the frames in flight
                     and synchronises the old stream, which has nothing left when the call returns; every frame's row is the baseline's
One JSON line per case goes to stdout: {"case", "ok", "error", "gates"}.  `gates` -- whether the frames' cross-stream edges were gates or
events on the caller's stream -- is the self-test's finding: reported, never required.  Exit status 1 when a case failed; a library error
(PfSlamError: a HIP error, a stream gate that gave up) ends the process at once with status 2 -- nothing more is started on the device."""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import test_gpu_observers as T  # noqa: E402
from stage_shadow import StageShadow  # noqa: E402

bits, FIELDS, FRAMES = T.bits, T.FIELDS, T.FRAMES


def stage_calls(pkg, world, torch, variant):
    s = torch.cuda.Stream()
    n = 192
    shadows = [StageShadow(n, kd_capacity=len(world["tree"]) + (1 << 16), variant=variant, pkg=pkg) for _ in range(2)]
    shadows[0].h.set_stream(s.cuda_stream)
    for sh in shadows:
        sh.set_map(world["tree"])
        sh.set_particles(T.clouds(n, 5)[-1])
    for i, scan in enumerate(world["scans"][:4]):
        for sh in shadows:
            sh.step(6 + i, scan)
        a, b = shadows
        assert a.trace() == b.trace() and (bits(a.pose) == bits(b.pose)).all(), i
    pa, pb = shadows[0].particles(), shadows[1].particles()
    for fld in FIELDS:
        assert (bits(pa[fld]) == bits(pb[fld])).all(), fld
    assert shadows[0].tree().tobytes() == shadows[1].tree().tobytes() and shadows[0].kd_size > len(world["tree"])
    for sh in shadows:
        sh.close()
    del s                          # (alive until here: behind the handles' close)
    return {}


def frames(pkg, world, torch, case):
    streams = []

    def on_stream(h):
        streams.append(torch.cuda.Stream())
        h.set_stream(streams[-1].cuda_stream)
    got = T.run(pkg, world, case, prepare=on_stream)
    mode = got[5]
    assert mode["round5_frame"] == T.CASES[case][2], mode
    T.assert_same(got, T.baseline(pkg, world, case), what="caller's stream, %s" % ("gates" if mode["gates"] else "events"))
    del streams[:]
    return {"gates": bool(mode["gates"])}


def change(pkg, world, torch):
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    idle, modes = [], []

    def setup(h):
        h.set_lag(1)
        h.set_stream(streams[0].cuda_stream)

    def after(h, i):
        if i == 4:
            h.set_stream(streams[1].cuda_stream)
            idle.append(streams[0].query())
    got = T.run(pkg, world, "r5", look=1, prepare=T.hooks(setup=setup, after=after, modes=modes))
    want = T.baseline(pkg, world, "r5", look=1)
    what = "stream changed, %s" % ("gates" if got[5]["gates"] else "events")
    for f, (a, b) in enumerate(zip(got[0], want[0])):
        assert a == b, "%s: frame %d" % (what, f + 1)
    # the gates' self-test runs again in front of frame 6 and the frame ring starts over behind it: the rows' passes publish in other frames
    # than in the baseline from there on, as under per-phase timing -- results, final state and invariants are compared, the counts are not
    T.assert_same(got, want, book=False, what=what)
    assert idle == [True] and modes == [True] * FRAMES, (idle, modes)
    del streams[:]
    return {"gates": bool(got[5]["gates"])}


CASE_LIST = (("stage-0", stage_calls, (0,)), ("stage-3", stage_calls, (3,)), ("frames-r5", frames, ("r5",)), ("frames-r4", frames, ("r4",)),
             ("change", change, ()))


def main():
    import torch
    pkg = importlib.import_module("gpu-icp-slam_amd")
    assert pkg.device_count() > 0 and torch.cuda.is_available()
    world = T.make_world(pkg)
    failed = 0
    for name, fn, args in CASE_LIST:
        rec = {"case": name, "ok": True, "error": None}
        try:
            rec.update(fn(pkg, world, torch, *args))
        except AssertionError as e:
            rec.update(ok=False, error=(str(e) or repr(e))[:2000])
            failed += 1
        except pkg.PfSlamError as e:
            rec.update(ok=False, error="PfSlamError: %s" % e)
            print(json.dumps(rec), flush=True)
            return 2
        print(json.dumps(rec), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
