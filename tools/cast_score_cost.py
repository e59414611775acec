#!/usr/bin/env python3
"""What pfslam_cast_score costs next to what it replaces, pfslam_cast with the ranges copied back and compared on the host: HIP events on
the handle's stream around whole calls (upload of the poses, every kernel, the waits, the copy back; the host's comparison is inside the
pair of events of the alternative, as wall time on the stream's clock), after a warm-up call, on the benchmark's 100 000-point map and on a
4000-point one, with 1081 beams (the noise-free scan from (0.5, 0.3, 0.1)); m = 1, 64, 4096 and a list of 15 000 poses, and the handle's own
particles (4096 of them) against the same poses as a list.

Median with min .. max of --calls calls.  The kernels one by one come from a kernel trace of --loop K calls of either entry point per size on
ONE map, in a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -o cast_score -- python tools/cast_score_cost.py --maps 4000 --loop 5

One process; run it under a time limit of its own:

    timeout -k 10 600 python tools/cast_score_cost.py

Sections 3 and 4 of profiles/cast_score.txt are this tool's output."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUE = (0.5, 0.3, 0.1)
SIZES = (1, 64, 4096, 15000)


def q(t):
    t = np.asarray(t)
    return "%8.3f [%.3f .. %.3f]" % (np.median(t), t.min(), t.max())


def poses_of(m, seed=3):
    rng = np.random.RandomState(seed)
    p = np.concatenate([rng.uniform(-15, 15, (m, 2)), rng.uniform(-3.2, 3.2, (m, 1))], axis=1).astype(np.float32)
    p[0] = TRUE
    return p


def host_rows(ranges, hit, scan, tol=np.float32(0.1), clip_q=160, z_min=np.float32(0.1), z_max=np.float32(20.0)):
    """The rows from pfslam_cast's ranges, on the host (numpy, float32): what a caller had to do before pfslam_cast_score."""
    u = tol * np.float32(0.0625)
    z = scan[None, :]
    valid = np.broadcast_to((z >= z_min) & (z <= z_max), ranges.shape)
    d = z - ranges
    a = np.abs(d)
    qq = np.minimum(np.rint(a / u), np.float32(clip_q)).astype(np.int32)
    vh = valid & hit
    agree, through = vh & (a <= tol), vh & (d > tol)
    rows = np.zeros((len(ranges), 8), np.int32)
    rows[:, 0] = valid.sum(axis=1)
    rows[:, 1], rows[:, 2] = agree.sum(axis=1), through.sum(axis=1)
    rows[:, 3] = vh.sum(axis=1) - rows[:, 1] - rows[:, 2]
    rows[:, 4] = rows[:, 0] - vh.sum(axis=1)
    rows[:, 5] = np.where(vh, qq, 0).sum(axis=1)
    rows[:, 6] = np.where(agree, qq * qq, 0).sum(axis=1)
    rows[:, 7] = rows[:, 5] + clip_q * rows[:, 4]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, nargs="+", default=[4000, 100000])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--loop", type=int, default=0, help="only this many calls of pfslam_cast and of pfslam_cast_score per size and map, for a kernel trace")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    pkg = importlib.import_module("gpu-icp-slam_amd")
    stream = torch.cuda.Stream()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for n_map in a.maps:
        pts, segs = pkg.synth.make_map_points(n_map, seed=1)
        scan = pkg.synth.make_scan(segs, TRUE, noise=0).astype(np.float32)
        h = pkg.PfSlam(4096, kd_capacity=1 << 18)
        h.set_stream(stream.cuda_stream)
        h.set_map(pkg.kd_create(pts))
        h.set_scan(scan)
        cloud = np.zeros(4096, pkg.PARTICLE_DTYPE)
        cloud["x"], cloud["y"], cloud["theta"] = poses_of(4096).T
        cloud["w"] = np.float32(1.0 / 4096)
        h.set_particles(cloud)
        if a.loop:
            for m in SIZES[:3]:
                for _ in range(a.loop):
                    r = h.cast(poses_of(m))
                    s = h.cast_score(poses_of(m))
                print("map of %d points, m = %d: %d calls each, %d hits, best %d" % (n_map, m, a.loop, r["stats"][1], s["best"]))
            h.close()
            continue

        def timed(fn, calls):
            fn()                                             # warm-up: buffers grown, code loaded
            t = []
            for _ in range(calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                r = fn()
                e1.record(stream)
                e1.synchronize()
                t.append(e0.elapsed_time(e1))
            return np.array(t), r

        def alternative(poses):
            r = h.cast(poses, no_hit=float("nan"))           # (a miss is a NaN: no range can be mistaken for one)
            with np.errstate(all="ignore"):
                return host_rows(r["ranges"], ~np.isnan(r["ranges"]), scan), r

        say("map of %d points, 1081 beams, default options; ms: median [min .. max]" % n_map)
        say("  m        calls   pfslam_cast_score              pfslam_cast alone              pfslam_cast + host comparison   score / cast   below by more than both spreads")
        for m in SIZES:
            poses = poses_of(m)
            calls = a.calls if m <= 64 else max(8, a.calls // 2)
            ts, s = timed(lambda: h.cast_score(poses), calls)
            tc, c = timed(lambda: h.cast(poses), calls)
            ta, (rows, _) = timed(lambda: alternative(poses), calls)
            assert (rows == s["rows"]).all(), "the host comparison and the call disagree"
            assert list(c["stats"]) == list(s["stats"])
            gap = np.median(tc) - np.median(ts)
            spreads = (ts.max() - ts.min()) + (tc.max() - tc.min())
            say("  %-8d %-7d %s   %s   %s   %.3f          %s (gap %.3f, spreads %.3f)"
                % (m, calls, q(ts), q(tc), q(ta), np.median(ts) / np.median(tc), "yes" if gap > spreads else "NO", gap, spreads))
            say("           best %d, row of the best %s, %d of %d rays hit" % (s["best"], s["rows"][max(s["best"], 0)].tolist(), s["stats"][1], s["stats"][0]))
        tp, p = timed(lambda: h.cast_score(particles=True), max(8, a.calls // 2))
        tl, l = timed(lambda: h.cast_score(poses_of(4096)), max(8, a.calls // 2))
        assert (p["rows"] == l["rows"]).all()
        say("  the handle's 4096 particles, read on the device: %s; the same poses as a list: %s" % (q(tp), q(tl)))
        tk, k = timed(lambda: h.cast_score(poses_of(4096), classes=True), max(8, a.calls // 2))
        say("  m = 4096 with the class bytes (4.4 MB back): %s" % q(tk))
        h.close()
    if not a.loop and a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
