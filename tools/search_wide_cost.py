#!/usr/bin/env python3
"""What pfslam_search_wide costs next to pfslam_search: HIP events on the handle's stream around whole calls, after a warm-up call, on the
benchmark's 100 000-point map and on a 4000-point one, with 1081 beams (the scan cast from (10, -8, 0.3)).

    whole map   +-20 m and a full turn around (0, 0, 0): 1601 x 1601 x 503 = 1 289 290 103 candidates in one pfslam_search_wide call,
                against the only exact answer the library had before: 503 pfslam_search calls, one per heading (half_theta = 0,
                the heading formed in float32 as the specification forms theta_a); the smallest (S, k) of the 503 must be the call's
    at the cap  713 x 713 x 33 (one pfslam_search call) and 725 x 725 x 33, just above (33 per-heading calls)
    default     41 x 41 x 33: the pyramid is overhead there

Median with 10th and 90th percentile of --calls calls; the 503-call baseline is run --baseline-runs times, each run one figure.
The kernels one by one come from a kernel trace of --loop K whole-map calls on ONE map:

    rocprofv3 --kernel-trace --stats -d DIR -o wide -- python tools/search_wide_cost.py --maps 4000 --loop 5

One process; run it under a time limit of its own:

    timeout -k 10 900 python tools/search_wide_cost.py

The figures of profiles/search_wide.txt are this tool's output."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
POSE = (10.0, -8.0, 0.3)
WHOLE = dict(half_x=800, half_y=800, half_theta=251)


def q(t):
    t = np.asarray(t)
    return "%9.3f (%.3f .. %.3f)" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, nargs="+", default=[4000, 100000])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--baseline-runs", type=int, default=2)
    ap.add_argument("--loop", type=int, default=0, help="only this many whole-map calls per map, for a kernel trace (see above)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    pkg = importlib.import_module("gpu-icp-slam_amd")
    stream = torch.cuda.Stream()
    zero = np.zeros(3, np.float32)
    near = np.array([10.1, -7.92, 0.27], np.float32)          # 0.10 m / 0.03 rad off the pose
    for n_map in a.maps:
        pts, segs = pkg.synth.make_map_points(n_map, seed=1)
        scan = pkg.synth.make_scan(segs, POSE, seed=7)
        h = pkg.PfSlam(64, kd_capacity=1 << 18)
        h.set_stream(stream.cuda_stream)
        h.set_map(pkg.kd_create(pts))
        h.set_scan(scan)
        if a.loop:
            for _ in range(a.loop):
                r = h.search_wide(zero, **WHOLE)
            print("map of %d points: %d whole-map calls, stats %s" % (n_map, a.loop, r["stats"].tolist()))
            h.close()
            continue

        def timed(fn, calls=a.calls):
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

        def per_heading(centre, ht, **opts):
            """The window's winner from one pfslam_search call per heading: (S, k, the winning call's result)."""
            row, best = (2 * opts["half_x"] + 1) * (2 * opts["half_y"] + 1), None
            for i in range(2 * ht + 1):
                theta = F(F(centre[2]) + F(F(i - ht) * F(0.0125)))
                r = h.search(np.array([centre[0], centre[1], theta], np.float32), half_theta=0, **opts)
                if r["status"] == 0 and (best is None or (r["score"], i * row + r["index"]) < best[:2]):
                    best = (r["score"], i * row + r["index"], r)
            return best

        print("map of %d points, 1081 beams, max_dist 0.2, stride 1, headings of 0.0125 rad; ms: median (p10 .. p90) of %d calls" % (n_map, a.calls))
        t, r = timed(lambda: h.search_wide(zero, **WHOLE))
        st = r["stats"]
        print("  whole map, 1601 x 1601 x 503 = %d candidates, one pfslam_search_wide call        %s ms" % (st[1], q(t)))
        print("    winner %d at %s, score %d; top level %d, %d nodes bounded above level 0, %d candidates scored (1 in %.0f), %d batches, box of %d cells"
              % (st[0], r["pose"].tolist(), r["score"], st[4], st[2], st[3], st[1] / max(int(st[3]), 1), st[5], st[6]), flush=True)
        tb, best = timed(lambda: per_heading(zero, 251, half_x=800, half_y=800), calls=a.baseline_runs)
        assert best[:2] == (r["score"], int(st[0])), "the 503 per-heading calls pick %r, the wide call %r" % (best[:2], (r["score"], int(st[0])))
        print("  the same winner from 503 pfslam_search calls of 1601 x 1601 x 1                    %s ms  (%d runs: %s)"
              % (q(tb), len(tb), ", ".join("%.1f" % v for v in tb)))
        print("    ratio of the medians: %.1f" % (np.median(tb) / np.median(t)), flush=True)
        for half, name in ((356, "713 x 713 x 33, just under pfslam_search's cap"), (362, "725 x 725 x 33, just above it")):
            opts = dict(half_x=half, half_y=half)
            t, r = timed(lambda: h.search_wide(near, half_theta=16, **opts))
            st = r["stats"]
            print("  %s: pfslam_search_wide   %s ms   (%d of %d candidates scored, %d nodes bounded, %d batches)" % (name, q(t), st[3], st[1], st[2], st[5]))
            if half == 356:
                t1, r1 = timed(lambda: h.search(near, half_theta=16, **opts))
                assert r1["index"] == st[0] and r1["score"] == r["score"]
                print("      one pfslam_search call                                    %s ms" % q(t1))
            t2, best = timed(lambda: per_heading(near, 16, **opts), calls=3)
            assert best[:2] == (r["score"], int(st[0]))
            print("      33 pfslam_search calls, one per heading                   %s ms" % q(t2), flush=True)
        t, r = timed(lambda: h.search_wide(near))
        t1, r1 = timed(lambda: h.search(near))
        assert r1["index"] == r["stats"][0]
        print("  default window, 41 x 41 x 33: pfslam_search_wide %s ms, pfslam_search %s ms   (%d of %d candidates scored)"
              % (q(t), q(t1), r["stats"][3], r["stats"][1]), flush=True)
        h.close()


if __name__ == "__main__":
    main()
