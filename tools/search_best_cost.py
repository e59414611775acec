#!/usr/bin/env python3
"""What pfslam_search_best costs next to pfslam_search_wide and next to the only exact alternative: HIP events on the handle's stream around
whole calls, after a warm-up call, on the benchmark's 100 000-point map and on a 4000-point one, with 1081 beams (the scan cast from
(10, -8, 0.3)).

    whole map   +-20 m and a full turn around (0, 0, 0): 1601 x 1601 x 503 = 1 289 290 103 candidates, 201 x 201 x 63 cells at the default
                pfslam_best_opts, beside pfslam_search_wide on the same inputs; count = 1, 8 and 64
    alternative 503 pfslam_search calls, one per heading, each with its volume copied back, the cells reduced on the host (numpy); its
                eight rows must be the call's.  Run --baseline-runs times (wall clock: the host's work is part of it)
    at the cap  713 x 713 x 33 and 725 x 725 x 33, and the default window 41 x 41 x 33, beside pfslam_search_wide

Median with 10th and 90th percentile of --calls calls.  The kernels one by one come from a kernel trace of --loop K whole-map calls on ONE
map, in a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -o best -- python tools/search_best_cost.py --maps 4000 --loop 5

One process; run it under a time limit of its own:

    timeout -k 10 900 python tools/search_best_cost.py

The figures of profiles/search_best.txt are this tool's output (--out)."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
POSE = (10.0, -8.0, 0.3)
WHOLE = dict(half_x=800, half_y=800, half_theta=251)
NONE = np.int64(2**63 - 1)


def q(t):
    t = np.asarray(t)
    return "%9.3f (%.3f .. %.3f)" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, nargs="+", default=[4000, 100000])
    ap.add_argument("--calls", type=int, default=11)
    ap.add_argument("--baseline-runs", type=int, default=1)
    ap.add_argument("--loop", type=int, default=0, help="only this many whole-map calls per map, for a kernel trace (see above)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_best.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    pkg = importlib.import_module("gpu-icp-slam_amd")
    stream = torch.cuda.Stream()
    zero = np.zeros(3, np.float32)
    near = np.array([10.1, -7.92, 0.27], np.float32)          # 0.10 m / 0.03 rad off the pose
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for n_map in a.maps:
        pts, segs = pkg.synth.make_map_points(n_map, seed=1)
        scan = pkg.synth.make_scan(segs, POSE, seed=7)
        h = pkg.PfSlam(64, kd_capacity=1 << 18)
        h.set_stream(stream.cuda_stream)
        h.set_map(pkg.kd_create(pts))
        h.set_scan(scan)
        if a.loop:
            for _ in range(a.loop):
                r = h.search_best(zero, **WHOLE)
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

        def alternative(centre, ht, count, ls, g, **opts):
            """The rows from one pfslam_search call per heading, every volume copied back, the cells reduced here: keys ascending."""
            nx, ny = 2 * opts["half_x"] + 1, 2 * opts["half_y"] + 1
            tx, ty, n = ((nx - 1) >> ls) + 1, ((ny - 1) >> ls) + 1, 1 << ls
            T = np.full(((2 * ht) // g + 1, ty, tx), NONE, np.int64)
            k = np.arange(nx * ny, dtype=np.int64).reshape(ny, nx)
            pad = np.full((ty * n, tx * n), NONE, np.int64)
            for i in range(2 * ht + 1):
                theta = F(F(centre[2]) + F(F(i - ht) * F(0.0125)))
                r = h.search(np.array([centre[0], centre[1], theta], np.float32), scores=True, half_theta=0, **opts)
                if r["status"] != 0:
                    continue
                pad[:ny, :nx] = (r["scores"][0].astype(np.int64) << 32) | (k + i * nx * ny)
                np.minimum(T[i // g], pad.reshape(ty, n, tx, n).min(axis=(1, 3)), out=T[i // g])
            return np.sort(T.ravel())[:count]

        say("map of %d points, 1081 beams, max_dist 0.2, stride 1, headings of 0.0125 rad; ms: median (p10 .. p90) of %d calls" % (n_map, a.calls))
        tw, w = timed(lambda: h.search_wide(zero, **WHOLE))
        sw = w["stats"]
        say("  whole map, 1601 x 1601 x 503 = %d candidates: pfslam_search_wide                       %s ms" % (sw[1], q(tw)))
        say("    winner %d, score %d; %d nodes bounded above level 0, %d candidates scored, %d batches, box of %d cells" % (sw[0], w["score"], sw[2], sw[3], sw[5], sw[6]))
        for count in (8, 1, 64):
            t, r = timed(lambda: h.search_best(zero, count=count, **WHOLE))
            st = r["stats"]
            assert st[0] == sw[0] and r["score"][0] == w["score"] and r["found"] == count
            say("  pfslam_search_best, count = %2d, tiles of 8 x 8, groups of 8 (%d cells)                  %s ms   %.2f x pfslam_search_wide"
                % (count, st[7], q(t), np.median(t) / np.median(tw)))
            say("    rows %s, scores %s" % (r["index"].tolist()[:8], r["score"].tolist()[:8]))
            say("    %d nodes bounded above level 0, %d candidates scored, %d batches" % (st[2], st[3], st[5]))
            if count == 8:
                t8, r8 = t, r
        tb = []
        for _ in range(a.baseline_runs):
            stream.synchronize()
            t0 = time.perf_counter()
            keys = alternative(zero, 251, 8, 3, 8, half_x=800, half_y=800)
            tb.append((time.perf_counter() - t0) * 1e3)
            assert (keys & 0xffffffff).tolist() == r8["index"].tolist() and (keys >> 32).tolist() == r8["score"].tolist(), \
                "the 503 volumes give %r, the call %r" % ((keys & 0xffffffff).tolist(), r8["index"].tolist())
        say("  the same eight rows from 503 pfslam_search calls, volumes copied back, cells reduced on the host   %s ms wall clock"
            % ", ".join("%.0f" % v for v in tb))
        say("    ratio to the count = 8 call's median: %.0f (the condition: more than 10)" % (np.median(tb) / np.median(t8)))
        for opts, name in ((dict(half_x=356, half_y=356, half_theta=16), "713 x 713 x 33, just under pfslam_search's cap"),
                           (dict(half_x=362, half_y=362, half_theta=16), "725 x 725 x 33, just above it"), (dict(), "the default window, 41 x 41 x 33")):
            tw, w = timed(lambda: h.search_wide(near, **opts))
            t, r = timed(lambda: h.search_best(near, **opts))
            st = r["stats"]
            assert st[0] == w["stats"][0]
            say("  %s: pfslam_search_best %s ms, pfslam_search_wide %s ms" % (name, q(t), q(tw)))
            say("    %d rows of %d cells; %d of %d candidates scored, %d nodes bounded, %d batches (pfslam_search_wide: %d, %d, %d)"
                % (r["found"], st[7], st[3], st[1], st[2], st[5], w["stats"][3], w["stats"][2], w["stats"][5]))
        h.close()
    if not a.loop:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
