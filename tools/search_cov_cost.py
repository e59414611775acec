#!/usr/bin/env python3
"""What pfslam_search_cov costs: HIP events on the handle's stream around whole calls -- the launches, the one result copy and the wait
included -- after a warm-up call, on the benchmark's 100 000-point map and on the 4000-point map of the tests, 1081 beams, the scan cast
from (0.5, 0.3, 0.1) and searched around (0.6, 0.22, 0.13) as tools/search_cost.py does, at three windows:

    default   41 x 41 x 33 = 55 473 candidates (14 tiles of 4096)
    filled    129 x 129 x 33 = 549 153 candidates (135 tiles): the window that fills the device in profiles/search.txt
    cap       713 x 713 x 33 = 16 776 177 candidates (4096 tiles), just under the cap of 2^24

and beside each, in the same process, pfslam_search with scores = NULL -- the parent's code path: it writes no volume -- so that the
difference is the volume's stores plus the reduction.  pfslam_search_scan_cov's default call without a map closes the list.

The three reduction launches alone (k_cov_moments, k_cov_centred, k_cov_final; k_cov_small up to one tile) come from a kernel trace of
--loop K calls of one window:

    rocprofv3 --kernel-trace --stats -d DIR -o search_cov -- python tools/search_cov_cost.py --maps 100000 --window cap --loop 10

Median with 10th and 90th percentile of --calls calls (5 at the cap).  One process; run it under a time limit of its own:

    timeout -k 10 600 python tools/search_cov_cost.py

The figures of profiles/search_cov.txt are this tool's output."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE, CENTRE = (0.5, 0.3, 0.1), np.array([0.6, 0.22, 0.13], np.float32)
REF_POSE, SCAN_POSE = (0.5, 0.3, 0.1), (0.58, 0.24, 0.125)
WINDOWS = (("default", dict()), ("filled", dict(half_x=64, half_y=64)), ("cap", dict(half_x=356, half_y=356)))


def q(t):
    t = np.asarray(t)
    return "%9.3f (%.3f .. %.3f)" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, nargs="+", default=[100000, 4000])
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--window", choices=[w for w, _ in WINDOWS], default="default", help="with --loop: the window of the traced calls")
    ap.add_argument("--loop", type=int, default=0, help="only this many pfslam_search_cov calls per map, for a kernel trace (see above)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("gpu-icp-slam_amd")

    def handle(n_map):
        pts, segs = pkg.synth.make_map_points(n_map, seed=1)
        h = pkg.PfSlam(64, kd_capacity=1 << 18)
        h.set_map(pkg.kd_create(pts))
        h.set_scan(pkg.synth.make_scan(segs, POSE, seed=7))
        return h

    if a.loop:
        opts = dict(WINDOWS)[a.window]
        for n_map in a.maps:
            h = handle(n_map)
            for _ in range(a.loop):
                r = h.search_cov(CENTRE, **opts)
            print("map of %d points: %d calls of %d candidates (%d tiles), Neff %g" % (n_map, a.loop, r["candidates"], (r["candidates"] + 4095) // 4096, r["neff"]))
            h.close()
        return
    import torch
    stream = torch.cuda.Stream()

    def timed(call, calls):
        call()                                           # warm-up: buffers grown, code loaded
        t = []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            r = call()
            e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        return np.array(t), r

    print("ms: median (p10 .. p90) of %d calls (5 at the cap); HIP events around whole calls; sigma 0.2" % a.calls)
    for n_map in a.maps:
        h = handle(n_map)
        h.set_stream(stream.cuda_stream)
        print("map of %d points, 1081 beams, 33 headings of 0.0125 rad, max_dist 0.2" % n_map)
        for name, opts in WINDOWS:
            calls = 5 if name == "cap" else a.calls
            ts, r = timed(lambda: h.search(CENTRE, **opts), calls)
            tc, c = timed(lambda: h.search_cov(CENTRE, **opts), calls)
            nx, na = 2 * opts.get("half_x", 20) + 1, 33
            print("  %-7s %d x %d x %d = %d candidates, %d tiles: Neff %.4g, border share %.3g, sd %.3g m / %.3g m / %.3g rad"
                  % (name, nx, nx, na, c["candidates"], (c["candidates"] + 4095) // 4096, c["neff"], c["edge"], c["raw"][3] ** 0.5, c["raw"][6] ** 0.5, c["raw"][8] ** 0.5))
            print("    pfslam_search, scores = NULL (no volume is written)        %s ms" % q(ts))
            print("    pfslam_search_cov, scores = NULL                           %s ms   (+ %.3f ms)" % (q(tc), np.median(tc) - np.median(ts)), flush=True)
            assert r["index"] == c["index"]
        h.close()
    pts, segs = pkg.synth.make_map_points(4000, seed=1)
    ref, scan = pkg.synth.make_scan(segs, REF_POSE, seed=7), pkg.synth.make_scan(segs, SCAN_POSE, seed=8)
    h = pkg.PfSlam(64, kd_capacity=1 << 16)              # no map
    h.set_stream(stream.cuda_stream)
    ts, _ = timed(lambda: h.search_scan(ref, REF_POSE, scan, CENTRE), a.calls)
    tc, c = timed(lambda: h.search_scan_cov(ref, REF_POSE, scan, CENTRE), a.calls)
    print("scan to scan, no map, 1081 beams, default window: Neff %.4g, border share %.3g" % (c["neff"], c["edge"]))
    print("    pfslam_search_scan, scores = NULL                          %s ms" % q(ts))
    print("    pfslam_search_scan_cov, scores = NULL                      %s ms   (+ %.3f ms)" % (q(tc), np.median(tc) - np.median(ts)), flush=True)
    h.close()


if __name__ == "__main__":
    main()
