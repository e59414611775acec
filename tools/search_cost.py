#!/usr/bin/env python3
"""What pfslam_search costs: HIP events on the handle's stream around whole calls, after a warm-up call, on the benchmark's 100 000-point
map (and a 4000-point one) with 1081 beams.

The field and the end points of a call depend on its headings and on half * stride, the cells the box is grown by -- not on how many
candidates share them.  So a window of halves (H, H) at stride s and one of halves (1, 1) at stride H * s build the SAME field from the
same end points, and the difference of the two calls' times is the scoring of (2H + 1)^2 - 9 candidates per heading:

    field     time of the (1, 1) call: end points + field + 9 candidates per heading + result, per 10^6 cells of its box
              (the box is recomputed here in double precision: a cell more or less per side)
    scoring   (time of the (H, H) call - time of the (1, 1) call) per 10^6 candidates, at stride 1 and stride 2
    default   one whole default call (41 x 41 x 33), without and with the score volume copied back
    cap       one call of 713 x 713 x 33 = 16 776 177 candidates, just under the cap of 2^24

The kernels one by one, the field kernel among them, come from a kernel trace of --loop K default calls on ONE map, whose box is printed:

    rocprofv3 --kernel-trace --stats -d DIR -o search -- python tools/search_cost.py --maps 100000 --loop 20

Median with 10th and 90th percentile of --calls calls.  One process; run it under a time limit of its own:

    timeout -k 10 600 python tools/search_cost.py

The figures of profiles/search.txt are this tool's output."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def q(t):
    t = np.asarray(t)
    return "%9.3f (%.3f .. %.3f)" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90))


def box_cells(scan, centre, thetas, grow, res=0.025):
    """Cells of the field a call builds: the bounding box of the in-range end points of all headings, grown by `grow` cells."""
    ang = np.deg2rad(-135.0 + 0.25 * np.arange(len(scan)))
    lo, hi = np.array([np.inf, np.inf]), np.array([-np.inf, -np.inf])
    for th in thetas:
        w = np.stack([scan * np.cos(ang + th), scan * np.sin(ang + th)], 1)
        w = w[(np.abs(w) < 20.0).all(axis=1)]
        if len(w):
            c = np.rint((w + np.array(centre[:2])) / res)
            lo, hi = np.minimum(lo, c.min(axis=0)), np.maximum(hi, c.max(axis=0))
    side = hi - lo + 1 + 2 * grow
    return int(side[0]), int(side[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, nargs="+", default=[100000, 4000])
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--loop", type=int, default=0, help="only this many default calls per map, for a kernel trace (see above)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.loop:
        pkg = importlib.import_module("gpu-icp-slam_amd")
        for n_map in a.maps:
            pts, segs = pkg.synth.make_map_points(n_map, seed=1)
            scan = pkg.synth.make_scan(segs, (0.5, 0.3, 0.1), seed=7)
            h = pkg.PfSlam(64, kd_capacity=1 << 18)
            h.set_map(pkg.kd_create(pts))
            h.set_scan(scan)
            c = np.array([0.6, 0.22, 0.13], np.float32)
            W, Hc = box_cells(scan, c, c[2] + (np.arange(33) - 16) * 0.0125, 20)
            for _ in range(a.loop):
                h.search(c)
            print("map of %d points: %d default calls, box %d x %d = %.3f M cells" % (n_map, a.loop, W, Hc, W * Hc / 1e6))
            h.close()
        return
    import torch
    pkg = importlib.import_module("gpu-icp-slam_amd")
    stream = torch.cuda.Stream()
    pose = (0.5, 0.3, 0.1)
    centre = np.array([0.6, 0.22, 0.13], np.float32)
    for n_map in a.maps:
        pts, segs = pkg.synth.make_map_points(n_map, seed=1)
        scan = pkg.synth.make_scan(segs, pose, seed=7)
        h = pkg.PfSlam(64, kd_capacity=1 << 18)
        h.set_stream(stream.cuda_stream)
        h.set_map(pkg.kd_create(pts))
        h.set_scan(scan)

        def timed(scores=False, calls=a.calls, **opts):
            h.search(centre, scores=scores, **opts)          # warm-up: buffers grown, code loaded
            t = []
            for _ in range(calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                r = h.search(centre, scores=scores, **opts)
                e1.record(stream)
                e1.synchronize()
                t.append(e0.elapsed_time(e1))
            return np.array(t), r

        print("map of %d points, 1081 beams (%d in range), 33 headings of 0.0125 rad, max_dist 0.2; ms: median (p10 .. p90) of %d calls"
              % (n_map, timed(calls=1, half_x=0, half_y=0, half_theta=0)[1]["beams"], a.calls))
        thetas = centre[2] + (np.arange(33) - 16) * 0.0125
        for stride, H in ((1, 64), (2, 32)):
            grow = H * stride
            W, Hc = box_cells(scan, centre, thetas, grow)
            tb, _ = timed(half_x=1, half_y=1, stride=grow)
            ta, r = timed(half_x=H, half_y=H, stride=stride)
            cand = r["candidates"] - 9 * 33
            d = np.median(ta) - np.median(tb)
            print("  stride %d: box %d x %d = %.3f M cells" % (stride, W, Hc, W * Hc / 1e6))
            print("    3 x 3 x 33 at stride %2d (end points + field + result)   %s ms   = %.3f ms per 10^6 cells" % (grow, q(tb), np.median(tb) / (W * Hc / 1e6)))
            print("    %d x %d x 33 at stride %d                              %s ms" % (2 * H + 1, 2 * H + 1, stride, q(ta)))
            print("    scoring: %.3f ms for %d candidates = %.3f ms per 10^6 candidates = %.0f candidates per ms" % (d, cand, d / (cand / 1e6), cand / d), flush=True)
        W, Hc = box_cells(scan, centre, thetas, 20)
        t, r = timed()
        print("  default call, 41 x 41 x 33 = %d candidates, box %d x %d       %s ms" % (r["candidates"], W, Hc, q(t)))
        t, _ = timed(scores=True)
        print("  default call with the score volume copied back               %s ms" % q(t))
        t, r = timed(calls=5, half_x=356, half_y=356)
        print("  713 x 713 x 33 = %d candidates (the cap is 2^24)         %s ms" % (r["candidates"], q(t)), flush=True)
        h.close()


if __name__ == "__main__":
    main()
