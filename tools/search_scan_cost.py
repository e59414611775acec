#!/usr/bin/env python3
"""What pfslam_search_scan costs: HIP events on the handle's stream around whole calls -- the two scans' uploads, the launches, the result
copy and the wait included -- after a warm-up call, and beside them, in the same process, pfslam_search's default call on a 4000-point
map (the two fields differ: context, not a ratio).

    default   the default window (41 x 41 x 33, max_dist 0.2: R = 10) on a handle WITHOUT a map, 1081 beams: the reference scan cast from
              (0.5, 0.3, 0.1), the searched one from (0.58, 0.24, 0.125), the centre (0.6, 0.22, 0.13); without and with the score volume
    search    pfslam_search's default call around the same centre on the 4000-point map the scans were cast on
    worst     max_dist 1.59999 (qcap 65535, R = 66) on a handle of 4096 beams: the 1081-beam scans repeated to 4096 ranges, and every
              range 0.1 m (4096 points whose neighbourhoods cover the same cells: the most contended words)

The kernels one by one, the field builder (k_scan_fill + k_scan_splat) among them, come from a kernel trace of --loop K calls:

    rocprofv3 --kernel-trace --stats -d DIR -o search_scan -- python tools/search_scan_cost.py --loop 20 [--worst]

Median with 10th and 90th percentile of --calls calls.  One process; run it under a time limit of its own:

    timeout -k 10 600 python tools/search_scan_cost.py

The figures of profiles/search_scan.txt are this tool's output."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_POSE, POSE, CENTRE = (0.5, 0.3, 0.1), (0.58, 0.24, 0.125), np.array([0.6, 0.22, 0.13], np.float32)
WORST = dict(max_dist=1.59999)


def q(t):
    t = np.asarray(t)
    return "%9.3f (%.3f .. %.3f)" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--loop", type=int, default=0, help="only this many calls, for a kernel trace (see above)")
    ap.add_argument("--worst", action="store_true", help="with --loop: the worst case (4096 beams, qcap 65535) instead of the default call")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("gpu-icp-slam_amd")
    pts, segs = pkg.synth.make_map_points(4000, seed=1)
    ref, scan = pkg.synth.make_scan(segs, REF_POSE, seed=7), pkg.synth.make_scan(segs, POSE, seed=8)
    if a.loop:
        nb = 4096 if a.worst else 1081
        h = pkg.PfSlam(64, n_beams=nb, kd_capacity=1 << 16)
        opts = WORST if a.worst else {}
        for _ in range(a.loop):
            r = h.search_scan(np.resize(ref, nb), REF_POSE, np.resize(scan, nb), CENTRE, **opts)
        print("%d calls of %d beams, %d points, qcap %d, %d candidates" % (a.loop, nb, r["points"], r["qcap"], r["candidates"]))
        h.close()
        return
    import torch
    stream = torch.cuda.Stream()

    def timed(call, calls=a.calls):
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

    print("ms: median (p10 .. p90) of %d calls; HIP events around whole calls" % a.calls)
    h = pkg.PfSlam(64, kd_capacity=1 << 16)               # no map
    h.set_stream(stream.cuda_stream)
    t, r = timed(lambda: h.search_scan(ref, REF_POSE, scan, CENTRE))
    print("pfslam_search_scan, no map, 1081 beams (%d points, %d searched beams in range), default window of %d candidates, qcap %d (R = 10)"
          % (r["points"], r["beams"], r["candidates"], r["qcap"]))
    print("  default call                                                 %s ms" % q(t))
    t, _ = timed(lambda: h.search_scan(ref, REF_POSE, scan, CENTRE, scores=True))
    print("  default call with the score volume copied back               %s ms" % q(t))
    h.set_scan(scan)
    t, _ = timed(lambda: h.search_scan(ref, REF_POSE, None, CENTRE))
    print("  default call, the handle's scan searched (one upload less)   %s ms" % q(t))
    t, r = timed(lambda: h.search_scan(ref, REF_POSE, scan, CENTRE, max_dist=0.5))
    print("  max_dist 0.5 (qcap %d, R = 22)                              %s ms" % (r["qcap"], q(t)), flush=True)
    h.close()
    m = pkg.PfSlam(64, kd_capacity=1 << 16)
    m.set_stream(stream.cuda_stream)
    m.set_map(pkg.kd_create(pts))
    m.set_scan(scan)
    t, r = timed(lambda: m.search(CENTRE))
    print("pfslam_search on the 4000-point map, the same scan and centre, default window (%d beams in range)" % r["beams"])
    print("  default call                                                 %s ms" % q(t))
    t, _ = timed(lambda: m.search_scan(ref, REF_POSE, None, CENTRE))
    print("  pfslam_search_scan's default call on that handle             %s ms" % q(t), flush=True)
    m.close()
    w = pkg.PfSlam(64, n_beams=4096, kd_capacity=1 << 16)
    w.set_stream(stream.cuda_stream)
    ref4, scan4 = np.resize(ref, 4096), np.resize(scan, 4096)
    t, r = timed(lambda: w.search_scan(ref4, REF_POSE, scan4, CENTRE, **WORST))
    print("worst case: 4096 beams, max_dist 1.59999 (qcap %d, R = 66), default window" % r["qcap"])
    print("  the scans repeated to 4096 ranges (%d points)               %s ms" % (r["points"], q(t)))
    near = np.full(4096, 0.1, np.float32)
    t, r = timed(lambda: w.search_scan(near, REF_POSE, near, CENTRE, **WORST))
    print("  every range 0.1 m (%d points around one cell)               %s ms" % (r["points"], q(t)))
    t, r = timed(lambda: w.search_scan(ref4, REF_POSE, scan4, CENTRE))
    print("  for comparison 4096 beams at the default max_dist (%d points) %s ms" % (r["points"], q(t)), flush=True)
    w.close()


if __name__ == "__main__":
    main()
