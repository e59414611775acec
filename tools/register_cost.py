#!/usr/bin/env python3
"""What pfslam_register costs against the only way to iterate the ICP step without it -- set_pose + pfslam_icp once per iteration, each
with its own launches, copies and stream waits -- and pfslam_nearest beside pfslam_traverse.

For 1, 10 and 40 iterations (eps 0: every iteration runs): wall time per call of PfSlam.register() with match 0 and with match 1, and of
the same number of host-driven set_pose() + icp() calls, each series behind a synchronize(); then per 1081 queries (the end points of the
scan at its pose) nearest() and traverse().  Median with 10th and 90th percentile over --calls calls after a warm-up, the series
alternating.  Maps: 4000 points and the benchmark's 100 000 points.  One process; run it under a time limit of its own:

    timeout -k 10 300 python tools/register_cost.py [--calls 50]

The figures of profiles/register.txt are this tool's output."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def series(fn, calls):
    t = np.empty(calls)
    for k in range(calls):
        t0 = time.perf_counter()
        fn()
        t[k] = time.perf_counter() - t0
    return t * 1e3


def q(t):
    return "%8.4f (%.4f .. %.4f)" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--maps", type=int, nargs="+", default=[4000, 100000])
    a = ap.parse_args()
    pkg = importlib.import_module("gpu-icp-slam_amd")
    pose = (0.5, 0.3, 0.1)
    start = np.array([0.6, 0.22, 0.13], np.float32)
    for n_map in a.maps:
        pts, segs = pkg.synth.make_map_points(n_map, seed=1)
        scan = pkg.synth.make_scan(segs, pose, seed=7)
        h = pkg.PfSlam(64, kd_capacity=1 << 18)
        h.set_map(pkg.kd_create(pts))
        h.set_scan(scan)
        print("map of %d points, 1081 beams; ms per call: median (p10 .. p90)" % n_map)
        print("  iterations   register match 0            register match 1            set_pose + icp from the host")
        for iters in (1, 10, 40):
            ref = dict(match=0, select=0, update=0, eps_xy=0.0, eps_theta=0.0, max_iters=iters)
            full = dict(eps_xy=0.0, eps_theta=0.0, max_iters=iters)

            def host_loop():
                p = start
                for _ in range(iters):
                    h.set_pose(p)
                    p, _ = h.icp(start=p)
                return p

            got = h.register(start, **ref)
            assert got["iterations"] == iters and (got["pose"].view(np.int32) == host_loop().view(np.int32)).all(), "the two paths disagree"
            fns = (lambda: h.register(start, **ref), lambda: h.register(start, **full), host_loop)
            for fn in fns:
                for _ in range(3):
                    fn()
            t = [[], [], []]
            for _ in range(5):                              # alternate the three series
                for k, fn in enumerate(fns):
                    h.synchronize()
                    t[k].append(series(fn, max(1, a.calls // 5)))
            t = [np.concatenate(x) for x in t]
            print("  %10d   %s   %s   %s" % (iters, q(t[0]), q(t[1]), q(t[2])), flush=True)
        ang = np.deg2rad(-135.0 + 0.25 * np.arange(1081)) + pose[2]
        xyz = np.zeros((1081, 3), np.float32)
        xyz[:, 0], xyz[:, 1] = pose[0] + scan * np.cos(ang), pose[1] + scan * np.sin(ang)
        fns = (lambda: h.nearest(xyz), lambda: h.traverse(xyz))
        for fn in fns:
            for _ in range(3):
                fn()
        t = [[], []]
        for _ in range(5):
            for k, fn in enumerate(fns):
                h.synchronize()
                t[k].append(series(fn, max(1, a.calls // 5)))
        t = [np.concatenate(x) for x in t]
        same = int((h.nearest(xyz)[0] == h.traverse(xyz)).sum())
        print("  per 1081 queries: nearest %s   traverse %s   (same node for %d of 1081)" % (q(t[0]), q(t[1]), same), flush=True)
        h.close()


if __name__ == "__main__":
    main()
