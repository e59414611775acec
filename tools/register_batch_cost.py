#!/usr/bin/env python3
"""What pfslam_register_batch costs against the only way to register from m starts without it: m successive pfslam_register calls.

For m in --rows (default 1, 16, 256, 1024) on a 4000-point and on the benchmark's 100 000-point map, 1081 beams, the default options with
eps 0 and --iters iterations (default 10: every iteration of every row runs): wall time per PfSlam.register_batch() call, and per m
PfSlam.register() calls from the same starts, each behind a synchronize().  Median with 10th and 90th percentile; the two series
alternate.  A sequential series of m calls is long, so it gets fewer samples than the batch: --seq-budget seconds per (map, m) at the
most, three samples at the least.  Then --full rows (default 4096, the cap of the entry point) with the default 40 iterations, eps 0:
the time behind the cap.

    --series batch        only the batch series
    --series sequential   only the m successive calls: with --tree DIR the package is imported from another checkout of the project, built
                          there -- the parent commit's, for a baseline that does not contain this feature at all
    --series both         (default) both from this tree, alternating

One process; run it under a time limit of its own:

    timeout -k 10 900 python tools/register_batch_cost.py

The figures of profiles/register_batch.txt are this tool's output."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def q(t):
    t = np.asarray(t)
    return "%10.3f (%.3f .. %.3f; %d samples)" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90), len(t))


def starts_of(m, pose, seed=3):
    """m starts: up to 0.3 m and 0.1 rad off the pose the scan was cast from."""
    rng = np.random.RandomState(seed)
    d = rng.uniform(-1.0, 1.0, (m, 3)) * np.array([0.3, 0.3, 0.1])
    return (np.array(pose, np.float64) + d).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--maps", type=int, nargs="+", default=[4000, 100000])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20, help="batch calls per (map, m)")
    ap.add_argument("--seq-budget", type=float, default=30.0, help="seconds of sequential calls per (map, m), three samples at the least")
    ap.add_argument("--full", type=int, default=4096, help="rows of the full launch timed at the end (0: none)")
    ap.add_argument("--series", choices=("both", "batch", "sequential"), default="both")
    ap.add_argument("--tree", default=ROOT, help="checkout to import the package from")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    pkg = importlib.import_module("gpu-icp-slam_amd")
    print("package of %s, series: %s" % (os.path.abspath(a.tree), a.series))
    pose = (0.5, 0.3, 0.1)
    for n_map in a.maps:
        pts, segs = pkg.synth.make_map_points(n_map, seed=1)
        scan = pkg.synth.make_scan(segs, pose, seed=7)
        h = pkg.PfSlam(64, kd_capacity=1 << 18)
        h.set_map(pkg.kd_create(pts))
        h.set_scan(scan)
        opts = dict(eps_xy=0.0, eps_theta=0.0, max_iters=a.iters)
        print("map of %d points, 1081 beams, %d iterations; ms: median (p10 .. p90)" % (n_map, a.iters))
        print("  %6s   %-48s %-48s %s" % ("rows", "one register_batch call", "m register calls", "ratio of the medians"))
        for m in a.rows:
            starts = starts_of(m, pose)

            def batch():
                return h.register_batch(starts, **opts)

            def sequential():
                return [h.register(s, **opts) for s in starts]

            tb, ts = [], []
            if a.series == "both":                      # the two paths give the same bits: checked once per (map, m), outside the timing
                got, want = batch(), sequential()
                for r in range(m):
                    assert (got["poses"][r].view(np.int32) == want[r]["pose"].view(np.int32)).all(), "row %d: the two paths disagree" % r
            if a.series != "sequential":
                for _ in range(3):
                    batch()
            if a.series != "batch":
                one = timed(sequential)                 # (also the warm-up)
                n_seq = int(max(3, min(a.calls, a.seq_budget * 1e3 / max(one, 1e-3))))
            else:
                n_seq = 0
            n_batch = a.calls if a.series != "sequential" else 0
            for blk in range(5):                        # alternate the two series in five blocks
                for _ in range(n_batch // 5 + (blk < n_batch % 5)):
                    h.synchronize()
                    tb.append(timed(batch))
                for _ in range(n_seq // 5 + (blk < n_seq % 5)):
                    h.synchronize()
                    ts.append(timed(sequential))
            ratio = "%.1f" % (np.median(ts) / np.median(tb)) if tb and ts else "-"
            print("  %6d   %-48s %-48s %s" % (m, q(tb) if tb else "-", q(ts) if ts else "-", ratio), flush=True)
        if a.full > 0 and a.series != "sequential":
            starts = starts_of(a.full, pose)
            full = dict(eps_xy=0.0, eps_theta=0.0)      # the default 40 iterations, every one of them
            h.register_batch(starts, **full)
            t = []
            for _ in range(5):
                h.synchronize()
                t.append(timed(lambda: h.register_batch(starts, **full)))
            print("  full launch: %d rows x 40 iterations: %s ms" % (a.full, q(t)), flush=True)
        h.close()


if __name__ == "__main__":
    main()
