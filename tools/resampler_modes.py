#!/usr/bin/env python3
"""What the resampler modes (pfslam_set_resampler) cost and buy on bench.py's workload: 100 000 particles, the 100 000-point map, five
dispersions, `--warmup` frames, then a `--steps`-frame window.  Per mode, on a fresh handle each:

  ms_per_step          wall time of the window (frames in flight, one synchronize at its end), best of `--repeats` handles
  resample_ms          the resample phase per frame: pfslam_set_timing(h, 2) / pfslam_get_timers slot 4, from a second pass over the same frames
                       (phase timing serialises the frame, so it is not part of the window above)
  resampled            frames of the window that resampled
  distinct_poses       np.unique over the (x, y, theta) of the particles read back right after the first frame that resampled

Prints one JSON line per mode and a closing line with the differences to mode 0.
    python tools/resampler_modes.py [--particles 100000] [--map-points 100000] [--steps 20] [--warmup 5] [--repeats 3]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--map-points", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    pkg = importlib.import_module("gpu-icp-slam_amd")
    pts, segs = pkg.synth.make_map_points(a.map_points, seed=1)
    tree = pkg.kd_create(pts)
    n_frames = a.warmup + a.steps
    scans = [pkg.synth.make_scan(segs, (0.002 * f, 0.001 * f, 0.0004 * f), seed=2000 + f) for f in range(n_frames)]
    cap = a.map_points + max(1 << 18, 1081 * n_frames)

    def engine(mode):
        h = pkg.PfSlam(a.particles, kd_capacity=cap)
        h.set_map(tree)
        h.set_resampler(mode)
        for f in range(1, 6):
            h.motion_update(f)
        return h

    results = {}
    for mode in (0, 1, 2):
        best = None
        for _ in range(a.repeats):                      # the window, frames in flight
            h = engine(mode)
            for k in range(a.warmup):
                h.step(6 + k, scans[k])
            h.synchronize()
            t0 = time.perf_counter()
            for k in range(a.warmup, n_frames):
                h.step(6 + k, scans[k])
            h.synchronize()
            dt = (time.perf_counter() - t0) * 1e3 / a.steps
            best = dt if best is None else min(best, dt)
            h.close()
        h = engine(mode)                                # the phase timers and the look behind the first resampled frame
        distinct, first, resampled = None, None, 0
        for k in range(n_frames):
            if k == a.warmup:
                h.set_timing(2)
            h.step(6 + k, scans[k])
            did = h.trace()["resampled"]
            resampled += did if k >= a.warmup else 0
            if did and distinct is None:
                p = h.particles()
                first = 6 + k
                distinct = len(np.unique(np.stack([p["x"], p["y"], p["theta"]], axis=1).view(np.int32), axis=0))
        t = h.timers()
        h.close()
        results[mode] = dict(mode=mode, particles=a.particles, steps=a.steps, ms_per_step=round(best, 4),
                             resample_ms=round(t["resample_ms"] / max(1, t["resample_count"]), 5), resample_frames_timed=t["resample_count"],
                             resampled=resampled, first_resampled_frame=first, distinct_poses=distinct)
        print(json.dumps(results[mode]), flush=True)
    base = results[0]
    print(json.dumps({"vs_mode_0": {m: dict(ms_per_step=round(results[m]["ms_per_step"] - base["ms_per_step"], 4),
                                             resample_ms=round(results[m]["resample_ms"] - base["resample_ms"], 5)) for m in (1, 2)}}))


if __name__ == "__main__":
    main()
