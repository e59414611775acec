#!/usr/bin/env python3
"""What pfslam_estimate costs against the only way to get the same numbers without it: read the whole cloud back
(pfslam_get_particles: a wait for the device, four device-to-host copies, a repack into 32-byte structs) and reduce it on the host.

For each particle count: 100 calls of PfSlam.estimate() and 100 of PfSlam.particles() + a numpy reduction (weighted mean, the six
centred moments, Neff, in float64), each series behind a synchronize(), wall time per call; median, 10th and 90th percentile.  One
process; run it under a time limit of its own:

    timeout -k 10 300 python tools/estimate_cost.py [--particles 1000 100000 1000000] [--calls 100]

The figures of profiles/estimate.txt are this tool's output."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_reduction(p):
    """Mean, covariance and Neff from a read-back cloud, as a caller would write it."""
    w = p["w"].astype(np.float64)
    s0 = w.sum()
    pos = np.stack([p["x"], p["y"], p["theta"]]).astype(np.float64)
    mean = (pos * w).sum(axis=1) / s0
    d = pos - mean[:, None]
    cov = (d * w) @ d.T / s0
    return mean, cov, s0 * s0 / (w * w).sum()


def series(fn, calls):
    t = np.empty(calls)
    for k in range(calls):
        t0 = time.perf_counter()
        fn()
        t[k] = time.perf_counter() - t0
    return t * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, nargs="+", default=[1000, 100000, 1000000])
    ap.add_argument("--calls", type=int, default=100)
    a = ap.parse_args()
    pkg = importlib.import_module("gpu-icp-slam_amd")
    print("particles   estimate() ms: median (p10 .. p90)   particles() + numpy ms: median (p10 .. p90)   read-back / estimate")
    for n in a.particles:
        rng = np.random.RandomState(n)
        p = np.zeros(n, pkg.PARTICLE_DTYPE)
        p["x"] = 12.3 + rng.normal(0, 0.015, n)
        p["y"] = -7.9 + rng.normal(0, 0.015, n)
        p["theta"] = 1.1 + rng.normal(0, 0.01, n)
        p["w"] = rng.uniform(0, 1, n)
        h = pkg.PfSlam(n)
        h.set_particles(p)
        est = h.estimate()
        mean, cov, neff = host_reduction(h.particles())
        assert np.allclose(est["mean"], mean, atol=1e-5) and np.allclose(est["cov"], cov, rtol=1e-3, atol=1e-9), "the two paths disagree"
        for fn in (h.estimate, lambda: host_reduction(h.particles())):   # warm both paths
            for _ in range(5):
                fn()
        h.synchronize()
        te = series(h.estimate, a.calls)
        h.synchronize()
        tr = series(lambda: host_reduction(h.particles()), a.calls)
        h.close()
        q = lambda t: (np.median(t), np.percentile(t, 10), np.percentile(t, 90))
        print("%9d   %8.4f (%.4f .. %.4f)                  %8.4f (%.4f .. %.4f)                        %6.1fx"
              % ((n,) + q(te) + q(tr) + (np.median(tr) / np.median(te),)), flush=True)


if __name__ == "__main__":
    main()
