#!/usr/bin/env python3
"""What pfslam_move_particles costs, and what it changes in a free-running loop.

Cost: HIP events on the handle's stream around --batch back-to-back calls (no host wait in between: the calls only enqueue), divided by
the batch, after a warm-up batch; beside it, in the same process and the same way, pfslam_shift_particles and pfslam_motion_update (the
dispersion: the same three erfcinv evaluations per particle, no sincos).  Context, not a ratio to meet.  Median with 10th and 90th
percentile of --calls batches.

Scenario (--scenario): tests/loop_scenario.py's free-running square loop (turns of a quarter circle, 0.1 m per frame), the commanded motion
of every frame handed over with pfslam_shift_particles, with pfslam_move_particles without noise, and with pfslam_move_particles with
floors of 1 cm / 0.005 rad; the distance of the frame's pose from the commanded trajectory, per frame.  Reported, not asserted.

One process; run it under a time limit of its own:

    timeout -k 10 600 python tools/move_cost.py [--particles 1000 100000 1000000] [--scenario]

The figures of profiles/move_particles.txt are this tool's output."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COV = np.array([0.106 ** 2, 0.3 * 0.106 * 0.003, -0.2 * 0.106 * 0.00037, 0.003 ** 2, 0.4 * 0.003 * 0.00037, 0.00037 ** 2], np.float32)


def q(t):
    t = np.asarray(t) * 1e3
    return "%9.2f (%.2f .. %.2f)" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90))


def cost(pkg, a):
    import torch
    stream = torch.cuda.Stream()

    def timed(call):
        for _ in range(a.batch):                          # warm-up: code loaded
            call()
        t = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.batch):
                call()
            e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / a.batch)
        return t

    print("us per call: median (p10 .. p90) of %d batches of %d calls; HIP events around each batch" % (a.calls, a.batch))
    print("particles   pfslam_shift_particles        pfslam_motion_update          pfslam_move_particles (full covariance)")
    for n in a.particles:
        rng = np.random.RandomState(n)
        p = np.zeros(n, pkg.PARTICLE_DTYPE)
        p["x"], p["y"] = 12.3 + rng.normal(0, 0.015, n), -7.9 + rng.normal(0, 0.015, n)
        p["theta"], p["w"] = 1.1 + rng.normal(0, 0.01, n), 1.0
        h = pkg.PfSlam(n)
        h.set_stream(stream.cuda_stream)
        h.set_particles(p)
        d = np.array([1e-4, -1e-4, 1e-5], np.float32)
        frame = [0]

        def move():
            frame[0] += 1
            h.move_particles(frame[0], d, COV, ref_theta=1.1, cov_scale=1e-4)

        def motion():
            frame[0] += 1
            h.motion_update(frame[0])

        ts, tm, tv = timed(lambda: h.shift_particles(d)), timed(motion), timed(move)
        h.close()
        print("%9d   %s   %s   %s" % (n, q(ts), q(tm), q(tv)), flush=True)


def scenario(pkg, a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import loop_scenario as LS
    nf = a.frames
    traj, scans = LS.trajectory_free(nf), LS.scans(pkg, nf)
    modes = (("shift", None), ("move, no noise", {}), ("move, floors 1 cm / 0.005 rad", dict(sigma_xy_min=0.01, sigma_theta_min=0.005)))
    print("free-running square loop, %d frames, %d particles: distance of the frame's pose from the commanded trajectory" % (nf, a.scenario_particles))
    print("%-32s  mean m    median m  max m     at frame  mean |heading| rad  largest frames: frame:m" % "odometry call")
    for name, kw in modes:
        h = pkg.PfSlam(a.scenario_particles, kd_capacity=1 << 20)
        err, herr = [], []
        for f in range(1, nf + 1):
            if f > 1:
                delta = traj[f - 1] - traj[f - 2]
                if kw is None:
                    h.shift_particles(delta)
                else:
                    h.move_particles(f, delta, None, ref_theta=float(traj[f - 2][2]), **kw)
            h.step(f, scans[f - 1])
            if f % 5 == 0 or f == nf:                     # (a look books the frames in flight)
                pose = np.asarray(h.pose, np.float64)
                err.append((f, float(np.hypot(pose[0] - traj[f - 1][0], pose[1] - traj[f - 1][1]))))
                herr.append(abs(pose[2] - traj[f - 1][2]))
        h.close()
        e = np.array([v for _, v in err])
        worst = sorted(err, key=lambda fv: -fv[1])[:4]
        print("%-32s  %.4f    %.4f    %.4f    %5d     %.5f             %s"
              % (name, e.mean(), np.median(e), e.max(), worst[0][0], np.mean(herr), " ".join("%d:%.3f" % fv for fv in worst)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, nargs="+", default=[1000, 100000, 1000000])
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--scenario", action="store_true", help="the scenario table instead of the cost table")
    ap.add_argument("--frames", type=int, default=130)
    ap.add_argument("--scenario-particles", type=int, default=20000)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("gpu-icp-slam_amd")
    (scenario if a.scenario else cost)(pkg, a)


if __name__ == "__main__":
    main()
