"""A frame composed of STAGE calls: an oracle for pfslam_step / pfslam_step_grid in either arithmetic mode.

TEST INFRASTRUCTURE (helper module, not a conftest).  In device-library mode (pfslam_set_trig(h, 1)) the CPU oracle cannot follow the
product, but every stage entry point of include/pfslam.h is pinned to the reference's own kernel compiled for gfx950 with zero mismatches
(tests/test_gpu_ref_kernels.py), and a frame is by definition the composition of those stages in the order of particleFilter
(kernel.cu:1702-1762; restated in oracle/pfslam_oracle.c, orc_slam_step).  StageShadow holds ONE PfSlam handle and steps it through
the public stage entry points in exactly that order; it never calls pfslam_step, pfslam_step_grid or pfslam_shard_*, so none of the
frame loop's own kernels (k_motion_count, k_icp_fused, k_walls, k_wall_runs, k_score_kd_cells as the frame launches it, ...) run in it.
tests/test_gpu_devlib_frames.py first proves the composition in the default mode -- shadow == CPU oracle == pfslam_step, every frame --
and then uses the shadow as the oracle of device-library frames.

The interface is the part of oracle_lib.Slam the tests use (step, step_grid, trace, pose, particles, tree / map, grid, cells, kd_size,
set_particles, set_map, set_grid, close).  The H11 half-array mirror (strict_host_mirror = 1, the default) is carried by the stage
kernels themselves (mirror_count: k_motion restores the weights from the mirror, the weight kernels write the first half of it, the
resample all of it), so the stage path reproduces it across frames and the shadow needs no host copy of its own."""
import importlib

import numpy as np


def _pkg():
    return importlib.import_module("gpu-icp-slam_amd")


class StageShadow:
    def __init__(self, n_particles, n_beams=1081, kd_capacity=1 << 20, strict_host_mirror=1, free_upload_bug=0, balance_period=100,
                 map_scale=None, map_res=None, trig=0, variant=None, pkg=None):
        self.pkg = pkg or _pkg()
        self.h = self.pkg.PfSlam(n_particles, n_beams=n_beams, kd_capacity=kd_capacity, strict_host_mirror=strict_host_mirror,
                                 free_upload_bug=free_upload_bug, balance_period=balance_period, map_scale=map_scale, map_res=map_res)
        self.n, self.nb = n_particles, n_beams
        self._trace = {"best": 0, "resampled": 0, "n_wall": 0, "n_free": 0, "n_insert": 0, "neff": 0.0, "kd_size": 0}
        self.dispersed = None   # the particles of the last frame right behind its dispersion (what the frame's scan-match pass scores)
        if trig:
            self.set_trig(trig)
        if variant is not None:
            self.set_variant(variant)

    # ---- options forwarded to the handle
    def set_trig(self, devlib):
        self.h.set_trig(devlib)

    def set_variant(self, v):
        self.h.set_variant(v)

    def set_particles(self, p):
        self.h.set_particles(p)

    def set_map(self, tree):
        self.h.set_map(tree)

    def set_grid(self, grid):
        self.h.set_grid(grid)

    def move_particles(self, frame, delta, cov=None, **opts):
        self.h.move_particles(frame, delta, cov, **opts)

    def motion_update(self, frame):
        """(the warm-up dispersions some tests put in front of their first frame)"""
        self.h.motion_update(frame)

    # ---- particleFilter (kernel.cu:1702-1762), as orc_slam_step composes it
    def step(self, frame, scan, keep_dispersed=False):
        h = self.h
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        h.maybe_balance(frame)                               # kernel.cu:1707-1711
        if h.kd_size == 0:                                   # kernel.cu:1714-1717: the first scan seeds the map at pose 0
            h.set_pose((0.0, 0.0, 0.0))
            h.set_scan(scan)
            h.update_map_kd()
            t = h.trace()
            self._trace = {"best": -1, "resampled": 0, "n_wall": t["n_wall"], "n_free": t["n_free"], "n_insert": 0, "neff": 0.0,
                           "kd_size": h.kd_size}
            return
        h.set_scan(scan)
        h.motion_update(frame)                               # PFMotionUpdate
        if keep_dispersed:
            self.dispersed = h.particles().copy()
        h.score_kd(fetch=False)                              # PFMeasurementUpdateKD: scores ...
        best, _, _ = h.measurement_update()                  # ... min / max / first argmax, weights; the best particle's pose stays on the device
        h.icp()                                              # transformPointICP: around the PREVIOUS pose, from the best particle
        h.update_map_kd()                                    # PFUpdateMapKD
        t = h.trace()
        did, neff = h.resample(frame)                        # PFResample
        self._trace = {"best": int(best), "resampled": int(did), "n_wall": t["n_wall"], "n_free": t["n_free"], "n_insert": t["n_insert"],
                       "neff": float(np.float32(neff)), "kd_size": h.kd_size}

    # ---- the same loop with the 2-D stages (orc_slam_step_grid)
    def step_grid(self, frame, scan):
        h = self.h
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        h.set_scan(scan)
        h.motion_update(frame)
        fit = h.score_grid()                                 # score + int min / max / first argmax + weights (kernel.cu:307-339)
        best = int(np.argmax(fit))                           # (first occurrence, as thrust::max_element)
        p = h.particles()
        h.set_pose((p["x"][best], p["y"][best], p["theta"][best]))
        h.update_map_grid()
        did, neff = h.resample(frame)
        self._trace = {"best": best, "resampled": int(did), "n_wall": 0, "n_free": 0, "n_insert": 0, "neff": float(np.float32(neff)),
                       "kd_size": 0}

    # ---- read-back
    def trace(self):
        return dict(self._trace)

    @property
    def pose(self):
        return self.h.pose

    @property
    def kd_size(self):
        return self.h.kd_size

    def particles(self):
        return self.h.particles()

    def tree(self):
        return self.h.map()

    map = tree

    @property
    def grid(self):
        return self.h.grid()

    def cells(self, which):
        return self.h.cells(which)

    def close(self):
        self.h.close()
