"""pfslam_register_batch restated: the rows are tests/register_ref.py's register, one call per start, and the pick of the best row is the
rule of include/pfslam.h in plain Python.

TEST INFRASTRUCTURE (helper module, not a test).  tests/test_register_batch_spec.py holds the rule to its edge cases and to the scenario
it was made for; tests/test_register_batch_kernel_text.py and tests/test_gpu_register_batch.py hold the kernel and the library to this."""
import numpy as np

import register_ref as R

CELL = 0.025                      # the map's resolution (m)
BEAM = np.deg2rad(0.25)           # the scan's angular step: 0.00437 rad
SCENARIO_POSES = ((0.5, 0.3, 0.1), (10.0, -8.0, 0.3))


def pick_best(info):
    """The row *best names, from info (m x 8: status, iterations, pairs, residual, ...) alone; -1 when no row is eligible."""
    info = np.asarray(info, np.float32).reshape(-1, 8)
    eligible = [r for r in range(len(info))
                if info[r, 0] in (0.0, 1.0) and info[r, 1] >= 1 and np.isfinite(info[r, 3])]
    if not eligible:
        return -1
    P = max(info[r, 2] for r in eligible)
    cand = [r for r in eligible if 2 * float(info[r, 2]) >= float(P)]
    # the smallest residual, then more pairs, then the lower row
    return min(cand, key=lambda r: (float(info[r, 3]), -float(info[r, 2]), r))


def info_rows(results):
    """m x 8 info of a list of register() results, as the C-ABI lays it out."""
    info = np.zeros((len(results), 8), np.float32)
    for r, res in enumerate(results):
        info[r, 0:4] = (res["status"], res["iterations"], res["pairs"], np.float32(res["residual"]))
    return info


def register_batch(tree, scan, starts, **opts):
    """pfslam_register_batch: dict with poses (m, 3), status, iterations, pairs, residual, info (m, 8) and best, like PfSlam.register_batch."""
    starts = np.ascontiguousarray(starts, np.float32).reshape(-1, 3)
    res = [R.register(tree, scan, s, **opts) for s in starts]
    info = info_rows(res)
    return {"poses": np.stack([r["pose"] for r in res]).astype(np.float32), "status": info[:, 0].astype(np.int32),
            "iterations": info[:, 1].astype(np.int32), "pairs": info[:, 2].astype(np.int32), "residual": info[:, 3].copy(), "info": info,
            "best": pick_best(info)}


def same_rows(got, want):
    """None when two register_batch() results agree bit for bit (poses and all eight info floats per row) and in best, else the first
    difference."""
    if got["poses"].shape != want["poses"].shape:
        return "shape: %r != %r" % (got["poses"].shape, want["poses"].shape)
    for r in range(len(want["poses"])):
        if not (R.bits(got["poses"][r]) == R.bits(want["poses"][r])).all():
            return "row %d pose: %r != %r" % (r, got["poses"][r].tolist(), want["poses"][r].tolist())
        if not (R.bits(got["info"][r]) == R.bits(want["info"][r])).all():
            return "row %d info: %r != %r" % (r, got["info"][r].tolist(), want["info"][r].tolist())
    if got["best"] != want["best"]:
        return "best: %r != %r" % (got["best"], want["best"])
    return None


def row_of_register(res):
    """(pose, info[8]) of one register() result (of the restatement or of PfSlam.register), for a bit comparison with a batch row."""
    info = np.zeros(8, np.float32)
    info[0:4] = (res["status"], res["iterations"], res["pairs"], np.float32(res["residual"]))
    return np.asarray(res["pose"], np.float32), info


def scenario_starts(p):
    """The 26 starts of the scenario: p + (dx, dy, dtheta), dx, dy in {-0.4, 0, 0.4}, dtheta in {-0.15, 0, 0.15}, without the centre."""
    out = []
    for dx in (-0.4, 0.0, 0.4):
        for dy in (-0.4, 0.0, 0.4):
            for dt in (-0.15, 0.0, 0.15):
                if dx == 0.0 and dy == 0.0 and dt == 0.0:
                    continue
                out.append((p[0] + dx, p[1] + dy, p[2] + dt))
    return np.array(out, np.float64).astype(np.float32)


def within_bounds(pose, p):
    err = np.abs(np.asarray(pose, np.float64) - np.array(p, np.float64))
    return bool(err[0] <= CELL and err[1] <= CELL and err[2] <= BEAM), err
