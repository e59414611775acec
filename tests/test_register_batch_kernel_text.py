"""The pfslam_register_batch kernel's own text, run on the CPU (no GPU needed): tests/register_batch_emu.cpp compiles the kernel cut out of
csrc/pfslam_register_batch.hip.inc -- behind the text of csrc/pfslam_register.hip.inc, csrc/pf_math.h, csrc/kd_device.h and the pieces of
csrc/pfslam_stages.hip.inc it reuses, none of them changed -- behind a small SIMT shim (a thread per GPU thread, barriers for
__syncthreads and the wave shuffles, the dynamic LDS a heap buffer of exactly the bytes the launch requests, the workgroups one after the
other) as a stand-alone program with -ffp-contract=off like the library, under AddressSanitizer and UBSan.  Every row must be the
restatement's register (tests/register_ref.py) bit for bit: pose, status, iterations, pairs, residual -- with either workgroup size the
host may pick -- which also shows that no index leaves the LDS buffer or a result row and that every thread reaches every barrier, in
rows that stop early too.  What it cannot show is the GPU's arithmetic and memory model: tests/test_gpu_register_batch.py does."""
import struct

import numpy as np
import pytest

import kernel_text as KT
from kernel_text import device_arrays
import register_batch_ref as B
import register_ref as R

START = np.array([0.6, 0.22, 0.13], np.float32)
# (map, beams, rows, threads, options)
CASES = [("p4000", 1, 3, 1024, dict(max_iters=3, min_pairs=1, max_dist=0.0)), ("p4000", 65, 3, 256, dict(max_iters=3)), ("p4000", 65, 3, 1024, dict(max_iters=2)),
         ("p4000", 1081, 3, 256, dict(max_iters=2)), ("p4000", 4096, 2, 1024, dict(max_iters=2)),
         ("np300", 1081, 2, 256, dict(max_iters=2, max_dist=0.0)), ("grown4500", 1025, 2, 1024, dict(max_iters=2)),
         ("p4000", 1081, 2, 256, dict(match=0, select=0, update=0, max_iters=3))]


def starts_of(m):
    """m starts around START, each its own run."""
    k = np.arange(m, dtype=np.float64)[:, None]
    return (START.astype(np.float64) + k * np.array([0.07, -0.05, 0.02])).astype(np.float32)


@pytest.fixture(scope="module")
def maps(pkg):
    p4000, segs, _ = R.planar_tree(4000, seed=1)
    grown, _ = R.grown_tree(4000, 500, seed=1)
    return {"p4000": p4000, "np300": R.nonplanar_tree(300), "grown4500": grown}, pkg.synth.make_scan(segs, (0.5, 0.3, 0.1), seed=7)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return KT.build(tmp_path_factory, "register_batch", ("k_register_batch", "HIP_DYNAMIC_SHARED", "kd_nearest_exact", "void svd3"), ("PF_LIDAR_RANGE", "PF_SVD_EPSILON"))


def run_emu(emu, tag, tree, scan, starts, threads, opts):
    d, exe = emu
    hot, z, parent, w, planar = device_arrays(tree)
    scan = np.ascontiguousarray(scan, np.float32)
    starts = np.ascontiguousarray(starts, np.float32).reshape(-1, 3)
    o = dict(R.DEFAULTS)
    o.update(opts)
    fin, fout = str(d / ("in_%s.bin" % tag)), str(d / ("out_%s.bin" % tag))
    with open(fin, "wb") as f:
        f.write(np.array([len(tree), planar, len(scan), len(starts), threads, 0, 0, 0], np.int32).tobytes())
        for a in (hot, z, parent, w, scan):
            f.write(np.ascontiguousarray(a).tobytes())
        f.write(struct.pack("<4i3fi", o["max_iters"], o["match"], o["select"], o["update"], o["max_dist"], o["eps_xy"], o["eps_theta"], o["min_pairs"]))
        f.write(starts.tobytes())
    KT.run(exe, fin, fout)
    out = np.fromfile(fout, np.float32).reshape(len(starts), 12)
    assert (out[:, 3] == 0).all() and (out[:, 8:] == 0).all()
    info = np.zeros((len(starts), 8), np.float32)
    info[:, 0:4] = out[:, 4:8]
    return {"poses": out[:, 0:3].copy(), "info": info, "status": info[:, 0].astype(np.int32), "iterations": info[:, 1].astype(np.int32),
            "best": B.pick_best(info)}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-m%d-t%d-%s" % (c[0], c[1], c[2], c[3], "ref" if c[4].get("match") == 0 else "i%d" % c[4]["max_iters"]))
def test_every_row_of_the_kernel_text_on_the_cpu_equals_the_restatement(emu, maps, case):
    trees, scan1081 = maps
    name, nb, m, threads, opts = case
    scan = np.resize(scan1081, nb) if nb != 1081 else scan1081
    starts = starts_of(m)
    got = run_emu(emu, "c_%s_%d_%d_%d" % (name, nb, threads, opts.get("match", 1)), trees[name], scan, starts, threads, opts)
    want = B.register_batch(trees[name], scan, starts, **opts)
    assert B.same_rows(got, want) is None, B.same_rows(got, want)
    assert nb == 1 or (want["iterations"] >= 1).any()


def test_a_forty_iteration_row_stops_on_eps(emu, maps):
    trees, scan = maps
    got = run_emu(emu, "eps40", trees["p4000"], scan, START[None, :], 256, {})
    want = B.register_batch(trees["p4000"], scan, START[None, :])
    assert B.same_rows(got, want) is None, B.same_rows(got, want)
    assert want["status"][0] == 1 and 1 < want["iterations"][0] < 40


@pytest.mark.parametrize("threads", [256, 1024])
def test_batches_that_mix_status_2_rows_status_3_rows_and_converging_rows(emu, maps, threads):
    """Without a gate a start whose targets overflow, or are NaN, reaches the fit (status 3); the rows between them stop on a coarse eps.
    With the gate the same starts, and one far from the map, keep no pair (status 2) beside a row that converges.  The failing rows
    come first and in the middle: a workgroup that leaves early must not disturb the rows behind it.  (No start with a non-finite
    HEADING here: csrc/pf_math.h converts the reduced angle to int, which the hardware defines for a NaN and UBSan rejects;
    tests/test_gpu_register_batch.py has that row.)"""
    trees, scan = maps
    starts = np.array([[3.0e38, 3.0e38, 0.1], [0.6, 0.22, 0.13], [np.nan, 0.3, 0.1], [0.52, 0.31, 0.102], [0.3, np.inf, 0.1]], np.float32)
    opts = dict(max_dist=0.0, max_iters=3, eps_xy=2e-2, eps_theta=5e-3)
    got = run_emu(emu, "mixed%d" % threads, trees["p4000"], scan[:65], starts, threads, opts)
    want = B.register_batch(trees["p4000"], scan[:65], starts, **opts)
    assert B.same_rows(got, want) is None, B.same_rows(got, want)
    print("no gate: status %s after %s iterations, best %d" % (want["status"].tolist(), want["iterations"].tolist(), want["best"]))
    assert want["status"][[0, 2, 4]].tolist() == [3, 3, 3] and (want["iterations"][[0, 2, 4]] == 0).all()
    assert want["status"][3] == 1 and want["status"][1] in (0, 1) and want["best"] in (1, 3)
    starts[4] = [100.0, 100.0, 0.1]
    opts = dict(max_iters=3, eps_xy=2e-2, eps_theta=5e-3)
    got = run_emu(emu, "gated%d" % threads, trees["p4000"], scan[:65], starts, threads, opts)
    want = B.register_batch(trees["p4000"], scan[:65], starts, **opts)
    assert B.same_rows(got, want) is None, B.same_rows(got, want)
    print("gated:   status %s after %s iterations, best %d" % (want["status"].tolist(), want["iterations"].tolist(), want["best"]))
    assert want["status"][[0, 2, 4]].tolist() == [2, 2, 2] and want["status"][3] == 1 and want["best"] in (1, 3)


def test_status_2_from_a_scan_of_rejected_ranges(emu, maps):
    trees, _ = maps
    far = np.full(65, 1000.0, np.float32)
    starts = starts_of(2)
    got = run_emu(emu, "s2", trees["p4000"], far, starts, 256, {})
    want = B.register_batch(trees["p4000"], far, starts)
    assert B.same_rows(got, want) is None and (got["status"] == 2).all() and (got["iterations"] == 0).all() and got["best"] == -1
    assert (R.bits(got["poses"]) == R.bits(starts)).all()
