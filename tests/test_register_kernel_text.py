"""The pfslam_nearest / pfslam_register kernels' own text, run on the CPU (no GPU needed): tests/register_emu.cpp compiles the kernels cut
out of csrc/pfslam_register.hip.inc -- with csrc/pf_math.h, csrc/kd_device.h and the pieces of csrc/pfslam_stages.hip.inc they reuse, none
of them changed -- behind a small SIMT shim (a thread per GPU thread, barriers for __syncthreads and the wave shuffles) as a stand-alone
program with -ffp-contract=off like the library, under AddressSanitizer and UBSan with every buffer at its exact size.  register must give
the restatement's status, pose and trace bit for bit (tests/register_ref.py), nearest its index and d2 -- which also shows that no index
leaves a buffer, that every thread reaches every barrier and that the stackless walk ends on every kind of tree the library holds.  What it
cannot show is the GPU's arithmetic and memory model: tests/test_gpu_register.py does."""
import struct

import numpy as np
import pytest

import kernel_text as KT
from kernel_text import device_arrays
import register_ref as R

MAPS = ("p2", "p3", "p4000", "np300", "grown4500")
# (map, beams, match, select, update, max_iters, max_dist)
CASES = [(m, 1081, 1, 1, 1, 4, 0.5 if m in ("p4000", "grown4500") else 0.0) for m in MAPS if m not in ("p2", "p3")]
CASES += [("p4000", nb, 1, 1, 1, 3, 0.5) for nb in (1, 64, 65, 1024, 1025, 4096)]
CASES += [("p4000", 1081, 0, 0, 0, 3, 0.5), ("grown4500", 1025, 0, 1, 1, 3, 0.5), ("np300", 65, 1, 0, 0, 3, 0.5), ("np300", 1024, 0, 1, 0, 2, 0.0),
          ("p2", 64, 0, 0, 1, 2, 0.5), ("p2", 1081, 1, 0, 0, 2, 0.5), ("p3", 1, 1, 0, 1, 2, 0.5), ("p3", 4096, 0, 0, 0, 2, 0.5),
          ("p4000", 1081, 1, 1, 1, 40, 0.5)]


@pytest.fixture(scope="module")
def maps(pkg):
    p4000, segs, _ = R.planar_tree(4000, seed=1)
    grown, _ = R.grown_tree(4000, 500, seed=1)
    out = {"p2": R.planar_tree(2, seed=1)[0], "p3": R.planar_tree(3, seed=1)[0], "p4000": p4000, "np300": R.nonplanar_tree(300),
           "grown4500": grown}
    depth = lambda t: max(len(_path(t, i)) for i in range(len(t) - 40, len(t)))
    assert depth(grown) > 3 * depth(p4000), "the insert-grown tree is meant to be deep"
    return out, pkg.synth.make_scan(segs, (0.5, 0.3, 0.1), seed=7)


def _path(tree, i):
    p = []
    while i >= 0:
        p.append(i)
        i = int(tree["parent"][i])
    return p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return KT.build(tmp_path_factory, "register", ("k_register", "kd_nearest_exact", "void svd3"), ("PF_LIDAR_RANGE", "PF_SVD_EPSILON"))


def run_emu(emu, tag, tree, scan, queries, opts, start, use_start=1):
    d, exe = emu
    hot, z, parent, w, planar = device_arrays(tree)
    scan = np.ascontiguousarray(scan, np.float32)
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    o = dict(R.DEFAULTS)
    o.update(opts)
    fin, fout = str(d / ("in_%s.bin" % tag)), str(d / ("out_%s.bin" % tag))
    with open(fin, "wb") as f:
        f.write(np.array([len(tree), planar, len(scan), len(q), use_start, 0, 0, 0], np.int32).tobytes())
        for a in (hot, z, parent, w, scan, q):
            f.write(np.ascontiguousarray(a).tobytes())
        f.write(struct.pack("<4i3fi", o["max_iters"], o["match"], o["select"], o["update"], o["max_dist"], o["eps_xy"], o["eps_theta"], o["min_pairs"]))
        f.write(np.ascontiguousarray(start, np.float32).tobytes())
    KT.run(exe, fin, fout)
    raw = np.fromfile(fout, np.uint8)
    res = {}
    off = 0
    if len(scan):
        k = 12 + 8 * o["max_iters"]
        out = raw[:4 * k].view(np.float32)
        off = 4 * k
        it = int(out[5])
        res["register"] = {"pose": out[0:3].copy(), "status": int(out[4]), "iterations": it, "pairs": int(out[6]), "residual": float(out[7]),
                           "trace": out[12:12 + 8 * it].reshape(-1, 8).copy()}
    if len(q):
        n = len(q)
        res["best"] = raw[off:off + 4 * n].view(np.int32)
        res["d2"] = raw[off + 4 * n:off + 8 * n].view(np.float32)
        res["visits"] = raw[off + 8 * n:off + 12 * n].view(np.uint32)
    return res


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-m%ds%du%d-i%d" % c[:6])
def test_register_kernel_text_on_the_cpu_equals_the_restatement(emu, maps, case):
    trees, scan1081 = maps
    name, nb, match, select, update, iters, max_dist = case
    scan = np.resize(scan1081, nb) if nb != 1081 else scan1081
    start = np.array([0.6, 0.22, 0.13], np.float32)
    opts = dict(match=match, select=select, update=update, max_iters=iters, max_dist=max_dist)
    got = run_emu(emu, "r_%s_%d_%d%d%d_%d" % case[:6], trees[name], scan, np.zeros((0, 3)), opts, start)["register"]
    want = R.register(trees[name], scan, start, **opts)
    assert R.same_result(got, want) is None, R.same_result(got, want)
    if iters == 40:
        assert want["status"] == 1 and 1 < want["iterations"] < 40     # (the run that stops on eps)


def test_register_kernel_text_statuses_2_and_3_and_the_handles_pose(emu, maps):
    trees, scan = maps
    tree = trees["p4000"]
    far = np.full(65, 1000.0, np.float32)
    got = run_emu(emu, "s2", tree, far, np.zeros((0, 3)), {}, [1.0, 2.0, 0.3])["register"]
    assert R.same_result(got, R.register(tree, far, [1.0, 2.0, 0.3])) is None and got["status"] == 2 and got["iterations"] == 0
    big = np.array([3.0e38, 3.0e38, 0.1], np.float32)     # x + t overflows under the reference's choices: not finite, status 3
    opts = dict(match=0, select=0, update=0, max_iters=3)
    got = run_emu(emu, "s3", tree, scan[:65], np.zeros((0, 3)), opts, big)["register"]
    want = R.register(tree, scan[:65], big, **opts)
    assert R.same_result(got, want) is None, R.same_result(got, want)
    print("status-3 probe: status %d after %d iterations" % (want["status"], want["iterations"]))
    # use_start = 0: the kernel reads the start from the pose buffer
    got = run_emu(emu, "hp", tree, scan[:65], np.zeros((0, 3)), dict(max_iters=2), [0.6, 0.22, 0.13], use_start=0)["register"]
    assert R.same_result(got, R.register(tree, scan[:65], [0.6, 0.22, 0.13], max_iters=2)) is None


@pytest.mark.parametrize("name", MAPS)
def test_nearest_kernel_text_on_the_cpu_equals_brute_force(emu, maps, name):
    trees, _ = maps
    tree = trees[name]
    q = R.tie_queries(tree, 2000)
    q[7] = [np.nan, 0.0, 0.0]
    q[8] = [0.0, -np.inf, 0.0]
    got = run_emu(emu, "n_" + name, tree, np.zeros(0), q, {}, [0, 0, 0])
    best, d2 = R.nearest(tree, q)
    assert (got["best"] == best).all(), np.nonzero(got["best"] != best)[0][:10]
    assert (R.bits(got["d2"]) == R.bits(d2)).all()
    assert got["best"][7] == -1 and got["best"][8] == -1
    print("%s: %d nodes, node evaluations per query: mean %.1f, max %d" % (name, len(tree), got["visits"].mean(), got["visits"].max()))


def test_tie_queries_do_hold_exact_ties(maps):
    """The query set is meant to exercise the lowest-index rule: count the queries whose two smallest distances are equal."""
    trees, _ = maps
    tree = trees["p4000"]
    q = R.tie_queries(tree, 2000)
    nx, ny = tree["x"][None, :], tree["y"][None, :]
    dx, dy = nx - q[:, 0:1], ny - q[:, 1:2]
    d = (dx * dx + dy * dy) + np.float32(0) * np.float32(0)
    two = np.partition(d, 1, axis=1)[:, :2]
    assert (two[:, 0] == two[:, 1]).sum() >= 50
