"""The pfslam_cast_score kernel's own text, run on the CPU (no GPU needed), after the pattern of tests/test_cast_kernel_text.py:
tests/cast_score_emu.cpp compiles the kernels cut out of csrc/pfslam_cast.hip.inc (the raster and the shared walk) and out of
csrc/pfslam_cast_score.hip.inc behind the SIMT shim, as a stand-alone program with -ffp-contract=off like the library, under
AddressSanitizer and UBSan, every buffer at exactly the size the entry point requests.  Rows, classes and stats must be the restatement's
(tests/cast_score_ref.py), bit for bit -- for the walk the library runs and for the plain walk, for the pose list (x, y, theta rows) and
for the particle block (three arrays with a stride between them).  What it cannot show is the GPU's arithmetic, its shuffles and its
atomics: tests/test_gpu_cast_score.py does."""

import numpy as np
import pytest

import cast_ref as CR
import cast_score_ref as SR
import kernel_text as KT
from kernel_text import poses_of

RES = (0.025, 0.025)


@pytest.fixture(scope="module")
def world(pkg):
    pts, segs = pkg.synth.make_map_points(4000, seed=1)
    return pts, pkg.synth.make_scan(segs, (0.5, 0.3, 0.1), noise=0).astype(np.float32)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    for sec, names in (("cast", ("k_cast_box", "k_cast_splat", "k_cast_count", "cast_walk", "k_cast_rays")), ("cast_score", ("k_cast_score", "cast_walk<SKIP>"))):
        for name in names:                                      # (each in its own section: either text names the other's functions too)
            assert name in KT.section(sec)
    return KT.build(tmp_path_factory, "cast_score", ())


def run_emu(emu, tag, nodes, poses, scan, nb, res=RES, soa=0, classes=True, cast=None, **opts):
    d, exe = emu
    c, o = CR.options(**(cast or {})), SR.options(**opts)
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 4)
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 3)
    m = len(poses)
    u, fcap = SR.unit(o["tol"], o["clip"])
    stride = m + 5 if soa else 0                     # (the block of a shard: the arrays lie `shard_stride` apart, the pad is never read)
    if soa:
        block = np.full((3, stride), np.nan, np.float32)
        block[:, :m] = poses.T
    else:
        block = poses
    fin, fout = str(d / ("in_%s.bin" % tag)), str(d / ("out_%s.bin" % tag))
    with open(fin, "wb") as f:
        f.write(np.array([nb, 0, m, len(nodes), c["inflate"], c["skip_cells"], soa, stride, o["count_miss"], int(fcap), int(classes), 0], np.int32).tobytes())
        f.write(np.array([res[0], res[1], c["max_range"], c["w_min"], o["tol"], u, o["z_min"], o["z_max"]], np.float32).tobytes())
        f.write(nodes.tobytes())
        f.write(np.ascontiguousarray(block).tobytes())
        f.write(np.ascontiguousarray(scan, np.float32).tobytes())
    KT.run(exe, fin, fout)
    raw = open(fout, "rb").read()
    rays = m * nb
    one = 64 + 32 * m + (rays if classes else 0)
    assert len(raw) == 2 * one
    out = []
    for at in (0, one):                              # the walk the library runs, then the plain walk
        rows = np.frombuffer(raw, np.int32, 8 * m, at + 64).reshape(m, 8)
        out.append({"stats": np.frombuffer(raw, np.int64, 8, at), "rows": rows, "best": SR.best_of(rows),
                    "classes": np.frombuffer(raw, np.uint8, rays, at + 64 + 32 * m).reshape(m, nb) if classes else None})
    return out


def check(emu, tag, nodes, poses, scan, nb, res=RES, cast=None, layouts=(0, 1), **opts):
    want = SR.score_map(nodes, poses, scan[:nb], nb, res, cast=cast, **opts)
    for soa in layouts:
        for classes in ((True, False) if soa == 0 and len(poses) <= 6 else (True,)):   # (without the class bytes: the pointer is NULL)
            got = run_emu(emu, "%s_%d%d" % (tag, soa, classes), nodes, poses, scan[:nb], nb, res, soa, classes, cast, **opts)
            for walk, g in zip(("jumping", "plain"), got):
                why = SR.same(g, want, classes=classes)
                assert why is None, "%s walk, %s poses, classes %r: %s" % (walk, "SoA" if soa else "AoS", classes, why)
    return want


@pytest.mark.parametrize("nb,m", [(1, 1), (65, 3), (255, 2), (257, 2), (1081, 1), (65, 65)])
def test_the_kernel_text_on_the_cpu_equals_the_restatement(emu, world, nb, m):
    pts, scan = world
    want = check(emu, "c_%d_%d" % (nb, m), pts, poses_of(m), scan, nb)
    print("%d beams x %d poses: row 0 %r, best %d, %d of %d rays hit" % (nb, m, want["rows"][0].tolist(), want["best"], want["stats"][1], want["stats"][0]))
    assert nb < 65 or (want["rows"][0, 0] > 0 and want["rows"][0, 1] > 0)
    if nb >= 255:
        assert want["best"] == 0


def test_every_class_dense_walls_no_cost_for_a_miss_and_the_smallest_tolerance(emu, world):
    pts, scan = world
    poses = np.concatenate([poses_of(4), [[np.nan, 0.0, 0.0], [3000.0, 0.0, 0.0]]]).astype(np.float32)
    s = scan.copy()
    s[::11], s[5::97], s[7::101] = np.nan, np.inf, -1.0
    want = check(emu, "classes", pts, poses, s, 1081)
    assert set(np.unique(want["classes"]).tolist()) == {0, 1, 2, 3, 4}
    assert (want["rows"][4:, 4] == want["rows"][4:, 0]).all(), "a pose that is not finite or far outside: every valid beam misses"
    check(emu, "dense", pts, poses, s, 257, cast=dict(w_min=-113.0, inflate=0, skip_cells=0), layouts=(1,))
    want = check(emu, "nomiss", pts, poses, s, 257, count_miss=0, layouts=(0,))
    assert (want["rows"][:, 7] == want["rows"][:, 5]).all()
    want = check(emu, "tol", pts, poses, s, 257, tol=1e-4, clip=0.2, z_max=3.0e38, layouts=(1,))
    assert want["qcap"] == 32000 and want["rows"][:, 5].max() > 32000
    want = check(emu, "empty", pts, poses, s, 65, cast=dict(w_min=500.0), layouts=(0,))
    assert (want["rows"][:, 4] == want["rows"][:, 0]).all() and want["best"] == -1 and want["stats"][1] == 0


def test_oblong_cells(emu, world):
    pts, scan = world
    want = check(emu, "oblong", pts, poses_of(3), scan, 1081, res=(0.025, 0.05))
    assert want["rows"][0, 1] > 0
