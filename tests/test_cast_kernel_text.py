"""The pfslam_cast kernels' own text, run on the CPU (no GPU needed), after the pattern of tests/test_search_scan_kernel_text.py:
tests/cast_emu.cpp compiles the kernels cut out of csrc/pfslam_cast.hip.inc behind the SIMT shim, as a stand-alone program with
-ffp-contract=off like the library, under AddressSanitizer and UBSan, every buffer at exactly the size the entry points request.
Ranges, cells, stats and the raster must be the restatement's (tests/cast_ref.py), bit for bit -- for the walk the library runs (it
jumps: into the box, out of empty tiles) and for the plain walk it is measured against (every cell tested), which shows that a jump
never passes an occupied cell and that no index leaves the tiles.  What it cannot show is the GPU's arithmetic and its atomics:
tests/test_gpu_cast.py does."""

import numpy as np
import pytest

import cast_ref as CR
import kernel_text as KT
from kernel_text import poses_of

RES = (0.025, 0.025)


@pytest.fixture(scope="module")
def pts(pkg):
    return pkg.synth.make_map_points(4000, seed=1)[0]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return KT.build(tmp_path_factory, "cast", ("k_cast_box", "k_cast_splat", "k_cast_count", "k_cast_rays", "k_cast_expand"))


def run_emu(emu, tag, nodes, poses, nb, res=RES, **opts):
    d, exe = emu
    o = CR.options(**opts)
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 4)
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 3)
    m = len(poses)
    fin, fout = str(d / ("in_%s.bin" % tag)), str(d / ("out_%s.bin" % tag))
    with open(fin, "wb") as f:
        f.write(np.array([nb, 0, m, len(nodes), o["inflate"], o["skip_cells"], 0, 0], np.int32).tobytes())
        f.write(np.array([res[0], res[1], o["max_range"], o["w_min"], o["no_hit"], 0, 0, 0], np.float32).tobytes())
        f.write(nodes.tobytes())
        f.write(poses.tobytes())
    KT.run(exe, fin, fout)
    raw = open(fout, "rb").read()
    stats = np.frombuffer(raw, np.int64, 8)
    rays = m * nb
    occ = np.frombuffer(raw, np.uint8, offset=64 + 24 * rays + 4).reshape(int(stats[6]), int(stats[7]))
    out = []
    for at in (64, 64 + 12 * rays):                  # the walk the library runs, then the plain walk
        ranges = np.frombuffer(raw, np.float32, rays, at).reshape(m, nb)
        cells = np.frombuffer(raw, np.int32, 2 * rays, at + 4 * rays).reshape(m, nb, 2)
        out.append({"ranges": ranges, "cells": cells, "stats": stats.copy(), "occ": occ})
    out[1]["stats"][1] = np.frombuffer(raw, np.int32, 1, 64 + 24 * rays)[0]
    return out


def check(emu, tag, nodes, poses, nb, res=RES, **opts):
    o = CR.options(**opts)
    ras = CR.Raster(nodes, res, o["w_min"], o["inflate"])
    want = CR.cast(ras, poses, nb, **opts)
    for walk, got in zip(("jumping", "plain"), run_emu(emu, tag, nodes, poses, nb, res, **opts)):
        assert CR.same(got, want) is None, "%s walk: %s" % (walk, CR.same(got, want))
        assert got["occ"].shape == ras.dense().shape and (got["occ"] == ras.dense()).all(), "the raster differs"
    return want


@pytest.mark.parametrize("nb,m", [(1, 1), (65, 3), (1081, 1), (65, 65)])
@pytest.mark.parametrize("inflate", [0, 3])
def test_the_kernel_text_on_the_cpu_equals_the_restatement(emu, pts, nb, m, inflate):
    want = check(emu, "c_%d_%d_%d" % (nb, m, inflate), pts, poses_of(m), nb, inflate=inflate)
    print("%d beams x %d poses, inflate %d: %d of %d rays hit, %d qualifying nodes, |O| %d, box %r" % ((nb, m, inflate) + tuple(want["stats"][[1, 0, 2, 3]]) + (list(want["stats"][4:]),)))
    assert want["stats"][2] > 1500 and (nb * m < 65 or 0 < want["stats"][1] <= want["stats"][0])


def test_poses_outside_the_box_and_an_empty_raster(emu, pts):
    out = np.array([[30.0, 0.0, 3.1], [-25.0, -25.0, 0.8], [0.0, 45.0, -1.6], [21.0, 21.0, -2.4], [3000.0, 0.0, 0.0], [np.nan, 0.0, 0.0]], np.float32)
    want = check(emu, "outside", pts, out, 1081)
    assert (want["cells"][:4, :, 0] != CR.MISS).any(axis=1).all() and (want["cells"][4:] == CR.MISS).all()
    want = check(emu, "outside_dense", pts, out, 65, w_min=-113.0, inflate=0, skip_cells=0)
    assert want["stats"][2] == len(pts)
    want = check(emu, "empty", pts, poses_of(3), 65, w_min=500.0)
    assert list(want["stats"]) == [195, 0, 0, 0, 0, 0, 0, 0]


def test_oblong_cells_the_largest_step_count_and_a_short_range(emu, pts):
    res = (0.025, 0.05)
    check(emu, "oblong", pts, poses_of(3), 1081, res=res)
    small = pts[:300].copy()
    small[:, :2] *= 0.05                              # a map 2 m wide in cells of 1.25 mm: the walk is 16384 cells long
    fine = (0.025 / 20, 0.025 / 20)
    far = float(np.float32(16384) * np.float32(fine[0]))     # (exact: a power of two)
    assert CR.refusal(65, res=fine, max_range=far) is None
    want = check(emu, "steps", small, [[0.01, 0.02, 0.1], [-3.0, 0.2, 0.0]], 1081, res=fine, max_range=far, w_min=-113.0)
    assert want["stats"][1] > 100
    want = check(emu, "short", pts, poses_of(3), 1081, max_range=5.0)
    assert 0 < want["stats"][1] < want["stats"][0]
