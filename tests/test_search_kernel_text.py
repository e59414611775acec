"""The pfslam_search kernels' own text, run on the CPU (no GPU needed): tests/search_emu.cpp compiles the four kernels cut out of
csrc/pfslam_search.hip.inc -- behind the text of csrc/pfslam_register.hip.inc (pf::kd_nearest_exact), csrc/pf_math.h, csrc/kd_device.h and
the pieces of csrc/pfslam_stages.hip.inc that text needs, none of them changed -- behind a small SIMT shim (a thread per GPU thread,
barriers for __syncthreads and the wave shuffles, the workgroups one after the other, every buffer at exactly the size pfslam_search
requests) as a stand-alone program with -ffp-contract=off like the library, under AddressSanitizer and UBSan.  The winner, the info
and the full score volume must be the restatement's (tests/search_ref.py), bit for bit and integer for integer -- which also shows
that no index leaves the field, the end-point list or the volume.  What it cannot show is the GPU's arithmetic and memory model:
tests/test_gpu_search.py does."""

import numpy as np
import pytest

import kernel_text as KT
from kernel_text import device_arrays
import register_ref as R
import search_ref as S

CENTRE = np.array([0.6, 0.22, 0.13], np.float32)     # 0.10 m / 0.03 rad off the pose the scan was cast from
# (map, beams, options): windows 1x1x1, 3x1x1 and 5x5x3, a 70-wide row (a partial second wave), stride 1 and 3
CASES = [("p4000", 1, dict(half_x=0, half_y=0, half_theta=0)),
         ("p4000", 1, dict(half_x=1, half_y=0, half_theta=0)),
         ("p4000", 65, dict(half_x=2, half_y=2, half_theta=1)),
         ("p4000", 65, dict(half_x=35, half_y=1, half_theta=0, stride=3)),
         ("p4000", 65, dict(half_x=35, half_y=0, half_theta=1, step_theta=0.03, max_dist=0.1)),
         ("p4000", 1081, dict(half_x=2, half_y=2, half_theta=1)),
         ("np300", 1081, dict(half_x=2, half_y=2, half_theta=1, stride=3, max_dist=0.5)),
         ("grown4500", 65, dict(half_x=2, half_y=2, half_theta=1, step_theta=0.05))]


@pytest.fixture(scope="module")
def maps(pkg):
    p4000, segs, _ = R.planar_tree(4000, seed=1)
    grown, _ = R.grown_tree(4000, 500, seed=1)
    trees = {"p4000": p4000, "np300": R.nonplanar_tree(300), "grown4500": grown}
    return trees, {k: S.Field(t) for k, t in trees.items()}, pkg.synth.make_scan(segs, (0.5, 0.3, 0.1), seed=7)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return KT.build(tmp_path_factory, "search", ("search_derive", "k_search_ends", "k_search_field", "k_search_score", "k_search_result", "kd_nearest_exact"), ("PF_LIDAR_RANGE", "PF_SVD_EPSILON"))


def run_emu(emu, tag, tree, scan, centre, opts, res=0.025):
    d, exe = emu
    hot, z, parent, w, planar = device_arrays(tree)
    scan = np.ascontiguousarray(scan, np.float32)
    o = dict(S.DEFAULTS)
    o.update(opts)
    fin, fout = str(d / ("in_%s.bin" % tag)), str(d / ("out_%s.bin" % tag))
    with open(fin, "wb") as f:
        f.write(np.array([len(tree), planar, len(scan), 0, o["half_x"], o["half_y"], o["half_theta"], o["stride"]], np.int32).tobytes())
        f.write(np.array([centre[0], centre[1], centre[2], o["step_theta"], o["max_dist"], res, 0, 0], np.float32).tobytes())
        for a in (hot, z, parent, w, scan):
            f.write(np.ascontiguousarray(a).tobytes())
    KT.run(exe, fin, fout)
    raw = np.fromfile(fout, np.int32)
    out = raw[:12].view(np.float32)
    assert out[3] == 0 and out[11] == 0
    shape = (2 * o["half_theta"] + 1, 2 * o["half_y"] + 1, 2 * o["half_x"] + 1)
    vol = raw[16:].reshape(shape)
    got = S.result_dict(out[0:3].copy(), out[4:12].copy(), vol)
    got["box"] = (int(raw[12]), int(raw[13]))
    return got


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%dx%dx%d-s%d" % (c[0], c[1], 2 * c[2]["half_x"] + 1, 2 * c[2]["half_y"] + 1,
                                                                            2 * c[2]["half_theta"] + 1, c[2].get("stride", 1)))
def test_the_kernel_text_on_the_cpu_equals_the_restatement(emu, maps, case):
    trees, fields, scan1081 = maps
    name, nb, opts = case
    scan = np.resize(scan1081, nb) if nb != 1081 else scan1081
    got = run_emu(emu, "c_%s_%d_%d_%d" % (name, nb, opts["half_x"], opts.get("stride", 1)), trees[name], scan, CENTRE, opts)
    want = S.search(fields[name], scan, CENTRE, **opts)
    assert S.same_result(got, want) is None, S.same_result(got, want)
    assert want["status"] == 0 and want["beams"] >= 1
    print("%s: winner %d of %d, score %d, qcap %d, %d beams, box %d x %d cells" % (case, want["index"], want["candidates"], want["score"], want["qcap"],
                                                                                 want["beams"], got["box"][0], got["box"][1]))
    assert (want["scores"] < want["qcap"] * want["beams"]).any() or nb == 1, "every candidate is saturated: the case shows nothing"


def test_status_2_and_a_heading_without_in_range_beams(emu, maps):
    """A scan of ranges 1000: every heading is skipped (status 2, the centre, k = -1, a volume of INT32_MAX).  Then one beam whose range
    puts it inside +-20 m at the first heading only: the other headings score INT32_MAX and take no part."""
    trees, fields, _ = maps
    opts = dict(half_x=1, half_y=1, half_theta=1, step_theta=0.3)
    far = np.full(65, 1000.0, np.float32)
    got = run_emu(emu, "s2", trees["p4000"], far, CENTRE, opts)
    want = S.search(fields["p4000"], far, CENTRE, **opts)
    assert S.same_result(got, want) is None, S.same_result(got, want)
    assert got["status"] == 2 and got["index"] == -1 and (got["scores"] == S.NONE).all() and (R.bits(got["pose"]) == R.bits(CENTRE)).all()
    # beam 0 looks along -135 degrees + theta: at 28 m it is inside the +-20 m square only within 0.6 degrees of the diagonal
    one = far.copy()
    one[0] = 28.0
    c0 = np.array([0.6, 0.22, 0.0], np.float32)           # (heading 1 of 3 looks along the diagonal exactly)
    want = S.search(fields["p4000"], one, c0, **opts)
    live = [(want["scores"][a] != S.NONE).all() for a in range(3)]
    assert any(live) and not all(live), live
    got = run_emu(emu, "one", trees["p4000"], one, c0, opts)
    assert S.same_result(got, want) is None, S.same_result(got, want)
    assert got["status"] == 0 and got["beams"] == 1


def test_qcap_65535_and_a_box_26_km_out_that_is_more_than_2048_cells_wide(emu, maps):
    """The top of the uint16 range.  Then a centre just inside +-2^20 cells with a window that grows the box past 2048 cells: a cell index
    times the box width passes 2^31 there, so UBSan holds the kernels to indexing the field relative to the box."""
    trees, fields, scan = maps
    opts = dict(half_x=2, half_y=2, half_theta=1, max_dist=1.59999)
    centre = np.array([3.0, 2.0, 0.13], np.float32)
    got = run_emu(emu, "top", trees["p4000"], scan[:65], centre, opts)
    want = S.search(fields["p4000"], scan[:65], centre, **opts)
    assert S.same_result(got, want) is None, S.same_result(got, want)
    assert got["qcap"] == 65535 and got["scores"].max() > 65535 and (got["scores"] % 65535 != 0).any()
    centre = np.array([0.6, 26000.0, 0.13], np.float32)
    opts = dict(half_x=17, half_y=1, half_theta=0, stride=64)
    got = run_emu(emu, "26km", trees["p4000"], scan[:65], centre, opts)
    want = S.search(fields["p4000"], scan[:65], centre, **opts)
    assert S.same_result(got, want) is None, S.same_result(got, want)
    assert got["beams"] == 65 and got["box"][0] > 2048 and (got["scores"] == 1024 * 65).all()


def test_a_centre_beyond_2_to_the_20_cells_saturates_every_beam(emu, maps):
    trees, fields, scan = maps
    centre = np.array([30000.0, 0.22, 0.13], np.float32)
    opts = dict(half_x=1, half_y=1, half_theta=0)
    got = run_emu(emu, "far", trees["p4000"], scan[:65], centre, opts)
    want = S.search(fields["p4000"], scan[:65], centre, **opts)
    assert S.same_result(got, want) is None, S.same_result(got, want)
    assert got["status"] == 0 and got["index"] == 0 and got["score"] == got["qcap"] * got["beams"] and got["box"] == (0, 0)
