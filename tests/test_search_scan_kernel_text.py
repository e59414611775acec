"""The pfslam_search_scan kernels' own text, run on the CPU (no GPU needed), after the pattern of tests/test_search_kernel_text.py:
tests/search_scan_emu.cpp compiles the three kernels cut out of csrc/pfslam_search_scan.hip.inc behind the unchanged text of
csrc/pfslam_search.hip.inc (k_search_ends, k_search_score, k_search_result as the library runs them) and what that reuses, behind the
SIMT shim, as a stand-alone program with -ffp-contract=off like the library, under AddressSanitizer and UBSan, every buffer at exactly
the size pfslam_search_scan requests.  Pose, info, the point count and the whole volume must be the restatement's
(tests/search_scan_ref.py: brute force over all points), bit for bit and integer for integer -- which also shows that the splat's
radius loses nothing, that no index leaves the field and that a word's other half survives a compare-and-swap.  What it cannot show is
the GPU's arithmetic, its memory model and real contention: tests/test_gpu_search_scan.py does."""

import numpy as np
import pytest

import kernel_text as KT
import register_ref as R
import search_ref as S
import search_scan_ref as SS

REF_POSE = np.array([0.5, 0.3, 0.1], np.float32)       # where the reference scan is cast from
POSE = (0.58, 0.24, 0.125)                             # where the searched scan is cast from
CENTRE = np.array([0.6, 0.22, 0.13], np.float32)       # 0.02 m / 0.005 rad off it
# (beams, options): windows 1x1x1 and 5x5x3, a 71-wide row at stride 3 (a partial second wave), 1 / 65 / 1081 beams
CASES = [(1, dict(half_x=0, half_y=0, half_theta=0)),
         (65, dict(half_x=2, half_y=2, half_theta=1)),
         (65, dict(half_x=35, half_y=1, half_theta=0, stride=3)),
         (65, dict(half_x=0, half_y=0, half_theta=0)),
         (1081, dict(half_x=2, half_y=2, half_theta=1)),
         (1081, dict(half_x=0, half_y=0, half_theta=0, max_dist=0.5))]


@pytest.fixture(scope="module")
def scans(pkg):
    _, segs, _ = R.planar_tree(4000, seed=1)
    return pkg.synth.make_scan(segs, tuple(REF_POSE), seed=7), pkg.synth.make_scan(segs, POSE, seed=8)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return KT.build(tmp_path_factory, "search_scan", ("search_derive", "k_search_ends", "k_search_score", "k_search_result", "k_scan_points", "k_scan_fill", "k_scan_splat"), ("PF_LIDAR_RANGE", "PF_SVD_EPSILON"))


def run_emu(emu, tag, ref_scan, ref_pose, scan, centre, opts, res=0.025):
    d, exe = emu
    ref_scan, scan = np.ascontiguousarray(ref_scan, np.float32), np.ascontiguousarray(scan, np.float32)
    o = dict(S.DEFAULTS)
    o.update(opts)
    fin, fout = str(d / ("in_%s.bin" % tag)), str(d / ("out_%s.bin" % tag))
    with open(fin, "wb") as f:
        f.write(np.array([len(scan), 0, o["half_x"], o["half_y"], o["half_theta"], o["stride"], 0, 0], np.int32).tobytes())
        f.write(np.array([centre[0], centre[1], centre[2], o["step_theta"], o["max_dist"], res, ref_pose[0], ref_pose[1], ref_pose[2], 0, 0, 0], np.float32).tobytes())
        f.write(ref_scan.tobytes())
        f.write(scan.tobytes())
    KT.run(exe, fin, fout)
    raw = np.fromfile(fout, np.int32)
    out = raw[:12].view(np.float32).copy()
    assert out[3] == 0 and out[11] == 0
    out[11] = np.float32(raw[14])                       # info[7]: the point count, as the library puts it there
    shape = (2 * o["half_theta"] + 1, 2 * o["half_y"] + 1, 2 * o["half_x"] + 1)
    got = S.result_dict(out[0:3].copy(), out[4:12].copy(), raw[16:].reshape(shape))
    got["box"], got["points"], got["R"] = (int(raw[12]), int(raw[13])), int(raw[14]), int(raw[15])
    return got


def check(emu, tag, ref_scan, ref_pose, scan, centre, opts):
    got = run_emu(emu, tag, ref_scan, ref_pose, scan, centre, opts)
    want = SS.search(ref_scan, ref_pose, scan, centre, **opts)
    assert S.same_result(got, want) is None, S.same_result(got, want)
    assert got["points"] == want["points"] and got["R"] == SS.radius(0.025, dict(S.DEFAULTS, **opts)["max_dist"])
    return got, want


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-%dx%dx%d-s%d-md%g" % (c[0], 2 * c[1]["half_x"] + 1, 2 * c[1]["half_y"] + 1, 2 * c[1]["half_theta"] + 1,
                                                                               c[1].get("stride", 1), c[1].get("max_dist", 0.2)))
def test_the_kernel_text_on_the_cpu_equals_the_restatement(emu, scans, case):
    nb, opts = case
    ref, scan = (np.resize(s, nb) if nb != 1081 else s for s in scans)
    got, want = check(emu, "c_%d_%d_%d_%g" % (nb, opts["half_x"], opts.get("stride", 1), opts.get("max_dist", 0.2)), ref, REF_POSE, scan, CENTRE, opts)
    assert want["status"] == 0 and want["beams"] >= 1 and want["points"] >= 1
    print("%s: winner %d of %d, score %d, qcap %d, %d beams, %d points, box %d x %d cells" % (case, want["index"], want["candidates"], want["score"], want["qcap"],
                                                                                            want["beams"], want["points"], got["box"][0], got["box"][1]))
    assert nb == 1 or (want["scores"] < want["qcap"] * want["beams"]).any(), "every candidate is saturated: the case shows nothing"


def test_qcap_of_1_and_of_65535(emu, scans):
    ref, scan = scans[0][:65], scans[1][:65]
    got, _ = check(emu, "q1", ref, REF_POSE, scan, CENTRE, dict(half_x=3, half_y=3, half_theta=1, max_dist=0.0045))
    assert got["qcap"] == 1 and got["R"] == 3 and got["scores"].max() <= 65 and got["scores"].min() < got["beams"]
    got, _ = check(emu, "q65535", ref, REF_POSE, scan, CENTRE, dict(half_x=2, half_y=2, half_theta=1, max_dist=1.59999))
    assert got["qcap"] == 65535 and got["R"] == 66 and got["scores"].max() > 65535 and (got["scores"] % 65535 != 0).any()


def test_no_point_one_point_and_a_reference_pose_30_m_away(emu, scans):
    """With no point every cell is qcap, the call succeeds and the winner is the ordinary one: candidate 0."""
    ref, scan = scans[0][:65], scans[1][:65]
    opts = dict(half_x=2, half_y=2, half_theta=1)
    got, _ = check(emu, "nopoint", np.full(65, 1000.0, np.float32), REF_POSE, scan, CENTRE, opts)
    assert got["points"] == 0 and got["status"] == 0 and got["index"] == 0 and (got["scores"] == 1024 * got["beams"]).all()
    one = np.full(65, 1000.0, np.float32)
    one[32] = ref[32]
    got, _ = check(emu, "onepoint", one, REF_POSE, scan, CENTRE, opts)
    assert got["points"] == 1 and (got["scores"] <= 1024 * got["beams"]).all()
    # the one point among the searched scan's own end points: the beams that end near it score below saturation
    got, _ = check(emu, "onepoint_same", one, REF_POSE, scans[0][:65], REF_POSE, opts)
    assert got["points"] == 1 and got["score"] < 1024 * got["beams"]
    away = REF_POSE + np.array([30.0, 0.0, 0.0], np.float32)
    got, _ = check(emu, "away", ref, away, scan, CENTRE, opts)
    assert got["points"] == 65 and got["index"] == 0 and (got["scores"] == 1024 * got["beams"]).all()
    # the searched scan without an in-range beam: status 2 whatever the field
    got, _ = check(emu, "status2", ref, REF_POSE, np.full(65, 1000.0, np.float32), CENTRE, opts)
    assert got["status"] == 2 and got["index"] == -1 and got["points"] == 65 and (got["scores"] == S.NONE).all()


def test_a_neighbourhood_that_straddles_the_box_s_corner(emu):
    """One searched beam: the box is its end-point cell grown by the window.  Reference points sit around each of the box's corners, so
    that their neighbourhoods (their own cells lie 4 cells outside the corner in both coordinates) are clipped in x and y, and last 10 cells
    beside it, where only the neighbourhood's edge column reaches the box and saturates."""
    scan = np.full(65, 1000.0, np.float32)
    scan[32] = 2.0
    centre = np.array([0.0, 0.0, 0.0], np.float32)
    opts = dict(half_x=3, half_y=2, half_theta=0)
    ref = np.full(65, 1000.0, np.float32)
    ref[30:35] = 2.0
    hits = 0
    for n, off in enumerate(((0.175, 0.15), (-0.175, 0.15), (0.175, -0.15), (-0.175, -0.15), (0.325, 0.0))):
        got, want = check(emu, "corner%d" % n, ref, np.array([off[0], off[1], 0.0], np.float32), scan, centre, opts)
        assert got["box"] == (7, 5) and got["beams"] == 1 and got["points"] == 5
        hits += int((want["scores"] < 1024).any())
        assert (want["scores"] == 1024).any(), "the neighbourhoods cover the whole box: nothing is clipped"
    assert hits == 4, "the reference points do not reach into the box"


def test_all_beams_at_range_0_1_fall_into_a_handful_of_cells(emu, scans):
    """1081 points within 0.1 m of the reference pose: every point's neighbourhood covers the same cells -- the most contended words."""
    near = np.full(1081, 0.1, np.float32)
    got, want = check(emu, "near", near, REF_POSE, near, CENTRE, dict(half_x=2, half_y=2, half_theta=1))
    assert got["points"] == 1081 and got["beams"] == 1081 and got["box"][0] <= 16 and got["box"][1] <= 16
    assert want["score"] < 1024 * 1081 // 4


def test_a_centre_26_km_out_with_a_box_more_than_2048_cells_wide(emu, scans):
    """Just inside +-2^20 cells: a cell index times the box width passes 2^31 there.  The reference scan is taken 0.05 m from the centre, so
    its points fall into the box and the float spacing out there (2 mm) decides the q."""
    ref, scan = scans[0][:65], scans[1][:65]
    centre = np.array([0.6, 26000.0, 0.13], np.float32)
    ref_pose = np.array([0.55, 26000.0, 0.125], np.float32)
    got, want = check(emu, "26km", ref, ref_pose, scan, centre, dict(half_x=17, half_y=1, half_theta=0, stride=64))
    assert got["beams"] == 65 and got["box"][0] > 2048 and got["points"] == 65
    assert (want["scores"] < 1024 * 65).any() and (want["scores"] == 1024 * 65).any()
