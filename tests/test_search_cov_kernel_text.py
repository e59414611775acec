"""The pfslam_search_cov kernels' own text, run on the CPU (no GPU needed), after the pattern of tests/test_search_scan_kernel_text.py:
tests/search_cov_emu.cpp compiles the kernels cut out of csrc/pfslam_search_cov.hip.inc behind the unchanged text of pfslam_estimate's
device functions (csrc/pfslam_stages.hip.inc), of csrc/pfslam_search.hip.inc and of csrc/pfslam_search_scan.hip.inc, and pf::exp2m of
csrc/pf_math.h, behind the SIMT shim, as a stand-alone program with -ffp-contract=off like the library, under AddressSanitizer and UBSan,
every buffer at exactly the size the entry point requests.  The call is pfslam_search_scan_cov's.  Pose, info and the volume must be the
search's, and cov_out the restatement's (tests/search_cov_ref.py), bit for bit -- which also shows that the stepped index (a, j, i) is
the divided one, that no index leaves a buffer and that every thread reaches every barrier.  What it cannot show is the GPU's arithmetic
and memory model: tests/test_gpu_search_cov.py does."""

import numpy as np
import pytest

import kernel_text as KT
import register_ref as R
import search_cov_ref as SC
import search_ref as S
import search_scan_ref as SS

REF_POSE = np.array([0.5, 0.3, 0.1], np.float32)       # where the reference scan is cast from
POSE = (0.58, 0.24, 0.125)                             # where the searched scan is cast from
CENTRE = np.array([0.6, 0.22, 0.13], np.float32)       # 0.02 m / 0.005 rad off it
# (beams, options, sigma): 1 candidate; 75; 4095 (one tile, one short of full); 4097 (a second tile of one element); 14 553 (tile edges
# inside rows and headings); 1 / 65 / 1081 beams
CASES = [(1, dict(half_x=0, half_y=0, half_theta=0), 0.2),
         (65, dict(half_x=0, half_y=0, half_theta=0), 0.2),
         (65, dict(half_x=2, half_y=2, half_theta=1), 0.2),
         (1081, dict(half_x=2, half_y=2, half_theta=1), 0.2),
         (65, dict(half_x=32, half_y=31, half_theta=0), 0.2),
         (65, dict(half_x=120, half_y=8, half_theta=0), 0.2),
         (65, dict(half_x=10, half_y=10, half_theta=16), 0.2),
         (65, dict(half_x=10, half_y=10, half_theta=16), 0.05)]
# the mixed-headings case: one finite beam of 20.5 m lying about 12.7 degrees from the x axis at the centre heading -- in range
# (|wx| < 20) only at the headings that turn it far enough from the axis
MIXED_BEAM, MIXED_ANGLE = 20.5, np.deg2rad(12.7)


def mixed_case(nb=65):
    """(scan, ref_scan, centre = ref_pose, options): the searched scan is that one beam, the reference scan the same beam 0.1 m shorter,
    so that the scores of the headings that take part differ from candidate to candidate."""
    b = nb // 2
    probe = np.full(nb, 1000.0, np.float32)
    probe[b] = 10.0
    t, inr = R.targets(probe, np.zeros(3, np.float32))              # the beam's angle is fixed by its index: where it points at heading 0
    assert inr[b]
    centre = np.array([0.0, 0.0, MIXED_ANGLE - np.arctan2(t[b, 1], t[b, 0])], np.float32)
    scan, ref = np.full(nb, 1000.0, np.float32), np.full(nb, 1000.0, np.float32)
    scan[b], ref[b] = MIXED_BEAM, MIXED_BEAM - 0.1
    return scan, ref, centre, dict(half_x=3, half_y=2, half_theta=8, step_theta=0.01)


@pytest.fixture(scope="module")
def scans(pkg):
    _, segs, _ = R.planar_tree(4000, seed=1)
    return pkg.synth.make_scan(segs, tuple(REF_POSE), seed=7), pkg.synth.make_scan(segs, POSE, seed=8)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return KT.build(tmp_path_factory, "search_cov", ("search_derive", "k_search_ends", "k_search_score", "k_search_result", "k_scan_points", "k_scan_fill", "k_scan_splat", "est_moments",
                                                    "est_centred", "est_finish", "k_cov_moments", "k_cov_centred", "k_cov_final", "k_cov_small"), ("PF_LIDAR_RANGE", "PF_SVD_EPSILON", "PF_SUM_TILE"))


def run_emu(emu, tag, ref_scan, ref_pose, scan, centre, opts, sigma, res=0.025):
    d, exe = emu
    ref_scan, scan = np.ascontiguousarray(ref_scan, np.float32), np.ascontiguousarray(scan, np.float32)
    o = dict(S.DEFAULTS)
    o.update(opts)
    fin, fout = str(d / ("in_%s.bin" % tag)), str(d / ("out_%s.bin" % tag))
    with open(fin, "wb") as f:
        f.write(np.array([len(scan), 0, o["half_x"], o["half_y"], o["half_theta"], o["stride"], 0, 0], np.int32).tobytes())
        f.write(np.array([centre[0], centre[1], centre[2], o["step_theta"], o["max_dist"], res, ref_pose[0], ref_pose[1], ref_pose[2], sigma, 0, 0],
                         np.float32).tobytes())
        f.write(ref_scan.tobytes())
        f.write(scan.tobytes())
    KT.run(exe, fin, fout)
    raw = np.fromfile(fout, np.int32)
    out = raw[:12].view(np.float32).copy()
    assert out[3] == 0 and out[11] == 0
    out[11] = np.float32(raw[14])                       # info[7]: the point count, as the library puts it there
    shape = (2 * o["half_theta"] + 1, 2 * o["half_y"] + 1, 2 * o["half_x"] + 1)
    got = S.result_dict(out[0:3].copy(), out[4:12].copy(), raw[32:].reshape(shape))
    got["points"], got["raw"] = int(raw[14]), raw[16:32].view(np.float32).copy()
    return got


def check(emu, tag, ref_scan, ref_pose, scan, centre, opts, sigma=0.2):
    got = run_emu(emu, tag, ref_scan, ref_pose, scan, centre, opts, sigma)
    want = SC.search_scan_cov(ref_scan, ref_pose, scan, centre, sigma=sigma, **opts)
    assert S.same_result(got, want) is None, S.same_result(got, want)
    assert SC.same_cov(got["raw"], want["raw"]) is None, SC.same_cov(got["raw"], want["raw"])
    return got, want


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-%dx%dx%d-sigma%g" % (c[0], 2 * c[1]["half_x"] + 1, 2 * c[1]["half_y"] + 1, 2 * c[1]["half_theta"] + 1, c[2]))
def test_the_kernel_text_on_the_cpu_equals_the_restatement(emu, scans, case):
    nb, opts, sigma = case
    ref, scan = (np.resize(s, nb) if nb != 1081 else s for s in scans)
    got, want = check(emu, "c_%d_%d_%d_%g" % (nb, opts["half_x"], opts["half_theta"], sigma), ref, REF_POSE, scan, CENTRE, opts, sigma)
    raw = want["raw"]
    print("%s: winner %d of %d, Neff %g, S0 %g, border share %g, sd %g / %g / %g" % (case, want["index"], want["candidates"], raw[9], raw[10], raw[13],
                                                                                   raw[3] ** 0.5, raw[6] ** 0.5, raw[8] ** 0.5))
    assert want["status"] == 0 and raw[10] >= 1 and raw[12] == want["candidates"] and raw[15] == 0
    if want["candidates"] == 1:
        assert raw[9] == 1 and raw[13] == 0 and (raw[3:9] == 0).all() and (R.bits(raw[0:3]) == R.bits(want["pose"])).all()
    elif nb > 1:
        assert raw[9] > 1, "one candidate holds all the weight: the case shows nothing"


def test_status_2_writes_zeros_but_the_candidates_and_the_scale(emu, scans):
    ref = scans[0][:65]
    for tag, opts in (("small", dict(half_x=2, half_y=2, half_theta=1)), ("tiles", dict(half_x=120, half_y=8, half_theta=0))):
        got, _ = check(emu, "status2_" + tag, ref, REF_POSE, np.full(65, 1000.0, np.float32), CENTRE, opts)
        raw = got["raw"]
        assert got["status"] == 2 and (got["scores"] == S.NONE).all()
        assert (raw[[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15]].view(np.int32) == 0).all() and raw[12] == got["scores"].size and raw[14] > 0


def test_a_window_in_which_some_headings_take_part_and_others_do_not(emu, scans):
    scan, ref, centre, opts = mixed_case()
    srch = S.Search(SS.PointField(SS.points_of(ref, centre)), scan, centre, **opts)
    live = np.array([srch.ends(a)[3] > 0 for a in range(srch.na)])
    assert live.any() and not live.all(), "the restatement must have both kinds of heading: %r" % live
    got, want = check(emu, "mixed", ref, centre, scan, centre, opts)
    vol = want["scores"]
    assert (vol[~live] == S.NONE).all() and (vol[live] != S.NONE).all() and want["status"] == 0
    assert 1 <= want["raw"][10] <= live.sum() * 35 and len(np.unique(vol[live])) > 1


def test_qcap_of_1_and_of_65535_with_differences_above_2_to_the_24(emu, scans):
    ref, scan = scans[0][:65], scans[1][:65]
    got, _ = check(emu, "q1", ref, REF_POSE, scan, CENTRE, dict(half_x=3, half_y=3, half_theta=1, max_dist=0.0045))
    assert got["qcap"] == 1 and got["raw"][9] > 1
    # sigma = 50 and stride 64: S - Smin passes 2^24 (the conversion to float rounds) with weights that are neither 0 nor 1
    opts = dict(half_x=2, half_y=2, half_theta=1, max_dist=1.59999, stride=64)
    got, want = check(emu, "q65535", scans[0], REF_POSE, scans[1], CENTRE, opts, sigma=50.0)
    d = want["scores"].astype(np.int64) - want["scores"].min()
    w = SC.weights(want["scores"], int(want["scores"].min()), want["raw"][14])
    big = d > (1 << 24)
    assert got["qcap"] == 65535 and big.any() and (d[big] % 2 == 1).any(), "no difference above 2^24 needs rounding"
    assert ((w[big.ravel()] > 0) & (w[big.ravel()] < 1)).all()
