"""The pfslam_search_wide kernels' own text, run on the CPU (no GPU needed): tests/search_wide_emu.cpp compiles the four kernels cut out of
csrc/pfslam_search_wide.hip.inc -- behind the text of csrc/pfslam_search.hip.inc (k_search_ends, k_search_field, k_search_result, launched
as they are) and what that text reuses, none of it changed -- behind the SIMT shim (tests/simt_shim.h) as a stand-alone program with
-ffp-contract=off like the library, under AddressSanitizer and UBSan, every buffer at exactly the size pfslam_search_wide requests.  The
winner and the info must be the restatement's (tests/search_ref.py: the full volume's smallest score, the lowest k among equal ones), bit
for bit -- which also shows that no index leaves a field level, the end-point list or a frontier buffer, whatever the frontier's size.
What it cannot show is the GPU's arithmetic and memory model: tests/test_gpu_search_wide.py does."""

import numpy as np
import pytest

import kernel_text as KT
from kernel_text import device_arrays
import register_ref as R
import search_ref as S
import search_wide_ref as Wd

CENTRE = np.array([0.6, 0.22, 0.13], np.float32)     # 0.10 m / 0.03 rad off the pose the scan was cast from
ROOM = 1 << 22                                       # the library's frontier
# (map, beams, options, frontier nodes): 1x1x1 (top level 0), 5x3x1 (smaller than one top block), 71x9x3 at stride 3 (two top blocks a
# heading, partial edge blocks), 33x33x3 with a frontier of 64 nodes (many batches), and a frontier of 4: one node a batch
CASES = [("p4000", 1, dict(half_x=0, half_y=0, half_theta=0), ROOM),
         ("p4000", 65, dict(half_x=2, half_y=1, half_theta=0), ROOM),
         ("p4000", 65, dict(half_x=35, half_y=4, half_theta=1, stride=3), ROOM),
         ("p4000", 65, dict(half_x=16, half_y=16, half_theta=1), 64),
         ("np300", 65, dict(half_x=4, half_y=2, half_theta=1, max_dist=0.5), 4),
         ("grown4500", 1081, dict(half_x=2, half_y=2, half_theta=1, step_theta=0.05), ROOM)]


@pytest.fixture(scope="module")
def maps(pkg):
    p4000, segs, _ = R.planar_tree(4000, seed=1)
    grown, _ = R.grown_tree(4000, 500, seed=1)
    trees = {"p4000": p4000, "np300": R.nonplanar_tree(300), "grown4500": grown}
    return trees, {k: S.Field(t) for k, t in trees.items()}, pkg.synth.make_scan(segs, (0.5, 0.3, 0.1), seed=7)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return KT.build(tmp_path_factory, "search_wide", ("search_derive", "k_search_ends", "k_search_field", "k_search_result", "k_wide_pyramid", "k_wide_top", "k_wide_score",
                                                     "k_wide_expand", "kd_nearest_exact"), ("PF_LIDAR_RANGE", "PF_SVD_EPSILON"))


def run_emu(emu, tag, tree, scan, centre, opts, room=ROOM, res=0.025):
    d, exe = emu
    hot, z, parent, w, planar = device_arrays(tree)
    scan = np.ascontiguousarray(scan, np.float32)
    o = dict(S.DEFAULTS)
    o.update(opts)
    fin, fout = str(d / ("in_%s.bin" % tag)), str(d / ("out_%s.bin" % tag))
    with open(fin, "wb") as f:
        f.write(np.array([len(tree), planar, len(scan), 0, o["half_x"], o["half_y"], o["half_theta"], o["stride"], room, 0], np.int32).tobytes())
        f.write(np.array([centre[0], centre[1], centre[2], o["step_theta"], o["max_dist"], res, 0, 0], np.float32).tobytes())
        for a in (hot, z, parent, w, scan):
            f.write(np.ascontiguousarray(a).tobytes())
    KT.run(exe, fin, fout)
    raw = np.fromfile(fout, np.uint8)
    out = raw[:48].view(np.float32)
    stats = raw[48:112].view(np.int64)
    assert out[3] == 0 and out[11] == 0 and len(raw) == 112
    got = S.result_dict(out[0:3].copy(), out[4:12].copy())
    got["stats"] = stats
    return got


def assert_winner(got, want, what=""):
    assert S.same_result(got, want, volume=False) is None, "%s: %s" % (what, S.same_result(got, want, volume=False))
    st = got["stats"]
    assert st[0] == want["index"] and st[1] == want["candidates"] == want["scores"].size and st[7] == 0
    assert st[3] <= st[1] and 0 <= st[4] <= Wd.MAX_LEVEL


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%dx%dx%d-s%d-room%d" % (c[0], c[1], 2 * c[2]["half_x"] + 1, 2 * c[2]["half_y"] + 1,
                                                                                   2 * c[2]["half_theta"] + 1, c[2].get("stride", 1), c[3]))
def test_the_kernel_text_on_the_cpu_picks_the_restatement_s_winner(emu, maps, case):
    trees, fields, scan1081 = maps
    name, nb, opts, room = case
    scan = np.resize(scan1081, nb) if nb != 1081 else scan1081
    got = run_emu(emu, "c_%s_%d_%d_%d" % (name, nb, opts["half_x"], room), trees[name], scan, CENTRE, opts, room)
    want = S.search(fields[name], scan, CENTRE, **opts)
    assert_winner(got, want, str(case))
    st = got["stats"]
    nx, ny = 2 * opts["half_x"] + 1, 2 * opts["half_y"] + 1
    assert want["status"] == 0 and st[4] == Wd.top_level(nx, ny) and st[6] == Wd.Wide(S.Search(fields[name], scan, CENTRE, **opts)).cells()
    print("%s: winner %d of %d, score %d; top level %d, %d nodes bounded, %d candidates scored, %d batches, box of %d cells"
          % (case, st[0], st[1], want["score"], st[4], st[2], st[3], st[5], st[6]))
    if room < ROOM:
        assert st[5] > st[4] + 1, "the small frontier did not cut a level into batches"
    else:
        assert st[5] <= st[4] + 1
    if nx * ny > 1 and (want["scores"] < want["qcap"] * want["beams"]).any() and nb > 1:
        assert st[3] < st[1] or st[1] <= 4, "nothing was pruned"


def test_a_constructed_tie_goes_to_the_lowest_k(emu, maps):
    trees, fields, _ = maps
    scan, centre, opts = Wd.tie_case(trees["p4000"], fields["p4000"])
    want = S.search(fields["p4000"], scan, centre, **opts)
    flat = want["scores"].ravel()
    assert want["qcap"] == 1 and flat.min() == 0 and (flat == 0).sum() >= 2 and want["index"] == np.flatnonzero(flat == 0)[0]
    for room in (ROOM, 16):
        assert_winner(run_emu(emu, "tie%d" % room, trees["p4000"], scan, centre, opts, room), want, "tie, frontier %d" % room)


def test_status_2_and_a_heading_without_in_range_beams(emu, maps):
    """A scan of ranges 1000: every heading is skipped (status 2, the centre, k = -1).  Then one beam whose range puts it inside +-20 m at
    one heading only: the nodes of the other headings are dropped and take no part."""
    trees, fields, _ = maps
    opts = dict(half_x=1, half_y=1, half_theta=1, step_theta=0.3)
    far = np.full(65, 1000.0, np.float32)
    got = run_emu(emu, "s2", trees["p4000"], far, CENTRE, opts)
    want = S.search(fields["p4000"], far, CENTRE, **opts)
    assert_winner(got, want, "status 2")
    assert got["status"] == 2 and got["stats"][0] == -1 and (R.bits(got["pose"]) == R.bits(CENTRE)).all() and got["stats"][6] == 0
    one = far.copy()
    one[0] = 28.0
    c0 = np.array([0.6, 0.22, 0.0], np.float32)           # (heading 1 of 3 looks along the diagonal exactly)
    want = S.search(fields["p4000"], one, c0, **opts)
    live = [(want["scores"][a] != S.NONE).all() for a in range(3)]
    assert any(live) and not all(live), live
    got = run_emu(emu, "one", trees["p4000"], one, c0, opts)
    assert_winner(got, want, "one heading")
    assert got["status"] == 0 and got["beams"] == 1


def test_a_box_26_km_out_that_is_more_than_2048_cells_wide_and_a_centre_beyond_2_to_the_20_cells(emu, maps):
    """The two cases of tests/test_search_kernel_text.py: a cell index times the box width passes 2^31 (UBSan holds the kernels to
    indexing every level relative to the box); and no end point has a cell, so every lookup is a spare cell: all candidates tie at
    qcap * beams and k = 0 wins."""
    trees, fields, scan = maps
    centre = np.array([0.6, 26000.0, 0.13], np.float32)
    opts = dict(half_x=17, half_y=1, half_theta=0, stride=64)
    got = run_emu(emu, "26km", trees["p4000"], scan[:65], centre, opts)
    want = S.search(fields["p4000"], scan[:65], centre, **opts)
    assert_winner(got, want, "26 km")
    assert got["beams"] == 65 and got["index"] == 0 and got["score"] == 1024 * 65 and got["stats"][6] > 2048 * 128
    centre = np.array([30000.0, 0.22, 0.13], np.float32)
    opts = dict(half_x=1, half_y=1, half_theta=0)
    got = run_emu(emu, "far", trees["p4000"], scan[:65], centre, opts)
    want = S.search(fields["p4000"], scan[:65], centre, **opts)
    assert_winner(got, want, "far")
    assert got["status"] == 0 and got["index"] == 0 and got["score"] == got["qcap"] * got["beams"] and got["stats"][6] == 0
