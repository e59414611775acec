"""The pfslam_search_best kernels' own text, run on the CPU (no GPU needed): tests/search_best_emu.cpp compiles the five kernels cut out of
csrc/pfslam_search_best.hip.inc -- behind the text of csrc/pfslam_search_wide.hip.inc and csrc/pfslam_search.hip.inc (k_search_ends,
k_search_field, k_wide_pyramid, k_wide_top, launched as they are) and what that text reuses, none of it changed -- behind the SIMT shim
(tests/simt_shim.h) as a stand-alone program with -ffp-contract=off like the library, under AddressSanitizer and UBSan, every buffer at
exactly the size pfslam_search_best requests.  The rows must be the restatement's (tests/search_best_ref.py: the full volume cut into
cells, the smallest key of each, the `count` smallest of those), bit for bit -- which also shows that no index leaves the table, the
list, a field level or a frontier buffer, whatever the frontier's size.  The cases are those of tests/test_search_wide_kernel_text.py,
each with count 1, 5 and 64.  What it cannot show is the GPU's arithmetic and memory model: tests/test_gpu_search_best.py does."""

import numpy as np
import pytest

import kernel_text as KT
from kernel_text import device_arrays
import register_ref as R
import search_best_ref as Bs
import search_ref as S
import search_wide_ref as Wd
from test_search_wide_kernel_text import CASES, CENTRE, ROOM

# (tile_log2, group_theta) per case of CASES: one cell; two tiles; partial tiles at stride 3; tiles of one candidate under a frontier of
# 64 nodes; groups larger than na under a frontier of 4; the defaults
CELLS = [(3, 8), (2, 1), (2, 2), (0, 1), (1, 8), (3, 8)]


@pytest.fixture(scope="module")
def maps(pkg):
    p4000, segs, _ = R.planar_tree(4000, seed=1)
    grown, _ = R.grown_tree(4000, 500, seed=1)
    trees = {"p4000": p4000, "np300": R.nonplanar_tree(300), "grown4500": grown}
    return trees, {k: S.Field(t) for k, t in trees.items()}, pkg.synth.make_scan(segs, (0.5, 0.3, 0.1), seed=7), {}


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return KT.build(tmp_path_factory, "search_best", ("search_derive", "k_search_ends", "k_search_field", "k_wide_pyramid", "k_wide_top", "k_best_score", "k_best_thr",
                                                     "k_best_expand", "k_best_compact", "k_best_rows", "kd_nearest_exact"), ("PF_LIDAR_RANGE", "PF_SVD_EPSILON"))


def run_emu(emu, tag, tree, scan, centre, opts, count, ls, g, room=ROOM, res=0.025):
    d, exe = emu
    hot, z, parent, w, planar = device_arrays(tree)
    scan = np.ascontiguousarray(scan, np.float32)
    o = dict(S.DEFAULTS)
    o.update(opts)
    fin, fout = str(d / ("in_%s.bin" % tag)), str(d / ("out_%s.bin" % tag))
    with open(fin, "wb") as f:
        f.write(np.array([len(tree), planar, len(scan), 0, o["half_x"], o["half_y"], o["half_theta"], o["stride"], room, count, ls, g], np.int32).tobytes())
        f.write(np.array([centre[0], centre[1], centre[2], o["step_theta"], o["max_dist"], res, 0, 0], np.float32).tobytes())
        for a in (hot, z, parent, w, scan):
            f.write(np.ascontiguousarray(a).tobytes())
    KT.run(exe, fin, fout)
    raw = np.fromfile(fout, np.uint8)
    found = int(raw[:8].view(np.int64)[0])
    assert 0 <= found <= count and len(raw) == 72 + found * (8 + 48)
    rows = raw[72 + 8 * found:].view(np.float32).reshape(found, 12)
    assert (rows[:, 3] == 0).all() and (rows[:, 11] == 0).all()
    return {"found": found, "stats": raw[8:72].view(np.int64), "index": raw[72:72 + 8 * found].view(np.int64), "poses": rows[:, 0:3].copy(), "info": rows[:, 4:12].copy()}


def wanted(maps, name, scan, centre, opts, count, ls, g):
    """The definition's rows, the volume computed once per window."""
    key = (name, len(scan), tuple(np.asarray(centre).tolist()), tuple(sorted(opts.items())))
    if key not in maps[3]:
        s = S.Search(maps[1][name], scan, centre, **opts)
        maps[3][key] = (s, s.volume())
    s, vol = maps[3][key]
    b = Bs.Best(s, ls, g)
    return s, vol, b, Bs.result_dict(s, b.rows(vol, count), None, b.cells)


def assert_rows(got, want, s, what=""):
    assert Bs.same_rows(got, want) is None, "%s: %s" % (what, Bs.same_rows(got, want))
    st = got["stats"]
    assert st[0] == (want["index"][0] if want["found"] else -1) and st[1] == s.cand and st[7] == want["cells"], (what, st.tolist())
    assert st[3] <= st[1] and 0 <= st[4] <= Wd.MAX_LEVEL


@pytest.mark.parametrize("count", [1, 5, 64])
@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda n: "%s-%d-%dx%dx%d-s%d-room%d" % (
    CASES[n][0], CASES[n][1], 2 * CASES[n][2]["half_x"] + 1, 2 * CASES[n][2]["half_y"] + 1, 2 * CASES[n][2]["half_theta"] + 1, CASES[n][2].get("stride", 1), CASES[n][3]))
def test_the_kernel_text_on_the_cpu_returns_the_restatement_s_rows(emu, maps, case, count):
    trees, fields, scan1081, _ = maps
    name, nb, opts, room = CASES[case]
    ls, g = CELLS[case]
    scan = np.resize(scan1081, nb) if nb != 1081 else scan1081
    got = run_emu(emu, "c%d_%d" % (case, count), trees[name], scan, CENTRE, opts, count, ls, g, room)
    s, vol, b, want = wanted(maps, name, scan, CENTRE, opts, count, ls, g)
    assert_rows(got, want, s, "%r count %d" % (CASES[case], count))
    st = got["stats"]
    assert want["found"] == min(count, b.cells) and st[4] == Wd.top_level(s.nx, s.ny) and st[6] == Wd.Wide(s).cells()
    assert (got["index"][0], want["info"][0][4]) == (s.pick(vol)[1], s.pick(vol)[0])          # row 0 is the single winner
    print("%s, tiles 2^%d, groups of %d, %d rows of %d cells: %d nodes bounded, %d of %d candidates scored, %d batches"
          % (CASES[case], ls, g, got["found"], st[7], st[2], st[3], st[1], st[5]))
    if room < ROOM:
        assert st[5] > st[4] + 1, "the small frontier did not cut a level into batches"
    else:
        assert st[5] <= st[4] + 1


def test_a_constructed_tie_keeps_the_lowest_k_of_every_cell(emu, maps):
    trees, fields, _, _ = maps
    scan, centre, opts = Wd.tie_case(trees["p4000"], fields["p4000"])
    for count, ls, g, room in ((1, 7, 1, ROOM), (8, 2, 1, ROOM), (64, 1, 1, 16)):
        s, vol, b, want = wanted(maps, "p4000", scan, centre, opts, count, ls, g)
        assert s.qcap == 1 and (vol == 0).sum() >= 2
        got = run_emu(emu, "tie%d_%d_%d" % (count, ls, room), trees["p4000"], scan, centre, opts, count, ls, g, room)
        assert_rows(got, want, s, "tie, count %d, tiles 2^%d, frontier %d" % (count, ls, room))
        assert got["index"][0] == np.flatnonzero(vol.ravel() == 0)[0]


def test_status_2_finds_no_row_and_a_heading_without_in_range_beams_has_no_cell(emu, maps):
    trees, fields, _, _ = maps
    opts = dict(half_x=1, half_y=1, half_theta=1, step_theta=0.3)
    far = np.full(65, 1000.0, np.float32)
    got = run_emu(emu, "s2", trees["p4000"], far, CENTRE, opts, 8, 0, 1)
    assert got["found"] == 0 and got["stats"][0] == -1 and got["stats"][6] == 0 and got["stats"][7] == 27
    one = far.copy()
    one[0] = 28.0
    c0 = np.array([0.6, 0.22, 0.0], np.float32)           # (heading 1 of 3 looks along the diagonal exactly)
    s, vol, b, want = wanted(maps, "p4000", one, c0, opts, 64, 0, 1)
    live = [(vol[a] != S.NONE).all() for a in range(3)]
    assert any(live) and not all(live) and want["found"] == 9 * sum(live)
    got = run_emu(emu, "one", trees["p4000"], one, c0, opts, 64, 0, 1)
    assert_rows(got, want, s, "one heading")


def test_a_box_26_km_out_and_a_centre_beyond_2_to_the_20_cells(emu, maps):
    """The two cases of tests/test_search_wide_kernel_text.py: a cell index times the box width passes 2^31; and no end point has a cell,
    so every candidate ties and the rows are the cells' lowest k in ascending k."""
    trees, fields, scan, _ = maps
    centre = np.array([0.6, 26000.0, 0.13], np.float32)
    opts = dict(half_x=17, half_y=1, half_theta=0, stride=64)
    s, vol, b, want = wanted(maps, "p4000", scan[:65], centre, opts, 5, 2, 1)
    got = run_emu(emu, "26km", trees["p4000"], scan[:65], centre, opts, 5, 2, 1)
    assert_rows(got, want, s, "26 km")
    assert got["found"] == 5 and got["index"].tolist() == [0, 4, 8, 12, 16] and got["stats"][6] > 2048 * 128
    centre = np.array([30000.0, 0.22, 0.13], np.float32)
    opts = dict(half_x=2, half_y=1, half_theta=0)
    s, vol, b, want = wanted(maps, "p4000", scan[:65], centre, opts, 8, 1, 1)
    got = run_emu(emu, "far", trees["p4000"], scan[:65], centre, opts, 8, 1, 1)
    assert_rows(got, want, s, "far")
    assert got["found"] == 6 and got["index"].tolist() == [0, 2, 4, 10, 12, 14] and got["stats"][6] == 0
