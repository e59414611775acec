"""pfslam_search_wide without a GPU: the entry point is carried by every layer (this fails on the parent commit), and the method the header
describes is sound as tests/search_wide_ref.py restates it --

  * at every level up to 3, for every block of windows that are no powers of two (edge blocks are partial), the bound LB is <= the
    smallest score search_ref's volume holds in the block; at level 0 it is the score; the block origin's k is the block's lowest;
  * the level-synchronous descent with the rule "drop only if (LB << 32 | k_origin) > the key" returns search_ref's winner, also in a
    constructed tie at qcap 1 with one beam, in the saturated far-centre case (k = 0) and with status 2;
  * a looser rule -- drop on LB >= the best S -- loses that tie's lowest k: the reason equality is kept.

The scans are the first 65 beams of the scenario's scan and the first 33 of synth.make_weird_scan (a zero range and a 1000 m one among them): the restatement looks every touched cell up by
brute force over the map's nodes, and the weird scan's end points share no cells."""
import os
import re

import numpy as np
import pytest

import register_batch_ref as B
import register_ref as R
import search_ref as S
import search_wide_ref as Wd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = {"37x21x3": dict(half_x=18, half_y=10, half_theta=1), "19x11x3-stride3": dict(half_x=9, half_y=5, half_theta=1, stride=3)}
CENTRE = (10.2, -7.85, 0.3)         # 8 and 6 cells off the pose the scenario's scan was cast from


def test_header_binding_classes_hooks_and_library_carry_the_entry_point(pkg):
    """Fails on the parent commit: the entry point does not exist there."""
    src = open(os.path.join(ROOT, "include", "pfslam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+pfslam_search_wide\s*\(\s*pfslam_handle\s*\*", code)
    assert "pfslam_search_wide" in pkg.binding.SYMBOLS
    assert callable(getattr(pkg.PfSlam, "search_wide", None))
    from importlib import import_module
    assert callable(getattr(import_module("gpu-icp-slam_amd.sharded").ShardedSlam, "search_wide", None))
    L = pkg.load()
    assert hasattr(L, "pfslam_search_wide") and hasattr(L, "pfslam_debug_search_frontier")
    hooks = open(os.path.join(ROOT, "gpu-icp-slam_amd", "csrc", "pfslam_testhooks.h")).read()
    assert "pfslam_debug_search_frontier" in hooks and "pfslam_debug_search_frontier" not in src
    spec = src[src.index("pfslam_search_wide: pfslam_search's winner"):src.index("int pfslam_search_wide(")]
    for word in ("bit for bit what pfslam_search returns", "2^31 - 1 candidates", "(2 half_x + 1)(2 half_y + 1) <= 2^24", "2^24 end points", "2^26 cells",
                 "(LB << 32 | k_origin) > the key", "8 x 128 MB", "profiles/search_wide.txt", "[5] batches"):
        assert word in spec, word
    kernel_h = open(os.path.join(ROOT, "gpu-icp-slam_amd", "host", "kernel.h")).read()
    assert re.search(r"bool\s+pfslamSearchWide\s*\(\s*glm::vec3 centre, float half_metres, float half_radians, glm::vec3 &pose, long long \*index\)", kernel_h)


def test_the_top_level_is_the_smallest_that_covers_the_longer_side_and_at_most_7():
    assert [Wd.top_level(n, 1) for n in (1, 2, 3, 4, 5, 37, 64, 65, 128, 129, 1601)] == [0, 1, 2, 2, 3, 6, 6, 7, 7, 7, 7]
    assert Wd.top_level(3, 41) == 6 and 1601 * 1601 * 503 == 1289290103 <= Wd.MAX_CAND and 1601 * 1601 <= Wd.MAX_ROW


@pytest.fixture(scope="module")
def world(pkg):
    p4000, segs, _ = R.planar_tree(4000, seed=1)
    trees = {"p4000": p4000, "np300": R.nonplanar_tree(300)}
    scans = {"scenario": np.resize(pkg.synth.make_scan(segs, B.SCENARIO_POSES[1], seed=7), 65), "weird": np.resize(pkg.synth.make_weird_scan(), 33)}
    return {"trees": trees, "fields": {k: S.Field(t) for k, t in trees.items()}, "scans": scans}


@pytest.mark.parametrize("window", sorted(WINDOWS))
@pytest.mark.parametrize("scan", ["scenario", "weird"])
@pytest.mark.parametrize("tree", ["p4000", "np300"])
def test_bounds_hold_for_every_block_and_the_descent_returns_the_winner(world, tree, scan, window):
    opts = dict(WINDOWS[window], max_dist=0.5 if tree == "np300" else 0.2)
    s = S.Search(world["fields"][tree], world["scans"][scan], CENTRE, **opts)
    vol = s.volume().astype(np.int64)
    w = Wd.Wide(s)
    assert (s.nx, s.ny, s.na) in ((37, 21, 3), (19, 11, 3))
    slack = []
    for L in range(4):
        n = 1 << L
        J, I = [g.ravel() for g in np.meshgrid(np.arange(0, s.ny, n), np.arange(0, s.nx, n), indexing="ij")]
        assert s.nx % n or L == 0                     # the last block of a row is partial
        for a in range(s.na):
            assert s.ends(a)[3] > 0
            lo = w.lb(a, I, J, L)
            least = np.array([vol[a, j:j + n, i:i + n].min() for i, j in zip(I, J)])
            assert (lo <= least).all(), "level %d heading %d: %d bounds exceed their block's smallest score" % (L, a, (lo > least).sum())
            if L == 0:
                assert (lo == vol[a].ravel()).all()
            slack.append(float((least - lo).mean()))
            # the origin's k is the block's lowest: every other candidate of the block has a larger i or j
            k = (a * s.ny + np.arange(s.ny)[:, None]) * s.nx + np.arange(s.nx)[None, :]
            assert all(k[j, i] == k[j:j + n, i:i + n].min() for i, j in zip(I, J))
    (Smin, kmin), count = w.descend()
    assert (Smin, kmin) == s.pick(vol)
    assert count["top"] == Wd.top_level(s.nx, s.ny) and count["scored"] <= s.cand
    print("%s %s %s: winner %d, score %d; mean slack of the bounds per level and heading %s; %d nodes bounded, %d of %d candidates scored"
          % (tree, scan, window, kmin, Smin, [round(v, 1) for v in slack], count["bounded"], count["scored"], s.cand))
    got = Wd.search_wide(world["fields"][tree], world["scans"][scan], CENTRE, **opts)
    assert S.same_result(got, S.search(world["fields"][tree], world["scans"][scan], CENTRE, **opts), volume=False) is None
    # from a lower top level too: the winner does not depend on where the descent starts
    assert Wd.Wide(s).descend(top=2)[0] == (Smin, kmin)


def test_a_constructed_tie_goes_to_the_lowest_k_and_a_looser_rule_loses_it(world):
    tree, field = world["trees"]["p4000"], world["fields"]["p4000"]
    scan, centre, opts = Wd.tie_case(tree, field)
    want = S.search(field, scan, centre, **opts)
    flat = want["scores"].ravel()
    holders = np.flatnonzero(flat == flat.min())
    assert want["qcap"] == 1 and want["beams"] == 1 and flat.min() == 0 and len(holders) >= 2 and want["index"] == holders[0]
    got = Wd.search_wide(field, scan, centre, **opts)
    assert S.same_result(got, want, volume=False) is None and got["index"] == holders[0]
    # the winner is no block's origin above level 0, so it is reached only by descending blocks whose LB EQUALS the best S
    nx = 2 * opts["half_x"] + 1
    assert (holders[0] % nx) % 2 and (holders[0] // nx) % 2
    s = S.Search(field, scan, centre, **opts)
    w = Wd.Wide(s)
    i, j = (holders[0] % nx) & ~1, (holders[0] // nx) & ~1
    assert w.lb(0, [i], [j], 1)[0] == 0 == flat.min(), "the block that holds the winner has LB == the best S: a rule that drops on equality loses it"


def test_the_saturated_far_centre_case_picks_k_0_and_status_2_has_none(world):
    field = world["fields"]["p4000"]
    for centre in ((1000.0, 1000.0, 0.0), (30000.0, 0.22, 0.13)):          # every cell saturates; no end point has a cell
        want = S.search(field, world["scans"]["scenario"], centre, half_x=5, half_y=3, half_theta=1)
        got = Wd.search_wide(field, world["scans"]["scenario"], centre, half_x=5, half_y=3, half_theta=1)
        assert S.same_result(got, want, volume=False) is None
        assert got["index"] == 0 and got["score"] == got["qcap"] * got["beams"]
        # every node ties with the key on LB; only the one with k_origin = 0 survives a level: the all-tied worst case costs four nodes a level
        assert got["count"]["scored"] <= 4 and got["count"]["bounded"] <= 3 + 4 * 4, got["count"]
    far = np.full(65, 1000.0, np.float32)
    got = Wd.search_wide(field, far, (0.6, 0.22, 0.13), half_x=5, half_y=3, half_theta=1, step_theta=0.3)
    want = S.search(field, far, (0.6, 0.22, 0.13), half_x=5, half_y=3, half_theta=1, step_theta=0.3)
    assert S.same_result(got, want, volume=False) is None and got["status"] == 2 and got["index"] == -1
