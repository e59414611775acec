"""The scenarios of tests/map_geometry_cases.py, checked on the oracle's output alone: each one still reaches the edge it was built
for (an odd size, a tail chunk, a partial block, a stride of the closed-form ray, a side of the grid, a clamp, an inexact float index).
tests/test_gpu_map_geometry.py runs the product against the oracle on exactly these scenarios.  No GPU needed."""
import numpy as np
import pytest

import map_geometry_cases as G


@pytest.fixture(scope="module")
def orc(oracle):
    return oracle


def test_map_sizes_have_the_properties_they_were_chosen_for(orc):
    dims = {d: G.dim_of(*G.SIZES[d]) for d in G.SIZES}
    assert all(d == v for d, v in dims.items()), dims
    M = {d: d * d for d in G.SIZES}
    assert M[3] == 9 and M[3] < 16                                        # less than one 16-cell chunk
    assert M[67] == 4489 and (M[67] + 4095) // 4096 == 2 and M[67] % 16 == 9 and M[67] - 4096 < 16 * 256  # second block nearly empty, ends in a tail
    assert M[151] % 16 == 1 and 151 % 2 == 1
    assert M[250] % 16 == 4 and M[250] % 4096 != 0
    assert M[1333] % 16 == 9 and M[1333] % 4096 != 0
    assert M[4800] % 16 == 0 and 4800 > 4096 and M[4800] > 1 << 24        # the float wall index is not exact
    assert {M[d] % 16 for d in G.SIZES} >= {0, 1, 4, 9}
    # the closed form's documented limit (include/pfslam.h, map_res_x): a ray of 20 m / res cells, k * deltay below 2^31
    assert all(20.0 / G.res_of(d) < 46341 for d in G.SIZES) and 46340 * 46340 < 1 << 31 <= 46341 * 46341


def test_one_beam_scans_end_on_every_short_offset(orc):
    """All 625 offsets of [-12, 12]^2 from the middle of the 67-cell map: the oracle's wall cell is exactly centre + offset."""
    dim, res = 67, G.res_of(67)
    c = dim // 2
    groups = set()
    for dx, dy in G.short_offsets():
        theta, scan = G.one_beam(dx, dy, res)
        assert G.beam_offset(theta, scan[0], res) == (dx, dy)
        fm, wm = G.masks(dim, scan, c, c, theta)
        assert np.flatnonzero(wm).tolist() == [(c + dx) * dim + (c + dy)], (dx, dy)
        assert int(fm.sum()) == max(abs(dx), abs(dy)), (dx, dy)          # one cell per step of the longer side; none for the zero ray
        groups.add(G.classify(dx, dy))
    assert groups == set(G.ALL_GROUPS) | {"zero"}


@pytest.mark.parametrize("lengths", [G.MASK_LENGTHS, G.FIND_LENGTHS], ids=["mask", "find_walls"])
def test_long_rays_cover_every_group_at_every_length(orc, lengths):
    """The 1333-cell map: offsets as the oracle gives them have the asked length on their longer side, and every axis, diagonal and
    octant (shallow and steep) is present at every length."""
    dim, res = 1333, G.res_of(1333)
    c = dim // 2
    for L in lengths:
        groups = set()
        for dx, dy in G.long_offsets(L):
            theta, scan = G.one_beam(dx, dy, res)
            off = G.beam_offset(theta, scan[0], res)
            assert off is not None and max(abs(off[0]), abs(off[1])) == L, (L, dx, dy, off)
            assert 0 <= c + off[0] < dim and 0 <= c + off[1] < dim
            groups.add(G.classify(*off))
        assert groups == set(G.ALL_GROUPS), (L, set(G.ALL_GROUPS) - groups)
        if lengths is G.MASK_LENGTHS:                                     # the whole ray is marked: L cells, more than one 64-lane trip
            theta, scan = G.one_beam(L, L // 9, res)
            fm, _ = G.masks(dim, scan, c, c, theta)
            assert int(fm.sum()) == L


def test_clipping_rays_leave_and_enter_through_every_side(orc):
    dim, res = 1333, G.res_of(1333)
    leave, enter, none_marked, some_marked = set(), set(), 0, 0
    xs, ys = set(), set()
    for cx, cy, dx, dy in G.clip_cases(dim):
        xs.add(cx); ys.add(cy)
        assert G.cell_of(dim, G.coord_of(dim, cx)) == cx and G.cell_of(dim, G.coord_of(dim, cy)) == cy
        theta, scan = G.one_beam(dx, dy, res)
        off = G.beam_offset(theta, scan[0], res)
        assert off == (dx, dy)
        fm, wm = G.masks(dim, scan, cx, cy, theta)
        start, end = G.side_of(dim, cx, cy), G.side_of(dim, cx + dx, cy + dy)
        marked = int(fm.sum())
        if start == "" and end != "" and marked:
            leave.add(end)
        if start != "" and end == "" and marked:
            enter.add(start)
        if start != "" or end != "":
            none_marked += marked == 0
            some_marked += marked > 0
        assert marked <= 100 and int(wm.sum()) == (end == "")
    want = {-40, -1, 0, dim - 1, dim, dim + 40}
    assert xs >= want and ys >= want
    assert leave >= {"x-", "x+", "y-", "y+"} and enter >= {"x-", "x+", "y-", "y+"}, (leave, enter)
    assert none_marked > 0 and some_marked > 0
    print("clipping: %d rays with an end outside mark cells, %d mark none" % (some_marked, none_marked))


def test_wall_index_is_inexact_in_float_at_4800_cells(orc):
    sc = G.size_scenario(4800)
    far = sc["scan"][460:621]
    assert (far >= 15.0).all() and (far <= 19.0).all()
    exact, flt = G.inexact_wall_cells(sc)
    n_inexact = int((exact != flt).sum())
    print("4800 cells: %d of %d wall cells have an inexact float index" % (n_inexact, len(exact)))
    assert n_inexact > 0 and exact.max() > 1 << 24
    assert (np.abs(exact - flt) <= 1).all() and flt.max() < 4800 * 4800
    # the oracle marks the float index, as the reference does (kernel.cu:545)
    assert np.flatnonzero(sc["wm"]).tolist() == sorted(set(flt.tolist()))


@pytest.mark.parametrize("dim", sorted(G.SIZES))
def test_size_scenarios_reach_the_clamps_and_the_grid_edges(orc, dim):
    sc = G.size_scenario(dim)
    fm, wm, before = sc["fm"].astype(bool), sc["wm"].astype(bool), sc["grid"].reshape(-1).copy()
    assert fm.any() and wm.any()
    after = G.update_grid(sc["grid"].copy(), dim, sc["pose"], sc["scan"]).reshape(-1)
    both = fm & wm
    if dim > 3:                                                           # (nine cells cannot hold every case)
        for v in G.CLAMP_VALUES:
            assert (before[fm & ~wm] == v).any() and (before[wm & ~fm] == v).any(), v
        assert (after[fm & ~wm & (before == -113)] == -113).all()        # the lower clamp: -113 - 1 stays
        assert (after[fm & ~wm & (before == -112)] == -113).all()
        assert (after[wm & ~fm & (before == 112)] == 113).all()          # the upper clamp: 112 + 4 and 113 + 4 -> 113
        assert (after[wm & ~fm & (before == 113)] == 113).all()
        assert both.any() and (after[both & (before == -113)] == -109).all()   # +4 behind the (clamped) -1
        assert (after[both & (before == 112)] == 113).all()
        n_out = sum(1 for j, r in enumerate(sc["scan"]) if (o := G.beam_offset(sc["pose"][2], r, G.res_of(dim), j)) is not None
                    and G.side_of(dim, sc["cx"] + o[0], sc["cy"] + o[1]) != "")
        # rays that leave the grid (the 40 m and 48 m maps are wider than the 20 m range: there only the corner pose's rays do)
        assert n_out > 0 or dim * G.res_of(dim) / 2 > 19.9
    assert (after[~fm & ~wm] == before[~fm & ~wm]).all()
    print("%d cells: %d free, %d wall, %d both" % (dim, fm.sum(), wm.sum(), both.sum()))
    # the robot in the far corner: both masks have cells in their last chunk (the tail branch when dim * dim % 16 != 0) and in the
    # last 4096-cell block, and rays leave through x+ and y+
    M = dim * dim
    co = G.size_scenario(dim, corner=True)
    assert (co["cx"], co["cy"]) == (dim - 1, max(dim - 3, 0))
    tail = M - (M % 16 or 16)
    assert co["fm"][tail:].any() and co["wm"][tail:].any(), "no marked cell in the last chunk"
    assert dim == 3 or (co["fm"][:tail].any() and co["wm"][:tail].any())        # (3 cells: the tail is the whole map)
    gone = {G.side_of(dim, co["cx"] + o[0], co["cy"] + o[1]) for j, r in enumerate(co["scan"])
            if (o := G.beam_offset(co["pose"][2], r, G.res_of(dim), j)) is not None}
    assert gone >= {"", "x+", "y+"}, gone


@pytest.mark.parametrize("dim", sorted(G.SIZES))
def test_score_scenarios_straddle_every_edge(orc, dim):
    sc = G.score_scenario(dim, 300)
    cells = G.score_cells(sc)
    for axis in (0, 1):
        c = cells[:, :, axis]
        for lo, hi in ((-1, 0), (dim - 1, dim)):
            per = [(c[i] <= lo).any() and (c[i] >= hi).any() for i in range(len(c))]
            assert any(per), (dim, axis, lo, hi)
    inside = ((cells >= 0) & (cells < dim)).all(axis=2)
    assert inside.any() and (~inside).any()
    want = G.score_grid(sc)
    assert len(set(want.tolist())) > 1
