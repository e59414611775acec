"""Whole frames and stage entry points at the particle counts where the host code changes the launch shape.

Every comparison is bit for bit against the CPU oracle (tests/oracle_lib.py; tests/resampler_ref.py for resampler modes 1 and 2,
tests/estimate_ref.py for pfslam_estimate); there is no tolerance anywhere in this file, and the reference is never a second product
handle -- except the shadow of section 1's systematic-resampler run (tests/stage_shadow.py, as tests/test_gpu_resampler.py uses it).

The edges, read out of csrc/ (test_the_size_lists_hold_every_edge_the_code_has reads the constants out of the sources again and
fails when one moves without the lists below):

  n > 64                 lane order by Hilbert cell (k_cell_count / k_cell_scan / k_cell_scatter) and any organisation at all
                         (org_use_cells: `h->n > 64`); 64 and below: identity order, plain traversal (variant 4: the plan without an order)
  n >= 65                cell rows in the frame loop and in the sharded frame (org_use_cells, frame_loop: 65) -> round-5 frame (frame_v2_ok)
  n >= 4608              cell rows / plan in stage calls and on the staged chain (plan_min_particles)
  used >= 256            beam chunks: k_reduce_groups<4> | <1> in the round-5 frame, k_reduce_partials_minmax_wide | k_reduce_partials_minmax on
                         the staged chain.  score_chunks gives 271 chunks up to 91 groups of 64 and 217 from 92 groups on: at 1081 beams the
                         edge is 5824 | 5825 particles (not 6144 | 6145, which stay in the lists: 96 | 97 groups, 217 chunks on either side)
  n <= 4096              k_resample_small + k_weights_small (frame_v2_finish, launch_resample, pfslam_step, score_grid_launch: PF_SUM_TILE =
                         4 * PF_SCAN_TILE) | tiled passes + k_sample_gather
  tiles                  (n + 1023) / 1024 scan tiles, (n + 4095) / 4096 sum tiles, (n + 255) / 256 and (n + 63) / 64 blocks and waves
  n <= 400000            2^18 | 2^21 Hilbert cells (launch_score, frame_v2_begin: bits 6 | 7; org_use_cells: Dside 64 | 128)
  not run here           (gn + 1023) / 1024 > 4096, i.e. above 4 194 304 particles: frame_v2_ok refuses round-5 frames, and launch_resample takes
                         k_scan_pmax + k_sample_gather<false, ...> instead of <true, ...> (nt > PF_PMAX_LDS).  One oracle frame there costs
                         some 16 s at 64 beams (1.6 s at 400 001) and 2 GB of partials at 1081: too much for a test of a few seconds
  shards                 a last shard of one particle; a shard of exactly 4608; shards of 64 | 65 (a 64-particle shard never runs round-5 frames)

Mutations this file was checked against (each once, on a scratch copy; with them five older GPU modules, their long tests left out):
  2^21 cells with k_cell_scan's grid left at 256 workgroups (and the order buffer zeroed, so that unwritten slots hold a valid index):
      both 400 001 cases fail; of the older tests test_gpu_edges.py::test_one_million_particles
  one `(gn + 4095) / 4096` of launch_weight_sums_with_scan_front turned into `gn / 4096`: 22 cases fail (KD frames from 4097 on except
      8192, 2-D frames at 4097 and 8193, every sharded layout); older: the 2-D device-library frames at 10 000 and two sharded cases
  first-argmax towards the higher index in k_reduce_partials_minmax_wide: the shared-best-fit frames fail at 64, 65, 4097 and 5824 and pass
      at 5825, where the other reduce runs; older: nine cases at 50, 1000 and 20 000 particles
  k_resample_small up to 4 * PF_SCAN_TILE + 1 particles in launch_resample: NOT caught, by this file or the older ones.  At 4097 particles
      the kernel's fifth wave scans the fifth tile, and every word written past the three 4-entry LDS arrays is read back by the thread
      that needs it before anything overwrites it: the results are bit-identical, and this file compares results only.
"""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import estimate_ref as E
import oracle_lib as O
import resampler_ref as R
from stage_shadow import StageShadow
from test_gpu_devlib_frames import assert_same_particles, corridor, environ, same_trace
from test_gpu_estimate import gather_by_hand, same16
from test_gpu_sharded import _VirtualRanks
from test_resampler_spec import skewed

gpu = pytest.mark.gpu          # (every test but the first: that one reads source text and runs with the CPU suite)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-icp-slam_amd", "csrc")
FIELDS = ("x", "y", "theta", "w")
NB = 1081

WAVE, BLOCK, SCAN_TILE, SUM_TILE, PLAN_MIN, BIG = 64, 256, 1024, 4096, 4608, 400000


def score_chunks(n, nb):
    """score_chunks + the two divisions behind it (csrc/pfslam_hip.hip) for integral map weights: (beams per chunk, chunks used)"""
    groups = (n + 63) // 64
    target = max(24576, min(65536, groups * 160))
    chunks = max(1, min((target + groups - 1) // groups, nb))
    bpc = (nb + chunks - 1) // chunks
    return bpc, (nb + bpc - 1) // bpc


WIDE_LAST = max(n for n in range(1, 20000) if score_chunks(n, NB)[1] >= 256)     # 5824 at 1081 beams

KD_SIZES = [1, 2, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 4607, 4608, 4609,
            WIDE_LAST - 1, WIDE_LAST, WIDE_LAST + 1, 6143, 6144, 6145, 8191, 8192, 8193]
GRID_SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193]
STAGE_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 4607, 4608, 4609, 8191, 8193]
EXTRA_ORGS = (65, 4097, 6145)          # also one stream, and events instead of gates
SYSTEMATIC = (4096, 4097, 8193)        # also pfslam_set_resampler(2) against the shadow, and pfslam_estimate behind the last frame


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def timed(fn):
    import functools

    @functools.wraps(fn)
    def wrapper(*a, **kw):
        t0 = time.perf_counter()
        try:
            return fn(*a, **kw)
        finally:
            dt = time.perf_counter() - t0
            print("[wall] %s %s: %.2f s" % (fn.__name__, {k: v for k, v in kw.items() if k in ("n", "lay", "mode", "variant")}, dt))
    return wrapper


# ---- the code's own numbers ----------------------------------------------------------------------------------------------------------------
def test_the_size_lists_hold_every_edge_the_code_has():
    """The constants behind the lists above, read out of the sources: a threshold that moves takes this test with it, and every edge has
    its two sides (and, where it is a tile, the size one above) in the lists of the sections that cross it."""
    hip = open(os.path.join(CSRC, "pfslam_hip.hip")).read()
    stages = open(os.path.join(CSRC, "pfslam_stages.hip.inc")).read()
    frame = open(os.path.join(CSRC, "pfslam_frame.hip.inc")).read()
    assert int(re.search(r"#define PF_SUM_TILE (\d+)", hip).group(1)) == SUM_TILE
    assert int(re.search(r"#define PF_SCAN_TILE (\d+)", hip).group(1)) == SCAN_TILE
    assert int(re.search(r'getenv\("PFSLAM_PLAN_MIN_N"\)\) : (\d+);', hip).group(1)) == PLAN_MIN
    assert re.search(r"\(frame_loop && !env_min\) \? (\d+) :", hip).group(1) == str(WAVE + 1)
    assert "h->variant != 1 && h->n > %d" % WAVE in hip and "h->n > %d && (h->n >= plan_min_n" % WAVE in hip
    assert len(re.findall(r"h->n <= (\d+) \? 6 : PF_CELL_BITS_MAX", hip + frame)) == 2
    assert set(re.findall(r"h->n <= (\d+) \? ", hip + frame)) == {str(BIG)}
    assert "std::max(24576, std::min(65536, groups * 160))" in hip
    assert "wide_reduce = used >= 256 &&" in hip and "if (used >= 256)" in frame
    assert "h->n <= 4 * PF_SCAN_TILE" in stages and len(re.findall(r"if \(n <= PF_SUM_TILE\)", frame)) == 2 and "h->n <= PF_SUM_TILE" in stages
    assert WIDE_LAST == 5824 and score_chunks(WIDE_LAST, NB) == (4, 271) and score_chunks(WIDE_LAST + 1, NB) == (5, 217)
    assert score_chunks(6144, NB) == score_chunks(6145, NB) == (5, 217)       # (no edge there)
    for edge in (WAVE, BLOCK, SCAN_TILE, SUM_TILE):
        for lst in (KD_SIZES, GRID_SIZES, STAGE_SIZES):
            assert {edge - 1, edge, edge + 1} <= set(lst), (edge, lst)
    for lst in (KD_SIZES, STAGE_SIZES):
        assert {PLAN_MIN - 1, PLAN_MIN, PLAN_MIN + 1} <= set(lst) and 2 * SUM_TILE + 1 in lst
    assert {WIDE_LAST - 1, WIDE_LAST, WIDE_LAST + 1} <= set(KD_SIZES)
    assert set(BIG_SIZES) == {BIG, BIG + 1}


# ---- the world -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kdworld(pkg):
    pts, segs = pkg.synth.make_map_points(2000, seed=1)
    tree = pkg.kd_create(pts)
    scans = [pkg.synth.make_scan(segs, (0.002 * i, 0.001 * i, 0.0004 * i), seed=2000 + i) for i in range(6)]
    return tree, scans


def row_of(e):
    """what is compared after every frame: the trace (neff as bits) and the pose bits"""
    t = e.trace()
    return (t["best"], t["resampled"], t["n_wall"], t["n_free"], t["n_insert"], int(bits(t["neff"])[0]), t["kd_size"]) + tuple(bits(e.pose).tolist())


_ORACLE = {}


def oracle_frames(kind, n, nb, scans, tree=None, first=6):
    """The CPU oracle through the frames, once per (kind, size, beams): rows, particles, map bytes (KD) or grid."""
    key = (kind, n, nb, len(scans))
    if key not in _ORACLE:
        with environ(ORC_THREADS="16"):
            o = O.Slam(n, n_beams=nb, kd_capacity=(len(tree) if tree is not None else 0) + (1 << 16))
            if tree is not None:
                o.set_map(tree)
            rows = []
            for i, s in enumerate(scans):
                (o.step_grid if kind == "grid" else o.step)(first + i, s)
                rows.append(row_of(o))
            _ORACLE[key] = {"rows": rows, "particles": o.particles().copy(), "map": o.tree().tobytes() if kind != "grid" else None,
                            "grid": o.grid.copy() if kind == "grid" else None}
            o.close()
    return _ORACLE[key]


def assert_resampling_branches(rows, n, what):
    """Each whole-frame case reaches the resampling and the non-resampling branch -- where the arithmetic lets it: one particle never
    resamples (Neff = 1 >= 0.7), two always do unless their fits tie (the weights are 0 and 1: Neff = 1 < 1.4)."""
    flags = {r[1] for r in rows}
    if n != 2:
        assert 0 in flags, "%s: every frame resampled" % what
    if n > 1:
        assert 1 in flags, "%s: no frame resampled" % what


def run_kd(pkg, tree, scans, n, nb, want, variant=0, serial=False, events=False, first=6):
    """pfslam_step through the frames on a fresh handle, every frame against the oracle's row; returns what ran: per frame
    (round-5 frame, cell rows, plan rows), the last frame mode, and the handle (open: the caller reads it and closes it)."""
    with environ(**({"PFSLAM_GATES": "0"} if events else {})):
        h = pkg.PfSlam(n, n_beams=nb, kd_capacity=len(tree) + (1 << 16))
    h.set_map(tree)
    if variant:
        h.set_variant(variant)
    if serial:
        h.set_serial(1)
    ran = []
    for i, s in enumerate(scans):
        h.step(first + i, s)
        got = row_of(h)
        assert got == want["rows"][i], "n %d variant %d frame %d: %s vs the oracle's %s" % (n, variant, first + i, got, want["rows"][i])
        fm = h.frame_mode()
        ran.append((fm["round5_frame"], h.cell_stats()["rows"] > 0, h.plan_stats()["rows"] > 0))
    assert_same_particles(h.particles(), want["particles"], "n %d variant %d" % (n, variant))
    assert h.map().tobytes() == want["map"], "n %d variant %d: maps differ" % (n, variant)
    return ran, h.frame_mode(), h


# ---- 1. whole KD frames ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", KD_SIZES)
@timed
@gpu
def test_kd_frames_equal_the_oracle_in_every_organisation(pkg, kdworld, n):
    """pfslam_step, 1081 beams, frames 6 .. 11 on the 2000-point map, against O.Slam.step: trace and pose after every frame, particles and map
    at the end -- in the default organisation, with cell rows forced (variant 3), on the staged chain with the plain traversal (variant 2)
    and with the shared-prefix plan (variant 4); at three sizes also on one stream and with events instead of gates; at three sizes with
    the systematic resampler against the shadow, and pfslam_estimate behind the last frame."""
    tree, scans = kdworld
    want = oracle_frames("kd", n, NB, scans, tree)
    assert_resampling_branches(want["rows"], n, "n %d" % n)
    seen = {}
    for variant in (0, 3, 2, 4):
        ran, _, h = run_kd(pkg, tree, scans, n, NB, want, variant)
        if variant == 0 and n in SYSTEMATIC:
            same16(h.estimate_raw(), E.estimate_particles(want["particles"]), "estimate behind the frames, n %d" % n)
        h.close()
        seen[variant] = ran
        r5 = [r[0] for r in ran]
        if variant == 3:     # cell rows forced: round-5 frames from 65 particles on, never at 64 and below
            if n > WAVE:
                assert all(r5) and all(r[1] for r in ran), (n, ran)
            else:
                assert not any(r5) and not any(r[1] for r in ran), (n, ran)
        elif variant == 2:   # plain traversal on the staged chain
            assert not any(r5) and not any(r[1] or r[2] for r in ran), (n, ran)
        elif variant == 4:   # the plan on the staged chain, at every count
            assert not any(r5) and all(r[2] for r in ran) and not any(r[1] for r in ran), (n, ran)
        else:                # default: the frame loop's cell rows start at 65 particles (and stay while the cloud is narrow enough for its size)
            if n > WAVE:
                assert r5[0] and ran[0][1], (n, ran)
                assert all(r[1] for r in ran if r[0]), (n, ran)
                # a frame whose cloud is too wide for the rows takes the staged chain: there the plan from plan_min_particles on, nothing below
                assert all((r[1], r[2]) == (False, n >= PLAN_MIN) for r in ran if not r[0]), (n, ran)
            else:
                assert not any(r5) and not any(r[1] or r[2] for r in ran), (n, ran)
    if n in EXTRA_ORGS:
        ran, fm, h = run_kd(pkg, tree, scans, n, NB, want, variant=3, serial=True)
        assert all(r[0] for r in ran) and fm["serial"], (n, ran, fm)
        h.close()
        ran, fm, h = run_kd(pkg, tree, scans, n, NB, want, variant=3, events=True)
        assert all(r[0] for r in ran) and not fm["gates"] and not fm["serial"], (n, ran, fm)
        h.close()
    if n in SYSTEMATIC:
        kw = dict(n_beams=NB, kd_capacity=len(tree) + (1 << 16))
        s = StageShadow(n, pkg=pkg, **kw)
        s.h.set_resampler(2)
        s.set_map(tree)
        h = pkg.PfSlam(n, **kw)
        h.set_resampler(2)
        h.set_variant(3)
        h.set_map(tree)
        flags = set()
        for i, scan in enumerate(scans):
            s.step(6 + i, scan); h.step(6 + i, scan)
            assert same_trace(h.trace(), s.trace()), (n, i, h.trace(), s.trace())
            assert (bits(h.pose) == bits(s.pose)).all(), (n, i)
            flags.add(h.trace()["resampled"])
        assert flags == {0, 1}, flags
        assert h.frame_mode()["round5_frame"]
        assert_same_particles(h.particles(), s.particles(), "systematic, n %d" % n)
        assert h.map().tobytes() == s.map().tobytes()
        same16(h.estimate_raw(), E.estimate_particles(s.particles()), "estimate behind systematic frames, n %d" % n)
        s.close(); h.close()
    print("n %d: round-5 frames of 6: default %d, variant 3 %d; cell rows / plan on the staged chain: default %s, variant 4 %s"
          % (n, sum(r[0] for r in seen[0]), sum(r[0] for r in seen[3]), [(r[1], r[2]) for r in seen[0] if not r[0]], all(r[2] for r in seen[4])))


TIED_SIZES = (64, 65, 4097, WIDE_LAST, WIDE_LAST + 1)


@pytest.mark.parametrize("n", TIED_SIZES)
@timed
@gpu
def test_kd_frames_whose_best_fit_is_shared_by_many_particles(pkg, kdworld, n):
    """The fits of the world's frames are all but distinct (one particle holds the maximum), so the frames above never ask which of several
    best particles the frame takes.  Here all beams but four are rejected (range 0): a fit is a sum of four integer map weights and the
    maximum of the first frame is shared (3 particles of 64, 301 of 4097).  first-argmax decides `best`, the pose and everything behind
    it: four frames in every organisation against O.Slam.step -- the staged chain's reduce is k_reduce_partials_minmax_wide up to 5824
    particles and k_reduce_partials_minmax above, the round-5 frame's k_reduce_groups<4> | <1>."""
    tree, scans = kdworld
    sparse = []
    for s in scans[:4]:
        t = np.zeros_like(s)
        keep = np.linspace(100, 980, 4).astype(int)
        t[keep] = s[keep]
        sparse.append(t)
    want = oracle_frames("kd-sparse", n, NB, sparse, tree)
    fit = O.score_kd(tree, O.add_noise(O.make_particles(n), 6), sparse[0], threads=16)    # the first frame's dispersion and scores, restated
    assert int(np.argmax(fit)) == want["rows"][0][0]
    assert (fit == fit.max()).sum() >= 2, "n %d: the maximum is not shared" % n
    for variant in (0, 2, 3, 4):
        ran, _, h = run_kd(pkg, tree, sparse, n, NB, want, variant)
        assert any(r[0] for r in ran) == (n > WAVE and variant in (0, 3)), (n, variant, ran)
        h.close()


# ---- 2. whole 2-D frames ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", GRID_SIZES)
@timed
@gpu
def test_grid_frames_equal_the_oracle(pkg, n):
    """pfslam_step_grid from an empty map, the corridor's first 8 scans, against O.Slam.step_grid: the trace after every frame, the grid and
    the particles at the end."""
    scans = corridor(pkg, 8)
    want = oracle_frames("grid", n, NB, scans, first=1)
    assert_resampling_branches(want["rows"], n, "2-D, n %d" % n)
    h = pkg.PfSlam(n, kd_capacity=1 << 16)
    for i, s in enumerate(scans):
        h.step_grid(1 + i, s)
        got = row_of(h)
        assert got == want["rows"][i], "2-D, n %d frame %d: %s vs the oracle's %s" % (n, 1 + i, got, want["rows"][i])
    assert not h.frame_mode()["round5_frame"]
    g = h.grid()
    assert (g == want["grid"]).all(), "2-D, n %d: %d grid cells differ" % (n, (g != want["grid"]).sum())
    assert_same_particles(h.particles(), want["particles"], "2-D, n %d" % n)
    h.close()


# ---- 3. stage entry points -------------------------------------------------------------------------------------------------------------------
_STAGE = {}


def stage_inputs(tree, scan, n):
    """particles dispersed once around the origin with random weights; the oracle's fits of them (computed once per size)"""
    if n not in _STAGE:
        p = O.add_noise(O.make_particles(n), 3)
        p["w"] = np.random.RandomState(n).uniform(0.1, 1.0, n).astype(np.float32)
        _STAGE[n] = (p, O.score_kd(tree, p, scan, threads=16))
    return _STAGE[n]


def tie_slots(n):
    """(earlier, later) slot of a fit that occurs twice: the later one is the very last particle, the earlier one the first particle of the
    last, partly filled tile -- of the largest of the code's tiles (4096, 1024, 256, 64) that n exceeds; where that tile holds the last
    particle alone (n = tile + 1), the first particle of the tile in front of it."""
    for t in (SUM_TILE, SCAN_TILE, BLOCK, WAVE):
        if n > t:
            t0 = (n - 1) // t * t
            return (t0 if t0 < n - 1 else t0 - t), n - 1
    return 0, n - 1


def oracle_measurement(p, fit):
    n = len(p)
    imin, imax = C.c_int(), C.c_int()
    O.lib().orc_minmax_first_f32(O.P(fit), n, C.byref(imin), C.byref(imax))
    fmin, fmax = fit[imin.value], fit[imax.value]
    want = p.copy()
    with np.errstate(all="ignore"):
        rng = np.float32(fmax) - np.float32(fmin)
        if rng > 0:    # (a range of zero leaves the weights alone: tests/test_gpu_stages.py)
            O.lib().orc_update_weights_f32(O.P(want), n, O.P(fit), float(np.float32(1) / rng), int(fmin))
    return imin.value, imax.value, fmin, fmax, want


@pytest.mark.parametrize("n", STAGE_SIZES)
@timed
@gpu
def test_score_and_measurement_stages_equal_the_oracle(pkg, kdworld, n):
    """pfslam_score_kd in variants 0 .. 4 against orc_score_kd, every fit; pfslam_measurement_update (best, fmin, fmax, every weight) against
    orc_minmax_first_f32 / orc_update_weights_f32 -- on the dispersed cloud, and on one whose maximal and minimal fit each occur twice and
    nowhere else: the maximum in the first slot of the last partly filled tile and in the very last slot, the minimum in the slots next to
    them (tie_slots: first-argmax across a tile edge)."""
    tree, scans = kdworld
    scan = scans[0]
    p, fit = stage_inputs(tree, scan, n)
    for variant in (0, 1, 2, 3, 4):
        h = pkg.PfSlam(n, kd_capacity=len(tree) + (1 << 16))
        h.set_variant(variant)
        h.set_map(tree); h.set_particles(p); h.set_scan(scan)
        got = h.score_kd()
        bad = int((bits(got) != bits(fit)).sum())
        assert bad == 0, "n %d variant %d: %d fits differ from the oracle's" % (n, variant, bad)
        rows, plan = h.cell_stats()["rows"] > 0, h.plan_stats()["rows"] > 0
        if variant == 0:      # organised from plan_min_particles on: cell rows (this cloud is narrow)
            assert (rows, plan) == ((True, False) if n >= PLAN_MIN else (False, False)), (n, rows, plan)
        elif variant == 3:
            assert (rows, plan) == ((True, False) if n > WAVE else (False, True)), (n, rows, plan)
        elif variant == 4:
            assert (rows, plan) == (False, True), (n, rows, plan)
        elif variant == 1:    # identity lane order: never the rows, the plan from plan_min_particles on
            assert (rows, plan) == (False, n >= PLAN_MIN), (n, rows, plan)
        else:
            assert (rows, plan) == (False, False), (n, variant, rows, plan)
        if variant == 0:
            imin, imax, fmin, fmax, want = oracle_measurement(p, fit)
            best, gmin, gmax = h.measurement_update()
            assert (best, bits(gmin), bits(gmax)) == (imax, bits(fmin), bits(fmax)), (n, best, imax)
            assert (bits(h.particles()["w"]) == bits(want["w"])).all(), n
        h.close()
    # ties across a tile edge (one particle has no second occurrence; two have no room for a second minimum)
    if n >= 2:
        e, later = tie_slots(n)
        q = p.copy()
        if n >= 4:
            inner = np.flatnonzero((fit > fit.min()) & (fit < fit.max()))
            assert len(inner), "n %d: every fit is extreme" % n
            for i in np.flatnonzero((fit == fit.max()) | (fit == fit.min())):     # vacate every natural extreme
                q[i] = p[inner[0]]
            for dst, src in ((e, int(np.argmax(fit))), (later, int(np.argmax(fit))), (e + 1, int(np.argmin(fit))), (later - 1, int(np.argmin(fit)))):
                q[dst] = p[src]
        else:
            q[later] = p[e]
        q["w"] = p["w"]
        qfit = O.score_kd(tree, q, scan, threads=16)
        imin2, imax2, fmin, fmax, want = oracle_measurement(q, qfit)
        assert imax2 == e and qfit[later] == fmax, (n, e, later, imax2)
        assert n < 4 or (imin2 == e + 1 and qfit[later - 1] == fmin), (n, e, later, imin2)
        h = pkg.PfSlam(n, kd_capacity=len(tree) + (1 << 16))
        h.set_map(tree); h.set_particles(q); h.set_scan(scan)
        got = h.score_kd()
        assert (bits(got) == bits(qfit)).all(), n
        best, gmin, gmax = h.measurement_update()
        assert (best, bits(gmin), bits(gmax)) == (imax2, bits(fmin), bits(fmax)), "n %d: best %d, the first of the two maxima is %d" % (n, best, imax2)
        if n >= 4:
            assert (bits(h.particles()["w"]) == bits(want["w"])).all(), n
        h.close()


@pytest.mark.parametrize("n", STAGE_SIZES)
@timed
@gpu
def test_motion_stage_equals_the_oracle(pkg, n):
    """pfslam_motion_update at frame 7 against orc_add_noise: every pose bit, the weights untouched."""
    p = O.add_noise(O.make_particles(n, 0.3, -0.2, 0.1), 3)
    p["w"] = np.random.RandomState(n + 1).uniform(0.1, 1.0, n).astype(np.float32)
    h = pkg.PfSlam(n)
    h.set_particles(p)
    h.motion_update(7)
    assert_same_particles(h.particles(), O.add_noise(p.copy(), 7), "motion, n %d" % n)
    h.close()


def one_hot(n, k):
    p = O.make_particles(n, w=0.0)
    p["x"] = np.arange(n)
    p["w"][k] = 1.0
    return p


@pytest.mark.parametrize("n", STAGE_SIZES)
@timed
@gpu
def test_resample_stage_equals_the_restatement(pkg, n):
    """pfslam_resample in modes 0, 1, 2 with x = the particle's index, against tests/resampler_ref.py: the skewed weights of
    tests/test_resampler_spec.py, only the last particle weighted (every draw lands on n - 1), only the first."""
    frame = 17
    cases = [("skewed", skewed(n)), ("last only", one_hot(n, n - 1)), ("first only", one_hot(n, 0))]
    for mode in (0, 1, 2):
        h = pkg.PfSlam(n)
        h.set_resampler(mode)
        for name, p in cases:
            did, neff, src = R.resample_ref(p, frame, mode)
            h.set_particles(p)
            did_g, neff_g = h.resample(frame)
            assert did_g == did and bits(neff_g) == bits(neff), (n, mode, name, did_g, did, neff_g, neff)
            got = h.particles()
            if not did:
                assert n == 1 or name == "skewed", (n, name)
                assert_same_particles(got, p, "%s, n %d mode %d: not resampled" % (name, n, mode))
                continue
            bad = int((got["x"] != src.astype(np.float32)).sum())
            assert bad == 0, "%s, n %d mode %d: %d sources differ from the restatement" % (name, n, mode, bad)
            assert (bits(got["y"]) == bits(p["y"][src])).all() and (bits(got["theta"]) == bits(p["theta"][src])).all() and (got["w"] == 1).all()
            if name == "last only":
                assert (src == n - 1).all()
            elif name == "first only":
                assert (src == 0).all()
        h.close()


# ---- 4. above 400 000 particles ---------------------------------------------------------------------------------------------------------------
BIG_SIZES = (BIG, BIG + 1)
BIG_NB = 64


@pytest.fixture(scope="module")
def bigworld(kdworld):
    tree, scans = kdworld
    return tree, [np.ascontiguousarray(s[:BIG_NB]) for s in scans[:3]]


@pytest.mark.parametrize("n", BIG_SIZES)
@timed
@gpu
def test_score_stage_on_either_side_of_400000_particles(pkg, bigworld, n):
    """pfslam_score_kd, 64 beams, variants 0, 1 and 3 against orc_score_kd, every fit: 2^18 Hilbert cells at 400 000, 2^21 at 400 001
    (k_cell_count with 7 bits, k_cell_scan over 2048 tiles, k_cell_scatter with 2048 tile totals); variant 1 never sorts."""
    tree, scans = bigworld
    p = O.add_noise(O.make_particles(n), 3)
    want = O.score_kd(tree, p, scans[0], threads=16)
    for variant in (0, 1, 3):
        h = pkg.PfSlam(n, n_beams=BIG_NB, kd_capacity=len(tree) + (1 << 16))
        h.set_variant(variant)
        h.set_map(tree); h.set_particles(p); h.set_scan(scans[0])
        got = h.score_kd()
        bad = int((bits(got) != bits(want)).sum())
        assert bad == 0, "n %d variant %d: %d of %d fits differ from the oracle's" % (n, variant, bad, n)
        assert (h.cell_stats()["rows"] > 0) == (variant != 1), (n, variant)
        h.close()


@pytest.mark.parametrize("n", BIG_SIZES)
@timed
@gpu
def test_kd_frames_on_either_side_of_400000_particles(pkg, bigworld, n):
    """Three frames of pfslam_step at 64 beams against O.Slam.step (whose resample searches once per distinct draw:
    orc_weighted_sample_indices_memo, held to the definition by tests/test_resampler_spec.py): rows, particles, map; round-5 frames."""
    tree, scans = bigworld
    want = oracle_frames("kd", n, BIG_NB, scans, tree)
    assert_resampling_branches(want["rows"], n, "n %d" % n)
    ran, fm, h = run_kd(pkg, tree, scans, n, BIG_NB, want)
    assert all(r[0] and r[1] for r in ran), (n, ran)
    h.close()


# ---- 5. sharded handles on one GPU -------------------------------------------------------------------------------------------------------------
# (global, world, stride).  9217 particles at stride 4608 are three shards (4608 + 4608 + 1); 4609 are the two the issue names.
LAYOUTS = [(129, 3, 64), (4097, 2, 4096), (8193, 3, 4096), (9217, 3, 4608), (4609, 2, 4608)]


@pytest.mark.parametrize("lay", LAYOUTS, ids=lambda l: "%d-%d-%d" % l)
@timed
@gpu
def test_ragged_shards_with_a_last_shard_of_one_particle(pkg, lay):
    """8 frames from the empty corridor map on virtual ranks with an explicit stride against O.Slam of the global size: every rank's pose
    and trace every frame, the concatenated particles and every rank's map at the end, pfslam_estimate on every rank behind hand-made
    all-gathers of buffers 5 -> 10 and 16 -> 17.  Shards of 64 particles and below never run round-5 frames; the others do."""
    torch = pytest.importorskip("torch")
    n, world, stride = lay
    scans = corridor(pkg, 8)
    with environ(ORC_THREADS="16"):
        o = O.Slam(n, kd_capacity=1 << 16)
        v = _VirtualRanks(pkg, torch, n, world, stride=stride, kd_capacity=1 << 16)
        assert [cnt for _, _, cnt in v.lay][-1] == 1 and sum(cnt for _, _, cnt in v.lay) == n
        flags, r5 = set(), [[] for _ in range(world)]
        for f, scan in enumerate(scans, start=1):
            o.step(f, scan)
            v.step(f, scan)
            want = row_of(o)
            for r, e in enumerate(v.engs):
                got = row_of(e)
                assert got == want, "%s frame %d rank %d: %s vs the oracle's %s" % (lay, f, r, got, want)   # (frame 1 seeds the map)
                r5[r].append(e.frame_mode()["round5_frame"])
            flags.add(want[1])
    assert flags == {0, 1}, flags
    for r, (_, _, cnt) in enumerate(v.lay):
        if cnt <= WAVE:
            assert not any(r5[r]), (lay, r, r5)
        else:   # the first scored frame starts from a cloud of no spread: cell rows, a round-5 frame; later ones while the cloud is narrow enough
            assert not r5[r][0] and r5[r][1], (lay, r, r5)
    got = [e.particles() for e in v.engs]
    assert_same_particles({fld: np.concatenate([g[fld] for g in got]) for fld in FIELDS}, o.particles(), "ranks of %s" % (lay,))
    for e in v.engs:
        assert e.map().tobytes() == o.tree().tobytes()
    gather_by_hand(v)
    want16 = E.estimate_particles(o.particles())
    for r, e in enumerate(v.engs):
        same16(e.estimate_raw(), want16, "%s rank %d" % (lay, r))
    print("%s: round-5 frames per rank of 7 stepped: %s" % (lay, [sum(x) for x in r5]))
    v.close(); o.close()
