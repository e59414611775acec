"""pfslam_search on the GPU against its restatement (tests/search_ref.py): the winner's pose and the eight info floats bit for bit, the
score volume integer for integer -- for scans of 1 to 4096 beams, in both trigonometry modes, on every kind of tree, for windows whose
rows cross wave edges and whose workgroups outnumber the compute units, at both ends of qcap, for centres whose end points have no
cells and scans whose headings have no beams.  Then behind frames in flight (it must read and change nothing), after its buffers grew
and the map was replaced, on sharded handles, through the replay binary, its refusals, and the scenario it was made for: search, then
pfslam_register from the winner.

There is no tolerance anywhere in this file but the scenario's one map cell and one beam step."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import register_batch_ref as B
import register_ref as R
import search_ref as S
from test_gpu_sharded import _VirtualRanks
from test_host_layer import HOST, SCENE_TXT, build_host

pytestmark = pytest.mark.gpu
CENTRE = np.array([0.6, 0.22, 0.13], np.float32)     # 0.10 m / 0.03 rad off the pose the scan was cast from
SMALL = dict(half_x=2, half_y=2, half_theta=1)


@pytest.fixture(scope="module")
def world(pkg):
    tree, segs, _ = R.planar_tree(4000, seed=1)
    trees = {"p4000": tree, "np300": R.nonplanar_tree(300), "grown4500": R.grown_tree(4000, 500, seed=1)[0]}
    return {"trees": trees, "fields": {k: S.Field(t) for k, t in trees.items()}, "scan": pkg.synth.make_scan(segs, (0.5, 0.3, 0.1), seed=7), "segs": segs}


def handle(pkg, world, name="p4000", nb=1081, scan=None):
    h = pkg.PfSlam(64, n_beams=nb, kd_capacity=1 << 16)
    h.set_map(world["trees"][name])
    if scan is None:
        scan = np.resize(world["scan"], nb) if nb != 1081 else world["scan"]
    h.set_scan(scan)
    return h, np.ascontiguousarray(scan, np.float32)


def device_targets(h):
    """register_ref.targets as the handle's ICP stage computes them in its current trigonometry mode (buffer 11 after pfslam_icp: the
    targets (x + wx, y + wy, 0, 4) of the in-range beams, zeros for the others): what the restatement stands on in the device-library
    mode, which the CPU oracle does not have."""
    torch = pytest.importorskip("torch")
    sharded = importlib.import_module("gpu-icp-slam_amd.sharded")

    def targets(scan, pose):
        h.set_pose(np.array(pose, np.float32))          # (the stage casts the scan from the handle's pose)
        h.icp(np.array(pose, np.float32))
        ptr, nbytes = h.device_ptr(11)
        t = torch.as_tensor(sharded._DevView(ptr, nbytes, "<f4", 4), device=torch.device("cuda", 0)).cpu().numpy().reshape(-1, 4)
        return np.ascontiguousarray(t[:, :3]), t[:, 3] != 0
    return targets


def assert_search(h, field, scan, centre, what="", targets=None, **opts):
    got = h.search(centre, scores=True, **opts)
    want = S.search(field, scan, centre, targets, **opts)
    diff = S.same_result(got, want)
    assert diff is None, "%s %r: %s" % (what, opts, diff)
    for k in ("status", "index", "beams", "score", "candidates", "qcap"):
        assert got[k] == want[k], k
    return got


# ---- 1. the volume ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 65, 1025, 4096])
def test_winner_info_and_volume_equal_the_restatement_in_both_trig_modes(pkg, world, nb):
    h, scan = handle(pkg, world, nb=nb)
    for trig in (0, 1):
        h.set_trig(trig)
        got = assert_search(h, world["fields"]["p4000"], scan, CENTRE, "beams %d trig %d" % (nb, trig), device_targets(h) if trig else None, **SMALL)
        assert got["status"] == 0 and got["scores"].shape == (3, 5, 5) and got["beams"] >= 1
    h.close()


@pytest.mark.parametrize("name", ["p4000", "np300", "grown4500"])
def test_volume_on_every_kind_of_tree(pkg, world, name):
    """np300 is non-planar: the field is still that of z = 0 queries."""
    h, scan = handle(pkg, world, name)
    got = assert_search(h, world["fields"][name], scan, CENTRE, name, max_dist=0.5 if name == "np300" else 0.2, **SMALL)
    assert got["status"] == 0 and (got["scores"] < got["qcap"] * got["beams"]).any()
    nothing = np.zeros(3, np.float32), np.zeros(8, np.float32)
    o = pkg.binding.SearchOpts()
    h.L.pfslam_search_default_opts(C.byref(o))
    o.half_x, o.half_y, o.half_theta = 2, 2, 1
    o.max_dist = 0.5 if name == "np300" else 0.2
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert h.L.pfslam_search(h._h, vp(CENTRE), C.byref(o), vp(nothing[0]), vp(nothing[1]), None) == 0      # scores may be NULL
    assert (R.bits(nothing[0]) == R.bits(got["pose"])).all() and (R.bits(nothing[1]) == R.bits(got["info"])).all()
    h.close()


# ---- 2. window shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(half_x=0, half_y=0, half_theta=0), dict(half_x=32, half_y=1, half_theta=1), dict(half_x=64, half_y=2, half_theta=0),
                                  dict(half_x=35, half_y=1, half_theta=0, stride=3), dict(half_x=4, half_y=4, half_theta=64, step_theta=0.002)],
                         ids=["1x1x1", "65x3x3", "129x5x1", "71x3x1-stride3", "9x9x129"])
def test_windows_whose_rows_cross_wave_edges_and_whose_workgroups_outnumber_the_compute_units(pkg, world, opts):
    """65- and 129-wide rows put a row's end in the first lane of a wave; 9 x 9 x 129 is 258 workgroups of one wave (two per heading: 64
    candidates and 17), more than the 256 compute units.  65 beams keep the restatement of up to 10 449 candidates short."""
    h, scan = handle(pkg, world, nb=65)
    got = assert_search(h, world["fields"]["p4000"], scan, CENTRE, "window", **opts)
    assert got["candidates"] == got["scores"].size <= 20000
    h.close()


def test_a_41_x_41_x_33_window_on_a_sample_of_2000_candidates_and_on_the_winner(pkg, world):
    """The default window, 55 473 candidates of 257 beams: the restatement scores a random sample and the winner; that the winner is the
    smallest score of the device's volume, the lowest k among equal ones, is read off the volume itself."""
    h, scan = handle(pkg, world, nb=257)
    got = h.search(CENTRE, scores=True)
    s = S.Search(world["fields"]["p4000"], scan, CENTRE)
    assert got["candidates"] == s.cand == 41 * 41 * 33 and got["scores"].shape == (33, 41, 41)
    flat = got["scores"].ravel()
    ks = np.random.RandomState(11).choice(s.cand, 2000, replace=False)
    want = s.scores_at(ks)
    assert (flat[ks] == want).all(), "%d of 2000 sampled scores differ" % (flat[ks] != want).sum()
    k = got["index"]
    assert k == int(flat.argmin()) and got["score"] == flat[k] == s.scores_at([k])[0]
    pose, info = s.result_of(int(flat[k]), k)
    assert (R.bits(got["pose"]) == R.bits(pose)).all() and (R.bits(got["info"]) == R.bits(info)).all()
    h.close()


# ---- 3. saturation ---------------------------------------------------------------------------------------------------------------------------
def test_qcap_of_1_and_of_65535_centres_without_cells_and_headings_without_beams(pkg, world):
    h, scan = handle(pkg, world, nb=65)
    f = world["fields"]["p4000"]
    lo = assert_search(h, f, scan, CENTRE, "qcap 1", max_dist=0.0045, half_x=3, half_y=3, half_theta=1)
    assert lo["qcap"] == 1 and lo["scores"].max() <= 65 and (lo["scores"].ravel() == lo["scores"].min()).sum() >= 2 and \
        lo["index"] == np.flatnonzero(lo["scores"].ravel() == lo["scores"].min())[0]               # a tie: the lowest k
    hi = assert_search(h, f, scan, np.array([3.0, 2.0, 0.13], np.float32), "qcap 65535", max_dist=1.59999, **SMALL)
    assert hi["qcap"] == 65535 and hi["scores"].max() > 65535 and (hi["scores"] < hi["qcap"] * hi["beams"]).any()
    assert (hi["scores"] % 65535 != 0).any()                                        # (not every beam is saturated or on a node)
    top = assert_search(h, f, scan, np.array([1000.0, 1000.0, 0.0], np.float32), "qcap 65535, saturated", max_dist=1.59999, half_x=1, half_y=1, half_theta=0)
    assert (top["scores"] == 65535 * top["beams"]).all()
    # a centre far from the map: every cell of the field saturates; a centre beyond 2^20 cells: no end point has a cell
    for centre in ((1000.0, 1000.0, 0.0), (30000.0, 0.22, 0.13), (0.6, -3.0e38, 0.13)):
        got = assert_search(h, f, scan, np.array(centre, np.float32), "centre %r" % (centre,), half_x=1, half_y=1, half_theta=0)
        assert got["status"] == 0 and got["index"] == 0 and (got["scores"] == 1024 * got["beams"]).all()
    # 26 km out, just inside +-2^20 cells, with a box more than 2048 cells wide: cell index times box width passes 2^31 -- the field is
    # indexed relative to the box, never by such a product
    got = assert_search(h, f, scan, np.array([0.6, 26000.0, 0.13], np.float32), "26 km", half_x=17, half_y=1, half_theta=0, stride=64)
    assert got["status"] == 0 and got["index"] == 0 and (got["scores"] == 1024 * got["beams"]).all() and got["beams"] == 65
    # a window that starts on the map and ends 20 m off it
    got = assert_search(h, f, scan, CENTRE, "wide", half_x=12, half_y=0, half_theta=0, stride=64)
    assert got["scores"].shape == (1, 1, 25) and got["scores"][0, 0, 12] < 1024 * got["beams"]
    # ranges that are rejected everywhere (status 2), and everywhere but at one heading
    far = np.full(65, 1000.0, np.float32)
    h.set_scan(far)
    opts = dict(half_x=1, half_y=1, half_theta=1, step_theta=0.3)
    got = assert_search(h, f, far, CENTRE, "status 2", **opts)
    assert got["status"] == 2 and got["index"] == -1 and (got["scores"] == S.NONE).all() and (R.bits(got["pose"]) == R.bits(CENTRE)).all()
    far[0] = 28.0        # beam 0 looks along -135 degrees + theta: inside the +-20 m square only within 0.6 degrees of the diagonal
    h.set_scan(far)
    got = assert_search(h, f, far, np.array([0.6, 0.22, 0.0], np.float32), "one heading", **opts)
    assert got["status"] == 0 and got["beams"] == 1 and (got["scores"][0] == S.NONE).all() and (got["scores"][2] == S.NONE).all() and 9 <= got["index"] < 18
    h.close()


def test_4096_beams_at_qcap_65535_reach_the_largest_score_the_header_allows(pkg, world):
    """S <= 4096 * 65535 < 2^31: every beam of a 4096-beam scan in range, every cell saturated at the top of the uint16 range; and the
    same handle on the map, where the scores are mixed."""
    scan = np.full(4096, 5.0, np.float32)
    h, _ = handle(pkg, world, nb=4096, scan=scan)
    f = world["fields"]["p4000"]
    got = assert_search(h, f, scan, np.array([1000.0, 1000.0, 0.0], np.float32), "4096 x 65535", max_dist=1.59999, half_x=1, half_y=1, half_theta=1)
    assert got["qcap"] == 65535 and got["beams"] == 4096 and (got["scores"] == 4096 * 65535).all() and got["score"] == 268431360 and got["index"] == 0
    got = assert_search(h, f, scan, CENTRE, "4096 beams on the map", max_dist=1.59999, **SMALL)
    assert got["qcap"] == 65535 and len(np.unique(got["scores"])) > 1
    h.close()


# ---- 4. its buffers and the map ----------------------------------------------------------------------------------------------------------------
def test_buffers_grow_from_a_small_call_to_a_large_one_and_a_replaced_map_is_the_one_read(pkg, world):
    h, scan = handle(pkg, world, nb=65)
    f = world["fields"]
    first = assert_search(h, f["p4000"], scan, CENTRE, "small", half_x=0, half_y=0, half_theta=0)
    assert_search(h, f["p4000"], scan, CENTRE, "large", half_x=40, half_y=6, half_theta=5, stride=2)     # field, end points, counts and volume all grow
    again = assert_search(h, f["p4000"], scan, CENTRE, "small again", half_x=0, half_y=0, half_theta=0)    # (the larger buffers serve a smaller call)
    assert S.same_result(first, again) is None
    small = assert_search(h, f["p4000"], scan, CENTRE, "5 x 5 x 3", **SMALL)
    h.set_map(world["trees"]["np300"])
    other = assert_search(h, f["np300"], scan, CENTRE, "replaced map", max_dist=0.5, **SMALL)
    assert not (other["scores"] == small["scores"]).all()
    h.set_scan(scan[::-1].copy())
    assert_search(h, f["np300"], scan[::-1].copy(), CENTRE, "replaced scan", max_dist=0.5, **SMALL)
    h.close()


# ---- 5. read-only --------------------------------------------------------------------------------------------------------------------------------
def test_search_behind_frames_in_flight_reads_and_changes_nothing(pkg):
    torch = pytest.importorskip("torch")
    sharded = importlib.import_module("gpu-icp-slam_amd.sharded")

    def buffers(e):
        out = []
        for which in (11, 12):
            ptr, nbytes = e.device_ptr(which)
            t = torch.as_tensor(sharded._DevView(ptr, nbytes, "<i4", 4), device=torch.device("cuda", 0))
            out.append(t.cpu().numpy().tobytes())
        return out

    n = 1000
    _, frames = pkg.synth.corridor_sequence(9, seed=5)
    h, twin = pkg.PfSlam(n, kd_capacity=1 << 16), pkg.PfSlam(n, kd_capacity=1 << 16)
    seen = []
    for f, (_, scan) in enumerate(frames, start=1):
        h.step(f, scan)
        twin.step(f, scan)
        if f in (4, 7):                                  # a frame is in flight (default lag): search books it first
            first = h.search(None, scores=True, half_x=1, half_y=1, half_theta=1)      # centre NULL: the pose of the frame just booked
            field = S.Field(h.map())
            want = S.search(field, scan, h.pose, half_x=1, half_y=1, half_theta=1)
            assert S.same_result(first, want) is None, (f, S.same_result(first, want))
            centre = (h.pose.astype(np.float64) + (0.05, -0.05, 0.02)).astype(np.float32)
            seen.append(assert_search(h, field, scan, centre, "frame %d" % f, half_x=3, half_y=2, half_theta=1, stride=2))
            h.search(centre)                                                             # the default window, no volume
            assert (R.bits(h.pose) == R.bits(twin.pose)).all()
            assert buffers(h) == buffers(twin), "buffers 11 / 12 after frame %d" % f
            assert h.check_cells()["violations"] == 0
    assert len(seen) == 2 and all(s["status"] == 0 for s in seen)
    assert (R.bits(h.pose) == R.bits(twin.pose)).all()
    ph, pt = h.particles(), twin.particles()
    for fld in ("x", "y", "theta", "w"):
        assert (R.bits(ph[fld]) == R.bits(pt[fld])).all(), fld
    assert h.map().tobytes() == twin.map().tobytes()
    assert buffers(h) == buffers(twin)
    assert h.check_cells()["violations"] == 0 and twin.check_cells()["violations"] == 0
    h.close(); twin.close()


# ---- 6. wrappers -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_every_rank_of_a_sharded_job_gets_the_unsharded_bits(pkg, nranks):
    torch = pytest.importorskip("torch")
    n = 1000
    kw = dict(kd_capacity=1 << 16)
    one = pkg.PfSlam(n, **kw)
    v = _VirtualRanks(pkg, torch, n, nranks, **kw)
    _, frames = pkg.synth.corridor_sequence(5, seed=5)
    for f, (_, scan) in enumerate(frames, start=1):
        one.step(f, scan)
        v.step(f, scan)
    v._sync()
    centre = (np.array(one.pose, np.float64) + (0.05, -0.05, 0.02)).astype(np.float32)
    opts = dict(half_x=6, half_y=4, half_theta=2)
    want = one.search(centre, scores=True, **opts)
    assert want["status"] == 0
    for r, e in enumerate(v.engs):
        diff = S.same_result(e.search(centre, scores=True, **opts), want)
        assert diff is None, "rank %d of %d: %s" % (r, nranks, diff)
    assert S.same_result(want, S.search(S.Field(one.map()), frames[-1][1], centre, **opts)) is None
    v.close(); one.close()


def test_sharded_wrapper_passes_search_through_without_a_collective(pkg):
    torch = pytest.importorskip("torch")
    sharded = importlib.import_module("gpu-icp-slam_amd.sharded")
    a = pkg.PfSlam(500, kd_capacity=1 << 16)
    s = sharded.ShardedSlam(pkg, 500, 0, 1, device=0, torch=torch, kd_capacity=1 << 16)
    _, frames = pkg.synth.corridor_sequence(4, seed=7)
    for f, (_, scan) in enumerate(frames, start=1):
        a.step(f, scan)
        s.step(f, scan)
    issued = s.collectives
    centre = (np.array(a.pose, np.float64) + (0.05, -0.05, 0.02)).astype(np.float32)
    assert S.same_result(s.search(centre, scores=True, half_x=5, half_y=5, half_theta=2), a.search(centre, scores=True, half_x=5, half_y=5, half_theta=2)) is None
    assert S.same_result(s.search(centre), a.search(centre), volume=False) is None and s.collectives == issued
    a.close(); s.eng.close()


def test_replay_binary_with_search_1_prints_the_handle_s_winner(tmp_path, pkg):
    """pfslamSearch (host/kernel.h) through `pfslam_replay ... search=1`: one line per frame with the candidate the library picks in the
    default window around the frame's pose and that candidate's pose, whose float bits are the C-ABI's."""
    build_host(pkg)
    _, frames = pkg.synth.corridor_sequence(6, seed=5)
    scene = tmp_path / "scene.txt"
    scene.write_text(SCENE_TXT)
    scans = np.stack([np.zeros(1081, np.float32)] + [s for _, s in frames])  # scans[0] is never used (frame starts at 1)
    lidar = tmp_path / "lidar.f32"
    scans.astype(np.float32).tofile(str(lidar))
    env = dict(os.environ, PFSLAM_PARTICLES="300", PFSLAM_KD_CAPACITY=str(1 << 16))
    out = subprocess.check_output([os.path.join(HOST, "pfslam_replay"), str(scene), str(lidar), "search=1"], env=env).decode()
    lines = [l for l in out.splitlines() if l.startswith("search ")]
    assert len(lines) == len(frames)
    h = pkg.PfSlam(300, kd_capacity=1 << 16)
    for f, ((_, scan), line) in enumerate(zip(frames, lines), start=1):
        h.step(f, scan)
        got = h.search(h.pose)
        tok = line.split()
        assert tok[1] == str(f) and tok[2] == "index" and int(tok[3]) == got["index"] and got["index"] >= 0, line
        assert tok[4] == "pose" and tok[8] == "bits" and len(tok) == 12, line
        assert [int(v, 16) for v in tok[9:12]] == got["pose"].view(np.uint32).tolist(), line
    h.close()
    out = subprocess.check_output([os.path.join(HOST, "pfslam_replay"), str(scene), str(lidar)], env=env).decode()
    assert not [l for l in out.splitlines() if l.startswith("search ")]


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_leave_the_outputs_and_the_handle_goes_on(pkg, world):
    h = pkg.PfSlam(64, kd_capacity=1 << 16)
    with pytest.raises(pkg.PfSlamError, match="pfslam_search: no map loaded"):
        h.search(CENTRE)
    h.set_map(world["trees"]["p4000"])
    h.set_scan(world["scan"])
    bad_opts = (dict(half_x=-1), dict(half_y=-1), dict(half_theta=-1), dict(stride=0), dict(stride=65), dict(step_theta=float("nan")),
                dict(step_theta=0.0), dict(step_theta=-0.01), dict(max_dist=0.0), dict(max_dist=float("inf")), dict(max_dist=float("nan")),
                dict(max_dist=0.004), dict(max_dist=1.6), dict(max_dist=1.60001), dict(half_x=2048, half_y=2048, half_theta=0), dict(half_x=0, half_y=0, half_theta=1 << 23),
                dict(half_x=0, half_y=0, half_theta=8000), dict(half_x=1000, half_y=0, half_theta=0, stride=64))
    for bad in bad_opts:
        cause = S.refusal(1081, CENTRE, **bad)
        assert cause is not None, bad
        with pytest.raises(pkg.PfSlamError, match="pfslam_search: .*%s" % cause.replace("^", r"\^").replace("(", r"\(").replace(")", r"\)")):
            h.search(CENTRE, **bad)
    assert h.search(CENTRE, half_theta=0, step_theta=0.0, **{k: v for k, v in SMALL.items() if k != "half_theta"})["status"] == 0   # no heading step needed
    for c in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)):
        with pytest.raises(pkg.PfSlamError, match="pfslam_search: the centre must be finite"):
            h.search(np.array(c, np.float32))
    with pytest.raises(TypeError):
        h.search(CENTRE, reserved_=1)
    for short in (CENTRE[:2], np.zeros(4, np.float32), []):
        with pytest.raises(ValueError, match="centre must be"):
            h.search(short)

    # through the C-ABI: every refusal returns non-zero and writes no output
    pose, info, vol = np.full(3, 7.5, np.float32), np.full(8, 7.5, np.float32), np.full(75, 77, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def options(**kw):
        o = pkg.binding.SearchOpts()
        h.L.pfslam_search_default_opts(C.byref(o))
        for k, v in dict(SMALL, **kw).items():
            if k == "reserved_":
                o.reserved_[1] = v
            else:
                setattr(o, k, v)
        return o

    good = options()

    def call(c=CENTRE, o=good, p=pose, i=info, handle=None):
        return h.L.pfslam_search(h._h if handle is None else handle, None if c is None else vp(c), None if o is None else C.byref(o),
                                 None if p is None else vp(p), None if i is None else vp(i), vp(vol))

    def untouched():
        return (pose == 7.5).all() and (info == 7.5).all() and (vol == 77).all()

    assert h.L.pfslam_search(None, vp(CENTRE), C.byref(good), vp(pose), vp(info), vp(vol)) != 0 and "bad argument" in h.L.pfslam_last_error().decode()
    for kw, cause in ((dict(o=None), "bad argument"), (dict(p=None), "bad argument"), (dict(i=None), "bad argument"),
                      (dict(o=options(reserved_=1)), "reserved_ must be 0"), (dict(o=options(stride=65)), "stride"), (dict(o=options(max_dist=1.6)), "1 .. 65535"),
                      (dict(o=options(half_x=1 << 30)), "2^24 candidates"), (dict(c=np.array([0, np.nan, 0], np.float32)), "centre must be finite")):
        assert call(**kw) != 0, kw
        assert cause in h.L.pfslam_last_error().decode(), (kw, h.L.pfslam_last_error())
        assert untouched(), "an output was written: %r" % (kw,)
    empty = pkg.PfSlam(64, kd_capacity=1 << 16)
    assert call(handle=empty._h) != 0 and "no map loaded" in h.L.pfslam_last_error().decode() and untouched()
    empty.close()
    oblong = pkg.PfSlam(64, kd_capacity=1 << 16, map_scale=(40.0, 80.0), map_res=(0.025, 0.05))     # (as many cells in x as in y)
    oblong.set_map(world["trees"]["p4000"])
    assert call(handle=oblong._h) != 0 and "map_res_x != map_res_y" in h.L.pfslam_last_error().decode() and untouched()
    oblong.close()
    h.set_pose(np.array([np.nan, 0.0, 0.0], np.float32))
    assert call(c=None) != 0 and "must be finite" in h.L.pfslam_last_error().decode() and untouched()
    with pytest.raises(pkg.PfSlamError, match="at most 4096 beams"):   # (no handle can hold more: the refusal of n_beams > 4096 cannot
        pkg.PfSlam(64, n_beams=4097, kd_capacity=1 << 16)             #  be reached through pfslam_create)
    assert call() == 0 and not untouched()
    want = S.search(world["fields"]["p4000"], world["scan"], CENTRE, **SMALL)
    assert S.same_result(S.result_dict(pose, info, vol.reshape(3, 5, 5)), want) is None
    h.set_pose(CENTRE)
    assert S.same_result(h.search(None, scores=True, **SMALL), want) is None           # centre NULL: the handle's pose
    h.close()


# ---- 8. the scenario -------------------------------------------------------------------------------------------------------------------------------
def test_the_scenario_search_then_register_meets_the_bound_from_all_26_centres(pkg, world):
    """What the feature is for (tests/test_search_spec.py): from (10, -8, 0.3) pfslam_register alone ends at the pose from 6 of 27 starts."""
    p = B.SCENARIO_POSES[1]
    scan = pkg.synth.make_scan(world["segs"], p, seed=7)
    h, _ = handle(pkg, world, scan=scan)
    window = dict(half_x=10, half_y=10, half_theta=16, stride=2, step_theta=0.0125)
    ok = alone = 0
    for centre in B.scenario_starts(p):
        got = h.search(centre, **window)
        err = np.abs(got["pose"].astype(np.float64) - np.array(p))
        assert got["status"] == 0 and err[0] <= 2 * B.CELL and err[1] <= 2 * B.CELL and err[2] <= 0.0125, (centre, err)
        reg = h.register(got["pose"], max_iters=20)
        inside, e2 = B.within_bounds(reg["pose"], p)
        assert inside, (centre, e2)
        ok += inside
        alone += B.within_bounds(h.register(centre, max_iters=20)["pose"], p)[0]
    # the restatement's winner from one centre, bit for bit (tests/test_search_spec.py holds the restatement to the bound)
    centre = B.scenario_starts(p)[12]
    want = S.search(world["fields"]["p4000"], scan, centre, **window)
    assert S.same_result(h.search(centre, scores=True, **window), want) is None
    print("search then register: %d of 26 centres meet the bound; pfslam_register alone: %d of 26" % (ok, alone))
    assert ok == 26
    h.close()
