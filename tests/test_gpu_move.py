"""pfslam_move_particles on the GPU: the stage on uploaded clouds against the restatement (tests/move_ref.py, held to the header by
tests/test_move_spec.py) bit for bit, also at the edges of its inputs (section 1b), the device-library trigonometry within an ulp of it,
sharded handles, the ordering behind frames in flight in every frame mode, the heading bound, the refusals and the C++ host layer.
Frames with moves against the CPU oracle are in tests/test_gpu_move_frames.py.

Apart from the device-library case, whose bound is derived in its docstring, every comparison is bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import move_ref as M
from test_gpu_sharded import _VirtualRanks
from test_host_layer import HOST, SCENE_TXT, build_host

pytestmark = pytest.mark.gpu
FIELDS = ("x", "y", "theta", "w")
F = np.float32
FRAME, REF_THETA = 9, 0.7
DELTA = np.array([0.31, -0.07, 0.045], F)
OPTS = dict(cov_scale=1.5, sigma_xy_min=0.007, sigma_theta_min=0.0036)
POSE = np.array([11.5, 9.25, REF_THETA + 0.13], F)
# the frames-in-flight drives: a full covariance of a centimetre, so that the filter keeps its track
SMALL = dict(cov_scale=0.01, sigma_xy_min=0.002, sigma_theta_min=0.0005)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_particles(got, want, what=""):
    for fld in FIELDS:
        assert (bits(got[fld]) == bits(want[fld])).all(), (what, fld, np.flatnonzero(bits(got[fld]) != bits(want[fld]))[:8])


def staged(pkg, n, p, trig=0):
    """A handle with the cloud p and POSE uploaded, moved once: (particles, pose)."""
    h = pkg.PfSlam(n)
    h.set_trig(trig)
    h.set_particles(p)
    h.set_pose(POSE)
    h.move_particles(FRAME, DELTA, M.CORRIDOR_COV, REF_THETA, **OPTS)
    out = h.particles(), np.array(h.pose, F)
    h.close()
    return out


# ---- 1. the stage ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 255, 256, 257, 1000])
def test_stage_equals_the_restatement(pkg, n):
    """Below, at and above the 64 lanes of a wave and the 256 threads of a workgroup; headings ref_theta +- 0.2 rad, a full covariance, a
    scale and both floors.  Particles and pose bit for bit; the weights are untouched."""
    x, y, th, w = M.cloud(n, REF_THETA, seed=1)
    got, pose = staged(pkg, n, M.particles_of(x, y, th, w))
    wx, wy, wt = M.move(x, y, th, FRAME, DELTA, M.CORRIDOR_COV, REF_THETA, **OPTS)
    same_particles(got, M.particles_of(wx, wy, wt, w), "n %d" % n)
    assert not (bits(got["x"]) == bits(x)).any()
    assert (bits(pose) == bits(M.move_pose(POSE, DELTA, M.CORRIDOR_COV, REF_THETA, **OPTS))).all()


def test_the_statistics_case_bit_for_bit(pkg):
    """The 65 536 draws whose second moments tests/test_move_spec.py holds to six standard errors of the covariance: particles at the origin
    with heading 0 = ref_theta ARE (mx, my, mt), so the GPU inherits that check bit for bit."""
    L, a, mx, my, mt = M.stat_case()
    n = M.STAT_N
    h = pkg.PfSlam(n)
    zero = np.zeros(n, F)
    h.set_particles(M.particles_of(zero, zero, zero, np.ones(n, F)))
    h.move_particles(M.STAT_FRAME, M.STAT_DELTA, M.CORRIDOR_COV)
    same_particles(h.particles(), M.particles_of(mx, my, mt, np.ones(n, F)))
    h.close()


def test_stage_with_the_device_library_is_within_an_ulp(pkg):
    """pfslam_set_trig(1): the device library's sinf / cosf and rocThrust's form of the normal draw.  Positions in [8.5, 15.5) and
    increments below 0.5 m keep every result in [8, 16), where an ulp is 2^-20 = 9.5e-7.  The two modes' s, c and z differ by at most 2 ulp
    each (the library's sinf / cosf are within 1 ulp of the truth, the specification's are correctly rounded but for 1e-8 of arguments;
    the two forms of the draw round once and twice), so c within 1.2e-7, s <= 0.2 within 3e-8, mx and my (< 0.5) within 6e-8 plus the
    roundings of their sums, 3e-8 each.  The increment c mx - s my then differs by at most
        |dc| |mx| + |c| |dmx| + |ds| |my| + |s| |dmy| + three roundings of values < 0.5
        = 6e-8 + 9e-8 + 1.5e-8 + 1.8e-8 + 9e-8 = 2.7e-7 < half an ulp of the result (4.8e-7),
    and two sums x + inc whose addends differ by less than half an ulp round to the same float or to neighbours: <= 1 ulp.  Headings are in
    [0.5, 0.9], ulp 6e-8, and mt (< 0.06) differs by a few 1e-9: <= 1 ulp as well.  The pose has no draw: the same bound."""
    n = 1000
    rng = np.random.RandomState(5)
    x, y = rng.uniform(8.5, 15.5, n).astype(F), rng.uniform(8.5, 15.5, n).astype(F)
    th = (REF_THETA + rng.uniform(-0.2, 0.2, n)).astype(F)
    w = np.ones(n, F)
    p = M.particles_of(x, y, th, w)
    opts = dict(cov_scale=0.04)
    Lf, _ = M.factor(M.CORRIDOR_COV, **opts)
    mx, my, mt = M.increments(M.draws(FRAME, np.arange(n)), DELTA, Lf)
    assert np.abs(mx).max() < 0.5 and np.abs(my).max() < 0.5 and np.abs(mt).max() < 0.06
    res = {}
    for trig in (0, 1):
        h = pkg.PfSlam(n)
        h.set_trig(trig)
        h.set_particles(p)
        h.set_pose(POSE)
        h.move_particles(FRAME, DELTA, M.CORRIDOR_COV, REF_THETA, **opts)
        res[trig] = (h.particles(), np.array(h.pose, F))
        h.close()
    wx, wy, wt = M.move(x, y, th, FRAME, DELTA, M.CORRIDOR_COV, REF_THETA, **opts)
    same_particles(res[0][0], M.particles_of(wx, wy, wt, w), "trig 0")
    worst = 0
    for fld in ("x", "y", "theta"):
        d = np.abs(bits(res[1][0][fld]).astype(np.int64) - bits(res[0][0][fld]).astype(np.int64))
        print("%s: %d of %d differ, largest %d ulp" % (fld, (d != 0).sum(), n, d.max()))
        worst = max(worst, int(d.max()))
    dp = np.abs(bits(res[1][1]).astype(np.int64) - bits(res[0][1]).astype(np.int64))
    print("pose: %s ulp" % dp.tolist())
    assert worst <= 1 and dp.max() <= 1
    assert (bits(res[1][0]["w"]) == bits(w)).all()


# ---- 1b. the stage's inputs at their edges (the same set runs the kernel text on the CPU: tests/test_move_kernel_text.py) --------------------
EDGES = M.edge_cases()


def staged_edge(pkg, k, x=None, th=None):
    """One call on a fresh handle with the case's cloud and pose uploaded: (particles, pose)."""
    kw = dict(M.EDGE_SHARD) if k["goff"] else {}
    assert kw.get("global_offset", 0) == k["goff"]
    h = pkg.PfSlam(k["n"], **kw)
    h.set_particles(M.particles_of(k["x"] if x is None else x, k["y"], k["th"] if th is None else th, k["w"]))
    h.set_pose(k["pose"])
    h.move_particles(k["frame"], k["delta"], k["cov"], k["ref_theta"], **k["opts"])
    out = h.particles(), np.array(h.pose, F)
    h.close()
    return out


@pytest.mark.parametrize("name", sorted(EDGES))
def test_stage_at_the_edges_of_its_inputs(pkg, name):
    """257 particles (65 for the shard) against the restatement bit for bit: headings +-pi around ref_theta; |phi| near 100 and 1100 rad
    with headings and ref_theta of opposite sign; ref_theta of +-1000; positions in [-2000, 2000) and below 1e-3; a first pivot of exactly
    0, a rank-1 covariance (p1 = p2 = 0) and cov_scale 0 with sigma_theta_min alone; frames 0, 1 and 4 194 303; and the last shard of a
    job of 2^24 + 64 particles, whose global indices 16 777 215 .. 16 777 279 cross 2^24."""
    k = EDGES[name]
    got, pose = staged_edge(pkg, k)
    wx, wy, wt, wpose = M.edge_want(k)
    same_particles(got, M.particles_of(wx, wy, wt, k["w"]), name)
    assert (bits(pose) == bits(wpose)).all(), (name, pose, wpose)
    moved = bits(got["theta"]) != bits(k["th"])
    assert moved.sum() >= k["n"] - 2, name                      # (every heading got its increment, but for one that rounds away)


def test_stage_without_noise_is_the_shift_on_the_device(pkg):
    """cov NULL, zero floors, every heading equal to ref_theta: pfslam_shift_particles(delta) on a second handle, bit for bit, particles and
    pose; operands that are not signed zeros, and the restatement agrees with both."""
    n, ref = M.EDGE_N, F(0.83)
    x, y, _, w = M.cloud(n, seed=31)
    p = M.particles_of(x, y, np.full(n, ref, F), w)
    delta = np.array([0.5, -0.125, 0.07], F) + F(1e-3)
    pose = np.array([3.0, -2.0, ref], F)
    res = []
    for call in ("move", "shift"):
        h = pkg.PfSlam(n)
        h.set_particles(p)
        h.set_pose(pose)
        if call == "move":
            h.move_particles(5, delta, None, float(ref))
        else:
            h.shift_particles(delta)
        res.append((h.particles(), np.array(h.pose, F)))
        h.close()
    same_particles(res[0][0], res[1][0], "move against shift")
    assert (bits(res[0][1]) == bits(res[1][1])).all()
    wx, wy, wt = M.move(x, y, p["theta"], 5, delta, None, float(ref))
    same_particles(res[0][0], M.particles_of(wx, wy, wt, w), "move against the restatement")
    assert not (bits(res[0][0]["x"]) == bits(x)).any()


def test_a_particle_that_is_not_finite_stays_so_and_keeps_to_itself(pkg):
    """One particle has a NaN heading, another x = +inf: every field the NaN heading enters is NaN, x stays +inf and that particle's y and
    heading are the restatement's; all other particles and the pose equal the restatement bit for bit."""
    k = EDGES["headings all round"]
    th, x = k["th"].copy(), k["x"].copy()
    th[M.NAN_AT], x[M.INF_AT] = np.nan, np.inf
    got, pose = staged_edge(pkg, k, x=x, th=th)
    wx, wy, wt, wpose = M.edge_want(k)
    assert np.isnan(got["x"][M.NAN_AT]) and np.isnan(got["y"][M.NAN_AT]) and np.isnan(got["theta"][M.NAN_AT])
    assert np.isinf(got["x"][M.INF_AT]) and got["x"][M.INF_AT] > 0
    rest = np.ones(k["n"], bool)
    rest[M.NAN_AT] = False
    assert (bits(got["y"][rest]) == bits(wy[rest])).all() and (bits(got["theta"][rest]) == bits(wt[rest])).all()
    rest[M.INF_AT] = False
    assert (bits(got["x"][rest]) == bits(wx[rest])).all()
    assert (bits(got["w"]) == bits(k["w"])).all()
    assert (bits(pose) == bits(wpose)).all()


# ---- 2. sharded handles ------------------------------------------------------------------------------------------------------------------
def test_the_concatenated_shards_are_the_unsharded_cloud(pkg):
    """1001 particles over 3 virtual ranks (strides 334, 334, 333): only the global index enters the draw."""
    torch = pytest.importorskip("torch")
    n = 1001
    x, y, th, w = M.cloud(n, REF_THETA, seed=2)
    p = M.particles_of(x, y, th, w)
    want, want_pose = staged(pkg, n, p)
    wx, wy, wt = M.move(x, y, th, FRAME, DELTA, M.CORRIDOR_COV, REF_THETA, **OPTS)
    same_particles(want, M.particles_of(wx, wy, wt, w), "unsharded")
    v = _VirtualRanks(pkg, torch, n, 3)
    assert [cnt for _, _, cnt in v.lay] == [334, 334, 333]
    for e, (_, off, cnt) in zip(v.engs, v.lay):
        e.set_particles(p[off:off + cnt])
        e.set_pose(POSE)
        e.move_particles(FRAME, DELTA, M.CORRIDOR_COV, REF_THETA, **OPTS)
    got = np.concatenate([e.particles() for e in v.engs])
    same_particles(got, want, "3 ranks")
    for e in v.engs:
        assert (bits(e.pose) == bits(want_pose)).all()
    v.close()


# ---- 3. frames in flight -----------------------------------------------------------------------------------------------------------------
def drive(pkg, n, frames, mode, variant, moves, seed_frames=()):
    """A corridor drive from an empty map with a move before every frame from the second on and no getter in between.  mode: "default" (a
    frame in flight), "serial" (every launch on one stream) or "lag0" (every step books its frame, and the handle is synchronised before
    every move)."""
    h = pkg.PfSlam(n, kd_capacity=1 << 16)
    if variant is not None:
        h.set_variant(variant)
    if mode == "serial":
        h.set_serial(1)
    if mode == "lag0":
        h.set_lag(0)
    for f, (pose, scan) in enumerate(frames, start=1):
        if f in moves:
            if mode == "lag0":
                h.synchronize()
            delta, cov, kw = moves[f]
            h.move_particles(f, delta, cov, **kw)
        h.step(f, scan)
    out = dict(pose=np.array(h.pose, F), particles=h.particles(), map=h.map().tobytes(), rows=h.cell_stats()["rows"])
    h.close()
    return out


@pytest.mark.parametrize("variant", [None, 3])
def test_moves_between_frames_in_flight_in_every_frame_mode(pkg, variant):
    """3000 particles, 12 corridor frames, the commanded motion with a full covariance before every frame from the second on: the default
    handle (a frame in flight when the move is enqueued), the one-stream handle and the handle that books every frame and is synchronised
    before every move end with the same pose, particles and map.  With set_variant(3) the scan-match ran on the cell rows."""
    n, nframes = 3000, 12
    _, frames = pkg.synth.corridor_sequence(nframes, seed=5)
    moves = {}
    for f in range(2, nframes + 1):
        prev, cur = np.array(frames[f - 2][0], F), np.array(frames[f - 1][0], F)
        moves[f] = (cur - prev, M.CORRIDOR_COV, dict(ref_theta=float(prev[2]), **SMALL))
    res = {mode: drive(pkg, n, frames, mode, variant, moves) for mode in ("default", "serial", "lag0")}
    for mode in ("serial", "lag0"):
        assert (bits(res[mode]["pose"]) == bits(res["default"]["pose"])).all(), mode
        same_particles(res[mode]["particles"], res["default"]["particles"], mode)
        assert res[mode]["map"] == res["default"]["map"], mode
    assert len(res["default"]["map"]) > 32 * 1000
    if variant == 3:
        assert all(r["rows"] > 0 for r in res.values()), {m: r["rows"] for m, r in res.items()}
    # the moves are not a no-op: the same drive without them ends elsewhere
    still = drive(pkg, n, frames, "default", variant, {})
    assert not (bits(still["particles"]["x"]) == bits(res["default"]["particles"]["x"])).all()


def test_the_heading_bound_moves_with_the_call(pkg):
    """One move of 164 full turns between two frames in flight at 5000 particles on the cell rows (set_variant(3)): the host's bound on
    |heading| must pass 512 rad at once, or the scan-match kernel runs without the direct form of cos / sin beyond 1024 rad.  The handle
    that never takes the cell rows and books every frame (set_variant(2), set_lag(0)) gives the same bits."""
    n, nframes = 5000, 14
    _, frames = pkg.synth.corridor_sequence(nframes, seed=13)
    moves = {6: (np.array([0.0, 0.0, 164 * 2 * np.pi], F), M.CORRIDOR_COV, dict(ref_theta=0.0, **SMALL))}
    got = drive(pkg, n, frames, "default", 3, moves)
    want = drive(pkg, n, frames, "lag0", 2, moves)
    assert got["rows"] > 0 and want["rows"] == 0
    assert float(got["pose"][2]) > 1024.0
    assert (bits(got["pose"]) == bits(want["pose"])).all()
    same_particles(got["particles"], want["particles"])
    assert got["map"] == want["map"]


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_a_following_frame_is_unaffected(pkg):
    n = 300
    _, frames = pkg.synth.corridor_sequence(3, seed=5)
    h, twin = pkg.PfSlam(n, kd_capacity=1 << 16), pkg.PfSlam(n, kd_capacity=1 << 16)
    for e in (h, twin):
        e.step(1, frames[0][1])
    nan, inf = float("nan"), float("inf")
    good = np.array([0.02, 0.01, 0.004], F)
    bad = [
        (dict(delta=[nan, 0, 0]), "delta is not finite"),
        (dict(delta=[0, 0, inf]), "delta is not finite"),
        (dict(cov=[1, 0, 0, 1, nan, 1]), "cov is not finite"),
        (dict(ref_theta=inf), "ref_theta is not finite"),
        (dict(cov_scale=nan), "cov_scale is not finite"),
        (dict(sigma_xy_min=inf), "a floor is not finite"),
        (dict(sigma_theta_min=nan), "a floor is not finite"),
        (dict(cov_scale=-1.0), "cov_scale is negative"),
        (dict(sigma_xy_min=-0.001), "a floor is negative"),
        (dict(sigma_theta_min=-0.001), "a floor is negative"),
        (dict(cov=[-1e-6, 0, 0, 1, 0, 1]), "covariance is not positive semi-definite"),
        (dict(cov=[1, 2, 0, 1, 0, 1]), "covariance is not positive semi-definite"),
        (dict(cov=[1, 0, 0.9, 1, 0.9, 1]), "covariance is not positive semi-definite"),
        (dict(cov=[3e38, 0, 0, 1, 0, 1], cov_scale=2.0), "covariance is not positive semi-definite"),
        # the order: a value that is not finite is named before a negative one, a negative one before the pivot
        (dict(delta=[nan, 0, 0], cov_scale=-1.0), "delta is not finite"),
        (dict(cov=[-1, 0, 0, 1, 0, 1], sigma_xy_min=-1.0), "a floor is negative"),
    ]
    for kw, cause in bad:
        kw = dict(kw)
        delta = kw.pop("delta", good)
        with pytest.raises(pkg.PfSlamError, match="pfslam_move_particles: %s" % cause):
            h.move_particles(2, delta, **kw)
    # what the binding cannot express: a NULL delta or opts, a reserved_ that is not 0 (named behind the values, before the pivot)
    L, o = pkg.load(), pkg.binding.MoveOpts()
    L.pfslam_move_default_opts(C.byref(o))
    dp = good.ctypes.data_as(C.c_void_p)
    for args in ((h._h, 2, None, None, C.byref(o)), (h._h, 2, dp, None, None)):
        assert L.pfslam_move_particles(*args) != 0
        assert L.pfslam_last_error().decode() == "pfslam_move_particles: bad argument"
    for k in range(4):
        o.reserved_[k] = 1
        neg = np.array([-1, 0, 0, 1, 0, 1], F)
        assert L.pfslam_move_particles(h._h, 2, dp, neg.ctypes.data_as(C.c_void_p), C.byref(o)) != 0
        assert L.pfslam_last_error().decode() == "pfslam_move_particles: reserved_ must be 0"
        o.reserved_[k] = 0
    # nothing was enqueued: the next frame is the twin's
    for e in (h, twin):
        e.step(2, frames[1][1])
    assert (bits(h.pose) == bits(twin.pose)).all()
    same_particles(h.particles(), twin.particles())
    assert h.map().tobytes() == twin.map().tobytes()
    h.close(); twin.close()


# ---- 5. the host layer -------------------------------------------------------------------------------------------------------------------
def test_replay_binary_with_odometry_2_equals_the_c_abi_driven_from_python(tmp_path, pkg):
    """pfslamSearchScanCov + pfslamMoveParticles (host/kernel.h) through `pfslam_replay ... odometry=2`: before every frame after the first
    the new scan is searched against the previous scan at the previous pose, and the particles move by the winner's delta with the search's
    covariance and the lattice's quantisation floors.  Every frame's pose bits equal the same sequence through the binding."""
    build_host(pkg)
    _, frames = pkg.synth.corridor_sequence(6, seed=5)
    scene = tmp_path / "scene.txt"
    scene.write_text(SCENE_TXT)
    scans = np.stack([np.zeros(1081, F)] + [s for _, s in frames])  # scans[0] is never used (frame starts at 1)
    lidar = tmp_path / "lidar.f32"
    scans.astype(F).tofile(str(lidar))
    env = dict(os.environ, PFSLAM_PARTICLES="300", PFSLAM_KD_CAPACITY=str(1 << 16))
    out = subprocess.check_output([os.path.join(HOST, "pfslam_replay"), str(scene), str(lidar), "odometry=2"], env=env).decode()
    lines = [l for l in out.splitlines() if l.startswith("odometry ")]
    poses = [l for l in out.splitlines() if l.startswith("frame ")]
    assert len(lines) == len(frames) - 1 and len(poses) == len(frames)
    floor_xy, floor_t = F(0.025) / np.sqrt(F(12.0)), F(0.0125) / np.sqrt(F(12.0))
    h = pkg.PfSlam(300, kd_capacity=1 << 16)
    prev = None
    for f, (_, scan) in enumerate(frames, start=1):
        if f > 1:
            got = h.search_scan_cov(frames[f - 2][1], prev, scan)
            tok = lines[f - 2].split()
            assert tok[1] == str(f) and tok[2] == "index" and int(tok[3]) == got["index"] and got["index"] >= 0, lines[f - 2]
            assert tok[4] == "delta" and tok[8] == "sd" and tok[12] == "bits" and len(tok) == 16, lines[f - 2]
            assert [int(v, 16) for v in tok[13:16]] == got["pose"].view(np.uint32).tolist(), lines[f - 2]
            sd = np.sqrt(got["raw"][[3, 6, 8]])
            assert np.allclose([float(v) for v in tok[9:12]], sd, atol=1e-6), lines[f - 2]
            h.move_particles(f, got["pose"] - prev, got["raw"][3:9], ref_theta=float(prev[2]), sigma_xy_min=float(floor_xy),
                             sigma_theta_min=float(floor_t))
        h.step(f, scan)
        prev = np.array(h.pose, F)
        assert [int(v, 16) for v in poses[f - 1].split()[7:10]] == prev.view(np.uint32).tolist(), poses[f - 1]
    h.close()
    # odometry=1 is what it was: the shift's lines, without "sd"
    out = subprocess.check_output([os.path.join(HOST, "pfslam_replay"), str(scene), str(lidar), "odometry=1"], env=env).decode()
    lines = [l for l in out.splitlines() if l.startswith("odometry ")]
    assert len(lines) == len(frames) - 1 and all(len(l.split()) == 12 and " sd " not in l for l in lines)
