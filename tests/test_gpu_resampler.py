"""pfslam_set_resampler on the GPU: modes 1 (one multinomial draw per particle) and 2 (systematic) through every path that resamples -- the
stage, the split stage of a sharded handle, whole frames (generic, 2-D, round-5 in its stream / gate / lag variants, sharded) and the C++ host
layer -- and mode 0 untouched.

The oracle of the stage is tests/resampler_ref.py (PFResample restated from the CPU oracle's primitives, pinned to the oracle in mode 0 by
tests/test_resampler_spec.py); the oracle of whole frames is tests/stage_shadow.py with the same mode set on its handle: a frame composed of
stage calls, whose resample is that stage.  Everything is bit for bit; there is no tolerance anywhere in this file."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from stage_shadow import StageShadow
from test_gpu_devlib_frames import assert_same_particles, compare_per_frame, corridor, look
from test_gpu_frame import run_frames, world                      # noqa: F401  (world: a fixture)
from test_gpu_sharded import _VirtualRanks
from test_host_layer import HOST, SCENE_TXT, build_host
from test_resampler_spec import CASES, ref

pytestmark = pytest.mark.gpu
FIELDS = ("x", "y", "theta", "w")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- 1. the stage ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_stage_equals_the_restatement(pkg, name, mode):
    """pfslam_resample with x = the particle's index: x read back is the source index.  n = 100 and 1000 are far below, 4097 one above the
    four scan tiles (nothing here is gated: the stage always takes the tiled passes and k_sample); the H8 case has a non-monotone cdf."""
    make, frame = [(m, f) for k, m, f in CASES if k == name][0]
    p = make()
    did, neff, src = ref(name, mode)
    h = pkg.PfSlam(len(p))
    h.set_resampler(mode)
    h.set_particles(p)
    did_g, neff_g = h.resample(frame)
    assert did_g == did == 1 and bits(neff_g) == bits(neff)
    got = h.particles()
    bad = int((got["x"] != src.astype(np.float32)).sum())
    assert bad == 0, "%d of %d sources differ from the restatement" % (bad, len(p))
    assert (bits(got["y"]) == bits(p["y"][src])).all() and (bits(got["theta"]) == bits(p["theta"][src])).all() and (got["w"] == 1).all()
    h.close()


# ---- 2. the split stage on virtual ranks ---------------------------------------------------------------------------------------------------
def test_split_stage_on_three_ranks_equals_the_single_handle(pkg):
    """pfslam_resample_plan / _gather around hand-made all-gathers, mode 2, 1001 = 334 + 334 + 333 particles: the draw depends on global
    quantities only, so the ranks' slices concatenated are the single handle's particles (and the restatement's sources)."""
    torch = pytest.importorskip("torch")
    n, world_size, frame, mode = 1001, 3, 17, 2
    rng = np.random.RandomState(n)
    p = O.make_particles(n)
    p["y"] = rng.normal(0, 1, n); p["theta"] = rng.normal(0, 1, n)
    p["w"] = rng.uniform(0, 1, n).astype(np.float32) ** 8
    p["x"] = np.arange(n)
    one = pkg.PfSlam(n)
    one.set_resampler(mode)
    one.set_particles(p)
    did, neff = one.resample(frame)
    want = one.particles()
    v = _VirtualRanks(pkg, torch, n, world_size)
    for e, (stride, off, cnt) in zip(v.engs, v.lay):
        e.set_resampler(mode)
        e.set_particles(p[off:off + cnt])
    v._sync()
    gw = torch.cat([b.w for b in v.bufs])                       # all-gather of the (padded) weights
    for b in v.bufs:
        b.gw.copy_(gw)
    v._sync()
    plans = [e.resample_plan(frame) for e in v.engs]
    assert all(d == did == 1 and bits(ne) == bits(neff) for d, ne in plans), plans
    v._sync()
    blocks = [b.pose_blocks() for b in v.bufs]                  # all-gather of the [x | y | theta] blocks
    g = torch.cat([loc for loc, _ in blocks])
    for _, glob in blocks:
        glob.copy_(g)
    v._sync()
    for e in v.engs:
        e.resample_gather()
    got = [e.particles() for e in v.engs]
    assert_same_particles({fld: np.concatenate([q[fld] for q in got]) for fld in FIELDS}, want, "ranks")
    src = np.concatenate([q["x"] for q in got]).astype(np.int32)
    assert (np.diff(src) >= 0).all() and len(np.unique(src)) > 100
    v.close(); one.close()


# ---- 3. whole frames from an empty map -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n,grid", [(50, False), (1000, False), (300, True)])
def test_frames_from_an_empty_map_equal_the_shadow(pkg, n, grid, mode):
    frames = corridor(pkg, 16 if grid else 14)
    kw = dict(kd_capacity=1 << 16)
    s = StageShadow(n, pkg=pkg, **kw)
    s.h.set_resampler(mode)
    h = pkg.PfSlam(n, **kw)
    h.set_resampler(mode)
    resampled = 0
    for f, scan in enumerate(frames, start=1):          # (compare_per_frame, one frame at a time: the trace is per frame)
        compare_per_frame([s, h], [scan], grid=grid, first=f)
        resampled += h.trace()["resampled"]
    assert resampled >= 1, "no frame resampled"
    s.close(); h.close()


# ---- 4. round-5 frames on the 100 000-point world --------------------------------------------------------------------------------------
_SHADOWS = {}


def shadow_on_world(pkg, tree, scans, n, n_frames, switch):
    """The shadow through run_frames' recipe (map, five dispersions, frames 6 ...); switch: {frame index: resampler mode}.  A row per frame,
    particles and map bytes behind the last."""
    key = (n, n_frames, tuple(sorted(switch.items())))
    if key not in _SHADOWS:
        s = StageShadow(n, pkg=pkg, kd_capacity=len(tree) + (1 << 18))
        s.set_map(tree)
        for f in range(1, 6):
            s.motion_update(f)
        rows = []
        for i in range(n_frames):
            if i in switch:
                s.h.set_resampler(switch[i])
            s.step(6 + i, scans[i])
            rows.append(look(s))
        _SHADOWS[key] = (rows, s.particles().copy(), s.map().tobytes())
        s.close()
    return _SHADOWS[key]


def systematic(h):
    h.set_resampler(2)


def test_round5_frames_equal_the_shadow_in_every_frame_variant(pkg, world):
    """n = 20 000, 12 frames, mode 2: four streams with gates, one stream, lag 0 -- frames in flight, looked at only at the end."""
    tree, scans = world
    n, n_frames = 20000, 12
    rows, parts, mapb = shadow_on_world(pkg, tree, scans, n, n_frames, {0: 2})
    assert sum(r[1] for r in rows) >= 1, "no frame resampled"
    kw = dict(look_every=0, inspect=lambda h: h.frame_mode())
    runs = (("four streams", run_frames(pkg, tree, scans[:n_frames], n, serial=False, prepare=systematic, **kw)),
            ("one stream", run_frames(pkg, tree, scans[:n_frames], n, serial=True, prepare=systematic, **kw)),
            ("lag 0", run_frames(pkg, tree, scans[:n_frames], n, serial=False, prepare=lambda h: (h.set_resampler(2), h.set_lag(0)), **kw)))
    for name, run in runs:
        assert run[0][-1] == rows[-1], "%s: %s vs the shadow's %s" % (name, run[0][-1], rows[-1])
        assert_same_particles(run[1], parts, name)
        assert run[2] == mapb, "%s: maps differ" % name
        assert run[4]["violations"] == 0 and run[5]["round5_frame"], name
    assert runs[1][1][5]["serial"] and not runs[0][1][5]["serial"] and runs[0][1][5]["gates"]


def test_sharded_round5_frames_equal_the_shadow(pkg, world):
    """The same frames on two virtual ranks, mode 2 on every rank: every frame's trace and pose, the particles and the map."""
    torch = pytest.importorskip("torch")
    tree, scans = world
    n, n_frames = 20000, 12
    rows, parts, mapb = shadow_on_world(pkg, tree, scans, n, n_frames, {0: 2})
    assert sum(r[1] for r in rows) >= 1, "no frame resampled"
    v = _VirtualRanks(pkg, torch, n, 2, kd_capacity=len(tree) + (1 << 18))
    for e in v.engs:
        e.set_map(tree)
        e.set_resampler(2)
        for f in range(1, 6):
            e.motion_update(f)
    v2_frames = 0
    for i in range(n_frames):
        v.step(6 + i, scans[i])
        assert look(v) == rows[i], "frame %d: ranks %s, shadow %s" % (6 + i, look(v), rows[i])
        v2_frames += all(e.frame_mode()["round5_frame"] for e in v.engs)
    assert v2_frames >= n_frames - 3, v2_frames    # (a shard whose cloud has grown too wide goes back to the staged chain for a frame)
    got = [e.particles() for e in v.engs]
    assert_same_particles({fld: np.concatenate([g[fld] for g in got]) for fld in FIELDS}, parts, "ranks")
    for e in v.engs:
        assert e.map().tobytes() == mapb
    v.close()


# ---- 5. the default untouched --------------------------------------------------------------------------------------------------------------
def test_mode_1_and_back_before_the_first_frame_is_the_oracle(pkg):
    n = 1000
    _, seq = pkg.synth.corridor_sequence(14, seed=5)
    o = O.Slam(n, kd_capacity=1 << 16)
    h = pkg.PfSlam(n, kd_capacity=1 << 16)
    h.set_resampler(1)
    h.set_resampler(0)
    resampled = 0
    for f, (_, scan) in enumerate(seq, start=1):
        o.step(f, scan); h.step(f, scan)
        assert h.trace() == o.trace(), (f, h.trace(), o.trace())
        assert (bits(h.pose) == bits(o.pose)).all(), f
        resampled += o.trace()["resampled"]
    assert resampled >= 1
    assert_same_particles(h.particles(), o.particles(), "frame")
    assert h.map().tobytes() == o.tree().tobytes()
    h.close(); o.close()


def test_switch_with_frames_in_flight_equals_a_shadow_switched_at_the_same_frames(pkg, world):
    """0 -> 2 -> 0 at frames 4 and 8 of 12 round-5 frames: pfslam_set_resampler books the frames in flight, the mode holds from the next one."""
    tree, scans = world
    n, n_frames, switch = 20000, 12, {0: 0, 4: 2, 8: 0}
    rows, parts, mapb = shadow_on_world(pkg, tree, scans, n, n_frames, switch)
    assert sum(r[1] for r in rows[:4]) and sum(r[1] for r in rows[4:8]) and sum(r[1] for r in rows[8:]), "a leg without a resample"
    h = pkg.PfSlam(n, kd_capacity=len(tree) + (1 << 18))
    h.set_map(tree)
    for f in range(1, 6):
        h.motion_update(f)
    for i in range(n_frames):
        if i in switch:
            h.set_resampler(switch[i])
        h.step(6 + i, scans[i])
    h.synchronize()
    assert look(h) == rows[-1] and h.frame_mode()["round5_frame"]
    assert_same_particles(h.particles(), parts, "switched")
    assert h.map().tobytes() == mapb
    h.close()


# ---- 6. the error path -----------------------------------------------------------------------------------------------------------------
def test_a_mode_out_of_range_is_refused_and_the_handle_keeps_its_mode(pkg):
    name, mode = "n1000", 2
    make, frame = [(m, f) for k, m, f in CASES if k == name][0]
    p = make()
    h = pkg.PfSlam(len(p))
    h.set_resampler(mode)
    for bad in (3, -1):
        with pytest.raises(pkg.PfSlamError, match="pfslam_set_resampler: 0 .reference seeding"):   # (pfslam_last_error's message)
            h.set_resampler(bad)
    h.set_particles(p)
    h.resample(frame)
    assert (h.particles()["x"] == ref(name, mode)[2].astype(np.float32)).all()
    h.close()


# ---- 7. the C++ host layer -----------------------------------------------------------------------------------------------------------------
def test_replay_binary_with_resampler_2_matches_the_python_handle(tmp_path, pkg):
    build_host(pkg)
    _, frames = pkg.synth.corridor_sequence(9, seed=5)
    scene = tmp_path / "scene.txt"
    scene.write_text(SCENE_TXT)
    scans = np.stack([np.zeros(1081, np.float32)] + [s for _, s in frames])  # scans[0] is never used (frame starts at 1)
    lidar = tmp_path / "lidar.f32"
    scans.astype(np.float32).tofile(str(lidar))
    env = dict(os.environ, PFSLAM_PARTICLES="300", PFSLAM_KD_CAPACITY=str(1 << 16))
    out = subprocess.check_output([os.path.join(HOST, "pfslam_replay"), str(scene), str(lidar), "resampler=2"], env=env).decode()
    lines = [l for l in out.splitlines() if l.startswith("frame ")]
    assert len(lines) == len(frames)
    h = pkg.PfSlam(300, kd_capacity=1 << 16)
    h.set_resampler(2)
    resampled = 0
    for f, ((_, scan), line) in enumerate(zip(frames, lines), start=1):
        h.step(f, scan)
        tok = line.split()
        assert [int(tok[k], 16) for k in (7, 8, 9)] == h.pose.view(np.uint32).tolist(), line
        resampled += h.trace()["resampled"]
    assert resampled >= 1
    h.close()
    r = subprocess.run([os.path.join(HOST, "pfslam_replay"), str(scene), str(lidar), "resampler=7"], env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "pfslam_set_resampler" in r.stderr
