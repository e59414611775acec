"""pfslam_estimate on the GPU: the stage on uploaded clouds (one launch up to 4096 particles, three above), behind whole frames with one in
flight, on sharded handles, its error path and the C++ host layer.

Every comparison is bit for bit against tests/estimate_ref.py (the specification restated from the oracle's canonical sum, held against
float64 by tests/test_estimate_spec.py) on particles() of the SAME handle; there is no tolerance anywhere in this file."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import estimate_ref as E
import oracle_lib as O
from test_gpu_sharded import _VirtualRanks
from test_host_layer import HOST, SCENE_TXT, build_host

pytestmark = pytest.mark.gpu
FIELDS = ("x", "y", "theta", "w")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same16(got, want, what=""):
    assert (bits(got) == bits(want)).all(), "%s: got %s, restatement %s" % (what, np.asarray(got).tolist(), np.asarray(want).tolist())


def gather_by_hand(v):
    """The two all-gathers of ShardedSlam.estimate between virtual ranks: weights 5 -> 10, pose blocks 16 -> 17."""
    torch = v.torch
    v._sync()
    gw = torch.cat([b.w for b in v.bufs])
    blocks = [b.pose_blocks() for b in v.bufs]
    g = torch.cat([loc for loc, _ in blocks])
    for b, (_, glob) in zip(v.bufs, blocks):
        b.gw.copy_(gw)
        glob.copy_(g)
    v._sync()


# ---- 1. the stage ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["one", "zeros"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 8193, 100000])
def test_stage_equals_the_restatement(pkg, n, weights):
    """Below, at and above the 64 lanes of a wave and the 4096 particles of a tile (one launch up to there, three beyond); 8193 is two full
    tiles plus one particle; random weights with about a quarter of them zero."""
    p = E.particles_of(*E.cloud(n, weights))
    h = pkg.PfSlam(n)
    h.set_particles(p)
    raw = h.estimate_raw()
    back = h.particles()
    for fld in FIELDS:
        assert (bits(back[fld]) == bits(p[fld])).all(), fld
    same16(raw, E.estimate_particles(back), "n %d" % n)
    d = h.estimate()
    assert d["n"] == n and (bits(d["mean"]) == bits(raw[0:3])).all() and (d["cov"] == d["cov"].T).all()
    assert (bits(d["cov"][np.triu_indices(3)]) == bits(raw[3:9])).all()
    assert bits(d["neff"]) == bits(raw[9]) and bits(d["sum_w"]) == bits(raw[10]) and bits(d["sum_w2"]) == bits(raw[11])
    h.close()


# ---- 2. whole frames ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 5000])
def test_estimate_behind_frames_in_flight_describes_the_cloud_and_changes_nothing(pkg, n):
    """A corridor drive from an empty map, 12 frames: estimate() behind frames 3, 7 and 12 with the default lag (a frame in flight) and on a
    lag-0 handle equals the restatement on particles() taken at the same moment; a twin that never asks ends with the same pose, particles
    and map bytes."""
    _, frames = pkg.synth.corridor_sequence(12, seed=5)
    kw = dict(kd_capacity=1 << 16)
    h, h0, twin = pkg.PfSlam(n, **kw), pkg.PfSlam(n, **kw), pkg.PfSlam(n, **kw)
    h0.set_lag(0)
    resampled, seen = 0, []
    for f, (_, scan) in enumerate(frames, start=1):
        for e in (h, h0, twin):
            e.step(f, scan)
        if f in (3, 7, 12):
            raw, raw0 = h.estimate_raw(), h0.estimate_raw()     # (books the frame in flight first)
            same16(raw, E.estimate_particles(h.particles()), "frame %d" % f)
            same16(raw0, raw, "lag 0, frame %d" % f)
            assert raw[12] == n
            seen.append(raw)
        resampled += h.trace()["resampled"]
    assert resampled >= 1, "no frame resampled"
    assert not (bits(seen[0]) == bits(seen[2])).all()
    for e, name in ((h, "lag 1"), (h0, "lag 0")):
        assert (bits(e.pose) == bits(twin.pose)).all(), name
        pe, pt = e.particles(), twin.particles()
        for fld in FIELDS:
            assert (bits(pe[fld]) == bits(pt[fld])).all(), (name, fld)
        assert e.map().tobytes() == twin.map().tobytes(), name
    for e in (h, h0, twin):
        e.close()


# ---- 3. sharded handles --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [3, 2])
def test_every_rank_of_a_sharded_job_gets_the_unsharded_bits(pkg, world):
    """5000 particles over 3 ranks (stride 1667: the edge of the first 4096-particle tile falls inside the last shard) and over 2: an uploaded
    cloud, then the same handles behind 6 sharded frames -- hand-made all-gathers of buffers 5 -> 10 and 16 -> 17, as ShardedSlam.estimate
    issues them."""
    torch = pytest.importorskip("torch")
    n = 5000
    p = E.particles_of(*E.cloud(n, "zeros"))
    kw = dict(kd_capacity=1 << 16)
    one = pkg.PfSlam(n, **kw)
    one.set_particles(p)
    want = one.estimate_raw()
    same16(want, E.estimate_particles(p), "unsharded")
    v = _VirtualRanks(pkg, torch, n, world, **kw)
    if world == 3:
        assert v.lay[0][0] == 1667
    for e, (stride, off, cnt) in zip(v.engs, v.lay):
        e.set_particles(p[off:off + cnt])
    gather_by_hand(v)
    for r, e in enumerate(v.engs):
        same16(e.estimate_raw(), want, "rank %d of %d" % (r, world))
    origin = O.make_particles(n)                                 # (the drive starts at the origin: back to the initial cloud)
    one.set_particles(origin)
    for e, (stride, off, cnt) in zip(v.engs, v.lay):
        e.set_particles(origin[off:off + cnt])
    _, frames = pkg.synth.corridor_sequence(6, seed=5)
    for f, (_, scan) in enumerate(frames, start=1):
        one.step(f, scan)
        v.step(f, scan)
    want = one.estimate_raw()
    same16(want, E.estimate_particles(one.particles()), "unsharded, frames")
    gather_by_hand(v)
    for r, e in enumerate(v.engs):
        same16(e.estimate_raw(), want, "rank %d of %d, frames" % (r, world))
    v.close(); one.close()


def test_sharded_wrapper_at_world_1_equals_the_plain_handle(pkg):
    torch = pytest.importorskip("torch")
    sharded = importlib.import_module("gpu-icp-slam_amd.sharded")
    n = 500
    a = pkg.PfSlam(n, kd_capacity=1 << 16)
    s = sharded.ShardedSlam(pkg, n, 0, 1, device=0, torch=torch, kd_capacity=1 << 16)
    _, frames = pkg.synth.corridor_sequence(8, seed=7)
    for f, (_, scan) in enumerate(frames, start=1):
        a.step(f, scan)
        s.step(f, scan)
    issued = s.collectives
    da, ds = a.estimate(), s.estimate()
    assert s.collectives == issued
    assert sorted(da) == sorted(ds) == ["cov", "mean", "n", "neff", "sum_w", "sum_w2"]
    for k in da:
        assert (bits(da[k]) == bits(ds[k])).all(), k
    same16(a.estimate_raw(), E.estimate_particles(a.particles()), "world 1")
    a.close(); s.eng.close()


# ---- 4. the error path ---------------------------------------------------------------------------------------------------------------------
def test_zero_weights_are_refused_with_the_cause_and_the_handle_goes_on(pkg):
    n = 300
    x, y, t, _ = E.cloud(n, "one")
    h = pkg.PfSlam(n, kd_capacity=1 << 16)
    h.set_particles(E.particles_of(x, y, t, np.zeros(n, np.float32)))
    with pytest.raises(pkg.PfSlamError, match="pfslam_estimate: the weights sum to 0"):
        h.estimate()
    out = np.full(16, 7.5, np.float32)
    assert h.L.pfslam_estimate(h._h, out.ctypes.data_as(C.c_void_p)) != 0
    assert (out == 7.5).all(), "out was written"
    assert b"finite and > 0" in h.L.pfslam_last_error()
    h.set_particles(E.particles_of(x, y, t, np.full(n, np.inf, np.float32)))
    with pytest.raises(pkg.PfSlamError, match="pfslam_estimate: the weights sum to inf"):
        h.estimate()
    h.set_particles(O.make_particles(n))                         # (the initial cloud: the drive below starts at the origin)
    _, frames = pkg.synth.corridor_sequence(4, seed=5)
    for f, (_, scan) in enumerate(frames, start=1):
        h.step(f, scan)
    same16(h.estimate_raw(), E.estimate_particles(h.particles()), "after the refusals")
    h.close()


# ---- 5. the C++ host layer -----------------------------------------------------------------------------------------------------------------
def test_replay_binary_with_estimate_1_prints_the_handle_s_estimate(tmp_path, pkg):
    """pfslamPoseEstimate (host/kernel.h) through `pfslam_replay ... estimate=1`: one line per frame whose ten float bits are the C-ABI's."""
    build_host(pkg)
    _, frames = pkg.synth.corridor_sequence(9, seed=5)
    scene = tmp_path / "scene.txt"
    scene.write_text(SCENE_TXT)
    scans = np.stack([np.zeros(1081, np.float32)] + [s for _, s in frames])  # scans[0] is never used (frame starts at 1)
    lidar = tmp_path / "lidar.f32"
    scans.astype(np.float32).tofile(str(lidar))
    env = dict(os.environ, PFSLAM_PARTICLES="300", PFSLAM_KD_CAPACITY=str(1 << 16))
    out = subprocess.check_output([os.path.join(HOST, "pfslam_replay"), str(scene), str(lidar), "estimate=1"], env=env).decode()
    poses = [l for l in out.splitlines() if l.startswith("frame ")]
    lines = [l for l in out.splitlines() if l.startswith("estimate ")]
    assert len(lines) == len(poses) == len(frames)
    h = pkg.PfSlam(300, kd_capacity=1 << 16)
    for f, ((_, scan), line, pose) in enumerate(zip(frames, lines, poses), start=1):
        h.step(f, scan)
        tok = line.split()
        assert tok[1] == str(f) and tok[2] == "mean" and tok[6] == "cov" and tok[13] == "neff" and tok[15] == "bits" and len(tok) == 26, line
        raw = h.estimate_raw()
        assert [int(v, 16) for v in tok[16:26]] == raw[0:10].view(np.uint32).tolist(), line
        assert np.allclose([float(v) for v in tok[3:6]], raw[0:3], atol=1e-6) and np.allclose([float(v) for v in tok[7:13]], raw[3:9], rtol=1e-6)
        assert [int(pose.split()[k], 16) for k in (7, 8, 9)] == h.pose.view(np.uint32).tolist(), pose
    h.close()
    out = subprocess.check_output([os.path.join(HOST, "pfslam_replay"), str(scene), str(lidar)], env=env).decode()
    assert not [l for l in out.splitlines() if l.startswith("estimate ")]
