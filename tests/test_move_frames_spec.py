"""Frames with odometry moves on the CPU: the oracle's pose hook (orc_slam_replace_poses) under tests/move_ref.py's move_oracle, and the
sharded orchestration over the oracle-backed engine under gloo.  Every comparison is bit for bit.

move_oracle is what tests/test_gpu_move_frames.py holds the product's frames to, so it is itself held to the one odometry call the oracle
has had all along: where pfslam_move_particles is pfslam_shift_particles by the header (cov NULL, no floors, every heading equal to
ref_theta), the moved oracle must be the shifted oracle -- at once and through the frames that follow, which read the HOST copy of the
particles (the dispersion uploads it) and its mirror weights."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import move_frames as MF
import move_ref as M
import oracle_lib as O
from test_sharded_gloo import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
bits = MF.bits


@pytest.mark.parametrize("strict", (1, 0))
def test_move_oracle_without_noise_is_the_oracles_shift_through_the_following_frames(pkg, strict):
    """Three corridor frames (weights and their half-array mirror differ by then), then a cloud around the pose whose headings all equal
    ref_theta, uploaded to both oracles; one is shifted, the other moved with cov None and no floors.  Particles and pose agree at once;
    the next two frames -- trace, pose, particles, map -- show that the host copy moved too and that no weight or mirror weight did."""
    n = 300
    frames = MF.corridor(pkg, 5)
    delta = np.array([0.046875, -0.0234375, 0.0107421875], F) + F(1e-3)      # (not signed zeros, and sums that round)
    pair = []
    for k in range(2):
        o = O.Slam(n, kd_capacity=1 << 16, strict_host_mirror=strict)
        for f in (1, 2, 3):
            o.step(f, frames[f - 1][1])
        pair.append(o)
    a, b = pair
    pose = a.pose
    rng = np.random.RandomState(3)
    p = a.particles()
    p["x"] = pose[0] + rng.uniform(-0.02, 0.02, n).astype(F)
    p["y"] = pose[1] + rng.uniform(-0.02, 0.02, n).astype(F)
    p["theta"] = pose[2]
    assert len(set(bits(p["w"]).tolist())) > 1                                # (the weights are not all alike: a touched one would show)
    for o in pair:
        o.set_particles(p)
    a.shift_particles(delta)
    M.move_oracle(b, 4, delta, None, ref_theta=float(pose[2]))
    assert not (bits(a.particles()["x"]) == bits(p["x"])).any()
    for f in (None, 4, 5):
        if f is not None:
            a.step(f, frames[f - 1][1]); b.step(f, frames[f - 1][1])
            assert MF.row_of(a) == MF.row_of(b), f
            assert bits(a.trace()["neff"]) == bits(b.trace()["neff"]), f
            assert a.tree().tobytes() == b.tree().tobytes(), f
        assert (bits(a.pose) == bits(b.pose)).all(), f
        MF.assert_same_particles(b.particles(), a.particles(), "behind frame %s" % f)
    assert a.trace()["n_insert"] > 0
    a.close(); b.close()


def test_the_pose_hook_touches_no_weight(pkg):
    """orc_slam_replace_poses writes x, y, theta and robotPos; the weights read back are the ones uploaded."""
    n = 65
    x, y, th, w = M.cloud(n, 0.3, seed=4)
    o = O.Slam(n, kd_capacity=16)
    o.set_particles(M.particles_of(x, y, th, w))
    o.replace_poses(y, th, x, np.array([1.5, -2.5, 0.25], F))
    got = o.particles()
    MF.assert_same_particles(got, M.particles_of(y, th, x, w))
    assert (bits(o.pose) == bits(np.array([1.5, -2.5, 0.25], F))).all()
    o.close()


def _worker(rank, world, port, n_global, setting, out_dir):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import oracle_engine as OE
    pkg = importlib.import_module("gpu-icp-slam_amd")
    sharded = importlib.import_module("gpu-icp-slam_amd.sharded")
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    stride, goff, n = sharded.shard_layout(n_global, world, rank)
    eng = OE.OracleShardEngine(n, goff, n_global, stride=stride)
    s = sharded.ShardedSlam(pkg, n_global, rank, world, dist=dist, torch=torch, engine=eng, buffers=OE.OracleBuffers(eng))
    frames = MF.corridor(pkg)
    moves = MF.commanded(frames, setting)
    log = []
    for f, (_, scan) in enumerate(frames, start=1):
        if f in moves:
            delta, cov, opts = moves[f]
            s.move_particles(f, delta, cov, **opts)
        s.step(f, scan)
        t = s.trace()
        log.append((t.get("best", -1), t.get("resampled", 0), t.get("kd_size", 0)) + tuple(eng.robot.view(np.int32).tolist()))
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), x=eng.x, y=eng.y, th=eng.th, w=eng.w, log=np.array(log, np.int64), tree=eng.tree[:eng.size])
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_global,setting", [(2, 600, "wide"), (3, 500, "small"), (3, 500, "floors")])
def test_sharded_ranks_with_moves_match_the_unsharded_oracle(tmp_path, pkg, world, n_global, setting):
    """ShardedSlam.move_particles before every frame from the second on, over OracleShardEngine under gloo (600 = 2 x 300; 500 = 167 + 167
    + 166): every rank's best particle, resample flag, map size and pose bits of every frame, the concatenated particles and the map equal
    ONE oracle moved by move_oracle.  The engine keys its draws by the global index and leaves the weights and their mirror alone."""
    mp.spawn(_worker, args=(world, _free_port(), n_global, setting, str(tmp_path)), nprocs=world, join=True)
    want = MF.oracle_drive(pkg, n_global, setting)
    MF.assert_conditions(want["rows"], "%d particles, %s" % (n_global, setting))
    want_log = [[r[0], r[1], r[5]] + list(r[6:9]) for r in want["rows"]]
    r = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % k)) for k in range(world)]
    for k in range(world):
        got = r[k]["log"].tolist()
        bad = [i + 1 for i in range(len(want_log)) if got[i] != want_log[i]]
        assert not bad, "rank %d differs from the oracle in frames %s" % (k, bad)
        assert r[k]["tree"].tobytes() == want["map"]
    for fld, key in (("x", "x"), ("y", "y"), ("theta", "th"), ("w", "w")):
        got = np.concatenate([r[k][key] for k in range(world)])
        assert (bits(got) == bits(want["particles"][fld])).all(), fld
