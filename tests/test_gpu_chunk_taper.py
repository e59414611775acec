"""The round-5 frame's scan-match launch with chunks that are not all of one size (csrc/score_plan.h: long chunks, the last rows shrink).

The partials are 16-bit integers and any order of adding them is exact, so every comparison here is bit for bit:
  * after every frame of pfslam_step, the fit of ALL particles (device buffer 1) against the stage-level pfslam_score_kd of the same
    particles on the same map -- that launch cuts the beams into uniform chunks (launch_score) -- and against the CPU oracle's
    score_kd on 1024 particles, the first and the last group of 64 among them;
  * pose, particles and map after the frames against a run on one stream (PFSLAM_SERIAL=1).
"The same particles on the same map": what the handle held after the previous frame (pfslam_get_particles, pfslam_get_map), dispersed by
the frame's own number -- pfslam_motion_update on the stage handle, orc_add_noise for the oracle.  One handle is alive at a time (the
frames run with their stream gates).
Sizes: 32 000 particles (chunks of 9 beams, the first count the test asks for above the taper's threshold of 8), 65 537 (the last wave has
one real lane) and 100 000 (the flagship) at 1081 beams; 100 000 at 4096 beams; 100 000 on a map whose weights reach +-3000, where 16-bit
partials allow 10 beams per chunk and the plan cuts 113 chunks instead of leaving the round-5 frame.
"""
import importlib
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_devlib_frames import environ

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-icp-slam_amd", "csrc")
SAMPLE = 1024


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def world(pkg):
    """the 2000-point map and the scans of tests/test_gpu_size_edges.py's frames"""
    pts, segs = pkg.synth.make_map_points(2000, seed=1)
    tree = pkg.kd_create(pts)
    scans = [pkg.synth.make_scan(segs, (0.002 * i, 0.001 * i, 0.0004 * i), seed=2000 + i) for i in range(6)]
    return {"tree": tree, "scans": scans}


def room_scans(nb, frames):
    """a smooth closed room, ranges in [3, 13] m (tests/test_gpu_upload_limits.py: neighbouring beams end in neighbouring cells)"""
    ang = np.radians(-135.0 + 0.25 * np.arange(nb))
    return [(8.0 + 5.0 * np.cos(3.0 * ang + 0.05 * f)).astype(np.float32) for f in range(frames)]


def plan_of(tmp_path_factory, n, nb, w):
    """csrc/score_plan.h's plan, through tests/score_plan_check.cpp (a host program; built once)"""
    global _CHECKER
    if _CHECKER is None:
        exe = str(tmp_path_factory.mktemp("plan") / "score_plan_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "score_plan_check.cpp"), "-o", exe])
        _CHECKER = exe
    head, starts = subprocess.run([_CHECKER, str(n), str(nb), str(w)], capture_output=True, text=True, check=True).stdout.splitlines()[:2]
    used, bpc, tapered, p16_ok, _ = [int(v) for v in head.split()]
    starts = [int(v) for v in starts.split()]
    return {"used": used, "bpc": bpc, "tapered": bool(tapered), "p16_ok": bool(p16_ok), "sizes": [b - a for a, b in zip(starts, starts[1:])]}


_CHECKER = None


def device_f32(pkg, h, which):
    import torch
    ptr, nbytes = h.device_ptr(which)
    sharded = importlib.import_module("gpu-icp-slam_amd.sharded")
    return torch.as_tensor(sharded._DevView(ptr, nbytes, "<f4", 4), device=torch.device("cuda", 0)).cpu().numpy().copy()


def run_frames(pkg, tree, scans, n, nb, serial=False, probe=0, first=6):
    """pfslam_step through the scans; per frame what the frame scored (particles and map in front of it) and the fit it left"""
    with environ(**({"PFSLAM_SERIAL": "1"} if serial else {})):
        h = pkg.PfSlam(n, n_beams=nb, kd_capacity=len(tree) + (1 << 17))
    h.set_map(tree)
    if probe:
        h.set_probe(probe)
    frames = []
    for i, s in enumerate(scans):
        before = {"p": h.particles(), "map": h.map(), "frame": first + i, "scan": s} if not serial else None
        h.step(first + i, s)
        if not serial:
            h.particles()       # (books the frame: everything it enqueued is done)
            before["fit"] = device_f32(pkg, h, 1)[:n]
            before["mode"] = h.frame_mode()
            frames.append(before)
    out = {"frames": frames, "pose": h.pose.copy(), "particles": h.particles(), "map": h.map().tobytes(), "mode": h.frame_mode(),
           "probe": h.probe(len(scans)) if probe else None}
    h.close()
    return out


def sample_of(n):
    """1024 particles: the first and the last group of 64, the rest drawn"""
    rest = np.random.RandomState(n).choice(np.arange(64, n - 64), SAMPLE - 128, replace=False)
    return np.sort(np.concatenate([np.arange(64), rest, np.arange(n - 64, n)]))


def check_frames(pkg, run, n, nb, what):
    """every frame's fit against the stage-level launch (uniform chunks) on a second handle and against the oracle's sample"""
    h = pkg.PfSlam(n, n_beams=nb, kd_capacity=len(run["frames"][0]["map"]) + (1 << 17))
    idx = sample_of(n)
    for f in run["frames"]:
        assert f["mode"]["round5_frame"], "%s frame %d: not a round-5 frame (%s)" % (what, f["frame"], f["mode"])
        h.set_map(f["map"]); h.set_particles(f["p"]); h.set_scan(f["scan"])
        h.motion_update(f["frame"])
        stage = h.score_kd()
        bad = np.flatnonzero(bits(stage) != bits(f["fit"]))
        print("%s frame %d: %d of %d fits differ from the stage-level score" % (what, f["frame"], len(bad), n))
        assert len(bad) == 0, "%s frame %d: %d fits differ from pfslam_score_kd, first at particle %d: %r vs %r" % (
            what, f["frame"], len(bad), bad[0], f["fit"][bad[0]], stage[bad[0]])
        moved = O.add_noise(f["p"].copy(), f["frame"])
        with environ(ORC_THREADS="16"):
            want = O.score_kd(f["map"], moved[idx], f["scan"], threads=16)
        bad = np.flatnonzero(bits(want) != bits(f["fit"][idx]))
        assert len(bad) == 0, "%s frame %d: %d of the %d sampled fits differ from the oracle's, first at particle %d: %r vs %r" % (
            what, f["frame"], len(bad), SAMPLE, idx[bad[0]], f["fit"][idx[bad[0]]], want[bad[0]])
    h.close()


def check_serial(pkg, run, tree, scans, n, nb, what):
    one = run_frames(pkg, tree, scans, n, nb, serial=True)
    assert one["mode"]["serial"] and one["mode"]["round5_frame"], one["mode"]
    assert (bits(one["pose"]) == bits(run["pose"])).all(), "%s: pose %s, on one stream %s" % (what, run["pose"], one["pose"])
    for fld in ("x", "y", "theta", "w"):      # (the record's other bytes are padding and host-side fields)
        bad = np.flatnonzero(bits(one["particles"][fld]) != bits(run["particles"][fld]))
        assert len(bad) == 0, "%s: %d particles differ from the one-stream run in %s, first at %d" % (what, len(bad), fld, bad[0])
    assert one["map"] == run["map"], "%s: maps differ from the one-stream run" % what


@pytest.mark.parametrize("n", [32000, 65537, 100000])
def test_frames_with_tapered_chunks_at_1081_beams(pkg, world, tmp_path_factory, n):
    """6 frames: fit of all particles == the stage-level score (uniform chunks) == the oracle's sample; pose, particles, map == one stream."""
    plan = plan_of(tmp_path_factory, n, 1081, 113)
    assert plan["tapered"] and plan["sizes"][0] > plan["sizes"][-1], plan
    assert n != 65537 or (n - 1) % 64 == 0        # (one real lane in the last wave)
    run = run_frames(pkg, world["tree"], world["scans"], n, 1081)
    check_frames(pkg, run, n, 1081, "n %d" % n)
    check_serial(pkg, run, world["tree"], world["scans"], n, 1081, "n %d" % n)


def test_frames_with_tapered_chunks_at_4096_beams(pkg, world, tmp_path_factory):
    n, nb = 100000, 4096
    plan = plan_of(tmp_path_factory, n, nb, 113)
    assert plan["tapered"] and plan["sizes"][0] > plan["sizes"][-1], plan
    scans = room_scans(nb, 2)
    run = run_frames(pkg, world["tree"], scans, n, nb)
    check_frames(pkg, run, n, nb, "4096 beams")
    check_serial(pkg, run, world["tree"], scans, n, nb, "4096 beams")


def test_large_map_weights_shorten_the_chunks(pkg, world, tmp_path_factory):
    """An uploaded map whose integer weights reach +-3000: 16-bit partials allow 10 beams per chunk (10 x 3000 <= 32767 < 11 x 3000), the
    uniform plan's 26 would not fit.  The frames stay round-5 frames, on more and shorter chunks; scores equal the oracle's sample."""
    n, nb = 100000, 1081
    tree = world["tree"].copy()
    rng = np.random.RandomState(17)
    w = rng.randint(-3000, 3001, len(tree)).astype(np.float32)
    w[:2] = (3000.0, -3000.0)
    tree["w"] = w
    plan = plan_of(tmp_path_factory, n, nb, 3000)
    assert plan["p16_ok"] and plan["bpc"] == 10 and 10 * 3000 <= 32767 < 11 * 3000, plan
    run = run_frames(pkg, tree, world["scans"][:3], n, nb)
    assert all(f["mode"]["round5_frame"] for f in run["frames"]), [f["mode"] for f in run["frames"]]
    assert np.abs(run["frames"][0]["map"]["w"]).max() == 3000.0
    check_frames(pkg, run, n, nb, "weights +-3000")


@pytest.mark.parametrize("n", [10000, 40000])
def test_the_probe_stamps_of_the_launchs_end(pkg, world, n):
    """Frame probe on: "last wave starts" and "last wave ends" are there in every frame -- uniform plan (10 000) and taper (40 000) --, and
    last wave starts <= last wave ends <= the reduce's stamp."""
    run = run_frames(pkg, world["tree"], world["scans"], n, 1081, probe=16)
    names, t, last = run["probe"]
    sc, ls, le, rd = [names.index(k) for k in ("C scan-match", "C scan-match: last wave starts", "C scan-match: last wave ends", "C reduce")]
    assert len(t) == len(world["scans"])
    for k, row in enumerate(t):
        print("n %d frame %d: scan-match %+.2f, last wave starts %+.2f, ends %+.2f, reduce %+.2f us" % (
            n, 6 + k, 0.0, row[ls] - row[sc], row[le] - row[sc], row[rd] - row[sc]))
        assert row[sc] > 0 and row[ls] > 0 and row[le] > 0 and row[rd] > 0, (k, row[[sc, ls, le, rd]])
        assert row[sc] <= row[ls] <= row[le] <= row[rd], (k, row[[sc, ls, le, rd]])
