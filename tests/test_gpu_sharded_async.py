"""The sharded frame under ASYNCHRONOUS, delayed all-gathers.

include/pfslam.h promises that stream order is all the ordering a caller of pfslam_shard_* has to provide: each all-gather goes on the
stream pfslam_shard_stream names, and the library's own cross-stream edges (events, or gates in a process with one handle) order every
reader of the gathered buffers 10, 15 and 17 behind the collective that fills it.  test_gpu_sharded.py synchronises the host between
every part and every collective, so a missing edge never shows there.  Here nothing waits for the device inside a frame:

  A  events mode: every rank of a job in this process (several handles: the edges are events), the all-gathers done like RCCL does
     them on the frame's own streams -- ready events, an optional delay kernel, device-to-device copies, done events, a barrier --
     against ONE handle stepping all particles (and the CPU oracle where the size allows), with every rank concurrent, one rank on one
     stream (its key all-gather rides the particle stream) or one rank on the staged chain.
  B  gates mode: one rank's handle alone in a child process, its peers' slices copied in from the arrays a synchronised run recorded.

A delay holds one collective back for many frame times; each case checks that the delay took effect and that the organisation it
names is what ran (pfslam_frame_mode)."""
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = ("best", "resampled", "n_wall", "n_free", "n_insert", "kd_size")
FIRST_DELAYED = 2       # stepped frames 0 and 1 run undelayed: they fill the gathered pose blocks with real poses, so a stale read on a
                        # broken tree gives a wrong result, not garbage coordinates
DELAY_FACTOR = 10.0     # an injected delay lasts at least this many undelayed frame times

# name -> (global particles, ranks, frames, source, read): "bench" = test_gpu_sharded._bench_like (a fixed 20 000-point map, frames 6 ..;
# shards large enough for lattice-cell rows), "corridor" = the map built by the SLAM step itself from frame 1 (re-balance at frame 5; small
# enough for the CPU oracle).  read: "frame" = pose and trace every frame (books them), "end" = only at the end (frames stay in flight).
# variant (pfslam_set_variant, every handle of the case): 3 = lattice-cell rows at any particle count -- 125-particle shards of the
# corridor's cloud would otherwise take the staged chain from their third frame on; the results are the same either way.
WORKLOADS = {
    "w2_cells": (30000, 2, 14, "bench", "end", 0),
    "w3_ragged": (30001, 3, 14, "bench", "end", 0),     # 10001 + 10001 + 9999
    "w8_small": (1000, 8, 14, "corridor", "frame", 3),  # 125 per shard: the keys can be there long before the pose blocks
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


class _Workload:
    def __init__(self, pkg, name):
        import test_gpu_sharded as TS
        self.name = name
        self.n, self.world, self.frames, self.kind, self.read, self.variant = WORKLOADS[name]
        if self.kind == "bench":
            self.tree, self.scans = TS._bench_like(pkg, self.n, n_frames=self.frames)
            self.first, self.cap = 6, len(self.tree) + (1 << 18)
        else:
            _, fr = pkg.synth.corridor_sequence(self.frames, seed=5)
            self.tree, self.scans = None, [s for _, s in fr]
            self.first, self.cap = 1, 1 << 16

    def frame_ids(self):
        return [self.first + i for i in range(len(self.scans))]

    def prepare(self, e):
        if self.variant:
            e.set_variant(self.variant)
        if self.tree is not None:
            e.set_map(self.tree)
            for f in range(1, 6):
                e.motion_update(f)

    def seeds(self, i):
        return self.tree is None and i == 0     # the corridor's first scan seeds the map


def _single(pkg, wl, variant=0, read=True):
    """ONE unsharded handle over the workload: per-frame pose bits, trace and frame mode of every stepped frame, final particles / map /
    trace; without `read` only the wall time per frame (nothing booked in between)."""
    e = pkg.PfSlam(wl.n, kd_capacity=wl.cap)
    wl.prepare(e)
    if variant:
        e.set_variant(variant)
    out = {"pose": [], "trace": [], "round5": []}
    t0 = time.perf_counter()
    for i, (f, s) in enumerate(zip(wl.frame_ids(), wl.scans)):
        e.step(f, s)
        if read and not wl.seeds(i):
            out["round5"].append(e.frame_mode()["round5_frame"])
            out["pose"].append(bits(e.pose).tolist())
            t = e.trace()
            out["trace"].append({k: t[k] for k in TRACE})
    e.synchronize()
    out["ms_per_frame"] = 1e3 * (time.perf_counter() - t0) / len(wl.scans)
    if read:
        t = e.trace()
        out["final_trace"] = {k: t[k] for k in TRACE}
        out["final_pose"] = bits(e.pose).tolist()
        p = e.particles()
        out["particles"] = {k: p[k].copy() for k in ("x", "y", "theta", "w")}
        out["map"] = e.map().tobytes()
    e.close()
    return out


@pytest.fixture(scope="module")
def refs(pkg):
    """Per workload: the single handle's results (default organisation and variant 2), its undelayed frame time, the oracle's frames."""
    cache = {}

    def get(name):
        if name not in cache:
            wl = _Workload(pkg, name)
            r = {"wl": wl, "one": _single(pkg, wl), "staged": _single(pkg, wl, variant=2)}
            r["ms_per_frame"] = min(_single(pkg, wl, read=False)["ms_per_frame"] for _ in range(2))
            if wl.kind == "corridor":
                import oracle_lib as O
                o = O.Slam(wl.n, kd_capacity=wl.cap)
                rows = []
                for i, (f, s) in enumerate(zip(wl.frame_ids(), wl.scans)):
                    o.step(f, s)
                    if not wl.seeds(i):
                        t = o.trace()
                        rows.append((bits(o.pose).tolist(), t["best"], t["resampled"], o.kd_size))
                r["oracle"] = {"rows": rows, "particles": o.particles(), "map": o.tree().tobytes()}
                o.close()
            cache[name] = r
        return cache[name]
    return get


def _calibrate_sleep(torch, stream_ptr):
    """Clock cycles of torch.cuda._sleep per millisecond, timed with events on `stream_ptr` (its cycles-to-time ratio is not documented)."""
    s = torch.cuda.ExternalStream(stream_ptr, device=torch.device("cuda", 0))
    rate = None
    with torch.cuda.stream(s):
        for cycles in (1 << 20, 1 << 20, 1 << 22):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            torch.cuda._sleep(cycles)
            b.record(s)
            b.synchronize()
            rate = cycles / max(a.elapsed_time(b), 1e-3)
    return rate


def _delay_cycles(rate, ms_per_frame):
    """Twice the target (the kernel counts a clock that may run faster than at calibration), at least 2 ms."""
    return int(2.0 * rate * max(DELAY_FACTOR * ms_per_frame, 2.0))


class _AsyncCollectives:
    """All-gather `k` of a frame across the ranks' handles the way RCCL runs it on the frame's own streams: every rank's
    pfslam_shard_stream(k) records "ready"; on every rank's stream: wait for every rank's ready, the optional delay kernel, device-to-device
    copies of every rank's local slice into this rank's gathered buffer, "done"; then every stream waits for every rank's done (the
    barrier a collective implies: no rank overwrites a local buffer a peer still reads).  All of step two is issued before any of step
    three, and nothing synchronises the host."""

    def __init__(self, torch, engs):
        self.torch, self.engs = torch, engs
        self.ext = {}
        self.keep = []          # the events of the frames in flight
        self.spans = []         # (collective, rank, start, end) timing events around every delay kernel
        self.streams = []       # per collective issued: every rank's stream pointer

    def _ext(self, ptr):
        s = self.ext.get(ptr)
        if s is None:
            s = self.ext[ptr] = self.torch.cuda.ExternalStream(ptr, device=self.torch.device("cuda", 0))
        return s

    def gather(self, k, srcs, dsts, delay_cycles=0):
        T = self.torch
        ptrs = [e.shard_stream(k) for e in self.engs]
        self.streams.append((k, ptrs))
        sts = [self._ext(p) for p in ptrs]
        seg = [s.numel() for s in srcs]
        for d in dsts:
            assert d.numel() == sum(seg)
        ready = []
        for s in sts:
            ev = T.cuda.Event()
            ev.record(s)
            ready.append(ev)
        done = []
        for r, s in enumerate(sts):
            with T.cuda.stream(s):
                for ev in ready:
                    s.wait_event(ev)
                if delay_cycles:
                    a, b = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
                    a.record(s)
                    T.cuda._sleep(delay_cycles)
                    b.record(s)
                    self.spans.append((k, r, a, b))
                off = 0
                for src in srcs:
                    dsts[r][off:off + src.numel()].copy_(src, non_blocking=True)
                    off += src.numel()
                ev = T.cuda.Event()
                ev.record(s)
                done.append(ev)
        for s in sts:
            for ev in done:
                s.wait_event(ev)
        self.keep.append((ready, done))


class _AsyncJob:
    """A sharded job of `world` handles in this process, stepped through pfslam_shard_* with _AsyncCollectives between the parts."""

    def __init__(self, pkg, torch, wl, org):
        sharded = importlib.import_module("gpu-icp-slam_amd.sharded")
        self.torch, self.wl = torch, wl
        lay = [sharded.shard_layout(wl.n, wl.world, r) for r in range(wl.world)]
        self.engs = [pkg.PfSlam(cnt, kd_capacity=wl.cap, global_offset=off, global_n=wl.n, shard_stride=stride) for stride, off, cnt in lay]
        self.odd = wl.world - 1     # the rank a non-concurrent organisation applies to: the last (ragged) one
        for e in self.engs:
            wl.prepare(e)
            if wl.kind == "corridor":
                e.set_shard_balance(True)
        if org == "serial":
            self.engs[self.odd].set_serial(1)
        elif org == "staged":
            self.engs[self.odd].set_variant(2)
        self.bufs = [sharded.GpuBuffers(e, torch, 0) for e in self.engs]
        self.coll = _AsyncCollectives(torch, self.engs)
        self.n_adopted = 0

    def _sync(self):
        for e in self.engs:
            e.synchronize()
        self.torch.cuda.synchronize()

    def _balance(self, f):
        """The one re-balance per job, between two frames (test_gpu_sharded.py's protocol: rank 0 builds, the others adopt its arrays)."""
        due = [e.shard_balance_due(f) for e in self.engs]
        assert len(set(due)) == 1
        if not due[0][0]:
            return
        self.engs[0].shard_balance_build(f)
        self._sync()
        src = self.bufs[0].tree_buffers(due[0][1])
        for b in self.bufs[1:]:
            for dst, s_ in zip(b.tree_buffers(due[0][1]), src):
                dst.copy_(s_)
        self._sync()
        for e in self.engs[1:]:
            e.shard_balance_adopt()
            self.n_adopted += 1

    def step(self, f, scan, delay_k=None, delay_cycles=0):
        """Returns True when the frame only seeded the map."""
        engs, bufs, c = self.engs, self.bufs, self.coll
        if self.wl.kind == "corridor":
            self._balance(f)
        seeded = [e.shard_disperse(f, scan) for e in engs]
        assert len(set(seeded)) == 1
        if seeded[0]:
            return True
        d = lambda k: delay_cycles if delay_k == k else 0
        blocks = [b.pose_blocks() for b in bufs]                    # the local block alternates: after shard_disperse, every frame
        c.gather(0, [loc for loc, _ in blocks], [glob for _, glob in blocks], d(0))
        for e in engs:
            e.shard_score()
        c.gather(1, [b.pack for b in bufs], [b.packs for b in bufs], d(1))   # the local record alternates: after shard_score
        for e in engs:
            e.shard_weights()
        c.gather(2, [b.w for b in bufs], [b.gw for b in bufs], d(2))
        for e in engs:
            e.shard_finish()
        return False

    def close(self):
        for e in self.engs:
            e.close()


def _check_modes(modes, streams, org, odd, n_stepped, gates):
    """modes[i][r]: frame_mode of rank r after stepped frame i; streams[i][r] = (stream of collective 0, of collective 1)."""
    world = len(modes[0])
    for i, row in enumerate(modes):
        for r, fm in enumerate(row):
            assert fm["gates"] == gates or not fm["round5_frame"], (i, r, fm)   # (a staged frame reports the handle's setting)
            assert fm["serial"] == (org == "serial" and r == odd), (i, r, fm)
    for r in range(world):
        r5 = sum(row[r]["round5_frame"] for row in modes)
        if org == "staged" and r == odd:
            assert r5 == 0, "rank %d was forced onto the staged chain and ran %d round-5 frames" % (r, r5)
            assert all(st[r][0] == st[r][1] for st in streams), "staged chain: every collective rides the handle's stream"
        else:
            assert r5 >= n_stepped - 3, "rank %d ran %d round-5 frames of %d" % (r, r5, n_stepped)
        if org == "serial" and r == odd:
            assert all(st[r][0] == st[r][1] for st in streams), "one-stream rank: its key all-gather rides the particle stream"
    if org != "staged":
        # the concurrent ranks' key all-gather rides the chain stream in (nearly) every frame (a frame that wipes the rows is on one stream)
        for r in range(world):
            if not (org == "serial" and r == odd):
                assert sum(st[r][0] != st[r][1] for st in streams) >= n_stepped - 3, r


def _check_spans(torch, spans, want_k, n_delayed, world, ms_per_frame):
    torch.cuda.synchronize()
    if want_k is None:
        assert not spans
        return []
    ks = sorted({k for k, _, _, _ in spans})
    assert ks == [want_k] and len(spans) == n_delayed * world, (ks, len(spans))
    ms = [a.elapsed_time(b) for _, _, a, b in spans]
    assert min(ms) >= DELAY_FACTOR * ms_per_frame, "a delay of %.3f ms is under %g undelayed frame times (%.3f ms)" % (min(ms), DELAY_FACTOR, ms_per_frame)
    return ms


@pytest.mark.parametrize("org", ["concurrent", "serial", "staged"])
@pytest.mark.parametrize("delay_k", [None, 0, 1, 2], ids=["no_delay", "delay_poses", "delay_keys", "delay_weights"])
@pytest.mark.parametrize("wname", list(WORKLOADS))
def test_async_gathers_events_mode_match_single_handle(pkg, refs, wname, delay_k, org):
    """Matrix A: every rank of the job in this process (edges: events), all-gathers asynchronous and one of them delayed by many frame
    times from the third stepped frame on; pose / trace / particles / map of ONE handle stepping all particles, bit for bit (and the
    CPU oracle's at 1000 particles); the cell rows' invariants hold on every rank; the organisation named is what ran."""
    torch = pytest.importorskip("torch")
    ref = refs(wname)
    wl, one = ref["wl"], ref["one"]
    if org == "staged":
        # the per-handle switch that moves a rank onto the staged chain gives the same results on one handle
        st = ref["staged"]
        assert not any(st["round5"]) and st["pose"] == one["pose"] and st["trace"] == one["trace"]
        assert st["map"] == one["map"] and all((bits(st["particles"][k]) == bits(one["particles"][k])).all() for k in ("x", "y", "theta", "w"))
    assert sum(one["round5"]) >= len(one["round5"]) - 3
    job = _AsyncJob(pkg, torch, wl, org)
    cycles = 0
    if delay_k is not None:
        cycles = _delay_cycles(_calibrate_sleep(torch, job.engs[0].shard_stream(0)), ref["ms_per_frame"])
    modes, streams, poses, traces = [], [], [], []
    stepped = 0
    for i, (f, s) in enumerate(zip(wl.frame_ids(), wl.scans)):
        n_coll = len(job.coll.streams)
        if job.step(f, s, delay_k, cycles if stepped >= FIRST_DELAYED else 0):
            continue
        stepped += 1
        st = job.coll.streams[n_coll:]
        streams.append([(st[0][1][r], st[1][1][r]) for r in range(wl.world)])
        modes.append([e.frame_mode() for e in job.engs])    # (host state: books nothing)
        if wl.read == "frame":                              # books the frame: the pose, and the trace, of every rank
            poses.append([bits(e.pose).tolist() for e in job.engs])
            traces.append([{k: v for k, v in e.trace().items() if k in TRACE} for e in job.engs])
    n_stepped = len(one["pose"])
    assert stepped == n_stepped
    ms = _check_spans(torch, job.coll.spans, delay_k, n_stepped - FIRST_DELAYED, wl.world, ref["ms_per_frame"])
    _check_modes(modes, streams, org, job.odd, n_stepped, gates=False)
    for e in job.engs:
        e.synchronize()
    if wl.read == "frame":
        for i in range(n_stepped):
            for r in range(wl.world):
                assert poses[i][r] == one["pose"][i], (i, r)
                assert traces[i][r] == one["trace"][i], (i, r, traces[i][r], one["trace"][i])
    for r, e in enumerate(job.engs):
        t = e.trace()
        assert {k: t[k] for k in TRACE} == one["final_trace"], (r, t, one["final_trace"])
        assert bits(e.pose).tolist() == one["final_pose"], r
    got = [e.particles() for e in job.engs]
    for fld in ("x", "y", "theta", "w"):
        assert (bits(np.concatenate([g[fld] for g in got])) == bits(one["particles"][fld])).all(), fld
    for r, e in enumerate(job.engs):
        assert e.map().tobytes() == one["map"], "rank %d: map differs from the single handle's" % r
        assert e.check_cells()["violations"] == 0, r
    if "oracle" in ref:
        o = ref["oracle"]
        assert job.n_adopted == wl.world - 1        # frame 5 re-balanced (one host build, broadcast)
        for i, (pose, best, resampled, kd_size) in enumerate(o["rows"]):
            assert one["pose"][i] == pose and one["trace"][i]["best"] == best and one["trace"][i]["resampled"] == resampled
            assert one["trace"][i]["kd_size"] == kd_size
        for fld in ("x", "y", "theta", "w"):
            assert (bits(np.concatenate([g[fld] for g in got])) == bits(o["particles"][fld])).all(), fld
        assert one["map"] == o["map"]
    job.close()
    if ms:
        print("%s delay %s: %d delays %.2f .. %.2f ms (frame %.3f ms)" % (wname, delay_k, len(ms), min(ms), max(ms), ref["ms_per_frame"]))


# ---- matrix B: gates mode, one rank's handle alone in a process ------------------------------------------------------------------------

GATES_WL = "w3_ragged"


@pytest.fixture(scope="module")
def gates_record(pkg, refs, tmp_path_factory):
    """The job of GATES_WL stepped with the SYNCHRONISED virtual-rank protocol of test_gpu_sharded.py: every frame's gathered arrays
    (buffers 17, 15, 10) and every rank's results, in a file the child processes read.  (No re-balance falls in the window: frames 6 .. 19.)"""
    torch = pytest.importorskip("torch")
    sharded = importlib.import_module("gpu-icp-slam_amd.sharded")
    ref = refs(GATES_WL)
    wl, one = ref["wl"], ref["one"]
    assert all(f % 100 != 5 for f in wl.frame_ids())
    lay = [sharded.shard_layout(wl.n, wl.world, r) for r in range(wl.world)]
    engs = [pkg.PfSlam(cnt, kd_capacity=wl.cap, global_offset=off, global_n=wl.n, shard_stride=stride) for stride, off, cnt in lay]
    for e in engs:
        wl.prepare(e)
    bufs = [sharded.GpuBuffers(e, torch, 0) for e in engs]

    def sync():
        for e in engs:
            e.synchronize()
        torch.cuda.synchronize()

    g17, g15, g10 = [], [], []
    per_rank = [{"pose": [], "trace": []} for _ in engs]
    for f, s in zip(wl.frame_ids(), wl.scans):
        assert not any([e.shard_disperse(f, s) for e in engs])
        sync()
        blocks = [b.pose_blocks() for b in bufs]
        g = torch.cat([loc for loc, _ in blocks])
        for _, glob in blocks:
            glob.copy_(g)
        sync()
        g17.append(g.cpu().numpy())
        for e in engs:
            e.shard_score()
        sync()
        packs = torch.cat([b.pack for b in bufs])
        for b in bufs:
            b.packs.copy_(packs)
        sync()
        g15.append(packs.cpu().numpy())
        for e in engs:
            e.shard_weights()
        sync()
        gw = torch.cat([b.w for b in bufs])
        for b in bufs:
            b.gw.copy_(gw)
        sync()
        g10.append(gw.cpu().numpy())
        for e in engs:
            e.shard_finish()
        for r, e in enumerate(engs):
            per_rank[r]["pose"].append(bits(e.pose).tolist())
            t = e.trace()
            per_rank[r]["trace"].append({k: t[k] for k in TRACE})
    sync()
    for r, e in enumerate(engs):
        assert per_rank[r]["pose"] == one["pose"] and per_rank[r]["trace"] == one["trace"]
        p = e.particles()
        per_rank[r]["particles"] = {k: p[k].copy() for k in ("x", "y", "theta", "w")}
        per_rank[r]["map"] = e.map().tobytes()
        assert per_rank[r]["map"] == one["map"]
        e.close()
    path = str(tmp_path_factory.mktemp("gates") / "record.npz")
    np.savez(path, g17=np.stack(g17), g15=np.stack(g15), g10=np.stack(g10))
    return {"path": path, "per_rank": per_rank, "wl": wl, "ms_per_frame": ref["ms_per_frame"]}


@pytest.mark.parametrize("delay_k", [0, 1], ids=["delay_poses", "delay_keys"])
@pytest.mark.parametrize("rank", [0, 2], ids=["rank0", "rank_last"])
def test_async_gathers_gates_mode_one_handle_per_process(gates_record, rank, delay_k, tmp_path):
    """Matrix B: one rank of GATES_WL alone in a fresh process (the only live handle: its edges are gates), every collective on the stream
    pfslam_shard_stream names: the delay kernel, its peers' slices from pinned host memory, its own slice device-to-device from its local
    buffer.  The same per-frame poses, traces, final particles and map as the rank of the synchronised run; gates in every frame."""
    rec = gates_record
    wl = rec["wl"]
    out = str(tmp_path / "child.npz")
    args = [sys.executable, os.path.abspath(__file__), "gates-child", rec["path"], GATES_WL, str(rank), str(delay_k), "%.6f" % rec["ms_per_frame"], out]
    p = subprocess.run(args, capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    got = np.load(out)
    res = json.loads(str(got["json"]))
    want = rec["per_rank"][rank]
    n_stepped = len(wl.scans)
    modes = res["modes"]
    assert len(modes) == n_stepped
    assert all(m["gates"] and m["round5_frame"] and not m["serial"] for m in modes[1:]), modes
    assert sum(a != b for a, b in res["streams"]) >= n_stepped - 3
    ms = res["delay_ms"]
    assert len(ms) == n_stepped - FIRST_DELAYED and min(ms) >= DELAY_FACTOR * rec["ms_per_frame"], (ms, rec["ms_per_frame"])
    for i in range(n_stepped):
        assert res["pose"][i] == want["pose"][i], i
        assert res["trace"][i] == want["trace"][i], (i, res["trace"][i], want["trace"][i])
    for fld in ("x", "y", "theta", "w"):
        assert (bits(got[fld]) == bits(want["particles"][fld])).all(), fld
    assert got["map"].tobytes() == want["map"], "the map differs from the synchronised run's"
    assert res["violations"] == 0
    print("rank %d delay %d: gates, %d delays %.2f .. %.2f ms (frame %.3f ms)" % (rank, delay_k, len(ms), min(ms), max(ms), rec["ms_per_frame"]))


def _gates_child(rec_path, wname, rank, delay_k, ms_per_frame, out_path):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    pkg = importlib.import_module("gpu-icp-slam_amd")
    sharded = importlib.import_module("gpu-icp-slam_amd.sharded")
    wl = _Workload(pkg, wname)
    stride, off, cnt = sharded.shard_layout(wl.n, wl.world, rank)
    e = pkg.PfSlam(cnt, kd_capacity=wl.cap, global_offset=off, global_n=wl.n, shard_stride=stride)   # (before any device work of torch's)
    wl.prepare(e)
    import torch
    rec = np.load(rec_path)
    host = {k: [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in rec[k]] for k in ("g17", "g15", "g10")}
    bufs = sharded.GpuBuffers(e, torch, 0)
    cycles = _delay_cycles(_calibrate_sleep(torch, e.shard_stream(0)), ms_per_frame)
    ext, spans, keep = {}, [], []

    def collective(k, local, glob, h_all, delay):
        ptr = e.shard_stream(k)
        s = ext.get(ptr)
        if s is None:
            s = ext[ptr] = torch.cuda.ExternalStream(ptr, device=torch.device("cuda", 0))
        seg = local.numel()
        a, b = rank * seg, (rank + 1) * seg
        assert glob.numel() == h_all.numel() == wl.world * seg
        with torch.cuda.stream(s):
            if delay:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(s)
                torch.cuda._sleep(delay)
                t1.record(s)
                spans.append((t0, t1))
            if a > 0:
                glob[:a].copy_(h_all[:a], non_blocking=True)
            if b < glob.numel():
                glob[b:].copy_(h_all[b:], non_blocking=True)
            glob[a:b].copy_(local, non_blocking=True)
        keep.append(h_all)
        return ptr

    res = {"pose": [], "trace": [], "modes": [], "streams": []}
    try:
        for i, (f, s) in enumerate(zip(wl.frame_ids(), wl.scans)):
            d = cycles if i >= FIRST_DELAYED else 0
            assert e.shard_disperse(f, s) == 0
            local, glob = bufs.pose_blocks()
            s0 = collective(0, local, glob, host["g17"][i], d if delay_k == 0 else 0)
            e.shard_score()
            s1 = collective(1, bufs.pack, bufs.packs, host["g15"][i], d if delay_k == 1 else 0)
            e.shard_weights()
            collective(2, bufs.w, bufs.gw, host["g10"][i], 0)
            e.shard_finish()
            res["streams"].append((s0, s1))
            res["modes"].append(e.frame_mode())
            res["pose"].append(bits(e.pose).tolist())
            t = e.trace()
            res["trace"].append({k: t[k] for k in TRACE})
        e.synchronize()
        torch.cuda.synchronize()
        res["delay_ms"] = [a.elapsed_time(b) for a, b in spans]
        res["violations"] = e.check_cells()["violations"]
        p = e.particles()
        np.savez(out_path, json=json.dumps(res), map=e.map().view(np.uint8), **{k: p[k] for k in ("x", "y", "theta", "w")})
        print("child: results written", flush=True)
    except BaseException:
        import traceback
        traceback.print_exc()
        raise
    finally:
        # torch's pinned-memory cache keeps an event per block, recorded on the handle's streams by the non-blocking copies: nothing of
        # torch's may outlive the handle's streams, so every device operation is finished and torch's objects go before the handle does
        try:
            e.synchronize()
        except Exception:
            pass
        torch.cuda.synchronize()
        del host, keep, spans, ext, bufs
        import gc
        gc.collect()
        e.close()
        print("child: handle closed", flush=True)
        sys.stdout.flush()
        sys.stderr.flush()
        # (and no interpreter teardown: torch's ROCm state outliving the handle's destroyed streams ended a child with SIGSEGV there)
        os._exit(0 if os.path.exists(out_path) else 1)


if __name__ == "__main__":
    if len(sys.argv) == 8 and sys.argv[1] == "gates-child":
        _gates_child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), float(sys.argv[6]), sys.argv[7])
    else:
        sys.exit("usage: %s gates-child RECORD WORKLOAD RANK COLLECTIVE MS_PER_FRAME OUT" % sys.argv[0])
