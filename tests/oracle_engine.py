"""An engine with the PfSlam stage interface backed by the CPU oracle (TEST INFRASTRUCTURE).  It lets the
multi-GPU orchestration (gpu-icp-slam_amd/sharded.py) run under gloo on CPU: same partitioning, same packed
keys, same collectives -- only the per-rank compute is the oracle's instead of the HIP kernels'."""
import ctypes as C

import numpy as np
import torch

import oracle_lib as O


def f32_to_ordered(f):
    s = np.ascontiguousarray(f, np.float32).view(np.int32).astype(np.int64)
    return (s ^ ((s >> 31) & 0x7fffffff)).astype(np.int64)


def ordered_to_f32(s):
    s = np.int64(s)
    v = np.int32(s ^ ((s >> 31) & 0x7fffffff))
    return np.array([v], np.int32).view(np.float32)[0]


def oracle_map_update(tree, size, robot, scan, cap, bug=0):
    """PFUpdateMapKD (kernel.cu:1406-1540) on a numpy tree buffer; returns the new size."""
    L = O.lib()
    dim = 1600
    fm, wm = O.get_walls(scan, 800, 800, robot[2])
    patch = O.default_patch()
    wall = np.zeros((2048, 4), np.float32)
    free = np.zeros((int(fm.sum()) + 1, 4), np.float32)
    nw, nf = C.c_int(), C.c_int()
    rb = np.ascontiguousarray(robot, np.float32)
    L.orc_masks_to_points(O.P(fm), O.P(wm), dim, dim, C.byref(patch), O.P(rb), O.P(wall), C.byref(nw), O.P(free), C.byref(nf))
    nw, nf = nw.value, nf.value
    if size == 0:
        if nw:
            L.orc_kd_create(O.P(wall), nw, O.P(tree))
        return nw
    if bug:
        free[nw:nf] = 0
    fc, _ = O.traverse_batch(tree, free[:nf, :3])
    wc, _ = O.traverse_batch(tree, wall[:nw, :3])
    L.orc_update_map_kd(O.P(tree), O.P(free), O.P(fc), nf, -1, C.byref(patch))
    L.orc_update_map_kd(O.P(tree), O.P(wall), O.P(wc), nw, 4, C.byref(patch))
    create = np.zeros(max(nw, 1), np.uint8)
    L.orc_test_correspondence(O.P(tree), O.P(wall), O.P(wc), nw, O.P(create), C.byref(patch))
    for i in range(nw):
        if create[i] and size < cap:
            O.kd_insert(tree, size, np.array([wall[i, 0], wall[i, 1], wall[i, 2], -100], np.float32))
            size += 1
    return size


class OracleBuffers:
    def __init__(self, eng):
        self.eng = eng
        self.stats = torch.from_numpy(eng.stats)
        self.pack = torch.from_numpy(eng.pack)
        self.packs = torch.from_numpy(eng.packs)
        self.w = torch.from_numpy(eng.w_pad)
        self.gw = torch.from_numpy(eng.gw_pad)

    def pose_blocks(self):
        return torch.from_numpy(self.eng.pblk), torch.from_numpy(self.eng.gpose)

    def tree_buffers(self, n_nodes):
        # the oracle keeps the reference's 32-byte nodes: one buffer of bytes does for the five device arrays of the GPU handle
        return [torch.from_numpy(self.eng.tree[:n_nodes].view(np.uint8).reshape(-1))]


class OracleShardEngine:
    """Rank `goff // stride` of a job of `gn` particles: the same buffers as the GPU handle (include/pfslam.h, buffers 5, 10,
    14-17), padded to the shard stride."""

    def __init__(self, n_local, goff, gn, kd_capacity=1 << 16, strict_host_mirror=1, balance_period=100, stride=0):
        self.n, self.goff, self.gn, self.cap = n_local, goff, gn, kd_capacity
        self.stride = stride or n_local
        self.world = (gn + self.stride - 1) // self.stride
        self.strict, self.period = strict_host_mirror, balance_period
        z = lambda k: np.zeros(k, np.float32)
        S, n = self.stride, n_local
        self.pblk = z(3 * S)                         # [x | y | theta], stride slots each
        self.x, self.y, self.th = self.pblk[0:n], self.pblk[S:S + n], self.pblk[2 * S:2 * S + n]
        self.w_pad = z(S); self.w = self.w_pad[:n]; self.w[:] = 1
        self.wm = np.ones(n, np.float32)
        # (a one-rank job: the global views alias the local arrays, as buffers 10 / 17 alias 5 / 16 on the GPU handle)
        self.gw_pad = z(self.world * S) if self.world > 1 else self.w_pad
        self.gw = self.gw_pad[:gn]
        self.gpose = z(self.world * 3 * S) if self.world > 1 else self.pblk
        self.stats = np.zeros(8, np.int64)
        self.pack = np.zeros(2, np.int64)            # this shard's packed {kmax, kmin}
        self.packs = np.zeros(2 * self.world, np.int64)
        self.start = z(4)
        self.tree = np.zeros(kd_capacity, O.NODE_DTYPE)
        self.size = 0
        self.robot = z(3)
        self.fit = z(n_local)
        self.scan = None
        self.src = None
        self.icp_delta = None
        self.external, self.builds, self.adopted = False, 0, 0
        # topology graph + loop-closure proposals inside the frame (replicated: pose and 2-D grid only; the KD frame never writes the grid)
        self.topo_mode, self.topo, self._closures = 0, None, np.zeros((0, 2), np.int32)
        self.grid = None

    # ---- helpers
    def _aos(self):
        p = O.make_particles(self.n)
        p["x"], p["y"], p["theta"], p["w"] = self.x, self.y, self.th, self.w
        return p

    def _from_aos(self, p):
        self.x[:], self.y[:], self.th[:], self.w[:] = p["x"], p["y"], p["theta"], p["w"]

    # ---- stage interface
    def set_scan(self, scan): self.scan = np.ascontiguousarray(scan, np.float32)
    def set_pose(self, pose): self.robot[:] = pose
    def set_map(self, tree): self.tree[:len(tree)] = tree; self.size = len(tree)
    def set_stream(self, s): pass
    def synchronize(self): pass
    @property
    def kd_size(self): return self.size
    @property
    def pose(self): return self.robot.copy()

    def set_topology(self, mode=1):
        self.topo_mode = int(mode)
        if self.topo is None:
            self.topo = O.Topology()
            p = O.default_patch()
            dim = int(np.float32(p.scale_x) / np.float32(p.res_x))
            self.grid = np.full((dim, dim), -100, np.int8)
    def closures(self): return self._closures.copy()
    def topology(self): return self.topo.nodes(), self.topo.node_idx
    def map(self): return self.tree[:self.size].copy()
    def particles(self): return self._aos()
    def set_particles(self, p): self._from_aos(p); self.wm[:] = p["w"]
    def shift_particles(self, delta):
        d = np.ascontiguousarray(delta, np.float32)
        self.x += d[0]; self.y += d[1]; self.th += d[2]
        self.robot += d

    def move_particles(self, frame, delta, cov=None, **opts):
        """pfslam_move_particles restated (tests/move_ref.py), the draw keyed by the global index; the weights and their mirror stay."""
        import move_ref as M
        x, y, th = M.move(self.x, self.y, self.th, frame, delta, cov, goff=self.goff, **opts)
        self.x[:], self.y[:], self.th[:] = x, y, th
        self.robot[:] = M.move_pose(self.robot, delta, cov, **opts)

    def maybe_balance(self, frame):
        if self.period > 0 and frame % self.period == 5 and self.size > 0:
            O.lib().orc_kd_balance(O.P(self.tree), self.size)
            self.builds += 1

    # one re-balance per node (include/pfslam.h, pfslam_shard_balance_*)
    def set_shard_balance(self, external): self.external = bool(external)

    def shard_balance_due(self, frame):
        return (self.period > 0 and frame % self.period == 5 and self.size > 0), self.size

    def shard_balance_build(self, frame):
        self.maybe_balance(frame)

    def shard_balance_adopt(self):
        self.adopted += 1

    def update_map_kd(self):
        self.size = oracle_map_update(self.tree, self.size, self.robot, self.scan, self.cap)

    def motion_update(self, frame):
        self.w[:] = self.wm  # H2D of the host-side particle array (kernel.cu:408)
        p = self._aos()
        O.add_noise(p, frame, idx0=self.goff)
        self._from_aos(p)

    def score_kd(self, fetch=True):
        self.fit = O.score_kd(self.tree, self._aos(), self.scan)
        return self.fit if fetch else None

    def measurement_local(self):
        gi = (self.goff + np.arange(self.n)).astype(np.int64)
        self.stats[:] = 0
        self.stats[0] = np.max((f32_to_ordered(self.fit) << 32) | (0xFFFFFFFF - gi))
        self.stats[1] = np.max(f32_to_ordered(-self.fit) << 32)

    def _apply_weights(self):
        fmax = ordered_to_f32(self.stats[0] >> 32)
        fmin = -ordered_to_f32(self.stats[1] >> 32)
        best = int(0xFFFFFFFF - (int(self.stats[0]) & 0xFFFFFFFF))
        rng = np.float32(fmax) - np.float32(fmin)
        if rng > 0:
            p = self._aos()
            O.lib().orc_update_weights_f32(O.P(p), self.n, O.P(self.fit), float(np.float32(1) / rng), int(fmin))
            self._from_aos(p)
        mirror = (self.gn + 1) // 2 if self.strict else 1 << 62
        sel = (self.goff + np.arange(self.n)) < mirror
        self.wm[sel] = self.w[sel]
        return best, float(fmin), float(fmax)

    def shard_disperse(self, frame, scan):
        """pfslam_shard_disperse: scan, re-balance if due, (first scan: seed the map), ICP solve, dispersion."""
        self.set_scan(scan)
        if not self.external:
            self.maybe_balance(frame)
        self.frame = frame
        self._trace = {"best": -1, "resampled": 0, "kd_size": self.size}
        if self.size == 0:
            self.set_pose(np.zeros(3, np.float32))
            self.update_map_kd()
            self._trace["kd_size"] = self.size
            return True
        # the replicated ICP solve depends on the scan, the previous pose and the map only (kernel.cu:984-990, 1081-1092)
        zero = np.zeros(3, np.float32)
        inc, _ = O.icp(self.tree, self.robot, zero, self.scan)
        self.icp_delta = inc.copy()
        self.motion_update(frame)
        return False

    def shard_score(self):
        """pfslam_shard_score: scan-match of this shard -> its packed min / max keys (the 16-byte record)."""
        self.score_kd(fetch=False)
        self.measurement_local()
        self.pack[0], self.pack[1] = self.stats[0], self.stats[1]

    def shard_weights(self):
        """pfslam_shard_weights: merge the gathered records, weights, pose = best particle + ICP increment."""
        rec = self.packs.reshape(self.world, 2)
        self.stats[0], self.stats[1] = rec[:, 0].max(), rec[:, 1].max()
        g = int(0xFFFFFFFF - (int(self.stats[0]) & 0xFFFFFFFF))   # the job's best particle: its pose out of the gathered pose blocks
        S = self.stride
        r, j = g // S, g % S
        blk = self.gpose[r * 3 * S:(r + 1) * 3 * S] if self.world > 1 else self.pblk
        self.start[:3] = (blk[j], blk[S + j], blk[2 * S + j])
        best, _, _ = self._apply_weights()
        self._trace["best"] = best
        self.robot[:] = self.start[:3] + self.icp_delta

    def shard_finish(self):
        """pfslam_shard_finish: the replicated map update at the ICP pose, Neff on the gathered weights, and -- decided
        from Neff alone -- the resample out of the pose blocks gathered right after the dispersion."""
        self.update_map_kd()
        did, neff = self.resample_plan(self.frame)
        if did:
            self.resample_gather()
        self._trace.update(resampled=did, neff=neff, kd_size=self.size)
        if self.topo_mode:  # //UpdateTopology(); //CheckLoopClosure(); (kernel.cu:1750-1751)
            self.topo.update(self.robot)
            self._closures = self.topo.loop_closure(self.grid, self.robot)

    def trace(self):
        return dict(self._trace)

    def resample_plan(self, frame):
        L = O.lib()
        gw = np.ascontiguousarray(self.gw)
        w2 = (gw * gw).astype(np.float32)
        r = np.float32(L.orc_sum_f32(O.P(gw), self.gn, 1))
        r2 = np.float32(L.orc_sum_f32(O.P(w2), self.gn, 1))
        neff = np.float32(r * r) / r2
        did = float(neff) < 0.7 * self.gn
        if did:
            cdf = np.zeros(self.gn, np.float32)
            L.orc_inclusive_scan_f32(O.P(gw), self.gn, O.P(cdf))
            self.src = np.zeros(self.n, np.int32)
            L.orc_weighted_sample_indices(O.P(cdf), self.gn, float(neff), frame, self.goff, self.n, O.P(self.src))
        return int(did), float(neff)

    def resample_gather(self):
        S = self.stride
        r, k = self.src // S, self.src % S
        blk = r.astype(np.int64) * 3 * S
        self.x[:], self.y[:], self.th[:] = self.gpose[blk + k], self.gpose[blk + S + k], self.gpose[blk + 2 * S + k]
        self.w[:] = 1
        self.wm[:] = 1
