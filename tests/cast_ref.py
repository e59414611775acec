"""pfslam_cast and pfslam_map_raster restated (include/pfslam.h) in numpy float32, one rounding per operation in the order written.

TEST INFRASTRUCTURE (helper module, not a test).  The raster is a sorted list of cell keys (so that a node 2^20 cells out costs nothing)
with a dense copy of the box when that is small; the cast tests, for every ray, the cells of a block of t at once -- the walk is a closed
form of t, nothing is carried from one cell to the next -- and keeps the smallest t that is occupied.  CleanLidarScan is the CPU oracle's
(orc_clean_lidar_scan); a caller that has the end points from elsewhere (the device-library trigonometry mode, which the oracle does not
have) passes them as `ends`.  tests/test_cast_spec.py pins this file to a cell-by-cell Python loop and holds what the feature is for;
tests/test_cast_kernel_text.py and tests/test_gpu_cast.py hold the kernels and the library to it bit for bit."""
import ctypes as C

import numpy as np

import oracle_lib as O

F = np.float32
CELL_MAX = 1 << 20
MISS = -2**31
DEFAULTS = dict(max_range=30.0, w_min=1.0, no_hit=30.0, inflate=1, skip_cells=1)
MAX_CELLS = 1 << 28
_DENSE = 1 << 26         # a box up to this many cells gets a dense copy


def options(**opts):
    o = dict(DEFAULTS)
    for k in opts:
        if k not in o:
            raise TypeError("no option %r" % k)
    o.update(opts)
    return o


def refusal(nb, m=1, poses=True, res=(0.025, 0.025), have_map=True, reserved=0, raster=False, **opts):
    """The cause the library names for refusing these arguments (before the raster is built), or None; the library's order."""
    o = options(**opts)
    if not raster:
        if m < 1 or m > 65536:
            return "m must be 1 .. 65536"
        if m * nb > 1 << 24:
            return "more than 2^24 rays"
        if not poses and m != 1:
            return "needs m == 1"
    if not np.isfinite(F(o["max_range"])) or not F(o["max_range"]) > 0:
        return "max_range must be finite and > 0"
    if not np.isfinite(F(o["w_min"])):
        return "w_min must be finite"
    if not 0 <= o["inflate"] <= 8:
        return "inflate must be 0 .. 8"
    if o["skip_cells"] < 0:
        return "skip_cells must be >= 0"
    if reserved:
        return "reserved_ must be 0"
    if not (F(o["max_range"]) / F(res[0]) <= F(16384) and F(o["max_range"]) / F(res[1]) <= F(16384)):
        return "must be <= 16384"
    if not have_map:
        return "no map loaded"
    return None


def xyw(nodes):
    """(x, y, w) float32 of a tree (a structured node array) or of an n x 4 array (x, y, z, w)."""
    a = np.asarray(nodes)
    if a.dtype.names:
        return [np.ascontiguousarray(a[k], np.float32) for k in ("x", "y", "w")]
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 4)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 3].copy()


def _key(kx, ky):
    return ((np.asarray(kx, np.int64) + (1 << 22)) << 32) | (np.asarray(ky, np.int64) + (1 << 22))


class Raster:
    """The occupied set O, its box and the two counts for one map and (w_min, inflate)."""

    def __init__(self, nodes, res=(0.025, 0.025), w_min=1.0, inflate=1):
        x, y, w = xyw(nodes)
        self.res = (F(res[0]), F(res[1]))
        with np.errstate(all="ignore"):
            nx, ny = np.rint(x / self.res[0]), np.rint(y / self.res[1])
            ok = (w >= F(w_min)) & (np.abs(nx) <= CELL_MAX) & (np.abs(ny) <= CELL_MAX)       # each is false for a NaN
        self.qualifying = int(ok.sum())
        self.inflate = int(inflate)
        if not self.qualifying:
            self.box = (0, 0, 0, 0)
            self.keys = np.zeros(0, np.int64)
        else:
            cx, cy = nx[ok].astype(np.int64), ny[ok].astype(np.int64)
            self.box = (int(cx.min()) - inflate, int(cy.min()) - inflate, int(cx.max() - cx.min()) + 1 + 2 * inflate, int(cy.max() - cy.min()) + 1 + 2 * inflate)
            own = np.unique(_key(cx, cy))
            ux, uy = (own >> 32) - (1 << 22), (own & 0xffffffff) - (1 << 22)
            d = np.arange(-inflate, inflate + 1, dtype=np.int64)
            self.keys = np.unique(_key((ux[:, None, None] + d[None, :, None]), (uy[:, None, None] + d[None, None, :])).ravel())
        self.occupied = len(self.keys)
        self._dense = None

    def too_large(self):
        return self.box[2] * self.box[3] > MAX_CELLS

    def dense(self):
        """occ as a W x H uint8 array: occ[kx - x0, ky - y0]."""
        if self._dense is None:
            x0, y0, W, H = self.box
            occ = np.zeros((W, H), np.uint8)
            if len(self.keys):
                occ[(self.keys >> 32) - (1 << 22) - x0, (self.keys & 0xffffffff) - (1 << 22) - y0] = 1
            self._dense = occ
        return self._dense

    def has(self, kx, ky):
        """Whether each cell is in O (any integer arrays of one shape)."""
        kx, ky = np.asarray(kx, np.int64), np.asarray(ky, np.int64)
        x0, y0, W, H = self.box
        if W * H <= _DENSE:
            cx, cy = kx - x0, ky - y0
            inside = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
            out = np.zeros(kx.shape, bool)
            if W * H:
                out[inside] = self.dense()[cx[inside], cy[inside]] != 0
            return out
        k = _key(np.clip(kx, -(1 << 21), 1 << 21), np.clip(ky, -(1 << 21), 1 << 21))
        at = np.minimum(np.searchsorted(self.keys, k), max(len(self.keys) - 1, 0))
        return (self.keys[at] == k) if len(self.keys) else np.zeros(kx.shape, bool)

    def stats(self, rays=0, hits=0):
        return np.array([rays, hits, self.qualifying, self.occupied] + list(self.box), np.int64)


def oracle_ends(pose, nb, max_range):
    """(x + wx, y + wy) of every beam, float32: CleanLidarScan(b, max_range, theta) of the CPU oracle, then one float addition each."""
    L = O.lib()
    x, y, th = [F(v) for v in pose]
    wx, wy = C.c_float(), C.c_float()
    X, Y = np.empty(nb, np.float32), np.empty(nb, np.float32)
    with np.errstate(all="ignore"):
        for b in range(nb):
            L.orc_clean_lidar_scan(b, float(F(max_range)), float(th), C.byref(wx), C.byref(wy))
            X[b], Y[b] = x + F(wx.value), y + F(wy.value)
    return X, Y


def cast(raster, poses, nb, ends=None, block=96, **opts):
    """pfslam_cast for the m x 3 poses: dict(ranges m x nb float32, cells m x nb x 2 int32, stats int64[8]).  `ends(pose, nb, max_range)`
    gives (x + wx, y + wy) per beam (default: the oracle's)."""
    o = options(**opts)
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 3)
    m = len(poses)
    rx, ry = raster.res
    X, Y = np.empty((m, nb), np.float32), np.empty((m, nb), np.float32)
    for r in range(m):
        X[r], Y[r] = (ends or oracle_ends)(poses[r], nb, o["max_range"])
    px, py = np.repeat(poses[:, 0], nb), np.repeat(poses[:, 1], nb)
    with np.errstate(all="ignore"):
        fsx, fex, fsy, fey = np.rint(px / rx), np.rint(X.ravel() / rx), np.rint(py / ry), np.rint(Y.ravel() / ry)
        ok = (np.abs(fsx) <= CELL_MAX) & (np.abs(fex) <= CELL_MAX) & (np.abs(fsy) <= CELL_MAX) & (np.abs(fey) <= CELL_MAX)
    z = np.zeros(m * nb, np.int64)
    sx, ex, sy, ey = [np.where(ok, v, 0).astype(np.int64) for v in (fsx, fex, fsy, fey)]
    dx, dy = ex - sx, ey - sy
    adx, ady = np.abs(dx), np.abs(dy)
    n = np.where(ok, np.maximum(adx, ady), z)
    xmajor = adx >= ady
    hit_t = np.full(m * nb, -1, np.int64)
    walking = np.nonzero(ok & (n > 0) & (n >= o["skip_cells"]))[0]
    for lo in range(0, len(walking), 8192):              # (a bound on the memory, nothing else)
        alive = walking[lo:lo + 8192]
        t0 = int(o["skip_cells"])
        while len(alive):
            t = t0 + np.arange(block, dtype=np.int64)[None, :]
            a = alive[:, None]
            nn = n[a]
            minor = (2 * t * np.where(xmajor[a], ady[a], adx[a]) + nn) // (2 * nn)
            kx = sx[a] + np.sign(dx[a]) * np.where(xmajor[a], t, minor)
            ky = sy[a] + np.sign(dy[a]) * np.where(xmajor[a], minor, t)
            occ = raster.has(kx, ky) & (t <= nn)
            any_hit = occ.any(axis=1)
            hit_t[alive[any_hit]] = t0 + occ[any_hit].argmax(axis=1)
            t0 += block
            alive = alive[~any_hit & (n[alive] >= t0)]
    ranges = np.full(m * nb, F(o["no_hit"]), np.float32)
    cells = np.full((m * nb, 2), MISS, np.int64)
    h = np.nonzero(hit_t >= 0)[0]
    if len(h):
        t, nn = hit_t[h], n[h]
        minor = (2 * t * np.where(xmajor[h], ady[h], adx[h]) + nn) // (2 * nn)
        kx = sx[h] + np.sign(dx[h]) * np.where(xmajor[h], t, minor)
        ky = sy[h] + np.sign(dy[h]) * np.where(xmajor[h], minor, t)
        ddx, ddy = kx.astype(np.float32) * rx - px[h], ky.astype(np.float32) * ry - py[h]
        ranges[h] = np.sqrt(ddx * ddx + ddy * ddy)
        cells[h, 0], cells[h, 1] = kx, ky
    return {"ranges": ranges.reshape(m, nb), "cells": cells.astype(np.int32).reshape(m, nb, 2), "stats": raster.stats(m * nb, len(h))}


def cast_map(nodes, poses, nb, res=(0.025, 0.025), ends=None, **opts):
    o = options(**opts)
    return cast(Raster(nodes, res, o["w_min"], o["inflate"]), poses, nb, ends, **opts)


def same(got, want, cells=True):
    """None when two cast() results agree bit for bit, else a description of the first difference."""
    g, w = np.ascontiguousarray(got["ranges"], np.float32), np.ascontiguousarray(want["ranges"], np.float32)
    if g.shape != w.shape:
        return "ranges: shape %r != %r" % (g.shape, w.shape)
    bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
    if len(bad):
        i = tuple(bad[0])
        return "ranges differ at %d places, first %r: %r != %r" % (len(bad), i, g[i], w[i])
    if cells:
        bad = np.argwhere(np.asarray(got["cells"]) != np.asarray(want["cells"]))
        if len(bad):
            i = tuple(bad[0][:2])
            return "cells differ at %d places, first %r: %r != %r" % (len(bad), i, got["cells"][i].tolist(), want["cells"][i].tolist())
    if list(got["stats"]) != list(want["stats"]):
        return "stats: %r != %r" % (list(got["stats"]), list(want["stats"]))
    return None
