"""pfslam_search_scan restated: tests/search_ref.py's Search, unchanged, on a field whose source is a list of points -- the end points of
a reference scan (register_ref.targets: step 1 of pfslam_register at the reference pose) -- instead of a tree's nodes.

TEST INFRASTRUCTURE (helper module, not a test).  PointField has search_ref.Field's interface (.res, .q(kx, ky, u, qcap)) and is brute
force over ALL points in numpy float32, one rounding per operation in the order of include/pfslam.h:
    dx = px - (float)kx * res     dy = py - (float)ky * res     d2 = min over the points of dx * dx + dy * dy
(pfslam_nearest's d2 with both z at 0: a square does not see the sign of its difference).  tests/test_search_scan_spec.py ties it to
search_ref.Field and holds the radius the device's builder visits to it; tests/test_search_scan_kernel_text.py and
tests/test_gpu_search_scan.py hold the kernels and the library to it, integer for integer and bit for bit."""
import numpy as np

import register_ref as R
import search_ref as S

F = np.float32


class PointField:
    """q of the lattice cells for one list of points (n x 2, any float32 values; a row with a NaN is no point), computed on demand, kept."""

    def __init__(self, points, res=0.025):
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        self.px, self.py = pts[:, 0].copy(), pts[:, 1].copy()
        self.res = F(res)
        self.keys = np.zeros(0, np.int64)
        self.d2 = np.zeros(0, np.float32)

    def brute_d2(self, kx, ky, chunk=2048):
        """d2 of every cell over every point; +inf with no point (and for a cell whose every d2 is a NaN)."""
        kx, ky = np.asarray(kx, np.int64).ravel(), np.asarray(ky, np.int64).ravel()
        out = np.full(len(kx), np.inf, np.float32)
        if not len(self.px):
            return out
        with np.errstate(all="ignore"):
            for lo in range(0, len(kx), chunk):
                x = (kx[lo:lo + chunk].astype(np.float32) * self.res)[:, None]
                y = (ky[lo:lo + chunk].astype(np.float32) * self.res)[:, None]
                dx, dy = self.px[None, :] - x, self.py[None, :] - y
                d = dx * dx + dy * dy
                out[lo:lo + chunk] = np.where(np.isnan(d), np.float32(np.inf), d).min(axis=1)
        return out

    def lookup_d2(self, kx, ky):
        k = S.Field.key(kx, ky)
        need = np.setdiff1d(np.unique(k), self.keys)
        if len(need):
            nkx, nky = (need >> 32) - (1 << 30), (need & ((1 << 32) - 1)) - (1 << 30)
            keys = np.concatenate([self.keys, need])
            vals = np.concatenate([self.d2, self.brute_d2(nkx, nky)])
            order = np.argsort(keys, kind="stable")
            self.keys, self.d2 = keys[order], vals[order]
        return self.d2[np.searchsorted(self.keys, k)]

    def q(self, kx, ky, u, qcap):
        """min((int)rintf(fdiv(d2, u)), qcap), saturating in float first."""
        with np.errstate(all="ignore"):
            r = np.rint(self.lookup_d2(kx, ky) / F(u))
        return np.where(r >= F(qcap), F(qcap), r).astype(np.int64)


def radius(res, max_dist):
    """R of the device's builder: ceil(max_dist / res) + 2 cells around a point's own cell."""
    return int(np.ceil(F(max_dist) / F(res))) + 2


def limited_q(points, kx, ky, res, u, qcap, rad):
    """q of the cells from only those points whose own cell (rint(px / res), rint(py / res)) is within `rad` cells of the cell in both
    coordinates -- what a splat of radius `rad` leaves; a point whose cell is not finite or lies outside +-(2^20 + rad) takes no part."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
    kx, ky = np.asarray(kx, np.int64).ravel(), np.asarray(ky, np.int64).ravel()
    res = F(res)
    with np.errstate(all="ignore"):
        fx, fy = np.rint(pts[:, 0] / res), np.rint(pts[:, 1] / res)
        ok = (np.abs(fx) <= S.CELL_MAX + rad) & (np.abs(fy) <= S.CELL_MAX + rad)
        pts, cx, cy = pts[ok], fx[ok].astype(np.int64), fy[ok].astype(np.int64)
        x, y = (kx.astype(np.float32) * res)[:, None], (ky.astype(np.float32) * res)[:, None]
        dx, dy = pts[None, :, 0] - x, pts[None, :, 1] - y
        d = dx * dx + dy * dy
        near = (np.abs(cx[None, :] - kx[:, None]) <= rad) & (np.abs(cy[None, :] - ky[:, None]) <= rad)
        d2 = np.where(near, d, np.float32(np.inf)).min(axis=1) if len(pts) else np.full(len(kx), np.inf, np.float32)
        r = np.rint(d2 / F(u))
    return np.where(r >= F(qcap), F(qcap), r).astype(np.int64)


def points_of(ref_scan, ref_pose, targets=None):
    """The points of a reference scan: (n_points x 2 float32)."""
    t, inr = (targets or R.targets)(np.ascontiguousarray(ref_scan, np.float32), np.asarray(ref_pose, np.float32))
    return np.ascontiguousarray(t[inr, :2], np.float32)


def refusal(nb, ref_scan=True, ref_pose=None, centre=None, res=(0.025, 0.025), **opts):
    """The cause pfslam_search_scan names for refusing these arguments, or None.  (The order is the library's: pfslam_search's without the
    map, the NULL reference scan behind the other NULL arguments, the reference pose in front of the centre.)"""
    o = dict(S.DEFAULTS)
    o.update(opts)
    if not ref_scan:
        return "ref_scan_host must not be NULL"
    early = S.refusal(nb, None, res, True, **o)
    if early in ("half_x, half_y and half_theta must be >= 0", "stride must be 1 .. 64", "step_theta must be finite", "max_dist must be finite and > 0"):
        return early
    if ref_pose is not None and not np.isfinite(np.asarray(ref_pose, np.float32)).all():
        return "the ref_pose must be finite"
    if centre is not None and not np.isfinite(np.asarray(centre, np.float32)).all():
        return "the centre must be finite"
    c = centre if centre is not None else (ref_pose if ref_pose is not None else (0.0, 0.0, 0.0))
    return S.refusal(nb, c, res, True, **o)


def search(ref_scan, ref_pose, scan, centre=None, targets=None, res=0.025, field=None, **opts):
    """pfslam_search_scan with the whole score volume: a dict like PfSlam.search_scan(..., scores=True)."""
    rp = np.zeros(3, np.float32) if ref_pose is None else np.asarray(ref_pose, np.float32)
    if field is None:
        field = PointField(points_of(ref_scan, rp, targets), res)
    got = S.search(field, scan, rp if centre is None else centre, targets, **opts)
    got["points"] = len(field.px)
    got["info"][7] = F(len(field.px))
    return got
