"""pfslam_search restated: the specification of include/pfslam.h in numpy float32 element-wise operations (one rounding each, in the order
written) on top of tests/register_ref.py's nearest (brute force over every node) and targets (the CPU oracle's CleanLidarScan).

TEST INFRASTRUCTURE (helper module, not a test).  The field is computed only for the cells a case touches and kept per tree, so that
the cases of one module share it.  tests/test_search_spec.py holds the rule to its edge cases and to the scenario it was made for;
tests/test_search_kernel_text.py and tests/test_gpu_search.py hold the kernels and the library to this, integer for integer and bit
for bit."""
import numpy as np

import register_ref as R

F = np.float32
DEFAULTS = dict(half_x=20, half_y=20, half_theta=16, stride=1, step_theta=0.0125, max_dist=0.2)
CELL_MAX = 1 << 20
NONE = 2**31 - 1                  # the score of a heading without an in-range beam
MAX_CAND, MAX_ENDS, MAX_FIELD = 1 << 24, 1 << 24, 1 << 26


def unit_cap(res, max_dist):
    """(u, qcap as a float32: the caller decides whether it is in range)."""
    res, md = F(res), F(max_dist)
    with np.errstate(all="ignore"):
        u = F(F(res * res) * F(0.0625))
        return u, np.rint(F(F(md * md) / u))


def refusal(nb, centre, res=(0.025, 0.025), have_map=True, **opts):
    """The cause pfslam_search names for refusing these arguments, or None.  (The order is the library's.)"""
    o = dict(DEFAULTS)
    o.update(opts)
    if o["half_x"] < 0 or o["half_y"] < 0 or o["half_theta"] < 0:
        return "half_x, half_y and half_theta must be >= 0"
    if not 1 <= o["stride"] <= 64:
        return "stride must be 1 .. 64"
    if not np.isfinite(F(o["step_theta"])) or (o["half_theta"] > 0 and not F(o["step_theta"]) > 0):
        return "step_theta must be finite"
    if not np.isfinite(F(o["max_dist"])) or not F(o["max_dist"]) > 0:
        return "max_dist must be finite and > 0"
    if centre is not None and not np.isfinite(np.asarray(centre, np.float32)).all():
        return "the centre must be finite"
    nx, ny, na = 2 * o["half_x"] + 1, 2 * o["half_y"] + 1, 2 * o["half_theta"] + 1
    if nx * ny * na > MAX_CAND:
        return "more than 2^24 candidates"
    if not have_map:
        return "no map loaded"
    if nb > 4096:
        return "n_beams > 4096"
    if F(res[0]) != F(res[1]):
        return "map_res_x != map_res_y"
    _, q = unit_cap(res[0], o["max_dist"])
    if not (q >= 1 and q <= 65535):
        return "it must be 1 .. 65535"
    if na * nb > MAX_ENDS:
        return "more than 2^24 end points"
    if centre is not None:
        c, r = np.asarray(centre, np.float32), F(res[0])
        with np.errstate(all="ignore"):
            side = []
            for v, h in ((c[0], o["half_x"]), (c[1], o["half_y"])):
                lo, hi = [int(np.clip(np.rint(F(F(v + F(d)) / r)), -CELL_MAX, CELL_MAX)) for d in (-20.0, 20.0)]
                side.append(hi - lo + 1 + 2 * h * o["stride"])
        if side[0] * side[1] > MAX_FIELD:
            return "at most 2^26 cells"
    return None


class Field:
    """d2 of the lattice cells of one tree (pfslam_nearest's d2 of ((float)kx * res, (float)ky * res, 0)), computed on demand and kept."""

    def __init__(self, tree, res=0.025):
        self.tree, self.res = tree, F(res)
        self.keys = np.zeros(0, np.int64)
        self.d2 = np.zeros(0, np.float32)

    @staticmethod
    def key(kx, ky):
        return (np.asarray(kx, np.int64) + (1 << 30)) * (1 << 32) + (np.asarray(ky, np.int64) + (1 << 30))

    def lookup_d2(self, kx, ky):
        k = self.key(kx, ky)
        need = np.setdiff1d(np.unique(k), self.keys)
        if len(need):
            nkx, nky = (need >> 32) - (1 << 30), (need & ((1 << 32) - 1)) - (1 << 30)
            q = np.zeros((len(need), 3), np.float32)
            q[:, 0] = nkx.astype(np.float32) * self.res
            q[:, 1] = nky.astype(np.float32) * self.res
            _, d2 = R.nearest(self.tree, q)
            keys = np.concatenate([self.keys, need])
            vals = np.concatenate([self.d2, d2])
            order = np.argsort(keys, kind="stable")
            self.keys, self.d2 = keys[order], vals[order]
        return self.d2[np.searchsorted(self.keys, k)]

    def q(self, kx, ky, u, qcap):
        """min((int)rintf(fdiv(d2, u)), qcap), saturating in float first (a d2 of +inf or one too large for the conversion has qcap)."""
        with np.errstate(all="ignore"):
            r = np.rint(self.lookup_d2(kx, ky) / F(u))
        return np.where(r >= F(qcap), F(qcap), r).astype(np.int64)


class Search:
    """One call: the candidates' geometry, the end points per heading, the scores of a heading or of single candidates, the result."""

    def __init__(self, field, scan, centre, targets=None, **opts):
        o = dict(DEFAULTS)
        o.update(opts)
        self.o, self.field, self.scan = o, field, np.ascontiguousarray(scan, np.float32)
        self.targets = targets or R.targets
        self.c = np.array(centre, np.float32)
        self.res = field.res
        self.u, q = unit_cap(self.res, o["max_dist"])
        assert 1 <= q <= 65535, "qcap %r: the call is refused" % q
        self.qcap = int(q)
        self.hx, self.hy, self.ht, self.stride = o["half_x"], o["half_y"], o["half_theta"], o["stride"]
        self.nx, self.ny, self.na = 2 * self.hx + 1, 2 * self.hy + 1, 2 * self.ht + 1
        self.cand = self.nx * self.ny * self.na
        self._ends = {}

    def theta(self, a):
        return F(self.c[2] + F(F(a - self.ht) * F(self.o["step_theta"])))

    def pose(self, k):
        i, j, a = k % self.nx, (k // self.nx) % self.ny, k // (self.nx * self.ny)
        x = F(self.c[0] + F(F((i - self.hx) * self.stride) * self.res))
        y = F(self.c[1] + F(F((j - self.hy) * self.stride) * self.res))
        return np.array([x, y, self.theta(a)], np.float32)

    def ends(self, a):
        """(ex, ey of the in-range beams that have a cell, in-range beams without one, in-range beams) of heading a."""
        if a not in self._ends:
            t, inr = self.targets(self.scan, (self.c[0], self.c[1], self.theta(a)))
            with np.errstate(all="ignore"):
                fx, fy = np.rint(t[inr, 0] / self.res), np.rint(t[inr, 1] / self.res)
                ok = (np.abs(fx) <= CELL_MAX) & (np.abs(fy) <= CELL_MAX)          # (false for a NaN)
            self._ends[a] = (fx[ok].astype(np.int64), fy[ok].astype(np.int64), int((~ok).sum()), int(inr.sum()))
        return self._ends[a]

    def heading_scores(self, a):
        """S of the (2 hy + 1) x (2 hx + 1) candidates of heading a."""
        ex, ey, bad, n_in = self.ends(a)
        if n_in == 0:
            return np.full((self.ny, self.nx), NONE, np.int64)
        dx = (np.arange(self.nx) - self.hx) * self.stride
        dy = (np.arange(self.ny) - self.hy) * self.stride
        S = np.full((self.ny, self.nx), bad * self.qcap, np.int64)
        if len(ex):
            kx = ex[:, None, None] + dx[None, None, :] + 0 * dy[None, :, None]
            ky = ey[:, None, None] + dy[None, :, None] + 0 * dx[None, None, :]
            S += self.field.q(kx, ky, self.u, self.qcap).sum(axis=0)
        return S

    def volume(self):
        return np.stack([self.heading_scores(a) for a in range(self.na)]).astype(np.int32)

    def scores_at(self, ks):
        """S of single candidates (for a sample of a large window)."""
        out = []
        for k in ks:
            i, j, a = k % self.nx, (k // self.nx) % self.ny, k // (self.nx * self.ny)
            ex, ey, bad, n_in = self.ends(a)
            if n_in == 0:
                out.append(NONE)
                continue
            s = bad * self.qcap
            if len(ex):
                s += int(self.field.q(ex + (i - self.hx) * self.stride, ey + (j - self.hy) * self.stride, self.u, self.qcap).sum())
            out.append(s)
        return np.array(out, np.int64)

    def result_of(self, S, k):
        """pose and info of the winner k with score S (k < 0: no heading has an in-range beam)."""
        info = np.zeros(8, np.float32)
        info[5], info[6] = F(self.cand), F(self.qcap)
        if k < 0:
            info[0], info[1] = 2, -1
            return self.c.copy(), info
        n_in = self.ends(k // (self.nx * self.ny))[3]
        info[1], info[2], info[4] = F(k), F(n_in), F(S)
        info[3] = F(F(F(S) * self.u) / F(n_in))
        return self.pose(k), info

    def pick(self, vol):
        """(S, k) of the smallest score of a volume, the lowest k among equal ones; (0, -1) when no heading takes part."""
        flat = np.asarray(vol, np.int64).ravel()
        live = np.repeat(np.array([self.ends(a)[3] > 0 for a in range(self.na)]), self.nx * self.ny)
        if not live.any():
            return 0, -1
        k = int(np.where(live, flat, np.int64(1) << 40).argmin())       # (argmin: the first among equal ones)
        return int(flat[k]), k


def result_dict(pose, info, scores=None):
    out = {"pose": np.asarray(pose, np.float32), "status": int(info[0]), "index": int(info[1]), "beams": int(info[2]), "mean_d2": float(info[3]),
           "score": int(info[4]), "candidates": int(info[5]), "qcap": int(info[6]), "info": np.asarray(info, np.float32)}
    if scores is not None:
        out["scores"] = scores
    return out


def search(field, scan, centre, targets=None, **opts):
    """pfslam_search with the whole score volume: a dict like PfSlam.search(centre, scores=True, **opts)."""
    s = Search(field, scan, centre, targets, **opts)
    vol = s.volume()
    S, k = s.pick(vol)
    pose, info = s.result_of(S, k)
    return result_dict(pose, info, vol)


def same_result(got, want, volume=True):
    """None when two search() results agree -- pose and info bit for bit, the volume integer for integer -- else the first difference."""
    if not (R.bits(got["pose"]) == R.bits(want["pose"])).all():
        return "pose: %r != %r" % (got["pose"].tolist(), want["pose"].tolist())
    if not (R.bits(got["info"]) == R.bits(want["info"])).all():
        return "info: %r != %r" % (got["info"].tolist(), want["info"].tolist())
    if volume:
        g, w = np.asarray(got["scores"]), np.asarray(want["scores"])
        if g.shape != w.shape:
            return "volume shape: %r != %r" % (g.shape, w.shape)
        if not (g == w).all():
            k = int(np.flatnonzero((g != w).ravel())[0])
            return "%d of %d scores differ, the first at k = %d: %d != %d" % ((g != w).sum(), g.size, k, g.ravel()[k], w.ravel()[k])
    return None
