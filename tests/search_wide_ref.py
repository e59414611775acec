"""pfslam_search_wide restated on top of tests/search_ref.py: the min-pooled pyramid, the lower bound of a block of translations and a
level-synchronous descent with the pruning rule of include/pfslam.h, in numpy.

TEST INFRASTRUCTURE (helper module, not a test).  The pyramid is written as what it MEANS -- M_L[x, y] = the smallest q of the
2^L x 2^L lattice block (step `stride`) with origin (x, y), cut at the call's box -- not as the kernel's four-term recursion, and is
computed only at the cells a bound touches.  tests/test_search_wide_spec.py holds it to search_ref's volume; the kernel text
(tests/test_search_wide_kernel_text.py) and the library (tests/test_gpu_search_wide.py) are held to search_ref's winner."""
import numpy as np

import register_ref as R
import search_ref as S

MAX_LEVEL = 7
MAX_CAND, MAX_ROW = 2**31 - 1, 1 << 24      # candidates of a call, of one heading


def top_level(nx, ny):
    """The smallest L <= 7 with 2^L >= the window's longer side."""
    L = 0
    while L < MAX_LEVEL and (1 << L) < max(nx, ny):
        L += 1
    return L


class Wide:
    """The box, the pyramid and the bounds of one call (a search_ref.Search)."""

    def __init__(self, s):
        self.s = s
        xs = np.concatenate([s.ends(a)[0] for a in range(s.na)])
        ys = np.concatenate([s.ends(a)[1] for a in range(s.na)])
        self.box = None                                   # no beam of any heading has a cell
        if len(xs):
            gx, gy = s.hx * s.stride, s.hy * s.stride
            self.box = (int(xs.min()) - gx, int(xs.max()) + gx, int(ys.min()) - gy, int(ys.max()) + gy)

    def cells(self):
        return 0 if self.box is None else (self.box[1] - self.box[0] + 1) * (self.box[3] - self.box[2] + 1)

    def M(self, L, kx, ky):
        """M_L at the lattice cells (kx, ky) (arrays, inside the box): the smallest q of the block, terms outside the box skipped."""
        s, n = self.s, 1 << L
        kx, ky = np.asarray(kx, np.int64), np.asarray(ky, np.int64)
        d = np.arange(n) * s.stride
        x = kx[..., None, None] + d[None, :] + 0 * d[:, None]
        y = ky[..., None, None] + d[:, None] + 0 * d[None, :]
        inside = (x <= self.box[1]) & (y <= self.box[3])
        assert ((kx >= self.box[0]) & (kx <= self.box[1]) & (ky >= self.box[2]) & (ky <= self.box[3])).all(), "a bound's index leaves the box"
        q = s.field.q(np.where(inside, x, kx[..., None, None]), np.where(inside, y, ky[..., None, None]), s.u, s.qcap)
        return q.min(axis=(-1, -2))

    def lb(self, a, I, J, L):
        """LB of the nodes (a, I[m], J[m], L): bad * qcap + the sum over the beams with a cell of M_L at the origin's cells."""
        s = self.s
        ex, ey, bad, n_in = s.ends(a)
        assert n_in > 0
        I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
        out = np.full(len(I), bad * s.qcap, np.int64)
        if len(ex):
            out += self.M(L, ex[None, :] + ((I - s.hx) * s.stride)[:, None], ey[None, :] + ((J - s.hy) * s.stride)[:, None]).sum(axis=1)
        return out

    def descend(self, top=None):
        """The level-synchronous descent: (S, k) of the winner ((0, -1): no heading takes part) and the counts
        {bounded: nodes above level 0, scored: level-0 candidates, top}."""
        s = self.s
        top = top_level(s.nx, s.ny) if top is None else top
        step = 1 << top
        J0, I0 = np.meshgrid(np.arange(0, s.ny, step), np.arange(0, s.nx, step), indexing="ij")
        nodes = {a: (I0.ravel(), J0.ravel()) for a in range(s.na) if s.ends(a)[3] > 0}
        key, count = None, {"bounded": 0, "scored": 0, "top": top}
        for L in range(top, -1, -1):
            level = []
            for a, (I, J) in nodes.items():
                if not len(I):
                    continue
                k0 = (a * s.ny + J) * s.nx + I
                lo, S0 = self.lb(a, I, J, L), self.lb(a, I, J, 0)
                assert (lo <= S0).all()
                count["scored" if L == 0 else "bounded"] += len(I)
                best = int(np.lexsort((k0, S0))[0])
                cand = (int(S0[best]), int(k0[best]))
                key = cand if key is None or cand < key else key
                level.append((a, I, J, k0, lo))
            if L == 0:
                break
            # after the whole level: a node leaves only if (LB, k0) > the key
            half, nodes = 1 << (L - 1), {}
            for a, I, J, k0, lo in level:
                keep = (lo < key[0]) | ((lo == key[0]) & (k0 <= key[1]))
                I, J = I[keep], J[keep]
                ci = np.concatenate([I, I + half, I, I + half])
                cj = np.concatenate([J, J, J + half, J + half])
                ok = (ci < s.nx) & (cj < s.ny)
                nodes[a] = (ci[ok], cj[ok])
        return (key if key is not None else (0, -1)), count


def search_wide(field, scan, centre, targets=None, top=None, **opts):
    """pfslam_search_wide by the restated descent: search_ref's result dict without the volume, plus the counts."""
    s = S.Search(field, scan, centre, targets, **opts)
    (Smin, k), count = Wide(s).descend(top)
    pose, info = s.result_of(Smin, k)
    out = S.result_dict(pose, info)
    out["index"], out["candidates"], out["count"] = k, s.cand, count
    return out


def tie_case(tree, field, half_x=18, half_y=10):
    """A constructed tie for nb = 1, qcap = 1: (scan, centre, opts) whose one beam ends on a lattice cell with q = 0 for two or more
    candidates of a single-heading window and on cells with q = 1 for most others: two map nodes that sit on lattice points less than
    the window apart, the first of them one cell up and right of the window's central candidate, so that the holders' i and j are odd: none is a block's
    origin above level 0.  The lowest k among the holders wins."""
    res = np.float32(0.025)
    u, _ = S.unit_cap(res, 0.0045)
    kx = np.rint(tree["x"] / res).astype(np.int64)
    ky = np.rint(tree["y"] / res).astype(np.int64)
    zero = np.flatnonzero(field.q(kx, ky, u, 1) == 0)
    cells = np.unique(np.stack([kx[zero], ky[zero]], axis=1), axis=0)
    scan = np.array([5.0], np.float32)
    t, inr = R.targets(scan, (0.0, 0.0, 0.0))
    assert inr[0]
    for n, (x1, y1) in enumerate(cells):
        for x2, y2 in cells[n + 1:]:
            if (x1, y1) != (x2, y2) and abs(x2 - x1) <= half_x and abs(y2 - y1) <= half_y:
                centre = np.array([np.float32(x1 - 1) * res - t[0, 0], np.float32(y1 - 1) * res - t[0, 1], 0.0], np.float32)
                return scan, centre, dict(half_x=half_x, half_y=half_y, half_theta=0, max_dist=0.0045)
    raise AssertionError("the map has no two q = 0 cells within one window of each other")
