"""pfslam_search_best restated on top of tests/search_ref.py and tests/search_wide_ref.py: the cells, their representatives read off the full
score volume, and the level-synchronous descent with the table of one key per cell, the threshold and the two drop rules of
include/pfslam.h, in numpy.

TEST INFRASTRUCTURE (helper module, not a test).  The rows are DEFINED by representatives(): the volume, cut into cells, the smallest key
of each.  descend() is the method; tests/test_search_best_spec.py holds it to the definition, the kernel text
(tests/test_search_best_kernel_text.py) and the library (tests/test_gpu_search_best.py) are held to the definition too."""
import numpy as np

import search_ref as S
import search_wide_ref as Wd

NONE = np.int64(2**63 - 1)            # a cell without a representative (the library's all ones)
SLICES = 4096
MAX_COUNT, MAX_CELLS = 64, 1 << 22
DEFAULTS = dict(count=8, tile_log2=3, group_theta=8)


def refusal(count, tile_log2, group_theta, nx=1, ny=1, na=1, reserved=0):
    """The cause pfslam_search_best names for refusing these pfslam_best_opts on a window it would otherwise take, or None."""
    if not 1 <= count <= MAX_COUNT:
        return "count must be 1 .. 64"
    if not 0 <= tile_log2 <= 7:
        return "tile_log2 must be 0 .. 7"
    if group_theta < 1:
        return "group_theta must be >= 1"
    if reserved:
        return "reserved_ must be 0"
    if (((nx - 1) >> tile_log2) + 1) * (((ny - 1) >> tile_log2) + 1) * ((na - 1) // group_theta + 1) > MAX_CELLS:
        return "more than 2^22 cells"
    return None


class Best:
    """The cells of one call (a search_ref.Search, tile_log2, group_theta)."""

    def __init__(self, s, tile_log2, group_theta):
        assert 0 <= tile_log2 <= 7 and group_theta >= 1
        self.s, self.ls, self.g = s, tile_log2, group_theta
        self.tx, self.ty = ((s.nx - 1) >> tile_log2) + 1, ((s.ny - 1) >> tile_log2) + 1
        self.groups = (s.na - 1) // group_theta + 1
        self.cells = self.tx * self.ty * self.groups

    def cell(self, k):
        s = self.s
        k = np.asarray(k, np.int64)
        i, j, a = k % s.nx, (k // s.nx) % s.ny, k // (s.nx * s.ny)
        return ((a // self.g) * self.ty + (j >> self.ls)) * self.tx + (i >> self.ls)

    def representatives(self, vol):
        """One key per cell from the full volume: the smallest S << 32 | k among the cell's candidates that take part, NONE without one."""
        s = self.s
        flat = np.asarray(vol, np.int64).ravel()
        k = np.arange(s.cand, dtype=np.int64)
        live = np.repeat(np.array([s.ends(a)[3] > 0 for a in range(s.na)]), s.nx * s.ny)
        T = np.full(self.cells, NONE, np.int64)
        np.minimum.at(T, self.cell(k[live]), (flat[live] << 32) | k[live])
        return T

    def rows(self, vol, count):
        """The definition: the keys of the `count` cells with the smallest representatives, ascending, as (S, k) pairs."""
        T = np.sort(self.representatives(vol))
        return [(int(v >> 32), int(v & 0xffffffff)) for v in T[:count] if v != NONE]

    @staticmethod
    def threshold(T, count, slices):
        """An upper bound of the final count-th smallest representative: the count-th smallest of T, or of its slice minima."""
        if slices:
            m = np.full(SLICES, NONE, np.int64)
            np.minimum.at(m, np.arange(len(T)) % SLICES, T)
            T = m
        return np.sort(T)[count - 1] if len(T) >= count else NONE

    def descend(self, count, slices=False, loose=False, top=None):
        """The level-synchronous descent: the rows as (S, k) pairs and the counts {bounded, scored, top}.  slices: the threshold from the
        4096 slice minima instead of the exact count-th smallest.  loose: a WRONG rule for the tests -- drop on LB >= the other side's S."""
        s, w = self.s, Wd.Wide(self.s)
        top = Wd.top_level(s.nx, s.ny) if top is None else top
        step = 1 << top
        J0, I0 = np.meshgrid(np.arange(0, s.ny, step), np.arange(0, s.nx, step), indexing="ij")
        nodes = {a: (I0.ravel(), J0.ravel()) for a in range(s.na) if s.ends(a)[3] > 0}
        T, count_of = np.full(self.cells, NONE, np.int64), {"bounded": 0, "scored": 0, "top": top}
        for L in range(top, -1, -1):
            level = []
            for a, (I, J) in nodes.items():
                if not len(I):
                    continue
                k0 = (a * s.ny + J) * s.nx + I
                lo, S0 = w.lb(a, I, J, L), w.lb(a, I, J, 0)
                assert (lo <= S0).all()
                count_of["scored" if L == 0 else "bounded"] += len(I)
                np.minimum.at(T, self.cell(k0), (S0 << 32) | k0)          # every node scored offers its origin to its cell
                level.append((a, I, J, k0, lo))
            if L == 0:
                break
            # after the whole level: the threshold, then the two rules
            thr = self.threshold(T, count, slices)
            half, nodes = 1 << (L - 1), {}
            for a, I, J, k0, lo in level:
                nk, mine = (lo << 32) | k0, T[self.cell(k0)]
                if loose:
                    keep = (lo < (thr >> 32)) & ((L > self.ls) | (lo < (mine >> 32)))
                else:
                    keep = (nk <= thr) & ((L > self.ls) | (nk <= mine))
                I, J = I[keep], J[keep]
                ci = np.concatenate([I, I + half, I, I + half])
                cj = np.concatenate([J, J, J + half, J + half])
                ok = (ci < s.nx) & (cj < s.ny)
                nodes[a] = (ci[ok], cj[ok])
        T = np.sort(T)
        return [(int(v >> 32), int(v & 0xffffffff)) for v in T[:count] if v != NONE], count_of


def result_dict(s, rows, count_of=None, cells=0):
    """PfSlam.search_best's dict for the rows (S, k) of the call s."""
    poses, info = np.zeros((len(rows), 3), np.float32), np.zeros((len(rows), 8), np.float32)
    for r, (Sr, k) in enumerate(rows):
        poses[r], info[r] = s.result_of(Sr, k)
    return {"poses": poses, "info": info, "index": np.array([k for _, k in rows], np.int64), "score": np.array([v for v, _ in rows], np.int64),
            "beams": info[:, 2].astype(np.int32), "found": len(rows), "candidates": s.cand, "cells": cells, "count": count_of}


def search_best(field, scan, centre, count=8, tile_log2=3, group_theta=8, targets=None, volume=True, **opts):
    """pfslam_search_best: by the definition (volume=True: the full volume's representatives) or by the restated descent."""
    s = S.Search(field, scan, centre, targets, **opts)
    b = Best(s, tile_log2, group_theta)
    if volume:
        return result_dict(s, b.rows(s.volume(), count), None, b.cells)
    rows, count_of = b.descend(count)
    return result_dict(s, rows, count_of, b.cells)


def same_rows(got, want):
    """None when two search_best() results agree -- found, index, poses and info bit for bit -- else the first difference."""
    import register_ref as R
    if got["found"] != want["found"]:
        return "found: %d != %d" % (got["found"], want["found"])
    if not (np.asarray(got["index"]) == np.asarray(want["index"])).all():
        return "index: %r != %r" % (np.asarray(got["index"]).tolist(), np.asarray(want["index"]).tolist())
    for name in ("poses", "info"):
        g, w = np.asarray(got[name], np.float32).reshape(want["found"], -1), np.asarray(want[name], np.float32)
        if not (R.bits(g) == R.bits(w)).all():
            r = int(np.flatnonzero((R.bits(g) != R.bits(w)).any(axis=1))[0])
            return "%s of row %d: %r != %r" % (name, r, g[r].tolist(), w[r].tolist())
    return None
