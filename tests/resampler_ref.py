"""PFResample restated from the CPU oracle's own exported primitives, for the three resampler modes of pfslam_set_resampler.

TEST INFRASTRUCTURE (helper module, not a test).  The CPU oracle is frozen and knows only the reference's seeding (mode 0).  This
restatement takes its sums from orc_sum_f32, its cdf from orc_inclusive_scan_f32, its seeds and draws from orc_engine_seed and
orc_uniform_real, and searches the first index with `not (rnd > cdf[idx])` exactly as orc_weighted_sample_indices does;
tests/test_resampler_spec.py pins it to orc_resample in mode 0 (neff bits and every source index), which proves every line of it except
the one that differs between the modes -- where thread i takes its rnd from (include/pfslam.h):

  0  rnd_i = uniform_real(engine_seed((int)Neff, frame, i), 0, maxv)                      the reference, collisions included (H5)
  1  rnd_i = uniform_real(engine_seed((int)Neff, i, frame), 0, maxv)                      one multinomial draw per particle
  2  u = uniform_real(engine_seed((int)Neff, frame, 0), 0, 1);  rnd_i = (float)(((i + u) * maxv) / gn)   systematic; Python floats are
     IEEE doubles, so the three operations below run in double in the order written and np.float32 rounds once."""
import ctypes as C

import numpy as np

import oracle_lib as O

EFFECTIVE_PARTICLES = 0.7   # kernel.cu:474


def sums_and_cdf(w):
    """(Neff as np.float32, cdf) of the weights w, with the oracle's canonical sum and scan (orc_resample's first lines)."""
    L = O.lib()
    w = np.ascontiguousarray(w, np.float32)
    n = len(w)
    w2 = np.ascontiguousarray(w * w)                      # kernCopyWeights squared: one float product each
    r2 = np.float32(L.orc_sum_f32(O.P(w2), n, 1))
    r = np.float32(L.orc_sum_f32(O.P(w), n, 1))
    with np.errstate(all="ignore"):
        neff = np.float32(np.float32(r * r) / r2)
    cdf = np.zeros(n, np.float32)
    L.orc_inclusive_scan_f32(O.P(w), n, O.P(cdf))
    return neff, cdf


def seed(neff, frame, i, mode):
    L = O.lib()
    if mode == 0:
        return L.orc_engine_seed(int(neff), frame, i)
    if mode == 1:
        return L.orc_engine_seed(int(neff), i, frame)
    return L.orc_engine_seed(int(neff), frame, 0)


def draws(neff, cdf, frame, mode):
    """rnd_i for every i < gn, as np.float32."""
    L = O.lib()
    gn = len(cdf)
    maxv = float(cdf[gn - 1])
    rnd = np.empty(gn, np.float32)
    if mode == 2:
        st = C.c_uint32(seed(neff, frame, 0, 2))
        u = float(L.orc_uniform_real(C.byref(st), 0.0, 1.0))
        for i in range(gn):
            rnd[i] = np.float32(((float(i) + u) * maxv) / float(gn))
        return rnd
    for i in range(gn):
        st = C.c_uint32(seed(neff, frame, i, mode))
        rnd[i] = L.orc_uniform_real(C.byref(st), 0.0, maxv)
    return rnd


def first_index(cdf, rnd):
    """`while (idx < n && rnd > cdf[idx]) idx++`, clamped to n - 1 -- for a non-monotone cdf too (H8): the first idx with not (rnd > cdf[idx])
    is the first idx whose running maximum is not below rnd, NaNs aside (a NaN cdf entry stops the walk: not (rnd > NaN))."""
    n = len(cdf)
    stop = ~(rnd[:, None] > cdf[None, :]) if n <= 2048 else None
    if stop is not None:
        idx = np.where(stop.any(axis=1), stop.argmax(axis=1), n - 1)
        return idx.astype(np.int32)
    out = np.empty(len(rnd), np.int32)
    for k, r in enumerate(rnd):
        s = ~(r > cdf)
        out[k] = s.argmax() if s.any() else n - 1
    return out


def resample_ref(particles, frame, mode):
    """-> (did, neff as np.float32, src): whether PFResample resamples these particles, and from which source every slot is filled."""
    neff, cdf = sums_and_cdf(particles["w"])
    gn = len(cdf)
    if not (float(neff) < EFFECTIVE_PARTICLES * gn):
        return 0, neff, None
    return 1, neff, first_index(cdf, draws(neff, cdf, frame, mode))
