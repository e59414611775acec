"""pfslam_estimate restated from the CPU oracle's exported canonical sum.

TEST INFRASTRUCTURE (helper module, not a test).  The CPU oracle is frozen and has no estimate; this restates the specification of
include/pfslam.h with numpy float32 element-wise operations (one rounding each, in the order written) and takes every sum from
orc_sum_f32, the project's canonical, rank-count-independent summation order:

    S0    = csum(w_i)                          S2 = csum(w_i * w_i)
    m_k   = csum(w_i * p_k,i) / S0             k = x, y, theta
    d_k,i = p_k,i - m_k
    C_kl  = csum((w_i * d_k,i) * d_l,i) / S0   (k, l) = xx, xy, xtheta, yy, ytheta, thetatheta
    Neff  = (S0 * S0) / S2

tests/test_estimate_spec.py holds it against a float64 computation; tests/test_gpu_estimate.py holds the GPU to it bit for bit."""
import numpy as np

import oracle_lib as O

PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))   # xx, xy, xtheta, yy, ytheta, thetatheta
F = np.float32


def csum(v):
    v = np.ascontiguousarray(v, np.float32)
    return F(O.lib().orc_sum_f32(O.P(v), len(v), 1))


def estimate16(x, y, theta, w):
    """The 16 floats pfslam_estimate writes, as a float32 array (non-finite where S0 is not finite or not > 0: the library refuses there)."""
    p = [np.ascontiguousarray(a, np.float32) for a in (x, y, theta)]
    w = np.ascontiguousarray(w, np.float32)
    out = np.zeros(16, np.float32)
    with np.errstate(all="ignore"):
        s0 = csum(w)
        s2 = csum(w * w)
        m = [F(csum(w * pk) / s0) for pk in p]
        d = [pk - mk for pk, mk in zip(p, m)]
        out[0:3] = m
        for q, (k, l) in enumerate(PAIRS):
            out[3 + q] = F(csum((w * d[k]) * d[l]) / s0)
        out[9] = F(F(s0 * s0) / s2)
    out[10], out[11], out[12] = s0, s2, F(len(w))
    return out


def estimate_particles(p):
    """estimate16 of a particle array (binding.PARTICLE_DTYPE)."""
    return estimate16(p["x"], p["y"], p["theta"], p["w"])


def estimate_f64(x, y, theta, w):
    """The same quantities in float64 with numpy's own sums: (mean[3], C[6] in PAIRS order, Neff)."""
    p = [np.asarray(a, np.float64) for a in (x, y, theta)]
    w = np.asarray(w, np.float64)
    s0 = w.sum()
    m = [(w * pk).sum() / s0 for pk in p]
    d = [pk - mk for pk, mk in zip(p, m)]
    c = [(w * d[k] * d[l]).sum() / s0 for k, l in PAIRS]
    return np.array(m), np.array(c), s0 * s0 / (w * w).sum()


def cloud(n, weights, seed=0):
    """A pose (12.3, -7.9, 1.1) plus N(0, 0.015 / 0.015 / 0.01) noise as float32; weights: "one", "random" (uniform in (0, 1)) or "zeros"
    (uniform with about a quarter of them exactly zero, never all)."""
    rng = np.random.RandomState(1000003 * seed + n)
    x = (12.3 + rng.normal(0, 0.015, n)).astype(np.float32)
    y = (-7.9 + rng.normal(0, 0.015, n)).astype(np.float32)
    t = (1.1 + rng.normal(0, 0.01, n)).astype(np.float32)
    if weights == "one":
        w = np.ones(n, np.float32)
    else:
        w = rng.uniform(0, 1, n).astype(np.float32)
        w[w == 0] = 0.5
        if weights == "zeros":
            w[rng.uniform(0, 1, n) < 0.25] = 0
            w[n // 2] = 0.75
    return x, y, t, w


def particles_of(x, y, t, w):
    p = np.zeros(len(x), O.PARTICLE_DTYPE)
    p["x"], p["y"], p["theta"], p["w"] = x, y, t, w
    return p
