"""pfslam_search_cov / pfslam_search_scan_cov restated: the volume and the winner from tests/search_ref.py / tests/search_scan_ref.py, the
weights of include/pfslam.h in numpy (float32 element-wise, one rounding each, in the order written; exp2m in float64, a multiply and an
add per Horner step, never fused), the moments from tests/estimate_ref.py's estimate16 and the border sum from its csum -- the project's
canonical summation order.

TEST INFRASTRUCTURE (helper module, not a test).  tests/test_search_cov_spec.py holds it against float64 and against the two scenarios it
was made for; tests/test_search_cov_kernel_text.py and tests/test_gpu_search_cov.py hold the kernels and the library to it bit for bit."""
import numpy as np

import estimate_ref as E
import search_ref as S
import search_scan_ref as SS

F = np.float32
LOG2E = np.array([0x3fb8aa3b], np.uint32).view(np.float32)[0]          # 1.442695f
C = [float.fromhex(c) for c in (
    "0x1p+0", "-0x1.62e42fefa39efp-1", "0x1.ebfbdff82c58ep-3", "-0x1.c6b08d704a0bfp-5", "0x1.3b2ab6fba4e77p-7", "-0x1.5d87fe78a6730p-10",
    "0x1.430912f86c786p-13", "-0x1.ffcbfc588b0c5p-17", "0x1.62c0223a5c822p-20", "-0x1.b5253d395e7c1p-24", "0x1.e4cf5158b8ec7p-28",
    "-0x1.e8cac7351bb22p-32", "0x1.c3bd650fc2983p-36", "-0x1.816193166d0f7p-40", "0x1.314964d5878a7p-44", "-0x1.c36e843b0401ep-49",
    "0x1.38e89ae79f8b1p-53")]


def exp2m_parts(t):
    """(p, n, live) of float32 arguments t >= 0: p the polynomial's value of f = t - n in float64, live = t < 64."""
    t = np.ascontiguousarray(t, np.float32)
    live = t < F(64.0)                                                  # (false for a NaN)
    tl = np.where(live, t, F(0))
    n = tl.astype(np.int64)                                             # (int)t: towards zero, t >= 0
    f = tl.astype(np.float64) - n.astype(np.float64)
    p = np.full(f.shape, C[16], np.float64)
    for k in range(15, -1, -1):
        p = p * f                                                       # two roundings: numpy has no fused multiply-add
        p = p + C[k]
    return p, n, live


def exp2m(t):
    p, n, live = exp2m_parts(t)
    return np.where(live, (p * np.ldexp(1.0, -n)).astype(np.float32), F(0))


def scale(u, sigma):
    """hs = fdiv(u * 1.442695f, (2.0f * sigma) * sigma)."""
    with np.errstate(all="ignore"):
        return F(F(F(u) * LOG2E) / F(F(F(2.0) * F(sigma)) * F(sigma)))


def weights(vol, smin, hs):
    """w_k of a volume (any shape, flattened k ascending): 0 for the candidates of a heading that takes no part."""
    v = np.asarray(vol, np.int64).ravel()
    part = v != S.NONE
    d = np.where(part, v - smin, 0).astype(np.int32)                    # exact
    with np.errstate(all="ignore"):
        t = d.astype(np.float32) * F(hs)                                # (the conversion rounds to nearest even above 2^24)
    return np.where(part, exp2m(t), F(0)).astype(np.float32)


def poses(c, o, res):
    """(x, y, theta, edge) of every candidate, k ascending; o = the search's options (all six)."""
    hx, hy, ht, stride = o["half_x"], o["half_y"], o["half_theta"], o["stride"]
    nx, ny, na = 2 * hx + 1, 2 * hy + 1, 2 * ht + 1
    c = np.asarray(c, np.float32)
    x = c[0] + ((np.arange(nx) - hx) * stride).astype(np.float32) * F(res)
    y = c[1] + ((np.arange(ny) - hy) * stride).astype(np.float32) * F(res)
    th = c[2] + (np.arange(na) - ht).astype(np.float32) * F(o["step_theta"])
    shape = (na, ny, nx)
    X = np.broadcast_to(x[None, None, :], shape).ravel()
    Y = np.broadcast_to(y[None, :, None], shape).ravel()
    T = np.broadcast_to(th[:, None, None], shape).ravel()
    ex, ey, ea = [(n > 1) & ((np.arange(n) == 0) | (np.arange(n) == n - 1)) for n in (nx, ny, na)]
    edge = (ex[None, None, :] | ey[None, :, None] | ea[:, None, None]).ravel()
    return X.astype(np.float32), Y.astype(np.float32), T.astype(np.float32), edge


def reduce(vol, centre, res, sigma=0.2, **opts):
    """cov_out (16 float32) of a score volume: the reduction alone.  Smin is the volume's smallest score among the headings that take part
    (the winner's, exact where info[4] rounds); with none taking part (status 2) all is zero but [12] and [14]."""
    o = dict(S.DEFAULTS)
    o.update(opts)
    u, _ = S.unit_cap(res, o["max_dist"])
    hs = scale(u, sigma)
    out = np.zeros(16, np.float32)
    cand = int(np.asarray(vol).size)
    v = np.asarray(vol, np.int64).ravel()
    if (v != S.NONE).any():
        w = weights(vol, int(v[v != S.NONE].min()), hs)
        x, y, t, edge = poses(centre, o, res)
        out = E.estimate16(x, y, t, w)
        with np.errstate(all="ignore"):
            out[13] = F(E.csum(np.where(edge, w, F(0)).astype(np.float32)) / out[10])
    out[12], out[14] = F(cand), hs
    return out


def with_cov(got, centre, res, sigma=0.2, **opts):
    """A search's dict (with its volume) plus raw, mean, cov, neff, edge as PfSlam.search_cov() returns them."""
    raw = reduce(got["scores"], centre, res, sigma, **opts)
    c = raw[3:9]
    got.update({"raw": raw, "mean": raw[0:3].copy(), "cov": np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]], np.float32),
                "neff": float(raw[9]), "edge": float(raw[13])})
    return got


def search_cov(field, scan, centre, targets=None, sigma=0.2, **opts):
    """pfslam_search_cov with the whole volume."""
    return with_cov(S.search(field, scan, centre, targets, **opts), centre, field.res, sigma, **opts)


def search_scan_cov(ref_scan, ref_pose, scan, centre=None, targets=None, res=0.025, field=None, sigma=0.2, **opts):
    """pfslam_search_scan_cov with the whole volume."""
    rp = np.zeros(3, np.float32) if ref_pose is None else np.asarray(ref_pose, np.float32)
    got = SS.search(ref_scan, rp, scan, centre, targets, res, field, **opts)
    return with_cov(got, rp if centre is None else centre, res, sigma, **opts)


def refusal(nb, scan_form=True, sigma=0.2, reserved=(0, 0, 0), cov=True, cov_out=True, **kw):
    """The cause pfslam_search_scan_cov (scan_form) or pfslam_search_cov names for refusing these arguments, or None: a NULL cov or
    cov_out with the other NULL arguments, then search_scan_ref.refusal's / search_ref.refusal's causes in their order (kw: their
    arguments), then the covariance's own."""
    if not cov or not cov_out:
        return "bad argument"
    if scan_form:
        early = SS.refusal(nb, **kw)
    else:
        kw = dict(kw)
        early = S.refusal(nb, kw.pop("centre", None), **kw)
    if early is not None:
        return early
    res, max_dist = kw.get("res", (0.025, 0.025))[0], kw.get("max_dist", S.DEFAULTS["max_dist"])
    s = F(sigma)
    if not np.isfinite(s) or not s > 0:
        return "sigma must be finite and > 0"
    if any(reserved):
        return "the reserved_ of pfslam_cov_opts must be 0"
    hs = scale(S.unit_cap(res, max_dist)[0], s)
    if not np.isfinite(hs) or not hs > 0:
        return "it must be finite and > 0"
    return None


def same_cov(got, want):
    """None when two cov_out agree bit for bit, else the first difference."""
    g, w = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if (g.view(np.int32) == w.view(np.int32)).all():
        return None
    k = int(np.flatnonzero(g.view(np.int32) != w.view(np.int32))[0])
    return "cov_out[%d]: %r != %r (got %r, want %r)" % (k, float(g[k]), float(w[k]), g.tolist(), w.tolist())
