"""pfslam_cast_score restated (include/pfslam.h) in numpy float32 on top of tests/cast_ref.py's cast, one rounding per operation in the
order written.

TEST INFRASTRUCTURE (helper module, not a test).  The expected range and whether a ray hits are cast_ref.cast's, as the specification
says; this file adds the measured scan, the classes, the rows, the pick and the refusals in the library's order.
tests/test_cast_score_spec.py pins it to a beam-by-beam Python loop and holds what the feature is for;
tests/test_cast_score_kernel_text.py and tests/test_gpu_cast_score.py hold the kernel and the library to it bit for bit."""
import numpy as np

import cast_ref as CR

F = np.float32
DEFAULTS = dict(tol=0.1, clip=1.0, z_min=0.1, z_max=20.0, count_miss=1)
COLUMNS = ("valid", "agree", "through", "short", "miss", "q1", "q2", "cost")
MAX_BEAMS = 4096


def options(**opts):
    o = dict(DEFAULTS)
    for k in opts:
        if k not in o:
            raise TypeError("no option %r" % k)
    o.update(opts)
    return o


def unit(tol, clip):
    """(u, rintf(fdiv(clip, u))) as float32: qcap is the second one where it lies in 16 .. 32767."""
    with np.errstate(all="ignore"):
        u = F(tol) * F(0.0625)
        return u, np.rint(F(clip) / u)


def refusal(nb, m=1, poses=True, source=0, n_particles=None, classes=False, res=(0.025, 0.025), have_map=True, cast=None, cast_reserved=0,
            reserved=0, **opts):
    """The cause the library names for refusing these arguments (before the raster is built), or None; the library's order."""
    o = options(**opts)
    if m < 1 or m > 65536:
        return "m must be 1 .. 65536"
    if nb > MAX_BEAMS:
        return "n_beams must be <= 4096"
    if source not in (0, 1):
        return "source must be 0 .. 1"
    if source == 0 and not poses and m != 1:
        return "needs m == 1"
    if source == 1 and (poses or m != n_particles):
        return "needs poses NULL and m == n_particles"
    if classes and m * nb > 1 << 24:
        return "more than 2^24 rays"
    why = CR.refusal(nb, res=res, reserved=cast_reserved, raster=True, **(cast or {}))
    if why:
        return why
    if not np.isfinite(F(o["tol"])) or not F(o["tol"]) >= F(1e-4):
        return "tol must be finite and >= 1e-4"
    if not np.isfinite(F(o["clip"])):
        return "clip must be finite"
    if not (np.isfinite(F(o["z_min"])) and np.isfinite(F(o["z_max"])) and F(o["z_min"]) <= F(o["z_max"])):
        return "z_min and z_max must be finite, z_min <= z_max"
    if o["count_miss"] not in (0, 1):
        return "count_miss must be 0 or 1"
    if reserved:
        return "reserved_ must be 0"
    fcap = unit(o["tol"], o["clip"])[1]
    if not (fcap >= 16 and fcap <= 32767):
        return "must be 16 .. 32767"
    if not have_map:
        return "no map loaded"
    return None


def best_of(rows):
    """The pick: among the rows with an agreeing beam the smallest cost, then the larger agree, then the lowest row; -1 for none."""
    rows = np.asarray(rows).reshape(-1, 8)
    ok = np.nonzero(rows[:, 1] > 0)[0]
    if not len(ok):
        return -1
    return int(ok[np.lexsort((ok, -rows[ok, 1].astype(np.int64), rows[ok, 7]))[0]])


def score_cast(cast, scan, **opts):
    """The rows of a cast() result (cast_ref.cast's dict) against the measured `scan`: dict(rows m x 8 int32, classes m x nb uint8,
    best, stats int64[8]) and the named columns."""
    o = options(**opts)
    assert refusal(cast["ranges"].shape[1], len(cast["ranges"]), **o) is None
    e = np.ascontiguousarray(cast["ranges"], np.float32)
    hit = np.asarray(cast["cells"])[..., 0] != CR.MISS
    m, nb = e.shape
    z = np.ascontiguousarray(scan, np.float32).reshape(1, nb)
    tol = F(o["tol"])
    u, fcap = unit(o["tol"], o["clip"])
    qcap = int(fcap)
    with np.errstate(all="ignore"):
        valid = np.broadcast_to((z >= F(o["z_min"])) & (z <= F(o["z_max"])), (m, nb))
        d = z - e
        a = np.abs(d)
        fq = np.rint(a / u)
        sat = fq >= F(qcap)
        q = np.where(sat, qcap, np.where(sat, 0, fq).astype(np.int64))
    vh = valid & hit
    classes = np.zeros((m, nb), np.uint8)
    classes[valid & ~hit] = 1
    classes[vh] = 4
    classes[vh & (d > tol)] = 3
    classes[vh & (a <= tol)] = 2
    rows = np.zeros((m, 8), np.int64)
    rows[:, 0] = valid.sum(axis=1)
    for k, c in ((1, 2), (2, 3), (3, 4), (4, 1)):
        rows[:, k] = (classes == c).sum(axis=1)
    rows[:, 5] = np.where(vh, q, 0).sum(axis=1)
    rows[:, 6] = np.where(classes == 2, q * q, 0).sum(axis=1)
    rows[:, 7] = rows[:, 5] + (qcap * rows[:, 4] if o["count_miss"] else 0)
    assert rows.max() < 2**31
    out = {"rows": rows.astype(np.int32), "classes": classes, "best": best_of(rows), "stats": np.asarray(cast["stats"], np.int64).copy(), "qcap": qcap, "u": u}
    for k, name in enumerate(COLUMNS):
        out[name] = out["rows"][:, k]
    return out


def score(raster, poses, scan, nb, ends=None, cast=None, **opts):
    """pfslam_cast_score for the m x 3 poses and the measured scan; `cast` are the cast's options (cast_ref.DEFAULTS over them)."""
    options(**opts)
    return score_cast(CR.cast(raster, poses, nb, ends, **(cast or {})), scan, **opts)


def score_map(nodes, poses, scan, nb, res=(0.025, 0.025), ends=None, cast=None, **opts):
    o = CR.options(**(cast or {}))
    return score(CR.Raster(nodes, res, o["w_min"], o["inflate"]), poses, scan, nb, ends, cast, **opts)


def same(got, want, classes=True):
    """None when two results agree bit for bit (rows, classes, best, stats), else a description of the first difference."""
    g, w = np.asarray(got["rows"]), np.asarray(want["rows"])
    if g.shape != w.shape:
        return "rows: shape %r != %r" % (g.shape, w.shape)
    bad = np.argwhere(g != w)
    if len(bad):
        r = int(bad[0][0])
        return "rows differ at %d places, first row %d: %r != %r" % (len(bad), r, g[r].tolist(), w[r].tolist())
    if classes:
        gc, wc = np.asarray(got["classes"]), np.asarray(want["classes"])
        if gc.shape != wc.shape:
            return "classes: shape %r != %r" % (gc.shape, wc.shape)
        bad = np.argwhere(gc != wc)
        if len(bad):
            i = tuple(bad[0])
            return "classes differ at %d places, first %r: %d != %d" % (len(bad), i, gc[i], wc[i])
    if "best" in got and int(got["best"]) != int(want["best"]):
        return "best: %d != %d" % (got["best"], want["best"])
    if list(got["stats"]) != list(want["stats"]):
        return "stats: %r != %r" % (list(got["stats"]), list(want["stats"]))
    return None
