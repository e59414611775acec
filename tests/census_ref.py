"""An independent count of what the plain scan-match traversal issues (TEST INFRASTRUCTURE, numpy only).

A restatement of the traversal csrc/kd_device.h documents and kd_resume<PLANAR> runs from the root (kd_nearest_ref), on the 32-byte
nodes pfslam_kd_create returns, for queries with z == 0 on a planar map:
  * greedy descent: a visit takes the node when sqrt(s) < sqrt(sBest), s = (dx * dx + dy * dy) in float, one rounding per operation; the
    query goes left exactly when node - query > 0 on the split axis; a z level (axis 2) always branches right;
  * behind a descent: stop when the best node did not change; else one look at the best node's parent -- stop at the root (H1) --,
    |query - parent| on the parent's axis (0 on a z level) against the best distance, and a re-descent of the side the query is NOT on
    (the true left child of a z level).
Counted per query, as the census instantiation counts per lane (KdCensusLocal):
  visits            trips of the descent loop                                                    -> lanes      (out[1])
  tests             looks at the parent, the one that ends at the root (H1) included: the kernel
                    books the test before it loads the parent index                              -> test_lanes (out[3])
  redescents        hyperplane tests that passed -- whether or not the far side holds a node: an
                    empty far side is a re-descent of zero visits                                -> out[6]
  redescents_noop   re-descents behind which the best node is the one it was                     -> out[7]
tests/test_census_ref.py pins the best indices to the CPU oracle's traversal (oracle_lib.traverse_batch) without a GPU;
tests/test_gpu_observers.py holds pfslam_score_census to the sums."""
import ctypes as C

import numpy as np

import oracle_lib as O

LIDAR_RANGE = np.float32(20.0)   # kernel.cu:44
KEYS = ("visits", "tests", "redescents", "redescents_noop")
ROOT_STOPS = "root_stops"   # tests that ended at the root (H1): the CPU oracle's visit count leaves exactly these out


def traverse(tree, qx, qy):
    """Best node and the four per-query counters of every query (qx[i], qy[i], 0)."""
    qx = np.ascontiguousarray(qx, np.float32)
    qy = np.ascontiguousarray(qy, np.float32)
    m = len(qx)
    axis, left, right, parent = (tree[k].astype(np.int64) for k in ("axis", "left", "right", "parent"))
    X, Y = np.ascontiguousarray(tree["x"], np.float32), np.ascontiguousarray(tree["y"], np.float32)
    assert not tree["z"].any(), "the restatement is the PLANAR traversal"
    best = np.zeros(m, np.int64)
    s_best = np.full(m, np.inf, np.float32)
    head = np.zeros(m, np.int64)
    prev = np.full(m, -1, np.int64)
    in_redesc = np.zeros(m, bool)
    alive = np.ones(m, bool)
    cnt = {k: np.zeros(m, np.int64) for k in KEYS + (ROOT_STOPS,)}
    while alive.any():
        while True:  # greedy descent of every query that still stands on a node
            i = np.nonzero(alive & (head >= 0))[0]
            if not len(i):
                break
            nd = head[i]
            cnt["visits"][i] += 1
            dx, dy = X[nd] - qx[i], Y[nd] - qy[i]
            s = dx * dx + dy * dy
            take = np.sqrt(s) < np.sqrt(s_best[i])
            s_best[i] = np.where(take, s, s_best[i])
            best[i] = np.where(take, nd, best[i])
            a = axis[nd]
            lt = (np.where(a == 0, dx, dy) > 0) & (a != 2)
            head[i] = np.where(lt, left[nd], right[nd])
        i = np.nonzero(alive)[0]
        same = best[i] == prev[i]
        cnt["redescents_noop"][i] += in_redesc[i] & same
        alive[i[same]] = False
        i = i[~same]
        cnt["tests"][i] += 1
        prev[i] = best[i]
        pi = parent[best[i]]
        cnt[ROOT_STOPS][i[pi < 0]] += 1
        alive[i[pi < 0]] = False  # H1
        i, pi = i[pi >= 0], pi[pi >= 0]
        a = axis[pi]
        pa, na = np.where(a == 0, qx[i], qy[i]), np.where(a == 0, X[pi], Y[pi])
        hd = np.where(a < 2, np.abs(pa - na), np.float32(0.0)).astype(np.float32)
        lt = (pa < na) & (a < 2)
        go = hd < np.sqrt(s_best[i])
        alive[i[~go]] = False
        i, pi, lt = i[go], pi[go], lt[go]
        head[i] = np.where(lt, right[pi], left[pi])
        in_redesc[i] = True
        cnt["redescents"][i] += 1
    return best.astype(np.int32), cnt


def queries(particles, scan):
    """Beam end points of every in-range (particle, beam) pair, in the map's frame, as EvaluateParticleKD forms them
    (kernel.cu:1198-1298; the CPU oracle's CleanLidarScan, which the product follows bit for bit): (qx, qy, particle, beam)."""
    L = O.lib()
    scan = np.ascontiguousarray(scan, np.float32)
    fx, fy = C.c_float(), C.c_float()
    qx, qy, pi, bj = [], [], [], []
    for i in range(len(particles)):
        x, y, th = (np.float32(particles[k][i]) for k in ("x", "y", "theta"))
        for j in range(len(scan)):
            L.orc_clean_lidar_scan(j, float(scan[j]), float(th), C.byref(fx), C.byref(fy))
            wx, wy = np.float32(fx.value), np.float32(fy.value)
            if abs(wx) < LIDAR_RANGE and abs(wy) < LIDAR_RANGE:
                qx.append(wx + x); qy.append(wy + y); pi.append(i); bj.append(j)
    return np.array(qx, np.float32), np.array(qy, np.float32), np.array(pi, np.int32), np.array(bj, np.int32)


def small_case(pkg):
    """The case both test modules count: a 300-node tree on the lattice, 130 particles (two full waves and a two-lane tail) and 65 beams,
    four of them out of range (1000 m) and one of range zero."""
    pts, _ = pkg.synth.make_map_points(300, seed=7)
    tree = pkg.kd_create(pts[:300])
    ang = np.radians(-135.0 + 0.25 * np.arange(65))
    scan = (8.0 + 5.0 * np.cos(40.0 * ang)).astype(np.float32)   # 3 .. 13 m: the end points sweep a few metres of the map
    assert len(tree) == 300
    scan[[3, 20, 41, 64]] = 1000.0
    scan[11] = 0.0
    # the cloud sits beside the root node, so the beam of range zero ends where the root is the best node (H1)
    p = O.make_particles(130, float(tree["x"][0]) + 0.02, float(tree["y"][0]) - 0.04, 0.2)
    for f in (1, 2, 3):
        O.add_noise(p, frame=f)
    return tree, p, scan


def census(tree, particles, scan):
    """The sums over the in-range (particle, beam) pairs, plus the queries and their best nodes."""
    qx, qy, pi, bj = queries(particles, scan)
    best, cnt = traverse(tree, qx, qy)
    out = {k: int(v.sum()) for k, v in cnt.items()}
    out.update(queries=len(qx), qx=qx, qy=qy, particle=pi, beam=bj, best=best, per_query=cnt)
    return out
