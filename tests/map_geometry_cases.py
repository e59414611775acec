"""Scenario builders shared by tests/test_map_geometry_spec.py (CPU: each scenario still reaches the edge it was built for) and
tests/test_gpu_map_geometry.py (GPU: the product against the oracle on the same scenarios): map sizes that are odd, tiny, no
multiple of a 16-cell chunk or of a 4096-cell block, or large enough for the float wall index to be inexact; single rays in every
octant and at the lengths around the 64-lane and 256-thread strides; robot cells outside the grid; preset grids at the clamps.

Everything here is plain numpy plus the oracle (tests/oracle_lib.py); nothing needs a GPU."""
import ctypes as C
import math

import numpy as np

import oracle_lib as O

# cells per side -> (scale, res); the size is int(float32(scale) / float32(res)) as pfslam_create and the oracle compute it
SIZES = {3: (0.35, 0.1), 67: (6.75, 0.1), 151: (15.15, 0.1), 250: (25.05, 0.1), 1333: (40.0, 0.03), 4800: (48.0, 0.01)}
MASK_LENGTHS = (63, 64, 65, 127, 128, 129)         # around trace_ray_wave's stride of 64 lanes
FIND_LENGTHS = (255, 256, 257, 511, 512, 513)      # around k_find_walls' stride of 256 threads
CLAMP_VALUES = (-113, -112, 112, 113)
LIDAR_RANGE = 20.0


def dim_of(scale, res):
    return int(np.float32(scale) / np.float32(res))


def res_of(dim):
    return SIZES[dim][1]


def patch(dim):
    s, r = SIZES[dim]
    return O.Patch(s, s, r, r)


def handle_kw(dim):
    s, r = SIZES[dim]
    return dict(map_scale=(s, s), map_res=(r, r))


def roundf(v):
    """C's roundf (halves away from zero) of a float32 value, as a Python int."""
    v = float(np.float32(v))
    return int(math.trunc(v + math.copysign(0.5, v)))


def cell_of(dim, x):
    """(int)roundf(0.5f * dim + x / res + res / 2): the cell of world coordinate x (PFUpdateMap's centre, FindWalls' end points)."""
    r = np.float32(res_of(dim))
    return roundf(np.float32(0.5) * np.float32(dim) + np.float32(x) / r + r / np.float32(2))


def coord_of(dim, cell):
    """A world coordinate whose cell is `cell` (cells outside the grid included)."""
    x = np.float32((cell - 0.5 * dim) * res_of(dim))
    assert cell_of(dim, x) == cell, (dim, cell, x)
    return x


def one_beam(dx, dy, res):
    """(theta, scan) of a one-beam scan that ends on cell offset (dx, dy): beam 0 looks along -135 degrees + theta."""
    theta = np.float32(math.atan2(dy, dx) + 0.75 * math.pi)
    return theta, np.array([math.hypot(dx, dy) * res], np.float32)


def beam_offset(theta, rng, res, beam=0):
    """The cell offset the oracle's kernGetWalls gives beam `beam`: roundf(w / res) per axis; None when the beam is out of range."""
    wx, wy = C.c_float(), C.c_float()
    O.lib().orc_clean_lidar_scan(beam, float(rng), float(theta), C.byref(wx), C.byref(wy))
    if not (abs(wx.value) < LIDAR_RANGE and abs(wy.value) < LIDAR_RANGE):
        return None
    r = np.float32(res)
    return roundf(np.float32(wx.value) / r), roundf(np.float32(wy.value) / r)


def masks(dim, scan, cx, cy, theta):
    """The oracle's free and wall masks (flat, x * dim + y) of a scan seen from cell (cx, cy)."""
    return O.get_walls(scan, int(cx), int(cy), np.float32(theta), dim, dim, res_of(dim))


def update_grid(grid, dim, pose, scan):
    """orc_update_map_grid in place on `grid` (dim x dim int8)."""
    pose = np.ascontiguousarray(pose, np.float32)
    scan = np.ascontiguousarray(scan, np.float32)
    p = patch(dim)
    O.lib().orc_update_map_grid(O.P(grid), dim, dim, C.byref(p), O.P(pose), O.P(scan), len(scan))
    return grid


def find_walls(grid, dim, a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    p = patch(dim)
    return O.lib().orc_find_walls(O.P(grid), dim, dim, C.byref(p), O.P(a), O.P(b))


# ---- rays ------------------------------------------------------------------------------------------------------------------------
def short_offsets(half=12):
    """Every offset of [-half, half]^2, the zero-length ray included."""
    return [(dx, dy) for dx in range(-half, half + 1) for dy in range(-half, half + 1)]


def classify(dx, dy):
    """The group of an offset: zero, the four axes, the four diagonals, or octant + shallow / steep (minor below / above half the major)."""
    if dx == 0 and dy == 0:
        return "zero"
    sx, sy = "+" if dx > 0 else "-", "+" if dy > 0 else "-"
    if dy == 0:
        return sx + "x"
    if dx == 0:
        return sy + "y"
    if abs(dx) == abs(dy):
        return "diag" + sx + sy
    major_x = abs(dx) > abs(dy)
    minor, major = (abs(dy), abs(dx)) if major_x else (abs(dx), abs(dy))
    return "oct" + sx + sy + ("x" if major_x else "y") + ("-shallow" if 2 * minor < major else "-steep")


ALL_GROUPS = (["+x", "-x", "+y", "-y"] + ["diag" + a + b for a in "+-" for b in "+-"] +
              ["oct" + a + b + m + s for a in "+-" for b in "+-" for m in "xy" for s in ("-shallow", "-steep")])


def long_offsets(length):
    """24 offsets whose longer side is `length` cells: the axes, the exact diagonals, one shallow and one steep ray per octant."""
    L = length
    out = [(L, 0), (-L, 0), (0, L), (0, -L)] + [(a * L, b * L) for a in (1, -1) for b in (1, -1)]
    for minor in (max(1, L // 9), L - L // 7):
        for a in (1, -1):
            for b in (1, -1):
                out += [(a * L, b * minor), (a * minor, b * L)]
    return out


def clip_cases(dim):
    """(cx, cy, dx, dy): robot cells -40, -1, 0, dim - 1, dim and dim + 40 on each axis (the other in the middle), the same on both
    diagonals of the grid, and from each of them twelve 100-cell rays: the axes, the diagonals, four oblique ones."""
    edge = (-40, -1, 0, dim - 1, dim, dim + 40)
    mid = dim // 2
    centres = [(e, mid) for e in edge] + [(mid, e) for e in edge] + [(e, e) for e in edge] + [(-1, dim), (dim, -1)]
    rays = [(100, 0), (-100, 0), (0, 100), (0, -100), (100, 100), (100, -100), (-100, 100), (-100, -100),
            (100, 37), (-100, -37), (37, -100), (-37, 100)]
    return [(cx, cy, dx, dy) for cx, cy in centres for dx, dy in rays]


def side_of(dim, x, y):
    """Which side of the grid a cell lies beyond ('' = inside; corners name both)."""
    return ("x-" if x < 0 else "x+" if x >= dim else "") + ("y-" if y < 0 else "y+" if y >= dim else "")


# ---- grids -----------------------------------------------------------------------------------------------------------------------
def random_grid(dim, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(-113, 114, (dim, dim)).astype(np.int8)


def clamp_grid(dim, seed, fm, wm):
    """A random grid that holds -113, -112, 112 and 113, in turn, on the cells a ray frees and on the cells a ray hits."""
    grid = random_grid(dim, seed)
    flat = grid.reshape(-1)
    for m in (fm, wm):
        idx = np.flatnonzero(m)
        flat[idx] = np.resize(np.array(CLAMP_VALUES, np.int8), len(idx))
    both = np.flatnonzero(fm.astype(bool) & wm.astype(bool))      # freed by one ray, hit by another: -1, then +4 behind it
    flat[both] = np.resize(np.array(CLAMP_VALUES, np.int8), len(both))
    return grid


def walls_30_31(dim, seed):
    """A grid dense in 30 (not a wall) and 31 (the weakest wall), for FindWalls' `> 30`."""
    rng = np.random.RandomState(seed)
    return rng.choice(np.array([30, 31, 30, 31, -100, 113, 0], np.int8), (dim, dim)).astype(np.int8)


# ---- whole-size scenarios ----------------------------------------------------------------------------------------------------------
def size_scenario(dim, seed=0, nb=1081, corner=False):
    """A pose near the middle of the map, a scan whose rays end inside and outside the grid, and the clamp grid of that scan.  At 4800
    cells the beams within 20 degrees of +x measure 15 to 19 m: their wall cells lie where x * dim + y passes 2^24.
    corner: the robot stands on cell (dim - 1, dim - 3) instead and its rays are 0 to 8 cells long, so that free and wall cells fall
    into the last 16-cell chunk of the masks (the tail, when dim * dim is no multiple of 16) and rays leave through two sides."""
    rng = np.random.RandomState(1000 + dim + seed + (500 if corner else 0))
    res = res_of(dim)
    reach = min(19.9, 0.7 * dim * res)
    scan = rng.uniform(0.0, reach, nb).astype(np.float32)
    theta = np.float32(rng.uniform(-3.0, 3.0))
    if dim == 4800 and not corner:
        theta = np.float32(0.0)
        scan = rng.uniform(0.0, 3.0, nb).astype(np.float32)
        scan[460:621] = rng.uniform(15.0, 19.0, 161).astype(np.float32)
    pose = np.array([rng.uniform(-1.4, 1.4) * res, rng.uniform(-1.4, 1.4) * res, theta], np.float32)
    if corner:
        scan = rng.uniform(0.0, 8.0 * res, nb).astype(np.float32)
        pose[0], pose[1] = coord_of(dim, dim - 1), coord_of(dim, max(dim - 3, 0))
    cx, cy = cell_of(dim, pose[0]), cell_of(dim, pose[1])
    fm, wm = masks(dim, scan, cx, cy, pose[2])
    return {"dim": dim, "pose": pose, "scan": scan, "cx": cx, "cy": cy, "fm": fm, "wm": wm, "grid": clamp_grid(dim, seed + 5, fm, wm)}


def inexact_wall_cells(sc):
    """Per in-range beam of a size scenario whose wall cell is inside the grid: (exact index, the float32 index wx * dim + wy)."""
    dim, res = sc["dim"], res_of(sc["dim"])
    exact, flt = [], []
    for j, r in enumerate(sc["scan"]):
        off = beam_offset(sc["pose"][2], r, res, beam=j)
        if off is None:
            continue
        wx, wy = sc["cx"] + off[0], sc["cy"] + off[1]
        if 0 <= wx < dim and 0 <= wy < dim:
            exact.append(wx * dim + wy)
            flt.append(int(np.float32(wx) * np.float32(dim) + np.float32(wy)))
    return np.array(exact, np.int64), np.array(flt, np.int64)


def score_scenario(dim, n, seed=0, nb=1081):
    """Particles on cells -1, 0, dim - 1 and dim of either axis (the other axis anywhere inside; every ninth particle anywhere) with
    scans of 0 to 3 cells, so that the end points of one particle fall on both sides of its edge; a random grid."""
    rng = np.random.RandomState(2000 + dim + seed)
    s, res = SIZES[dim]
    half = 0.5 * s / res                                           # EvaluateParticle's origin: 0.5f * scale / res, no integer
    p = O.make_particles(n)
    edge = (-1, 0, dim - 1, dim)
    for i in range(n):
        c = [rng.uniform(0, dim - 1), rng.uniform(0, dim - 1)]
        if i % 9 != 8:
            c[(i // 4) % 2] = edge[i % 4]
        p["x"][i], p["y"][i] = (c[0] - half) * res, (c[1] - half) * res
    p["theta"] = rng.uniform(-3.0, 3.0, n)
    scan = rng.uniform(0.0, 3.0 * res, nb).astype(np.float32)
    return {"dim": dim, "particles": p, "scan": scan, "grid": random_grid(dim, seed + 9)}


def score_cells(sc):
    """End-point cells (n x nb x 2) of a score scenario in double precision: good enough to say on which side of an edge they fall."""
    dim = sc["dim"]
    s, res = SIZES[dim]
    p, scan = sc["particles"], sc["scan"].astype(np.float64)
    ang = np.radians(-135.0 + 0.25 * np.arange(len(scan)))[None, :] + p["theta"].astype(np.float64)[:, None]
    wx = scan[None, :] * np.cos(ang) + p["x"].astype(np.float64)[:, None]
    wy = scan[None, :] * np.sin(ang) + p["y"].astype(np.float64)[:, None]
    return np.stack([np.floor(0.5 * s / res + wx / res + 0.5), np.floor(0.5 * s / res + wy / res + 0.5)], axis=2).astype(np.int64)


def score_grid(sc):
    p, scan, dim = sc["particles"], sc["scan"], sc["dim"]
    want = np.zeros(len(p), np.int32)
    pa = patch(dim)
    O.lib().orc_score_grid(O.P(sc["grid"]), dim, dim, C.byref(pa), O.P(p), len(p), O.P(scan), len(scan), O.P(want))
    return want


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def room(dim, nb, f):
    """A closed, three-lobed room around the robot, scaled with the map: 0.11 to 0.19 of its side away."""
    ang = np.radians(-135.0 + 0.25 * np.arange(nb))
    r = 6.0 + 1.5 * np.cos(3.0 * ang + 0.05 * f) + np.random.RandomState(40 + f).uniform(-0.01, 0.01, nb)
    return (r * (SIZES[dim][0] / 40.0)).astype(np.float32)


def frame_scans(dim, nb=1081, frames=4):
    return [room(dim, nb, f) for f in range(frames)]
