"""ctypes binding of include/pfslam.h (libpfslam_hip.so).  No fallback of any kind."""
import ctypes as C
import os

import numpy as np

from . import build as _build

NODE_DTYPE = np.dtype(
    [("axis", "<i4"), ("left", "<i4"), ("right", "<i4"), ("parent", "<i4"),
     ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("w", "<f4")])
PARTICLE_DTYPE = np.dtype(
    {"names": ["x", "y", "theta", "w", "cluster", "map"],
     "formats": ["<f4", "<f4", "<f4", "<f4", "u1", "<u8"],
     "offsets": [0, 4, 8, 12, 16, 24], "itemsize": 32})

# every symbol include/pfslam.h declares (checked by tests/test_cabi_symbols.py)
SYMBOLS = [
    "pfslam_default_config", "pfslam_create", "pfslam_destroy", "pfslam_last_error", "pfslam_device_count",
    "pfslam_set_stream", "pfslam_synchronize", "pfslam_step", "pfslam_step_grid", "pfslam_shard_disperse", "pfslam_shard_score", "pfslam_shard_weights", "pfslam_shard_finish", "pfslam_shard_stream", "pfslam_get_pose", "pfslam_get_particles",
    "pfslam_get_map", "pfslam_get_grid", "pfslam_get_trace", "pfslam_get_cells", "pfslam_set_map",
    "pfslam_set_particles", "pfslam_shift_particles", "pfslam_set_scan", "pfslam_set_pose", "pfslam_set_grid", "pfslam_motion_update",
    "pfslam_score_kd", "pfslam_measurement_update", "pfslam_icp", "pfslam_update_map_kd", "pfslam_resample",
    "pfslam_score_grid", "pfslam_update_map_grid", "pfslam_traverse", "pfslam_measurement_local",
    "pfslam_measurement_apply", "pfslam_device_ptr", "pfslam_time_score_kd", "pfslam_set_variant", "pfslam_set_lag",
    "pfslam_kd_create", "pfslam_kd_insert_list", "pfslam_kd_insert_node", "pfslam_kd_balance", "pfslam_set_timing", "pfslam_get_timers", "pfslam_resample_plan", "pfslam_resample_gather", "pfslam_maybe_balance", "pfslam_kd_size", "pfslam_topology_update", "pfslam_find_walls",
    "pfslam_check_loop_closure", "pfslam_get_topology", "pfslam_set_topology", "pfslam_get_closures", "pfslam_score_census", "pfslam_set_census", "pfslam_get_census_log", "pfslam_ubench_gather", "pfslam_plan_stats", "pfslam_cell_stats", "pfslam_kd_parallel_sort", "pfslam_kd_sort_threads", "pfslam_kd_whole_node",
    "pfslam_set_serial", "pfslam_set_trig", "pfslam_set_resampler", "pfslam_estimate", "pfslam_debug_check_cells", "pfslam_set_probe", "pfslam_get_probe", "pfslam_probe_name", "pfslam_frame_mode",
    "pfslam_nearest", "pfslam_register", "pfslam_register_default_opts", "pfslam_register_batch", "pfslam_search", "pfslam_search_default_opts", "pfslam_search_scan", "pfslam_search_wide",
    "pfslam_search_cov", "pfslam_search_scan_cov", "pfslam_search_cov_default_opts", "pfslam_search_best", "pfslam_search_best_default_opts",
    "pfslam_cast", "pfslam_cast_default_opts", "pfslam_map_raster", "pfslam_cast_score", "pfslam_cast_score_default_opts",
    "pfslam_move_particles", "pfslam_move_default_opts",
    "pfslam_time_score_grid", "pfslam_set_shard_balance", "pfslam_shard_balance_due", "pfslam_shard_balance_build", "pfslam_shard_balance_adopt",
]


class Config(C.Structure):
    _fields_ = [("n_particles", C.c_int32), ("n_beams", C.c_int32),
                ("map_scale_x", C.c_float), ("map_scale_y", C.c_float),
                ("map_res_x", C.c_float), ("map_res_y", C.c_float),
                ("kd_capacity", C.c_int32), ("device", C.c_int32),
                ("strict_host_mirror", C.c_int32), ("free_upload_bug", C.c_int32),
                ("balance_period", C.c_int32), ("global_offset", C.c_int32), ("global_n", C.c_int32),
                ("shard_stride", C.c_int32), ("reserved_", C.c_int32 * 2)]


class RegisterOpts(C.Structure):
    """pfslam_register_opts (include/pfslam.h)."""
    _fields_ = [("max_iters", C.c_int32), ("match", C.c_int32), ("select", C.c_int32), ("update", C.c_int32),
                ("max_dist", C.c_float), ("eps_xy", C.c_float), ("eps_theta", C.c_float), ("min_pairs", C.c_int32)]


class SearchOpts(C.Structure):
    """pfslam_search_opts (include/pfslam.h)."""
    _fields_ = [("half_x", C.c_int32), ("half_y", C.c_int32), ("half_theta", C.c_int32), ("stride", C.c_int32),
                ("step_theta", C.c_float), ("max_dist", C.c_float), ("reserved_", C.c_int32 * 2)]


class CovOpts(C.Structure):
    """pfslam_cov_opts (include/pfslam.h)."""
    _fields_ = [("sigma", C.c_float), ("reserved_", C.c_int32 * 3)]


class BestOpts(C.Structure):
    """pfslam_best_opts (include/pfslam.h)."""
    _fields_ = [("count", C.c_int32), ("tile_log2", C.c_int32), ("group_theta", C.c_int32), ("reserved_", C.c_int32)]


class CastOpts(C.Structure):
    """pfslam_cast_opts (include/pfslam.h)."""
    _fields_ = [("max_range", C.c_float), ("w_min", C.c_float), ("no_hit", C.c_float), ("inflate", C.c_int32), ("skip_cells", C.c_int32),
                ("reserved_", C.c_int32 * 3)]


class CastScoreOpts(C.Structure):
    """pfslam_cast_score_opts (include/pfslam.h)."""
    _fields_ = [("tol", C.c_float), ("clip", C.c_float), ("z_min", C.c_float), ("z_max", C.c_float), ("count_miss", C.c_int32), ("source", C.c_int32),
                ("reserved_", C.c_int32 * 2)]


class MoveOpts(C.Structure):
    """pfslam_move_opts (include/pfslam.h)."""
    _fields_ = [("ref_theta", C.c_float), ("cov_scale", C.c_float), ("sigma_xy_min", C.c_float), ("sigma_theta_min", C.c_float),
                ("reserved_", C.c_int32 * 4)]


CAST_SCORE_COLUMNS = ("valid", "agree", "through", "short", "miss", "q1", "q2", "cost")
REGISTER_STATUS = {0: "max_iters", 1: "converged", 2: "too_few_pairs", 3: "not_finite"}


class PfSlamError(RuntimeError):
    pass


_lib = None


def _one_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.  If this library initialises /opt/rocm's copy first,
    a later `import torch` in the same process sees "No HIP GPUs" (two runtimes).  When torch is installed but not
    yet imported, pre-load ITS runtime globally so that both bind to one copy.  No torch -> nothing to do."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("PFSLAM_NO_TORCH_HIP"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Build (if stale) and load libpfslam_hip.so.  Raises if that is not possible."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("PFSLAM_LIB") or _build.LIB  # (PFSLAM_LIB: an A/B build of the same sources, tools/experiments)
    try:
        if path == _build.LIB and _build.stale():
            _build.build()
    except Exception as e:  # a prebuilt .so that travelled with the snapshot is still usable
        if not os.path.exists(path):
            raise PfSlamError("libpfslam_hip.so is missing and could not be built: %s" % e)
    _one_hip_runtime()
    L = C.CDLL(path)
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.pfslam_last_error.restype = C.c_char_p
    L.pfslam_default_config.restype = None
    L.pfslam_default_config.argtypes = [vp]
    L.pfslam_create.argtypes = [vp, vp]
    L.pfslam_destroy.argtypes = [vp]
    L.pfslam_set_stream.argtypes = [vp, vp]
    L.pfslam_synchronize.argtypes = [vp]
    L.pfslam_step.argtypes = [vp, i32, vp]
    L.pfslam_step_grid.argtypes = [vp, i32, vp]
    L.pfslam_shard_disperse.argtypes = [vp, i32, vp, vp]
    L.pfslam_shard_score.argtypes = [vp]
    L.pfslam_shard_weights.argtypes = [vp]
    L.pfslam_shard_finish.argtypes = [vp]
    L.pfslam_shard_stream.argtypes = [vp, i32, vp]
    L.pfslam_time_score_grid.argtypes = [vp, i32, vp, vp]
    L.pfslam_set_shard_balance.argtypes = [vp, i32]
    L.pfslam_shard_balance_due.argtypes = [vp, i32, vp, vp]
    L.pfslam_shard_balance_build.argtypes = [vp, i32]
    L.pfslam_shard_balance_adopt.argtypes = [vp]
    L.pfslam_get_pose.argtypes = [vp, vp]
    L.pfslam_get_particles.argtypes = [vp, vp, vp]
    L.pfslam_get_map.argtypes = [vp, vp, vp]
    L.pfslam_get_grid.argtypes = [vp, vp, vp, vp]
    L.pfslam_get_trace.argtypes = [vp, vp]
    L.pfslam_get_cells.argtypes = [vp, i32, vp, i32, vp]
    L.pfslam_set_map.argtypes = [vp, vp, i32]
    L.pfslam_set_particles.argtypes = [vp, vp, i32]
    L.pfslam_set_scan.argtypes = [vp, vp, i32]
    L.pfslam_shift_particles.argtypes = [vp, vp]
    L.pfslam_set_pose.argtypes = [vp, vp]
    L.pfslam_set_grid.argtypes = [vp, vp, i32, i32]
    L.pfslam_motion_update.argtypes = [vp, i32]
    L.pfslam_score_kd.argtypes = [vp, vp]
    L.pfslam_measurement_update.argtypes = [vp, vp, vp, vp]
    L.pfslam_icp.argtypes = [vp, vp, vp, vp]
    L.pfslam_update_map_kd.argtypes = [vp]
    L.pfslam_resample.argtypes = [vp, i32, vp, vp]
    L.pfslam_resample_plan.argtypes = [vp, i32, vp, vp]
    L.pfslam_resample_gather.argtypes = [vp]
    L.pfslam_maybe_balance.argtypes = [vp, i32]
    L.pfslam_kd_size.argtypes = [vp]
    L.pfslam_topology_update.argtypes = [vp, vp]
    L.pfslam_find_walls.argtypes = [vp, vp, vp, vp]
    L.pfslam_check_loop_closure.argtypes = [vp, vp, i32, vp]
    L.pfslam_get_topology.argtypes = [vp, vp, i32, vp, vp]
    L.pfslam_set_topology.argtypes = [vp, i32]
    L.pfslam_get_closures.argtypes = [vp, vp, i32, vp]
    L.pfslam_score_census.argtypes = [vp, vp]
    L.pfslam_set_census.argtypes = [vp, i32]
    L.pfslam_get_census_log.argtypes = [vp, vp, i32, vp]
    L.pfslam_ubench_gather.argtypes = [vp, vp]
    L.pfslam_plan_stats.argtypes = [vp, vp]
    L.pfslam_cell_stats.argtypes = [vp, vp]
    L.pfslam_set_serial.argtypes = [vp, i32]
    L.pfslam_set_trig.argtypes = [vp, i32]
    L.pfslam_set_resampler.argtypes = [vp, i32]
    L.pfslam_estimate.argtypes = [vp, vp]
    L.pfslam_register_default_opts.restype = None
    L.pfslam_register_default_opts.argtypes = [vp]
    L.pfslam_nearest.argtypes = [vp, vp, i32, vp, vp]
    L.pfslam_register.argtypes = [vp, vp, vp, vp, vp, vp]
    L.pfslam_register_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.pfslam_search_default_opts.restype = None
    L.pfslam_search_default_opts.argtypes = [vp]
    L.pfslam_search.argtypes = [vp, vp, vp, vp, vp, vp]
    L.pfslam_search_scan.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pfslam_search_cov_default_opts.restype = None
    L.pfslam_search_cov_default_opts.argtypes = [vp]
    L.pfslam_search_cov.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.pfslam_search_scan_cov.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pfslam_search_wide.argtypes = [vp, vp, vp, vp, vp, vp]
    L.pfslam_search_best_default_opts.restype = None
    L.pfslam_search_best_default_opts.argtypes = [vp]
    L.pfslam_search_best.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pfslam_cast_default_opts.restype = None
    L.pfslam_cast_default_opts.argtypes = [vp]
    L.pfslam_cast.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.pfslam_map_raster.argtypes = [vp, vp, vp, vp, C.c_size_t]
    L.pfslam_cast_score_default_opts.restype = None
    L.pfslam_cast_score_default_opts.argtypes = [vp]
    L.pfslam_cast_score.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.pfslam_move_default_opts.restype = None
    L.pfslam_move_default_opts.argtypes = [vp]
    L.pfslam_move_particles.argtypes = [vp, i32, vp, vp, vp]
    L.pfslam_debug_check_cells.argtypes = [vp, vp]
    L.pfslam_set_probe.argtypes = [vp, i32]
    L.pfslam_get_probe.argtypes = [vp, vp, i32, vp, vp]
    L.pfslam_frame_mode.argtypes = [vp, vp]
    L.pfslam_probe_name.argtypes = [i32]
    L.pfslam_probe_name.restype = C.c_char_p
    L.pfslam_score_grid.argtypes = [vp, vp]
    L.pfslam_update_map_grid.argtypes = [vp]
    L.pfslam_traverse.argtypes = [vp, vp, i32, vp]
    L.pfslam_measurement_local.argtypes = [vp]
    L.pfslam_measurement_apply.argtypes = [vp, vp, vp, vp]
    L.pfslam_device_ptr.argtypes = [vp, i32, vp, vp]
    L.pfslam_time_score_kd.argtypes = [vp, i32, vp]
    L.pfslam_set_variant.argtypes = [vp, i32]
    L.pfslam_set_lag.argtypes = [vp, i32]
    L.pfslam_kd_create.argtypes = [vp, i32, vp]
    L.pfslam_kd_insert_node.argtypes = [vp, vp, i32]
    L.pfslam_kd_insert_list.argtypes = [vp, i32, vp, i32, i32]
    L.pfslam_kd_balance.argtypes = [vp, i32]
    L.pfslam_debug_math.argtypes = [vp, i32, vp, i32, vp]
    L.pfslam_debug_search_frontier.argtypes = [vp, i32]
    L.pfslam_set_timing.argtypes = [vp, i32]
    L.pfslam_get_timers.argtypes = [vp, vp]
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _chk(rc, what=""):
    if rc != 0:
        raise PfSlamError("%s failed: %s" % (what, load().pfslam_last_error().decode()))


def device_count():
    return load().pfslam_device_count()


def estimate_dict(out16):
    """pfslam_estimate's 16 floats -> mean (3), cov (3 x 3, symmetric), neff, sum_w, sum_w2, n."""
    o = np.asarray(out16, np.float32)
    xx, xy, xt, yy, yt, tt = o[3:9]
    return {"mean": o[0:3].copy(), "cov": np.array([[xx, xy, xt], [xy, yy, yt], [xt, yt, tt]], np.float32),
            "neff": float(o[9]), "sum_w": float(o[10]), "sum_w2": float(o[11]), "n": int(o[12])}


# ---- host-side map structure (no GPU needed) -------------------------------------------------
def kd_create(points_xyzw):
    pts = np.ascontiguousarray(points_xyzw, dtype=np.float32).reshape(-1, 4)
    out = np.zeros(len(pts), dtype=NODE_DTYPE)
    _chk(load().pfslam_kd_create(_p(pts), len(pts), _p(out)), "pfslam_kd_create")
    return out


def kd_insert_node(nodes, size, p4):
    p = np.ascontiguousarray(p4, dtype=np.float32)
    _chk(load().pfslam_kd_insert_node(_p(p), _p(nodes), size), "pfslam_kd_insert_node")


def kd_balance(nodes, size):
    _chk(load().pfslam_kd_balance(_p(nodes), size), "pfslam_kd_balance")


# ---- libpfslam_mgpu.so: the sharded frame with its all-gathers on librccl, launched into the frame's own streams (include/pfslam_mgpu.h)
MGPU_SYMBOLS = ["pfslam_mgpu_make_id", "pfslam_mgpu_create", "pfslam_mgpu_destroy", "pfslam_mgpu_step", "pfslam_mgpu_barrier_max",
                "pfslam_mgpu_stats", "pfslam_mgpu_time_collectives", "pfslam_mgpu_last_error"]
MGPU_ID_BYTES = 256
_mgpu = None


def load_mgpu():
    """ctypes handle of host/libpfslam_mgpu.so (built by `make -C gpu-icp-slam_amd/host`, which __graft_entry__.build() runs)."""
    global _mgpu
    if _mgpu is not None:
        return _mgpu
    load()  # (libpfslam_hip.so first: the multi-GPU library links it)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "libpfslam_mgpu.so")
    if not os.path.exists(path):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.dirname(path), "libpfslam_mgpu.so"], stdout=subprocess.DEVNULL)
    M = C.CDLL(path, mode=C.RTLD_GLOBAL)
    vp, i32 = C.c_void_p, C.c_int32
    M.pfslam_mgpu_last_error.restype = C.c_char_p
    M.pfslam_mgpu_make_id.argtypes = [vp]
    M.pfslam_mgpu_create.argtypes = [vp, i32, i32, vp, vp]
    M.pfslam_mgpu_destroy.argtypes = [vp]
    M.pfslam_mgpu_step.argtypes = [vp, i32, vp]
    M.pfslam_mgpu_barrier_max.argtypes = [vp, vp]
    M.pfslam_mgpu_stats.argtypes = [vp, vp]
    M.pfslam_mgpu_time_collectives.argtypes = [vp, i32, vp]
    _mgpu = M
    return M


def mgpu_make_id():
    """The job id rank 0 makes (two ncclUniqueId); the caller carries the bytes to the other ranks."""
    M = load_mgpu()
    buf = (C.c_ubyte * MGPU_ID_BYTES)()
    if M.pfslam_mgpu_make_id(buf):
        raise PfSlamError("pfslam_mgpu_make_id failed: %s" % M.pfslam_mgpu_last_error().decode())
    return bytes(buf)


class MgpuRank:
    """One rank of a sharded job stepped natively: pfslam_mgpu_step = the four pfslam_shard_* calls with the three RCCL all-gathers
    launched straight into the frame's own streams."""

    def __init__(self, eng, world, rank, job_id=None):
        self.M, self.eng = load_mgpu(), eng
        self._m = C.c_void_p(0)
        idbuf = (C.c_ubyte * MGPU_ID_BYTES).from_buffer_copy(job_id) if job_id is not None else None
        self._chk(self.M.pfslam_mgpu_create(idbuf, world, rank, eng._h, C.byref(self._m)), "pfslam_mgpu_create")

    def _chk(self, rc, what):
        if rc != 0:
            raise PfSlamError("%s failed: %s" % (what, self.M.pfslam_mgpu_last_error().decode()))

    def step(self, frame, scan):
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        self._chk(self.M.pfslam_mgpu_step(self._m, frame, _p(scan)), "pfslam_mgpu_step")

    def barrier_max(self, value=None):
        v = C.c_double(0.0 if value is None else value)
        self._chk(self.M.pfslam_mgpu_barrier_max(self._m, C.byref(v) if value is not None else None), "pfslam_mgpu_barrier_max")
        return v.value

    def stats(self):
        out = (C.c_int * 4)()
        self._chk(self.M.pfslam_mgpu_stats(self._m, out), "pfslam_mgpu_stats")
        return {"collectives": out[0], "balance_builds": out[1], "balance_broadcasts": out[2], "world": out[3]}

    def time_collectives(self, reps=20):
        ms = (C.c_float * 3)()
        self._chk(self.M.pfslam_mgpu_time_collectives(self._m, reps, ms), "pfslam_mgpu_time_collectives")
        return {"pose_blocks": ms[0], "records": ms[1], "weights": ms[2]}

    def close(self):
        if self._m:
            self.M.pfslam_mgpu_destroy(self._m)
            self._m = C.c_void_p(0)


class PfSlam:
    """One handle = one GPU's shard of particles + a replica of the map."""

    def __init__(self, n_particles, n_beams=1081, kd_capacity=1 << 20, device=0, strict_host_mirror=1,
                 free_upload_bug=0, balance_period=100, global_offset=0, global_n=0, shard_stride=0, map_scale=None, map_res=None):
        L = load()
        cfg = Config()
        L.pfslam_default_config(C.byref(cfg))
        cfg.n_particles, cfg.n_beams, cfg.kd_capacity, cfg.device = n_particles, n_beams, kd_capacity, device
        if map_scale is not None:   # (x, y) extent of the map in metres (default 40 x 40, data/map_settings.txt)
            cfg.map_scale_x, cfg.map_scale_y = map_scale
        if map_res is not None:     # (x, y) cell size in metres (default 0.025)
            cfg.map_res_x, cfg.map_res_y = map_res
        cfg.strict_host_mirror, cfg.free_upload_bug, cfg.balance_period = strict_host_mirror, free_upload_bug, balance_period
        cfg.global_offset, cfg.global_n, cfg.shard_stride = global_offset, global_n, shard_stride
        self.cfg = cfg
        self.n, self.nb = n_particles, n_beams
        self._h = C.c_void_p()
        _chk(L.pfslam_create(C.byref(cfg), C.byref(self._h)), "pfslam_create")
        self.L = L

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.L.pfslam_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- uploads
    def set_map(self, nodes):
        nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
        _chk(self.L.pfslam_set_map(self._h, _p(nodes), len(nodes)), "pfslam_set_map")

    def set_particles(self, particles):
        particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
        _chk(self.L.pfslam_set_particles(self._h, _p(particles), len(particles)), "pfslam_set_particles")

    def set_scan(self, scan):
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        _chk(self.L.pfslam_set_scan(self._h, _p(scan), len(scan)), "pfslam_set_scan")

    def set_pose(self, pose):
        pose = np.ascontiguousarray(pose, dtype=np.float32)
        _chk(self.L.pfslam_set_pose(self._h, _p(pose)), "pfslam_set_pose")

    def set_grid(self, grid):
        grid = np.ascontiguousarray(grid, dtype=np.int8)
        _chk(self.L.pfslam_set_grid(self._h, _p(grid), grid.shape[0], grid.shape[1]), "pfslam_set_grid")

    def set_stream(self, stream_ptr):
        _chk(self.L.pfslam_set_stream(self._h, C.c_void_p(stream_ptr)), "pfslam_set_stream")

    def set_variant(self, v):
        _chk(self.L.pfslam_set_variant(self._h, v), "pfslam_set_variant")

    def set_timing(self, enable):
        _chk(self.L.pfslam_set_timing(self._h, int(enable)), "pfslam_set_timing")

    def timers(self):
        out = (C.c_double * 12)()
        _chk(self.L.pfslam_get_timers(self._h, out), "pfslam_get_timers")
        d = {"score_ms": out[0], "score_launches": int(out[1])}
        for k, name in enumerate(("motion", "measurement", "map", "resample", "plan"), start=1):
            d[name + "_ms"] = out[2 * k]
            d[name + "_count"] = int(out[2 * k + 1])
        return d

    def set_lag(self, frames):
        """Frames pfslam_step may leave in flight (0 = every step books its own frame before it returns; default 1)."""
        _chk(self.L.pfslam_set_lag(self._h, frames), "pfslam_set_lag")

    def synchronize(self):
        _chk(self.L.pfslam_synchronize(self._h), "pfslam_synchronize")

    # -- stages
    def shift_particles(self, delta):
        """Odometry hook: every particle and robotPos += (dx, dy, dtheta)."""
        d = np.ascontiguousarray(delta, dtype=np.float32)
        _chk(self.L.pfslam_shift_particles(self._h, _p(d)), "pfslam_shift_particles")

    def move_particles(self, frame, delta, cov=None, ref_theta=0.0, cov_scale=1.0, sigma_xy_min=0.0, sigma_theta_min=0.0):
        """The odometry motion model (include/pfslam.h, pfslam_move_particles): every particle moves by `delta` = (dx, dy, dtheta), given
        in the frame of heading `ref_theta`, rotated into its own frame, plus Gaussian noise of covariance cov_scale * cov + the floors,
        drawn per (frame, global particle index).  cov: None (zero), the six entries xx, xy, xtheta, yy, ytheta, thetatheta (raw[3:9] of
        search_cov() / search_scan_cov()) or their symmetric 3 x 3 matrix (the dict's "cov").  Enqueued behind the frames in flight."""
        d = np.ascontiguousarray(delta, dtype=np.float32).reshape(-1)
        if d.shape != (3,):
            raise ValueError("move_particles(): delta must be (dx, dy, dtheta), got %d values" % d.size)
        c = None
        if cov is not None:
            c = np.ascontiguousarray(cov, dtype=np.float32)
            if c.shape == (3, 3):
                c = np.ascontiguousarray(c[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]])
            c = c.reshape(-1)
            if c.shape != (6,):
                raise ValueError("move_particles(): cov must hold 6 entries or be 3 x 3, got %d values" % c.size)
        o = MoveOpts()
        self.L.pfslam_move_default_opts(C.byref(o))
        o.ref_theta, o.cov_scale, o.sigma_xy_min, o.sigma_theta_min = ref_theta, cov_scale, sigma_xy_min, sigma_theta_min
        _chk(self.L.pfslam_move_particles(self._h, frame, _p(d), None if c is None else _p(c), C.byref(o)), "pfslam_move_particles")

    def motion_update(self, frame):
        _chk(self.L.pfslam_motion_update(self._h, frame), "pfslam_motion_update")

    def score_kd(self, fetch=True):
        if not fetch:
            _chk(self.L.pfslam_score_kd(self._h, None), "pfslam_score_kd")
            return None
        fit = np.empty(self.n, np.float32)
        _chk(self.L.pfslam_score_kd(self._h, _p(fit)), "pfslam_score_kd")
        return fit

    def time_score_grid(self, iters):
        a, b = C.c_float(), C.c_float()
        _chk(self.L.pfslam_time_score_grid(self._h, iters, C.byref(a), C.byref(b)), "pfslam_time_score_grid")
        return a.value, b.value

    def time_score_kd(self, iters):
        ms = C.c_float()
        _chk(self.L.pfslam_time_score_kd(self._h, iters, C.byref(ms)), "pfslam_time_score_kd")
        return ms.value

    def measurement_update(self):
        best, fmin, fmax = C.c_int(), C.c_float(), C.c_float()
        _chk(self.L.pfslam_measurement_update(self._h, C.byref(best), C.byref(fmin), C.byref(fmax)),
             "pfslam_measurement_update")
        return best.value, fmin.value, fmax.value

    def measurement_local(self):
        _chk(self.L.pfslam_measurement_local(self._h), "pfslam_measurement_local")

    def measurement_apply(self, fetch=True):
        if not fetch:  # no read-back, no host synchronisation
            _chk(self.L.pfslam_measurement_apply(self._h, None, None, None), "pfslam_measurement_apply")
            return None
        best, fmin, fmax = C.c_int(), C.c_float(), C.c_float()
        _chk(self.L.pfslam_measurement_apply(self._h, C.byref(best), C.byref(fmin), C.byref(fmax)),
             "pfslam_measurement_apply")
        return best.value, fmin.value, fmax.value

    def icp(self, start=None, fetch=True):
        """start=None: use the device-resident best-particle pose left by measurement_apply.
        fetch=False: launch only (no read-back, no host synchronisation)."""
        if not fetch:
            _chk(self.L.pfslam_icp(self._h, None, None, None), "pfslam_icp")
            return None
        out = np.zeros(3, np.float32)
        dbg = np.zeros(32, np.float32)
        if start is None:
            _chk(self.L.pfslam_icp(self._h, None, _p(out), _p(dbg)), "pfslam_icp")
        else:
            start = np.ascontiguousarray(start, dtype=np.float32)
            _chk(self.L.pfslam_icp(self._h, _p(start), _p(out), _p(dbg)), "pfslam_icp")
        return out, dbg

    def update_map_kd(self):
        _chk(self.L.pfslam_update_map_kd(self._h), "pfslam_update_map_kd")

    def resample(self, frame):
        did, neff = C.c_int(), C.c_float()
        _chk(self.L.pfslam_resample(self._h, frame, C.byref(did), C.byref(neff)), "pfslam_resample")
        return did.value, neff.value

    def maybe_balance(self, frame):
        _chk(self.L.pfslam_maybe_balance(self._h, frame), "pfslam_maybe_balance")

    @property
    def kd_size(self):
        return self.L.pfslam_kd_size(self._h)

    # -- topology graph / loop-closure proposal (kernel.cu:623-795)
    def topology_update(self):
        n = C.c_int()
        _chk(self.L.pfslam_topology_update(self._h, C.byref(n)), "pfslam_topology_update")
        return n.value

    def find_walls(self, a_xy, b_xy):
        a = np.ascontiguousarray(a_xy, np.float32); b = np.ascontiguousarray(b_xy, np.float32)
        n = C.c_int()
        _chk(self.L.pfslam_find_walls(self._h, _p(a), _p(b), C.byref(n)), "pfslam_find_walls")
        return n.value

    def check_loop_closure(self, cap=4096):
        pairs = np.zeros((cap, 2), np.int32)
        n = C.c_int()
        _chk(self.L.pfslam_check_loop_closure(self._h, _p(pairs), cap, C.byref(n)), "pfslam_check_loop_closure")
        return pairs[:min(n.value, cap)].copy()

    def set_topology(self, enable=True):
        """UpdateTopology + CheckLoopClosure at the end of every step() / step_grid() (kernel.cu:1750-1751)."""
        _chk(self.L.pfslam_set_topology(self._h, int(enable)), "pfslam_set_topology")

    def closures(self, cap=65536):
        pairs = np.zeros((cap, 2), np.int32)
        n = C.c_int()
        _chk(self.L.pfslam_get_closures(self._h, _p(pairs), cap, C.byref(n)), "pfslam_get_closures")
        return pairs[:min(n.value, cap)].copy()

    def topology(self, cap=4096):
        nodes = np.zeros((cap, 3), np.float32)
        n, idx = C.c_int(), C.c_int()
        _chk(self.L.pfslam_get_topology(self._h, _p(nodes), cap, C.byref(n), C.byref(idx)), "pfslam_get_topology")
        return nodes[:n.value].copy(), idx.value

    def score_census(self):
        """One counting launch of the score kernel on the current state (see include/pfslam.h)."""
        out = (C.c_ulonglong * 8)()
        _chk(self.L.pfslam_score_census(self._h, out), "pfslam_score_census")
        return {"trips": int(out[0]), "visits": int(out[1]), "tests": int(out[2]), "test_lanes": int(out[3]),
                "uniform_trips": int(out[4]), "prefix_trips": int(out[5]), "redescents": int(out[6]), "redescents_noop": int(out[7])}

    def set_census(self, enable=True):
        """Log what every scoring pass issues (counting instantiation on the same inputs, see include/pfslam.h)."""
        _chk(self.L.pfslam_set_census(self._h, int(enable)), "pfslam_set_census")

    def census_log(self, cap=1024):
        out = np.zeros((cap, 8), np.uint64)
        n = C.c_int()
        _chk(self.L.pfslam_get_census_log(self._h, _p(out), cap, C.byref(n)), "pfslam_get_census_log")
        keys = ("trips", "visits", "tests", "test_lanes", "uniform_trips", "prefix_trips", "redescents", "redescents_noop")
        return [dict(zip(keys, (int(v) for v in row))) for row in out[:min(n.value, cap)]]

    def plan_stats(self):
        out = (C.c_double * 10)()
        _chk(self.L.pfslam_plan_stats(self._h, out), "pfslam_plan_stats")
        keys = ("rows", "path_len", "candidates", "frac_complete", "frac_no_plan", "frac_full", "box_dx", "box_dy", "box_dtheta", "waves")
        return dict(zip(keys, [float(v) for v in out]))

    def cell_stats(self):
        """The persistent lattice-cell rows (all zero when the last scoring pass did not use them)."""
        out = (C.c_double * 16)()
        _chk(self.L.pfslam_cell_stats(self._h, out), "pfslam_cell_stats")
        keys = ("cells", "rows", "candidates", "redescent_candidates", "cells_without_row", "pool_slots", "window_kx", "window_ky",
                "walked_from_root", "extended", "reused", "claimed", "flags", "updates", "wipes", "suspended")
        return dict(zip(keys, [float(v) for v in out]))

    def set_serial(self, on):
        _chk(self.L.pfslam_set_serial(self._h, int(on)), "pfslam_set_serial")

    def check_cells(self):
        """Invariants of the persistent cell rows, checked on the device (include/pfslam.h): counts + violations (must be zero)."""
        out = (C.c_longlong * 16)()
        _chk(self.L.pfslam_debug_check_cells(self._h, out), "pfslam_debug_check_cells")
        keys = ("records", "unwalked", "fresh", "published", "row_words", "pending_words", "fallback_words", "dead",
                "v_unwalked_not_pending", "v_unpublished_word", "v_row_outside_alloc", "v_row_not_candidate", "v_watched_link_has_child",
                "v_bad_link", "v_dead_has_row", "v_counters")
        d = dict(zip(keys, [int(v) for v in out]))
        d["violations"] = sum(v for k, v in d.items() if k.startswith("v_"))
        return d

    def set_trig(self, devlib):
        """1: the device library's cosf / sinf / erfcinvf instead of the pf_math.h specification (include/pfslam.h, pfslam_set_trig)."""
        _chk(self.L.pfslam_set_trig(self._h, 1 if devlib else 0), "pfslam_set_trig")

    def set_resampler(self, mode):
        """Where a resample's thread i takes its draw from: 0 the reference's seeding (512 distinct draws whatever N is, H5), 1 one
        multinomial draw per particle, 2 systematic resampling (include/pfslam.h, pfslam_set_resampler).  Sharded: the same on every rank."""
        _chk(self.L.pfslam_set_resampler(self._h, int(mode)), "pfslam_set_resampler")

    def estimate_raw(self):
        """The 16 floats of pfslam_estimate (include/pfslam.h) as a float32 array."""
        out = np.zeros(16, np.float32)
        _chk(self.L.pfslam_estimate(self._h, _p(out)), "pfslam_estimate")
        return out

    def estimate(self):
        """Weighted mean pose, 3x3 covariance and Neff of the cloud, reduced on the device (include/pfslam.h, pfslam_estimate): the heading
        mean is linear.  Sharded handles: buffers 10 and 17 must hold the gathered weights and pose blocks (ShardedSlam.estimate does that)."""
        return estimate_dict(self.estimate_raw())

    def nearest(self, xyz):
        """Exact nearest map node of every query point (include/pfslam.h, pfslam_nearest): (index, squared distance); index -1 for a
        query with a non-finite coordinate."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        best = np.empty(len(xyz), np.int32)
        d2 = np.empty(len(xyz), np.float32)
        _chk(self.L.pfslam_nearest(self._h, _p(xyz), len(xyz), _p(best), _p(d2)), "pfslam_nearest")
        return best, d2

    def register(self, start=None, **opts):
        """Iterated scan-to-map ICP on the device (include/pfslam.h, pfslam_register) from `start` (None: the handle's pose).  Options by
        name (max_iters, match, select, update, max_dist, eps_xy, eps_theta, min_pairs) over pfslam_register_default_opts.  Returns pose,
        status (0 max_iters, 1 converged, 2 too few pairs, 3 not finite), iterations, pairs, residual and trace (iterations x 8:
        x', y', theta', their three increments, pairs, mean squared residual).  Reads the handle's state, writes none of it."""
        o = RegisterOpts()
        self.L.pfslam_register_default_opts(C.byref(o))
        for k, v in opts.items():
            if k not in dict(RegisterOpts._fields_):
                raise TypeError("register() has no option %r" % k)
            setattr(o, k, v)
        pose, info = np.zeros(3, np.float32), np.zeros(8, np.float32)
        trace = np.zeros((max(1, min(int(o.max_iters), 64)), 8), np.float32)
        st = None if start is None else np.ascontiguousarray(start, dtype=np.float32)
        _chk(self.L.pfslam_register(self._h, None if st is None else _p(st), C.byref(o), _p(pose), _p(info), _p(trace)), "pfslam_register")
        it = int(info[1])
        return {"pose": pose, "status": int(info[0]), "iterations": it, "pairs": int(info[2]), "residual": float(info[3]),
                "trace": trace[:it].copy()}

    def register_batch(self, starts, **opts):
        """pfslam_register from every row of `starts` (m x 3) in one launch (include/pfslam.h, pfslam_register_batch); options as for
        register().  Returns poses (m, 3), status, iterations, pairs (int arrays), residual (float32 array), info (m, 8: the rows as
        pfslam_register returns them) and best, the row the header's rule picks (-1: none is eligible).  Row r is bit for bit
        register(starts[r], **opts) without its trace."""
        o = RegisterOpts()
        self.L.pfslam_register_default_opts(C.byref(o))
        for k, v in opts.items():
            if k not in dict(RegisterOpts._fields_):
                raise TypeError("register_batch() has no option %r" % k)
            setattr(o, k, v)
        st = np.ascontiguousarray(starts, dtype=np.float32).reshape(-1, 3)
        m = len(st)
        poses, info = np.zeros((max(m, 1), 3), np.float32), np.zeros((max(m, 1), 8), np.float32)
        best = C.c_int(-1)
        _chk(self.L.pfslam_register_batch(self._h, _p(st), m, C.byref(o), _p(poses), _p(info), C.byref(best)), "pfslam_register_batch")
        return {"poses": poses, "status": info[:, 0].astype(np.int32), "iterations": info[:, 1].astype(np.int32),
                "pairs": info[:, 2].astype(np.int32), "residual": info[:, 3].copy(), "info": info, "best": int(best.value)}

    def search(self, centre=None, scores=False, **opts):
        """Windowed correlative scan-to-map search (include/pfslam.h, pfslam_search) around `centre` (None: the handle's pose).  Options by
        name (half_x, half_y, half_theta, stride, step_theta, max_dist) over pfslam_search_default_opts.  Returns pose, status (0 ok,
        2 no heading has an in-range beam), index (the winner's k, -1 with status 2), beams, mean_d2, score, candidates, qcap, info (the
        eight floats) and, with scores=True, scores: S of every candidate, shaped (2 half_theta + 1, 2 half_y + 1, 2 half_x + 1).  Reads
        the handle's state, writes none of it."""
        o = SearchOpts()
        self.L.pfslam_search_default_opts(C.byref(o))
        for k, v in opts.items():
            if k not in ("half_x", "half_y", "half_theta", "stride", "step_theta", "max_dist"):
                raise TypeError("search() has no option %r" % k)
            setattr(o, k, v)
        pose, info = np.zeros(3, np.float32), np.zeros(8, np.float32)
        c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float32).reshape(-1)
        if c is not None and c.shape != (3,):
            raise ValueError("search(): centre must be (x, y, theta), got %d values" % c.size)
        vol = None
        if scores:
            shape = tuple(2 * max(int(v), 0) + 1 for v in (o.half_theta, o.half_y, o.half_x))
            if shape[0] * shape[1] * shape[2] <= 1 << 24:     # (a larger window is the library's to refuse)
                vol = np.zeros(shape, np.int32)
        _chk(self.L.pfslam_search(self._h, None if c is None else _p(c), C.byref(o), _p(pose), _p(info), None if vol is None else _p(vol)), "pfslam_search")
        out = {"pose": pose, "status": int(info[0]), "index": int(info[1]), "beams": int(info[2]), "mean_d2": float(info[3]), "score": int(info[4]),
               "candidates": int(info[5]), "qcap": int(info[6]), "info": info}
        if scores:
            out["scores"] = vol
        return out

    def search_scan(self, ref_scan, ref_pose=None, scan=None, centre=None, scores=False, **opts):
        """Correlative scan-to-scan search (include/pfslam.h, pfslam_search_scan): search()'s window around `centre` (None: ref_pose) scored
        against a distance field built from the end points of `ref_scan` taken at `ref_pose` (None: (0, 0, 0)); `scan` is the scan that is
        searched (None: the handle's scan).  No map is needed.  Options and the returned dict are search()'s, plus points: the reference
        beams in range.  Reads the handle's scan at most, writes none of its state."""
        o = SearchOpts()
        self.L.pfslam_search_default_opts(C.byref(o))
        for k, v in opts.items():
            if k not in ("half_x", "half_y", "half_theta", "stride", "step_theta", "max_dist"):
                raise TypeError("search_scan() has no option %r" % k)
            setattr(o, k, v)
        pose, info = np.zeros(3, np.float32), np.zeros(8, np.float32)
        ref = np.ascontiguousarray(ref_scan, dtype=np.float32).reshape(-1)
        sc = None if scan is None else np.ascontiguousarray(scan, dtype=np.float32).reshape(-1)
        for name, a in (("ref_scan", ref), ("scan", sc)):
            if a is not None and len(a) != self.nb:
                raise ValueError("search_scan(): %s must hold n_beams = %d ranges, got %d" % (name, self.nb, len(a)))
        rp = None if ref_pose is None else np.ascontiguousarray(ref_pose, dtype=np.float32).reshape(-1)
        c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float32).reshape(-1)
        for name, a in (("ref_pose", rp), ("centre", c)):
            if a is not None and a.shape != (3,):
                raise ValueError("search_scan(): %s must be (x, y, theta), got %d values" % (name, a.size))
        vol = None
        if scores:
            shape = tuple(2 * max(int(v), 0) + 1 for v in (o.half_theta, o.half_y, o.half_x))
            if shape[0] * shape[1] * shape[2] <= 1 << 24:     # (a larger window is the library's to refuse)
                vol = np.zeros(shape, np.int32)
        opt = lambda a: None if a is None else _p(a)
        _chk(self.L.pfslam_search_scan(self._h, _p(ref), opt(rp), opt(sc), opt(c), C.byref(o), _p(pose), _p(info), opt(vol)), "pfslam_search_scan")
        out = {"pose": pose, "status": int(info[0]), "index": int(info[1]), "beams": int(info[2]), "mean_d2": float(info[3]), "score": int(info[4]),
               "candidates": int(info[5]), "qcap": int(info[6]), "points": int(info[7]), "info": info}
        if scores:
            out["scores"] = vol
        return out

    def _cast_opts(self, who, opts):
        o = CastOpts()
        self.L.pfslam_cast_default_opts(C.byref(o))
        for k, v in opts.items():
            if k not in ("max_range", "w_min", "no_hit", "inflate", "skip_cells"):
                raise TypeError("%s() has no option %r" % (who, k))
            setattr(o, k, v)
        return o

    def cast(self, poses=None, cells=False, **opts):
        """The scan the map predicts from each of the m x 3 `poses` (None: the handle's pose), by a walk of every beam through a raster
        of the map's nodes (include/pfslam.h, pfslam_cast).  Options by name (max_range, w_min, no_hit, inflate, skip_cells) over
        pfslam_cast_default_opts.  Returns ranges (m x n_beams float32), cells (m x n_beams x 2 int32 with cells=True, else None; a miss
        is INT32_MIN twice) and stats (int64[8]: rays, hits, qualifying nodes, occupied cells, x0, y0, W, H).  Reads the handle's map,
        writes none of its state."""
        o = self._cast_opts("cast", opts)
        ps = None
        m = 1
        if poses is not None:
            ps = np.ascontiguousarray(poses, dtype=np.float32)
            if ps.ndim == 1 and ps.size == 3:
                ps = ps.reshape(1, 3)
            if ps.ndim != 2 or ps.shape[1] != 3:
                raise ValueError("cast(): poses must be m x (x, y, theta), got shape %r" % (ps.shape,))
            m = len(ps)
        rows = m if m * self.nb <= 1 << 24 else 0      # (a larger call is the library's to refuse)
        ranges = np.zeros((rows, self.nb), np.float32)
        ce = np.zeros((rows, self.nb, 2), np.int32) if cells else None
        stats = np.zeros(8, np.int64)
        _chk(self.L.pfslam_cast(self._h, None if ps is None else _p(ps), m, C.byref(o), _p(ranges), None if ce is None else _p(ce), _p(stats)), "pfslam_cast")
        return {"ranges": ranges, "cells": ce, "stats": stats}

    def map_raster(self, **opts):
        """The occupancy raster pfslam_cast walks through (include/pfslam.h, pfslam_map_raster; cast()'s options): (box, occ) with
        box = (x0, y0, W, H) in cells and occ a W x H uint8 array, occ[kx - x0, ky - y0] = 1 for an occupied cell."""
        o = self._cast_opts("map_raster", opts)
        stats = np.zeros(8, np.int64)
        _chk(self.L.pfslam_map_raster(self._h, C.byref(o), _p(stats), None, 0), "pfslam_map_raster")
        W, H = int(stats[6]), int(stats[7])
        occ = np.zeros((W, H), np.uint8)
        if W * H:
            _chk(self.L.pfslam_map_raster(self._h, C.byref(o), _p(stats), _p(occ), W * H), "pfslam_map_raster")
        return tuple(int(v) for v in stats[4:8]), occ

    def cast_score(self, poses=None, scan=None, particles=False, classes=False, **opts):
        """The beam-model score of each of the m x 3 `poses` (None: the handle's pose; particles=True: the handle's own particles, read on
        the device): the measured `scan` (None: the handle's scan) against the scan the map predicts from the pose, reduced to eight
        integers per pose on the device (include/pfslam.h, pfslam_cast_score).  Options by name over the defaults of both structures:
        the cast's (max_range, w_min, inflate, skip_cells; no_hit is not read) and tol, clip, z_min, z_max, count_miss.  Returns rows (m x 8 int32), its
        columns by name (valid, agree, through, short, miss, q1, q2, cost), rms (float64: sqrt(q2 / agree) in metres over the agreeing
        beams, nan where none agrees), classes (m x n_beams uint8 with classes=True, else None), best (the row picked, -1 for none) and
        stats (int64[8], as cast()'s).  Reads the handle's map, scan and particles, writes none of its state."""
        ours = ("tol", "clip", "z_min", "z_max", "count_miss")
        co = self._cast_opts("cast_score", {k: v for k, v in opts.items() if k not in ours})
        so = CastScoreOpts()
        self.L.pfslam_cast_score_default_opts(C.byref(so))
        for k in ours:
            if k in opts:
                setattr(so, k, opts[k])
        so.source = 1 if particles else 0
        ps = None
        m = self.n if particles else 1
        if poses is not None:
            ps = np.ascontiguousarray(poses, dtype=np.float32)
            if ps.ndim == 1 and ps.size == 3:
                ps = ps.reshape(1, 3)
            if ps.ndim != 2 or ps.shape[1] != 3:
                raise ValueError("cast_score(): poses must be m x (x, y, theta), got shape %r" % (ps.shape,))
            m = len(ps)
        sc = None
        if scan is not None:
            sc = np.ascontiguousarray(scan, dtype=np.float32).ravel()
            if sc.size != self.nb:
                raise ValueError("cast_score(): scan must have n_beams = %d ranges, got %d" % (self.nb, sc.size))
        held = m if 1 <= m <= 65536 else 0                 # (a call outside the caps is the library's to refuse)
        rows = np.zeros((held, 8), np.int32)
        cl = np.zeros((held if m * self.nb <= 1 << 24 else 0, self.nb), np.uint8) if classes else None
        best = C.c_int(-1)
        stats = np.zeros(8, np.int64)
        _chk(self.L.pfslam_cast_score(self._h, None if ps is None else _p(ps), m, None if sc is None else _p(sc), C.byref(co), C.byref(so), _p(rows),
                                      None if cl is None else _p(cl), C.byref(best), _p(stats)), "pfslam_cast_score")
        out = {"rows": rows, "classes": cl, "best": int(best.value), "stats": stats}
        for k, name in enumerate(CAST_SCORE_COLUMNS):
            out[name] = rows[:, k]
        with np.errstate(all="ignore"):
            out["rms"] = np.sqrt(rows[:, 6].astype(np.float64) / rows[:, 1]) * float(np.float32(so.tol) * np.float32(0.0625))
        return out

    def _cov_opts(self, sigma):
        q = CovOpts()
        self.L.pfslam_search_cov_default_opts(C.byref(q))
        if sigma is not None:
            q.sigma = sigma
        return q

    @staticmethod
    def _cov_dict(out, raw):
        """The covariance part of search_cov()'s / search_scan_cov()'s dict from the 16 floats of cov_out."""
        c = raw[3:9]
        out.update({"mean": raw[0:3].copy(), "cov": np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]], np.float32),
                    "neff": float(raw[9]), "edge": float(raw[13]), "raw": raw})
        return out

    def search_cov(self, centre=None, scores=False, sigma=None, **opts):
        """search() plus how well its winner is determined (include/pfslam.h, pfslam_search_cov): the score volume weighted with the
        likelihood of independent Gaussian beam errors of `sigma` metres (None: pfslam_search_cov_default_opts, 0.2) and reduced as
        estimate() reduces the cloud.  Returns search()'s dict plus mean (3), cov (3 x 3: x, y, theta), neff (the effective number of
        candidates), edge (the share of the weight on the window's border: not small = the window cuts the distribution) and raw (the
        16 floats of cov_out)."""
        o = SearchOpts()
        self.L.pfslam_search_default_opts(C.byref(o))
        for k, v in opts.items():
            if k not in ("half_x", "half_y", "half_theta", "stride", "step_theta", "max_dist"):
                raise TypeError("search_cov() has no option %r" % k)
            setattr(o, k, v)
        q = self._cov_opts(sigma)
        pose, info, raw = np.zeros(3, np.float32), np.zeros(8, np.float32), np.zeros(16, np.float32)
        c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float32).reshape(-1)
        if c is not None and c.shape != (3,):
            raise ValueError("search_cov(): centre must be (x, y, theta), got %d values" % c.size)
        vol = None
        if scores:
            shape = tuple(2 * max(int(v), 0) + 1 for v in (o.half_theta, o.half_y, o.half_x))
            if shape[0] * shape[1] * shape[2] <= 1 << 24:     # (a larger window is the library's to refuse)
                vol = np.zeros(shape, np.int32)
        _chk(self.L.pfslam_search_cov(self._h, None if c is None else _p(c), C.byref(o), C.byref(q), _p(pose), _p(info), _p(raw),
                                      None if vol is None else _p(vol)), "pfslam_search_cov")
        out = {"pose": pose, "status": int(info[0]), "index": int(info[1]), "beams": int(info[2]), "mean_d2": float(info[3]), "score": int(info[4]),
               "candidates": int(info[5]), "qcap": int(info[6]), "info": info}
        if scores:
            out["scores"] = vol
        return self._cov_dict(out, raw)

    def search_scan_cov(self, ref_scan, ref_pose=None, scan=None, centre=None, scores=False, sigma=None, **opts):
        """search_scan() plus how well its winner is determined (include/pfslam.h, pfslam_search_scan_cov); `sigma` and the added
        entries mean, cov, neff, edge and raw as search_cov()'s."""
        o = SearchOpts()
        self.L.pfslam_search_default_opts(C.byref(o))
        for k, v in opts.items():
            if k not in ("half_x", "half_y", "half_theta", "stride", "step_theta", "max_dist"):
                raise TypeError("search_scan_cov() has no option %r" % k)
            setattr(o, k, v)
        q = self._cov_opts(sigma)
        pose, info, raw = np.zeros(3, np.float32), np.zeros(8, np.float32), np.zeros(16, np.float32)
        ref = np.ascontiguousarray(ref_scan, dtype=np.float32).reshape(-1)
        sc = None if scan is None else np.ascontiguousarray(scan, dtype=np.float32).reshape(-1)
        for name, a in (("ref_scan", ref), ("scan", sc)):
            if a is not None and len(a) != self.nb:
                raise ValueError("search_scan_cov(): %s must hold n_beams = %d ranges, got %d" % (name, self.nb, len(a)))
        rp = None if ref_pose is None else np.ascontiguousarray(ref_pose, dtype=np.float32).reshape(-1)
        c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float32).reshape(-1)
        for name, a in (("ref_pose", rp), ("centre", c)):
            if a is not None and a.shape != (3,):
                raise ValueError("search_scan_cov(): %s must be (x, y, theta), got %d values" % (name, a.size))
        vol = None
        if scores:
            shape = tuple(2 * max(int(v), 0) + 1 for v in (o.half_theta, o.half_y, o.half_x))
            if shape[0] * shape[1] * shape[2] <= 1 << 24:     # (a larger window is the library's to refuse)
                vol = np.zeros(shape, np.int32)
        opt = lambda a: None if a is None else _p(a)
        _chk(self.L.pfslam_search_scan_cov(self._h, _p(ref), opt(rp), opt(sc), opt(c), C.byref(o), C.byref(q), _p(pose), _p(info), _p(raw), opt(vol)),
             "pfslam_search_scan_cov")
        out = {"pose": pose, "status": int(info[0]), "index": int(info[1]), "beams": int(info[2]), "mean_d2": float(info[3]), "score": int(info[4]),
               "candidates": int(info[5]), "qcap": int(info[6]), "points": int(info[7]), "info": info}
        if scores:
            out["scores"] = vol
        return self._cov_dict(out, raw)

    def search_wide(self, centre=None, **opts):
        """pfslam_search's winner over windows of up to 2^31 - 1 candidates, found by branch and bound (include/pfslam.h,
        pfslam_search_wide).  Returns search()'s dict without scores, index and candidates exact (from stats), plus stats: the eight
        int64 {k, candidates, nodes bounded above level 0, candidates scored, top level, batches, cells of the field box, 0}."""
        o = SearchOpts()
        self.L.pfslam_search_default_opts(C.byref(o))
        for k, v in opts.items():
            if k not in ("half_x", "half_y", "half_theta", "stride", "step_theta", "max_dist"):
                raise TypeError("search_wide() has no option %r" % k)
            setattr(o, k, v)
        pose, info, stats = np.zeros(3, np.float32), np.zeros(8, np.float32), np.zeros(8, np.int64)
        c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float32).reshape(-1)
        if c is not None and c.shape != (3,):
            raise ValueError("search_wide(): centre must be (x, y, theta), got %d values" % c.size)
        _chk(self.L.pfslam_search_wide(self._h, None if c is None else _p(c), C.byref(o), _p(pose), _p(info), _p(stats)), "pfslam_search_wide")
        return {"pose": pose, "status": int(info[0]), "index": int(stats[0]), "beams": int(info[2]), "mean_d2": float(info[3]), "score": int(info[4]),
                "candidates": int(stats[1]), "qcap": int(info[6]), "info": info, "stats": stats}

    def search_best(self, centre=None, count=8, tile_log2=3, group_theta=8, **opts):
        """The best candidate of each of the `count` best cells of a search window (include/pfslam.h, pfslam_search_best): a cell is a tile of
        2^tile_log2 x 2^tile_log2 translations times group_theta consecutive headings.  The window's options are search()'s.  Returns poses
        (found, 3), info (found, 8), index (int64, the rows' k), score and beams per row, found and stats: pfslam_search_wide's eight int64
        with the number of cells in [7].  Row 0 is search_wide()'s winner; the rows are register_batch()'s `starts`."""
        o = SearchOpts()
        self.L.pfslam_search_default_opts(C.byref(o))
        for k, v in opts.items():
            if k not in ("half_x", "half_y", "half_theta", "stride", "step_theta", "max_dist"):
                raise TypeError("search_best() has no option %r" % k)
            setattr(o, k, v)
        b = BestOpts(int(count), int(tile_log2), int(group_theta), 0)
        rows = min(max(int(count), 1), 64)
        poses, info, index = np.zeros((rows, 3), np.float32), np.zeros((rows, 8), np.float32), np.zeros(rows, np.int64)
        stats, found = np.zeros(8, np.int64), C.c_int(0)
        c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float32).reshape(-1)
        if c is not None and c.shape != (3,):
            raise ValueError("search_best(): centre must be (x, y, theta), got %d values" % c.size)
        _chk(self.L.pfslam_search_best(self._h, None if c is None else _p(c), C.byref(o), C.byref(b), _p(poses), _p(info), _p(index), C.byref(found),
                                       _p(stats)), "pfslam_search_best")
        n = int(found.value)
        return {"poses": poses[:n].copy(), "info": info[:n].copy(), "index": index[:n].copy(), "score": info[:n, 4].astype(np.int64),
                "beams": info[:n, 2].astype(np.int32), "found": n, "stats": stats}

    def frame_mode(self):
        out = (C.c_int * 4)()
        _chk(self.L.pfslam_frame_mode(self._h, out), "pfslam_frame_mode")
        return {"round5_frame": bool(out[0]), "gates": bool(out[1]), "serial": bool(out[2]), "publish_lag": int(out[3])}

    def set_probe(self, frames):
        _chk(self.L.pfslam_set_probe(self._h, int(frames)), "pfslam_set_probe")

    def probe(self, frames=4096):
        """Wall-clock stamps of the launches of the last round-5 frames: (names, array[f][slot], last ticket).  Absolute values of the device's
        100 MHz wall clock in microseconds (subtract a frame's scan-match stamp for a timeline: tools/frame_probe.py); 0 = that launch did not run in that frame."""
        buf = np.zeros((frames, 32), np.uint64)
        n, last = C.c_int(0), C.c_int(0)
        _chk(self.L.pfslam_get_probe(self._h, _p(buf), frames, C.byref(n), C.byref(last)), "pfslam_get_probe")
        names = []
        for k in range(32):
            s = self.L.pfslam_probe_name(k).decode()
            if not s:
                break
            names.append(s)
        t = buf[:n.value, :len(names)].astype(np.float64) * 0.01
        return names, t, last.value

    def ubench_gather(self):
        out = (C.c_double * 4)()
        _chk(self.L.pfslam_ubench_gather(self._h, out), "pfslam_ubench_gather")
        return {"wave_gathers_per_s": out[0], "cus": int(out[1]), "nominal_ghz": out[2], "cycles_per_wave_gather": out[3]}

    def resample_plan(self, frame):
        did, neff = C.c_int(), C.c_float()
        _chk(self.L.pfslam_resample_plan(self._h, frame, C.byref(did), C.byref(neff)), "pfslam_resample_plan")
        return did.value, neff.value

    def resample_gather(self):
        _chk(self.L.pfslam_resample_gather(self._h), "pfslam_resample_gather")

    def score_grid(self):
        fit = np.empty(self.n, np.int32)
        _chk(self.L.pfslam_score_grid(self._h, _p(fit)), "pfslam_score_grid")
        return fit

    def update_map_grid(self):
        _chk(self.L.pfslam_update_map_grid(self._h), "pfslam_update_map_grid")

    def step(self, frame, scan):
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        _chk(self.L.pfslam_step(self._h, frame, _p(scan)), "pfslam_step")

    def shard_disperse(self, frame, scan):
        """Sharded frame (see include/pfslam.h): scan, re-balance, ICP fork, dispersion; True when the frame only seeded the map."""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        seeded = C.c_int(0)
        _chk(self.L.pfslam_shard_disperse(self._h, frame, _p(scan), C.byref(seeded)), "pfslam_shard_disperse")
        return bool(seeded.value)

    def shard_score(self):
        _chk(self.L.pfslam_shard_score(self._h), "pfslam_shard_score")

    def shard_weights(self):
        _chk(self.L.pfslam_shard_weights(self._h), "pfslam_shard_weights")

    def shard_finish(self):
        _chk(self.L.pfslam_shard_finish(self._h), "pfslam_shard_finish")

    def shard_stream(self, which):
        """hipStream_t (as an int) collective `which` (0 pose blocks, 1 keys, 2 weights) of the frame being enqueued goes into."""
        st = C.c_void_p(0)
        _chk(self.L.pfslam_shard_stream(self._h, which, C.byref(st)), "pfslam_shard_stream")
        return st.value or 0

    # -- multi-GPU re-balance: one host build per node (include/pfslam.h)
    def set_shard_balance(self, external):
        _chk(self.L.pfslam_set_shard_balance(self._h, 1 if external else 0), "pfslam_set_shard_balance")

    def shard_balance_due(self, frame):
        """(due, n_nodes); books the frames in flight when the re-balance period hits."""
        due, n = C.c_int(0), C.c_int(0)
        _chk(self.L.pfslam_shard_balance_due(self._h, frame, C.byref(due), C.byref(n)), "pfslam_shard_balance_due")
        return bool(due.value), n.value

    def shard_balance_build(self, frame):
        _chk(self.L.pfslam_shard_balance_build(self._h, frame), "pfslam_shard_balance_build")

    def shard_balance_adopt(self):
        _chk(self.L.pfslam_shard_balance_adopt(self._h), "pfslam_shard_balance_adopt")

    def step_grid(self, frame, scan):
        """One frame of the 2-D occupancy-grid variant (motion, grid score + weights, grid update, resample)."""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        _chk(self.L.pfslam_step_grid(self._h, frame, _p(scan)), "pfslam_step_grid")

    def traverse(self, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        best = np.empty(len(xyz), np.int32)
        _chk(self.L.pfslam_traverse(self._h, _p(xyz), len(xyz), _p(best)), "pfslam_traverse")
        return best

    def debug_math(self, which, x):
        x = np.ascontiguousarray(x, dtype=np.float32).ravel()
        out = np.empty(len(x) * (2 if which in (0, 6, 7, 8) else 1), np.float32)
        _chk(self.L.pfslam_debug_math(self._h, which, _p(x), len(x), _p(out)), "pfslam_debug_math")
        if which in (6, 8):
            return out.view(np.int32).reshape(-1, 2)
        return out.reshape(-1, 2) if which in (0, 7) else out

    # -- read-back
    @property
    def pose(self):
        out = np.zeros(3, np.float32)
        _chk(self.L.pfslam_get_pose(self._h, _p(out)), "pfslam_get_pose")
        return out

    def particles(self):
        ptr, n = C.c_void_p(), C.c_int()
        _chk(self.L.pfslam_get_particles(self._h, C.byref(ptr), C.byref(n)), "pfslam_get_particles")
        buf = (C.c_char * (32 * n.value)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=PARTICLE_DTYPE).copy()

    def map(self):
        ptr, n = C.c_void_p(), C.c_int()
        _chk(self.L.pfslam_get_map(self._h, C.byref(ptr), C.byref(n)), "pfslam_get_map")
        if n.value == 0:
            return np.zeros(0, NODE_DTYPE)
        buf = (C.c_char * (32 * n.value)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=NODE_DTYPE).copy()

    def grid(self):
        ptr, dx, dy = C.c_void_p(), C.c_int(), C.c_int()
        _chk(self.L.pfslam_get_grid(self._h, C.byref(ptr), C.byref(dx), C.byref(dy)), "pfslam_get_grid")
        buf = (C.c_char * (dx.value * dy.value)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=np.int8).reshape(dx.value, dy.value).copy()

    def trace(self):
        t = np.zeros(8, np.int32)
        _chk(self.L.pfslam_get_trace(self._h, _p(t)), "pfslam_get_trace")
        return {"best": int(t[0]), "resampled": int(t[1]), "n_wall": int(t[2]), "n_free": int(t[3]),
                "n_insert": int(t[4]), "neff": float(t[5:6].view(np.float32)[0]), "kd_size": int(t[6])}

    def cells(self, which):
        cap = 1600 * 1600
        out = np.empty(cap, np.int32)
        n = C.c_int()
        _chk(self.L.pfslam_get_cells(self._h, which, _p(out), cap, C.byref(n)), "pfslam_get_cells")
        return out[:n.value].copy()

    def device_ptr(self, which):
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        _chk(self.L.pfslam_device_ptr(self._h, which, C.byref(ptr), C.byref(nbytes)), "pfslam_device_ptr")
        return ptr.value, nbytes.value
