"""ctypes binding of the C ABI in include/fast_vgicp_hip.h (libfast_vgicp_hip.so).

This is the only way Python reaches the engine: plain pointers and sizes, no torch types.
There is no CPU fallback -- if the shared library is missing, importing the handles fails loudly.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

# enum ordinals (== the reference's enum class ordinals, gicp_settings.hpp:7-11 / ndt_settings.hpp:6)
REG_NONE, REG_MIN_EIG, REG_NORMALIZED_MIN_EIG, REG_PLANE, REG_FROBENIUS = range(5)
DIRECT27, DIRECT7, DIRECT1, DIRECT_RADIUS = range(4)
NDT_P2D, NDT_D2D = 0, 1
COMPUTE_FP64, COMPUTE_FP32, COMPUTE_CUDA_COMPAT = 0, 1, 2
VOXEL_ADDITIVE, VOXEL_ADDITIVE_WEIGHTED, VOXEL_MULTIPLICATIVE = range(3)
VOXEL_NDT_SUMS = 3  # `mode` of a snapshot of an NDT map (FVH_VOXEL_NDT_SUMS): never a VGICP accumulation mode

EXPORTED_SYMBOLS = None  # filled by _declared_symbols()


class LmParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("rotation_epsilon", C.c_double), ("transformation_epsilon", C.c_double), ("lm_max_iterations", C.c_int),
                ("lm_init_lambda_factor", C.c_double), ("optimizer", C.c_int)]


class LmResult(C.Structure):
    _fields_ = [("T", C.c_double * 16), ("H", C.c_double * 36), ("final_error", C.c_double), ("converged", C.c_int), ("nr_iterations", C.c_int),
                ("num_linearize", C.c_int), ("num_error_evals", C.c_int), ("lm_failed", C.c_int), ("num_launches", C.c_int)]


class EngineParams(C.Structure):
    """fvh_engine_params (include/fast_vgicp_hip.h): the routes / thresholds / watchdogs of ONE handle"""
    _fields_ = [("struct_size", C.c_int), ("sort_mode", C.c_int), ("sort_items", C.c_int), ("sort_fused_bits", C.c_int), ("sort_two_pass_max", C.c_int),
                ("sort_coop_watchdog_ticks", C.c_ulonglong), ("knn_nearest_first_max_points", C.c_int), ("knn_block", C.c_int), ("coherent_min_points", C.c_int),
                ("bitmap_min_points", C.c_int), ("bitmap_max_bytes", C.c_ulonglong), ("persistent", C.c_int), ("persist_watchdog_ticks", C.c_ulonglong),
                ("peer_watchdog_ticks", C.c_ulonglong), ("lm_everywhere", C.c_int), ("cost_prio", C.c_int), ("cost_split", C.c_int), ("cost_group_max", C.c_int),
                ("cost_max_blocks", C.c_int), ("cost_target_items", C.c_longlong), ("zerocopy_result", C.c_int), ("host_wait_block", C.c_int),
                ("result_query_spins", C.c_ulonglong), ("side_stream", C.c_int), ("pinned_upload_max", C.c_ulonglong), ("zerocopy_upload_max", C.c_ulonglong),
                ("avg_fused", C.c_int), ("nn1_seed", C.c_int)]


def default_engine_params():
    p = EngineParams()
    load().fvh_default_engine_params(C.byref(p))
    return p


class MapScore(C.Structure):
    """fvh_map_score (include/fast_vgicp_hip.h): what fvh_*_score_source / _score_cloud report"""
    _fields_ = [("n_points", C.c_int), ("n_used", C.c_int), ("n_in_voxel", C.c_int), ("n_near", C.c_int), ("n_explained", C.c_int),
                ("sum_best_m2", C.c_double), ("sum_score_max", C.c_double), ("sum_score_all", C.c_double)]


class RayCast(C.Structure):
    """fvh_ray_cast (include/fast_vgicp_hip.h): what fvh_*_cast_rays_source / _cast_rays_cloud report"""
    _fields_ = [("n_rays", C.c_int), ("n_used", C.c_int), ("n_hit", C.c_int), ("n_hit_at_origin", C.c_int), ("n_cells", C.c_longlong)]


class FvhError(RuntimeError):
    pass


_LIB = None


def lib_path():
    return os.environ.get("FVH_LIB_PATH") or _build.LIB_PATH  # override: A/B runs against another build of the same ABI


def load():
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise FvhError("libfast_vgicp_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'`; there is no CPU fallback." % path)
        L = C.CDLL(path)
        L.fvh_vgicp_last_error.restype = C.c_char_p
        L.fvh_ndt_last_error.restype = C.c_char_p
        L.fvh_voxelgrid_last_error.restype = C.c_char_p
        for fn in (L.fvh_vgicp_align_multi, L.fvh_ndt_align_multi):
            fn.argtypes = ALIGN_MULTI_ARGTYPES
            fn.restype = C.c_int
        L.fvh_debug_lm_replay.argtypes = LM_REPLAY_ARGTYPES
        L.fvh_debug_lm_replay.restype = C.c_int
        fn = getattr(L, "fvh_debug_regularize", None)  # (absent from an older build of the ABI named by FVH_LIB_PATH)
        if fn is not None:
            fn.argtypes = REGULARIZE_ARGTYPES
            fn.restype = C.c_int
        for name, argtypes in OUTLIER_ARGTYPES.items():  # (doubles in the middle of the list: a bare Python float would not convert)
            fn = getattr(L, name, None)
            if fn is None:  # FVH_LIB_PATH names an older build of the ABI (A/B runs): calling the method then raises AttributeError
                continue
            fn.argtypes = argtypes
            fn.restype = C.c_int
        for name, argtypes in list(DESKEW_ARGTYPES.items()) + list(CLUSTER_ARGTYPES.items()) + list(PLANE_ARGTYPES.items()):
            fn = getattr(L, name, None)
            if fn is None:  # (an older build of the ABI, as above)
                continue
            fn.argtypes = argtypes
            fn.restype = C.c_int
        _LIB = L
    return _LIB


# fvh_{vgicp,ndt}_align_multi(handle, k, guesses16, params, results, grid_blocks_out)
ALIGN_MULTI_ARGTYPES = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
MAX_MULTI = 64  # hypotheses per align_multi call


def _outlier_argtypes():
    """fvh_voxelgrid_{crop_range, remove_statistical_outliers, remove_radius_outliers}[_strided|_device] + the getters, as the header declares them"""
    h, p, i, d = C.c_void_p, C.c_void_p, C.c_int, C.c_double
    params = {"crop_range": [d, d], "remove_statistical_outliers": [i, d], "remove_radius_outliers": [d, i]}
    out = {}
    for base, tail in params.items():
        out["fvh_voxelgrid_" + base] = [h, p, i] + tail + [p]
        out["fvh_voxelgrid_" + base + "_strided"] = [h, p, i, i] + tail + [p]
        out["fvh_voxelgrid_" + base + "_device"] = [h, p, i, i] + tail + [p]
    out["fvh_voxelgrid_get_kept_indices"] = [h, p]
    out["fvh_voxelgrid_get_scores"] = [h, p, p]
    out["fvh_voxelgrid_profile_get_class"] = [h, C.c_char_p, p, p]
    return out


OUTLIER_ARGTYPES = _outlier_argtypes()


def _deskew_argtypes():
    """fvh_voxelgrid_deskew[_strided|_device], as the header declares them"""
    h, p, i, d = C.c_void_p, C.c_void_p, C.c_int, C.c_double
    tail = [p, i, p, p, i, d, p]  # times, time_stride, knot_times, knot_poses, K, t_ref, out_n
    return {"fvh_voxelgrid_deskew": [h, p, i] + tail, "fvh_voxelgrid_deskew_strided": [h, p, i, i] + tail, "fvh_voxelgrid_deskew_device": [h, p, i, i] + tail}


DESKEW_ARGTYPES = _deskew_argtypes()


def _cluster_argtypes():
    """fvh_voxelgrid_cluster_euclidean[_strided|_device] and fvh_voxelgrid_get_cluster_labels, as the header declares them"""
    h, p, i, d = C.c_void_p, C.c_void_p, C.c_int, C.c_double
    tail = [d, i, i, p, p]  # tolerance, min_cluster_size, max_cluster_size, num_clusters, out_n
    return {"fvh_voxelgrid_cluster_euclidean": [h, p, i] + tail, "fvh_voxelgrid_cluster_euclidean_strided": [h, p, i, i] + tail,
            "fvh_voxelgrid_cluster_euclidean_device": [h, p, i, i] + tail, "fvh_voxelgrid_get_cluster_labels": [h, p, p]}


CLUSTER_ARGTYPES = _cluster_argtypes()


def _plane_argtypes():
    """fvh_voxelgrid_segment_plane[_strided|_device] and fvh_voxelgrid_get_plane_model, as the header declares them"""
    h, p, i, d = C.c_void_p, C.c_void_p, C.c_int, C.c_double
    tail = [d, i, C.c_ulonglong, p, d, i, p, p, p]  # distance_threshold, max_iterations, seed, axis, eps_angle, flags, coefficients, num_inliers, out_n
    return {"fvh_voxelgrid_segment_plane": [h, p, i] + tail, "fvh_voxelgrid_segment_plane_strided": [h, p, i, i] + tail,
            "fvh_voxelgrid_segment_plane_device": [h, p, i, i] + tail, "fvh_voxelgrid_get_plane_model": [h, p, p, p, p]}


PLANE_ARGTYPES = _plane_argtypes()
PLANE_KEEP_OUTLIERS, PLANE_REFINE = 1, 2  # enum fvh_plane_flags


def declared_symbols():
    """Every function declared in include/fast_vgicp_hip.h (parsed from the header)."""
    import re
    hdr = open(_build.HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(fvh_[a-z0-9_]+)\s*\(", hdr)))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return C.c_void_p(a.__array_interface__["data"][0])  # (a.ctypes.data_as costs 3.7 us a call)


def _colmajor16(T):
    return np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(4, 4).T)


def _lm_params(max_iterations=64, rotation_epsilon=2e-3, transformation_epsilon=5e-4, lm_max_iterations=10, lm_init_lambda_factor=1e-9, optimizer=0):
    """optimizer: 0 Levenberg-Marquardt (default), 1 Gauss-Newton (LSQ_OPTIMIZER_TYPE, lsq_registration.hpp:15)"""
    return LmParams(max_iterations, rotation_epsilon, transformation_epsilon, lm_max_iterations, lm_init_lambda_factor, optimizer)


_IDENTITY16 = np.ascontiguousarray(np.eye(4))  # the default guess / parameters of align(): built once (these calls sit between two LM kernels, with the GPU idle)
_DEFAULT_LM = _lm_params()


def _result_dict(r):
    # one view over the struct's 52 leading doubles (the arrays keep `r` alive): this runs between an align and the next launch,
    # with the GPU idle
    a = np.frombuffer(r, dtype=np.float64, count=52)
    return dict(T=a[:16].reshape(4, 4).T, H=a[16:].reshape(6, 6).T, final_error=r.final_error, converged=bool(r.converged),
                nr_iterations=r.nr_iterations, iterations=r.nr_iterations + 1, num_linearize=r.num_linearize, num_error_evals=r.num_error_evals,
                lm_failed=bool(r.lm_failed), num_launches=r.num_launches)


# ---- map snapshot files (VGICPCore / NDTMapCore .map_save / map_load; FastVGICPCuda::saveTargetMap / loadTargetMap write the same bytes) ----
# little-endian: magic "FVHVMAP\0" (8 bytes) | version u32 = 1 | mode i32 | num_inserts i32 | num_voxels i32 | num_points i64 | resolution f64
# (40 bytes) | coords i32[n][3] | sums f64[n][10] | ages u32[n]          ("Map snapshot files")
MAP_FILE_MAGIC = b"FVHVMAP\0"
MAP_FILE_VERSION = 1
_MAP_FILE_HEADER = np.dtype([("magic", "S8"), ("version", "<u4"), ("mode", "<i4"), ("num_inserts", "<i4"), ("num_voxels", "<i4"), ("num_points", "<i8"), ("resolution", "<f8")])


def _snapshot_arrays(snapshot):
    coords = np.ascontiguousarray(snapshot["coords"], dtype=np.int32).reshape(-1, 3)
    sums = np.ascontiguousarray(snapshot["sums"], dtype=np.float64).reshape(-1, 10)
    ages = snapshot.get("ages")
    ages = np.zeros(len(coords), np.uint32) if ages is None else np.ascontiguousarray(ages, dtype=np.uint32).reshape(-1)
    if not (len(coords) == len(sums) == len(ages)):
        raise FvhError("map snapshot: coords, sums and ages differ in length (%d, %d, %d)" % (len(coords), len(sums), len(ages)))
    return coords, sums, ages


def write_map_file(path, snapshot):
    """Write a snapshot (the dict VGICPCore.map_export returns) to `path`. Needs no GPU."""
    coords, sums, ages = _snapshot_arrays(snapshot)
    hdr = np.zeros(1, _MAP_FILE_HEADER)
    hdr["magic"], hdr["version"], hdr["mode"], hdr["num_inserts"] = MAP_FILE_MAGIC, MAP_FILE_VERSION, int(snapshot["mode"]), int(snapshot["num_inserts"])
    hdr["num_voxels"], hdr["num_points"], hdr["resolution"] = len(coords), int(snapshot["num_points"]), float(snapshot["resolution"])
    with open(path, "wb") as f:
        f.write(hdr.tobytes())
        f.write(coords.astype("<i4", copy=False).tobytes())
        f.write(sums.astype("<f8", copy=False).tobytes())
        f.write(ages.astype("<u4", copy=False).tobytes())


def read_map_file(path):
    """-> the snapshot dict of write_map_file's file; FvhError for a file that is not one (magic, version, size). Needs no GPU."""
    with open(path, "rb") as f:
        raw = f.read()
    hs = _MAP_FILE_HEADER.itemsize
    if len(raw) < hs:
        raise FvhError("%s: not a map snapshot (shorter than the header)" % path)
    # (magic compared on the raw bytes: numpy strips an S8's trailing NUL)
    if raw[:8] != MAP_FILE_MAGIC:
        raise FvhError("%s: not a map snapshot (magic)" % path)
    hdr = np.frombuffer(raw, _MAP_FILE_HEADER, count=1)[0]
    if int(hdr["version"]) != MAP_FILE_VERSION:
        raise FvhError("%s: map snapshot version %d, this build reads %d" % (path, int(hdr["version"]), MAP_FILE_VERSION))
    n = int(hdr["num_voxels"])
    if n < 0 or len(raw) != hs + n * (12 + 80 + 4):
        raise FvhError("%s: map snapshot truncated or corrupt (%d voxels need %d bytes, file has %d)" % (path, n, hs + max(n, 0) * 96, len(raw)))
    o = hs
    coords = np.frombuffer(raw, "<i4", 3 * n, o).reshape(n, 3).astype(np.int32); o += 12 * n
    sums = np.frombuffer(raw, "<f8", 10 * n, o).reshape(n, 10).astype(np.float64); o += 80 * n
    ages = np.frombuffer(raw, "<u4", n, o).astype(np.uint32)
    return dict(resolution=float(hdr["resolution"]), mode=int(hdr["mode"]), num_inserts=int(hdr["num_inserts"]), num_points=int(hdr["num_points"]), num_voxels=n,
                coords=coords, sums=sums, ages=ages)


def clear_rays_check(min_range, max_range, end_margin, min_misses, origin=None):
    """The refusals of fvh_*_clear_rays_* that need no handle, given before the call (FvhError): the library gives the same ones, and
    those that need the map (max_range beyond 4096 voxels) or the cloud. Needs no GPU."""
    import math
    if origin is not None and not (np.size(origin) == 3 and np.all(np.isfinite(np.asarray(origin, np.float64)))):
        raise FvhError("map_clear_rays: origin must be 3 finite values")
    if not min_range >= 0.0:
        raise FvhError("map_clear_rays: min_range must be >= 0")
    if not math.isfinite(max_range) or max_range < min_range:
        raise FvhError("map_clear_rays: max_range must be finite and >= min_range")
    if not math.isfinite(end_margin) or end_margin < 0.0:
        raise FvhError("map_clear_rays: end_margin must be finite and >= 0")
    if int(min_misses) < 1:
        raise FvhError("map_clear_rays: min_misses must be >= 1")


class _IncrementalMap:
    """The incremental target map of a handle class whose C prefix has map_* / voxelmap_* calls (mixed into VGICPCore and NDTMapCore)."""

    # ---- incremental target map (include/fast_vgicp_hip.h: fvh_vgicp_map_* / fvh_ndt_map_*; the calls VGICPCore and NDTMapCore share) ----
    def map_begin(self, expected_voxels=0):
        """Start (or restart) an empty incremental target map at the handle's resolution (and, VGICP, voxel accumulation mode)."""
        self._call("map_begin", int(expected_voxels))

    def map_insert_source(self, T=None):
        """Add the current source (VGICP: points + covariances; NDT: points) to the map at pose T (4x4, default identity)."""
        t = _IDENTITY16 if T is None else _colmajor16(T)
        self._call("map_insert_source", _p(t))

    def map_prune(self, center=None, radius=0.0, max_age=0):
        """Drop voxels further than `radius` from `center` (None: no distance rule) and those untouched by the last max_age inserts (0: no age rule). -> voxels removed"""
        removed = C.c_int(0)
        c = None if center is None else np.ascontiguousarray(center, np.float64).reshape(3)
        self._call("map_prune", None if c is None else _p(c), C.c_double(radius), int(max_age), C.byref(removed))
        return removed.value

    def map_info(self):
        inc, nv, cap, ni, dr = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        npts = C.c_longlong(0)
        self._call("map_get_info", C.byref(inc), C.byref(nv), C.byref(cap), C.byref(ni), C.byref(npts), C.byref(dr))
        return dict(incremental=bool(inc.value), num_voxels=nv.value, capacity=cap.value, num_inserts=ni.value, num_points=npts.value, dropped=dr.value)

    # ---- snapshots of the incremental map (fvh_{vgicp,ndt}_voxelmap_export / _import / _merge_from) ----
    def map_export(self):
        """The live incremental map as a snapshot: header fields + coords (n, 3) int32, sums (n, 10) float64 (the device's own per-voxel sums)
        and ages (n,) uint32, rows in ascending packed-key order (z-major, then y, then x)."""
        nv, mode, ni = C.c_int(0), C.c_int(0), C.c_int(0)
        res, npts = C.c_double(0.0), C.c_longlong(0)
        self._call("voxelmap_export", C.byref(nv), C.byref(res), C.byref(mode), C.byref(ni), C.byref(npts), None, None, None)
        n = nv.value
        coords, sums, ages = np.empty((n, 3), np.int32), np.empty((n, 10), np.float64), np.empty(n, np.uint32)
        if n:
            self._call("voxelmap_export", C.byref(nv), C.byref(res), C.byref(mode), C.byref(ni), C.byref(npts), _p(coords), _p(sums), _p(ages))
        return dict(resolution=res.value, mode=mode.value, num_inserts=ni.value, num_points=npts.value, num_voxels=n, coords=coords, sums=sums, ages=ages)

    def map_import(self, snapshot):
        """ADD a snapshot's voxels into the live map (restore: map_begin() first): sums and counts add, ages and the insert count carry over."""
        coords, sums, ages = _snapshot_arrays(snapshot)
        n = len(coords)
        self._call("voxelmap_import", n, _p(coords) if n else None, _p(sums) if n else None, _p(ages) if n else None, C.c_double(snapshot["resolution"]), int(snapshot["mode"]),
                   int(snapshot["num_inserts"]), C.c_longlong(int(snapshot["num_points"])))

    def map_merge_from(self, other):
        """ADD the live map of `other` (a handle of the same class on the same device, same resolution and mode) into this one, device to device; `other` is unchanged."""
        self._call("voxelmap_merge_from", other.h)

    def map_save(self, path):
        write_map_file(path, self.map_export())


class _PosedMap:
    """A live map added under a rigid pose, and re-anchored in place (include/fast_vgicp_hip.h: fvh_{vgicp,ndt}_posed_merge_from /
    _transform_map): mixed into VGICPMapCore and NDTMapCore, the handle classes for scan-to-map work."""

    def map_merge_from_posed(self, other, T):
        """ADD the live map of `other`, seen from pose T (4x4, other's frame -> this map's frame, rigid), into this one on the device: every
        voxel's sums are transformed in closed form and go to the voxel of their own mean (fvh_*_posed_merge_from).
        -> rows skipped because their mean left the key range"""
        skipped, t = C.c_int(0), _colmajor16(T)
        self._call("posed_merge_from", other.h, _p(t), C.byref(skipped))
        return skipped.value

    def map_transform(self, T):
        """Re-anchor the live map by the rigid pose T in place (fvh_*_transform_map): what map_begin on a fresh handle +
        map_merge_from_posed(this, T) would hold; insert count, num_points and ages stay. -> rows skipped"""
        skipped, t = C.c_int(0), _colmajor16(T)
        self._call("transform_map", _p(t), C.byref(skipped))
        return skipped.value


class _RayClearing:
    """Free-space carving on the live incremental map (include/fast_vgicp_hip.h: fvh_{vgicp,ndt}_clear_rays_source / _cloud): mixed into
    VGICPMapCore and NDTMapCore, the handle classes for scan-to-map work."""

    def map_clear_rays(self, T=None, xyz=None, origin=None, min_range=0.0, max_range=100.0, end_margin=0.0, min_misses=1, device_ptr=None, n=None, stride=3):
        """Free-space carving (fvh_*_clear_rays_source / _cloud): drop the voxels that at least min_misses rays of this call cross and none
        ends in. The rays run from `origin` (scan frame, None: (0, 0, 0)) to the current source points (xyz and device_ptr None), to the
        host points xyz (m, 3), or to n device points at device_ptr (stride 3 or 4 floats), all at pose T (4x4, default identity); rays outside
        [min_range, max_range] metres are skipped and a walk stops end_margin metres in front of its endpoint. -> (voxels removed, rays used)"""
        clear_rays_check(min_range, max_range, end_margin, min_misses, origin)
        t = _IDENTITY16 if T is None else _colmajor16(T)
        o = None if origin is None else np.ascontiguousarray(origin, np.float64).reshape(3)
        removed, used = C.c_int(0), C.c_int(0)
        tail = (_p(t), None if o is None else _p(o), C.c_double(min_range), C.c_double(max_range), C.c_double(end_margin), int(min_misses), C.byref(removed), C.byref(used))
        if device_ptr is not None:
            self._call("clear_rays_cloud", C.c_void_p(device_ptr), int(n), int(stride), 1, *tail)
        elif xyz is not None:
            a = _f32(xyz).reshape(-1, 3)
            self._call("clear_rays_cloud", _p(a) if len(a) else None, len(a), 3, 0, *tail)
        else:
            self._call("clear_rays_source", *tail)
        return removed.value, used.value


class _MapScoring:
    """A posed scan scored against the handle's target voxel map, batch or incremental (include/fast_vgicp_hip.h: fvh_{vgicp,ndt}_score_source /
    _score_cloud): mixed into VGICPMapCore and NDTMapCore, the handle classes for scan-to-map work."""

    def map_score(self, T=None, xyz=None, device_ptr=None, n=None, stride=3, neighbors=DIRECT7, min_points=1, max_m2=float("inf"), score_scale=1.0, per_point=False):
        """How well the map explains a scan at pose T (4x4, default identity): the current source points (xyz and device_ptr None), the host points
        xyz (m, 3), or n device points at device_ptr (stride 3 or 4 floats). Around every point the voxels of `neighbors` (DIRECT1 / DIRECT7 /
        DIRECT27) with >= min_points points are looked up; a point is explained when its best squared Mahalanobis distance is finite and <= max_m2; scores
        are exp(-0.5 * score_scale * m2). Read-only on the handle. -> dict of the struct's fields plus overlap = n_in_voxel / n_used, nvtl =
        sum_score_max / n_near, tp = sum_score_all / n_used (NaN on a zero denominator); per_point adds found, best (int32) and best_m2
        (float64), one row per point in input order (skipped points: -1, -1, NaN)."""
        t = _IDENTITY16 if T is None else _colmajor16(T)
        out = MapScore()
        head = (_p(t), int(neighbors), int(min_points), C.c_double(max_m2), C.c_double(score_scale), C.byref(out))
        if device_ptr is not None:
            m = int(n)
        elif xyz is not None:
            a = _f32(xyz).reshape(-1, 3)
            m = len(a)
        else:  # the rows a source score writes are the source cloud's
            cnt = C.c_int(0)
            if per_point:
                self._call("get_num_source_points", C.byref(cnt))
            m = cnt.value
        found = np.empty(m, np.int32) if per_point else None
        best = np.empty(m, np.int32) if per_point else None
        best_m2 = np.empty(m, np.float64) if per_point else None
        rows = tuple(_p(v) if per_point and m else None for v in (found, best, best_m2))
        if device_ptr is not None:
            self._call("score_cloud", C.c_void_p(device_ptr), m, int(stride), 1, *head, *rows)
        elif xyz is not None:
            self._call("score_cloud", _p(a) if m else None, m, 3, 0, *head, *rows)
        else:
            self._call("score_source", *head, *rows)
        r = {name: getattr(out, name) for name, _ in MapScore._fields_}
        nan = float("nan")
        r["overlap"] = r["n_in_voxel"] / r["n_used"] if r["n_used"] else nan
        r["nvtl"] = r["sum_score_max"] / r["n_near"] if r["n_near"] else nan
        r["tp"] = r["sum_score_all"] / r["n_used"] if r["n_used"] else nan
        if per_point:
            r["found"], r["best"], r["best_m2"] = found, best, best_m2
        return r


def ray_endpoints(origin, directions, length, T=None):
    """Rays given as directions, for map_cast_rays: -> (xyz, max_range). xyz: float32 (m, 3) endpoints origin + length * unit direction in the
    scan frame (directions need not be unit; length: a scalar or one value per ray); max_range: the value to pass with them at pose T (4x4,
    default identity), chosen so that NO ray of these is skipped for range: the library measures a ray between the float32 roundings of the
    POSED origin and endpoint, which can come out longer than `length` by a few float32 roundings of the posed coordinates. Needs no GPU."""
    o = np.asarray(origin, np.float64).reshape(3)
    d = np.asarray(directions, np.float64).reshape(-1, 3)
    norm = np.sqrt((d * d).sum(axis=1))
    if not (np.all(np.isfinite(o)) and np.all(np.isfinite(d)) and np.all(norm > 0.0)):
        raise FvhError("ray_endpoints: origin and directions must be finite and no direction may be zero")
    ln = np.broadcast_to(np.asarray(length, np.float64), (len(d),))
    if not (np.all(np.isfinite(ln)) and np.all(ln > 0.0)):
        raise FvhError("ray_endpoints: length must be finite and > 0")
    xyz = (o + d / norm[:, None] * ln[:, None]).astype(np.float32)
    if not len(xyz):
        return xyz, 0.0
    # the library's own measure, r = |(float)(R p + t) - (float)(R o + t)|, formed here in numpy; how numpy adds up R p + t may move a
    # float32 rounding by one ulp of the posed coordinate on either end, per axis: four ulps of the largest posed magnitude times sqrt(3) cover it
    M = np.eye(4) if T is None else np.asarray(T, np.float64).reshape(4, 4)
    po = (M[:3, :3] @ o + M[:3, 3]).astype(np.float32).astype(np.float64)
    pp = (xyz.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32).astype(np.float64)
    r = float(np.sqrt(((pp - po) ** 2).sum(axis=1)).max())
    big = max(float(np.abs(po).max()), float(np.abs(pp).max()))
    return xyz, r + 4.0 * 2.0 ** -23 * big * 1.7320508075688772 + r * 2.0 ** -50


class _RayCasting:
    """Rays cast into the handle's target voxel map, batch or incremental (include/fast_vgicp_hip.h: fvh_{vgicp,ndt}_cast_rays_source /
    _cast_rays_cloud): mixed into VGICPMapCore and NDTMapCore, the handle classes for scan-to-map work."""

    def map_cast_rays(self, T=None, xyz=None, device_ptr=None, n=None, stride=3, origin=None, min_range=0.0, max_range=100.0, min_points=1, max_m2=float("inf"), per_ray=True):
        """What the map says a sensor at pose T (4x4, default identity) should see along each ray: the segments from `origin` (scan frame,
        None: (0, 0, 0)) to the current source points (xyz and device_ptr None), to the host points xyz (m, 3), or to n device points at
        device_ptr (stride 3 or 4 floats) are walked through the grid; in every voxel with >= min_points points the segment's point of
        smallest squared Mahalanobis distance to the voxel's Gaussian is found, and the first voxel where it is <= max_m2 (and beyond
        min_range metres) is the hit. Rays longer than max_range are skipped. Read-only on the handle. -> dict of the struct's fields;
        per_ray adds hit (int32: 1, 0 no hit, -1 skipped), cell (m, 3) int32, range and m2 (float64), one row per ray in input order.
        (ray_endpoints() makes endpoints and a max_range out of directions.)"""
        t = _IDENTITY16 if T is None else _colmajor16(T)
        o = None if origin is None else np.ascontiguousarray(origin, np.float64).reshape(3)
        out = RayCast()
        head = (_p(t), None if o is None else _p(o), C.c_double(min_range), C.c_double(max_range), int(min_points), C.c_double(max_m2), C.byref(out))
        if device_ptr is not None:
            m = int(n)
        elif xyz is not None:
            a = _f32(xyz).reshape(-1, 3)
            m = len(a)
        else:  # the rows a cast to the source writes are the source cloud's
            cnt = C.c_int(0)
            if per_ray:
                self._call("get_num_source_points", C.byref(cnt))
            m = cnt.value
        hit = np.empty(m, np.int32) if per_ray else None
        cell = np.empty((m, 3), np.int32) if per_ray else None
        rng = np.empty(m, np.float64) if per_ray else None
        m2 = np.empty(m, np.float64) if per_ray else None
        rows = tuple(_p(v) if per_ray and m else None for v in (hit, cell, rng, m2))
        if device_ptr is not None:
            self._call("cast_rays_cloud", C.c_void_p(device_ptr), m, int(stride), 1, *head, *rows)
        elif xyz is not None:
            self._call("cast_rays_cloud", _p(a) if m else None, m, 3, 0, *head, *rows)
        else:
            self._call("cast_rays_source", *head, *rows)
        r = {name: getattr(out, name) for name, _ in RayCast._fields_}
        if per_ray:
            r["hit"], r["cell"], r["range"], r["m2"] = hit, cell, rng, m2
        return r


class _MapTarget:
    """The live incremental map as the handle's target cloud (include/fast_vgicp_hip.h: fvh_{vgicp,ndt}_target_from_map, _get_target_points):
    mixed into VGICPMapCore and NDTMapCore, the handle classes for scan-to-map work."""

    def target_from_map(self, min_points=1):
        """The target cloud becomes one point per voxel with >= min_points points -- the voxel's mean (VGICP: + its covariance as the target
        covariance), rows in ascending packed-key order: with min_points <= 1 row i is row i of map_export(). A snapshot: call it again after
        an insert or a prune. The map stays live and untouched. -> number of points (0: the handle has no target cloud)"""
        n = C.c_int(0)
        self._call("target_from_map", int(min_points), C.byref(n))
        return n.value

    def get_target_points(self):
        """The current target cloud, (n, 3) float32 in its original order (however it was set: host, device, filter, target_from_map)."""
        n = C.c_int(0)
        self._call("get_num_target_points", C.byref(n))
        out = np.empty((n.value, 3), np.float32)
        self._call("get_target_points", _p(out) if n.value else None)
        return out


class _Core:
    _prefix = ""

    def __init__(self, device=0):
        self._lib = load()
        if "_fns" not in type(self).__dict__:
            type(self)._fns = {}  # per class (VGICPCore / NDTCore have different prefixes)
        self.device = int(device)
        self.h = C.c_void_p()
        rc = getattr(self._lib, self._prefix + "create")(int(device), C.byref(self.h))
        if rc != 0:
            raise FvhError("%screate failed with status %d" % (self._prefix, rc))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            getattr(self._lib, self._prefix + "destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args):
        fn = self._fns.get(name)
        if fn is None:  # (bound once per class: the attribute lookup on the CDLL sits between an align and the next launch)
            fn = self._fns[name] = getattr(self._lib, self._prefix + name)
        rc = fn(self.h, *args)
        if rc != 0:
            msg = getattr(self._lib, self._prefix + "last_error")(self.h)
            raise FvhError("%s%s: status %d: %s" % (self._prefix, name, rc, msg.decode() if msg else ""))

    # ---- shared API ----
    def get_engine_params(self):
        p = EngineParams()
        self._call("get_engine_params", C.byref(p))
        return p

    def set_engine_params(self, **fields):
        """change some of this handle's engine parameters (names: fvh_engine_params), e.g. set_engine_params(persistent=0, sort_mode=1)"""
        p = self.get_engine_params()
        for k, v in fields.items():
            if k not in dict(EngineParams._fields_) or k == "struct_size":
                raise FvhError("unknown engine parameter %r" % k)
            setattr(p, k, v)
        self._call("set_engine_params", C.byref(p))
        return p

    def set_resolution(self, r):
        self._call("set_resolution", C.c_double(r))

    def set_neighbor_search_method(self, method, radius=-1.0):
        self._call("set_neighbor_search_method", int(method), C.c_double(radius))

    def set_precision(self, p):
        self._call("set_precision", int(p))

    def swap_source_and_target(self):
        self._call("swap_source_and_target")

    def set_source_cloud(self, xyz):
        a = _f32(xyz)
        self._call("set_source_cloud", _p(a), len(a))

    def set_target_cloud(self, xyz):
        a = _f32(xyz)
        self._call("set_target_cloud", _p(a), len(a))

    def set_source_cloud_device(self, ptr, n, stride=3):
        self._call("set_source_cloud_device", C.c_void_p(ptr), int(n), int(stride))

    def set_target_cloud_device(self, ptr, n, stride=3):
        self._call("set_target_cloud_device", C.c_void_p(ptr), int(n), int(stride))

    def update_correspondences(self, T):
        t = _colmajor16(T)
        self._call("update_correspondences", _p(t))

    def compute_error(self, T, derivatives=True):
        t = _colmajor16(T)
        err = C.c_double(0)
        if derivatives:
            H = np.empty((6, 6), np.float64)
            b = np.empty(6, np.float64)
            self._call("compute_error", _p(t), _p(H), _p(b), C.byref(err))
            return err.value, H.T.copy(), b
        self._call("compute_error", _p(t), None, None, C.byref(err))
        return err.value

    def linearize(self, T):
        """LsqRegistration::linearize of the reference wrappers: update_correspondences + compute_error."""
        self.update_correspondences(T)
        return self.compute_error(T, True)

    def align(self, guess=None, **lm):
        g = _IDENTITY16 if guess is None else _colmajor16(guess)
        p = _lm_params(**lm) if lm else _DEFAULT_LM
        r = LmResult()
        self._call("align", _p(g), C.byref(p), C.byref(r))
        return _result_dict(r)

    def align_multi(self, guesses, **lm):
        """K independent registrations of the same pair from K initial guesses ((K, 4, 4) or a list of 4x4) in one launch. Returns one
        align() result dict per guess, each with `grid_blocks`: the workgroups per hypothesis -- result k equals, bit for bit, align(guess k)
        on a handle whose cost_max_blocks is that number."""
        g = np.asarray(guesses, dtype=np.float64)
        if g.ndim != 3 or g.shape[1:] != (4, 4):
            raise FvhError("align_multi: guesses must be (K, 4, 4), got %s" % (g.shape,))
        k = g.shape[0]
        cm = np.ascontiguousarray(np.transpose(g, (0, 2, 1)))  # column-major per pose
        p = _lm_params(**lm) if lm else _DEFAULT_LM
        res = (LmResult * max(k, 1))()
        nb = C.c_int(0)
        self._call("align_multi", int(k), _p(cm), C.byref(p), res, C.byref(nb))
        out = []
        for i in range(k):
            d = _result_dict(res[i])
            d["grid_blocks"] = nb.value
            out.append(d)
        return out

    def fitness_score(self, T, max_range=1.7976931348623157e308):
        t = _colmajor16(T)
        s = C.c_double(0)
        self._call("fitness_score", _p(t), C.c_double(max_range), C.byref(s))
        return s.value

    def synchronize(self):
        self._call("synchronize")

    def set_lm_trace(self, on=True):
        self._call("set_lm_trace", int(on))

    def get_lm_trace(self):
        """Rows {i, y0, yi, rho, lambda, |d|} of the last align (one per trial step), as LsqRegistration's debug print."""
        n = C.c_int(0)
        self._call("get_lm_trace", C.byref(n), None)
        out = np.empty((n.value, 6), np.float64)
        if n.value:
            self._call("get_lm_trace", C.byref(n), _p(out))
        return out

    def profile_enable(self, on=True):
        self._call("profile_enable", int(on))

    def profile_reset(self):
        self._call("profile_reset")

    def profile_get(self, cls):
        ms = C.c_double(0)
        n = C.c_int(0)
        self._call("profile_get", cls.encode(), C.byref(ms), C.byref(n))
        return ms.value, n.value

    def comm_init(self, unique_id, nranks, rank):
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        self._call("comm_init", buf, int(nranks), int(rank))

    def comm_destroy(self):
        self._call("comm_destroy")

    def get_num_correspondences(self):
        n = C.c_int(0)
        self._call("get_num_correspondences", C.byref(n))
        return n.value


def comm_unique_id():
    buf = (C.c_char * 128)()
    rc = load().fvh_comm_unique_id(buf)
    if rc != 0:
        raise FvhError("fvh_comm_unique_id failed: %d" % rc)
    return bytes(buf)


def debug_slot_pool(device=0):
    """(reserved, active, recent) of the process-wide pool that splits a device's co-resident workgroup slots between concurrent aligns."""
    r, a, c = C.c_int(0), C.c_int(0), C.c_int(0)
    load().fvh_debug_slot_pool(int(device), C.byref(r), C.byref(a), C.byref(c))
    return r.value, a.value, c.value


def debug_sort_routes():
    """[cooperative, one workgroup, two-launch passes, four-launch passes]: Morton sorts queued by this process so far, per route"""
    a = (C.c_int * 4)()
    rc = load().fvh_debug_sort_routes(a)
    if rc != 0:
        raise FvhError("fvh_debug_sort_routes: status %d" % rc)
    return list(a)


def debug_xcd_local():
    """(wanted, placement_aborts): whether persistent launches still use XCD-local hand-offs, and how many launches the placement check ended."""
    w, a = C.c_int(0), C.c_int(0)
    load().fvh_debug_xcd_local(C.byref(w), C.byref(a))
    return w.value, a.value


# fvh_debug_lm_replay(device, guess16, params, n_steps, sums, rows, steps_run)
LM_REPLAY_ARGTYPES = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
LM_REPLAY_ROW = 133  # FVH_LM_REPLAY_ROW
LM_REPLAY_INTS = ("phase", "outer_iter", "inner_iter", "converged", "lm_failed", "num_linearize", "num_error_evals", "nr_iterations", "corr_cur", "delta_converged")
PH_LINEARIZE, PH_TRIAL, PH_DONE, PH_TRIAL_FINAL = 0, 1, 2, 6  # LmState::phase (kernels_cost.hpp)


def _lm_replay_pose(a):
    T = np.eye(4)
    T[:3, :3] = a[:9].reshape(3, 3)
    T[:3, 3] = a[9:12]
    return T


def lm_replay_row(row):
    """One row of fvh_debug_lm_replay (layout: include/fast_vgicp_hip.h) as a dict: ints, floats, 4x4 poses, 6x6 H / final_H."""
    row = np.asarray(row, np.float64)
    d = {name: int(row[i]) for i, name in enumerate(LM_REPLAY_INTS)}
    d.update({"lambda": float(row[10]), "nu": float(row[11]), "y0": float(row[12]), "d": row[13:19].copy()})
    d.update(x0=_lm_replay_pose(row[19:31]), xi=_lm_replay_pose(row[31:43]), x_lin=_lm_replay_pose(row[43:55]))
    d.update(H=row[55:91].reshape(6, 6).copy(), b=row[91:97].copy(), final_H=row[97:133].reshape(6, 6).copy())
    return d


def debug_lm_replay(guess, sums, device=0, **lm):
    """The device LM step alone on scripted sums ((n_steps, 32) doubles, one row per evaluation): a list with one lm_replay_row dict per
    step taken -- the replay stops when the state is done -- or, when max_iterations <= 0 ends it before any step, the initial state alone.
    `lm`: the fvh_lm_params fields, as align()."""
    s = np.ascontiguousarray(sums, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] != 32:
        raise FvhError("debug_lm_replay: sums must be (n_steps, 32), got %s" % (s.shape,))
    n = s.shape[0]
    g = _IDENTITY16 if guess is None else _colmajor16(guess)
    p = _lm_params(**lm)
    rows = np.full((max(n, 1), LM_REPLAY_ROW), np.nan)
    taken = C.c_int(-1)
    fn = load().fvh_debug_lm_replay
    rc = fn(int(device), _p(g), C.byref(p), n, _p(s), _p(rows), C.byref(taken))
    if rc != 0:
        raise FvhError("fvh_debug_lm_replay: status %d" % rc)
    return [lm_replay_row(r) for r in rows[:max(taken.value, 1)]]


# fvh_debug_regularize(device, n, sym6, method, w3, V9, reg6)
REGULARIZE_ARGTYPES = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]


def debug_regularize(sym6, method, device=0):
    """The device eigen solver and regulariser alone (dev_math.hpp: sym_eig3, regularize_cov), fp64 in and out. sym6: (n, 6) {xx, xy, xz, yy, yz, zz}
    or (n, 3, 3) symmetric. -> (w (n, 3) ascending, V (n, 3, 3) with the eigenvectors in the columns, reg (n, 3, 3) = regularize_cov(method))."""
    s = np.asarray(sym6, dtype=np.float64)
    if s.ndim == 3 and s.shape[1:] == (3, 3):
        s = s.reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]]
    if s.ndim != 2 or s.shape[1] != 6:
        raise FvhError("debug_regularize: sym6 must be (n, 6) or (n, 3, 3), got %s" % (s.shape,))
    s = np.ascontiguousarray(s)
    n = s.shape[0]
    w, V, r = np.full((max(n, 1), 3), np.nan), np.full((max(n, 1), 9), np.nan), np.full((max(n, 1), 6), np.nan)
    rc = load().fvh_debug_regularize(int(device), n, _p(s), int(method), _p(w), _p(V), _p(r))
    if rc != 0:
        raise FvhError("fvh_debug_regularize: status %d" % rc)
    return w, V.reshape(-1, 3, 3), r[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def device_count():
    n = C.c_int(0)
    rc = load().fvh_device_count(C.byref(n))
    return n.value if rc == 0 else 0


class VGICPCore(_Core, _IncrementalMap):
    """fast_gicp::cuda::FastVGICPCudaCore on the HIP engine (same method names, snake_case as in the .cuh)."""
    _prefix = "fvh_vgicp_"

    # ---- pipelined scan streams (include/fast_vgicp_hip.h: fvh_vgicp_align_async ...) ----
    def align_async(self, guess=None, **lm):
        """Launch the LM kernel and return; align_wait() collects the result. In between only prepare_source_device() may be used."""
        self._g = _IDENTITY16 if guess is None else _colmajor16(guess)
        self._lm = _lm_params(**lm) if lm else _DEFAULT_LM
        self._call("align_async", _p(self._g), C.byref(self._lm))

    def align_wait(self):
        r = LmResult()
        self._call("align_wait", C.byref(r))
        return _result_dict(r)

    def prepare_source_device(self, ptr, n, stride=3, k=20, regularization=REG_PLANE, rbf=False, stages=3):
        """The NEXT source cloud (device pointer) into the prepared slot, on the handle's second stream: Morton sort, exact k-NN + covariances
        (or RBF covariances), and the scan's own voxel map -- beside whatever runs on the main stream."""
        self._call("prepare_source_device", C.c_void_p(ptr), int(n), int(stride), int(k), int(regularization), 1 if rbf else 0, int(stages))

    def prepare_source(self, xyz, k=20, regularization=REG_PLANE, rbf=False, stages=2):
        """The same for a host cloud (N x 3 float32): consumed before the call returns."""
        a = np.ascontiguousarray(xyz, np.float32)
        self._call("prepare_source", _p(a), len(a), 3, int(k), int(regularization), 1 if rbf else 0, int(stages))

    def adopt_prepared_source(self):
        self._call("adopt_prepared_source")

    # ---- multi-GPU through peer-mapped exchange regions (no RCCL) ----
    def peer_export(self, max_points):
        """-> (64-byte IPC handle, raw device pointer of the region)"""
        buf = (C.c_char * 64)()
        ptr = C.c_ulonglong(0)
        self._call("peer_export", int(max_points), buf, C.byref(ptr))
        return bytes(buf), ptr.value

    def peer_attach(self, nranks, rank, ranks_on_this_device, ipc_handles, process_local_ptrs=None):
        blob = b"".join(bytes(h) for h in ipc_handles)
        assert len(blob) == 64 * nranks
        hbuf = (C.c_char * len(blob)).from_buffer_copy(blob)
        pbuf = None
        if process_local_ptrs is not None:
            pbuf = (C.c_ulonglong * nranks)(*[int(p) for p in process_local_ptrs])
        self._call("peer_attach", int(nranks), int(rank), int(ranks_on_this_device), hbuf, pbuf)

    def set_target_map_sharding(self, on=True, margin_voxels=2):
        """Multi-GPU: this rank's target voxel map holds the voxels around its tile of the source only (rebuilt per align)."""
        self._call("set_target_map_sharding", 1 if on else 0, int(margin_voxels))

    def debug_spatial_order(self, which="source"):
        """(order, tile_boxes): the Morton order of a cloud (original index per sorted position) and the boxes of its 64-point tiles"""
        n = self.num_points(which)
        order = np.empty(max(n, 1), np.int32)
        boxes = np.empty(((max(n, 1) + 63) // 64, 8), np.float32)
        self._call("debug_get_spatial_order", 0 if which == "source" else 1, _p(order), _p(boxes))
        return order[:n], boxes[: (n + 63) // 64]

    def debug_live_map_voxels(self):
        n = C.c_int(0)
        self._call("debug_get_live_map_voxels", C.byref(n))
        return n.value

    def debug_map_shard(self):
        a, b = C.c_int(0), C.c_int(0)
        self._call("debug_get_map_shard", C.byref(a), C.byref(b))
        return bool(a.value), b.value

    def peer_detach(self):
        self._call("peer_detach")

    def peer_selfcheck(self, timeout_seconds=5.0):
        """Collective: a store of every rank reaches every rank (FvhError with the missing ranks otherwise)."""
        m = C.c_int(0)
        self._call("peer_selfcheck", C.c_double(timeout_seconds), C.byref(m))
        return m.value

    def set_voxel_accumulation_mode(self, mode):
        self._call("set_voxel_accumulation_mode", int(mode))

    def set_kernel_params(self, kernel_width, kernel_max_dist):
        self._call("set_kernel_params", C.c_double(kernel_width), C.c_double(kernel_max_dist))

    def num_points(self, which):
        n = C.c_int(0)
        self._call("get_num_%s_points" % which, C.byref(n))
        return n.value

    def set_source_neighbors(self, k, idx):
        a = np.ascontiguousarray(idx, np.int32)
        self._call("set_source_neighbors", int(k), _p(a))

    def set_target_neighbors(self, k, idx):
        a = np.ascontiguousarray(idx, np.int32)
        self._call("set_target_neighbors", int(k), _p(a))

    def find_source_neighbors(self, k):
        self._call("find_source_neighbors", int(k))

    def find_target_neighbors(self, k):
        self._call("find_target_neighbors", int(k))

    def calculate_source_covariances(self, method=REG_PLANE):
        self._call("calculate_source_covariances", int(method))

    def calculate_target_covariances(self, method=REG_PLANE):
        self._call("calculate_target_covariances", int(method))

    def calculate_source_covariances_rbf(self, method=REG_PLANE):
        self._call("calculate_source_covariances_rbf", int(method))

    def calculate_target_covariances_rbf(self, method=REG_PLANE):
        self._call("calculate_target_covariances_rbf", int(method))

    def set_source_covariances(self, covs):
        a = np.ascontiguousarray(covs, np.float64)
        self._call("set_source_covariances", _p(a))

    def set_target_covariances(self, covs):
        a = np.ascontiguousarray(covs, np.float64)
        self._call("set_target_covariances", _p(a))

    def get_neighbors(self, which):
        k = C.c_int(0)
        self._call("get_%s_neighbors" % which, C.byref(k), None)
        out = np.empty((self.num_points(which), k.value), np.int32)
        self._call("get_%s_neighbors" % which, C.byref(k), _p(out))
        return out

    def get_covariances(self, which):
        out = np.empty((self.num_points(which), 3, 3), np.float32)
        self._call("get_%s_covariances" % which, _p(out))
        return out

    def create_target_voxelmap(self):
        self._call("create_target_voxelmap")

    # ---- incremental target map: what takes covariances / picks a voxel type (the rest: _IncrementalMap) ----
    def map_insert_cloud(self, xyz, covs, T=None, device_ptr=None, n=None, stride=3):
        """Add a cloud that is not the source: host points (N x 3 float32) or a device pointer (device_ptr, n, stride), covariances N x 3 x 3 on the host."""
        t = _IDENTITY16 if T is None else _colmajor16(T)
        c = np.ascontiguousarray(covs, np.float64)
        if device_ptr is not None:
            self._call("map_insert_cloud", C.c_void_p(device_ptr), int(n), int(stride), _p(c), _p(t), 1)
        else:
            a = _f32(xyz)
            self._call("map_insert_cloud", _p(a), len(a), 3, _p(c), _p(t), 0)

    def map_load(self, path):
        """Add the file's map into the live map; a handle with no live map takes the file's resolution and mode and starts one sized for it."""
        snap = read_map_file(path)
        if not self.map_info()["incremental"]:
            self.set_resolution(snap["resolution"])
            self.set_voxel_accumulation_mode(VOXEL_MULTIPLICATIVE if snap["mode"] == 2 else VOXEL_ADDITIVE)
            self.map_begin(max(snap["num_voxels"], 1))
        self.map_import(snap)
        return snap

    def get_voxelmap(self):
        n = C.c_int(0)
        self._call("get_num_voxels", C.byref(n))
        nv = n.value
        coords = np.empty((nv, 3), np.int32)
        num = np.empty(nv, np.int32)
        means = np.empty((nv, 3), np.float32)
        covs = np.empty((nv, 3, 3), np.float32)
        self._call("get_voxel_coords", _p(coords))
        self._call("get_voxel_num_points", _p(num))
        self._call("get_voxel_means", _p(means))
        self._call("get_voxel_covs", _p(covs))
        return coords, num, means, covs

    def get_voxel_correspondences(self):
        n = self.get_num_correspondences()
        out = np.empty((n, 2), np.int32)
        self._call("get_voxel_correspondences", _p(out))
        return out

    def debug_set_voxel_hint(self, n):
        self._call("debug_set_voxel_hint", int(n))

    # ---- FastGICP (nearest target point) on the same handle ----
    def gicp_set_max_correspondence_distance(self, d):
        self._call("gicp_set_max_correspondence_distance", C.c_double(d))

    def gicp_swap_source_and_target(self):
        self._call("gicp_swap_source_and_target")

    def gicp_update_correspondences(self, T):
        t = _colmajor16(T)
        self._call("gicp_update_correspondences", _p(t))

    def gicp_compute_error(self, T, derivatives=True):
        t = _colmajor16(T)
        err = C.c_double(0)
        if derivatives:
            H = np.empty((6, 6), np.float64)
            b = np.empty(6, np.float64)
            self._call("gicp_compute_error", _p(t), _p(H), _p(b), C.byref(err))
            return err.value, H.T.copy(), b
        self._call("gicp_compute_error", _p(t), None, None, C.byref(err))
        return err.value

    def gicp_linearize(self, T):
        """FastGICP::linearize (fast_gicp_impl.hpp:159-213): update_correspondences + sums."""
        self.gicp_update_correspondences(T)
        return self.gicp_compute_error(T, True)

    def gicp_align(self, guess=None, **lm):
        g = _IDENTITY16 if guess is None else _colmajor16(guess)
        p = _lm_params(**lm) if lm else _DEFAULT_LM
        r = LmResult()
        self._call("gicp_align", _p(g), C.byref(p), C.byref(r))
        return _result_dict(r)

    def gicp_get_correspondences(self):
        out = np.empty(self.num_points("source"), np.int32)
        self._call("gicp_get_correspondences", _p(out))
        return out

    def debug_persist_aborts(self):
        n = C.c_int(0)
        self._call("debug_get_persist_aborts", C.byref(n))
        return n.value

    def debug_persist_grid(self):
        b, c = C.c_int(0), C.c_int(0)
        self._call("debug_get_persist_grid", C.byref(b), C.byref(c))
        return b.value, c.value

    def debug_table_capacity(self):
        n = C.c_int(0)
        self._call("debug_get_table_capacity", C.byref(n))
        return n.value

    def debug_skipped_points(self):
        n = C.c_int(0)
        self._call("debug_get_skipped_points", C.byref(n))
        return n.value


class VGICPMapCore(VGICPCore, _MapTarget, _PosedMap, _RayClearing, _MapScoring, _RayCasting):
    """A VGICP handle for scan-to-map work: VGICPCore (which has the map_* calls) + target_from_map / get_target_points, on the same C handle
    type -- as NDTMapCore is to NDTCore."""


class VoxelGrid:
    """pcl::VoxelGrid / pcl::ApproximateVoxelGrid on the device (fvh_voxelgrid_*): same output points in the same
    order as the PCL filters the reference's callers run before registration (src/align.cpp:136-147)."""

    EXACT, APPROXIMATE = 0, 1

    def __init__(self, device=0):
        self._lib = load()
        self._h = C.c_void_p()
        self._n_in = 0  # input size of the last crop / outlier / cluster call (scores(), cluster_labels())
        self.num_clusters = 0  # kept components of the last cluster_euclidean call
        self._plane_h = 0  # max_iterations of the last segment_plane call (plane_model())
        rc = self._lib.fvh_voxelgrid_create(int(device), C.byref(self._h))
        if rc != 0:
            raise FvhError("fvh_voxelgrid_create failed: %d" % rc)

    def close(self):
        if self._h:
            self._lib.fvh_voxelgrid_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise FvhError("%s: %s (code %d)" % (what, (self._lib.fvh_voxelgrid_last_error(self._h) or b"").decode(), rc))

    def filter(self, xyz, leaf, method=APPROXIMATE):
        """Host array in, host array out (float32 Nx3)."""
        a = _f32(np.asarray(xyz).reshape(-1, 3))
        n = C.c_int(0)
        self._check(self._lib.fvh_voxelgrid_filter(self._h, int(method), _p(a), len(a), C.c_float(leaf), C.byref(n)), "fvh_voxelgrid_filter")
        out = np.empty((n.value, 3), np.float32)
        self._check(self._lib.fvh_voxelgrid_get_points(self._h, _p(out)), "fvh_voxelgrid_get_points")
        return out

    def filter_strided(self, buf, stride, leaf, method=APPROXIMATE):
        """Host array of n x `stride` floats (e.g. a KITTI xyzi buffer, stride 4); only the first three of each row are used."""
        a = _f32(np.asarray(buf).reshape(-1, stride))
        n = C.c_int(0)
        self._check(self._lib.fvh_voxelgrid_filter_strided(self._h, int(method), _p(a), len(a), int(stride), C.c_float(leaf), C.byref(n)), "fvh_voxelgrid_filter_strided")
        out = np.empty((n.value, 3), np.float32)
        self._check(self._lib.fvh_voxelgrid_get_points(self._h, _p(out)), "fvh_voxelgrid_get_points")
        return out

    def share_stream(self, core):
        """Run this filter on the stream of a registration handle (NDTCore / VGICPCore; None: back to its own): its output is then
        ordered before whatever that handle queues next, and filter_device(..., asynchronous=True) may return while the last kernel
        of the filter is still running. The registration handle must outlive the sharing."""
        if core is None:
            self._check(self._lib.fvh_voxelgrid_share_stream_with_ndt(self._h, None), "fvh_voxelgrid_share_stream_with_ndt")
        elif isinstance(core, NDTCore):
            self._check(self._lib.fvh_voxelgrid_share_stream_with_ndt(self._h, core.h), "fvh_voxelgrid_share_stream_with_ndt")
        else:
            self._check(self._lib.fvh_voxelgrid_share_stream_with_vgicp(self._h, core.h), "fvh_voxelgrid_share_stream_with_vgicp")

    def share_prepare_stream(self, core):
        """Run this filter on the SECOND stream of an NDTCore / VGICPCore (the one prepare_source_device works on): the next frame is
        filtered beside the LM kernel of the current one."""
        if isinstance(core, NDTCore):
            self._check(self._lib.fvh_voxelgrid_share_prepare_stream_with_ndt(self._h, core.h), "fvh_voxelgrid_share_prepare_stream_with_ndt")
        else:
            self._check(self._lib.fvh_voxelgrid_share_prepare_stream_with_vgicp(self._h, core.h), "fvh_voxelgrid_share_prepare_stream_with_vgicp")

    def filter_device(self, d_ptr, n, leaf, method=APPROXIMATE, stride=3, asynchronous=False, want_pointer=True):
        """Device pointer in (n points, `stride` floats apart); returns (device pointer to packed xyz, count) valid until the next filter call.
        asynchronous (after share_stream): the count is final on return, the points are complete in the shared stream's order only.
        want_pointer=False: (0, count) -- for callers that hand the output over with NDTCore.*_from_voxelgrid (one ABI call less per frame)."""
        m = C.c_int(0)
        fn = self._lib.fvh_voxelgrid_filter_device_async if asynchronous else self._lib.fvh_voxelgrid_filter_device
        self._check(fn(self._h, int(method), C.c_void_p(d_ptr), int(n), int(stride), C.c_float(leaf), C.byref(m)), "fvh_voxelgrid_filter_device")
        if not want_pointer:
            return 0, m.value
        ptr = C.c_void_p()
        self._check(self._lib.fvh_voxelgrid_device_points(self._h, C.byref(ptr), C.byref(m)), "fvh_voxelgrid_device_points")
        return ptr.value or 0, m.value

    def get_points(self, n):
        """Host copy of the last filter_device() result (n = the count it returned); ordered after the filter on its stream."""
        out = np.empty((int(n), 3), np.float32)
        self._check(self._lib.fvh_voxelgrid_get_points(self._h, _p(out)), "fvh_voxelgrid_get_points")
        return out

    def profile_enable(self, on=True):
        self._check(self._lib.fvh_voxelgrid_profile_enable(self._h, int(on)), "profile_enable")

    def profile_reset(self):
        self._check(self._lib.fvh_voxelgrid_profile_reset(self._h), "profile_reset")

    def profile_get(self, cls="downsample"):
        """(total ms, launches) of one profile class of the filter's engine: "downsample", "sort", "knn", "outlier_count", "outlier_score", "compact", "deskew", "cluster", "plane" """
        ms, n = C.c_double(0), C.c_int(0)
        if cls == "downsample":
            self._check(self._lib.fvh_voxelgrid_profile_get(self._h, C.byref(ms), C.byref(n)), "profile_get")
        else:
            self._check(self._lib.fvh_voxelgrid_profile_get_class(self._h, cls.encode(), C.byref(ms), C.byref(n)), "profile_get_class")
        return ms.value, n.value

    # ---- range crop / outlier removal (fvh_voxelgrid_crop_range, _remove_statistical_outliers, _remove_radius_outliers): the kept points in
    # input order, bit copies of the input; kept_indices() / scores() describe the last of these calls ----
    def _stage(self, name, points, stride, *tail):
        """One stage call (crop / outlier / deskew / cluster / plane) in the form its points ask for: a host array of n x `stride` floats
        (fvh_voxelgrid_<name>, or _strided when stride != 3) or a (device pointer, n) pair (_device). `tail`: the stage's own arguments."""
        if isinstance(points, tuple):
            sym, n = "fvh_voxelgrid_" + name + "_device", int(points[1])
            head = (C.c_void_p(points[0]), n, int(stride))
        else:
            a = _f32(np.asarray(points).reshape(-1, stride))
            n = len(a)
            sym, head = ("fvh_voxelgrid_" + name, (_p(a), n)) if stride == 3 else ("fvh_voxelgrid_" + name + "_strided", (_p(a), n, int(stride)))
        self._n_in = max(n, 0)  # what scores() and cluster_labels() size their arrays by
        self._check(getattr(self._lib, sym)(self._h, *head, *tail), sym)

    def _outlier_host(self, name, xyz, stride, *params):
        n = C.c_int(0)
        self._stage(name, xyz, stride, *params, C.byref(n))
        return self.get_points(n.value)

    def _outlier_device(self, name, d_ptr, n, stride, *params):
        self._stage(name, (d_ptr, n), stride, *params, C.byref(C.c_int(0)))
        return self.device_points()

    def crop_range(self, xyz, min_sq_norm=1e-3, max_sq_norm=float("inf"), stride=3):
        """Keep the finite points with min_sq_norm <= |p|^2 (fp32) <= max_sq_norm; (m, 3) float32. The defaults are the reference's origin filter."""
        return self._outlier_host("crop_range", xyz, stride, float(min_sq_norm), float(max_sq_norm))

    def crop_range_device(self, d_ptr, n, min_sq_norm=1e-3, max_sq_norm=float("inf"), stride=3):
        """Device pointer in; (device pointer to packed xyz, count) as filter_device returns them."""
        return self._outlier_device("crop_range", d_ptr, n, stride, float(min_sq_norm), float(max_sq_norm))

    def remove_statistical_outliers(self, xyz, mean_k=20, stddev_mul=1.0, stride=3):
        """Keep the points whose mean distance to their mean_k nearest neighbours is at most mean + stddev_mul * stddev of that quantity."""
        return self._outlier_host("remove_statistical_outliers", xyz, stride, int(mean_k), float(stddev_mul))

    def remove_statistical_outliers_device(self, d_ptr, n, mean_k=20, stddev_mul=1.0, stride=3):
        return self._outlier_device("remove_statistical_outliers", d_ptr, n, stride, int(mean_k), float(stddev_mul))

    def remove_radius_outliers(self, xyz, radius=0.8, min_neighbors=2, stride=3):
        """Keep the points with at least min_neighbors other points within `radius`."""
        return self._outlier_host("remove_radius_outliers", xyz, stride, float(radius), int(min_neighbors))

    def remove_radius_outliers_device(self, d_ptr, n, radius=0.8, min_neighbors=2, stride=3):
        """The pointer may be this handle's own device_points(): stages chain on one handle."""
        return self._outlier_device("remove_radius_outliers", d_ptr, n, stride, float(radius), int(min_neighbors))

    # ---- motion compensation of a sweep (fvh_voxelgrid_deskew): every point moved into the sensor frame of t_ref along the piecewise
    # constant-twist trajectory through the knot poses; n points out, in input order. Run it FIRST in a chain: crop and voxel filter
    # change the indexing the times refer to. ----
    @staticmethod
    def _knots(knot_times, knot_poses, t_ref):
        tau = np.ascontiguousarray(knot_times, dtype=np.float64).reshape(-1)
        T = np.asarray(knot_poses, dtype=np.float64).reshape(-1, 4, 4)
        if len(T) != len(tau):
            raise ValueError("deskew: %d knot times but %d knot poses" % (len(tau), len(T)))
        T = np.ascontiguousarray(T.transpose(0, 2, 1))  # (K, 4, 4) row-major indexing -> the ABI's column-major matrices
        if t_ref is None:
            if len(tau) == 0:
                raise ValueError("deskew: no knots")
            t_ref = tau[-1]
        return tau, T, float(t_ref)

    def deskew(self, xyz, times, knot_times, knot_poses, t_ref=None, stride=3, time_stride=1):
        """Host arrays in, (n, 3) float32 out. times: one float32 per point (time_stride 1), or None with stride 4 and time_stride 4:
        xyzt rows, the time in the 4th float. knot_poses: (K, 4, 4), sensor-at-that-instant -> one fixed frame. t_ref None: knot_times[-1].
        A point with a non-finite coordinate or time comes out as NaNs (crop_range drops it)."""
        a = _f32(np.asarray(xyz).reshape(-1, stride))
        tau, T, t_ref = self._knots(knot_times, knot_poses, t_ref)
        n = C.c_int(0)
        if times is None:
            if stride != 4:
                raise ValueError("deskew: times=None needs xyzt rows (stride 4)")
            tp = C.c_void_p(a.__array_interface__["data"][0] + 12)
        else:
            t = _f32(times).reshape(-1)
            if len(t) < (len(a) - 1) * int(time_stride) + 1 and len(a):
                raise ValueError("deskew: %d times for %d points at time_stride %d" % (len(t), len(a), time_stride))
            tp = _p(t)
        self._stage("deskew", a, stride, tp, int(time_stride), _p(tau), _p(T), len(tau), t_ref, C.byref(n))
        return self.get_points(n.value)

    def deskew_device(self, d_xyz, n, d_times, knot_times, knot_poses, t_ref=None, stride=3, time_stride=1):
        """Device pointers in (the knots stay host arrays); (device pointer to packed xyz, count) as filter_device returns them.
        d_xyz may be this handle's own device_points()."""
        tau, T, t_ref = self._knots(knot_times, knot_poses, t_ref)
        self._stage("deskew", (d_xyz, n), stride, C.c_void_p(d_times), int(time_stride), _p(tau), _p(T), len(tau), t_ref, C.byref(C.c_int(0)))
        return self.device_points()

    # ---- Euclidean cluster extraction (fvh_voxelgrid_cluster_euclidean): connected components of "closer than tolerance", a size window,
    # clusters numbered by their smallest input index. The kept points are the handle's output (get_points / device_points /
    # kept_indices / scores work on it as after an outlier filter). ----
    def cluster_euclidean(self, points, tolerance, min_size=1, max_size=0, device=False, stride=3):
        """(labels int32[n]: cluster number per INPUT point or -1, sizes int32[num_clusters]). points: a host array of n x `stride`
        floats, or with device=True a (device pointer, n) pair -- which may be this handle's own device_points()."""
        nc, m = C.c_int(0), C.c_int(0)
        try:
            self._stage("cluster_euclidean", tuple(points) if device else points, stride, float(tolerance), int(min_size), int(max_size), C.byref(nc), C.byref(m))
        finally:
            self.num_clusters = nc.value  # (0 after a refused call)
        return self.cluster_labels()

    def cluster_labels(self):
        """(labels, sizes) of the last cluster_euclidean call on this handle"""
        labels, sizes = np.empty(self._n_in, np.int32), np.empty(self.num_clusters, np.int32)
        self._check(self._lib.fvh_voxelgrid_get_cluster_labels(self._h, _p(labels), _p(sizes)), "fvh_voxelgrid_get_cluster_labels")
        return labels, sizes

    # ---- plane segmentation by RANSAC (fvh_voxelgrid_segment_plane): H hypotheses from a counter-based generator, all scored in one sweep,
    # optional axis constraint and least-squares refit. The inliers (or with keep_outliers everything else) are the handle's output
    # (get_points / device_points / kept_indices / scores work on it as after an outlier filter). ----
    def segment_plane(self, points, distance_threshold, max_iterations=256, seed=0, axis=None, eps_angle=0.0, keep_outliers=False, refine=False, device=False, stride=3, flags=None):
        """(coefficients float64[4]: unit normal and d >= 0, num_inliers). points: a host array of n x `stride` floats, or with device=True
        a (device pointer, n) pair -- which may be this handle's own device_points(). flags: the raw flag word instead of the two booleans."""
        co, ni, m = np.zeros(4, np.float64), C.c_int(0), C.c_int(0)
        ax = None if axis is None else np.ascontiguousarray(axis, np.float64).reshape(3)
        tail = (float(distance_threshold), int(max_iterations), int(seed) & 0xFFFFFFFFFFFFFFFF, None if ax is None else _p(ax), float(eps_angle),
                int(flags) if flags is not None else (PLANE_KEEP_OUTLIERS if keep_outliers else 0) | (PLANE_REFINE if refine else 0), _p(co), C.byref(ni), C.byref(m))
        self._plane_h = max(int(max_iterations), 0)
        self._stage("segment_plane", tuple(points) if device else points, stride, *tail)
        return co, ni.value

    def plane_model(self):
        """dict(coefficients float64[4], sample int32[3], winner, valid, count_winner, num_inliers, counts int32[H]) of the last segment_plane
        call made through this object (the C getter writes max_iterations counts: the array is sized by that call's max_iterations)"""
        co, sample, info, counts = np.zeros(4, np.float64), np.zeros(3, np.int32), np.zeros(4, np.int32), np.empty(self._plane_h, np.int32)
        self._check(self._lib.fvh_voxelgrid_get_plane_model(self._h, _p(co), _p(sample), _p(info), _p(counts)), "fvh_voxelgrid_get_plane_model")
        return dict(coefficients=co, sample=sample, winner=int(info[0]), valid=int(info[1]), count_winner=int(info[2]), num_inliers=int(info[3]), counts=counts)

    def device_points(self):
        """(device pointer to the packed xyz of the last output, count)"""
        ptr, m = C.c_void_p(), C.c_int(0)
        self._check(self._lib.fvh_voxelgrid_device_points(self._h, C.byref(ptr), C.byref(m)), "fvh_voxelgrid_device_points")
        return ptr.value or 0, m.value

    def kept_indices(self):
        """Ascending indices into the input of the points the last crop / outlier call kept (int32)."""
        _, m = self.device_points()
        idx = np.empty(m, np.int32)
        self._check(self._lib.fvh_voxelgrid_get_kept_indices(self._h, _p(idx)), "fvh_voxelgrid_get_kept_indices")
        return idx

    def scores(self):
        """(float32[n_in] score per INPUT point of the last crop / outlier call, the threshold it was held against)"""
        s = np.empty(self._n_in, np.float32)
        t = C.c_double(0)
        self._check(self._lib.fvh_voxelgrid_get_scores(self._h, _p(s), C.byref(t)), "fvh_voxelgrid_get_scores")
        return s, t.value


class NDTCore(_Core):
    """fast_gicp::cuda::NDTCudaCore on the HIP engine."""
    _prefix = "fvh_ndt_"

    def set_distance_mode(self, mode):
        self._call("set_distance_mode", int(mode))

    def create_voxelmaps(self):
        self._call("create_voxelmaps")

    def create_target_voxelmap(self):
        self._call("create_target_voxelmap")

    def create_source_voxelmap(self):
        self._call("create_source_voxelmap")

    # ---- pipelined frame streams (include/fast_vgicp_hip.h: fvh_ndt_align_async ...) ----
    def align_async(self, guess=None, **lm):
        """Launch the LM kernel and return; align_wait() collects the result. In between only prepare_source_device() (and a VoxelGrid
        that shares the prepare stream) may be used on this handle."""
        self._g = _IDENTITY16 if guess is None else _colmajor16(guess)
        self._lm = _lm_params(**lm) if lm else _DEFAULT_LM
        self._call("align_async", _p(self._g), C.byref(self._lm))

    def align_wait(self):
        r = LmResult()
        self._call("align_wait", C.byref(r))
        return _result_dict(r)

    def prepare_source_device(self, ptr, n, stride=3):
        """The NEXT source cloud (device pointer) into the handle's prepared slot, on its second stream: widened and, for D2D, its
        voxel map built, beside whatever runs on the main stream."""
        self._call("prepare_source_device", C.c_void_p(ptr), int(n), int(stride))

    def prepare_source(self, xyz):
        """The same for a host cloud (N x 3 float32): consumed before the call returns."""
        a = np.ascontiguousarray(xyz, np.float32)
        self._call("prepare_source", _p(a), len(a), 3)

    # ---- the filter's last ApproximateVoxelGrid output becomes the cloud without a copy (fvh_ndt_*_from_voxelgrid) ----
    def set_source_cloud_from_voxelgrid(self, vg):
        self._call("set_source_cloud_from_voxelgrid", vg._h)

    def set_target_cloud_from_voxelgrid(self, vg):
        self._call("set_target_cloud_from_voxelgrid", vg._h)

    def prepare_source_from_voxelgrid(self, vg):
        self._call("prepare_source_from_voxelgrid", vg._h)

    def adopt_prepared_source(self):
        self._call("adopt_prepared_source")

    def debug_set_voxel_hint(self, which, n):
        self._call("debug_set_voxel_hint", 0 if which == "source" else 1, int(n))

    def debug_table_capacity(self, which):
        n = C.c_int(0)
        self._call("debug_get_table_capacity", 0 if which == "source" else 1, C.byref(n))
        return n.value

    def set_source_tile(self, rank, nranks):
        """Evaluate tile `rank` of `nranks` of the source only (P2D: points in Morton order, D2D: source voxels ranked by key): linearize /
        compute_error return PARTIAL sums, to be added over the ranks; nranks = 1 switches it off."""
        self._call("set_source_tile", int(rank), int(nranks))

    def get_num_voxels(self, which):
        n = C.c_int(0)
        self._call("get_num_voxels", 0 if which == "source" else 1, C.byref(n))
        return n.value

    def get_voxel_correspondences(self):
        """(n, 2): (source element, target voxel index of get_voxelmap("target")); the source element is a point index (P2D) or an
        index into get_voxelmap("source") (D2D)."""
        n = self.get_num_correspondences()
        out = np.empty((max(n, 1), 2), np.int32)
        self._call("get_voxel_correspondences", _p(out))
        return out[:n]

    def get_voxelmap(self, which):
        w = 1 if which == "target" else 0
        n = C.c_int(0)
        self._call("get_num_voxels", w, C.byref(n))
        nv = n.value
        coords = np.empty((nv, 3), np.int32)
        num = np.empty(nv, np.int32)
        means = np.empty((nv, 3), np.float32)
        covs = np.empty((nv, 3, 3), np.float32)
        self._call("get_voxels", w, _p(coords), _p(num), _p(means), _p(covs))
        return coords, num, means, covs


class NDTMapCore(NDTCore, _IncrementalMap, _MapTarget, _PosedMap, _RayClearing, _MapScoring, _RayCasting):
    """An NDT handle with the calls of its incremental target map (include/fast_vgicp_hip.h: fvh_ndt_map_* / fvh_ndt_voxelmap_*): map_begin,
    map_insert_source, map_prune, map_info, map_export, map_import, map_merge_from, map_save come from _IncrementalMap as on VGICPCore; NDT
    voxels take points only. Everything else is NDTCore's, on the same C handle type."""

    def map_insert_cloud(self, xyz, T=None, device_ptr=None, n=None, stride=3):
        """Add a cloud that is not the source: host points (N x 3 float32) or a device pointer (device_ptr, n, stride)."""
        t = _IDENTITY16 if T is None else _colmajor16(T)
        if device_ptr is not None:
            self._call("map_insert_cloud", C.c_void_p(device_ptr), int(n), int(stride), _p(t), 1)
        else:
            a = _f32(xyz)
            self._call("map_insert_cloud", _p(a), len(a), 3, _p(t), 0)

    def debug_skipped_points(self):
        n = C.c_int(0)
        self._call("debug_get_skipped_points", C.byref(n))
        return n.value

    def map_load(self, path):
        """Add the file's map (mode VOXEL_NDT_SUMS) into the live map; a handle with no live map takes the file's resolution and starts one sized for it."""
        snap = read_map_file(path)
        if not self.map_info()["incremental"]:
            self.set_resolution(snap["resolution"])
            self.map_begin(max(snap["num_voxels"], 1))
        self.map_import(snap)
        return snap
