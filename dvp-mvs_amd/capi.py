"""ctypes binding of the engine's C ABI (include/dvp_mvs.h -> libdvp_mvs_hip.so).

This is harness glue for tests and bench.py; the product is the shared library.  Loading fails
loudly when the HIP library is missing or cannot be built — there is no CPU fallback.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("DVP_MVS_LIB") or os.path.join(_HERE, "libdvp_mvs_hip.so")   # override: A/B builds
_LIB = None

STAGES = dict(gen_edge_inform=0, find_nearest_strong=1, gen_neighbours=2, neighbour_update=3,
              random_init=4, strong_update=5, ransac_fit=6, weak_update=7, get_depth_normal=8,
              filter_strong=9, depth_to_weak=10, local_refine=11)
STAGE_NAMES = {v: k for k, v in STAGES.items()}
STAGE_NAMES[12] = "strong_prep"   # timing bucket only (snapshot copies + sample search of every strong_update), not launchable
N_TIMING = 13
BUFFERS = dict(planes=(0, np.float32, 4), costs=(1, np.float32, 1), selected_views=(2, np.uint32, 1),
               view_weight=(3, np.uint8, 32), weak_info=(4, np.uint8, 1), weak_reliable=(5, np.uint8, 1),
               weak_nearest_strong=(6, np.int16, 2), neighbours_map=(7, np.int32, 1),
               neighbours=(8, np.int16, 2), fit_planes=(9, np.float32, 4), candidate=(10, np.int16, 2),
               edge=(11, np.uint8, 1), edge_neigh=(12, np.int16, 2), label=(13, np.int32, 1),
               label_boundary=(14, np.int16, 2), complex=(15, np.float32, 1), radius=(16, np.int32, 1))

# every symbol include/dvp_mvs.h declares
EXPORTS = ["dvp_ctx_create", "dvp_ctx_destroy", "dvp_ctx_reserve", "dvp_last_error", "dvp_upload_images", "dvp_upload_depths",
           "dvp_upload_images_device", "dvp_upload_depths_device", "dvp_upload_cameras", "dvp_upload_state", "dvp_upload_state_rescaled",
           "dvp_reset_state", "dvp_save_state", "dvp_restore_state", "dvp_set_params", "dvp_set_seed", "dvp_set_sampler", "dvp_set_profiling", "dvp_image_format", "dvp_strong_update_form", "dvp_run_patchmatch",
           "dvp_run_stage", "dvp_synchronize", "dvp_download_state", "dvp_download_maps", "dvp_download_maps_begin", "dvp_download_maps_finish", "dvp_buffer_bytes", "dvp_download_buffer",
           "dvp_upload_buffer", "dvp_weak_count", "dvp_get_timings", "dvp_reset_timings", "dvp_eval_cost_vectors",
           "dvp_bench_cost_kernel", "dvp_build_id",
           "dvp_fuse_create", "dvp_fuse_destroy", "dvp_fuse_last_error", "dvp_fuse_set_view", "dvp_fuse_view", "dvp_fuse_view_graded", "dvp_fuse_consistency", "dvp_fuse_count", "dvp_fuse_download", "dvp_fuse_last_rounds",
           "dvp_jpeg_bound", "dvp_jpeg_encode", "dvp_jpeg_last_error", "dvp_preview_begin", "dvp_preview_finish", "dvp_preview_pixels",
           "dvp_canny_edge_map", "dvp_edge_hysteresis", "dvp_edge_last_error", "dvp_edge_map_begin", "dvp_edge_map_finish",
           "dvp_clean_selected_views", "dvp_viewclean_last_error", "dvp_set_view_cleanup",
           "dvp_labels_sizes", "dvp_labels_create", "dvp_labels_destroy", "dvp_labels_run", "dvp_labels_stage", "dvp_labels_timings", "dvp_label_map", "dvp_labels_last_error",
           "dvp_images_create", "dvp_images_destroy", "dvp_images_put", "dvp_images_drop", "dvp_images_size", "dvp_images_bytes", "dvp_images_level", "dvp_images_last_error",
           "dvp_download_image",
           "dvp_jpeg_decode", "dvp_jpeg_decode_into_store", "dvp_jpeg_decode_timings", "dvp_jpeg_decode_last_error",
           "dvp_jpeg_set_entropy", "dvp_jpeg_entropy_stats", "dvp_jpeg_entropy_phases", "dvp_jpeg_scan_records",
           "dvp_plane_prior", "dvp_plane_prior_stage", "dvp_plane_prior_timings",
           "dvp_view_scores", "dvp_convert_image", "dvp_pairs_last_error",
           "dvp_undistort_image", "dvp_undistort_last_error",
           "dvp_cloud_distances", "dvp_cloud_evaluate", "dvp_cloud_last_error",
           "dvp_cloud_prepare", "dvp_cloud_evaluate_prepared", "dvp_cloud_prep_last_error",
           "dvp_cloud_icp_step", "dvp_cloud_refine_alignment", "dvp_cloud_icp_last_error",
           "dvp_cloud_scan_gaps", "dvp_cloud_evaluate_scans", "dvp_cloud_scan_last_error",
           "dvp_mesh_create", "dvp_mesh_destroy", "dvp_mesh_add_view", "dvp_mesh_build", "dvp_mesh_block_count", "dvp_mesh_vertex_count", "dvp_mesh_face_count",
           "dvp_mesh_download", "dvp_mesh_download_volume", "dvp_mesh_set_table", "dvp_mesh_timings", "dvp_mesh_last_error"]
# ... and the one whose name holds a digit (a scan of the header for [a-z_] names does not see it)
EXPORTS_WITH_DIGITS = ["dvp_upload_images_u8"]
PREVIEW_DEPTH, PREVIEW_NORMAL, PREVIEW_WEAK = 1, 2, 4
PRIOR_STAGE_OWNER, PRIOR_STAGE_RATE, PRIOR_STAGE_DEPTH = 0, 1, 2


class DvpTimings(ctypes.Structure):
    _fields_ = [("stage_ms", ctypes.c_double * 13), ("stage_launches", ctypes.c_int32 * 13),
                ("iter_loop_ms", ctypes.c_double), ("total_ms", ctypes.c_double),
                ("ncc_evals", ctypes.c_uint64 * 13)]


def build(force=False):
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU)."""
    args = ["make", "-s", "-C", os.path.join(_HERE, "csrc")]
    if force:
        args.insert(1, "-B")
    subprocess.check_call(args)


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            build()
        L = ctypes.CDLL(_SO)   # raises OSError if the HIP runtime / library is missing
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.dvp_ctx_create.argtypes = [ci, ci, ci, ci, ctypes.POINTER(vp)]
        L.dvp_ctx_destroy.argtypes = [vp]
        L.dvp_ctx_reserve.argtypes = [vp, ci, ci]
        L.dvp_last_error.restype = ctypes.c_char_p
        L.dvp_last_error.argtypes = [vp]
        for n in ("dvp_upload_images", "dvp_upload_depths", "dvp_upload_images_device", "dvp_upload_depths_device"):
            getattr(L, n).argtypes = [vp, vp, ci]
        L.dvp_upload_cameras.argtypes = [vp, vp, ci]
        L.dvp_upload_state.argtypes = [vp] * 7
        L.dvp_upload_state_rescaled.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp]
        L.dvp_reset_state.argtypes = [vp]
        L.dvp_save_state.argtypes = [vp]
        L.dvp_restore_state.argtypes = [vp]
        L.dvp_set_params.argtypes = [vp, vp]
        L.dvp_set_seed.argtypes = [vp, ctypes.c_uint64]
        L.dvp_set_sampler.argtypes = [vp, ci]
        L.dvp_set_profiling.argtypes = [vp, ci]
        L.dvp_image_format.argtypes = [vp]
        L.dvp_strong_update_form.argtypes = [vp]
        L.dvp_run_patchmatch.argtypes = [vp]
        L.dvp_run_stage.argtypes = [vp, ci, ci, ci]
        L.dvp_synchronize.argtypes = [vp]
        L.dvp_download_state.argtypes = [vp] * 5
        L.dvp_download_maps.argtypes = [vp] * 6
        L.dvp_download_maps_begin.argtypes = [vp, vp]
        L.dvp_download_maps_finish.argtypes = [vp] * 6
        L.dvp_buffer_bytes.restype = ctypes.c_longlong
        L.dvp_buffer_bytes.argtypes = [vp, ci]
        L.dvp_download_buffer.argtypes = [vp, ci, vp]
        L.dvp_upload_buffer.argtypes = [vp, ci, vp]
        L.dvp_weak_count.argtypes = [vp]
        L.dvp_get_timings.argtypes = [vp, ctypes.POINTER(DvpTimings)]
        L.dvp_reset_timings.argtypes = [vp]
        L.dvp_eval_cost_vectors.argtypes = [vp, vp, vp, ci, vp, ctypes.POINTER(ctypes.c_float)]
        L.dvp_build_id.restype = ctypes.c_char_p
        L.dvp_build_id.argtypes = []
        L.dvp_bench_cost_kernel.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint64)]
        ll = ctypes.c_longlong
        L.dvp_jpeg_bound.restype = ll
        L.dvp_jpeg_bound.argtypes = [ci, ci, ci]
        L.dvp_jpeg_encode.argtypes = [ci, vp, ci, ci, ci, ll, ci, ci, vp, ll, ctypes.POINTER(ll)]
        L.dvp_jpeg_last_error.restype = ctypes.c_char_p
        L.dvp_jpeg_last_error.argtypes = []
        L.dvp_preview_begin.argtypes = [vp, ci, ci]
        L.dvp_preview_finish.argtypes = [vp, ci, vp, ll, ctypes.POINTER(ll)]
        L.dvp_preview_pixels.argtypes = [vp, ci, vp]
        L.dvp_canny_edge_map.argtypes = [ci, vp, ci, ci, ll, vp]
        L.dvp_edge_hysteresis.argtypes = [ci, vp, ci, ci, vp]
        L.dvp_edge_last_error.restype = ctypes.c_char_p
        L.dvp_edge_last_error.argtypes = []
        L.dvp_edge_map_begin.argtypes = [vp, ci]
        L.dvp_edge_map_finish.argtypes = [vp, vp]
        L.dvp_clean_selected_views.argtypes = [ci, vp, ci, ci, ci, ci, vp]
        L.dvp_viewclean_last_error.restype = ctypes.c_char_p
        L.dvp_viewclean_last_error.argtypes = []
        L.dvp_set_view_cleanup.argtypes = [vp, ci, ci, ci]
        pi = ctypes.POINTER(ci)
        L.dvp_labels_sizes.argtypes = [ci, ci, ci, pi, pi, pi, pi, pi]
        L.dvp_labels_create.argtypes = [ci, ctypes.POINTER(vp)]
        L.dvp_labels_destroy.argtypes = [vp]
        L.dvp_labels_run.argtypes = [vp, vp, ci, ci, ll, ci, vp]
        L.dvp_labels_stage.argtypes = [vp, ci, vp]
        L.dvp_labels_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ll)]
        L.dvp_label_map.argtypes = [ci, vp, ci, ci, ll, ci, vp]
        L.dvp_labels_last_error.restype = ctypes.c_char_p
        L.dvp_labels_last_error.argtypes = []
        L.dvp_images_create.argtypes = [ci, ctypes.POINTER(vp)]
        L.dvp_images_destroy.argtypes = [vp]
        L.dvp_images_put.argtypes = [vp, ci, vp, ci, ci, ll]
        L.dvp_images_drop.argtypes = [vp, ci]
        L.dvp_images_size.argtypes = [vp, ci, pi, pi]
        L.dvp_images_bytes.restype = ll
        L.dvp_images_bytes.argtypes = [vp]
        L.dvp_images_level.argtypes = [vp, ci, ci, ci, ci, ci, vp]
        L.dvp_images_last_error.restype = ctypes.c_char_p
        L.dvp_images_last_error.argtypes = []
        L.dvp_jpeg_decode.argtypes = [ci, vp, ll, ci, vp, ll, pi, pi]
        L.dvp_jpeg_decode_into_store.argtypes = [vp, ci, vp, ll, vp, ll]
        L.dvp_jpeg_decode_timings.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ll)]
        L.dvp_jpeg_decode_last_error.restype = ctypes.c_char_p
        L.dvp_jpeg_decode_last_error.argtypes = []
        L.dvp_jpeg_set_entropy.restype = None
        L.dvp_jpeg_set_entropy.argtypes = [ci]
        L.dvp_jpeg_entropy_stats.argtypes = [ctypes.POINTER(ll)]
        L.dvp_jpeg_entropy_phases.argtypes = [ctypes.POINTER(ctypes.c_double)]
        L.dvp_jpeg_scan_records.argtypes = [ci, vp, ll, ci, ci, pi, ctypes.POINTER(ll), ctypes.POINTER(ll), ctypes.POINTER(vp), ctypes.POINTER(vp)]
        L.dvp_upload_images_u8.argtypes = [vp, vp, vp, ci, ci]
        L.dvp_download_image.argtypes = [vp, ci, vp, ci]
        L.dvp_plane_prior.argtypes = [vp, vp, ci, ci, vp, vp, ci, vp, pi]
        L.dvp_plane_prior_stage.argtypes = [vp, ci, vp]
        L.dvp_plane_prior_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ll)]
        L.dvp_view_scores.argtypes = [ci, ci, vp, vp, vp, ll, vp, vp, vp]
        L.dvp_convert_image.argtypes = [ci, vp, ci, ci, ll, ci, ci, ci, ci, vp]
        L.dvp_pairs_last_error.restype = ctypes.c_char_p
        L.dvp_pairs_last_error.argtypes = []
        L.dvp_undistort_image.argtypes = [ci, vp, ci, ci, ll, ci, vp, ci, vp]
        L.dvp_undistort_last_error.restype = ctypes.c_char_p
        L.dvp_undistort_last_error.argtypes = []
        L.dvp_cloud_distances.argtypes = [ci, vp, ll, vp, ll, ctypes.c_float, vp]
        L.dvp_cloud_evaluate.argtypes = [ci, vp, ll, vp, ll, vp, ci, vp, vp, vp, vp, vp]
        L.dvp_cloud_last_error.restype = ctypes.c_char_p
        L.dvp_cloud_last_error.argtypes = []
        L.dvp_cloud_prepare.argtypes = [ci, vp, ll, vp, vp, vp, vp]
        L.dvp_cloud_evaluate_prepared.argtypes = [ci, vp, ll, vp, vp, ll, vp, vp, ci, vp, vp, vp, vp, vp, vp]
        L.dvp_cloud_prep_last_error.restype = ctypes.c_char_p
        L.dvp_cloud_prep_last_error.argtypes = []
        L.dvp_cloud_icp_step.argtypes = [ci, vp, ll, vp, ll, vp, ctypes.c_float, vp, vp, vp, vp]
        L.dvp_cloud_refine_alignment.argtypes = [ci, vp, ll, vp, ll, vp, vp, vp, ci, vp, vp, ci, vp]
        L.dvp_cloud_icp_last_error.restype = ctypes.c_char_p
        L.dvp_cloud_icp_last_error.argtypes = []
        L.dvp_cloud_scan_gaps.argtypes = [ci, vp, ci, ci, vp, ll, vp, vp, vp]
        L.dvp_cloud_evaluate_scans.argtypes = [ci, vp, ll, vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp]
        L.dvp_cloud_scan_last_error.restype = ctypes.c_char_p
        L.dvp_cloud_scan_last_error.argtypes = []
        L.dvp_fuse_consistency.argtypes = [vp, ci, vp, ci, ci, vp]
        L.dvp_mesh_create.argtypes = [ci, ctypes.c_float, ctypes.c_float, ci, ctypes.POINTER(vp)]
        L.dvp_mesh_destroy.argtypes = [vp]
        L.dvp_mesh_add_view.argtypes = [vp, vp, ci, ci, vp, vp, vp]
        L.dvp_mesh_build.argtypes = [vp]
        for n in ("dvp_mesh_block_count", "dvp_mesh_vertex_count", "dvp_mesh_face_count"):
            getattr(L, n).restype = ll
            getattr(L, n).argtypes = [vp]
        L.dvp_mesh_download.argtypes = [vp, vp, vp, vp]
        L.dvp_mesh_download_volume.argtypes = [vp, vp, vp, vp, vp]
        L.dvp_mesh_set_table.argtypes = [vp, ll]
        L.dvp_mesh_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ll), ctypes.POINTER(ll)]
        L.dvp_mesh_last_error.restype = ctypes.c_char_p
        L.dvp_mesh_last_error.argtypes = []
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


class DvpError(RuntimeError):
    pass


def jpeg_encode(pixels, quality=95, restart=0, device=0):
    """baseline JPEG of a (H, W) grey or (H, W, 3) BGR uint8 image, encoded on the GPU (include/dvp_mvs.h dvp_jpeg_encode);
    restart = MCUs per restart interval, 0 = the engine's choice"""
    L = lib()
    a = np.asarray(pixels)
    assert a.dtype == np.uint8 and a.ndim in (2, 3) and (a.ndim == 2 or a.shape[2] == 3), (a.dtype, a.shape)
    if a.strides[-1] != 1 or (a.ndim == 3 and a.strides[1] != 3):
        a = np.ascontiguousarray(a)
    H, W = a.shape[:2]
    C = 1 if a.ndim == 2 else 3
    cap = L.dvp_jpeg_bound(W, H, C)
    if cap < 0:
        raise DvpError("dvp_jpeg_bound: bad geometry %dx%dx%d" % (W, H, C))
    dst = np.empty(cap, np.uint8)
    n = ctypes.c_longlong(0)
    if L.dvp_jpeg_encode(device, _p(a), W, H, C, a.strides[0], int(quality), int(restart), _p(dst), cap, ctypes.byref(n)) != 0:
        raise DvpError(L.dvp_jpeg_last_error().decode())
    return dst[:n.value].tobytes()


def view_scores(obs_offsets, obs_point_ids, centres, point_ids, xyz, device=0):
    """the (N, N) uint32 view-selection scores of a COLMAP model, computed on the GPU (include/dvp_mvs.h dvp_view_scores): image i's
    point ids are obs_point_ids[obs_offsets[i]:obs_offsets[i + 1]] (-1 = none), centres (N, 3), the points point_ids (P,) at xyz (P, 3)"""
    L = lib()
    off = np.ascontiguousarray(obs_offsets, np.int64)
    ids = np.ascontiguousarray(obs_point_ids, np.int64)
    c = np.ascontiguousarray(centres, np.float64)
    pid = np.ascontiguousarray(point_ids, np.int64)
    x = np.ascontiguousarray(xyz, np.float64)
    N = off.size - 1
    if N < 1 or c.size != 3 * N or x.size != 3 * pid.size or (N >= 1 and ids.size != off[-1]):
        raise ValueError("view_scores: the arrays' sizes do not fit together")
    out = np.empty((N, N), np.uint32)
    if L.dvp_view_scores(device, N, _p(off), _p(ids) if ids.size else None, _p(c), pid.size, _p(pid) if pid.size else None, _p(x) if pid.size else None, _p(out)) != 0:
        raise DvpError(L.dvp_pairs_last_error().decode())
    return out


def convert_image(bgr, pad_w, pad_h, out_w, out_h, device=0):
    """the (out_h, out_w, 3) picture the COLMAP converter writes from a (H, W, 3) B, G, R uint8 picture: zero padding to pad_w x pad_h,
    then OpenCV's nearest-neighbour resize (include/dvp_mvs.h dvp_convert_image)"""
    L = lib()
    a = np.asarray(bgr)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.strides[2] != 1 or a.strides[1] != 3:
        raise ValueError("convert_image: a (H, W, 3) uint8 picture with dense rows is required")
    out = np.empty((max(int(out_h), 0), max(int(out_w), 0), 3), np.uint8)
    if L.dvp_convert_image(device, _p(a), a.shape[1], a.shape[0], a.strides[0], int(pad_w), int(pad_h), int(out_w), int(out_h), _p(out)) != 0:
        raise DvpError(L.dvp_pairs_last_error().decode())
    return out


def _cloud(points, what):
    a = np.ascontiguousarray(points, np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s: a (N, 3) array of points is required" % what)
    return a


def cloud_distances(query, target, max_distance, device=0):
    """(N,) float32 squared distances from every query point to its nearest target, +inf beyond max_distance, NaN for a query with a
    non-finite coordinate, computed on the GPU (include/dvp_mvs.h dvp_cloud_distances)"""
    L = lib()
    q, t = _cloud(query, "cloud_distances"), _cloud(target, "cloud_distances")
    out = np.empty(len(q), np.float32)
    if L.dvp_cloud_distances(device, _p(q), len(q), _p(t), len(t), float(max_distance), _p(out)) != 0:
        raise DvpError(L.dvp_cloud_last_error().decode())
    return out


def cloud_evaluate(recon, truth, tolerances, device=0, distances=False):
    """dict(within_recon, within_truth: (K,) int64; used: (2,) int64; accuracy, completeness, f1: (K,) float64 fractions) of a
    reconstructed cloud against a ground-truth cloud (include/dvp_mvs.h dvp_cloud_evaluate); distances=True adds d2_recon, d2_truth"""
    L = lib()
    r, t = _cloud(recon, "cloud_evaluate"), _cloud(truth, "cloud_evaluate")
    tol = np.ascontiguousarray(tolerances, np.float32).reshape(-1)
    wr, wt, used = np.zeros(max(tol.size, 1), np.int64), np.zeros(max(tol.size, 1), np.int64), np.zeros(2, np.int64)
    dr = np.empty(len(r), np.float32) if distances else None
    dt = np.empty(len(t), np.float32) if distances else None
    if L.dvp_cloud_evaluate(device, _p(r), len(r), _p(t), len(t), _p(tol), tol.size, _p(wr), _p(wt), _p(used), _p(dr), _p(dt)) != 0:
        raise DvpError(L.dvp_cloud_last_error().decode())
    wr, wt = wr[:tol.size], wt[:tol.size]
    a = wr / used[0] if used[0] else np.zeros(tol.size)
    c = wt / used[1] if used[1] else np.zeros(tol.size)
    with np.errstate(invalid="ignore", divide="ignore"):
        f1 = np.where(a + c > 0, 2 * a * c / (a + c), 0.0)
    out = dict(within_recon=wr, within_truth=wt, used=used, accuracy=a, completeness=c, f1=f1)
    if distances:
        out.update(d2_recon=dr, d2_truth=dt)
    return out


# COLMAP's camera model ids (csrc/dvp_undistort.hpp)
CAMERA_MODELS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4, "OPENCV_FISHEYE": 5, "FULL_OPENCV": 6, "FOV": 7,
                 "SIMPLE_RADIAL_FISHEYE": 8, "RADIAL_FISHEYE": 9, "THIN_PRISM_FISHEYE": 10}


def undistort_image(bgr, model, params, device=0):
    """the (H, W, 3) B, G, R uint8 picture resampled into the pinhole camera with its COLMAP camera's fx, fy, cx, cy and size
    (include/dvp_mvs.h dvp_undistort_image); model: COLMAP's name or id, params: COLMAP's order; rows may be padded"""
    L = lib()
    a = np.asarray(bgr)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.strides[2] != 1 or a.strides[1] != 3:
        raise ValueError("undistort_image: a (H, W, 3) uint8 picture with dense pixels is required")
    p = np.ascontiguousarray(params, np.float64).reshape(-1)
    out = np.empty((a.shape[0], a.shape[1], 3), np.uint8)
    if L.dvp_undistort_image(device, _p(a), a.shape[1], a.shape[0], a.strides[0], CAMERA_MODELS.get(model, model), _p(p), p.size, _p(out)) != 0:
        raise DvpError(L.dvp_undistort_last_error().decode())
    return out


def _file_bytes(file):
    return np.frombuffer(bytes(file), np.uint8)


def jpeg_size(file, channels=1):
    """(width, height) of a JPEG file's bytes from its frame header (dvp_jpeg_decode with no output: nothing runs on the device)"""
    L = lib()
    f = _file_bytes(file)
    w, h = ctypes.c_int(0), ctypes.c_int(0)
    if L.dvp_jpeg_decode(0, _p(f) if f.size else None, f.size, int(channels), None, 0, ctypes.byref(w), ctypes.byref(h)) != 0:
        raise DvpError(L.dvp_jpeg_decode_last_error().decode())
    return w.value, h.value


def jpeg_decode(file, channels=1, device=0):
    """a baseline JPEG file's bytes decoded with the inverse DCT and the colour conversion on the GPU (include/dvp_mvs.h
    dvp_jpeg_decode): the (H, W) uint8 luma plane for channels = 1, the (H, W, 3) B, G, R image for 3"""
    L = lib()
    f = _file_bytes(file)
    W, H = jpeg_size(f, channels)
    out = np.empty((H, W) if channels == 1 else (H, W, 3), np.uint8)
    if L.dvp_jpeg_decode(device, _p(f), f.size, int(channels), _p(out), out.strides[0], None, None) != 0:
        raise DvpError(L.dvp_jpeg_decode_last_error().decode())
    return out


def jpeg_decode_timings():
    """dict(host_ms, device_ms, record_bytes, blocks) of this thread's last jpeg_decode / ImageStore.put_jpeg"""
    ms, n = (ctypes.c_double * 2)(), (ctypes.c_longlong * 2)()
    lib().dvp_jpeg_decode_timings(ms, n)
    return dict(host_ms=ms[0], device_ms=ms[1], record_bytes=int(n[0]), blocks=int(n[1]))


ENTROPY_PATHS = ("host", "device", "fell back")
ENTROPY_PHASES = ("prescan", "upload", "sync", "count", "scans", "write", "reconstruct")


def jpeg_set_entropy(on_device):
    """where the Huffman scan of jpeg_decode / ImageStore.put_jpeg runs from now on, process-wide (dvp_jpeg_set_entropy)"""
    lib().dvp_jpeg_set_entropy(1 if on_device else 0)


def jpeg_entropy_stats():
    """this thread's last decode (dvp_jpeg_entropy_stats): dict(path = host | device | fell back, segments, subsequences, chunks,
    longest_chain, rounds, uploaded_bytes, decodes)"""
    n = (ctypes.c_longlong * 8)()
    lib().dvp_jpeg_entropy_stats(n)
    return dict(path=ENTROPY_PATHS[int(n[0])], segments=int(n[1]), subsequences=int(n[2]), chunks=int(n[3]), longest_chain=int(n[4]), rounds=int(n[5]),
                uploaded_bytes=int(n[6]), decodes=int(n[7]))


def jpeg_entropy_phases():
    """milliseconds per phase of this thread's last device-path decode in a process run with DVP_JPEG_ENTROPY_SERIAL=1"""
    ms = (ctypes.c_double * 7)()
    lib().dvp_jpeg_entropy_phases(ms)
    return dict(zip(ENTROPY_PHASES, (float(v) for v in ms)))


def jpeg_scan_records(file, luma_only=False, on_device=False, device=0):
    """the coefficient records of a JPEG file's scan (dvp_jpeg_scan_records): a list of (offsets, records) uint32 arrays per
    component, None for a component that luma_only leaves out"""
    L = lib()
    f = _file_bytes(file)
    comps = ctypes.c_int(0)
    n_off, n_rec = (ctypes.c_longlong * 3)(), (ctypes.c_longlong * 3)()
    args = (device, _p(f) if f.size else None, f.size, 1 if luma_only else 0, 1 if on_device else 0, ctypes.byref(comps), n_off, n_rec)
    if L.dvp_jpeg_scan_records(*args, None, None) != 0:
        raise DvpError(L.dvp_jpeg_decode_last_error().decode())
    off = [np.empty(int(n_off[i]), np.uint32) for i in range(3)]
    rec = [np.empty(int(n_rec[i]), np.uint32) for i in range(3)]
    po, pr = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in off]), (ctypes.c_void_p * 3)(*[a.ctypes.data for a in rec])
    if L.dvp_jpeg_scan_records(*args, po, pr) != 0:
        raise DvpError(L.dvp_jpeg_decode_last_error().decode())
    return [(off[i], rec[i]) if n_off[i] else None for i in range(comps.value)]


def canny_edge_map(grey, device=0):
    """the depth-edge prior (EdgeSegment mode 0) of a (H, W) uint8 image, computed on the GPU (include/dvp_mvs.h
    dvp_canny_edge_map): (H, W) uint8, 255 = edge"""
    L = lib()
    a = np.asarray(grey)
    assert a.dtype == np.uint8 and a.ndim == 2, (a.dtype, a.shape)
    if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
        a = np.ascontiguousarray(a)
    H, W = a.shape
    out = np.empty((H, W), np.uint8)
    if L.dvp_canny_edge_map(device, _p(a), W, H, a.strides[0], _p(out)) != 0:
        raise DvpError(L.dvp_edge_last_error().decode())
    return out


def edge_hysteresis(map3, device=0):
    """Canny's hysteresis alone on a (H, W) uint8 map of 0 = candidate, 1 = nothing, 2 = strong (dvp_edge_hysteresis):
    (H, W) uint8, 255 = edge, no frame fix-ups"""
    L = lib()
    a = np.ascontiguousarray(map3, np.uint8)
    assert a.ndim == 2, a.shape
    H, W = a.shape
    out = np.empty((H, W), np.uint8)
    if L.dvp_edge_hysteresis(device, _p(a), W, H, _p(out)) != 0:
        raise DvpError(L.dvp_edge_last_error().decode())
    return out


def clean_selected_views(views, num_src, min_region, device=0):
    """ProcessProblem's visibility-mask clean-up of a (H, W) uint32 map of selected-view words, computed on the GPU
    (include/dvp_mvs.h dvp_clean_selected_views): (H, W) uint32"""
    L = lib()
    a = np.ascontiguousarray(views, np.uint32)
    assert a.ndim == 2, a.shape
    H, W = a.shape
    out = np.empty((H, W), np.uint32)
    if L.dvp_clean_selected_views(device, _p(a), W, H, int(num_src), int(min_region), _p(out)) != 0:
        raise DvpError(L.dvp_viewclean_last_error().decode())
    return out


def labels_sizes(width, height, scale):
    """dict(quarter=(rows, cols), level=(rows, cols), weak_tex_num=n) of the label prior (dvp_labels_sizes)"""
    L = lib()
    v = [ctypes.c_int(0) for _ in range(5)]
    if L.dvp_labels_sizes(int(width), int(height), int(scale), *[ctypes.byref(x) for x in v]) != 0:
        raise DvpError(L.dvp_labels_last_error().decode())
    return dict(quarter=(v[1].value, v[0].value), level=(v[3].value, v[2].value), weak_tex_num=v[4].value)


def _grey_rows(grey):
    a = np.asarray(grey)
    assert a.dtype == np.uint8 and a.ndim == 2, (a.dtype, a.shape)
    if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
        a = np.ascontiguousarray(a)
    return a


def label_map(grey, scale, device=0):
    """the label prior (EdgeSegment mode 1) of a full-size (H, W) uint8 image at pyramid level `scale`, computed on the GPU
    (include/dvp_mvs.h dvp_label_map): level-size int32, 0 = textured, -1 = a small flat region, k >= 1 = a flat region"""
    L = lib()
    a = _grey_rows(grey)
    H, W = a.shape
    out = np.empty(labels_sizes(W, H, scale)["level"], np.int32)
    if L.dvp_label_map(device, _p(a), W, H, a.strides[0], int(scale), _p(out)) != 0:
        raise DvpError(L.dvp_labels_last_error().decode())
    return out


class LabelJob:
    """a dvp_labels job: its own stream and device scratch, kept from one image to the next"""
    STAGES = dict(quarter=(0, np.uint8), texture=(1, np.uint8), region=(2, np.int32), lines=(3, np.uint8), resized=(4, np.uint8), cleaned=(5, np.uint8))

    def __init__(self, device=0):
        self.L = lib()
        h = ctypes.c_void_p()
        if self.L.dvp_labels_create(device, ctypes.byref(h)) != 0:
            raise DvpError(self.L.dvp_labels_last_error().decode())
        self.h, self.sizes = h, None

    def close(self):
        if getattr(self, "h", None):
            self.L.dvp_labels_destroy(self.h)
            self.h = None

    __del__ = close

    def run(self, grey, scale):
        a = _grey_rows(grey)
        H, W = a.shape
        sizes = labels_sizes(W, H, scale)
        out = np.empty(sizes["level"], np.int32)
        if self.L.dvp_labels_run(self.h, _p(a), W, H, a.strides[0], int(scale), _p(out)) != 0:
            raise DvpError(self.L.dvp_labels_last_error().decode())
        self.sizes = sizes
        return out

    def stage(self, name):
        """an intermediate map of the last run: quarter, texture, region, lines (quarter size), resized, cleaned (level size)"""
        which, dt = self.STAGES[name]
        shape = self.sizes["level" if which >= 4 else "quarter"] if self.sizes else (1, 1)
        out = np.empty(shape, dt)
        if self.L.dvp_labels_stage(self.h, which, _p(out)) != 0:
            raise DvpError(self.L.dvp_labels_last_error().decode())
        return out

    def timings(self):
        """dict(part_a_ms, host_ms, part_b_ms, regions, outline_points) of the last run"""
        ms, n = (ctypes.c_double * 3)(), (ctypes.c_longlong * 2)()
        if self.L.dvp_labels_timings(self.h, ms, n) != 0:
            raise DvpError(self.L.dvp_labels_last_error().decode())
        return dict(part_a_ms=ms[0], host_ms=ms[1], part_b_ms=ms[2], regions=int(n[0]), outline_points=int(n[1]))


class ImageStore:
    """a dvp_images store: decoded (H, W) uint8 images resident on one device, under integer ids; every pyramid level of
    every image is made from them on the device (include/dvp_mvs.h)"""

    def __init__(self, device=0):
        self.L = lib()
        h = ctypes.c_void_p()
        if self.L.dvp_images_create(device, ctypes.byref(h)) != 0:
            raise DvpError(self.L.dvp_images_last_error().decode())
        self.h = h

    def _ck(self, rc):
        if rc != 0:
            raise DvpError(self.L.dvp_images_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.dvp_images_destroy(self.h)
            self.h = None

    __del__ = close

    def put(self, image_id, grey):
        a = _grey_rows(grey)
        self._ck(self.L.dvp_images_put(self.h, int(image_id), _p(a), a.shape[1], a.shape[0], a.strides[0]))

    def put_jpeg(self, image_id, file, want_plane=False):
        """the luma plane of a JPEG file's bytes reconstructed on the device straight into the slot (dvp_jpeg_decode_into_store);
        want_plane: the (H, W) uint8 plane is copied back and returned"""
        f = _file_bytes(file)
        out = None
        if want_plane:
            W, H = jpeg_size(f, 1)
            out = np.empty((H, W), np.uint8)
        if self.L.dvp_jpeg_decode_into_store(self.h, int(image_id), _p(f) if f.size else None, f.size, _p(out), out.strides[0] if want_plane else 0) != 0:
            raise DvpError(self.L.dvp_jpeg_decode_last_error().decode())
        return out

    def drop(self, image_id):
        self._ck(self.L.dvp_images_drop(self.h, int(image_id)))

    def size(self, image_id):
        """(width, height) of a stored image"""
        w, h = ctypes.c_int(0), ctypes.c_int(0)
        self._ck(self.L.dvp_images_size(self.h, int(image_id), ctypes.byref(w), ctypes.byref(h)))
        return w.value, h.value

    def bytes(self):
        return int(self.L.dvp_images_bytes(self.h))

    def level(self, image_id, level_w, level_h, pad_w=0, pad_h=0):
        """the (level_h, level_w) float32 level of a stored image on a pad_w x pad_h canvas (0: the image's own size)"""
        out = np.empty((max(int(level_h), 0), max(int(level_w), 0)), np.float32)
        self._ck(self.L.dvp_images_level(self.h, int(image_id), int(pad_w), int(pad_h), int(level_w), int(level_h), _p(out)))
        return out


class Context:
    """One reference view on one GPU (dvp_ctx).  Method names follow oracle.oracle.Oracle so the
    parity tests drive both through the same code."""

    def __init__(self, width, height, num_images, device=0):
        self.L = lib()
        self.W, self.H, self.NI = width, height, num_images
        h = ctypes.c_void_p()
        if self.L.dvp_ctx_create(device, width, height, num_images, ctypes.byref(h)) != 0:
            raise DvpError(self.L.dvp_last_error(None).decode())
        self.h = h

    def _ck(self, rc):
        if rc != 0:
            raise DvpError(self.L.dvp_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.dvp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _planes_ptrs(self, imgs):
        arrs = [np.ascontiguousarray(imgs[i], np.float32) for i in range(self.NI)]
        for a in arrs:
            assert a.shape == (self.H, self.W)
        ptrs = (ctypes.c_void_p * self.NI)(*[a.ctypes.data for a in arrs])
        return arrs, ptrs

    def set_images(self, images):
        arrs, ptrs = self._planes_ptrs(images)
        self._ck(self.L.dvp_upload_images(self.h, ptrs, self.W))

    def set_images_u8(self, store, ids, pad_w, pad_h):
        """the levels of the stored images `ids` at the context's size, made on the device (dvp_upload_images_u8)"""
        a = np.ascontiguousarray(ids, np.int32)
        assert a.shape == (self.NI,), a.shape
        self._ck(self.L.dvp_upload_images_u8(self.h, store.h, _p(a), int(pad_w), int(pad_h)))

    def image(self, i):
        """the (H, W) float32 image i the context holds"""
        out = np.empty((self.H, self.W), np.float32)
        self._ck(self.L.dvp_download_image(self.h, int(i), _p(out), self.W))
        return out

    def set_depths(self, depths):
        arrs, ptrs = self._planes_ptrs(depths)
        self._ck(self.L.dvp_upload_depths(self.h, ptrs, self.W))

    def set_images_device(self, dev_ptrs, pitch_floats):
        ptrs = (ctypes.c_void_p * self.NI)(*dev_ptrs)
        self._ck(self.L.dvp_upload_images_device(self.h, ptrs, pitch_floats))

    def set_depths_device(self, dev_ptrs, pitch_floats):
        ptrs = (ctypes.c_void_p * self.NI)(*dev_ptrs)
        self._ck(self.L.dvp_upload_depths_device(self.h, ptrs, pitch_floats))

    def set_cameras(self, cams):
        a = np.ascontiguousarray(cams)
        assert a.dtype.itemsize == 112
        self._ck(self.L.dvp_upload_cameras(self.h, _p(a), len(a)))

    def set_params(self, params):
        a = np.ascontiguousarray(params).reshape(1)
        assert a.dtype.itemsize == 76
        self._ck(self.L.dvp_set_params(self.h, _p(a)))
        self.params = a

    def reserve(self, weak_pixels=0, flags=3):
        """optional buffers ahead of their first use (include/dvp_mvs.h: dvp_ctx_reserve)"""
        self._ck(self.L.dvp_ctx_reserve(self.h, int(weak_pixels), int(flags)))

    def set_seed(self, seed):
        self._ck(self.L.dvp_set_seed(self.h, seed))

    def set_sampler(self, s):
        self._ck(self.L.dvp_set_sampler(self.h, s))

    def set_profiling(self, on):
        self._ck(self.L.dvp_set_profiling(self.h, int(on)))

    def upload_state(self, planes=None, views=None, weak=None, edge=None, label=None, radius=None):
        c = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
        args = [c(planes, np.float32), c(views, np.uint32), c(weak, np.uint8), c(edge, np.uint8), c(label, np.int32), c(radius, np.int32)]
        self._ck(self.L.dvp_upload_state(self.h, *[_p(a) for a in args]))

    def upload_state_rescaled(self, src_w, src_h, depth, normal, views, weak=None, radius=None, radius_fallback=5, edge=None, label=None):
        """the coarser level's maps at their own size, up-sampled on the device (include/dvp_mvs.h)"""
        c = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
        args = [c(depth, np.float32), c(normal, np.float32), c(views, np.uint32), c(weak, np.uint8), c(radius, np.int32)]
        tail = [c(edge, np.uint8), c(label, np.int32)]
        self._ck(self.L.dvp_upload_state_rescaled(self.h, int(src_w), int(src_h), *[_p(a) for a in args], int(radius_fallback), *[_p(a) for a in tail]))

    def reset_state(self):
        self._ck(self.L.dvp_reset_state(self.h))

    def image_format(self):
        """0: float planes, 1: byte planes (8-bit exact image set), 2: binary16 planes (every texel a binary16 value in
        [0, 255], not all integers: down-sampled levels of 8-bit images) — include/dvp_mvs.h dvp_image_format"""
        return int(self.L.dvp_image_format(self.h))

    def strong_update_form(self):
        """the split strong update's decision bracket (4, 6, 8, 10, 12, 16; 32: the streaming kernel of DVP_STRONG_WIDE), 0: a
        monolithic kernel; accounts for the cost buffers once a strong update has tried them — include/dvp_mvs.h
        dvp_strong_update_form"""
        return int(self.L.dvp_strong_update_form(self.h))

    def save_state(self):
        self._ck(self.L.dvp_save_state(self.h))

    def restore_state(self):
        self._ck(self.L.dvp_restore_state(self.h))

    def download_state(self):
        L = self.W * self.H
        planes = np.empty((L, 4), np.float32)
        views = np.empty(L, np.uint32)
        weak = np.empty(L, np.uint8)
        radius = np.empty(L, np.int32)
        self._ck(self.L.dvp_download_state(self.h, _p(planes), _p(views), _p(weak), _p(radius)))
        return planes, views, weak, radius

    def download_maps(self):
        """depth / normal / selected_views / states / radius as the driver stores them (include/dvp_mvs.h)"""
        L = self.W * self.H
        depth = np.empty(L, np.float32)
        normal = np.empty((L, 3), np.float32)
        views = np.empty(L, np.uint32)
        weak = np.empty(L, np.uint8)
        radius = np.empty(L, np.int32)
        self._ck(self.L.dvp_download_maps(self.h, _p(depth), _p(normal), _p(views), _p(weak), _p(radius)))
        return depth, normal, views, weak, radius

    def download_maps_begin(self, depth_device_copy=None):
        """first step of download_maps: the maps are staged on the device (and the depth map copied to the device address
        `depth_device_copy`, if given); the context may be reset / uploaded to / run again before download_maps_finish"""
        self._ck(self.L.dvp_download_maps_begin(self.h, ctypes.c_void_p(depth_device_copy) if depth_device_copy else None))

    def download_maps_finish(self):
        """second step (any thread): the staged maps -> host"""
        L = self.W * self.H
        depth = np.empty(L, np.float32)
        normal = np.empty((L, 3), np.float32)
        views = np.empty(L, np.uint32)
        weak = np.empty(L, np.uint8)
        radius = np.empty(L, np.int32)
        self._ck(self.L.dvp_download_maps_finish(self.h, _p(depth), _p(normal), _p(views), _p(weak), _p(radius)))
        return depth, normal, views, weak, radius

    def preview_begin(self, kinds=PREVIEW_DEPTH | PREVIEW_NORMAL | PREVIEW_WEAK, quality=95):
        """render + encode the previews of the current planes / weak map on the device (include/dvp_mvs.h dvp_preview_begin)"""
        self._ck(self.L.dvp_preview_begin(self.h, int(kinds), int(quality)))

    def preview_finish(self, kind):
        """the JPEG file of one begun preview kind (PREVIEW_DEPTH / _NORMAL / _WEAK)"""
        n = ctypes.c_longlong(0)
        self.L.dvp_preview_finish(self.h, int(kind), None, 0, ctypes.byref(n))   # size query (fails on the capacity)
        if n.value <= 0:
            raise DvpError(self.L.dvp_last_error(self.h).decode())
        dst = np.empty(n.value, np.uint8)
        self._ck(self.L.dvp_preview_finish(self.h, int(kind), _p(dst), n.value, ctypes.byref(n)))
        return dst.tobytes()

    def preview_pixels(self, kind):
        """the rendered BGR image of one begun preview kind, (H, W, 3) uint8"""
        out = np.empty((self.H, self.W, 3), np.uint8)
        self._ck(self.L.dvp_preview_pixels(self.h, int(kind), _p(out)))
        return out

    def set_view_cleanup(self, enable, num_src=0, min_region=0):
        """while on, download_maps (begin) hands out the selected-view words after the visibility-mask clean-up"""
        self._ck(self.L.dvp_set_view_cleanup(self.h, int(bool(enable)), int(num_src), int(min_region)))

    def edge_map_begin(self, install=True):
        """the Canny edge prior of image 0 on the context's stream; install: also into the context's edge buffer"""
        self._ck(self.L.dvp_edge_map_begin(self.h, int(bool(install))))

    def edge_map_finish(self):
        """the oldest begun edge map not fetched yet, (H, W) uint8 (any thread)"""
        out = np.empty((self.H, self.W), np.uint8)
        self._ck(self.L.dvp_edge_map_finish(self.h, _p(out)))
        return out

    def plane_prior(self, dep_raw, xy, xyz, file_camera):
        """the FIRST_INIT plane prior into the context's planes (include/dvp_mvs.h dvp_plane_prior): dep_raw (rows, cols) float32
        as dep/<id>.dmb holds it, xy (n, 2) / xyz (n, 3) the sparse points, file_camera the unscaled camera record; returns the
        status: 0 = planes written, 1 = no usable input, planes untouched"""
        a = np.ascontiguousarray(dep_raw, np.float32)
        assert a.ndim == 2, a.shape
        p2 = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        p3 = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        assert len(p2) == len(p3), (p2.shape, p3.shape)
        cam = np.ascontiguousarray(file_camera).reshape(1)
        assert cam.dtype.itemsize == 112
        status = ctypes.c_int(-1)
        self._ck(self.L.dvp_plane_prior(self.h, _p(a) if a.size else None, a.shape[1], a.shape[0], _p(p2) if len(p2) else None, _p(p3) if len(p3) else None,
                                        len(p2), _p(cam), ctypes.byref(status)))
        if status.value == 0:
            self._prior_shape = a.shape
        return status.value

    def plane_prior_stage(self, which):
        """an intermediate map of the last plane_prior with status 0: PRIOR_STAGE_OWNER (int32) / _RATE (float32) at the dep map's
        size, PRIOR_STAGE_DEPTH (float32) at the context's"""
        shape = (self.H, self.W) if which == PRIOR_STAGE_DEPTH else getattr(self, "_prior_shape", (1, 1))
        out = np.empty(shape, np.int32 if which == PRIOR_STAGE_OWNER else np.float32)
        self._ck(self.L.dvp_plane_prior_stage(self.h, int(which), _p(out)))
        return out

    def plane_prior_timings(self):
        """dict(ms=[host part, uploads, kernels], triangles=n, sweep_rows=n) of the last plane_prior with status 0"""
        ms = (ctypes.c_double * 3)()
        counts = (ctypes.c_longlong * 2)()
        self._ck(self.L.dvp_plane_prior_timings(self.h, ms, counts))
        return dict(ms=list(ms), triangles=int(counts[0]), sweep_rows=int(counts[1]))

    def get(self, name):
        bid, dt, k = BUFFERS[name]
        nbytes = self.L.dvp_buffer_bytes(self.h, bid)
        out = np.empty(nbytes // np.dtype(dt).itemsize, dt)
        self._ck(self.L.dvp_download_buffer(self.h, bid, _p(out)))
        return out.reshape(-1, k) if k > 1 else out

    def set(self, name, arr):
        bid, dt, k = BUFFERS[name]
        a = np.ascontiguousarray(arr, dt)
        assert a.nbytes == self.L.dvp_buffer_bytes(self.h, bid), (name, a.nbytes)
        self._ck(self.L.dvp_upload_buffer(self.h, bid, _p(a)))

    def weak_count(self):
        return self.L.dvp_weak_count(self.h)

    def run_stage(self, name, it=0, colour=0):
        self._ck(self.L.dvp_run_stage(self.h, STAGES[name], it, colour))

    def run_patchmatch(self):
        self._ck(self.L.dvp_run_patchmatch(self.h))

    def synchronize(self):
        self._ck(self.L.dvp_synchronize(self.h))

    def timings(self, reset=False):
        t = DvpTimings()
        self._ck(self.L.dvp_get_timings(self.h, ctypes.byref(t)))
        out = dict(stage_ms={STAGE_NAMES[i]: t.stage_ms[i] for i in range(N_TIMING)},
                   stage_launches={STAGE_NAMES[i]: t.stage_launches[i] for i in range(N_TIMING)},
                   ncc_evals={STAGE_NAMES[i]: t.ncc_evals[i] for i in range(N_TIMING)},
                   iter_loop_ms=t.iter_loop_ms, total_ms=t.total_ms)
        if reset:
            self._ck(self.L.dvp_reset_timings(self.h))
        return out

    def eval_cost_vectors(self, px, planes):
        px = np.ascontiguousarray(px, np.int32)
        planes = np.ascontiguousarray(planes, np.float32)
        n = len(px)
        out = np.empty((n, self.NI - 1), np.float32)
        ms = ctypes.c_float(0)
        self._ck(self.L.dvp_eval_cost_vectors(self.h, _p(px), _p(planes), n, _p(out), ctypes.byref(ms)))
        self.last_kernel_ms = ms.value
        return out

    def bench_cost_kernel(self, repeat=5):
        ms = ctypes.c_float(0)
        ev = ctypes.c_uint64(0)
        self._ck(self.L.dvp_bench_cost_kernel(self.h, repeat, ctypes.byref(ms), ctypes.byref(ev)))
        return ms.value, ev.value


def from_scene(scene, params, seed=1234, sampler=0, depths=None, device=0):
    c = Context(scene["width"], scene["height"], len(scene["cameras"]), device=device)
    c.set_images(scene["images"])
    c.set_cameras(scene["cameras"])
    c.set_params(params)
    c.set_seed(seed)
    c.set_sampler(sampler)
    if depths is not None:
        c.set_depths(depths)
    return c


class DvpCloudPrep(ctypes.Structure):
    _fields_ = [("transform", ctypes.c_void_p), ("crop_axis", ctypes.c_int), ("axis_min", ctypes.c_double), ("axis_max", ctypes.c_double),
                ("polygon_xyz", ctypes.c_void_p), ("num_polygon", ctypes.c_int), ("voxel", ctypes.c_double)]


def _cloud_prep(transform=None, crop=None, voxel=0.0):
    """(DvpCloudPrep, the arrays it points into).  crop = dict(axis=0 | 1 | 2 or "X" | "Y" | "Z", axis_min, axis_max, polygon=(n, 3))"""
    p, keep = DvpCloudPrep(None, -1, 0.0, 0.0, None, 0, float(voxel)), []
    if transform is not None:
        m = np.ascontiguousarray(transform, np.float64).reshape(-1)
        if m.size != 16:
            raise ValueError("a transform holds 16 numbers, got %d" % m.size)
        keep.append(m)
        p.transform = m.ctypes.data
    if crop is not None:
        axis = crop["axis"]
        poly = np.ascontiguousarray(crop["polygon"], np.float64)
        if poly.ndim != 2 or poly.shape[1] != 3:
            raise ValueError("a crop polygon is an (n, 3) array")
        keep.append(poly)
        p.crop_axis = "XYZ".index(axis) if isinstance(axis, str) else int(axis)
        p.axis_min, p.axis_max = float(crop["axis_min"]), float(crop["axis_max"])
        p.polygon_xyz, p.num_polygon = poly.ctypes.data, len(poly)
    return p, keep


def cloud_prepare(xyz, transform=None, crop=None, voxel=0.0, device=0):
    """dict(xyz: (M, 3) float32, first_index: (M,) int64 input index of every output point, counts: (4,) int64 finite, after the
    transform, inside the crop, output) of one cloud prepared on the GPU (include/dvp_mvs.h dvp_cloud_prepare)"""
    L = lib()
    a = _cloud(xyz, "cloud_prepare")
    p, keep = _cloud_prep(transform, crop, voxel)
    out, first, counts = np.empty((len(a), 3), np.float32), np.empty(len(a), np.int64), np.zeros(4, np.int64)
    if L.dvp_cloud_prepare(device, _p(a), len(a), ctypes.byref(p), _p(out), _p(first), _p(counts)) != 0:
        raise DvpError(L.dvp_cloud_prep_last_error().decode())
    return dict(xyz=out[:counts[3]].copy(), first_index=first[:counts[3]].copy(), counts=counts)


def cloud_evaluate_prepared(recon, truth, tolerances, prep_recon=None, prep_truth=None, device=0, distances=False):
    """cloud_evaluate's dict of the two clouds after each has been prepared on the GPU, plus counts: (2, 4) int64; prep_recon /
    prep_truth = dict(transform=, crop=, voxel=) as cloud_prepare takes them (include/dvp_mvs.h dvp_cloud_evaluate_prepared); the
    distances refer to the prepared points"""
    L = lib()
    r, t = _cloud(recon, "cloud_evaluate_prepared"), _cloud(truth, "cloud_evaluate_prepared")
    pr, keep_r = _cloud_prep(**(prep_recon or {}))
    pt, keep_t = _cloud_prep(**(prep_truth or {}))
    tol = np.ascontiguousarray(tolerances, np.float32).reshape(-1)
    wr, wt, used = np.zeros(max(tol.size, 1), np.int64), np.zeros(max(tol.size, 1), np.int64), np.zeros(2, np.int64)
    counts = np.zeros((2, 4), np.int64)
    dr = np.empty(len(r), np.float32) if distances else None
    dt = np.empty(len(t), np.float32) if distances else None
    if L.dvp_cloud_evaluate_prepared(device, _p(r), len(r), ctypes.byref(pr), _p(t), len(t), ctypes.byref(pt), _p(tol), tol.size, _p(wr), _p(wt), _p(used), _p(dr), _p(dt),
                                     _p(counts)) != 0:
        raise DvpError(L.dvp_cloud_prep_last_error().decode())
    wr, wt = wr[:tol.size], wt[:tol.size]
    a = wr / used[0] if used[0] else np.zeros(tol.size)
    c = wt / used[1] if used[1] else np.zeros(tol.size)
    with np.errstate(invalid="ignore", divide="ignore"):
        f1 = np.where(a + c > 0, 2 * a * c / (a + c), 0.0)
    out = dict(within_recon=wr, within_truth=wt, used=used, accuracy=a, completeness=c, f1=f1, counts=counts)
    if distances:
        out.update(d2_recon=dr[:counts[0, 3]].copy(), d2_truth=dt[:counts[1, 3]].copy())
    return out


class DvpCloudScan(ctypes.Structure):
    _fields_ = [("xyz", ctypes.c_void_p), ("num", ctypes.c_longlong), ("transform", ctypes.c_double * 16)]


def _cloud_scans(scans, what):
    """(DvpCloudScan array or None, the point arrays it points into, total points).  A scan is (xyz, transform) - (N, 3) points in
    the scanner's frame, 16 numbers - or (xyz, transform, num) with a count of its own"""
    keep, total = [], 0
    arr = (DvpCloudScan * max(len(scans), 1))()
    for k, scan in enumerate(scans):
        a = _cloud(scan[0], what)
        m = np.ascontiguousarray(scan[1], np.float64).reshape(-1)
        if m.size != 16:
            raise ValueError("a transform holds 16 numbers, got %d" % m.size)
        keep.append(a)
        arr[k].xyz, arr[k].num = a.ctypes.data, (len(a) if len(scan) < 3 else int(scan[2]))
        arr[k].transform[:] = m.tolist()
        total += len(a)
    return arr, keep, total


def cloud_scan_gaps(scans, queries, cube_size=1024, device=0, maps=False, truth=False):
    """dict(gap: (N,) float32 of the queries - the largest distance by which a scan's range map lies behind the point, -inf where no
    scan observes its direction, NaN for a non-finite point) from the scans' cube maps made on the GPU (include/dvp_mvs.h
    dvp_cloud_scan_gaps); maps=True adds maps: (S, 6, R, R) float32 squared ranges, truth=True truth: (sum N_s, 3) float32"""
    L = lib()
    arr, keep, total = _cloud_scans(scans, "cloud_scan_gaps")
    q = _cloud(queries, "cloud_scan_gaps")
    R = int(cube_size)
    gap = np.empty(len(q), np.float32)
    m = np.empty((len(scans), 6, R, R), np.float32) if maps and 0 < R <= 4096 else None
    t = np.empty((total, 3), np.float32) if truth else None
    if L.dvp_cloud_scan_gaps(device, ctypes.byref(arr), len(scans), R, _p(q), len(q), _p(gap), _p(m), _p(t)) != 0:
        raise DvpError(L.dvp_cloud_scan_last_error().decode())
    out = dict(gap=gap)
    if maps:
        out["maps"] = m
    if truth:
        out["truth"] = t
    return out


def cloud_evaluate_scans(recon, scans, tolerances, prep_recon=None, prep_truth=None, cube_size=1024, device=0, distances=False):
    """cloud_evaluate_prepared's dict of a reconstruction against the truth cloud of laser scans, with ETH3D's observed-space accuracy:
    free_space, unobserved: (K,) int64, accuracy = within_recon / (within_recon + free_space), f1 from it and the completeness
    (include/dvp_mvs.h dvp_cloud_evaluate_scans); distances=True adds d2_recon and gap of the prepared reconstructed points"""
    L = lib()
    r = _cloud(recon, "cloud_evaluate_scans")
    arr, keep, total = _cloud_scans(scans, "cloud_evaluate_scans")
    pr, keep_r = _cloud_prep(**(prep_recon or {}))
    pt, keep_t = _cloud_prep(**(prep_truth or {}))
    tol = np.ascontiguousarray(tolerances, np.float32).reshape(-1)
    wr, wt, fs = (np.zeros(max(tol.size, 1), np.int64) for _ in range(3))
    used, counts = np.zeros(2, np.int64), np.zeros((2, 4), np.int64)
    dr = np.empty(len(r), np.float32) if distances else None
    gap = np.empty(len(r), np.float32) if distances else None
    if L.dvp_cloud_evaluate_scans(device, _p(r), len(r), ctypes.byref(pr) if prep_recon is not None else None, ctypes.byref(arr), len(scans),
                                  ctypes.byref(pt) if prep_truth is not None else None, int(cube_size), _p(tol), tol.size, _p(wr), _p(wt), _p(used), _p(fs), _p(counts), _p(dr),
                                  _p(gap)) != 0:
        raise DvpError(L.dvp_cloud_scan_last_error().decode())
    wr, wt, fs = wr[:tol.size], wt[:tol.size], fs[:tol.size]
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(wr + fs > 0, wr / (wr + fs), 0.0)
        c = wt / used[1] if used[1] else np.zeros(tol.size)
        f1 = np.where(a + c > 0, 2 * a * c / (a + c), 0.0)
    out = dict(within_recon=wr, within_truth=wt, used=used, free_space=fs, unobserved=used[0] - wr - fs, accuracy=a, completeness=c, f1=f1, counts=counts)
    if distances:
        out.update(d2_recon=dr[:counts[0, 3]].copy(), gap=gap[:counts[0, 3]].copy())
    return out


class DvpIcpStage(ctypes.Structure):
    _fields_ = [("voxel", ctypes.c_double), ("max_distance", ctypes.c_double), ("max_iterations", ctypes.c_int)]


class DvpIcpLog(ctypes.Structure):
    _fields_ = [("stage", ctypes.c_int), ("step", ctypes.c_int), ("n_src", ctypes.c_longlong), ("n", ctypes.c_longlong), ("rmse", ctypes.c_double)]


def cloud_icp_step(src, tgt, max_distance, increment=None, device=0):
    """dict(nearest: (N,) int32 index of every source's corresponding target or -1, e: (N,) float32 its squared distance or +inf, sums:
    (16,) float64 tree sums of the correspondences, count) of one ICP step on the GPU (include/dvp_mvs.h dvp_cloud_icp_step)"""
    L = lib()
    s, t = _cloud(src, "cloud_icp_step"), _cloud(tgt, "cloud_icp_step")
    D = None if increment is None else np.ascontiguousarray(increment, np.float64).reshape(-1)
    if D is not None and D.size != 16:
        raise ValueError("an increment holds 16 numbers, got %d" % D.size)
    nearest, e, sums, count = np.empty(len(s), np.int32), np.empty(len(s), np.float32), np.zeros(16, np.float64), np.zeros(1, np.int64)
    if L.dvp_cloud_icp_step(device, _p(s), len(s), _p(t), len(t), _p(D), float(max_distance), _p(nearest), _p(e), _p(sums), _p(count)) != 0:
        raise DvpError(L.dvp_cloud_icp_last_error().decode())
    return dict(nearest=nearest, e=e, sums=sums, count=int(count[0]))


def cloud_refine_alignment(recon, truth, stages, transform=None, crop=None, device=0):
    """dict(matrix: (16,) float64 the refined transform of the reconstruction, log: [(stage, step, n_src, n, rmse)]) of the ICP stages
    [(voxel, max_distance, max_iterations), ...] on the GPU, from the initial transform (None: identity), both clouds cropped by crop
    (include/dvp_mvs.h dvp_cloud_refine_alignment)"""
    L = lib()
    r, t = _cloud(recon, "cloud_refine_alignment"), _cloud(truth, "cloud_refine_alignment")
    pr, keep_r = _cloud_prep(transform, crop)
    pt, keep_t = _cloud_prep(None, crop)
    st = (DvpIcpStage * max(len(stages), 1))(*[DvpIcpStage(float(v), float(d), int(k)) for v, d, k in stages])
    capacity = sum(max(int(k), 0) for _, _, k in stages) if len(stages) <= 8 else 0
    log, count, out = (DvpIcpLog * max(capacity, 1))(), ctypes.c_int(0), np.zeros(16, np.float64)
    if L.dvp_cloud_refine_alignment(device, _p(r), len(r), _p(t), len(t), ctypes.byref(pr), ctypes.byref(pt), st, len(stages), _p(out), log, capacity, ctypes.byref(count)) != 0:
        raise DvpError(L.dvp_cloud_icp_last_error().decode())
    return dict(matrix=out, log=[(g.stage, g.step, g.n_src, g.n, g.rmse) for g in log[:min(count.value, capacity)]])


def mesh_build(views, voxel, truncation=None, min_weight=2, device=0, table_slots=None, volume=False, timings=False):
    """dict(vertices: (V, 3) float32, colours: (V, 3) uint8 b g r, faces: (F, 3) int32, blocks) of the TSDF volume and its surface nets
    built on the GPU from views = [(camera record, depth (H, W) float32, mask (H, W) uint8, bgr (H, W, 3) uint8), ...]
    (include/dvp_mvs.h dvp_mesh_*); truncation None = 4 voxels; table_slots = the block table's first size; volume=True adds keys, sf,
    w, colour_sums; timings=True adds ms (allocation, integration, extraction), regrows, bytes"""
    L = lib()
    job = ctypes.c_void_p()
    tau = 4.0 * float(voxel) if truncation is None else float(truncation)
    if L.dvp_mesh_create(device, float(voxel), tau, int(min_weight), ctypes.byref(job)) != 0:
        raise DvpError(L.dvp_mesh_last_error().decode())
    try:
        if table_slots is not None and L.dvp_mesh_set_table(job, int(table_slots)) != 0:
            raise DvpError(L.dvp_mesh_last_error().decode())
        for cam, depth, mask, bgr in views:
            c = np.ascontiguousarray(cam).reshape(1)
            d, m, b = np.ascontiguousarray(depth, np.float32), np.ascontiguousarray(mask, np.uint8), np.ascontiguousarray(bgr, np.uint8)
            if c.itemsize != 112 or d.ndim != 2 or m.shape != d.shape or b.shape != d.shape + (3,):
                raise ValueError("mesh_build: a view is (camera record, depth (H, W), mask (H, W), bgr (H, W, 3))")
            if L.dvp_mesh_add_view(job, _p(c), d.shape[1], d.shape[0], _p(d), _p(m), _p(b)) != 0:
                raise DvpError(L.dvp_mesh_last_error().decode())
        if L.dvp_mesh_build(job) != 0:
            raise DvpError(L.dvp_mesh_last_error().decode())
        nv, nf, nb = L.dvp_mesh_vertex_count(job), L.dvp_mesh_face_count(job), L.dvp_mesh_block_count(job)
        out = dict(vertices=np.empty((nv, 3), np.float32), colours=np.empty((nv, 3), np.uint8), faces=np.empty((nf, 3), np.int32), blocks=nb)
        if L.dvp_mesh_download(job, _p(out["vertices"]), _p(out["colours"]), _p(out["faces"])) != 0:
            raise DvpError(L.dvp_mesh_last_error().decode())
        if volume:
            out.update(keys=np.empty(nb, np.uint64), sf=np.empty((nb, 512), np.float32), w=np.empty((nb, 512), np.int32), colour_sums=np.empty((nb, 512, 4), np.uint32))
            if L.dvp_mesh_download_volume(job, _p(out["keys"]), _p(out["sf"]), _p(out["w"]), _p(out["colour_sums"])) != 0:
                raise DvpError(L.dvp_mesh_last_error().decode())
        if timings:
            ms, regrows, nbytes = (ctypes.c_double * 3)(), ctypes.c_longlong(0), ctypes.c_longlong(0)
            if L.dvp_mesh_timings(job, ms, ctypes.byref(regrows), ctypes.byref(nbytes)) != 0:
                raise DvpError(L.dvp_mesh_last_error().decode())
            out.update(ms=list(ms), regrows=regrows.value, bytes=nbytes.value)
        return out
    finally:
        L.dvp_mesh_destroy(job)
