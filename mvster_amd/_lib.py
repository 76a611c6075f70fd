"""ctypes binding of libmvster_hip.so (C ABI: include/mvster_hip.h).

There is deliberately no fallback: if the shared library is missing, importing
`mvster_amd.ops` on a GPU box fails loudly instead of silently running PyTorch ops.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MVSTER_LIB") or os.path.join(_HERE, "csrc", "libmvster_hip.so")   # env: A/B builds

ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_LAUNCH = -1, -2, -3, -4      # MVSTER_ERR_* of include/mvster_hip.h
ERRORS = {-1: "NULL pointer", -2: "bad shape", -3: "unsupported channel/tile combination", -4: "kernel launch failed"}

_f = ctypes.c_void_p     # device pointers are passed as integers
_i = ctypes.c_int
_l = ctypes.c_long
_fl = ctypes.c_float

SIGNATURES = {
    "mvster_relative_projection": [_f, _f, _i, _i, _f],
    "mvster_relative_projection_multi": [_f, _i, _f, _i, _i, _f],
    "mvster_pack_images": [_f, _i, _f, _i, _i, _i, _f],
    "mvster_pack_images_u8": [_f, _f, _i, _i, _i, _f],
    "mvster_load_pack_images_u8": [_f, _l, _f, _f, _f, _l, _f, _f, _i, _i, _i, _f],
    "mvster_forward_prologue": [_f, _i, _f, _i, _i, _i, _f, _i, _f, _f, _i, _f, _i, _i, _i, _i, _f],
    "mvster_warp_agg_fwd": [_f, _f, _f, _f, _f, _f] + [_i] * 9 + [_l] * 3 + [_i, _i, _fl, _i, _f],
    "mvster_warp_agg_fwd_indexed": [_f, _f, _f, _f, _f, _f] + [_i] * 10 + [_fl, _i, _f],
    "mvster_warp_agg_fwd_counted": [_f, _f, _f, _f, _f, _f] + [_i] * 9 + [_l] * 3 + [_i, _i, _fl, _i, _f, _f],
    "mvster_warp_agg_fwd_indexed_counted": [_f, _f, _f, _f, _f, _f] + [_i] * 10 + [_fl, _i, _f, _f],
    "mvster_gather_views": [_f, _f, _f, _i, _i, _i, _l, _f],
    "mvster_warp_agg_fwd_sched": [_f] * 6 + [_i, _f, _f, _f] + [_i] * 9 + [_l] * 3 + [_i, _fl, _i, _f],
    "mvster_warp_agg_bwd": [_f] * 11 + [_i] * 9 + [_l] * 3 + [_i, _i, _fl, _f],
    "mvster_warp_agg_bwd_scratch": [_i] * 8 + [_f, _f],
    "mvster_warp_agg_bwd_sorted_scratch": [_i] * 8 + [_f, _f],
    "mvster_warp_agg_bwd_sorted": [_f] * 11 + [_i] * 9 + [_l] * 3 + [_i, _i, _fl, _f],
    "mvster_init_range": [_f, _i, _f, _i, _i, _i, _i, _i, _f],
    "mvster_schedule_inverse_range": [_f, _f, _f, _i, _i, _i, _i, _f],
    "mvster_schedule_range": [_f, _f, _f, _i, _i, _i, _i, _f],
    "mvster_select_depth": [_f, _f, _f, _f, _i, _f, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _fl, _f],
    "mvster_select_depth_bwd": [_f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _f],
    "mvster_upsample_bilinear": [_f, _f, _i, _i, _i, _i, _i, _f],
    "mvster_upsample_bilinear_multi": [_f, _f, _f, _f, _i, _i, _i, _i, _f],
    "mvster_conv_mfma": [_f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _i, _f, _i, _i, _i, _i, _f],
    "mvster_conv_small": [_f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _f],
    "mvster_conv_narrow": [_f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _f],
    "mvster_conv_narrow4": [_f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _f],
    "mvster_conv_narrow_pair": [_f, _f, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _f],
    "mvster_conv_narrow_pair_planes": [_f] + [_i] * 4 + [_f] * 7 + [_i] * 3 + [_f, _i, _f, _f, _i, _f] + [_i] * 4 + [_f],
    "mvster_deconv_select": [_f] * 14 + [_i] * 6 + [_fl, _f],
    "mvster_deconv_select_riders": [_f] * 14 + [_i] * 6 + [_fl] + [_f] * 4 + [_i] * 3 + [_f],
    "mvster_deconv_small": [_f, _f, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _f],
    "mvster_fpn_tail_gather": [_f, _f, _f, _f, _i, _i, _i, _i, _f],
    "mvster_fpn_lateral_up": [_f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _f],
    "mvster_fpn_tail_fused": [_f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _f],
    "mvster_fpn_tail_gather_bwd": [_f, _f, _i, _i, _i, _i, _i, _f],
    "mvster_pack_conv_weights": [_f, _f] + [_i] * 6 + [_l] * 5 + [_i, _f],
    "mvster_pack_wino_weights": [_f, _f, _i, _i, _i, _i, _l, _l, _l, _l, _l, _i, _f],
    "mvster_pack_wino_batch": [_f, _i, _i, _f],
    "mvster_pack_conv_weights_classes": [_f, _f, _i, _i, _i, _i, _i, _f, _f, _f, _f],
    "mvster_conv_wgrad": [_f, _f, _f] + [_i] * 20 + [_f],
    "mvster_conv_wgrad_slots": [_i] * 12,
    "mvster_bn_relu_fwd": [_f, _f, _f, _f, _f, _l, _i, _i, _i, _f],
    "mvster_conv_wgrad_finish": [_f, _f] + [_i] * 10 + [_f],
    "mvster_bn_slots": [_l, _i, _i],
    "mvster_col_sum": [_f, _f, _f, _f, _l, _i, _f],
    "mvster_bn_train_slots": [_l, _i, _i],
    "mvster_bn_train_fwd": [_f] * 10 + [_l, _i, _i, _i, _fl, _fl, _f],
    "mvster_bn_train_bwd": [_f] * 7 + [_l, _i, _i, _i, _f],
    "mvster_conv_wgrad_finish_batch": [_f, _i, _f],
    "mvster_bn_relu_bwd_reduce": [_f] * 11 + [_l, _i, _i, _i, _f],
    "mvster_bn_relu_bwd_apply": [_f] * 8 + [_l, _i, _i, _i, _i, _f],
    "mvster_upsample2x_cl_fwd": [_f, _f, _i, _i, _i, _i, _f],
    "mvster_upsample2x_cl_bwd": [_f, _f, _i, _i, _i, _i, _f],
    "mvster_upsample2x_nearest_cl": [_f, _f, _i, _i, _i, _i, _i, _f],
    "mvster_sinkhorn": [_f, _f, _f, _f, _f, _i, _i, _l, _i, _fl, _f],
    "mvster_sinkhorn_continuous": [_f, _f, _f, _f, _f, _f, _i, _i, _l, _i, _fl, _f],
    "mvster_stage_loss_terms": [_f, _f, _f, _f, _f, _f, _i, _i, _l, _i, _f],
    "mvster_stage_loss_slots": [_l],
    "mvster_stage_loss_fwd": [_f] * 9 + [_i, _i, _l, _i, _fl, _fl, _fl, _f],
    "mvster_stage_loss_bwd": [_f] * 6 + [_fl, _fl, _f, _f, _i, _i, _l, _f],
    "mvster_mono_depth_fwd": [_f] * 5 + [_i, _l, _f],
    "mvster_mono_depth_bwd": [_f] * 6 + [_i, _l, _f],
    "mvster_upcat_fwd": [_f, _f, _f, _i, _i, _i, _i, _i, _f],
    "mvster_upcat_bwd": [_f, _f, _f, _i, _i, _i, _i, _i, _f],
    "mvster_fine_weights_fwd": [_f] * 6 + [_i, _i, _i, _f],
    "mvster_fine_weights_bwd": [_f] * 9 + [_i, _i, _i, _f],
    "mvster_fused_adam": [_f, _f, _f, _f, _i, _f, _f, _f, _f] + [ctypes.c_double] * 4 + [_f],
    "mvster_geo_filter": [_f] * 10 + [_i, _i, _i, _fl, _fl, _f],
    "mvster_geo_scene_blocks": [_i, _i, _i],
    "mvster_geo_scene_filter": [_f] * 13 + [_i] * 5 + [_fl, _i, _fl, _fl, _f],
    "mvster_geo_scene_filter_dynamic": [_f] * 14 + [_i] * 5 + [_fl, _i, _fl, _fl, _f],
    "mvster_geo_scene_emit": [_f] * 5 + [_i, _f, _f, _f, _l, _i, _i, _i, _i, _f],
    "mvster_voxel_thin_blocks": [_l],
    "mvster_voxel_thin_insert": [_f, _l, _fl, _f, _f, _l, _f, _f, _f, _f],
    "mvster_voxel_thin_emit": [_f, _f, _l, _fl, _i] + [_f] * 8 + [_l, _f],
    "mvster_cloud_grid_build": [_f, _l, _f, _f, _f, _f, _f, _f, _l, _f, _f],
    "mvster_cloud_nn_query": [_f, _f, _f, _l, _f, _f, _l, _f, _f, _l, _l, _fl, _fl, _f, _f, _f, _f],
    "mvster_cloud_score_slots": [_l],
    "mvster_cloud_score": [_f, _l, _fl, _fl, _f, _f, _f],
    "mvster_eval_reduce_init": [_f, _l, _fl, _f, _f, _f],
    "mvster_eval_reduce_rounds": [_f, _l, _f, _f, _l, _f, _l, _fl, _i, _f, _l, _l, _f, _f, _i, _f],
    "mvster_eval_flags": [_f, _l, _f, _l, _l, _l, _f, _i, _f, _f, _f],
    "mvster_eval_stats_slots": [_l],
    "mvster_eval_stats": [_f, _f, _l, _i, _fl, _f, _f, _f, _f, _f],
    "mvster_reg_blocks": [_l],
    "mvster_reg_transform": [_f, _l, _f, _f, _f],
    "mvster_reg_crop_flags": [_f, _l, _f, _f, _i, _i, _i, _f, _f, _f, _f],
    "mvster_reg_crop_emit": [_f, _f, _l, _f, _f, _f, _l, _i, _f, _f, _f, _f],
    "mvster_reg_sum_rows": [_l],
    "mvster_reg_sums": [_f, _f, _f, _l, _f, _l, _f, _f, _f],
    "mvster_reg_histogram": [_f, _l, _f, _i, _f, _f],
    "mvster_cloud_knn_query": [_f, _f, _f, _l, _f, _f, _l, _f, _f, _l, _l, _fl, _fl, _i, _i, _l, _f, _f, _f, _f],
    "mvster_cloud_knn_mean": [_f, _f, _l, _f, _f, _l, _f, _l, _l, _fl, _fl, _i, _f, _f, _f],
    "mvster_cloud_knn_normals": [_f, _f, _l, _f, _f, _l, _f, _l, _l, _fl, _fl, _i, _f, _f, _f, _f, _f],
    "mvster_cloud_radius_count": [_f, _f, _l, _f, _f, _l, _f, _l, _l, _fl, _fl, _f, _f],
    "mvster_cloud_knn_stats_rows": [_l],
    "mvster_cloud_knn_stats": [_f, _l, ctypes.c_double, _f, _f, _f],
    "mvster_cloud_keep_flags": [_f, _f, _i, _f, _f, _l, _f, _f, _f, _f],
    "mvster_sfm_pair_scores": [_f, _i, _f, _l, _f, _f, _l, _f, _l] + [ctypes.c_double] * 3 + [_f, _f],
    "mvster_sfm_depth_ranges": [_f, _i, _f, _l, _f, _f, _l, _f, _f, _f, _f],
    "mvster_sfm_select_sources": [_f, _i, _i, _f, _f, _f, _f],
    "mvster_undistort_cameras": [_f, _i] + [ctypes.c_double] * 3 + [_i] + [ctypes.c_double] * 2 + [_f, _f],
    "mvster_undistort_points": [_f, _i, _f, _l, _i, _f, _f, _f, _f],
    "mvster_undistort_images": [_f, _l, _f, _l, _f, _l, _f, _f, _i, _l, _f, _f, _i, _f],
    "mvster_mesh_blocks": [_l],
    "mvster_tsdf_integrate": [_f, _f, _f, _f, _i, _i, _i] + [ctypes.c_double] * 4 + [_i, _i, _i, ctypes.c_double, _f, _f, _f, _f, _f],
    "mvster_mesh_count": [_f, _f, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f],
    "mvster_mesh_emit_vertices": [_f, _f, _f] + [ctypes.c_double] * 4 + [_i, _i, _i, _f, _f, _f, _l, _f, _f, _f],
    "mvster_mesh_emit_triangles": [_f, _f, _i, _i, _i, _i, _f, _f, _f, _f, _l, _l, _f, _f],
    "mvster_tsdf_sparse_bricks": [_i, _i, _i],
    "mvster_tsdf_sparse_mark": [_f, _f, _f, _i, _i, _i] + [ctypes.c_double] * 4 + [_i, _i, _i, ctypes.c_double, _f, _f],
    "mvster_tsdf_sparse_compact_count": [_f, _l, _f, _f, _f],
    "mvster_tsdf_sparse_compact_emit": [_f, _l, _f, _l, _f, _f, _f],
    "mvster_tsdf_sparse_integrate": [_f, _f, _f, _f, _i, _i, _i] + [ctypes.c_double] * 4 + [_i, _i, _i, ctypes.c_double, _f, _l] + [_f] * 5,
    "mvster_mesh_sparse_count": [_f, _f, _f, _f, _l, _i, _i, _i, _i] + [_f] * 7,
    "mvster_mesh_sparse_emit_vertices": [_f] * 6 + [_l] + [ctypes.c_double] * 4 + [_i, _i, _i, _f, _f, _f, _l, _f, _f, _f, _f],
    "mvster_mesh_sparse_emit_triangles": [_f, _f, _f, _f, _l, _i, _i, _i, _i, _f, _f, _f, _f, _l, _l, _f, _f],
    "mvster_mesh_clean_work": [_l, _l, _f, _f],
    "mvster_mesh_clean_plan": [_f, _f, _l, _l, _i, _l, _i, _f, _l] + [_f] * 7 + [_l, _f, _f, _f],
    "mvster_mesh_normals_blocks": [_l],
    "mvster_mesh_clean_emit": [_f, _f, _f, _l, _l, _f, _f, _l, _l] + [_f] * 6,
    "mvster_mesh_vertex_normals": [_f, _f, _l, _l] + [_f] * 6,
    "mvster_depth_metrics_slots": [_l],
    "mvster_depth_metrics": [_f] * 5 + [_i, _i, _l, _f, _f, _f, _f],
    "mvster_pooled_metrics": [_f] * 5 + [_i, _i, _l, _f, _f, _f, _f],
    "mvster_scalar_accumulate": [_f, _i, _f, _f, _f],
    "mvster_scalar_gather_accumulate": [_f, _i, _f, _f, _f, _f],
    "mvster_scalar_reset": [_f, _i, _f, _f],
    "mvster_mfma_probe": [_f, _f, _f, _f],
    "mvster_gather_batch": [_f, _i, _i, _f],
    "mvster_last_kernel": [],
    "mvster_build_flags": [],
}
RESTYPES = {"mvster_last_kernel": ctypes.c_char_p}     # everything else returns an int status

_lib = None


def load():
    """Load the library once; raise with build instructions if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "mvster_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no PyTorch fallback for the HIP path." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        lax = bool(os.environ.get("MVSTER_LIB")) and bool(os.environ.get("MVSTER_LIB_LAX"))   # A/B against an older build
        for name, argtypes in SIGNATURES.items():
            if lax and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)        # AttributeError if the library does not export it
            fn.argtypes = argtypes
            fn.restype = RESTYPES.get(name, ctypes.c_int)
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s (code %d)" % (what, ERRORS.get(rc, "unknown error"), rc))


def has_probes():
    """True when the loaded library is the probe build (experiment switches, kernel forms kept for the record)."""
    lib = load()
    return hasattr(lib, "mvster_build_flags") and bool(lib.mvster_build_flags() & 1)


def last_kernel():
    """Kernel name (profiler spelling) the most recent convolution / fused-warp launch of this thread dispatched."""
    return load().mvster_last_kernel().decode()
