"""ctypes binding of libvkunet.so (the C ABI declared in include/vk_unet.h).

There is no CPU / eager fallback anywhere in this package: if the shared library is missing or does
not load, importing the compute entry points raises."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["VK_LIB"]) if os.environ.get("VK_LIB") else PKG_DIR / "libvkunet.so"   # VK_LIB: diagnostic builds
CSRC = PKG_DIR / "csrc"

VK_F32, VK_BF16, VK_F16 = 0, 1, 2
VK_LOSS_BINARY, VK_LOSS_MULTILABEL, VK_LOSS_MULTICLASS = 0, 1, 2
VK_ENC_RESNET18, VK_ENC_RESNET34, VK_ENC_RESNET50 = 18, 34, 50
VK_ADAMW_MAX_GROUPS = 8
VK_NORM_L2, VK_NORM_INF = 0, 1
VK_TILE_MAX_ORIGINS, VK_TILE_MAX_SIDE = 64, 4096
VK_BLEND_PROB, VK_BLEND_LOGIT = 0, 1
VK_PATCH_FORCE_GENERAL = 1


class VkError(RuntimeError):
    pass


class vk_src(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("C", C.c_int), ("up", C.c_int), ("scale", C.c_void_p),
                ("shift", C.c_void_p), ("relu", C.c_int)]


class vk_conv_desc(C.Structure):
    _fields_ = [("dtype", C.c_int), ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Ho", C.c_int),
                ("Wo", C.c_int), ("K", C.c_int), ("R", C.c_int), ("S", C.c_int), ("stride", C.c_int),
                ("pad", C.c_int), ("transposed", C.c_int), ("src0", vk_src), ("src1", vk_src)]


class vk_bnr(C.Structure):
    _fields_ = [("z", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p), ("sums", C.c_void_p), ("mask", C.c_void_p),
                ("accumulate", C.c_int)]


class vk_letterbox_desc(C.Structure):
    _fields_ = [("h", C.c_int), ("w", C.c_int), ("src_stride", C.c_int), ("size", C.c_int), ("nh", C.c_int),
                ("nw", C.c_int), ("top", C.c_int), ("left", C.c_int), ("pad_value", C.c_int)]


class vk_tile_desc(C.Structure):
    _fields_ = [("h", C.c_int), ("w", C.c_int), ("src_stride", C.c_int), ("T", C.c_int), ("overlap", C.c_int), ("ny", C.c_int),
                ("nx", C.c_int), ("ys", C.c_int * VK_TILE_MAX_ORIGINS), ("xs", C.c_int * VK_TILE_MAX_ORIGINS), ("view_mask", C.c_int),
                ("pad_value", C.c_int), ("C", C.c_int)]


class vk_geom_desc(C.Structure):
    _fields_ = [("h", C.c_int), ("w", C.c_int), ("bin_thresh", C.c_float), ("morph_kernel", C.c_int), ("open_iter", C.c_int),
                ("close_iter", C.c_int), ("min_area", C.c_int), ("max_components", C.c_int)]


class vk_geom_det(C.Structure):
    _fields_ = [("label", C.c_int), ("area", C.c_int), ("box", C.c_int * 8), ("cx", C.c_float), ("cy", C.c_float),
                ("rw", C.c_float), ("rh", C.c_float), ("ux", C.c_float), ("uy", C.c_float), ("hull_n", C.c_int),
                ("reserved", C.c_int), ("d1", C.c_double), ("d2", C.c_double), ("d_mean", C.c_double)]


class vk_geom_quad(C.Structure):
    _fields_ = [("label", C.c_int), ("area", C.c_int), ("box", C.c_int * 8), ("cx", C.c_float), ("cy", C.c_float),
                ("valid", C.c_int), ("branch", C.c_int), ("n_candidates", C.c_int), ("contour_n", C.c_int), ("hull_n", C.c_int),
                ("flags", C.c_int), ("quality", C.c_double), ("d1", C.c_double), ("d2", C.c_double), ("d_mean", C.c_double)]


class vk_aug_params(C.Structure):
    _fields_ = [("d4", C.c_int), ("rotate", C.c_int), ("cos_a", C.c_float), ("sin_a", C.c_float), ("photo", C.c_int),
                ("alpha", C.c_float), ("beta", C.c_float), ("blur_ksize", C.c_int), ("noise_scale", C.c_float),
                ("noise_seed", C.c_uint32), ("clahe_limit", C.c_int)]


class vk_patch_item(C.Structure):
    _fields_ = [("img_off", C.c_int64), ("msk_off", C.c_int64), ("h", C.c_int), ("w", C.c_int), ("row_off", C.c_int64)]


class vk_patch_params(C.Structure):
    _fields_ = [("item", C.c_int), ("k", C.c_int), ("oy", C.c_int), ("ox", C.c_int), ("zoom", C.c_float), ("cos_a", C.c_float),
                ("sin_a", C.c_float), ("reserved", C.c_int)]


VK_CP_MAX_PASTES, VK_CP_MAX_SLOTS, VK_CP_MAX_SIDE = 8, 256, 4096
CP_REC_FIELDS = ("donor", "sx0", "sy0", "sw", "sh", "d4", "dx0", "dy0", "dw", "dh")


class vk_cp_rec(C.Structure):
    _fields_ = [(f, C.c_int32) for f in CP_REC_FIELDS]


def vk_cp_recs_dev_bytes(n: int) -> int:
    return n * (VK_CP_MAX_PASTES * C.sizeof(vk_cp_rec) + 4)


VK_MG_MAX_INDENTS, VK_MG_MAX_SCRATCHES, VK_MG_MAX_BLOBS, VK_MG_MAX_RECTS = 8, 64, 8, 4
VK_MG_MIN_SIDE, VK_MG_MAX_SIDE, VK_MG_COORD_MARGIN = 16, 1024, 8192


class vk_mg_indent(C.Structure):
    _fields_ = [("vx", C.c_int32 * 4), ("vy", C.c_int32 * 4), ("ax", C.c_int32), ("ay", C.c_int32), ("shade", C.c_int32 * 4),
                ("slope", C.c_int32 * 4), ("ridge", C.c_int32), ("ridge_hw", C.c_int32), ("halo_r", C.c_int32), ("halo_depth", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class vk_mg_scratch(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("x", "y", "dx", "dy", "hw", "depth", "t0", "t1")]


class vk_mg_blob(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("x", "y", "r", "dark")]


class vk_mg_rect(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("thickness", C.c_int32), ("color", C.c_int32 * 3)]


class vk_mg_scene(C.Structure):
    _fields_ = [("n_indents", C.c_int32), ("n_scratches", C.c_int32), ("n_blobs", C.c_int32), ("n_rects", C.c_int32), ("base", C.c_int32),
                ("tint", C.c_int32 * 3), ("grad_x", C.c_int32), ("grad_y", C.c_int32), ("grad_cx", C.c_int32), ("grad_cy", C.c_int32),
                ("vig_cx", C.c_int32), ("vig_cy", C.c_int32), ("vig", C.c_int32), ("tex_amp", C.c_int32), ("tex_cos", C.c_int32),
                ("tex_sin", C.c_int32), ("tex_lu", C.c_int32), ("tex_lv", C.c_int32), ("tex_seed", C.c_uint32), ("blur_r", C.c_int32),
                ("noise_amp", C.c_int32), ("noise_seed", C.c_uint32), ("reserved", C.c_int32 * 8),
                ("indents", vk_mg_indent * VK_MG_MAX_INDENTS), ("scratches", vk_mg_scratch * VK_MG_MAX_SCRATCHES),
                ("blobs", vk_mg_blob * VK_MG_MAX_BLOBS), ("rects", vk_mg_rect * VK_MG_MAX_RECTS)]


VK_EDT_MAX_SIDE, VK_EDT_NONE = 4096, 0x7FFFFFFF
VK_EDT_FG, VK_EDT_BG, VK_EDT_EDGE, VK_EDT_ROWS_ENVELOPE, VK_EDT_ROWS_SEARCH = 0, 1, 2, 0x100, 0x200
VK_EDT_SRC_U8, VK_EDT_SRC_F32 = 0, 1
VK_BOUNDARY_LOSS_WS_BYTES = 32768


class vk_boundary_rec(C.Structure):
    _fields_ = [("n_pred", C.c_int64), ("n_gt", C.c_int64), ("area_pred", C.c_int64), ("area_gt", C.c_int64), ("max2_pg", C.c_int32),
                ("max2_gp", C.c_int32), ("q95_2_pg", C.c_int32), ("q95_2_gp", C.c_int32), ("sum_pg", C.c_double), ("sum_gp", C.c_double),
                ("within_pg", C.c_int64 * 8), ("within_gp", C.c_int64 * 8), ("band_inter", C.c_int64), ("band_union", C.c_int64),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class vk_seg_loss_cfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("terms", C.c_uint32), ("has_ignore", C.c_int32),
                ("ignore_index", C.c_int32), ("w_pix", C.c_float), ("w_focal", C.c_float), ("w_dice", C.c_float),
                ("w_jaccard", C.c_float), ("w_tversky", C.c_float), ("pix_smooth", C.c_float), ("pix_denom_valid", C.c_int32),
                ("has_pos_weight", C.c_int32), ("pos_weight", C.c_float * 16), ("focal_has_alpha", C.c_int32),
                ("focal_alpha", C.c_float), ("focal_gamma", C.c_float),
                ("dice_smooth", C.c_float), ("dice_eps", C.c_float), ("dice_log", C.c_int32), ("dice_classes", C.c_uint32),
                ("jaccard_smooth", C.c_float), ("jaccard_eps", C.c_float), ("jaccard_log", C.c_int32), ("jaccard_classes", C.c_uint32),
                ("tversky_smooth", C.c_float), ("tversky_eps", C.c_float), ("tversky_log", C.c_int32), ("tversky_classes", C.c_uint32),
                ("tversky_alpha", C.c_float), ("tversky_beta", C.c_float), ("tversky_gamma", C.c_float),
                ("w_mcc", C.c_float), ("mcc_eps", C.c_float)]


class vk_lovasz_cfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("per_image", C.c_int32), ("has_ignore", C.c_int32),
                ("ignore_index", C.c_int32)]


SWEEP_FIELDS = ("stats", "per_image", "dice", "iou", "mean_dice", "mean_iou", "micro_stats", "micro", "ap", "auc", "best_dice", "best_iou",
                "best_f1", "best_mean", "group_dice", "group_iou", "group_mean_dice", "group_mean_iou", "epoch_dice", "epoch_iou",
                "epoch_mean_dice", "epoch_mean_iou")


class vk_sweep_layout(C.Structure):
    _fields_ = [(f, C.c_size_t) for f in SWEEP_FIELDS + ("total_bytes", "workspace_bytes")]


INST_INT_FIELDS = ("tp", "fp", "fn", "n_rel", "n_pred_used", "n_gt_used", "n_split", "n_merge", "overflow_pred", "overflow_gt", "n_images")
INST_FLOAT_FIELDS = ("sum_iou", "sum_abs_d", "sum_rel_d", "sum_signed_rel_d", "sum_hv_rel", "max_abs_d")


class vk_inst_stats(C.Structure):
    _fields_ = [(f, C.c_int64) for f in INST_INT_FIELDS] + [(f, C.c_double) for f in INST_FLOAT_FIELDS]


VK_SUBPIX_CORNER, VK_SUBPIX_LINES = 0, 1
VK_SUBPIX_MAX_WIN, VK_SUBPIX_MAX_REACH, VK_SUBPIX_MAX_STATIONS = 15, 15, 32
SUBPIX_FLAGS = {"singular": 1, "left_map": 2, "not_converged": 4, "restored": 8, "short_side": 16, "no_edge": 32, "parallel": 64}


class vk_subpix_params(C.Structure):
    _fields_ = [("method", C.c_int), ("win", C.c_int), ("zero_zone", C.c_int), ("max_iter", C.c_int), ("eps", C.c_double),
                ("wt", C.c_double * (2 * VK_SUBPIX_MAX_WIN + 1)), ("n_stations", C.c_int), ("reach", C.c_int), ("lo", C.c_double),
                ("hi", C.c_double), ("level", C.c_double), ("max_shift", C.c_double)]


class vk_subpix_quad(C.Structure):
    _fields_ = [("label", C.c_int), ("area", C.c_int), ("valid", C.c_int), ("reserved", C.c_int), ("flags", C.c_int * 4),
                ("iters", C.c_int * 4), ("v", C.c_double * 8), ("vs", C.c_double * 8), ("d1", C.c_double), ("d2", C.c_double),
                ("d_mean", C.c_double)]


VK_KP_VERT_I32, VK_KP_VERT_F64 = 0, 1
VK_KP_MAX_RADIUS16, VK_KP_MAX_NMS, VK_KP_MAX_SEARCH, VK_KP_MAX_CWIN = 192, 8, 31, 7
VK_KP_TABLE_MEMORY, VK_KP_TABLE_LDS, VK_KP_TABLE_LDS_MAX = 1, 2, 15360
VK_KP_PARABOLA, VK_KP_CENTROID = 0, 1
KP_FLAGS = {"no_peak": 128, "at_edge": 256, "shared": 512}


class vk_kp_peak(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("value", C.c_float), ("reserved", C.c_int32)]


class vk_kp_params(C.Structure):
    _fields_ = [("method", C.c_int), ("search", C.c_int), ("cwin", C.c_int), ("min_peak", C.c_double), ("floor_frac", C.c_double)]


VK_KP_LOSS_MAX_EXP = 8


class vk_kp_loss_cfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("heat_planes", C.c_uint32), ("bce_planes", C.c_uint32), ("w_heat", C.c_float),
                ("w_bce", C.c_float), ("alpha", C.c_int32), ("beta", C.c_int32), ("pos_threshold", C.c_float),
                ("has_pos_weight", C.c_int32), ("pos_weight", C.c_float * 16)]


ZOOM_STATUS = {"clipped": 1, "scale_clamped_lo": 2, "scale_clamped_hi": 4, "zoomed": 16, "no_target": 32, "refine_failed": 64,
               "disagrees": 128, "no_window": 256}
VK_ZOOM_FAIL_MASK = 0x7F
VK_ZOOM_STAGED = 1


class vk_zoom_params(C.Structure):
    _fields_ = [("S", C.c_int), ("max_windows", C.c_int), ("margin", C.c_double), ("s_min", C.c_double), ("s_max", C.c_double)]


class vk_zoom_window(C.Structure):
    _fields_ = [("map", C.c_int), ("slot", C.c_int), ("status", C.c_int), ("pad", C.c_int), ("X0", C.c_double), ("Y0", C.c_double),
                ("s", C.c_double)]


class vk_zoom_image(C.Structure):
    _fields_ = [("ptr", C.c_uint64), ("h", C.c_int), ("w", C.c_int), ("stride", C.c_int64)]


VK_RENDER_RGB = 1
VK_RENDER_DIRECT = 1
VK_RENDER_MASK_U8, VK_RENDER_MASK_F32 = 0, 1
VK_RENDER_COORD_BOX, VK_RENDER_COORD_V, VK_RENDER_COORD_VS = 0, 1, 2
VK_RENDER_MAX_COORD = 1 << 20
VK_RENDER_LABEL_MAX = 24
RENDER_CHARS = "#0123456789 mean=.px?"


class vk_render_blend(C.Structure):
    _fields_ = [("color", C.c_uint8 * 3), ("pad", C.c_uint8), ("alpha", C.c_float), ("beta", C.c_float), ("gamma", C.c_float)]


class vk_render_style(C.Structure):
    _fields_ = [("palette", (C.c_uint8 * 3) * 8), ("diag", C.c_uint8 * 3), ("pad", C.c_uint8), ("thickness", C.c_int), ("text_scale", C.c_int)]


class vk_render_prim(C.Structure):
    _fields_ = [("rank", C.c_int32), ("slot", C.c_int32), ("corner", C.c_int32 * 8), ("anchor", C.c_int32 * 2), ("bbox", C.c_int32 * 4),
                ("diag", C.c_uint8 * 4), ("color", C.c_uint8 * 3), ("label_len", C.c_uint8), ("diag_color", C.c_uint8 * 3),
                ("thickness", C.c_uint8), ("text_scale", C.c_uint8), ("pad", C.c_uint8 * 3), ("label", C.c_uint8 * VK_RENDER_LABEL_MAX)]


class vk_render_view(C.Structure):
    _fields_ = [("src", C.c_uint64), ("src_stride", C.c_int64), ("mask", C.c_uint64), ("mask_stride", C.c_int64), ("out", C.c_uint64 * 3),
                ("out_stride", C.c_int64 * 3), ("h", C.c_int), ("w", C.c_int)]


class vk_adamw_group(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float)]


VK_AVG_EMA, VK_AVG_SWA = 0, 1
VK_AVG_MAX_RANGES = 4


class vk_avg_rule(C.Structure):
    _fields_ = [("kind", C.c_int), ("decay", C.c_float), ("warmup", C.c_int)]


class vk_avg_range(C.Structure):
    _fields_ = [("avg", C.c_void_p), ("src", C.c_void_p), ("n", C.c_size_t)]


class vk_unet_config(C.Structure):
    _fields_ = [("N", C.c_int), ("size", C.c_int), ("dtype", C.c_int), ("training", C.c_int), ("width", C.c_int)]


class vk_tensor_info(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("kind", C.c_int), ("dims", C.c_int * 4), ("ndim", C.c_int),
                ("offset", C.c_int64), ("numel", C.c_int64)]


vp, ci, cf, cd, sz, i64 = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_int64
P = C.POINTER

# name -> (restype, argtypes); every symbol include/vk_unet.h declares
SIGNATURES = {
    "vk_version": (ci, []),
    "vk_last_error_string": (C.c_char_p, []),
    "vk_has_gfx950_code": (ci, []),
    "vk_probe_mfma_rate": (ci, [ci, ci, vp, P(C.c_double), vp]),
    "vk_set_reserved_cus": (ci, [ci]),
    "vk_debug_hold_cus": (ci, [ci, ci, ci, ci, vp, sz, vp, vp]),
    "vk_debug_set_stamp_buffer": (ci, [vp]),
    "vk_prof_enable": (ci, [ci]),
    "vk_prof_collect": (ci, [C.c_char_p, sz]),
    "vk_conv_fwd": (ci, [P(vk_conv_desc), vp, vp, vp, ci, ci, vp, vp]),
    "vk_conv_dgrad_pool2": (ci, [P(vk_conv_desc), vp, vp, vp, ci, ci, vp]),
    "vk_conv_dgrad_fused": (ci, [P(vk_conv_desc), vp, vp, vp, ci, ci, P(vk_bnr), vp]),
    "vk_head_bwd_fused": (ci, [ci, ci, ci, ci, P(vk_src), vp, vp, vp, vp, vp, P(vk_bnr), vp, sz, vp]),
    "vk_halo_pack": (ci, [ci, ci, ci, vp, vp, vp]),
    "vk_conv_uses_halo_pack": (ci, [P(vk_conv_desc)]),
    "vk_conv_fwd_packed": (ci, [P(vk_conv_desc), vp, vp, vp, ci, ci, vp, vp]),
    "vk_conv_fwd_splitk": (ci, [P(vk_conv_desc), vp, vp, vp, sz, vp]),
    "vk_stem_fwd": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, vp]),
    "vk_conv_wgrad": (ci, [P(vk_conv_desc), vp, vp, vp, sz, vp]),
    "vk_conv1x1_fwd": (ci, [P(vk_conv_desc), vp, vp, ci, vp, vp]),
    "vk_conv1x1_wgrad": (ci, [P(vk_conv_desc), vp, vp, vp, sz, vp]),
    "vk_conv_wgrad_batch_supports": (ci, [P(vk_conv_desc)]),
    "vk_conv_wgrad_batch": (ci, [P(vk_conv_desc), P(vp), P(vp), ci, ci, vp, sz, vp, sz, vp]),
    "vk_stem_wgrad": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, sz, vp]),
    "vk_stem_wgrad_bn": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
    "vk_stem_wgrad_c": (ci, [ci, ci, ci, ci, ci, vp, vp, vp, vp, sz, vp]),
    "vk_stem_wgrad_bn_c": (ci, [ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
    "vk_conv_bwd_onepass": (ci, [P(vk_conv_desc), vp, vp, vp, vp, vp, P(vk_bnr), vp, vp, sz, vp]),
    "vk_stem_dgrad": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]),
    "vk_stem_dgrad_c": (ci, [ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]),
    "vk_letterbox_preprocess": (ci, [P(vk_letterbox_desc), vp, vp, vp]),
    "vk_letterbox_postprocess_mask": (ci, [P(vk_letterbox_desc), vp, cf, vp, vp]),
    "vk_letterbox_postprocess_prob": (ci, [P(vk_letterbox_desc), vp, vp, vp]),
    "vk_letterbox_postprocess_labels": (ci, [P(vk_letterbox_desc), ci, vp, vp, vp]),
    "vk_letterbox_postprocess_mask_multi": (ci, [P(vk_letterbox_desc), ci, vp, cf, vp, vp]),
    "vk_letterbox_postprocess_prob_multi": (ci, [P(vk_letterbox_desc), ci, ci, vp, vp, vp]),
    "vk_tile_preprocess": (ci, [P(vk_tile_desc), vp, vp, vp]),
    "vk_tile_blend": (ci, [P(vk_tile_desc), ci, vp, cf, vp, vp, vp]),
    "vk_geom_workspace_bytes": (i64, [P(vk_geom_desc), ci]),
    "vk_geom_minarearect": (ci, [P(vk_geom_desc), ci, vp, vp, vp, vp, vp, sz, vp]),
    "vk_geom_quadrilateral": (ci, [P(vk_geom_desc), ci, ci, vp, vp, vp, vp, vp, sz, vp]),
    "vk_geom_slot_map": (ci, [P(vk_geom_desc), ci, vp, sz, vp, vp]),
    "vk_letterbox_u8": (ci, [P(vk_letterbox_desc), vp, vp, vp]),
    "vk_letterbox_mask_u8": (ci, [P(vk_letterbox_desc), vp, vp, vp]),
    "vk_augment_workspace_bytes": (C.c_size_t, [ci, ci]),
    "vk_augment_batch": (ci, [ci, ci, ci, vp, vp, vp, P(vk_aug_params), vp, vp, vp, C.c_size_t, vp, vp, vp]),
    "vk_patch_index": (ci, [ci, P(vk_patch_item), vp, sz, vp, sz, vp, sz, vp]),
    "vk_patch_batch": (ci, [ci, ci, ci, vp, vp, vp, vp, P(vk_patch_params), vp, ci, vp, vp, vp, vp]),
    "vk_cp_boxes": (ci, [ci, ci, ci, vp, ci, vp, vp]),
    "vk_cp_alpha": (ci, [ci, ci, ci, vp, vp, vp, vp]),
    "vk_cp_paste": (ci, [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "vk_mg_scenes_dev_bytes": (sz, [ci]),
    "vk_mg_render": (ci, [ci, ci, vp, vp, sz, vp, vp, vp]),
    "vk_edt_workspace_bytes": (sz, [ci, ci, ci]),
    "vk_edt_sq": (ci, [ci, ci, ci, vp, ci, cf, ci, vp, vp, sz, vp]),
    "vk_boundary_phi": (ci, [ci, ci, ci, vp, vp, vp, vp]),
    "vk_boundary_stats_workspace_bytes": (sz, [ci, ci, ci]),
    "vk_boundary_stats": (ci, [ci, ci, ci, vp, ci, cf, vp, ci, cf, ci, P(C.c_int32), C.c_int32, vp, vp, sz, vp]),
    "vk_boundary_loss": (ci, [ci, ci, ci, vp, vp, cf, vp, vp, vp, sz, vp]),
    "vk_input_transform": (ci, [ci, ci, ci, ci, vp, vp, vp]),
    "vk_input_transform_c": (ci, [ci, ci, ci, ci, ci, vp, vp, vp]),
    "vk_input_mix": (ci, [ci, ci, sz, vp, P(cf), P(cf), vp, vp]),
    "vk_bn_finalize": (ci, [ci, ci, vp, cd, vp, vp, vp, vp, cf, cf, vp, vp, vp, vp, vp]),
    "vk_bn_relu_maxpool": (ci, [ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]),
    "vk_maxpool_bwd": (ci, [ci, ci, ci, ci, ci, vp, vp, vp, vp]),
    "vk_maxpool_bwd_bn_reduce": (ci, [ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]),
    "vk_bn_add_relu": (ci, [ci, sz, ci, vp, vp, vp, vp, vp, vp, vp, vp]),
    "vk_bn_bwd_reduce": (ci, [ci, sz, ci, vp, vp, ci, vp, vp, vp, vp, vp]),
    "vk_bn_bwd_coeffs": (ci, [ci, vp, cd, vp, vp, vp, vp, vp, vp, vp]),
    "vk_bn_bwd_coeffs_frozen": (ci, [ci, vp, vp, vp, vp, vp, vp, vp, vp]),
    "vk_bn_bwd_apply": (ci, [ci, sz, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp]),
    "vk_bn_bwd_apply_fused": (ci, [ci, sz, ci, vp, vp, ci, vp, vp, vp, vp, cd, vp, vp, vp, vp, vp, vp, vp, ci, vp]),
    "vk_upsample2x_bwd": (ci, [ci, ci, ci, ci, ci, vp, vp, ci, vp]),
    "vk_head_fwd": (ci, [ci, ci, ci, ci, P(vk_src), vp, vp, vp, vp]),
    "vk_dec4_tail_eval": (ci, [ci, ci, ci, ci, P(vk_src), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "vk_head_bwd": (ci, [ci, ci, ci, ci, P(vk_src), vp, vp, vp, vp, vp, vp, sz, vp]),
    "vk_bce_dice_loss": (ci, [sz, vp, vp, vp, vp, vp, cf, cf, cf, vp]),
    "vk_head_fwd_multi": (ci, [ci, ci, ci, ci, ci, P(vk_src), vp, vp, vp, vp]),
    "vk_head_multi_workspace_bytes": (sz, [ci]),
    "vk_head_bwd_multi": (ci, [ci, ci, ci, ci, ci, P(vk_src), vp, vp, vp, vp, vp, P(vk_bnr), vp, sz, vp]),
    "vk_multi_loss_workspace_bytes": (sz, [ci, ci, ci]),
    "vk_multilabel_loss": (ci, [ci, ci, ci, vp, vp, vp, sz, vp, vp, cf, cf, cf, vp]),
    "vk_multiclass_loss": (ci, [ci, ci, ci, vp, vp, vp, sz, vp, vp, cf, cf, cf, vp]),
    "vk_seg_loss_cfg_size": (sz, []),
    "vk_seg_loss_workspace_bytes": (sz, [ci, ci, ci]),
    "vk_seg_loss": (ci, [P(vk_seg_loss_cfg), ci, ci, ci, vp, vp, vp, sz, vp, vp, cf, vp]),
    "vk_lovasz_cfg_size": (sz, []),
    "vk_lovasz_workspace_bytes": (sz, [P(vk_lovasz_cfg), ci, ci, ci]),
    "vk_lovasz_loss": (ci, [P(vk_lovasz_cfg), ci, ci, ci, vp, vp, vp, sz, vp, vp, cf, ci, vp]),
    "vk_lovasz_flat_workspace_bytes": (sz, [ci, i64]),
    "vk_lovasz_flat": (ci, [vp, vp, ci, i64, vp, sz, vp, vp, vp, vp]),
    "vk_seg_metrics_workspace_bytes": (C.c_size_t, [ci]),
    "vk_seg_metrics": (ci, [ci, sz, vp, vp, ci, cf, cf, vp, sz, vp, vp]),
    "vk_seg_metrics_multi_workspace_bytes": (sz, [ci, ci]),
    "vk_seg_metrics_multi": (ci, [ci, ci, ci, sz, vp, vp, ci, cf, cf, vp, sz, vp, vp, vp, vp]),
    "vk_sweep_hist": (ci, [ci, sz, sz, vp, vp, ci, ci, ci, ci, ci, vp, vp, ci, vp, vp, vp]),
    "vk_sweep_curves_layout": (ci, [ci, ci, ci, ci, P(vk_sweep_layout)]),
    "vk_sweep_curves_out_bytes": (sz, [ci, ci, ci, ci]),
    "vk_sweep_curves": (ci, [ci, ci, ci, vp, vp, ci, cf, vp, sz, vp, sz, vp]),
    "vk_inst_contingency": (ci, [ci, ci, ci, vp, vp, ci, ci, vp, vp]),
    "vk_inst_match": (ci, [ci, ci, ci, vp, vp, vp, ci, vp, vp, sz, vp, sz, vp, vp, vp, vp, vp, ci, vp]),
    "vk_subpix_refine": (ci, [P(vk_subpix_params), ci, ci, ci, vp, vp, sz, sz, ci, vp, ci, vp, vp, vp]),
    "vk_kp_targets": (ci, [ci, ci, ci, vp, sz, sz, ci, ci, vp, ci, vp, ci, vp, sz, ci, vp]),
    "vk_kp_peaks_workspace_bytes": (sz, [ci, ci, ci]),
    "vk_kp_peaks": (ci, [ci, ci, ci, vp, sz, cd, ci, ci, vp, vp, vp, sz, vp]),
    "vk_kp_refine": (ci, [P(vk_kp_params), ci, ci, ci, vp, sz, vp, sz, sz, ci, vp, ci, vp, vp, vp]),
    "vk_kp_loss_cfg_size": (sz, []),
    "vk_kp_loss_workspace_bytes": (sz, [ci, ci, ci]),
    "vk_kp_loss": (ci, [P(vk_kp_loss_cfg), ci, ci, ci, vp, vp, vp, sz, vp, vp, vp, cf, ci, vp]),
    "vk_zoom_windows": (ci, [P(vk_zoom_params), ci, vp, sz, sz, ci, vp, ci, vp, vp, vp, vp, vp]),
    "vk_zoom_gather": (ci, [ci, ci, vp, ci, P(vk_zoom_image), vp, ci, ci, vp, vp]),
    "vk_zoom_merge": (ci, [ci, cd, ci, vp, vp, sz, sz, ci, vp, ci, vp, ci, ci, vp, vp, vp, vp, vp, vp]),
    "vk_render_val_panels": (ci, [ci, ci, ci, vp, vp, vp, P(cd), P(cd), P(vk_render_blend), ci, vp, i64, vp]),
    "vk_render_primitives": (ci, [ci, vp, sz, sz, ci, ci, ci, ci, vp, ci, vp, P(vk_render_style), vp, vp, vp, vp]),
    "vk_render_draw": (ci, [ci, P(vk_render_view), vp, ci, cf, P(vk_render_blend), vp, vp, ci, ci, vp]),
    "vk_render_reduce": (ci, [ci, ci, ci, vp, i64, vp, i64, vp]),
    "vk_render_glyph": (ci, [ci, P(C.c_uint8)]),
    "vk_adamw_step": (ci, [sz, vp, vp, vp, vp, cf, cf, cf, cf, cf, ci, cf, vp, vp, ci, vp]),
    "vk_amp_check_inf": (ci, [sz, vp, vp, vp]),
    "vk_amp_unscale_check": (ci, [sz, vp, vp, vp, vp]),
    "vk_adamw_step_amp": (ci, [sz, vp, vp, vp, vp, cf, cf, cf, cf, cf, vp, cf, vp, vp, vp, vp, ci, vp]),
    "vk_adamw_segment_blocks": (ci, [ci, P(i64), P(C.c_int32), ci]),
    "vk_adamw_step_amp_segments": (ci, [ci, vp, ci, vp, vp, vp, vp, vp, cf, cf, cf, cf, cf, vp, cf, vp, vp, vp, vp]),
    "vk_adamw_step_groups": (ci, [ci, vp, vp, ci, vp, vp, vp, vp, vp, ci, P(vk_adamw_group), vp, cf, vp, vp, vp, vp, vp]),
    "vk_grad_norm_segments": (ci, [ci, vp, ci, vp, vp, ci, cf, cf, vp, vp, vp]),
    "vk_avg_update": (ci, [ci, P(vk_avg_range), vk_avg_rule, vp, vp, vp, vp]),
    "vk_avg_swap": (ci, [ci, P(vk_avg_range), vp]),
    "vk_adamw_step_amp_avg": (ci, [sz, vp, vp, vp, vp, cf, cf, cf, cf, cf, vp, cf, vp, vp, vp, vp, ci, vp, vp, vk_avg_rule, vp, vp, vp, sz,
                                   vp]),
    "vk_unet_create": (ci, [P(vk_unet_config), P(vp)]),
    "vk_unet_create_ex": (ci, [P(vk_unet_config), ci, P(vp)]),
    "vk_unet_num_classes": (ci, [vp]),
    "vk_unet_create_enc": (ci, [P(vk_unet_config), ci, ci, P(vp)]),
    "vk_unet_encoder": (ci, [vp]),
    "vk_unet_create_in": (ci, [P(vk_unet_config), ci, ci, ci, P(vp)]),
    "vk_unet_in_channels": (ci, [vp]),
    "vk_unet_destroy": (None, [vp]),
    "vk_unet_set_side_stream": (ci, [vp, ci]),
    "vk_unet_num_tensors": (ci, [vp]),
    "vk_unet_tensor_info": (ci, [vp, ci, P(vk_tensor_info)]),
    "vk_unet_param_numel": (i64, [vp]),
    "vk_unet_buffer_numel": (i64, [vp]),
    "vk_unet_workspace_bytes": (i64, [vp]),
    "vk_unet_num_buckets": (ci, [vp]),
    "vk_unet_bucket_range": (ci, [vp, ci, P(i64), P(i64)]),
    "vk_unet_bind": (ci, [vp, vp, vp, vp, vp, vp, sz]),
    "vk_unet_refresh_weights": (ci, [vp, vp]),
    "vk_unet_forward": (ci, [vp, vp, vp, ci, vp]),
    "vk_unet_loss": (ci, [vp, vp, vp, vp, cf, cf, cf, vp]),
    "vk_unet_loss_ex": (ci, [vp, ci, vp, vp, vp, cf, cf, cf, vp]),
    "vk_unet_loss_cfg": (ci, [vp, P(vk_seg_loss_cfg), vp, vp, vp, cf, vp]),
    "vk_unet_loss_lovasz": (ci, [vp, P(vk_seg_loss_cfg), P(vk_lovasz_cfg), cf, vp, vp, vp, sz, vp, cf, vp]),
    "vk_unet_loss_kp": (ci, [vp, P(vk_seg_loss_cfg), P(vk_kp_loss_cfg), vp, vp, vp, sz, vp, cf, vp]),
    "vk_unet_backward": (ci, [vp, vp, ci, ci, vp]),
    "vk_unet_set_trainable": (ci, [vp, P(C.c_uint8), ci]),
    "vk_unet_set_bn_frozen": (ci, [vp, P(C.c_uint8), ci]),
    "vk_unet_set_input_grad": (ci, [vp, vp]),
    "vk_unet_zero_grad": (ci, [vp, vp]),
    "vk_unet_debug_tensor": (ci, [vp, C.c_char_p, P(vp), P(ci * 4)]),
    "vk_comm_unique_id": (ci, [vp]),
    "vk_comm_init": (ci, [ci, ci, vp, P(vp)]),
    "vk_comm_world": (ci, [vp]),
    "vk_allreduce_bucket": (ci, [vp, vp, sz, vp]),
    "vk_comm_broadcast": (ci, [vp, vp, sz, ci, vp]),
    "vk_comm_destroy": (ci, [vp]),
}

_lib = None


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile every HIP source for gfx950 into libvkunet.so (in-tree, next to this file)."""
    srcs = list(CSRC.glob("*.hip")) + list(CSRC.glob("*.h")) + [PKG_DIR.parent / "include" / "vk_unet.h"]
    if not force and LIB_PATH.exists() and all(LIB_PATH.stat().st_mtime >= s.stat().st_mtime for s in srcs):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not Path(hipcc).exists():
        raise VkError(f"hipcc not found at {hipcc}; cannot build libvkunet.so")
    cmd = ["make", "-C", str(CSRC), f"-j{min(4, os.cpu_count() or 1)}", f"HIPCC={hipcc}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if verbose:
        print(r.stdout[-2000:], r.stderr[-2000:])
    if r.returncode != 0 or not LIB_PATH.exists():
        raise VkError("building libvkunet.so failed:\n" + r.stdout[-3000:] + r.stderr[-3000:])
    return LIB_PATH


def lib():
    """The loaded library with typed entry points.  Raises VkError when it is absent: no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise VkError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                      f"(make -C {CSRC}); this package has no CPU fallback")
    try:
        L = C.CDLL(str(LIB_PATH))
    except OSError as e:  # pragma: no cover
        raise VkError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is None:
            raise VkError(f"{LIB_PATH} does not export {name}")
        fn.restype = res
        fn.argtypes = args
    if L.vk_version() != 1:
        raise VkError("libvkunet.so ABI version mismatch")
    _lib = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().vk_last_error_string().decode(errors="replace")
        kind = "argument/state error" if rc < 0 else f"hipError {rc}"
        raise VkError(f"{what or 'libvkunet'}: {kind}: {msg}")


def dtype_code(dt) -> int:
    import torch
    return {torch.float32: VK_F32, torch.bfloat16: VK_BF16, torch.float16: VK_F16}[dt]


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def current_stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream


def prof_collect():
    """Aggregate per-kernel-family timings recorded since vk_prof_enable(1): {tag: dict(n, ms, flops, bytes)}."""
    buf = C.create_string_buffer(1 << 16)
    n = lib().vk_prof_collect(buf, len(buf))
    out = {}
    for line in buf.raw[:max(n, 0)].decode().splitlines():
        tag, cnt, ms, fl, by = line.split()
        out[tag] = dict(n=int(cnt), ms=float(ms), flops=float(fl), bytes=float(by))
    return out
