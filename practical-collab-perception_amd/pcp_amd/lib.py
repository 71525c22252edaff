"""ctypes binding of libpcp_hip.so (the C ABI declared in include/pcp_hip.h).

The library is built in-tree by `make -C practical-collab-perception_amd/csrc` (or __graft_entry__.build()).  There is NO
fallback: if the shared object is missing or a symbol cannot be resolved the import of the product path fails loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PCP_HIP_LIB') or os.path.abspath(os.path.join(_HERE, '..', 'lib', 'libpcp_hip.so'))   # override: kernel A/B builds

c_f = ctypes.c_float
c_i32 = ctypes.c_int32
c_i64 = ctypes.c_int64
c_sz = ctypes.c_size_t
vp = ctypes.c_void_p


class Grid(ctypes.Structure):
    _fields_ = [('min_x', c_f), ('min_y', c_f), ('min_z', c_f), ('voxel_x', c_f), ('voxel_y', c_f), ('voxel_z', c_f),
                ('nx', c_i32), ('ny', c_i32), ('batch_size', c_i32)]


class PackJob(ctypes.Structure):
    """pcp_pack_job_t (include/pcp_hip_train.h)"""
    _fields_ = [('w', ctypes.c_void_p), ('cout', ctypes.c_int32), ('cin', ctypes.c_int32), ('transpose', ctypes.c_int32),
                ('direct_cout_pad', ctypes.c_int32), ('direct', ctypes.c_void_p), ('winograd', ctypes.c_void_p),
                ('winograd_cout_pad', ctypes.c_int32), ('f4_cout_pad', ctypes.c_int32), ('u4f', ctypes.c_void_p), ('u4h', ctypes.c_void_p),
                ('block_start', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class Conv3x3(ctypes.Structure):
    _fields_ = [('batch', c_i32), ('in_h', c_i32), ('in_w', c_i32), ('cin', c_i32), ('cout', c_i32), ('cout_pad', c_i32),
                ('stride', c_i32), ('ld_in', c_i32), ('ld_out', c_i32), ('relu', c_i32)]


class MpConv3x3(ctypes.Structure):
    """pcp_mp_conv3x3_t (include/pcp_hip_mp.h)"""
    _fields_ = [('batch', c_i32), ('in_h', c_i32), ('in_w', c_i32), ('cin', c_i32), ('cout', c_i32), ('cout_pad', c_i32),
                ('stride', c_i32), ('ld_in', c_i32), ('ld_out', c_i32), ('relu', c_i32), ('in_dtype', c_i32), ('out_dtype', c_i32)]


class MpWgrad3x3(ctypes.Structure):
    """pcp_mp_wgrad3x3_t (include/pcp_hip_mp.h)"""
    _fields_ = [('batch', c_i32), ('in_h', c_i32), ('in_w', c_i32), ('cin', c_i32), ('cout', c_i32), ('stride', c_i32),
                ('ld_x', c_i32), ('ld_dy', c_i32), ('x_dtype', c_i32), ('dy_dtype', c_i32), ('accumulate', c_i32)]


class MpPackJob(ctypes.Structure):
    """pcp_mp_pack_job_t (include/pcp_hip_mp.h)"""
    _fields_ = [('w', vp), ('packed', vp), ('cout', c_i32), ('cin', c_i32), ('transpose', c_i32), ('out_pad', c_i32), ('block_start', c_i32),
                ('reserved', c_i32)]


class MpPointwise(ctypes.Structure):
    """pcp_mp_pointwise_t (include/pcp_hip_mp.h)"""
    _fields_ = [('mode', c_i32), ('rows', c_i64), ('batch', c_i32), ('in_h', c_i32), ('in_w', c_i32), ('cin', c_i32), ('cout', c_i32),
                ('cout_pad', c_i32), ('ld_in', c_i32), ('ld_out', c_i32), ('relu', c_i32), ('in_dtype', c_i32), ('out_dtype', c_i32)]


class MpRowMap(ctypes.Structure):
    """pcp_mp_rowmap_t (include/pcp_hip_mp.h)"""
    _fields_ = [('ptr', vp), ('ld', c_i32), ('channels', c_i32), ('lattice', c_i32), ('grid_h', c_i32), ('grid_w', c_i32), ('ky', c_i32),
                ('kx', c_i32), ('dtype', c_i32), ('extent_bytes', ctypes.c_uint64)]


DT_F32, DT_BF16 = 0, 1


class Pointwise(ctypes.Structure):
    _fields_ = [('mode', c_i32), ('rows', c_i64), ('batch', c_i32), ('in_h', c_i32), ('in_w', c_i32), ('cin', c_i32),
                ('cout', c_i32), ('cout_pad', c_i32), ('ld_in', c_i32), ('ld_out', c_i32), ('relu', c_i32),
                ('in2', vp), ('ld_in2', c_i32), ('k_split', c_i32), ('residual', vp), ('ld_res', c_i32)]


class DetHead(ctypes.Structure):
    _fields_ = [('boxes', vp), ('scores', vp), ('labels', vp), ('keep', vp), ('keep_count', vp), ('class_map', vp), ('k', c_i32),
                ('keep_max', c_i32)]


class Decode(ctypes.Structure):
    _fields_ = [('batch', c_i32), ('h', c_i32), ('w', c_i32), ('ld', c_i32), ('num_class', c_i32), ('ch_center', c_i32),
                ('ch_z', c_i32), ('ch_dim', c_i32), ('ch_rot', c_i32), ('ch_hm', c_i32), ('k', c_i32), ('stride', c_f),
                ('voxel_x', c_f), ('voxel_y', c_f), ('min_x', c_f), ('min_y', c_f), ('limit', c_f * 6),
                ('use_score_thresh', c_i32), ('score_thresh', c_f), ('activated', c_i32)]


class DecodeHead(ctypes.Structure):
    """pcp_decode_head_t: one head of pcp_centerhead_decode_ext"""
    _fields_ = [('d', Decode), ('head', vp), ('ch_vel', c_i32), ('ch_iou', c_i32), ('iou_alpha', c_f), ('boxes', vp), ('scores', vp),
                ('labels', vp), ('cell', vp), ('count', vp), ('vel', vp)]


class DetHeadExt(ctypes.Structure):
    _fields_ = [('h', DetHead), ('vel', vp)]


class Anchor(ctypes.Structure):
    _fields_ = [('batch', c_i32), ('h', c_i32), ('w', c_i32), ('ld', c_i32), ('anchors_per_loc', c_i32), ('num_class', c_i32),
                ('num_dir_bins', c_i32), ('ch_cls', c_i32), ('ch_box', c_i32), ('ch_dir', c_i32), ('dir_offset', c_f),
                ('dir_limit_offset', c_f), ('dir_period', c_f), ('use_score_thresh', c_i32), ('score_thresh', c_f)]


class RowMap(ctypes.Structure):
    _fields_ = [('ptr', vp), ('ld', c_i32), ('channels', c_i32), ('lattice', c_i32), ('grid_h', c_i32), ('grid_w', c_i32),
                ('ky', c_i32), ('kx', c_i32)]


class Target(ctypes.Structure):
    _fields_ = [('batch', c_i32), ('h', c_i32), ('w', c_i32), ('num_class', c_i32), ('k', c_i32), ('stride', c_f), ('voxel_x', c_f),
                ('voxel_y', c_f), ('min_x', c_f), ('min_y', c_f), ('gaussian_overlap', c_f), ('min_radius', c_i32)]


class HeadLoss(ctypes.Structure):
    _fields_ = [('batch', c_i32), ('h', c_i32), ('w', c_i32), ('ld', c_i32), ('ld_d', c_i32), ('num_class', c_i32), ('ch_hm', c_i32),
                ('reg_ch', c_i32 * 8), ('k', c_i32), ('cls_weight', c_f), ('loc_weight', c_f), ('code_weights', c_f * 8)]


DET_MAX_HEADS = 8            # PCP_DET_MAX_HEADS: heads per call of the _ext entry points
TGT_MAX_CLASSES = 32
HEADLOSS_MAX_CODES = 16


class TargetHead(ctypes.Structure):
    """pcp_target_head_t: one head of pcp_centerhead_targets_ext"""
    _fields_ = [('num_class', c_i32), ('class_to_local', c_i32 * TGT_MAX_CLASSES), ('heatmap', vp), ('target_boxes', vp), ('inds', vp),
                ('mask', vp), ('head', vp), ('ld', c_i32), ('ch_center', c_i32), ('ch_z', c_i32), ('ch_dim', c_i32), ('ch_rot', c_i32)]


class HeadLossHead(ctypes.Structure):
    """pcp_headloss_head_t: one head of pcp_centerhead_loss_ext"""
    _fields_ = [('head', vp), ('dhead', vp), ('heatmap', vp), ('target_boxes', vp), ('inds', vp), ('mask', vp), ('ld', c_i32),
                ('ld_d', c_i32), ('ch_hm', c_i32), ('num_class', c_i32), ('n_codes', c_i32), ('reg_ch', c_i32 * HEADLOSS_MAX_CODES),
                ('tb_width', c_i32)]


class HeadLossExt(ctypes.Structure):
    _fields_ = [('batch', c_i32), ('h', c_i32), ('w', c_i32), ('k', c_i32), ('cls_weight', c_f), ('loc_weight', c_f),
                ('code_weights', c_f * HEADLOSS_MAX_CODES)]


class AnchorAssign(ctypes.Structure):
    _fields_ = [('batch', c_i32), ('h', c_i32), ('w', c_i32), ('anchors_per_loc', c_i32), ('num_class', c_i32), ('num_groups', c_i32),
                ('slot_group', c_i32 * 32), ('group_class', c_i32 * 8), ('matched', c_f * 8), ('unmatched', c_f * 8)]


class AnchorLoss(ctypes.Structure):
    _fields_ = [('batch', c_i32), ('h', c_i32), ('w', c_i32), ('ld', c_i32), ('ld_d', c_i32), ('anchors_per_loc', c_i32),
                ('num_class', c_i32), ('num_dir_bins', c_i32), ('ch_cls', c_i32), ('ch_box', c_i32), ('ch_dir', c_i32),
                ('dir_offset', c_f), ('dir_period', c_f), ('cls_weight', c_f), ('loc_weight', c_f), ('dir_weight', c_f),
                ('code_weights', c_f * 7)]


AUG_FLIP_X, AUG_FLIP_Y, AUG_ROTATE, AUG_SCALE, AUG_TRANSLATE = 1, 2, 3, 4, 5       # PCP_AUG_* (include/pcp_hip_train.h)
AUG_MAX_STAGES, AUG_MAX_BATCH, AUG_TABLE_STRIDE = 8, 64, 12
AUG_MIN_ROW_STRIDE, AUG_MAX_ROW_STRIDE, AUG_TILE_ROWS = 4, 15, 512
GTS_MAX_GROUPS, GTS_MAX_CAND, GTS_MAX_BOXES, GTS_CAND_STRIDE, GTS_ACC_STRIDE = 16, 64, 512, 10, 4      # PCP_GTS_* (include/pcp_hip_train.h)


EVAL_MAX_BOXES, EVAL_THRESHOLDS, EVAL_RECORD_WORDS, EVAL_POINTS, EVAL_NAN_ORIENT, EVAL_NAN_VEL = 512, 4, 8, 101, 1, 2     # PCP_EVAL_* (include/pcp_hip.h)


class WorldAug(ctypes.Structure):
    """pcp_world_aug_t (include/pcp_hip_train.h)"""
    _fields_ = [('n_stages', c_i32), ('stage', c_i32 * AUG_MAX_STAGES), ('batch', c_i32), ('hd_map', c_i32), ('filter', c_i32),
                ('range', c_f * 6), ('raw_heading', c_i32)]


# PCP_OBJ_* (include/pcp_hip_train.h)
OBJ_TRANSLATE_X, OBJ_TRANSLATE_Y, OBJ_TRANSLATE_Z, OBJ_SCALE, OBJ_ROTATE = 1, 2, 3, 4, 5
OBJ_DROP_TOP, OBJ_DROP_BOTTOM, OBJ_DROP_LEFT, OBJ_DROP_RIGHT = 6, 7, 8, 9
OBJ_WORLD_DROP_TOP, OBJ_WORLD_DROP_BOTTOM, OBJ_WORLD_DROP_LEFT, OBJ_WORLD_DROP_RIGHT = 10, 11, 12, 13
OBJ_MAX_STAGES, OBJ_MAX_BOXES, OBJ_LDS_BOXES, OBJ_STATE_STRIDE, OBJ_PARAM_STRIDE = 16, 512, 64, 12, 4


class ObjectAug(ctypes.Structure):
    """pcp_object_aug_t (include/pcp_hip_train.h)"""
    _fields_ = [('n_stages', c_i32), ('stage', c_i32 * OBJ_MAX_STAGES), ('batch', c_i32), ('limit_heading', c_i32)]


class HunterMeta(ctypes.Structure):
    _fields_ = [('batch', c_i32), ('max_inst', c_i32), ('num_sweeps', c_i32), ('sweep_col', c_i32), ('inst_col', c_i32)]


class HunterLoss(ctypes.Structure):
    _fields_ = [('n', c_i64), ('stride', c_i32), ('n_fg', c_i32), ('n_local', c_i32), ('n_inst', c_i32), ('c', c_i32),
                ('batch', c_i32), ('max_inst', c_i32), ('num_sweeps', c_i32),
                ('points', vp), ('gt_boxes', vp), ('instances_tf', vp),
                ('fg_idx', vp), ('fg_local', vp), ('local_key', vp), ('local_inst', vp), ('inst_key', vp),
                ('head', vp), ('ld_head', c_i32), ('local_feat', vp), ('ld_local_feat', c_i32), ('locals_feat', vp), ('ld_locals_feat', c_i32),
                ('locals_tf', vp), ('ld_locals_tf', c_i32), ('coef_fg', c_f), ('coef_locals', c_f), ('grad_scale', c_f),
                ('dhead', vp), ('ld_dhead', c_i32), ('dlocal_feat_fg', vp), ('dlocals_feat', vp), ('dlocals_tf', vp), ('ld_dlocals_tf', c_i32),
                ('losses', vp), ('labels', vp), ('tgt_embedding', vp), ('tgt_offset', vp),
                ('gt_stride', c_i32)]               # floats per gt_boxes row (GT_BOX_MIN_WIDTH .. GT_BOX_MAX_WIDTH); 0 = 8


GT_BOX_MIN_WIDTH, GT_BOX_MAX_WIDTH = 8, 16          # include/pcp_hip_train.h: PCP_GT_BOX_MIN_WIDTH / PCP_GT_BOX_MAX_WIDTH


def check_gt_box_width(width, what='gt_boxes'):
    """the refusal of the HunterJr training kernels, on the host and before any launch"""
    if not GT_BOX_MIN_WIDTH <= int(width) <= GT_BOX_MAX_WIDTH:
        raise ValueError('%s rows have %d columns: the HunterJr training kernels take %d (x y z dx dy dz heading class) up to %d, the '
                         'number of box codes the head kernels take' % (what, int(width), GT_BOX_MIN_WIDTH, GT_BOX_MAX_WIDTH))
    return int(width)


PW_PLAIN, PW_SPACE2DEPTH, PW_DEPTH2SPACE = 0, 1, 2
RELU_PRE_RESIDUAL = 2          # pcp_pointwise relu value: relu(x W^T + b + residual)

# every symbol include/pcp_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'pcp_abi_version': (c_i32, []),
    'pcp_status_string': (ctypes.c_char_p, [c_i32]),
    'pcp_set_option': (c_i32, [c_i32, c_i64]),
    'pcp_get_option': (c_i64, [c_i32]),
    'pcp_pillar_index_export': (c_i32, [ctypes.POINTER(Grid), vp, c_i64, c_i32, vp, vp, vp, vp, vp, vp]),
    'pcp_voxelize_workspace_bytes': (c_sz, [ctypes.POINTER(Grid), c_i64]),
    'pcp_voxelize': (c_i32, [vp, c_i64, c_i32, ctypes.POINTER(Grid), vp, c_sz, vp, vp, vp, vp, vp]),
    'pcp_pfn_scatter': (c_i32, [vp, c_i64, c_i32, c_i32, ctypes.POINTER(Grid), vp, vp, vp, vp, vp, vp, vp, vp]),
    'pcp_pillarise_rows_workspace_bytes': (c_sz, [ctypes.POINTER(Grid), c_i64, c_i32]),
    'pcp_pillarise_rows': (c_i32, [vp, c_i64, c_i32, c_i32, ctypes.POINTER(Grid), vp, c_sz, vp, vp, vp, vp, c_i32, vp]),
    'pcp_pfn_rows': (c_i32, [ctypes.POINTER(Grid), vp, c_i64, c_i32, vp, vp, vp, vp, vp, vp, vp]),
    'pcp_pfn_features': (c_i32, [vp, c_i64, c_i32, c_i32, ctypes.c_uint32, ctypes.POINTER(Grid), vp, c_i32, vp, vp, vp]),
    'pcp_pfn_cat_pillar_max': (c_i32, [vp, c_i32, vp, c_i32, vp, c_i64, c_i32, vp, c_i32, vp]),
    'pcp_canvas_clear': (c_i32, [ctypes.POINTER(Grid), vp, c_i64, vp, vp]),
    'pcp_fill_zero': (c_i32, [vp, c_sz, vp]),
    'pcp_conv3x3': (c_i32, [ctypes.POINTER(Conv3x3), vp, vp, vp, vp, vp]),
    'pcp_sparse_conv3x3_s2': (c_i32, [vp, ctypes.POINTER(Grid), vp, c_i64, vp, vp, c_i32, c_i32, vp, c_i32, vp]),
    'pcp_conv3x3_winograd': (c_i32, [ctypes.POINTER(Conv3x3), vp, vp, vp, vp, vp]),
    'pcp_conv3x3_winograd_plan': (c_i32, [ctypes.POINTER(Conv3x3), ctypes.POINTER(c_i32), ctypes.POINTER(ctypes.c_double)]),
    'pcp_conv3x3_winograd_ws_supported': (c_i32, [ctypes.POINTER(Conv3x3)]),
    'pcp_conv3x3_winograd_ws': (c_i32, [ctypes.POINTER(Conv3x3), vp, vp, vp, vp, vp]),
    'pcp_conv3x3_winograd_ws_plan': (c_i32, [ctypes.POINTER(Conv3x3), ctypes.POINTER(c_i32), ctypes.POINTER(ctypes.c_double)]),
    'pcp_conv3x3_winograd4f': (c_i32, [ctypes.POINTER(Conv3x3), vp, vp, vp, vp, vp]),
    'pcp_conv3x3_winograd4f_plan': (c_i32, [ctypes.POINTER(Conv3x3), ctypes.POINTER(ctypes.c_double)]),
    'pcp_conv3x3_winograd4h': (c_i32, [ctypes.POINTER(Conv3x3), vp, vp, vp, vp, vp]),
    'pcp_conv3x3_winograd4h_plan': (c_i32, [ctypes.POINTER(Conv3x3), ctypes.POINTER(ctypes.c_double)]),
    'pcp_conv3x3_winograd4c': (c_i32, [ctypes.POINTER(Conv3x3), vp, vp, vp, vp, vp]),
    'pcp_conv3x3_winograd4c_plan': (c_i32, [ctypes.POINTER(Conv3x3), ctypes.POINTER(ctypes.c_double)]),
    'pcp_conv3x3_winograd4_workspace_bytes': (c_i32, [ctypes.POINTER(Conv3x3), ctypes.POINTER(c_sz)]),
    'pcp_conv3x3_winograd4': (c_i32, [ctypes.POINTER(Conv3x3), vp, vp, vp, vp, vp, vp]),
    'pcp_conv3x3_winograd4_timed': (c_i32, [ctypes.POINTER(Conv3x3), vp, vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_float),
                                            ctypes.POINTER(ctypes.c_double)]),
    'pcp_conv3x3_bf16x3': (c_i32, [ctypes.POINTER(Conv3x3), vp, vp, vp, vp, vp]),
    'pcp_conv3x3_bf16': (c_i32, [ctypes.POINTER(Conv3x3), vp, vp, vp, vp, vp]),
    'pcp_conv3x3_grouped_small': (c_i32, [vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.POINTER(c_i32), vp, vp, vp, c_i32, vp]),
    'pcp_pointwise': (c_i32, [ctypes.POINTER(Pointwise), vp, vp, vp, vp, vp]),
    'pcp_decode_workspace_bytes': (c_sz, [ctypes.POINTER(Decode)]),
    'pcp_centerhead_decode': (c_i32, [ctypes.POINTER(Decode), vp, vp, c_sz, vp, vp, vp, vp, vp, vp]),
    'pcp_centerhead_decode_ext': (c_i32, [ctypes.POINTER(DecodeHead), c_i32, vp]),
    'pcp_gather_detections_ext': (c_i32, [ctypes.POINTER(DetHeadExt), c_i32, c_i32, c_i32, vp, vp, vp, vp, vp]),
    'pcp_avgpool_nhwc': (c_i32, [vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, vp, c_i32, vp]),
    'pcp_sc_gate': (c_i32, [vp, c_i32, vp, c_i32, vp, c_i32, c_i32, c_i32, vp, c_i32, c_i32, c_i32, c_i32, c_i32, vp]),
    'pcp_column_id_mask': (c_i32, [vp, ctypes.c_int64, c_i32, c_i32, vp, vp]),
    'pcp_column_id_counts': (c_i32, [vp, ctypes.c_int64, c_i32, c_i32, vp, vp]),
    'pcp_agent_frame_live': (c_i32, [vp, c_i64, c_i32, c_i32, c_i32, vp, vp]),
    'pcp_zero_maps_unless': (c_i32, [vp, c_i64, c_i32, ctypes.POINTER(c_i32), vp, vp]),
    'pcp_select_transform_compact_workspace_bytes': (c_sz, [c_i64, c_i32]),
    'pcp_select_transform_compact': (c_i32, [vp, c_i64, c_i32, c_i32, c_i32, ctypes.POINTER(c_f), c_i32, ctypes.POINTER(c_f),
                                             ctypes.POINTER(ctypes.c_uint8), vp, c_i64, vp, c_sz, vp, ctypes.POINTER(Grid), vp, c_sz, vp]),
    'pcp_select_transform_compact_dev': (c_i32, [vp, c_i64, c_i32, c_i32, c_i32, ctypes.POINTER(c_f), c_i32, vp, vp, vp, c_i64, vp, c_sz, vp,
                                                 ctypes.POINTER(Grid), vp, c_sz, vp]),
    'pcp_warp_nearest_batch_dev': (c_i32, [vp, vp, vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, vp]),
    'pcp_voxelize_cells_ready': (c_i32, [vp, c_i64, c_i32, ctypes.POINTER(Grid), vp, c_sz, vp, vp, vp, vp]),
    'pcp_gather_detections': (c_i32, [ctypes.POINTER(DetHead), c_i32, c_i32, c_i32, vp, vp, vp, vp, vp]),
    'pcp_nms_workspace_bytes': (c_sz, [c_i32, c_i32]),
    'pcp_nms_rotated': (c_i32, [vp, vp, c_i32, c_i32, vp, c_f, c_i32, c_i32, vp, c_sz, vp, vp, vp]),
    'pcp_nms_normal': (c_i32, [vp, vp, c_i32, c_i32, vp, c_f, c_i32, c_i32, vp, c_sz, vp, vp, vp]),
    'pcp_boxes_bev_pairwise': (c_i32, [vp, c_i32, vp, c_i32, c_i32, vp, vp]),
    'pcp_warp_nearest': (c_i32, [vp, vp, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.POINTER(c_f), c_i32, vp]),
    'pcp_warp_nearest_batch': (c_i32, [vp, vp, ctypes.POINTER(c_f), c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, vp]),
    'pcp_softmax_fuse': (c_i32, [ctypes.POINTER(vp), c_i32, vp, c_i32, c_i64, c_i32, c_i32, c_i32, vp, vp]),
    'pcp_disco_weight_fuse': (c_i32, [ctypes.POINTER(vp), c_i32, c_i32, c_i32, c_i64, vp, vp, vp, vp, vp, vp, vp, c_i32, vp, c_i32, vp]),
    'pcp_disco_weight_fuse_live': (c_i32, [ctypes.POINTER(vp), c_i32, c_i32, c_i32, c_i64, vp, vp, vp, vp, vp, vp, vp, c_i32, ctypes.POINTER(c_i32), vp, vp]),
    'pcp_bev_sample_bilinear': (c_i32, [vp, c_i32, c_i32, c_i32, c_i32, c_i32, vp, c_i64, c_i32, c_f, c_f, c_f, c_f, vp, vp,
                                        c_i32, vp]),
    'pcp_hunter_point_head': (c_i32, [vp, c_i32, c_i32, c_i32, c_i32, c_i32, vp, c_i64, c_i32, c_f, c_f, c_f, c_f, vp, vp, vp, vp, vp,
                                      vp, c_i32, c_i32, vp, c_i32, vp, vp]),
    'pcp_hunter_point_head_ex': (c_i32, [vp, c_i32, c_i32, c_i32, c_i32, c_i32, vp, c_i64, c_i32, c_f, c_f, c_f, c_f, vp, vp, vp, vp, vp,
                                         vp, c_i32, c_i32, vp, c_i32, vp, vp, vp, c_i32, c_f, vp, vp]),
    'pcp_voxelize_row_order': (c_i32, [ctypes.POINTER(Grid), vp, c_i64, vp, vp, vp]),
    'pcp_voxelize_sort_pillar_rows': (c_i32, [ctypes.POINTER(Grid), vp, c_i64, vp]),
    'pcp_hunter_apply_flow': (c_i32, [vp, c_i64, c_i32, vp, c_i32, c_f, vp, vp]),
    'pcp_select_transform_points': (c_i32, [vp, c_i64, c_i32, c_i32, c_f, c_i32, ctypes.POINTER(c_f), ctypes.POINTER(ctypes.c_uint8),
                                            vp, c_i32, vp]),
    'pcp_bev_scatter_mean_workspace_bytes': (c_sz, [c_i32, c_i32, c_i32, c_i64]),
    'pcp_bev_scatter_mean': (c_i32, [vp, c_i64, c_i32, vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_f, c_f, c_f, c_f, vp, c_sz,
                                     vp, c_i32, vp]),
    'pcp_anchor_decode': (c_i32, [ctypes.POINTER(Anchor), vp, vp, vp, vp, vp, vp, vp]),
    'pcp_topk_boxes': (c_i32, [vp, vp, vp, c_i32, c_i64, c_i32, vp, vp, vp, vp, vp, vp]),
    'pcp_points_in_boxes': (c_i32, [vp, c_i32, c_i32, c_i32, vp, c_i32, c_i32, vp, vp]),
    'pcp_hunter_foreground_workspace_bytes': (c_sz, [c_i64]),
    'pcp_hunter_foreground_rows': (c_i32, [vp, c_i64, c_i32, vp, c_i32, c_f, vp, c_sz, vp, vp, vp, vp]),
    'pcp_modar_ingest_batched_workspace_bytes': (c_sz, [c_i32, c_i64]),
    'pcp_modar_ingest_batched': (c_i32, [vp, vp, vp, vp, c_i32, c_i32, vp, c_i32, vp, vp, c_i64, vp, vp, vp, vp, c_sz, vp, vp]),
    'pcp_modar_ingest': (c_i32, [vp, c_i32, vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_double), c_f, vp, vp]),
    'pcp_det_eval_match': (c_i32, [vp, vp, vp, vp, c_i32, c_i32, c_i32, vp, c_i32, c_i32, c_i32, ctypes.POINTER(c_f), c_i32, vp, vp, c_i64, vp, vp, vp]),
    'pcp_det_eval_curves_workspace_bytes': (c_sz, [c_i64]),
    'pcp_det_eval_curves_stride': (c_i32, []),
    'pcp_det_eval_curves': (c_i32, [vp, c_i64, vp, vp, c_i32, c_i32, vp, vp, c_sz, vp, vp]),
}

# include/pcp_hip_train.h
SYMBOLS.update({
    'pcp_bn_workspace_bytes': (c_sz, [c_i32]),
    'pcp_bn_train_stats': (c_i32, [vp, c_i64, c_i32, c_i32, vp, vp, c_f, c_f, vp, vp, vp, vp, vp, vp, vp, vp]),
    'pcp_scale_shift_act': (c_i32, [vp, c_i64, c_i32, c_i32, vp, vp, c_i32, vp, c_i32, vp]),
    'pcp_bn_act_backward': (c_i32, [vp, c_i32, vp, c_i32, c_i64, c_i32, vp, vp, vp, vp, c_i32, vp, vp, vp, c_i32, vp, c_i32, vp]),
    'pcp_colsum': (c_i32, [vp, c_i64, c_i32, c_i32, vp, vp, c_i32, vp]),
    'pcp_bn_train_sums': (c_i32, [vp, c_i64, c_i32, c_i32, vp, vp, vp]),
    'pcp_bn_train_stats_from_sums': (c_i32, [vp, c_i64, c_i32, vp, vp, c_f, c_f, vp, vp, vp, vp, vp, vp, vp]),
    'pcp_bn_bwd_sums': (c_i32, [vp, c_i32, vp, c_i32, c_i64, c_i32, vp, vp, vp, vp, c_i32, vp, vp, vp]),
    'pcp_bn_bwd_apply_from_sums': (c_i32, [vp, c_i32, vp, c_i32, c_i64, c_i32, vp, vp, vp, vp, c_i32, vp, vp, c_i64, vp, vp, vp, c_i32, vp, c_i32, vp]),
    'pcp_accumulate': (c_i32, [vp, c_i32, vp, c_i32, c_i64, c_i32, c_f, vp]),
    'pcp_dilate2x': (c_i32, [vp, c_i32, c_i32, c_i32, c_i32, c_i32, vp, c_i32, vp]),
    'pcp_conv3x3_wgrad_workspace_bytes': (c_sz, [ctypes.POINTER(Conv3x3)]),
    'pcp_conv3x3_wgrad': (c_i32, [ctypes.POINTER(Conv3x3), vp, vp, vp, c_sz, vp, c_i32, vp]),
    'pcp_pointwise_wgrad_workspace_bytes': (c_sz, [c_i64, c_i32, c_i32]),
    'pcp_pointwise_wgrad': (c_i32, [ctypes.POINTER(RowMap), ctypes.POINTER(RowMap), c_i64, vp, c_sz, vp, c_i32, c_i32, vp]),
    'pcp_centerhead_targets': (c_i32, [ctypes.POINTER(Target), vp, c_i32, vp, vp, vp, vp, vp]),
    'pcp_loss_workspace_bytes': (c_sz, []),
    'pcp_centerhead_loss': (c_i32, [ctypes.POINTER(HeadLoss), vp, vp, vp, vp, vp, c_f, vp, vp, vp, vp]),
    'pcp_centerhead_targets_ext': (c_i32, [ctypes.POINTER(Target), ctypes.POINTER(TargetHead), c_i32, vp, c_i32, c_i32, c_i32, vp]),
    'pcp_centerhead_loss_ext_workspace_bytes': (c_sz, [c_i32]),
    'pcp_centerhead_loss_ext': (c_i32, [ctypes.POINTER(HeadLossExt), ctypes.POINTER(HeadLossHead), c_i32, c_f, vp, c_sz, vp, vp, vp]),
    'pcp_anchor_assign_workspace_bytes': (c_sz, [ctypes.POINTER(AnchorAssign), c_i32]),
    'pcp_anchor_assign_targets': (c_i32, [ctypes.POINTER(AnchorAssign), vp, vp, c_i32, vp, c_sz, vp, vp, vp, vp]),
    'pcp_anchor_loss_workspace_bytes': (c_sz, [c_i32]),
    'pcp_anchor_loss': (c_i32, [ctypes.POINTER(AnchorLoss), vp, vp, vp, vp, c_f, vp, c_sz, vp, vp, vp]),
    'pcp_hunter_meta_workspace_bytes': (c_sz, [ctypes.POINTER(HunterMeta), c_i64]),
    'pcp_hunter_meta': (c_i32, [ctypes.POINTER(HunterMeta), vp, c_i64, c_i32, vp, c_sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    'pcp_segment_max': (c_i32, [vp, c_i32, vp, c_i64, vp, c_i64, c_i32, vp, c_i32, vp, vp]),
    'pcp_segment_max_backward': (c_i32, [vp, c_i32, vp, c_i64, c_i32, vp, vp, c_i32, vp]),
    'pcp_rows_scatter_add': (c_i32, [vp, c_i32, vp, c_i64, c_i32, vp, c_i32, vp]),
    'pcp_hunter_local_centroids': (c_i32, [vp, c_i32, vp, vp, c_i32, c_i32, vp, c_sz, vp, vp, c_i32, vp]),
    'pcp_hunter_object_cat': (c_i32, [vp, vp, vp, vp, vp, c_i32, c_i32, vp, c_i32, vp]),
    'pcp_hunter_object_cat_backward': (c_i32, [vp, c_i32, vp, vp, c_i32, c_i32, c_i32, vp, vp, vp]),
    'pcp_hunter_loss_workspace_bytes': (c_sz, [c_i64, c_i32, c_i32, c_i32]),
    'pcp_hunter_losses': (c_i32, [ctypes.POINTER(HunterLoss), vp, c_sz, vp]),
    'pcp_softmax_fuse2_backward': (c_i32, [vp, c_i32, vp, c_i32, vp, c_i32, c_i64, c_i32, vp, c_i32, vp, c_i32, vp]),
    'pcp_bev_scatter_mean_backward': (c_i32, [vp, c_i32, c_i32, c_i32, c_i64, vp, c_i32, c_i32, vp, vp, c_i32, vp, c_i32, vp]),
    'pcp_bev_sample_bilinear_backward': (c_i32, [vp, c_i32, vp, vp, c_i64, c_i32, vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_f, c_f, c_f, c_f, vp,
                                                 c_i32, vp, c_i32, vp]),
    'pcp_filter_gt_boxes': (c_i32, [vp, c_i32, c_i32, ctypes.POINTER(c_f), vp, vp]),
    'pcp_filter_gt_boxes_w': (c_i32, [vp, c_i32, c_i32, c_i32, ctypes.POINTER(c_f), vp, vp]),
    'pcp_distill_loss': (c_i32, [vp, c_i32, vp, c_i32, c_i64, c_i32, c_f, c_f, vp, vp, vp, c_i32, c_i32, vp]),
    'pcp_masked_smooth_l1_rows': (c_i32, [vp, c_i32, vp, c_i32, c_i64, c_i32, c_f, vp, vp, vp]),
    'pcp_pfn_train_features': (c_i32, [vp, c_i64, c_i32, c_i32, ctypes.POINTER(Grid), vp, vp, vp, vp]),
    'pcp_pfn_train_features_w': (c_i32, [vp, c_i64, c_i32, c_i32, c_i32, ctypes.POINTER(Grid), vp, vp, vp, vp]),
    'pcp_pfn_train_mid': (c_i32, [ctypes.POINTER(Grid), vp, c_i64, vp, vp, vp, vp, vp, vp]),
    'pcp_pfn_train_out': (c_i32, [ctypes.POINTER(Grid), vp, c_i64, vp, vp, vp, vp, vp, vp, vp]),
    'pcp_pfn_train_route_out_grad': (c_i32, [ctypes.POINTER(Grid), vp, c_i64, c_i64, vp, vp, vp, vp, vp]),
    'pcp_pfn_train_route_mid_grad': (c_i32, [ctypes.POINTER(Grid), vp, c_i64, vp, vp, vp, vp]),
    'pcp_disco_weight_logits': (c_i32, [ctypes.POINTER(vp), c_i32, c_i32, vp, vp, c_i64, vp, c_i32, vp]),
    'pcp_disco_fuse_backward_workspace_bytes': (c_sz, []),
    'pcp_disco_fuse_backward': (c_i32, [ctypes.POINTER(vp), c_i32, c_i32, c_i32, vp, c_i32, vp, c_i32, ctypes.POINTER(vp), c_i32, vp,
                                        c_i64, vp, c_i32, ctypes.POINTER(vp), vp, vp, vp, c_i32, vp]),
    'pcp_grad_sqnorm': (c_i32, [vp, c_i64, vp, c_i32, vp]),
    'pcp_pack_conv3x3': (c_i32, [vp, c_i32, c_i32, c_i32, vp, c_i32, vp, c_i32, vp, c_i32, vp]),
    'pcp_pack_conv3x3_winograd4': (c_i32, [vp, c_i32, c_i32, c_i32, vp, vp, c_i32, vp]),
    'pcp_pack_conv3x3_group_blocks': (c_i32, [vp]),
    'pcp_pack_conv3x3_group': (c_i32, [vp, c_i32, c_i32, vp]),
    'pcp_adam_step': (c_i32, [vp, vp, vp, vp, c_i64, c_f, c_f, c_f, c_f, c_f, c_i64, c_f, vp, c_f, vp]),
    'pcp_avgpool_nhwc_backward': (c_i32, [vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, vp, c_i32, c_i32, vp]),
    'pcp_sc_gate_backward': (c_i32, [vp, c_i32, vp, c_i32, vp, c_i32, vp, c_i32, c_i32, c_i32, vp, c_i32, vp, c_i32, vp, c_i32, c_i32, vp, c_i32,
                                     c_i32, c_i32, c_i32, c_i32, vp]),
    'pcp_add_relu': (c_i32, [vp, c_i32, vp, c_i32, vp, c_i32, c_i64, c_i32, vp]),
    'pcp_add_relu_backward': (c_i32, [vp, c_i32, vp, c_i32, vp, c_i32, vp, c_i32, c_i64, c_i32, vp]),
    'pcp_world_augment_points_workspace_bytes': (c_sz, [c_i64]),
    'pcp_world_augment_points': (c_i32, [ctypes.POINTER(WorldAug), vp, vp, c_i64, c_i32, vp, vp, vp, c_sz, vp]),
    'pcp_world_augment_boxes': (c_i32, [ctypes.POINTER(WorldAug), vp, vp, c_i32, c_i32, vp, c_i32, c_i32, vp]),
    'pcp_object_augment_boxes': (c_i32, [ctypes.POINTER(ObjectAug), vp, vp, c_i32, c_i32, vp, vp, vp]),
    'pcp_object_augment_points_workspace_bytes': (c_sz, [c_i64]),
    'pcp_object_augment_points': (c_i32, [ctypes.POINTER(ObjectAug), vp, vp, c_i32, vp, vp, c_i64, c_i32, vp, vp, vp, c_sz, vp]),
    'pcp_frame_extent_workspace_bytes': (c_sz, [c_i64, c_i32]),
    'pcp_frame_extent': (c_i32, [vp, c_i64, c_i32, c_i32, c_i32, vp, vp, c_sz, vp]),
    'pcp_object_augment_drop_boxes': (c_i32, [vp, c_i32, c_i32, c_i32, vp, c_i32, c_i32, vp, vp, c_i32, vp, vp, vp, vp, vp]),
    'pcp_gt_sample_select': (c_i32, [vp, c_i32, c_i32, c_i32, vp, c_i32, vp, vp, c_i32, vp, c_i32, vp, c_i32, vp, vp]),
    'pcp_gt_sample_paste_points': (c_i32, [vp, c_i64, c_i32, c_i32, vp, c_i32, vp, c_i32, vp, vp, vp, vp, c_i32, c_i64, vp, vp, vp]),
    'pcp_gt_sample_paste_boxes': (c_i32, [vp, c_i32, c_i32, c_i32, vp, c_i32, c_i32, vp, c_i32, vp, c_i32, vp, vp, vp, vp, vp, c_i32, vp]),
})

# include/pcp_hip_mp.h (mixed-precision training loop, config 5)
SYMBOLS.update({
    'pcp_mp_bn_train_stats': (c_i32, [vp, c_i32, c_i64, c_i32, c_i32, vp, vp, c_f, c_f, vp, vp, vp, vp, vp, vp, vp, vp]),
    'pcp_mp_scale_shift_act': (c_i32, [vp, c_i32, c_i64, c_i32, c_i32, vp, vp, c_i32, vp, c_i32, c_i32, vp]),
    'pcp_mp_bn_act_backward': (c_i32, [vp, c_i32, c_i32, vp, c_i32, c_i32, c_i64, c_i32, vp, vp, vp, vp, c_i32, vp, vp, vp, c_i32, vp, c_i32,
                                       c_i32, vp]),
    'pcp_mp_bn_train_sums': (c_i32, [vp, c_i32, c_i64, c_i32, c_i32, vp, vp, vp]),
    'pcp_mp_bn_bwd_sums': (c_i32, [vp, c_i32, c_i32, vp, c_i32, c_i32, c_i64, c_i32, vp, vp, vp, vp, c_i32, vp, vp, vp]),
    'pcp_mp_bn_bwd_apply_from_sums': (c_i32, [vp, c_i32, c_i32, vp, c_i32, c_i32, c_i64, c_i32, vp, vp, vp, vp, c_i32, vp, vp, c_i64, vp, vp, vp,
                                              c_i32, vp, c_i32, c_i32, vp]),
    'pcp_mp_colsum': (c_i32, [vp, c_i32, c_i64, c_i32, c_i32, vp, vp, c_i32, vp]),
    'pcp_mp_accumulate': (c_i32, [vp, c_i32, c_i32, vp, c_i32, c_i32, c_i64, c_i32, c_f, vp]),
    'pcp_mp_dilate2x': (c_i32, [vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, vp, c_i32, vp]),
    'pcp_mp_pfn_train_mid': (c_i32, [ctypes.POINTER(Grid), vp, c_i64, vp, vp, vp, vp, c_i32, vp, vp]),
    'pcp_mp_pfn_train_out': (c_i32, [ctypes.POINTER(Grid), vp, c_i64, vp, c_i32, vp, vp, vp, vp, vp, c_i32, vp]),
    'pcp_mp_pfn_train_route_out_grad': (c_i32, [ctypes.POINTER(Grid), vp, c_i64, c_i64, vp, c_i32, vp, vp, vp, c_i32, vp]),
    'pcp_mp_pfn_train_route_mid_grad': (c_i32, [ctypes.POINTER(Grid), vp, c_i64, vp, c_i32, vp, vp, vp]),
    'pcp_mp_sparse_conv3x3_s2': (c_i32, [vp, ctypes.POINTER(Grid), vp, c_i64, vp, vp, c_i32, c_i32, vp, c_i32, c_i32, vp]),
    'pcp_mp_conv3x3_packed_bytes': (c_sz, [c_i32, c_i32]),
    'pcp_mp_pack_conv3x3': (c_i32, [vp, c_i32, c_i32, c_i32, vp, vp, c_i32, vp]),
    'pcp_mp_pack_conv3x3_group_blocks': (c_i32, [vp]),
    'pcp_mp_pack_conv3x3_group': (c_i32, [vp, c_i32, c_i32, vp]),
    'pcp_mp_conv3x3': (c_i32, [ctypes.POINTER(MpConv3x3), vp, vp, vp, vp, vp]),
    'pcp_mp_conv3x3_plan': (c_i32, [ctypes.POINTER(MpConv3x3), ctypes.POINTER(c_i32), ctypes.POINTER(ctypes.c_double)]),
    'pcp_mp_conv3x3_wgrad_workspace_bytes': (c_sz, [ctypes.POINTER(MpWgrad3x3)]),
    'pcp_mp_conv3x3_wgrad': (c_i32, [ctypes.POINTER(MpWgrad3x3), vp, vp, vp, vp, c_sz, vp]),
    'pcp_mp_pointwise': (c_i32, [ctypes.POINTER(MpPointwise), vp, vp, vp, vp, vp]),
    'pcp_mp_warp_nearest': (c_i32, [vp, c_i32, vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.POINTER(c_f), c_i32, vp]),
    'pcp_mp_softmax_fuse': (c_i32, [ctypes.POINTER(vp), c_i32, c_i32, vp, c_i32, c_i64, c_i32, c_i32, c_i32, vp, vp]),
    'pcp_mp_disco_fuse_backward': (c_i32, [ctypes.POINTER(vp), c_i32, c_i32, c_i32, c_i32, vp, c_i32, vp, c_i32, ctypes.POINTER(vp), c_i32, vp, c_i64,
                                           vp, c_i32, ctypes.POINTER(vp), vp, vp, vp, c_i32, vp]),
    'pcp_mp_pointwise_wgrad_workspace_bytes': (c_sz, [c_i64, c_i32, c_i32]),
    'pcp_mp_pointwise_wgrad': (c_i32, [ctypes.POINTER(MpRowMap), ctypes.POINTER(MpRowMap), c_i64, vp, c_sz, vp, c_i32, c_i32, vp]),
})
SYMBOLS.update({
    'pcp_hard_voxelize_workspace_bytes': (c_sz, [ctypes.POINTER(Grid), c_i64]),
    'pcp_hard_voxelize': (c_i32, [vp, c_i64, c_i32, ctypes.POINTER(Grid), c_i32, c_i32, c_i64, vp, c_sz, vp, vp, vp, vp]),
    'pcp_hard_voxelize_gather': (c_i32, [vp, c_i64, c_i32, c_i32, ctypes.POINTER(Grid), c_i32, vp, c_sz, c_i64, vp, vp, vp]),
    'pcp_pillar_vfe': (c_i32, [vp, vp, vp, c_i64, c_i32, c_i32, ctypes.c_uint32, ctypes.POINTER(c_f), ctypes.POINTER(c_f), vp, vp, c_i32, vp, vp]),
})
SYMBOLS.update({
    'pcp_mean_vfe_workspace_bytes': (c_sz, [ctypes.POINTER(Grid), c_i64]),
    'pcp_mean_vfe': (c_i32, [vp, c_i64, c_i32, ctypes.POINTER(Grid), c_i32, vp, c_sz, vp, vp, vp]),
    'pcp_mean_vfe_features': (c_i32, [vp, c_i64, c_i32, c_i32, ctypes.POINTER(Grid), c_i32, vp, c_sz, c_i64, vp, vp]),
    'pcp_spconv_table_bytes': (c_sz, [c_i32, c_i32, c_i32, c_i32]),
    'pcp_spconv_table_build': (c_i32, [vp, c_i64, c_i32, c_i32, c_i32, c_i32, vp, c_sz, vp, vp, vp]),
    'pcp_spconv_build_subm': (c_i32, [vp, c_i64, c_i32, c_i32, c_i32, c_i32, vp, c_sz, vp, vp, vp]),
    'pcp_spconv_strided_sites': (c_i32, [vp, c_i64, c_i32, c_i32, c_i32, c_i32, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32),
                                         ctypes.POINTER(c_i32), vp, c_sz, vp, vp]),
    'pcp_spconv_build_strided': (c_i32, [c_i32, c_i32, c_i32, c_i32, vp, c_sz, vp, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32),
                                         ctypes.POINTER(c_i32), vp, c_sz, c_i64, vp, vp, vp]),
    'pcp_spconv3d': (c_i32, [vp, c_i64, c_i32, c_i32, vp, c_i32, c_i64, vp, vp, vp, c_i32, c_i32, vp, vp]),
    'pcp_spconv_dense': (c_i32, [vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, vp, c_sz, vp, vp, vp]),
})
SYMBOLS.update({
    'pcp_spconv_invert_nbr': (c_i32, [vp, c_i32, c_i64, c_i64, vp, vp]),
    'pcp_spconv3d_wgrad_workspace_bytes': (c_sz, [c_i64, c_i32, c_i32, c_i32, c_i32]),
    'pcp_spconv3d_wgrad': (c_i32, [vp, c_i64, c_i32, c_i32, vp, vp, c_i32, c_i64, c_i32, c_i32, vp, c_sz, vp, c_i32, vp]),
    'pcp_spconv_dense_backward': (c_i32, [vp, vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, vp, vp]),
})

# PCP_OPT_* of include/pcp_hip.h.  The C library never reads the environment; the PCP_* variables of earlier rounds are mapped onto the option
# table ONCE, here, when the library is loaded (set_option() changes an option later, e.g. from a test)
OPTIONS = {'pfn_crowd': 0, 'pfn_crowd_blocks': 1, 'pfn_wps': 2, 'wino4c_nw': 3, 'mp_th16_min': 4, 'mp_diag': 5, 'vox_aggregate': 6,
           'conv_s2_form': 7, 'gts_paste_form': 8}
_OPTION_ENV = {'PCP_PFN_CROWD': 'pfn_crowd', 'PCP_PFN_CROWD_BLOCKS': 'pfn_crowd_blocks', 'PCP_PFN_WPS': 'pfn_wps', 'PCP_WINO4C_NW': 'wino4c_nw',
               'PCP_MP_TH16_MIN': 'mp_th16_min', 'PCP_MP_DIAG': 'mp_diag', 'PCP_VOX_AGGREGATE': 'vox_aggregate', 'PCP_CONV_S2_FORM': 'conv_s2_form', 'PCP_GTS_PASTE_FORM': 'gts_paste_form'}

_LIB = None


class PcpError(RuntimeError):
    pass


def load():
    """dlopen the library once; raises (never falls back) when it is absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.isfile(LIB_PATH):
        raise PcpError('libpcp_hip.so not found at %s -- build it with `make -C practical-collab-perception_amd/csrc` '
                       '(or python -c "import __graft_entry__ as g; g.build()"); there is no CPU fallback.' % LIB_PATH)
    import torch  # noqa: F401  -- makes sure torch's own libamdhip64 (same SONAME) is the HIP runtime both sides use
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing: loud by design
        fn.restype = res
        fn.argtypes = args
    if lib.pcp_abi_version() != 1:
        raise PcpError('libpcp_hip.so ABI version mismatch')
    for env, name in _OPTION_ENV.items():
        v = os.environ.get(env, '')
        if v.strip():
            if lib.pcp_set_option(OPTIONS[name], int(v)) != 0:
                raise PcpError('%s=%s: pcp_set_option refused it' % (env, v))
    _LIB = lib
    return lib


def set_option(name, value):
    """override a built-in launch rule of the library (A/B runs, tests); value None restores the rule.  Returns the previous override (None = rule)."""
    lib = load()
    prev = int(lib.pcp_get_option(OPTIONS[name]))
    check(lib.pcp_set_option(OPTIONS[name], -1 if value is None else int(value)), 'pcp_set_option')
    return None if prev < 0 else prev


def check(status, what):
    if status != 0:
        raise PcpError('%s failed: %s' % (what, load().pcp_status_string(status).decode()))
