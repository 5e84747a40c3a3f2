"""ctypes binding of libeffdet_hip.so (include/effdet_hip.h, include/effdet_soft_nms.h, include/effdet_ema.h, include/effdet_dwconv_plan.h,
include/effdet_live_tiles.h, include/effdet_needed_tiles.h, include/effdet_box_loss.h, include/effdet_loss_opts.h, include/effdet_atss.h, include/effdet_conv_plan.h, include/effdet_wbf.h, include/effdet_mosaic.h, include/effdet_affine.h,
include/effdet_opt_groups.h, include/effdet_gate_operand.h, include/effdet_wgrad_plan.h, include/effdet_resample.h, include/effdet_slices.h,
include/effdet_quality_loss.h, include/effdet_tal.h, include/effdet_op_point.h, include/effdet_track.h, include/effdet_assign.h, include/effdet_draw.h).

The library is the product: there is NO CPU / eager fallback.  ``lib()`` raises if the shared
library is missing and every op raises if a call returns a non-zero status.

``SIGNATURES`` declares every entry point's return and parameter types once; ``lib()`` binds them (``restype`` / ``argtypes``) at
load, so no call site casts an argument: ints, floats and addresses (``ptr()``, ``stream_ptr()``, ``ndarray.ctypes.data``) are passed
as they are.  A new entry point is one line in that table.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must be imported first: the .so binds to torch's already-loaded libamdhip64)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('EFFDET_HIP_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libeffdet_hip.so')   # override: A/B experiment builds (tools/)
MAX_SEG = 5
MAX_CONV_SEG = 10                  # effdet_conv_t: 5 pyramid levels x 2 independent convs of one geometry (the head's two towers)
ABI_VERSION = 11                   # EFFDET_ABI_VERSION of include/effdet_hip.h this binding was written against (tests/test_abi.py)
F32, BF16, F32_BF16X3, F32_SPLIT = 0, 1, 2, 3      # F32_BF16X3: fp32 storage, bf16x3 products (conv2d / conv2d_wgrad only); F32_SPLIT: [32 hi | 32 lo] bf16 pairs
F32_HSPLIT = 4                                     # the f16x3 forward arithmetic: [32 x f16 hi | 32 x f16 lo * 2^11] activations, row-scaled f16 hi | lo weights
ACT_NONE, ACT_RELU, ACT_SWISH, ACT_SIGMOID = 0, 1, 2, 3
RES_NONE, RES_ADD, RES_RELU_MASK, RES_SWISH_GRAD = 0, 1, 2, 3
TUNE_IGEMM_BIG, TUNE_IGEMM_BIG_MIN_M, TUNE_SPLIT_PERS, TUNE_IGEMM_KORD, TUNE_SPLIT_KORD = 0, 1, 2, 3, 4
TUNE_ROWSLAB = 5                   # row-slab activation staging of the split-layout 3x3 convs: 1 (default) on, 0 per-tap staging
TUNE_SHORT_TILE = 7                # 32-pixel workgroup tiles for the small-map exact-fp32 / bf16x3 convs: 1 (default) on, 0 the 128-pixel plans (index 6 is no key: EFFDET_EINVAL)

_ERR = {-1: 'EFFDET_EINVAL', -2: 'EFFDET_ELAUNCH', -3: 'EFFDET_EUNSUPPORTED'}


class Seg(C.Structure):
    _fields_ = [('H', C.c_int), ('W', C.c_int), ('Ho', C.c_int), ('Wo', C.c_int),
                ('in_off', C.c_longlong), ('in_bstride', C.c_longlong),
                ('out_off', C.c_longlong), ('out_bstride', C.c_longlong)]


class ConvDesc(C.Structure):
    _fields_ = [('x', C.c_void_p), ('w', C.c_void_p), ('y', C.c_void_p), ('z', C.c_void_p), ('res', C.c_void_p),
                ('scale', C.c_void_p), ('shift', C.c_void_p), ('rowscale', C.c_void_p),
                ('bc_scale', C.c_void_p), ('bc_shift', C.c_void_p),
                ('dtype', C.c_int), ('out_f32', C.c_int),
                ('B', C.c_int), ('Cin', C.c_int), ('Cout', C.c_int), ('KH', C.c_int), ('KW', C.c_int),
                ('stride', C.c_int), ('pad_t', C.c_int), ('pad_l', C.c_int),
                ('ldx', C.c_int), ('ldy', C.c_int), ('act', C.c_int), ('res_mode', C.c_int),
                ('nseg', C.c_int), ('seg', Seg * MAX_CONV_SEG), ('w_image_stride', C.c_longlong), ('y_split', C.c_void_p), ('range_flag', C.c_void_p),
                ('seg_w', C.c_void_p * MAX_CONV_SEG), ('seg_shift', C.c_void_p * MAX_CONV_SEG)]


class WgradDesc(C.Structure):
    _fields_ = [('x', C.c_void_p), ('dz', C.c_void_p), ('dw', C.c_void_p), ('dbias', C.c_void_p),
                ('dtype', C.c_int),
                ('B', C.c_int), ('Cin', C.c_int), ('Cout', C.c_int), ('KH', C.c_int), ('KW', C.c_int),
                ('stride', C.c_int), ('pad_t', C.c_int), ('pad_l', C.c_int),
                ('ldx', C.c_int), ('lddz', C.c_int), ('nseg', C.c_int), ('image_splits', C.c_int), ('seg', Seg * MAX_SEG)]


class PrepJob(C.Structure):      # effdet_prep_job_t
    _fields_ = [('a', C.c_void_p), ('b', C.c_void_p), ('c', C.c_void_p), ('d', C.c_void_p), ('out', C.c_void_p),
                ('kind', C.c_int), ('dtype', C.c_int), ('n0', C.c_int), ('n1', C.c_int), ('n2', C.c_int), ('n3', C.c_int),
                ('n4', C.c_int), ('eps', C.c_float)]


class UnpackJob(C.Structure):    # effdet_unpack_job_t
    _fields_ = [(n, C.c_void_p) for n in ('g', 'scale', 'w_oihw', 'dw_oihw', 'wsum', 'dsum_part', 'mean', 'invstd', 'dgamma', 'dbeta',
                                          'dbias_out', 'slab_scale', 'slab_cscale')] + \
               [(n, C.c_int) for n in ('accumulate', 'Cout', 'Cin', 'KH', 'KW', 'Cin_pad', 'nslabs', 'slabs_per_scale')]


class SeParamJob(C.Structure):   # effdet_se_param_job_t
    _fields_ = [(n, C.c_void_p) for n in ('du', 'dmid', 'sw', 'pool', 'dw1', 'db1', 'dw2', 'db2')] + \
               [('B', C.c_int), ('C', C.c_int), ('Cse', C.c_int), ('inv_hw', C.c_float)]


class DwUnpackJob(C.Structure):  # effdet_dw_unpack_job_t
    _fields_ = [(n, C.c_void_p) for n in ('g_kkc', 'scale', 'w_c1kk', 'dw_c1kk', 'wsum', 'dsum', 'mean', 'invstd', 'dgamma', 'dbeta')] + \
               [('C', C.c_int), ('kk', C.c_int)]


class _TailUnion(C.Union):
    _fields_ = [('conv', UnpackJob), ('se', SeParamJob), ('dw', DwUnpackJob)]


class TailJob(C.Structure):      # effdet_tail_job_t
    _fields_ = [('kind', C.c_int), ('u', _TailUnion)]


class JpegInfo(C.Structure):     # effdet_jpeg_info_t
    _fields_ = [(n, C.c_int) for n in ('width', 'height', 'ncomp', 'sampling', 'restart_interval', 'mcus_x', 'mcus_y')] + \
               [('blocks_w', C.c_int * 3), ('blocks_h', C.c_int * 3), ('reason', C.c_int), ('coef_bytes', C.c_longlong)]


class JpegDesc(C.Structure):     # effdet_jpeg_desc_t
    _fields_ = [(n, C.c_int) for n in ('width', 'height', 'ncomp', 'sampling', 'status')] + \
               [('blocks_w', C.c_int * 3), ('blocks_h', C.c_int * 3), ('idct_wg0', C.c_int), ('rgb_wg0', C.c_int), ('reserved', C.c_int),
                ('coef_off', C.c_longlong * 3), ('qt', (C.c_ushort * 64) * 3)]


class TrainCtl(C.Structure):     # effdet_train_ctl_t
    _fields_ = [(n, C.c_int) for n in ('skip', 'pending', 'applied', 'skipped')] + [('loss_count', C.c_longlong), ('loss_sum', C.c_double)]


class EmaCtl(C.Structure):       # effdet_ema_ctl_t (include/effdet_ema.h)
    _fields_ = [('updates', C.c_int), ('reserved', C.c_int * 3)]


class LossOpts(C.Structure):     # effdet_loss_opts_t (include/effdet_loss_opts.h)
    _fields_ = [(n, C.c_float) for n in ('alpha', 'gamma', 'label_smoothing', 'beta', 'reg_weight', 'pos_iou', 'neg_iou')] + \
               [('low_quality', C.c_int), ('box_kind', C.c_int), ('box_weight', C.c_float)]


ATSS_MAX_LEVELS, ATSS_MAX_TOPK = 8, 16               # EFFDET_ATSS_MAX_LEVELS, EFFDET_ATSS_MAX_TOPK


class Atss(C.Structure):         # effdet_atss_t (include/effdet_atss.h)
    _fields_ = [('topk', C.c_int), ('num_levels', C.c_int), ('level_start', C.c_longlong * (ATSS_MAX_LEVELS + 1))]


QUALITY_QFL, QUALITY_VFL = 1, 2                     # EFFDET_QUALITY_*


class QualityLoss(C.Structure):  # effdet_quality_loss_t (include/effdet_quality_loss.h)
    _fields_ = [('kind', C.c_int), ('beta', C.c_float), ('alpha', C.c_float), ('gamma', C.c_float)]


TAL_MAX_TOPK = 16                                   # EFFDET_TAL_MAX_TOPK


class Tal(C.Structure):          # effdet_tal_t (include/effdet_tal.h)
    _fields_ = [('topk', C.c_int), ('alpha', C.c_float), ('beta', C.c_float), ('aligned_target', C.c_int)]


class ConvPlanInfo(C.Structure):   # effdet_conv_plan_info_t (include/effdet_conv_plan.h)
    _fields_ = [(n, C.c_int) for n in ('id', 'form', 'persistent', 'tile_m', 'tile_n', 'stages', 'threads', 'mtiles', 'ntiles', 'grid',
                                       'ksteps', 'kord', 'lds_bytes', 'm32')] + [('reserved', C.c_int * 2)]


class WgradPlanInfo(C.Structure):   # effdet_wgrad_plan_info_t (include/effdet_wgrad_plan.h)
    _fields_ = [(n, C.c_int) for n in ('path', 'splits', 'nfast', 'mchunk', 'ntiles', 'jtiles', 'stage_pixels', 'allr', 'thin_ns', 'gate',
                                       'nseg')] + [('first', C.c_int * MAX_SEG), ('count', C.c_int * MAX_SEG), ('reserved', C.c_int * 3)]


WBF_MAX_VIEWS, WBF_MAX_IN = 8, 4096                  # EFFDET_WBF_MAX_VIEWS, EFFDET_WBF_MAX_IN


class Wbf(C.Structure):          # effdet_wbf_t (include/effdet_wbf.h)
    _fields_ = [(n, C.c_void_p * WBF_MAX_VIEWS) for n in ('score', 'label', 'boxes', 'count')] + \
               [('A', C.c_longlong * WBF_MAX_VIEWS)] + [(n, C.c_float * WBF_MAX_VIEWS) for n in ('weight', 'width', 'mul')] + \
               [('flip', C.c_int * WBF_MAX_VIEWS)] + [(n, C.c_int) for n in ('V', 'B', 'top_n', 'conf_type')] + \
               [('iou_thr', C.c_float), ('skip_thr', C.c_float)] + \
               [(n, C.c_void_p) for n in ('out_score', 'out_label', 'out_boxes', 'out_count')]


RESAMPLE_NCHW, RESAMPLE_NHWC = 0, 1                  # EFFDET_RESAMPLE_NCHW, EFFDET_RESAMPLE_NHWC


class Resample(C.Structure):     # effdet_resample_t (include/effdet_resample.h)
    _fields_ = [('src', C.c_void_p), ('dst', C.c_void_p)] + \
               [(n, C.c_int) for n in ('src_layout', 'dtype', 'B', 'H', 'W', 'Ho', 'Wo', 'C', 'flip')] + \
               [('src_ld', C.c_longlong), ('src_bstride', C.c_longlong)]


SLICE_MAX_TILES, SLICE_MAX_IN = 1024, 8192           # EFFDET_SLICE_MAX_TILES, EFFDET_SLICE_MAX_IN
SLICE_NMS, SLICE_NMM, SLICE_IOU, SLICE_IOS = 0, 1, 0, 1     # EFFDET_SLICE_* method and metric


class SliceTile(C.Structure):    # effdet_slice_tile_t (include/effdet_slices.h)
    _fields_ = [('x0', C.c_int), ('y0', C.c_int), ('mx', C.c_float), ('my', C.c_float)]


class SliceImages(C.Structure):  # effdet_slice_images_t (include/effdet_slices.h)
    _fields_ = [('src', C.c_void_p), ('dst', C.c_void_p), ('tiles', C.c_void_p)] + \
               [(n, C.c_int) for n in ('src_layout', 'dtype', 'B', 'H', 'W', 'C', 'T', 't0', 't1', 'h', 'w')] + \
               [('src_ld', C.c_longlong), ('src_bstride', C.c_longlong)]


class SliceMerge(C.Structure):   # effdet_slice_merge_t (include/effdet_slices.h)
    _fields_ = [(n, C.c_void_p) for n in ('score', 'label', 'boxes', 'count', 'tiles')] + \
               [(n, C.c_int) for n in ('B', 'TPI', 'R', 'method', 'metric', 'class_aware', 'max_det')] + \
               [(n, C.c_float) for n in ('W', 'H', 'thr', 'skip_thr')] + \
               [(n, C.c_void_p) for n in ('out_score', 'out_label', 'out_boxes', 'out_count')]


TAIL_UNPACK, TAIL_SE_PARAMS, TAIL_DW_UNPACK = 0, 1, 2

_lib = None

# The one place where the C signatures of include/effdet_hip.h live: '<return>:<parameters>' per entry point, in the header's order,
# one letter per C type.  lib() turns each entry into restype / argtypes, so a call site passes plain Python ints and floats and ctypes
# converts (or refuses) them by the declared type; tests/test_abi.py parses the header's prototypes and compares them with this table.
#   i int    q long long    I unsigned    Q unsigned long long    f float    d double    s effdet_stream_t
#   p any pointer (typed or void*, struct, scalar or array): c_void_p takes an int address, None, byref(struct), a ctypes array
#   returns: i, q, z const char*, v void
_CTYPE = {'i': C.c_int, 'q': C.c_longlong, 'I': C.c_uint, 'Q': C.c_ulonglong, 'f': C.c_float, 'd': C.c_double,
          'p': C.c_void_p, 's': C.c_void_p, 'z': C.c_char_p, 'v': None}
SIGNATURES = {
    'effdet_conv2d': 'i:ps',
    'effdet_scale_pack_weight': 'i:pppiiiis',
    'effdet_conv2d_kernel': 'i:p',
    'effdet_tuning_set': 'i:ii',
    'effdet_conv2d_wgrad_workspace_bytes': 'q:p',
    'effdet_conv2d_wgrad_splits': 'i:p',
    'effdet_conv2d_wgrad_seg_slabs': 'i:ppp',
    'effdet_conv2d_wgrad_kernel': 'i:p',
    'effdet_conv2d_wgrad': 'i:ppqs',
    'effdet_pack_conv_weight': 'i:pppiiiiiiis',
    'effdet_unpack_conv_wgrad': 'i:pppppiiiiiiipppis',
    'effdet_unpack_conv_wgrad_bn': 'i:pppppppppiiiiiipis',
    'effdet_unpack_conv_wgrad_batch': 'i:pis',
    'effdet_backward_tail': 'i:pis',
    'effdet_prepare_params': 'i:pppis',
    'effdet_bn_fold': 'i:ppppfpppis',
    'effdet_bn_param_grad': 'i:ppppppis',
    'effdet_dwconv_fwd_pool_groups': 'i:iiiiii',
    'effdet_dwconv_fwd': 'i:pppppppiiiiiiiiiiiis',
    'effdet_mbconv_expand_dw_pool_groups': 'i:iiiii',
    'effdet_mbconv_expand_dw_fwd': 'i:pppppppppiiiiiiiiiiis',
    'effdet_dwconv_dgrad': 'i:pppppiiiiiiiiiiis',
    'effdet_dwconv_wgrad_workspace_bytes': 'q:iiiiiiiiiii',
    'effdet_dwconv_wgrad': 'i:pppppqiiiiiiiiiiiis',
    'effdet_dwconv_bwd_workspace_bytes': 'q:iiiiiiiiiii',
    'effdet_dwconv_bwd': 'i:ppppppppqiiiiiiiiiiis',
    'effdet_pw_bwd_slabs': 'i:qii',
    'effdet_pw_bwd': 'i:ppppppppqiis',
    'effdet_pw_dgrad_se_supported': 'i:qii',
    'effdet_pw_dgrad_se': 'i:ppppppppqiiiis',
    'effdet_dw_pack_weight': 'i:ppiis',
    'effdet_dw_unpack_wgrad': 'i:pppppiis',
    'effdet_dw_unpack_wgrad_bn': 'i:pppppppppiis',
    'effdet_se_gate_fwd': 'i:pipppppppiiifs',
    'effdet_se_gate_fwd_split': 'i:pippppppppiiifs',
    'effdet_channel_scale': 'i:pppiiiqis',
    'effdet_se_dgate_slabs': 'i:q',
    'effdet_se_dgate_from_wgrad': 'i:pppppiiiis',
    'effdet_se_dgate': 'i:pppiiiqis',
    'effdet_se_gate_bwd_workspace_floats': 'q:iii',
    'effdet_se_gate_bwd': 'i:piippppppppppppiiifs',
    'effdet_se_bwd_apply': 'i:pppppiiqis',
    'effdet_act_bwd': 'i:ppppiiiqs',
    'effdet_add_inplace': 'i:ppiqs',
    'effdet_colsum': 'i:ppiqiis',
    'effdet_bifpn_fuse_fwd': 'i:pppppiiiiiiiiis',
    'effdet_bifpn_fuse_fwd2': 'i:ppppppiiiiiiiiips',
    'effdet_bifpn_fuse_bwd': 'i:pppppppiiippiiiiiiiiis',
    'effdet_bifpn_weight_bwd': 'i:pppiis',
    'effdet_anchors': 'i:piis',
    'effdet_num_anchors': 'q:ii',
    'effdet_decode_score': 'i:ppppppiqiffs',
    'effdet_nms_workspace_bytes': 'q:iq',
    'effdet_nms': 'i:ppffpppqiqs',
    'effdet_gather_dets': 'i:ppppppppiqs',
    'effdet_loss_workspace_bytes': 'q:iqi',
    'effdet_focal_loss_fwd': 'i:ppppppqiqiis',
    'effdet_focal_loss_bwd': 'i:ppppppppiiqiis',
    'effdet_focal_loss_bwd_pix': 'i:pppppppipiiqiis',
    'effdet_focal_loss_fwd_grad': 'i:ppppppqpiiiqiis',
    'effdet_focal_loss_bwd_reg': 'i:ppppppiiiqis',
    'effdet_opt_chunk': 'i:',
    'effdet_clip_adamw_step': 'i:pppppppiippffffffips',
    'effdet_train_gate': 'i:pps',
    'effdet_grad_accumulate': 'i:pppppiips',
    'effdet_clip_adamw_step_gated': 'i:ppppppppiippffffffpps',
    'effdet_pad_rows': 'i:ppiqqiiiiis',
    'effdet_to_split': 'i:ppqs',
    'effdet_to_split2': 'i:pppqps',
    'effdet_nhwc_to_nchw_f32': 'i:ppiiiiis',
    'effdet_nchw_f32_to_nhwc': 'i:ppiiiiiis',
    'effdet_drop_connect_scales': 'i:ppiiQQps',
    'effdet_philox4x32_10': 'v:ppp',
    'effdet_preprocess_batch': 'i:pppppppiiiiipps',
    'effdet_finalize_dets': 'i:pppppfiippiqs',
    'effdet_voc_match': 'i:ppppiiiidppps',
    'effdet_voc_ap_workspace_bytes': 'q:q',
    'effdet_voc_ap': 'i:ppqpipqppppps',
    'effdet_coco_slots': 'q:iii',
    'effdet_coco_match': 'i:ppppiiiipipiipppppps',
    'effdet_coco_accumulate_workspace_bytes': 'q:qi',
    'effdet_coco_accumulate': 'i:pppppqIpipipiipipqppps',
    'effdet_augment_train': 'i:ppppiippppiipps',
    'effdet_augment_resize': 'i:pppiiippiipps',
    'effdet_augment_boxes': 'i:ppiiipiddpps',
    'effdet_jpeg_probe': 'i:pqp',
    'effdet_jpeg_entropy_batch': 'i:ppipqppip',
    'effdet_jpeg_reconstruct': 'i:ppiiipppps',
    'effdet_head_out_bwd': 'i:pppppiqqs',
    'effdet_version': 'z:',
    'effdet_abi_version': 'i:',
}
SYMBOLS = list(SIGNATURES)
# Entry points added within ABI generation 11, declared in include/effdet_soft_nms.h (same letters; tests/test_soft_nms_host.py compares
# this table with that header's prototypes).  A library of the generation built before them lacks the symbols: callers go through
# require().
ADDED_SIGNATURES = {
    'effdet_soft_nms_workspace_bytes': 'q:iqi',
    'effdet_soft_nms': 'i:pppffifiiippppqiqs',
}
# The parameter EMA of the clip + AdamW step and the in-place weight swap, declared in include/effdet_ema.h (same generation, same
# letters, same rule: callers go through require(); tests/test_ema_host.py compares this table with that header's prototypes).
EMA_SIGNATURES = {
    'effdet_clip_adamw_step_ema': 'i:ppppppppiippffffffifipps',
    'effdet_clip_adamw_step_gated_ema': 'i:pppppppppiippfffffffippps',
    'effdet_ema_swap': 'i:pppppiis',
}
# The host-only query of the depthwise launch plans, declared in include/effdet_dwconv_plan.h (same generation, same letters, same
# rule; tests/test_dwconv_cases_host.py compares this table with that header's prototype).
PLAN_SIGNATURES = {
    'effdet_dwconv_plan_info': 'i:iiiiiiiiiiiiip',
}
# The liveness flags of the sparse regression-tower gradients and the two launches that take them, declared in
# include/effdet_live_tiles.h (same generation, same letters, same rule; tests/test_live_tiles_host.py compares this table with that
# header's prototypes).
LIVE_SIGNATURES = {
    'effdet_live_tiles_counts': 'q:iipppp',
    'effdet_live_tiles': 'i:piiiippppps',
    'effdet_conv2d_live': 'i:ppis',
    'effdet_conv2d_wgrad_live': 'i:ppqps',
}
# The positive-pixel map, the flags derived from it and the conv launch that skips the tiles nobody reads (the sparse regression-tower
# FORWARD), declared in include/effdet_needed_tiles.h (same generation, same letters, same rule; tests/test_needed_tiles_host.py
# compares this table with that header's prototypes).
NEEDED_SIGNATURES = {
    'effdet_positive_pixel_map': 'i:ppiqiippps',
    'effdet_live_tiles_from_map': 'i:piippppps',
    'effdet_conv2d_needed': 'i:ppis',
}
# The compacted 32-pixel unit lists and the flagged conv launches in the gathered form, declared in include/effdet_unit_lists.h (same
# generation, same letters, same rule; tests/test_unit_lists_host.py compares this table with that header's prototypes).
UNIT_LISTS_SIGNATURES = {
    'effdet_unit_lists': 'i:ppqqpps',
    'effdet_conv2d_needed_units': 'i:pppppis',
    'effdet_conv2d_live_units': 'i:pppppis',
}
UNIT_COUNTS = 4                    # EFFDET_UNIT_COUNTS
# The IoU-family box regression losses, declared in include/effdet_box_loss.h (same generation, same letters, same rule;
# tests/test_box_loss_host.py compares this table with that header's prototypes).
BOX_LOSS_SIGNATURES = {
    'effdet_box_loss_fwd': 'i:ppppppqiqiiifs',
    'effdet_box_loss_fwd_grad': 'i:ppppppqpiiiqiiifs',
    'effdet_box_loss_bwd_reg': 'i:ppppppiiiqiifs',
}
# The options of the detection loss (focal alpha / gamma, label smoothing, smooth-L1 knee and weight, matcher bands, low-quality
# matches), declared in include/effdet_loss_opts.h (same generation, same letters, same rule; tests/test_loss_options_host.py compares
# this table with that header's prototypes).  The options travel as a LossOpts struct in host memory (byref).
LOSS_OPTS_SIGNATURES = {
    'effdet_loss_opts_workspace_bytes': 'q:iqii',
    'effdet_loss_opts_fwd': 'i:ppppppqiqiips',
    'effdet_loss_opts_fwd_grad': 'i:ppppppqpiiiqiips',
    'effdet_loss_opts_bwd_cls': 'i:pppppiiiqiips',
    'effdet_loss_opts_bwd_reg': 'i:ppppppiiiqips',
}
# The ATSS matcher of the detection loss, declared in include/effdet_atss.h (same generation, same letters, same rule;
# tests/test_atss_host.py compares this table and Atss with that header).  The forward twins of effdet_loss_opts_fwd / _fwd_grad with
# an Atss struct (host memory, byref) between the options and the stream; the backward calls are the options' own.
ATSS_SIGNATURES = {
    'effdet_loss_atss_workspace_bytes': 'q:iqiip',
    'effdet_loss_atss_fwd': 'i:ppppppqiqiipps',
    'effdet_loss_atss_fwd_grad': 'i:ppppppqpiiiqiipps',
}
# The IoU-aware class losses (quality focal / varifocal), declared in include/effdet_quality_loss.h (same generation, same letters, same
# rule; tests/test_quality_loss_host.py compares this table and QualityLoss with that header).  The twins of effdet_loss_opts_fwd /
# _fwd_grad / _bwd_cls with an Atss struct or NULL (the forward calls) and a QualityLoss struct (host memory, byref) in front of the stream.
QUALITY_LOSS_SIGNATURES = {
    'effdet_loss_quality_workspace_bytes': 'q:iqiip',
    'effdet_loss_quality_fwd': 'i:ppppppqiqiippps',
    'effdet_loss_quality_fwd_grad': 'i:ppppppqpiiiqiippps',
    'effdet_loss_quality_bwd_cls': 'i:pppppiiiqiipps',
}
# The task-aligned matcher of the detection loss, declared in include/effdet_tal.h (same generation, same letters, same rule;
# tests/test_tal_host.py compares this table and Tal with that header).  The forward twins of effdet_loss_quality_fwd / _fwd_grad with a
# Tal struct (host memory, byref) in the place of the Atss one and a QualityLoss struct or NULL; the backward calls are the options' and
# the quality loss's own.  effdet_loss_tal_metrics: the inspection call.
TAL_SIGNATURES = {
    'effdet_loss_tal_workspace_bytes': 'q:iqiip',
    'effdet_loss_tal_fwd': 'i:ppppppqiqiippps',
    'effdet_loss_tal_fwd_grad': 'i:ppppppqpiiiqiippps',
    'effdet_loss_tal_metrics': 'i:pppppiqiips',
}
# The host-only query of the dense-conv launch plan, declared in include/effdet_conv_plan.h (same generation, same letters, same rule;
# tests/test_conv_plan_cases_host.py compares this table and ConvPlanInfo with that header).
CONV_PLAN_SIGNATURES = {
    'effdet_conv2d_plan_info': 'i:pp',
}
# Weighted Boxes Fusion of several views' detection lists, declared in include/effdet_wbf.h (same generation, same letters, same rule;
# tests/test_wbf_host.py compares this table and Wbf with that header).  The views, options and outputs travel as a Wbf struct in host
# memory (byref).
WBF_SIGNATURES = {
    'effdet_wbf_workspace_bytes': 'q:iii',
    'effdet_wbf': 'i:ppqs',
}
# Mosaic and MixUp in front of the 'train' augmentation chain, declared in include/effdet_mosaic.h (same generation, same letters, same
# rule; tests/test_mosaic_host.py compares this table with that header's prototypes).
MOSAIC_SIGNATURES = {
    'effdet_mosaic_compose': 'i:ppppiiips',
    'effdet_mosaic_boxes': 'i:ppiipiffpips',
}
# The random affine / perspective warp between the mosaic stage and the 'train' chain, declared in include/effdet_affine.h (same
# generation, same letters, same rule; tests/test_affine_host.py compares this table with that header's prototypes).
AFFINE_SIGNATURES = {
    'effdet_affine_warp': 'i:ppppiiips',
    'effdet_affine_boxes': 'i:ppiipidddpps',
}
# Two weight gradients of one geometry as one launch, declared in include/effdet_wgrad_pair.h (same generation, same letters, same
# rule; tests/test_wgrad_pair_host.py compares this table with that header's prototype).
WGRAD_PAIR_SIGNATURES = {
    'effdet_conv2d_wgrad_pair': 'i:pppqps',
}
# Parameter groups and the SGD rule of the fused optimizer step, declared in include/effdet_opt_groups.h (same generation, same letters,
# same rule; tests/test_opt_groups_host.py compares this table with that header's prototype).
OPT_GROUPS_SIGNATURES = {
    'effdet_opt_step_groups': 'i:iippppppppppiiipppfiipps',
}
# The squeeze-excite gate applied in the project conv's operand registers (forward and per-image weight gradient), declared in
# include/effdet_gate_operand.h (same generation, same letters, same rule; tests/test_gate_operand_host.py compares this table with that
# header's prototypes).
GATE_OPERAND_SIGNATURES = {
    'effdet_conv2d_gated': 'i:ppis',
    'effdet_conv2d_gated_plan_info': 'i:ppip',
    'effdet_conv2d_wgrad_gated': 'i:ppipqs',
    'effdet_conv2d_wgrad_gated_kernel': 'i:ppi',
}
# The host-only query of the weight-gradient launch plan, declared in include/effdet_wgrad_plan.h (same generation, same letters, same
# rule; tests/test_wgrad_plan_cases_host.py compares this table and WgradPlanInfo with that header).
WGRAD_PLAN_SIGNATURES = {
    'effdet_conv2d_wgrad_plan_info': 'i:pp',
}
# The model-input resampler (scaled TTA views, mixed-size ensembles), declared in include/effdet_resample.h (same generation, same
# letters, same rule; tests/test_resample_host.py compares this table and Resample with that header).  The geometry travels as a
# Resample struct in host memory (byref).
RESAMPLE_SIGNATURES = {
    'effdet_resample_images': 'i:ps',
}
# Sliced inference (tile extractor, cross-tile merge), declared in include/effdet_slices.h (same generation, same letters, same rule;
# tests/test_slices_host.py compares this table and SliceTile / SliceImages / SliceMerge with that header).  Geometry and options travel
# as structs in host memory (byref).
SLICES_SIGNATURES = {
    'effdet_slice_images': 'i:ps',
    'effdet_slice_merge_workspace_bytes': 'q:iii',
    'effdet_slice_merge': 'i:ppqs',
}
# Operating-point metrics (confidence curves, confusion matrix), declared in include/effdet_op_point.h (same generation, same letters,
# same rule; tests/test_op_point_host.py compares this table with that header's prototypes).
OP_POINT_SIGNATURES = {
    'effdet_op_curves_workspace_bytes': 'q:q',
    'effdet_op_curves': 'i:ppqpipipqppppppps',
    'effdet_confusion_match': 'i:ppppiiiifdps',
}
OP_MAX_THRESHOLDS = 4096                                                                         # EFFDET_OP_MAX_THRESHOLDS
# Multi-object tracking (ByteTrack over finalize_dets' rows), declared in include/effdet_track.h (same generation, same letters, same
# rule; tests/test_track_host.py compares this table with that header's prototypes).
TRACK_SIGNATURES = {
    'effdet_track_state_bytes': 'q:ii',
    'effdet_track_reset': 'i:piips',
    'effdet_track_step': 'i:ppiipiffffffiiippps',
    'effdet_track_overflow': 'i:piips',
}
TRACK_MAX_TRACKS, TRACK_MAX_DET, TRACK_ROW_WORDS = 256, 128, 28                                  # EFFDET_TRACK_*
# Optimal assignment (the batched op and the tracker's assignment stage), declared in include/effdet_assign.h (same generation, same
# letters, same rule; tests/test_assign_host.py compares this table with that header's prototypes).
ASSIGN_SIGNATURES = {
    'effdet_assign': 'i:piiippfppps',
    'effdet_track_step_assign': 'i:ppiipiffffffiiipppis',
}
ASSIGN_MAX_ROWS, ASSIGN_MAX_COLS, ASSIGN_SCALE_BITS = 256, 128, 20                               # EFFDET_ASSIGN_*
ASSIGNMENTS = ('greedy', 'optimal')                                                              # EFFDET_ASSIGN_GREEDY, _OPTIMAL in order
# The device renderer (boxes, fills and labels into uint8 frames), declared in include/effdet_draw.h (same generation, same letters,
# same rule; tests/test_draw_host.py compares this table with that header's prototypes).
DRAW_SIGNATURES = {
    'effdet_draw_detections': 'i:pppiiipiipppppipiiiiiiiis',
    'effdet_draw_glyph': 'Q:i',
}
DRAW_MAX_ROWS, DRAW_NAME_MAX, DRAW_MAX_THICKNESS, DRAW_MAX_TEXT_SCALE, DRAW_TEXT_MAX = 1024, 16, 16, 8, 32     # EFFDET_DRAW_*
DRAW_TILE_W, DRAW_TILE_H, DRAW_MAX_SIDE, DRAW_MAX_BATCH = 64, 16, 1 << 20, 65535
WGRAD_PATHS = ('tiled', 'thin', 'split', 'stem')                                                # EFFDET_WGRAD_PATH_* in order
OPT_ROW, OPT_RULE_ADAMW, OPT_RULE_SGD, OPT_GATED, OPT_EMA = 8, 0, 1, 1, 2      # EFFDET_OPT_* of that header
CONV_FORMS = ('plain', 'bf16x3', 'split', 'hsplit', 'skinny')                                     # EFFDET_CONV_FORM_* in order
LIVE_RADII = 6                     # EFFDET_LIVE_RADII: flags for dilation radius 0 .. 5
DW_PLAN_FWD, DW_PLAN_DGRAD, DW_PLAN_WGRAD, DW_PLAN_BWD, DW_PLAN_EXPAND_FWD = 0, 1, 2, 3, 4      # EFFDET_DW_PLAN_*
DW_INFO = ('cq', 'tpi', 'ppt', 'nbuf', 'groups', 'nslab', 'direct')                              # EFFDET_DW_INFO_* in order


def lib():
    """Load (once) and return the HIP library; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'libeffdet_hip.so is missing (%s). Build it with `python -m efficientdet.pytorch_amd.build` '
                '(or __graft_entry__.build()). There is no CPU fallback for this path.' % LIB_PATH)
        cand = C.CDLL(LIB_PATH)
        # a stale build (or a foreign EFFDET_HIP_LIB) with other signatures would be called with shifted arguments: refuse it
        got = int(cand.effdet_abi_version()) if hasattr(cand, 'effdet_abi_version') else 0
        if got != ABI_VERSION:
            raise RuntimeError('%s has ABI generation %d, this binding needs %d: rebuild it (`python -m efficientdet.pytorch_amd.build`)'
                               % (LIB_PATH, got, ABI_VERSION))
        _lib = cand
        for name, sig in list(SIGNATURES.items()) + list(ADDED_SIGNATURES.items()) + list(EMA_SIGNATURES.items()) + \
                list(PLAN_SIGNATURES.items()) + list(LIVE_SIGNATURES.items()) + list(BOX_LOSS_SIGNATURES.items()) + \
                list(LOSS_OPTS_SIGNATURES.items()) + list(ATSS_SIGNATURES.items()) + list(CONV_PLAN_SIGNATURES.items()) + \
                list(WBF_SIGNATURES.items()) + list(NEEDED_SIGNATURES.items()) + list(MOSAIC_SIGNATURES.items()) + \
                list(WGRAD_PAIR_SIGNATURES.items()) + list(OPT_GROUPS_SIGNATURES.items()) + list(GATE_OPERAND_SIGNATURES.items()) + \
                list(WGRAD_PLAN_SIGNATURES.items()) + list(AFFINE_SIGNATURES.items()) + list(RESAMPLE_SIGNATURES.items()) + \
                list(UNIT_LISTS_SIGNATURES.items()) + list(SLICES_SIGNATURES.items()) + list(QUALITY_LOSS_SIGNATURES.items()) + \
                list(TAL_SIGNATURES.items()) + list(OP_POINT_SIGNATURES.items()) + list(TRACK_SIGNATURES.items()) + \
                list(ASSIGN_SIGNATURES.items()) + list(DRAW_SIGNATURES.items()):
            f = getattr(_lib, name, None)      # an additive entry point the library predates stays unbound: require() refuses it
            if f is not None:
                f.restype, f.argtypes = _CTYPE[sig[0]], [_CTYPE[c] for c in sig[2:]]
    return _lib


def require(*names):
    """-> lib(), after checking that it exports every one of names: a library built before an additive entry point (same ABI
    generation, fewer symbols) is refused with the rebuild message instead of a ctypes AttributeError at the call."""
    L = lib()
    missing = [n for n in names if not hasattr(L, n)]
    if missing:
        raise RuntimeError('%s does not export %s: it predates this binding, rebuild it (`python -m efficientdet.pytorch_amd.build`)'
                           % (LIB_PATH, ', '.join(missing)))
    return L


def check(status, what):
    if status != 0:
        raise RuntimeError('%s failed: %s (%d)' % (what, _ERR.get(status, 'unknown'), status))


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream_ptr():
    """hipStream_t of torch's current stream on the current device (every launch asks: the raw-handle query is ~0.3 us, the
    torch.cuda.current_stream() object ~9 us -- 1.2 ms of host time per eager D0 train step)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """Device address of tensor t as an int (None for no tensor: a null pointer)."""
    return None if t is None else t.data_ptr()


def dtype_code(t):
    if t == torch.float32:
        return F32
    if t == torch.bfloat16:
        return BF16
    raise TypeError('unsupported storage dtype %s' % t)
