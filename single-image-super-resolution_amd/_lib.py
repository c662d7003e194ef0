"""ctypes binding of libsisr_hip.so (C ABI: include/sisr_hip.h).

The library is the product: there is NO CPU or eager-PyTorch fallback.  If it is missing or does
not match this mirror of the header, importing the hot path raises.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
LIB_PATH = os.environ.get('SISR_LIB') or os.path.join(CSRC, 'libsisr_hip.so')      # SISR_LIB: developer builds

# enums (sisr_hip.h)
PRO_NONE, PRO_ACT, PRO_AFFINE_ACT, PRO_BNBWD, PRO_BNACT_BWD, PRO_ACT_BWD, PRO_TANH_BWD, PRO_RES_AFFINE = range(8)
X_NHWC, X_NCHW, X_UNSHUFFLE2 = range(3)
Y_NHWC, Y_NCHW, Y_SHUFFLE2 = range(3)
EPI_NONE, EPI_TANH = range(2)
JPEG_444, JPEG_420 = range(2)                # subsampling codes of sisr_jpeg_fwd / sisr_jpeg_bwd
JPEG_GRAD_STE, JPEG_GRAD_CUBIC = range(2)
PIX_L1, PIX_CHARBONNIER, PIX_MSE = range(3)  # pix_kind of sisr_image_loss_fwd / sisr_image_loss_bwd
FREQ_L1, FREQ_CHARBONNIER, FREQ_FOCAL = range(3)   # kind of sisr_freq_loss_fwd / sisr_freq_loss_bwd
FREQ_MAX_SIDE = 256                          # SISR_FREQ_MAX_SIDE: the longest view side the DFT kernels take
ARTIFACT_MAX_K = 11                          # SISR_ARTIFACT_MAX_K: the largest window of sisr_artifact_fwd
PERCEP_MAX_TAPS = 8                          # SISR_PERCEP_MAX_TAPS: the most taps sisr_percep_* take
PERCEP_L1, PERCEP_L2, PERCEP_FRO = range(3)  # crit codes of sisr_percep_fwd / sisr_percep_bwd
CX_MAX_POINTS = 2304                         # SISR_CX_MAX_POINTS: the most points (H W) of a tap sisr_cx_* take
CX_WS_TABLES, CX_WS_SIM, CX_WS_FWD, CX_WS_BWD = range(4)    # `which` of sisr_cx_ws_bytes
GAUSS_MAX_K = 63                             # SISR_GAUSS_MAX_K: the longest filter of sisr_gauss_blur_* / sisr_usm_fwd
RESIZE_AREA, RESIZE_BILINEAR, RESIZE_BICUBIC = range(3)      # mode codes of sisr_resize_fwd / sisr_resize_bwd
RESIZE_MAX_TAPS = 64                         # SISR_RESIZE_MAX_TAPS: the row length of sisr_resize_taps_host's table
NIQE_MAX_BLOCK, NIQE_FEATURES, NIQE_TABLE = 96, 36, 9801   # SISR_NIQE_*: the largest block, the features of a block, the entries of the alpha table
ROUTE_GENERIC, ROUTE_DEEP, ROUTE_TOIMAGE, ROUTE_TRUNK, ROUTE_THIN = range(5)      # enum SisrRoute: what the sisr_*_route calls answer

_f = C.c_void_p      # device pointers travel as void*
_i32 = C.c_int32
_i64 = C.c_int64
_f32 = C.c_float


class ConvPlan(C.Structure):
    _fields_ = [(n, _i32) for n in (
        'TH', 'TW', 'TN', 'tiles_y', 'tiles_x', 'n_groups', 'n_tiles', 'CK', 'PS', 'KROWP', 'n_chunk',
        'CoutPad', 'msub', 'nsub', 'lds_bytes', 'wpk_elems', 'variant')] + [
        (n, C.c_uint32) for n in ('m_tiles_x', 'm_thw', 'm_tw', 'm_iw', 'm_wrow')]


class DeepPlan(C.Structure):
    _fields_ = ([(n, _i32) for n in ('enabled', 'TH', 'TW', 'tiles_x', 'tiles_q', 'BN', 'n_ntiles', 'n_chunk', 'split', 'cps',
                                     'PR', 'IW', 'IH_max', 'NIT', 'wimg_elems', 'classes')] +
                [('ws_bytes', _i64)] +
                [(n, C.c_uint32) for n in ('m_tiles_x', 'm_tw', 'm_ho', 'm_pr', 'm_iw', 'rsv2')])


class ConvDesc(C.Structure):
    _fields_ = ([(n, _f) for n in ('x1', 'x2', 'pa', 'pb', 'pd', 'ps', 'pt', 'wpk', 'bias', 'res', 'y',
                                   'stat_part', 'cnt_part', 'bnb_x', 'bnb_scale', 'bnb_shift', 'bnb_mean',
                                   'bnb_invstd', 'bnb_slope_p', 'bnb_part', 'x_out',
                                   'fin_stat', 'fin_cnt', 'fin_gamma', 'fin_beta', 'fin_rm', 'fin_rv', 'fin_k')] +
                [(n, _i32) for n in ('N', 'H', 'W', 'Cin', 'Ho', 'Wo', 'Cout', 'KH', 'KW', 'stride',
                                     'pad_y', 'pad_x', 'x_mode', 'pro_mode')] +
                [('pro_slope_p', _f), ('pro_slope', _f32)] +
                [('y_mode', _i32), ('epi_act', _i32), ('bnb_act', _i32), ('bnb_slope', _f32)] +
                [(n, _i32) for n in ('y_sy', 'y_oy', 'y_sx', 'y_ox', 'y_H', 'y_W')] +
                [(n, _i32) for n in ('x_bf16', 'y_bf16', 'res_bf16', 'bnbx_bf16')] +
                [('fin_rows', _i32), ('fin_momentum', _f32), ('fin_eps', _f32), ('mfma_split', _i32)] +
                [('plan', ConvPlan)] +
                [('wdeep', _f), ('deep_ws', _f), ('epi_scale_p', _f), ('wdeep_c', _f * 4), ('deep_ckh', _i32 * 4), ('deep', DeepPlan)])


class WgradDeepPlan(C.Structure):
    _fields_ = ([(n, _i32) for n in ('enabled', 'TH', 'TW', 'tiles_x', 'tiles_q', 'n_tiles', 'PR', 'IW', 'IH_max', 'IWd', 'IHd_max',
                                     'NPOS_max', 'XP_max', 'NITX', 'NITD', 'n_pb', 'tiles_per_pb', 'n_cib', 'n_cob', 'lds_bytes', 'slab_bf16', 'batch_first_wg')] +
                [(n, C.c_uint32) for n in ('m_tiles_x', 'm_tw', 'm_ho', 'm_pr', 'm_iw', 'm_iwd')])


class WgradDesc(C.Structure):
    _fields_ = ([(n, _f) for n in ('x1', 'x2', 'pa', 'pb', 'pd', 'ps', 'pt',
                                   'g1', 'g2', 'qa', 'qb', 'qd', 'qs', 'qt', 'slab', 'bias_slab')] +
                [(n, _i32) for n in ('N', 'H', 'W', 'Cin', 'Ho', 'Wo', 'Cout', 'KH', 'KW', 'stride',
                                     'pad_y', 'pad_x', 'x_mode', 'pro_mode')] +
                [('pro_slope_p', _f), ('pro_slope', _f32), ('g_mode', _i32), ('gpro_mode', _i32),
                 ('gpro_slope_p', _f), ('gpro_slope', _f32)] +
                [(n, _i32) for n in ('TH', 'TW', 'TN', 'tiles_y', 'tiles_x', 'n_groups', 'n_tiles',
                                     'CK', 'PS', 'KROWP', 'n_chunk', 'CoutPad',
                                     'NJ', 'NP', 'NT', 'TSTEP', 'TVALID',
                                     'grid_x', 'n_slabs', 'slab_elems', 'lds_bytes')] +
                [(n, C.c_uint32) for n in ('m_tiles_x', 'm_tiles_y', 'm_iw', 'm_twp', 'm_kw')] +
                [('x_bf16', _i32), ('g_bf16', _i32), ('mfma_split', _i32)] +
                [('slab_stride', _i64), ('deep', WgradDeepPlan)])


WIMG_F32, WIMG_BF16, WIMG_DEEP = range(3)
WEIGHT_IMAGES = 5


class WeightImage(C.Structure):
    _fields_ = [('dst', _f)] + [(n, _i32) for n in ('format', 'transposed', 'KH', 'KW', 'R0y', 'Sy', 'R0x', 'Sx',
                                                    'CK', 'PS', 'KROWP', 'n_chunk', 'CoutPad', 'extra')]


class WeightDesc(C.Structure):
    _fields_ = ([(n, _f) for n in ('w_orig', 'u', 'v', 'u_used', 'v_used', 'sigma', 'sn_work')] +
                [(n, _i32) for n in ('Cout', 'Cin', 'KH', 'KW', 'training', 'shuffle2', 'wdp_scaled')] +
                [('img', WeightImage * WEIGHT_IMAGES)])


class WeightGradDesc(C.Structure):
    _fields_ = ([(n, _f) for n in ('dwpk', 'w_orig', 'u_used', 'v_used', 'sigma', 'grad', 'dbias_pk',
                                   'grad_bias')] +
                [(n, _i32) for n in ('Cout', 'Cin', 'KH', 'KW', 'shuffle2', 'CK', 'PS', 'KROWP', 'n_chunk',
                                     'CoutPad', 'layout')])


class AdamDesc(C.Structure):
    _fields_ = [('p', _f), ('m', _f), ('v', _f), ('g', _f), ('numel', _i64), ('block_start', _i64)]


class EmaDesc(C.Structure):
    _fields_ = [('ema', _f), ('src', _f), ('numel', _i64), ('block_start', _i64), ('mode', _i32), ('pad', _i32)]


class ImageRec(C.Structure):
    _fields_ = [('offset', _i64), ('H', _i32), ('W', _i32)]


class DegradeMix(C.Structure):
    _fields_ = ([('K', _i32), ('ksize_min', _i32), ('blur_prob', _f32), ('sinc_prob', _f32), ('kernel_probs', _f32 * 6)] +
                [(n, _f32) for n in ('sigma_lo', 'sigma_hi', 'beta_g_lo', 'beta_g_hi', 'beta_p_lo', 'beta_p_hi', 'noise_lo', 'noise_hi',
                                     'shot_lo', 'shot_hi', 'gaussian_prob', 'grey_prob', 'final_sinc_prob')])


class BnBwdDesc(C.Structure):
    _fields_ = ([(n, _f) for n in ('dy', 'x', 'scale', 'shift', 'mean', 'invstd', 'gamma', 'work',
                                   'qa', 'qb', 'qd', 'dgamma', 'dbeta', 'dslope')] +
                [('P', _i64), ('C', _i32), ('act_mode', _i32), ('slope_p', _f), ('slope', _f32),
                 ('grid', _i32), ('dy_bf16', _i32), ('x_bf16', _i32)])


class ToImageBwdDesc(C.Structure):
    _fields_ = ([(n, _f) for n in ('pre', 'dy', 'out', 'wpk', 'slope_p', 'g', 'slab', 'bias_slab', 'dslope_part', 'dslope')] +
                [(n, _i32) for n in ('N', 'H', 'W', 'Cin', 'Cout', 'KH', 'KW', 'stride', 'pad_y', 'pad_x', 'pre_bf16', 'g_bf16',
                                     'w_CK', 'w_PS', 'w_KROWP', 'w_CoutPad', 'CK', 'PS', 'KROWP', 'n_chunk', 'CoutPad', 'slab_elems')] +
                [('slope', _f32), ('slab_stride', _i64)])


_SIGS = {
    'sisr_conv2d_plan': [C.POINTER(ConvDesc)],
    'sisr_conv2d_f32': [C.POINTER(ConvDesc), _f],
    'sisr_wgrad_plan': [C.POINTER(WgradDesc), _i32],
    'sisr_conv2d_wgrad_f32': [C.POINTER(WgradDesc), _f],
    'sisr_conv2d_plan_bf16': [C.POINTER(ConvDesc)],
    'sisr_conv2d_bf16': [C.POINTER(ConvDesc), _f],
    'sisr_conv2d_deep_plan': [C.POINTER(ConvDesc), _i32, _i32, _i32],
    'sisr_conv2d_deep_eligible': [C.POINTER(ConvDesc)],
    'sisr_conv2d_trunk_eligible': [C.POINTER(ConvDesc)],
    'sisr_conv2d_bf16_parts': [C.POINTER(ConvDesc)],
    'sisr_conv2d_trunk_f32_eligible': [C.POINTER(ConvDesc)],
    'sisr_conv2d_f32_parts': [C.POINTER(ConvDesc)],
    'sisr_conv2d_f32_bnb_parts': [C.POINTER(ConvDesc)],
    'sisr_conv2d_thin_eligible': [C.POINTER(ConvDesc)],
    'sisr_conv2d_toimage_eligible': [C.POINTER(ConvDesc)],
    'sisr_conv2d_toimage_f32_eligible': [C.POINTER(ConvDesc)],
    'sisr_wgrad_trunk_eligible': [C.POINTER(WgradDesc)],
    'sisr_wgrad_bf16_slabs': [C.POINTER(WgradDesc)],
    'sisr_wgrad_trunk_f32_eligible': [C.POINTER(WgradDesc)],
    'sisr_wgrad_f32_slabs': [C.POINTER(WgradDesc)],
    'sisr_wgrad_thin_eligible': [C.POINTER(WgradDesc)],
    'sisr_wgrad_toimage_eligible': [C.POINTER(WgradDesc)],
    'sisr_wgrad_toimage_f32_eligible': [C.POINTER(WgradDesc)],
    'sisr_wgrad_plan_bf16': [C.POINTER(WgradDesc), _i32],
    'sisr_wgrad_deep_plan': [C.POINTER(WgradDesc), _i32],
    'sisr_wgrad_deep_eligible': [C.POINTER(WgradDesc)],
    'sisr_wgrad_deep_batch': [C.POINTER(WgradDesc), _f, _i32, _f],
    'sisr_wgrad_trunk_batch_arg_bytes': [],
    'sisr_wgrad_trunk_batch_args': [C.POINTER(WgradDesc), _i32, _f],
    'sisr_wgrad_trunk_batch': [C.POINTER(WgradDesc), _f, _i32, _i32, _f],
    'sisr_wgrad_trunk_f32_batch_arg_bytes': [],
    'sisr_wgrad_trunk_f32_batch_args': [C.POINTER(WgradDesc), _i32, _f],
    'sisr_wgrad_trunk_f32_batch': [C.POINTER(WgradDesc), _f, _i32, _i32, _f],
    'sisr_conv2d_wgrad_bf16': [C.POINTER(WgradDesc), _f],
    'sisr_tr16_selftest': [_f, _f],
    'sisr_slab_reduce_f32': [_f, _f, _i32, _i64, _i64, _f],
    'sisr_slab_reduce_multi': [_f, _f, _f, _f, _f, _i32, _f],
    'sisr_wgrad_bf16_slab_lead': [C.POINTER(WgradDesc)],
    'sisr_conv2d_bf16_route': [C.POINTER(ConvDesc)],
    'sisr_conv2d_f32_route': [C.POINTER(ConvDesc)],
    'sisr_wgrad_bf16_route': [C.POINTER(WgradDesc)],
    'sisr_wgrad_f32_route': [C.POINTER(WgradDesc)],
    'sisr_weights_prepare': [_f, _i32, _i32, _i32, _f],
    'sisr_weights_sn': [_f, _i32, _i32, _i32, _f],
    'sisr_weights_pack': [_f, _i32, _i32, _i32, _f],
    'sisr_weights_pack_deep': [_f, _i32, _i32, _i32, _f],
    'sisr_weight_image_bytes': [C.POINTER(WeightImage)],
    'sisr_weights_grad': [_f, _i32, _f, _i32, _f],
    'sisr_weights_grad_fast': [_f, _i32, _f, _i32, _i32, _f],
    'sisr_weights_grad_tiles': [C.POINTER(WeightGradDesc)],
    'sisr_bn_finalize': [_f, _f, _i32, _i32, _f, _f, _f, _f, _f32, _f32, _f, _f, _f, _f, _f],
    'sisr_bn_eval_consts': [_f, _f, _f, _f, _f32, _i32, _f, _f, _f],
    'sisr_bn_bwd_plan': [C.POINTER(BnBwdDesc)],
    'sisr_bn_bwd': [C.POINTER(BnBwdDesc), _f],
    'sisr_bn_bwd_finalize': [C.POINTER(BnBwdDesc), _f],
    'sisr_bn_bwd_finalize_slab': [C.POINTER(BnBwdDesc), _f, _f, _i32, _i64, _i64, _f],
    'sisr_eltwise_res_affine': [_f, _f, _f32, _f, _f, _f, _f, _i64, _i32, _i32, _f],
    'sisr_prelu_slope_grad': [_f, _f, _i64, _f, _f, _i32, _f],
    'sisr_toimage_bwd_f32_eligible': [C.POINTER(ToImageBwdDesc)],
    'sisr_toimage_bwd_f32_parts': [C.POINTER(ToImageBwdDesc)],
    'sisr_toimage_bwd_f32': [C.POINTER(ToImageBwdDesc), _f],
    'sisr_toimage_bwd_desc_bytes': [],
    'sisr_add': [_f, _f, _f, _i64, _i32, _f],
    'sisr_adam_blocks': [_i64],
    'sisr_adam_step': [_f, _i32, _i64] + [C.c_double] * 7 + [_f],
    'sisr_adam_norm_ws_doubles': [_i64],
    'sisr_adam_grad_sumsq': [_f, _i32, _i64, _f, _f],
    'sisr_adam_prepare': [_f, _i32, _f, _i32, C.c_double, C.c_double, _f, _i64, C.c_double, _i32, _i32, _f, _f, _f],
    'sisr_adam_step_dev': [_f, _i32, _i64, _f, _f] + [C.c_double] * 4 + [_f],
    'sisr_ema_prepare': [_f, C.c_double, C.c_double, _f, _f, _f],
    'sisr_ema_update': [_f, _i32, _i64, _f, _f],
    'sisr_ema_swap': [_f, _i32, _i64, _f],
    'sisr_nhwc_to_nchw': [_f, _f, _f, _f, _f32, _f, _i64, _i32, _i32, _i32, _i32, _i32, _f],
    'sisr_nchw_to_nhwc': [_f, _i64, _f, _i32, _i32, _i32, _i32, _i32, _f],
    'sisr_nchw_grad_to_nhwc4': [_f, _f, _f, _i32, _i32, _i32, _i32, _i32, _f],
    'sisr_maxpool2_fwd': [_f, _f, _i32, _i32, _i32, _i32, _i32, _f],
    'sisr_maxpool2_relu_bwd': [_f, _f, _f, _i32, _i32, _i32, _i32, _i32, _f],
    'sisr_add_relu_masked': [_f, _f, _f, _f, _i64, _i32, _f],
    'sisr_fc_forward': [_f, _f32, _f, _f, _f, _i32, _i32, _i32, _i32, _f],
    'sisr_fc_dgrad_splits': [_i32, _i32],
    'sisr_fc_dgrad': [_f, _f, _f, _f, _i32, _i32, _i32, _f],
    'sisr_fc_wgrad': [_f, _f, _f32, _f, _f, _i32, _i32, _i32, _f],
    'sisr_act_bwd': [_f, _f, _f, _i64, _i32, _f32, _f],
    'sisr_fc_head_ws_floats': [_i32],
    'sisr_fc_head_forward': [_f, _f, _f, _f, _f, _f32, _f, _f, _f, _i32, _i32, _i32, _f],
    'sisr_fc_head_backward': [_f, _f, _f, _f, _f32, _f, _f, _f, _f, _i32, _i32, _f],
    'sisr_fc1_dgrad': [_f, _f, _f, _i32, _i32, _i32, _f],
    'sisr_fc_wgrad_rows': [_f, _f, _f32, _f, _i32, _i32, _i32, _f],
    'sisr_resize_coeffs': [_i32, _i32, _f, _f],
    'sisr_resize_u8_normalize': [_f, _f, _i32, _i32, _i32, _i32, _i32, _i32, _f, _f, _i32, _f, _f, _i32, _f32, _f32, _f],
    'sisr_patch_draw': [_f, C.c_uint64] + [_i32] * 10 + [_f, _f],
    'sisr_patch_draws_host': [_i64, C.c_uint64] + [_i32] * 10 + [_f],
    'sisr_patch_gather': [_f, _i32, _i32, _i32, _i32, _f, _i32, _i32, _i32, _f32, _f32, _f, _i32, _f],
    'sisr_patch_draw_table': [_f, C.c_uint64] + [_i32] * 7 + [_f] + [_i32] * 3 + [_f, _f],
    'sisr_patch_draws_table_host': [_i64, C.c_uint64] + [_i32] * 7 + [_f] + [_i32] * 3 + [_f],
    'sisr_patch_gather_table': [_f, _i64, _f, _i32, _i32, _f, _i32, _i32, _i32, _f32, _f32, _f, _i32, _f],
    'sisr_degrade_draw': [_f, C.c_uint64, _i32, _i32, _i32, _f32, _f32, _i32, _f32, _f32, _f, _f, _f, _f],
    'sisr_degrade_params_host': [_i64, C.c_uint64, _i32, _i32, _i32, _f32, _f32, _i32, _f32, _f32, _f, _f, _f],
    'sisr_degrade_noise_host': [_i64, C.c_uint64, _i32, _i64, _i64, _f],
    'sisr_degrade_fwd': [_f, _f, _f, _f, C.c_uint64, _i32, _f] + [_i32] * 8 + [_f],
    'sisr_degrade_bwd': [_f, _f, _f, _f] + [_i32] * 7 + [_f],
    'sisr_degrade_mix_bytes': [],
    'sisr_degrade_draw_mix': [_f, C.c_uint64, _i32, _i32, C.POINTER(DegradeMix), _f, _f, _f, _f, _f, _f],
    'sisr_degrade_mix_host': [_i64, C.c_uint64, _i32, _i32, C.POINTER(DegradeMix), _f, _f, _f, _f],
    'sisr_degrade_noise_fwd': [_f, _f, _f, C.c_uint64, _i32, _f] + [_i32] * 5 + [_f],
    'sisr_degrade_noise_bwd': [_f, _f, _f] + [_i32] * 4 + [_f],
    'sisr_degrade_noise_grey_host': [_i64, C.c_uint64, _i32, _i64, _i64, _f],
    'sisr_jpeg_tables': [_f, C.c_uint64, _i32, _i32, _i32, _i32, _f, _f, _f],
    'sisr_jpeg_tables_host': [_i64, C.c_uint64, _i32, _i32, _i32, _i32, _f, _f],
    'sisr_jpeg_fwd': [_f, _f, _f] + [_i32] * 6 + [_f],
    'sisr_jpeg_bwd': [_f, _f, _f, _f, _f] + [_i32] * 6 + [_f],
    'sisr_tile_axis': [_i32, _i32, _i32, _f, _f, _i32],
    'sisr_tile_gather_f32': [_f, _i32, _i32, _i32, _f, _i32, _i32, _i32, _f, _f],
    'sisr_tile_stitch': [_f, _f, _f, _f, _i32, _f, _f, _i32] + [_i32] * 7 + [_f32, _i32, _f32, _f32, _f, _i32, _f],
    'sisr_bicubic_fwd': [_f, _f, _i32, _i32, _i32, _i32, _i32, _i32, _f],
    'sisr_bicubic_bwd': [_f, _f, _f, _i32, _i32, _i32, _i32, _i32, _f],
    'sisr_image_metrics_ws_floats': [_i32, _i32, _i32, _i32, _i32, _i32],
    'sisr_image_metrics': [_f, _f, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _f, _f, _f, _f],
    'sisr_mse_ws_floats': [_i64],
    'sisr_mse_fwd': [_f, _f, _i64, _f32, _f, _f, _f],
    'sisr_mse_bwd': [_f, _f, _f, _i64, _f32, _f, _f, _f],
    'sisr_bce_fwd': [_f, _f, _f32, _i64, _f32, _f, _f, _f],
    'sisr_bce_bwd': [_f, _f, _f32, _i64, _f32, _f, _f, _f],
    'sisr_image_loss_ws_floats': [_i32] * 7,
    'sisr_image_loss_fwd': [_f, _f] + [_i32] * 6 + [_f32, _f32, _f32, _i32, _f32, _f, _f, _f, _f, _f],
    'sisr_image_loss_bwd': [_f, _f, _f] + [_i32] * 6 + [_f32, _f32, _f32, _i32, _f32, _f, _f, _f],
    'sisr_ms_ssim_ws_floats': [_i32] * 8,
    'sisr_ms_ssim_fwd': [_f, _f] + [_i32] * 6 + [_f32, _i32, C.POINTER(_f32), _f, _f, _f, _f, _f, _f],
    'sisr_ms_ssim_bwd': [_f] * 6 + [_i32] * 6 + [_f32, _i32, C.POINTER(_f32), _f, _f, _f, _f],
    'sisr_freq_loss_ws_floats': [_i32] * 7,
    'sisr_freq_loss_fwd': [_f, _f] + [_i32] * 7 + [_f32, _f32, _f, _f, _f, _f, _f],
    'sisr_freq_loss_bwd': [_f, _f, _f] + [_i32] * 7 + [_f32, _f32, _f, _f, _f, _f],
    'sisr_artifact_ws_floats': [_i32, _i32, _i32],
    'sisr_artifact_fwd': [_f, _f, _f] + [_i32] * 5 + [_f32, _f, _f, _f, _f],
    'sisr_artifact_bwd': [_f, _f, _f, _f] + [_i32] * 4 + [_f32, _f, _f, _f],
    'sisr_percep_ws_bytes': [_i32, _i32, C.POINTER(_i32), _i32, _i32],
    'sisr_percep_gram': [_f, _i32, _i64, _i32, C.POINTER(_i32), _f, _f, _f],
    'sisr_percep_fwd': [_f, _f, _i32, _i64, _i32, C.POINTER(_i32), C.POINTER(_f32), _f32, _f32, _i32, _f, _f, _f, _f, _f, _f, _f],
    'sisr_percep_bwd': [_f] * 7 + [_i32, _i64, _i32, C.POINTER(_i32), C.POINTER(_f32), _f32, _f32, _i32, _f, _f, _f],
    'sisr_cx_ws_bytes': [_i32, _i32, C.POINTER(_i32), _i32],
    'sisr_cx_sim': [_f, _f, _i32, _i64, _i32, C.POINTER(_i32), _f, _f, _f],
    'sisr_cx_fwd': [_f, _f, _i32, _i64, _i32, C.POINTER(_i32), C.POINTER(_f32), _f32, _f32, _f, _f, _f, _f, _f, _f],
    'sisr_cx_bwd': [_f] * 5 + [_i32, _i64, _i32, C.POINTER(_i32), C.POINTER(_f32), _f32, _f32, _f, _f, _f],
    'sisr_niqe_ws_bytes': [_i32] * 5,
    'sisr_niqe_features': [_f] + [_i32] * 5 + [_f32, _f32, _i32, _f, _f, _f, _f, _f],
    'sisr_niqe_score': [_f, _i32, _i32, _f, _f, _f, _f, _f],
    'sisr_gauss_taps_host': [_i32, _f32, _f],
    'sisr_gauss_blur_fwd': [_f, _f, _f, _i64, _i32, _i32, _i32, _f],
    'sisr_gauss_blur_bwd': [_f, _f, _f, _i64, _i32, _i32, _i32, _f],
    'sisr_usm_ws_bytes': [_i64, _i32, _i32],
    'sisr_usm_fwd': [_f, _f, _i32, _f32, _f32, _f32, _f32, _f, _f, _f, _i64, _i32, _i32, _f],
    'sisr_resize_taps_host': [_i32, _i32, _i32, _f, _f, _f],
    'sisr_resize_fwd': [_f, _f, _f] + [_i32] * 6 + [_f],
    'sisr_resize_bwd': [_f, _f, _f] + [_i32] * 6 + [_f],
    'sisr_resize_modes_draw': [_f, C.c_uint64, _i32, _i32, _f32, _f32, _f32, _f, _f],
    'sisr_resize_modes_host': [_i64, C.c_uint64, _i32, _i32, _f32, _f32, _f32, _f],
    'sisr_struct_sizes': [C.POINTER(_i32), _i32],
    'sisr_device_info': [C.POINTER(_i32), C.POINTER(_i32), C.c_char_p, _i32],
    'sisr_mfma_selftest': [_f, _f],
    'sisr_clear_last_error': [],
}
EXPORTS = sorted(list(_SIGS) + ['sisr_version'])

_lib = None


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 with hipcc (cross-compiles without a GPU)."""
    r = subprocess.run(['make', '-C', CSRC, '-j8'], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode != 0 or not os.path.exists(LIB_PATH):
        raise RuntimeError('building libsisr_hip.so failed (hipcc --offload-arch=gfx950)')
    return LIB_PATH


def lib():
    """The loaded library.  Raises RuntimeError if it is absent or mismatched -- no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            'libsisr_hip.so not found at %s: the MI355X HIP library IS the implementation of this '
            'path (no CPU/eager fallback). Build it with `python __graft_entry__.py build` or '
            '`make -C %s`.' % (LIB_PATH, CSRC))
    L = C.CDLL(LIB_PATH)
    for name, args in _SIGS.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    L.sisr_adam_blocks.restype = C.c_int64
    L.sisr_adam_norm_ws_doubles.restype = C.c_int64
    L.sisr_wgrad_bf16_slab_lead.restype = C.c_int64
    L.sisr_weight_image_bytes.restype = C.c_int64
    L.sisr_usm_ws_bytes.restype = C.c_int64
    L.sisr_percep_ws_bytes.restype = C.c_int64
    L.sisr_cx_ws_bytes.restype = C.c_int64
    L.sisr_niqe_ws_bytes.restype = C.c_int64
    L.sisr_version.restype = C.c_char_p
    L.sisr_version.argtypes = []
    sizes = (_i32 * 9)()
    n = L.sisr_struct_sizes(sizes, 9)
    mine = [C.sizeof(t) for t in (ConvDesc, WgradDesc, WeightDesc, WeightGradDesc, BnBwdDesc, ConvPlan, DeepPlan, WgradDeepPlan,
                                  ImageRec)]
    if n != 9 or list(sizes[:9]) != mine:
        raise RuntimeError('libsisr_hip.so does not match the Python mirror of sisr_hip.h: %s vs %s'
                           % (list(sizes[:9]), mine))
    if L.sisr_toimage_bwd_desc_bytes() != C.sizeof(ToImageBwdDesc):
        raise RuntimeError('libsisr_hip.so does not match the Python mirror of SisrToImageBwdDesc')
    if L.sisr_degrade_mix_bytes() != C.sizeof(DegradeMix):
        raise RuntimeError('libsisr_hip.so does not match the Python mirror of SisrDegradeMix')
    _lib = L
    return L


def check(status, what):
    if status != 0:
        raise RuntimeError('%s failed with status %d' % (what, status))


def check_count(value, what):
    """entry points that answer a sizing question return a count >= 0 or a negative status"""
    if value < 0:
        raise RuntimeError('%s failed with status %d' % (what, value))
    return value
