"""ctypes binding of liblsi_hip.so (C ABI: include/lsi_hip.h).

There is NO fallback: if the shared library is missing, or an op is handed a
tensor that does not live on a ROCm device, this module raises.  PyTorch is used
only for device memory, streams and autograd bookkeeping.
"""
import ctypes
import os

import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# LSI_HIP_LIB=hooks selects the instrumented build (build.py --hooks) whose
# stream kernel honours the timing-experiment bits of LsiSplatDesc.reserved
# (any other value picks liblsi_hip_<value>.so: experiment builds)
SO_PATH = os.path.join(_PKG, 'liblsi_hip_%s.so' % os.environ['LSI_HIP_LIB'] if
                       os.environ.get('LSI_HIP_LIB') else 'liblsi_hip.so')

LSI_OK = 0
LSI_COMPOSE, LSI_WANT_DISP, LSI_HAS_MASK, LSI_WS_KEEP = 1, 2, 4, 8
LSI_DETERMINISTIC = 16
LSI_PACKED_RGBD = 32
LSI_GRAD_M = 64
LSI_PATH_AUTO, LSI_PATH_ATOMIC, LSI_PATH_ROWBAND, LSI_PATH_STREAM = 0, 1, 2, 3
LSI_PATH_TILE = 4
LSI_SCENE_IMG, LSI_SCENE_DISP, LSI_SCENE_IMG_ROOM, LSI_SCENE_DISP_ROOM = 1, 2, 4, 8
LSI_SCENE_MAX_PLANES = 16
LSI_FC_BN, LSI_FC_X_F32, LSI_FC_OUT_F32 = 1, 2, 4
LSI_IMAGE_MAX_PIXELS = 16843009
LSI_AUG_FLIP = 1
LSI_VIS_SKIP, LSI_VIS_RGB, LSI_VIS_GRAY, LSI_VIS_LUT, LSI_VIS_ABSDIFF = 0, 1, 2, 3, 4
LSI_VIS_MAX_ITEMS = 256
LSI_LIDAR_INVERSE = 1
LSI_DEPTH_SUP_SILOG, LSI_DEPTH_SUP_L1 = 0, 1
LSI_GEO_CONS_RATIO, LSI_GEO_CONS_L1 = 0, 1
LSI_LIDAR_TILE_H, LSI_LIDAR_TILE_W = 16, 64
LSI_FILL_CONF, LSI_FILL_SPLAT = 0, 1
LSI_FILL_TILE, LSI_FILL_MID_MAX_PIXELS = 32, 2560
PATH_NAMES = {1: 'atomic', 2: 'rowband', 3: 'stream', 4: 'tile'}

_c_f = ctypes.POINTER(ctypes.c_float)
_c_i = ctypes.POINTER(ctypes.c_int32)


class LsiStreamAdapt(ctypes.Structure):
  _fields_ = [('state', ctypes.c_int32), ('pending', ctypes.c_int32),
              ('seq', ctypes.c_uint32), ('calls', ctypes.c_uint32),
              ('ctr_dev', ctypes.c_void_p), ('ctr_host', ctypes.c_void_p)]


class LsiSplatDesc(ctypes.Structure):
  _fields_ = (
      [(n, ctypes.c_int32) for n in ('L', 'B', 'H', 'W', 'Ht', 'Wt')] +
      [(n, ctypes.c_int64) for n in (
          'tex_sl', 'tex_sb', 'tex_sy', 'tex_sx', 'tex_sc',
          'disp_sl', 'disp_sb', 'disp_sy', 'disp_sx',
          'mask_sl', 'mask_sb', 'mask_sy', 'mask_sx')] +
      [(n, ctypes.c_float) for n in (
          'trg_downsampling', 'max_disp', 'zbuf_scale', 'bg_wt')] +
      [('flags', ctypes.c_uint32), ('path', ctypes.c_int32),
       ('tune_rows', ctypes.c_int32), ('tune_threads', ctypes.c_int32),
       ('tune_window', ctypes.c_int32), ('reserved', ctypes.c_int32),
       ('adapt', ctypes.c_void_p)])


class LsiLossDesc(ctypes.Structure):
  _fields_ = (
      [(n, ctypes.c_int32) for n in ('L', 'B', 'H', 'W')] +
      [(n, ctypes.c_int64) for n in (
          'img_sl', 'img_sb', 'img_sy', 'img_sx', 'img_sc',
          'mask_sl', 'mask_sb', 'mask_sy', 'mask_sx',
          'disp_sl', 'disp_sb', 'disp_sy', 'disp_sx',
          'trg_sb', 'trg_sy', 'trg_sx', 'trg_sc')] +
      [(n, ctypes.c_float) for n in ('bg_layer_disp', 'max_disp', 'zbuf_scale')] +
      [('reserved', ctypes.c_int32)])


class LsiSsimDesc(ctypes.Structure):
  _fields_ = (
      [(n, ctypes.c_int32) for n in ('nl', 'B', 'Ht', 'Wt', 'H', 'W', 'x_min',
                                     'y_min', 'win')] +
      [(n, ctypes.c_float) for n in ('sigma', 'c1', 'c2')] +
      [(n, ctypes.c_int64) for n in ('t_sb', 't_sy', 't_sx', 't_sc')])


class LsiEdgeSmoothDesc(ctypes.Structure):
  _fields_ = (
      [(n, ctypes.c_int32) for n in ('L', 'B', 'H', 'W', 'order', 'normalise')] +
      [(n, ctypes.c_int64) for n in ('d_sl', 'd_sb', 'd_sy', 'd_sx',
                                     'g_sl', 'g_sb', 'g_sy', 'g_sx', 'g_sc')] +
      [(n, ctypes.c_float) for n in ('alpha', 'eps')])


class LsiDepthSupDesc(ctypes.Structure):
  _fields_ = (
      [(n, ctypes.c_int32) for n in ('P', 'H', 'W', 'mode')] +
      [(n, ctypes.c_int64) for n in ('p_sp', 'p_sy', 'p_sx', 'g_sp', 'g_sy', 'g_sx')] +
      [(n, ctypes.c_float) for n in ('valid_above', 'g_min', 'g_max', 'eps', 'lam')] +
      [('reserved', ctypes.c_int32)])


class LsiGeoConsDesc(ctypes.Structure):
  _fields_ = (
      [(n, ctypes.c_int32) for n in ('P', 'H', 'W', 'mode')] +
      [(n, ctypes.c_int64) for n in ('d_sp', 'd_sy', 'd_sx', 'e_sp', 'e_sy', 'e_sx')] +
      [('shift', ctypes.c_int32), ('occl_thresh', ctypes.c_float)])


class LsiConvDesc(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int32) for n in (
      'N', 'H', 'W', 'Cin', 'OH', 'OW', 'Cout', 'KH', 'KW', 'stride', 'pad_t', 'pad_l')]


class LsiSceneDesc(ctypes.Structure):
  _fields_ = ([(n, ctypes.c_int32) for n in ('B', 'V', 'P', 'Hs', 'Ws', 'H', 'W',
                                             'n_box', 'soft')] +
              [('min_disp', ctypes.c_float), ('temp', ctypes.c_float),
               ('outputs', ctypes.c_uint32)])


class LsiFcDesc(ctypes.Structure):
  _fields_ = ([(n, ctypes.c_int32) for n in ('M', 'K', 'N', 'groups', 'taps')] +
              [('flags', ctypes.c_uint32), ('w_sn', ctypes.c_int64),
               ('w_sk', ctypes.c_int64), ('tap_off', ctypes.c_int64 * 4),
               ('eps', ctypes.c_float), ('reserved', ctypes.c_int32)])


class LsiPackJob(ctypes.Structure):
  _fields_ = ([('w', ctypes.c_void_p), ('dst', ctypes.c_void_p)] +
              [(n, ctypes.c_int32) for n in ('D0', 'D1', 'khw', 'tr', 'ntaps', 'block0')] +
              [('tap', ctypes.c_int8 * 56)])


class LsiConvIO(ctypes.Structure):
  _fields_ = ([(n, ctypes.c_void_p) for n in ('x', 'x2', 'packed', 'out', 'out2',
                                              'bn_workspace', 'workspace')] +
              [('workspace_bytes', ctypes.c_size_t), ('c1', ctypes.c_int32),
               ('groups', ctypes.c_int32)])


class LsiImageDesc(ctypes.Structure):
  _fields_ = ([('offset', ctypes.c_int64)] +
              [(n, ctypes.c_int32) for n in ('H', 'W', 'C', 'reserved')])


class LsiAugmentDesc(ctypes.Structure):
  _fields_ = ([('offset', ctypes.c_int64)] +
              [(n, ctypes.c_int32) for n in ('H', 'W', 'C')] +
              [('flags', ctypes.c_uint32)] +
              [(n, ctypes.c_int32) for n in ('y0', 'x0', 'ch', 'cw', 'table',
                                             'reserved')] +
              [('gain', ctypes.c_float * 3), ('reserved2', ctypes.c_int32)])


class LsiVisSheet(ctypes.Structure):
  _fields_ = ([(n, ctypes.c_int32) for n in ('rows', 'cols', 'cell_h', 'cell_w',
                                             'gutter', 'n_items')] +
              [('bg', ctypes.c_uint8 * 3), ('nan', ctypes.c_uint8 * 3),
               ('reserved', ctypes.c_uint8 * 2)])


class LsiScanDesc(ctypes.Structure):
  _fields_ = [('first', ctypes.c_int64), ('n', ctypes.c_int32),
              ('reserved', ctypes.c_int32)]


class LsiVisItem(ctypes.Structure):
  _fields_ = ([('src', ctypes.c_void_p), ('ref', ctypes.c_void_p)] +
              [(n, ctypes.c_int64) for n in ('s_y', 's_x', 's_c', 'r_y', 'r_x', 'r_c')] +
              [(n, ctypes.c_int32) for n in ('kind', 'H', 'W', 'C', 'zoom', 'reserved')] +
              [('lo', ctypes.c_float), ('inv', ctypes.c_float)])


# name -> (restype, argtypes); every symbol include/lsi_hip.h declares.
_I32, _I64, _VP, _SZ = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
_DP = ctypes.POINTER(LsiSplatDesc)
_LP = ctypes.POINTER(LsiLossDesc)
_CP = ctypes.POINTER(LsiConvDesc)
_F32 = ctypes.c_float
SIGNATURES = {
    'lsi_version': (ctypes.c_int, []),
    'lsi_strerror': (ctypes.c_char_p, [ctypes.c_int]),
    'lsi_bg_weight': (ctypes.c_float, [ctypes.c_double] * 3),
    'lsi_rowband_ok': (ctypes.c_int, [_DP, _VP]),
    'lsi_stream_ok': (ctypes.c_int, [_DP, _VP]),
    'lsi_splat_workspace_bytes': (_SZ, [_DP]),
    'lsi_stream_adapt_state': (ctypes.c_int, [ctypes.POINTER(LsiStreamAdapt)]),
    'lsi_splat_fwd': (ctypes.c_int, [_DP] + [_VP] * 8 + [_SZ, _VP]),
    'lsi_splat_bwd_workspace_bytes': (_SZ, [_DP]),
    'lsi_splat_bwd': (ctypes.c_int, [_DP] + [_VP] * 12 + [_SZ, _VP]),
    'lsi_splat_bwd_m': (ctypes.c_int, [_DP] + [_VP] * 13 + [_SZ, _VP]),
    'lsi_splat_bwd_disp_workspace_bytes': (_SZ, [_DP]),
    'lsi_splat_bwd_disp': (ctypes.c_int, [_DP] + [_VP] * 15 + [_SZ, _VP]),
    'lsi_splat_fwd_both': (ctypes.c_int, [_DP] + [_VP] * 9 + [_SZ, _VP]),
    'lsi_splat_bwd_both': (ctypes.c_int, [_DP] + [_VP] * 16 + [_SZ, _VP]),
    'lsi_splat_bwd_both_m': (ctypes.c_int, [_DP] + [_VP] * 17 + [_SZ, _VP]),
    'lsi_project_indices': (ctypes.c_int, [_DP] + [_VP] * 6),
    'lsi_splat_generic': (ctypes.c_int, [_I32] * 6 + [_VP] * 4),
    'lsi_splat_generic_bwd': (ctypes.c_int, [_I32] * 6 + [_VP] * 6),
    'lsi_scatter_add': (ctypes.c_int, [_I32, _I64, _I64] + [_VP] * 4),
    'lsi_bilinear_fwd': (ctypes.c_int, [_I32] * 6 + [_VP] * 4),
    'lsi_conv3x3_pred_bwd_workspace_bytes': (_SZ, [_I32] * 3),
    'lsi_conv3x3_wgrad_workspace_bytes': (_SZ, [_I32] * 5),
    'lsi_conv3x3_wgrad': (ctypes.c_int, [_I32] * 5 + [_VP] * 4 + [_SZ, _VP]),
    'lsi_conv3x3_pred_bwd': (ctypes.c_int, [_I32] * 4 + [_VP] * 7 + [_SZ, _VP]),
    'lsi_conv3x3_c32_fwd': (ctypes.c_int, [_I32] * 5 + [_VP] * 3 + [_F32, _VP, _VP]),
    'lsi_projection_matrices': (ctypes.c_int, [_I32] + [_VP] * 4 + [_I32, _VP]),
    'lsi_bilinear_taps': (ctypes.c_int, [_I32] * 6 + [_VP] * 5),
    'lsi_bilinear_bwd': (ctypes.c_int, [_I32] * 6 + [_VP] * 6),
    'lsi_bilinear_taps_bwd': (ctypes.c_int, [_I32] * 6 + [_VP] * 5 + [_VP]),
    'lsi_loss_workspace_bytes': (_SZ, []),
    'lsi_zbuf_comp_loss_fwd': (ctypes.c_int, [_LP] + [_VP] * 6 + [_SZ, _VP]),
    'lsi_zbuf_comp_loss_bwd': (ctypes.c_int, [_LP] + [_VP] * 9),
    'lsi_disp_reg_loss_fwd': (ctypes.c_int, [_I32] * 4 + [_I64] * 4 + [_VP] * 3 +
                              [_SZ, _VP]),
    'lsi_disp_reg_loss_bwd': (ctypes.c_int, [_I32] * 4 + [_I64] * 4 + [_VP] * 4),
    'lsi_view_synth_loss_fwd': (ctypes.c_int, [_I32] * 8 + [_VP] * 2 + [_I64] * 4 +
                                [_VP] * 2 + [_SZ, _VP]),
    'lsi_view_synth_loss_bwd': (ctypes.c_int, [_I32] * 8 + [_VP] * 2 + [_I64] * 4 +
                                [_VP] * 3),
    'lsi_ssim_window': (ctypes.c_int, [_I32, _F32, _VP]),
    'lsi_ssim_loss_fwd': (ctypes.c_int, [ctypes.POINTER(LsiSsimDesc)] + [_VP] * 4 +
                          [_SZ, _VP]),
    'lsi_ssim_loss_bwd': (ctypes.c_int, [ctypes.POINTER(LsiSsimDesc)] + [_VP] * 5),
    'lsi_eval_ssim': (ctypes.c_int, [ctypes.POINTER(LsiSsimDesc)] + [_VP] * 4 +
                      [_SZ, _VP]),
    'lsi_edge_smooth_workspace_bytes': (_SZ, [ctypes.POINTER(LsiEdgeSmoothDesc)]),
    'lsi_edge_smooth_loss_fwd': (ctypes.c_int, [ctypes.POINTER(LsiEdgeSmoothDesc)] +
                                 [_VP] * 5 + [_SZ, _VP]),
    'lsi_edge_smooth_loss_bwd': (ctypes.c_int, [ctypes.POINTER(LsiEdgeSmoothDesc)] +
                                 [_VP] * 6),
    'lsi_depth_sup_workspace_bytes': (_SZ, [ctypes.POINTER(LsiDepthSupDesc)]),
    'lsi_depth_sup_loss_fwd': (ctypes.c_int, [ctypes.POINTER(LsiDepthSupDesc)] +
                               [_VP] * 6 + [_SZ, _VP]),
    'lsi_depth_sup_loss_bwd': (ctypes.c_int, [ctypes.POINTER(LsiDepthSupDesc)] +
                               [_VP] * 7),
    'lsi_geo_cons_workspace_bytes': (_SZ, [ctypes.POINTER(LsiGeoConsDesc)]),
    'lsi_geo_cons_loss_fwd': (ctypes.c_int, [ctypes.POINTER(LsiGeoConsDesc)] +
                              [_VP] * 7 + [_SZ, _VP]),
    'lsi_geo_cons_loss_bwd': (ctypes.c_int, [ctypes.POINTER(LsiGeoConsDesc)] +
                              [_VP] * 8),
    'lsi_compose_fwd': (ctypes.c_int, [_I32, _I64, _I32] + [_VP] * 3 +
                        [_I32, _F32, _F32, _VP, _VP]),
    'lsi_compose_depth_fwd': (ctypes.c_int, [_I32, _I64] + [_VP] * 2 +
                              [_I32, _F32, _F32, _F32, _VP, _VP]),
    'lsi_compose_bwd': (ctypes.c_int, [_I32, _I64, _I32] + [_VP] * 3 +
                        [_I32, _F32, _F32] + [_VP] * 5),
    'lsi_compose_depth_bwd': (ctypes.c_int, [_I32, _I64] + [_VP] * 2 +
                              [_I32, _F32, _F32, _F32] + [_VP] * 3),
    'lsi_eval_workspace_bytes': (_SZ, []),
    'lsi_eval_view_metrics': (ctypes.c_int, [_I32] * 8 + [_VP] * 3 + [_I64] * 4 +
                              [_VP] * 3 + [ctypes.c_uint32, _F32] + [_VP] * 2 +
                              [_SZ, _VP]),
    'lsi_eval_layer_metrics': (ctypes.c_int, ([_LP] + [_VP] * 6) * 2 + [_VP] * 2 +
                               [_SZ, _VP]),
    'lsi_eval_depth_workspace_bytes': (_SZ, [_I32] * 4),
    'lsi_eval_depth_metrics': (ctypes.c_int, [_I32] * 3 + [_VP] * 4 + [_I32] * 4 +
                               [_F32] * 3 + [ctypes.c_uint32] + [_VP] * 3 + [_SZ, _VP]),
    'lsi_disocclusion_mask': (ctypes.c_int, [_I32] * 5 + [_VP] * 3 + [_F32, _VP, _VP]),
    'lsi_render_planes': (ctypes.c_int, [ctypes.POINTER(LsiSceneDesc)] + [_VP] * 8),
    'lsi_render_planes_bwd_workspace_bytes': (_SZ, [ctypes.POINTER(LsiSceneDesc)]),
    'lsi_render_planes_bwd': (ctypes.c_int, [ctypes.POINTER(LsiSceneDesc)] +
                              [_VP] * 9 + [_SZ, _VP]),
    'lsi_conv2d_supported': (ctypes.c_int, [_CP]),
    'lsi_conv2d_packed_bytes': (_SZ, [_CP]),
    'lsi_conv2d_pack': (ctypes.c_int, [_CP, _I32, _VP, _VP, _SZ, _VP]),
    'lsi_conv2d_pack_job': (ctypes.c_int, [_CP, _I32, _VP, _VP, _SZ,
                                           ctypes.POINTER(LsiPackJob), _c_i]),
    'lsi_conv2d_pack_many': (ctypes.c_int, [_VP, _I32, _I32, _VP]),
    'lsi_conv2d_fwd': (ctypes.c_int, [_CP] + [_VP] * 4),
    'lsi_conv2d_bwd_data': (ctypes.c_int, [_CP] + [_VP] * 4),
    'lsi_conv2d_fwd_bnstats': (ctypes.c_int, [_CP] + [_VP] * 4 + [_I32, _VP]),
    'lsi_conv2d_bwd_data_bnstats': (ctypes.c_int, [_CP] + [_VP] * 4 + [_I32, _VP]),
    'lsi_conv2d_fwd_cat': (ctypes.c_int, [_CP, _VP, _VP, _I32, _VP, _VP, _VP, _I32, _VP]),
    'lsi_conv2d_bwd_data_cat': (ctypes.c_int, [_CP, _VP, _VP, _VP, _VP, _I32, _VP]),
    'lsi_conv2d_wgrad_cat': (ctypes.c_int, [_CP, _VP, _VP, _I32, _VP, _VP, _I32, _VP, _SZ, _VP]),
    'lsi_conv2d_workspace_bytes': (_SZ, [_CP, _I32]),
    'lsi_conv2d_run': (ctypes.c_int, [_CP, _I32, ctypes.POINTER(LsiConvIO), _VP]),
    'lsi_conv2d_wgrad_workspace_bytes': (_SZ, [_CP]),
    'lsi_conv2d_wgrad': (ctypes.c_int, [_CP] + [_VP] * 4 + [_SZ, _VP]),
    'lsi_conv2d_first_supported': (ctypes.c_int, [_CP]),
    'lsi_conv2d_first_fwd': (ctypes.c_int, [_CP, _VP, _I32, _VP, _I32, _VP, _VP, _I32, _VP]),
    'lsi_conv2d_first_wgrad_workspace_bytes': (_SZ, [_CP]),
    'lsi_conv2d_first_wgrad': (ctypes.c_int, [_CP, _VP, _I32, _VP, _VP, _I32, _VP, _SZ, _VP]),
    'lsi_conv2d_f32_supported': (ctypes.c_int, [_CP]),
    'lsi_conv2d_f32_packed_bytes': (_SZ, [_CP]),
    'lsi_conv2d_f32_pack': (ctypes.c_int, [_CP, _I32, _VP, _VP, _SZ, _VP]),
    'lsi_conv2d_f32_pack_job': (ctypes.c_int, [_CP, _I32, _VP, _VP, _SZ,
                                               ctypes.POINTER(LsiPackJob), _c_i]),
    'lsi_conv2d_f32_pack_many': (ctypes.c_int, [_VP, _I32, _I32, _VP]),
    'lsi_conv2d_f32_workspace_bytes': (_SZ, [_CP, _I32]),
    'lsi_conv2d_f32_run': (ctypes.c_int, [_CP, _I32, ctypes.POINTER(LsiConvIO), _VP]),
    'lsi_conv2d_wgrad_f32_workspace_bytes': (_SZ, [_CP]),
    'lsi_conv2d_wgrad_f32': (ctypes.c_int, [_CP, _VP, _VP, _I32, _VP, _VP, _I32, _VP, _SZ,
                                            _VP]),
    'lsi_bn_workspace_floats': (_SZ, [_I64, _I32, _I32, _I32]),
    'lsi_bn_launch_workgroups': (_I32, [_I64, _I32, _I32, _I32]),
    'lsi_bn_relu_fwd': (ctypes.c_int, [_VP] * 5 + [_I64, _I32, _I32, _I32, _F32, _I32, _VP]),
    'lsi_bn_relu_bwd': (ctypes.c_int, [_VP] * 7 + [_I64, _I32, _I32, _I32, _I32, _VP]),
    'lsi_bn_relu_norm': (ctypes.c_int, [_VP] * 5 + [_I64, _I32, _I32, _I32, _F32, _I32, _VP]),
    'lsi_bn_stats_discard': (ctypes.c_int, [_VP, _I32, _VP]),
    'lsi_fc_desc_bytes': (_SZ, []),
    'lsi_fc_supported': (ctypes.c_int, [ctypes.POINTER(LsiFcDesc)]),
    'lsi_fc_workspace_bytes': (_SZ, [ctypes.POINTER(LsiFcDesc)]),
    'lsi_fc_fwd': (ctypes.c_int, [ctypes.POINTER(LsiFcDesc)] + [_VP] * 7 + [_SZ, _VP]),
    'lsi_fc_bwd': (ctypes.c_int, [ctypes.POINTER(LsiFcDesc)] + [_VP] * 10 + [_SZ, _VP]),
    'lsi_area_resize_u8': (ctypes.c_int, [_I32, _VP, _VP, _VP, _SZ] + [_I32] * 3 +
                           [_VP, _VP]),
    'lsi_augment_resize_u8': (ctypes.c_int, [_I32, _VP, _VP, _VP, _SZ, _I64, _I32] +
                              [_I32] * 3 + [_VP, _VP]),
    'lsi_augment_sample_u16': (ctypes.c_int, [_I32, _VP, _VP, _VP, _SZ, _I32, _I32,
                                              _VP, _VP]),
    'lsi_visual_sheet_size': (ctypes.c_int, [ctypes.POINTER(LsiVisSheet),
                                             ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    'lsi_visual_pack_u8': (ctypes.c_int, [ctypes.POINTER(LsiVisSheet), _VP, _VP, _VP, _VP,
                                          _I64, _VP]),
    'lsi_sgm_workspace_bytes': (_SZ, [_I32] * 6),
    'lsi_sgm_disparity_u8': (ctypes.c_int, [_I32] * 4 + [_VP] * 2 + [_I32] * 6 +
                             [_VP] * 3 + [_SZ, _VP]),
    'lsi_disparity_filter_workspace_bytes': (_SZ, [_I32] * 5),
    'lsi_disparity_filter_u16': (ctypes.c_int, [_I32] * 3 + [_VP] * 2 + [_I32] * 3 +
                                 [_VP, _SZ, _VP]),
    'lsi_lidar_workspace_bytes': (_SZ, [_I32] * 6),
    'lsi_lidar_rasterize': (ctypes.c_int, [_I32] * 4 + [_VP] * 3 + [_I64, _VP, _F32, _F32,
                                                                  _I32, _I32, _F32,
                                                                  ctypes.c_uint32] +
                            [_VP, _VP, _SZ, _VP]),
    'lsi_fill_holes_workspace_bytes': (_SZ, [_I32] * 4),
    'lsi_fill_holes': (ctypes.c_int, [_I32] * 4 + [_VP, _VP, _I32, _F32, _F32, _F32,
                                                   _VP, _VP, _SZ, _VP]),
}

_lib = None


def lib():
  """The loaded shared library; raises if it has not been built."""
  global _lib
  if _lib is None:
    if not os.path.exists(SO_PATH):
      raise RuntimeError(
          'liblsi_hip.so is missing (%s). Build it with '
          '`python layered-scene-inference_amd/build.py`; there is no CPU or '
          'PyTorch fallback for the lsi HIP ops.' % SO_PATH)
    handle = ctypes.CDLL(SO_PATH)
    for name, (res, args) in SIGNATURES.items():
      fn = getattr(handle, name)  # AttributeError => ABI mismatch, loudly
      fn.restype = res
      fn.argtypes = args
    _lib = handle
  return _lib


def check(rc, what):
  if rc != LSI_OK:
    msg = lib().lsi_strerror(rc).decode()
    raise RuntimeError('%s failed: %s (code %d)' % (what, msg, rc))


def require_device(*tensors):
  """Every tensor must be fp32 on one ROCm device; returns that device."""
  dev = None
  for t in tensors:
    if t is None:
      continue
    if not t.is_cuda:
      raise RuntimeError(
          'lsi HIP ops need tensors on a ROCm GPU (got device %s); there is no '
          'CPU fallback' % t.device)
    if t.dtype != torch.float32 and t.dtype != torch.int32:
      raise RuntimeError('lsi HIP ops are fp32 (got %s)' % t.dtype)
    if dev is None:
      dev = t.device
    elif t.device != dev:
      raise RuntimeError('tensors on different devices: %s vs %s' %
                         (dev, t.device))
  return dev


def ptr(t):
  """Device address for a c_void_p parameter: a plain int (every entry point has
  its argtypes declared in SIGNATURES, so ctypes converts it itself -- a
  c_void_p object per argument costs half a microsecond of an eager step that
  makes hundreds of these calls)."""
  return None if t is None else t.data_ptr()


_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream_ptr(device):
  """The current HIP stream of `device` as an integer.  torch's raw accessor
  where it exists: `torch.cuda.current_stream(device).cuda_stream` builds a
  Stream object per call -- 5 us, 160 times per eager training step
  (profiles/r06/host_profile_L4.txt: 0.8 ms of a 10.6 ms launch side)."""
  if _RAW_STREAM is not None:
    idx = device.index
    if idx is None:
      idx = torch.cuda.current_device()
    return _RAW_STREAM(idx)
  return torch.cuda.current_stream(device).cuda_stream


def bg_weight(bg_layer_disp, max_disp, zbuf_scale):
  return float(lib().lsi_bg_weight(float(bg_layer_disp), float(max_disp),
                                   float(zbuf_scale)))
