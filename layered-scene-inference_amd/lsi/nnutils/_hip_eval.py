"""ctypes bindings of the fused evaluation kernels (include/lsi_hip.h,
csrc/lsi_eval.hip, csrc/lsi_depth_metrics.hip): the view-synthesis and per-layer
metrics accumulated into a device array of SLOT_COUNT doubles, the depth
accuracy metrics into DEPTH_SLOT_COUNT doubles of their own, and the
dis-occlusion mask.  For tensors on a ROCm device; there is no fallback: a
missing library raises in lsi._C.lib().
None of these calls synchronises with the host."""
import ctypes

import torch

from lsi import _C


def _slots(prefix, names):
  return {n: getattr(_C, prefix + n) for n in names.split()}


# the header's LSI_EVAL_* slots of the accumulator
SLOTS = _slots('LSI_EVAL_', 'COMPOSE_SUM COMPOSE_NORM COMPOSE_DISOCC_SUM '
               'COMPOSE_DISOCC_NORM DEPTH_SUM DEPTH_NORM DEPTH_DISOCC_SUM '
               'DEPTH_DISOCC_NORM PSNR_SUM PSNR_COUNT FG_TEX_SUM FG_DISP_SUM FG_NORM '
               'BG_TEX_SUM BG_DISP_SUM BG_NORM')
SLOT_COUNT = _C.LSI_EVAL_SLOTS
LSI_EVAL_DISOCC_U8, LSI_EVAL_VALID_GT = _C.LSI_EVAL_DISOCC_U8, _C.LSI_EVAL_VALID_GT

# metric name (the keys of eval_metrics.aggregate) -> (sum slot, normaliser slot)
METRICS = {
    'compose_splat_loss': ('COMPOSE_SUM', 'COMPOSE_NORM'),
    'compose_splat_loss_disocc': ('COMPOSE_DISOCC_SUM', 'COMPOSE_DISOCC_NORM'),
    'depth_splat_loss': ('DEPTH_SUM', 'DEPTH_NORM'),
    'depth_splat_loss_disocc': ('DEPTH_DISOCC_SUM', 'DEPTH_DISOCC_NORM'),
    'psnr': ('PSNR_SUM', 'PSNR_COUNT'),
    'fg_tex_error': ('FG_TEX_SUM', 'FG_NORM'),
    'fg_disp_error': ('FG_DISP_SUM', 'FG_NORM'),
    'bg_tex_error': ('BG_TEX_SUM', 'BG_NORM'),
    'bg_disp_error': ('BG_DISP_SUM', 'BG_NORM'),
}


def workspace(dev):
  n = int(_C.lib().lsi_eval_workspace_bytes())
  return torch.empty((n,), dtype=torch.uint8, device=dev), n


def _check_acc(acc, dev):
  if (acc.device != dev or acc.dtype != torch.float64 or
      acc.numel() != SLOT_COUNT or not acc.is_contiguous()):
    raise RuntimeError('the accumulator is %d contiguous float64 on %s' %
                       (SLOT_COUNT, dev))


def _require_fp32(fn, **tensors):
  """_C.require_device lets int32 through (the index tensors of other entry
  points); every array the metric kernels read is fp32, and an int32 one would
  be read as float bits."""
  for name, t in tensors.items():
    if t is not None and t.dtype != torch.float32:
      raise RuntimeError('%s: %s must be fp32 (got %s)' % (fn, name, t.dtype))


def _map(t, shape, what):
  """A contiguous B x H x W (x 1) map; no copy when it already is one."""
  if t is None:
    return None
  if tuple(t.shape) not in (shape, shape + (1,)):
    raise ValueError('%s must be %s (x 1), got %s' % (what, shape, tuple(t.shape)))
  return t.contiguous()


def view_metrics(acc, ws, ws_bytes, recons, recons_disp, target, x_min, y_min,
                 valid=None, disocc=None, gt_disp=None, valid_above=None):
  """lsi_eval_view_metrics: adds the metrics of one rendered view to `acc`.
  recons nl x B x Ht x Wt x 3, recons_disp nl x B x Ht x Wt x 1 or None, target
  B x H x W x 3 (any strides); valid / disocc / gt_disp B x H x W (x 1) or None,
  disocc fp32 or bool.  With valid_above, `valid` is a map and a pixel is valid
  where it exceeds that value."""
  dev = _C.require_device(recons, recons_disp, target, valid, gt_disp)
  _require_fp32('view_metrics', recons=recons, recons_disp=recons_disp, target=target,
                valid_mask=valid, gt_disp_trg=gt_disp)
  _check_acc(acc, dev)
  nl, b, ht, wt, c = recons.shape
  if c != 3 or tuple(target.shape[:1] + target.shape[3:]) != (b, 3):
    raise ValueError('view_metrics: 3-channel images of one batch size')
  _, h, w, _ = target.shape
  if h % ht or w % wt:
    raise ValueError('view_metrics: the target (%d x %d) is no integer multiple '
                     'of the rendering (%d x %d)' % (h, w, ht, wt))
  recons = recons.contiguous()
  if recons_disp is not None:
    if tuple(recons_disp.shape) != (nl, b, ht, wt, 1):
      raise ValueError('view_metrics: recons_disp must be %s' % ((nl, b, ht, wt, 1),))
    recons_disp = recons_disp.contiguous()
  flags = 0
  if disocc is not None:
    if not disocc.is_cuda or disocc.device != dev:
      raise RuntimeError('lsi HIP ops need tensors on a ROCm GPU (got device %s); '
                         'there is no CPU fallback' % disocc.device)
    if disocc.dtype in (torch.bool, torch.uint8):
      flags |= LSI_EVAL_DISOCC_U8
    elif disocc.dtype != torch.float32:
      raise RuntimeError('the dis-occlusion mask is fp32 or bool (got %s)' %
                         disocc.dtype)
  valid = _map(valid, (b, h, w), 'valid_mask')
  disocc = _map(disocc, (b, h, w), 'disocc_mask')
  gt_disp = _map(gt_disp, (b, h, w), 'gt_disp_trg')
  if valid_above is not None and valid is not None:
    flags |= LSI_EVAL_VALID_GT
  ts = target.stride()
  rc = _C.lib().lsi_eval_view_metrics(
      nl, b, ht, wt, h, w, int(x_min), int(y_min), _C.ptr(recons),
      _C.ptr(recons_disp), _C.ptr(target), ts[0], ts[1], ts[2], ts[3],
      _C.ptr(valid), _C.ptr(disocc), _C.ptr(gt_disp), flags,
      0.0 if valid_above is None else float(valid_above), _C.ptr(acc),
      _C.ptr(ws), ws_bytes, _C.stream_ptr(dev))
  _C.check(rc, 'lsi_eval_view_metrics')


def ssim_metric(acc2, recons, target, x_min, y_min, win, sigma):
  """lsi_eval_ssim: adds the sum of layer 0's SSIM over the windows and their
  number to `acc2`, two contiguous float64 on the device -- an accumulator of
  its own, not part of the SLOT_COUNT doubles."""
  from lsi.loss import _hip as loss_hip  # pylint: disable=g-import-not-at-top
  dev = _C.require_device(recons, target)
  if (acc2.device != dev or acc2.dtype != torch.float64 or acc2.numel() != 2 or
      not acc2.is_contiguous()):
    raise RuntimeError('the SSIM accumulator is 2 contiguous float64 on %s' % dev)
  recons = recons.contiguous()
  d = loss_hip.ssim_desc(recons, target, x_min, y_min, win, sigma, 'ssim_metric')
  # (the loss kernels' workspace: two partial sums per block)
  ws, n = loss_hip._workspace(dev)
  loss_hip.CALLS['ssim_eval'] += 1
  rc = _C.lib().lsi_eval_ssim(ctypes.byref(d), _C.ptr(recons), _C.ptr(target),
                              _C.ptr(acc2), _C.ptr(ws), n, _C.stream_ptr(dev))
  _C.check(rc, 'lsi_eval_ssim')


# the header's LSI_DEPTH_* slots of the depth accumulator (lsi_eval_depth_metrics)
DEPTH_SLOTS = _slots('LSI_DEPTH_', 'ABS_REL SQ_REL RMSE RMSE_LOG A1 A2 A3 SCALE IMAGES')
DEPTH_SLOT_COUNT, DEPTH_PER_IMAGE = _C.LSI_DEPTH_SLOTS, _C.LSI_DEPTH_PER_IMAGE
LSI_DEPTH_MASK_U8, LSI_DEPTH_MEDIAN = _C.LSI_DEPTH_MASK_U8, _C.LSI_DEPTH_MEDIAN
# metric name -> sum slot; the normaliser of every one is the IMAGES slot
DEPTH_METRICS = {
    'depth_abs_rel': 'ABS_REL', 'depth_sq_rel': 'SQ_REL', 'depth_rmse': 'RMSE',
    'depth_rmse_log': 'RMSE_LOG', 'depth_a1': 'A1', 'depth_a2': 'A2', 'depth_a3': 'A3',
    'depth_scale': 'SCALE',
}


def depth_workspace(dev, b, h, w, median):
  n = int(_C.lib().lsi_eval_depth_workspace_bytes(b, h, w, 1 if median else 0))
  return torch.empty((n,), dtype=torch.uint8, device=dev), n


def depth_metrics(acc9, pred, gt, gt_scale, ws, ws_bytes, mask=None, crop=None,
                  valid_above=0., depth_min=1e-3, depth_max=80., median=False,
                  per_image=None):
  """lsi_eval_depth_metrics: adds the depth accuracy of pred (B x H x W (x 1)
  inverse depth, fp32 or bf16) against gt (the same shape, fp32) to `acc9`, 9
  contiguous float64 on the device.  gt_scale: B fp32 on the device; mask
  B x H x W (x 1) fp32 or bool; crop (y0, y1, x0, x1) or None for the whole
  image; per_image: B x 10 float64 to be overwritten, or None."""
  if pred.dtype == torch.bfloat16:
    pred = pred.float()
  dev = _C.require_device(pred, gt, gt_scale)
  if (acc9.device != dev or acc9.dtype != torch.float64 or
      acc9.numel() != DEPTH_SLOT_COUNT or not acc9.is_contiguous()):
    raise RuntimeError('the depth accumulator is %d contiguous float64 on %s' %
                       (DEPTH_SLOT_COUNT, dev))
  if pred.dim() not in (3, 4):
    raise ValueError('depth_metrics: pred must be B x H x W (x 1), got %s' %
                     (tuple(pred.shape),))
  b, h, w = pred.shape[:3]
  pred = _map(pred, (b, h, w), 'pred')
  gt = _map(gt, (b, h, w), 'gt')
  if gt_scale.dtype != torch.float32 or tuple(gt_scale.shape) != (b,):
    raise ValueError('depth_metrics: gt_scale must be %d fp32, got %s %s' %
                     (b, gt_scale.dtype, tuple(gt_scale.shape)))
  gt_scale = gt_scale.contiguous()
  flags = LSI_DEPTH_MEDIAN if median else 0
  if mask is not None:
    if not mask.is_cuda or mask.device != dev:
      raise RuntimeError('lsi HIP ops need tensors on a ROCm GPU (got device %s); '
                         'there is no CPU fallback' % mask.device)
    if mask.dtype in (torch.bool, torch.uint8):
      flags |= LSI_DEPTH_MASK_U8
    elif mask.dtype != torch.float32:
      raise RuntimeError('the depth mask is fp32 or bool (got %s)' % mask.dtype)
    mask = _map(mask, (b, h, w), 'mask')
  if per_image is not None and (
      per_image.device != dev or per_image.dtype != torch.float64 or
      tuple(per_image.shape) != (b, DEPTH_PER_IMAGE) or not per_image.is_contiguous()):
    raise RuntimeError('per_image is %d x %d contiguous float64 on %s' %
                       (b, DEPTH_PER_IMAGE, dev))
  y0, y1, x0, x1 = (0, h, 0, w) if crop is None else [int(v) for v in crop]
  rc = _C.lib().lsi_eval_depth_metrics(
      b, h, w, _C.ptr(pred), _C.ptr(gt), _C.ptr(mask), _C.ptr(gt_scale), y0, y1, x0,
      x1, float(valid_above), float(depth_min), float(depth_max), flags,
      _C.ptr(acc9), _C.ptr(per_image), _C.ptr(ws), ws_bytes, _C.stream_ptr(dev))
  _C.check(rc, 'lsi_eval_depth_metrics')


def _layer_desc(tex, disp, bg_layer_disp):
  d = _C.LsiLossDesc()
  d.L, d.B, d.H, d.W = tex.shape[:4]
  d.img_sl, d.img_sb, d.img_sy, d.img_sx, d.img_sc = tex.stride()
  d.disp_sl, d.disp_sb, d.disp_sy, d.disp_sx = disp.stride()[:4]
  d.bg_layer_disp = float(bg_layer_disp)
  return d


def layer_metrics(acc, ws, ws_bytes, ldi_src, ldi_trg, imgs_src, imgs_trg, gt,
                  bg_layer_disp):
  """lsi_eval_layer_metrics: ldi_* = [tex L x B x H x W x 3, masks, disps
  L x B x H x W x 1] with any strides; gt as eval_metrics.layer_prediction_metrics
  takes it.  The four *_bg entries come together or not at all."""
  bg_keys = ('src_gt_disp_bg', 'src_gt_tex_bg', 'trg_gt_disp_bg', 'trg_gt_tex_bg')
  n_bg = sum(k in gt for k in bg_keys)
  if n_bg not in (0, len(bg_keys)):
    raise ValueError('layer_metrics: gt needs all of %s or none (got %s)' %
                     (bg_keys, sorted(k for k in bg_keys if k in gt)))
  views = []
  for ldi, img, side in ((ldi_src, imgs_src, 'src'), (ldi_trg, imgs_trg, 'trg')):
    tex, disp = ldi[0], ldi[2]
    nl, b, h, w, c = tex.shape
    if c != 3 or tuple(disp.shape) != (nl, b, h, w, 1):
      raise ValueError('layer_metrics: tex L x B x H x W x 3, disps L x B x H x W x 1')
    if tuple(img.shape) != (b, h, w, 3):
      raise ValueError('layer_metrics: images must be %s' % ((b, h, w, 3),))
    views.append((tex, disp, img.contiguous(),
                  _map(gt[side + '_gt_disp'], (b, h, w), side + '_gt_disp'),
                  _map(gt.get(side + '_gt_disp_bg'), (b, h, w), side + '_gt_disp_bg'),
                  None if n_bg == 0 else gt[side + '_gt_tex_bg'].contiguous()))
    if n_bg and tuple(views[-1][5].shape) != (b, h, w, 3):
      raise ValueError('layer_metrics: %s_gt_tex_bg must be %s' % (side, (b, h, w, 3)))
  dev = _C.require_device(*[t for v in views for t in v])
  for v, side in zip(views, ('src', 'trg')):
    _require_fp32('layer_metrics', **{'%s %s' % (side, k): t for k, t in zip(
        ('tex', 'disps', 'image', 'gt_disp', 'gt_disp_bg', 'gt_tex_bg'), v)})
  _check_acc(acc, dev)
  args = []
  for v in views:
    args += [ctypes.byref(_layer_desc(v[0], v[1], bg_layer_disp))]
    args += [_C.ptr(t) for t in v]
  rc = _C.lib().lsi_eval_layer_metrics(*args, _C.ptr(acc), _C.ptr(ws), ws_bytes,
                                       _C.stream_ptr(dev))
  _C.check(rc, 'lsi_eval_layer_metrics')


def disocclusion_mask(disps_src, disps_trg, src2trg_mat, thresh):
  """lsi_disocclusion_mask: disps B x H x W x 1, src2trg_mat B x 4 x 4; the source
  points are the pixel centres.  Returns the B x Hs x Ws x 1 fp32 mask."""
  dev = _C.require_device(disps_src, disps_trg, src2trg_mat)
  _require_fp32('disocclusion_mask', disps_src=disps_src, disps_trg=disps_trg,
                src2trg_mat=src2trg_mat)
  b, hs, ws_, _ = disps_src.shape
  _, ht, wt, _ = disps_trg.shape
  if tuple(src2trg_mat.shape) != (b, 4, 4) or disps_trg.shape[0] != b:
    raise ValueError('disocclusion_mask: src2trg_mat must be %s' % ((b, 4, 4),))
  disps_src, disps_trg = disps_src.contiguous(), disps_trg.contiguous()
  mat = src2trg_mat.contiguous()
  mask = torch.empty((b, hs, ws_, 1), dtype=torch.float32, device=dev)
  rc = _C.lib().lsi_disocclusion_mask(b, hs, ws_, ht, wt, _C.ptr(disps_src),
                                      _C.ptr(disps_trg), _C.ptr(mat), float(thresh),
                                      _C.ptr(mask), _C.stream_ptr(dev))
  _C.check(rc, 'lsi_disocclusion_mask')
  return mask
