"""torch.autograd bindings of the fused loss kernels (include/lsi_hip.h,
csrc/lsi_loss.hip).  Used for tensors on a ROCm device; there is no fallback:
a missing library raises in lsi._C.lib()."""
import ctypes

import torch

from lsi import _C


def _workspace(dev):
  n = int(_C.lib().lsi_loss_workspace_bytes())
  return torch.empty((n,), dtype=torch.uint8, device=dev), n


def _f32(t):
  return t if t.dtype == torch.float32 else t.float()


class _ZbufComp(torch.autograd.Function):
  """lsi_zbuf_comp_loss_fwd / _bwd (reference loss.py:66-115)."""

  @staticmethod
  def forward(ctx, imgs, masks, disps, trg, bg_layer_disp, max_disp, zbuf_scale):
    dev = _C.require_device(imgs, masks, disps, trg)
    nl, b, h, w, c = imgs.shape
    if c != 3:
      raise ValueError('zbuffer_composition_loss: 3-channel images (got %d)' % c)
    d = _C.LsiLossDesc()
    d.L, d.B, d.H, d.W = nl, b, h, w
    d.img_sl, d.img_sb, d.img_sy, d.img_sx, d.img_sc = imgs.stride()
    d.disp_sl, d.disp_sb, d.disp_sy, d.disp_sx = disps.stride()[:4]
    if masks is not None:
      d.mask_sl, d.mask_sb, d.mask_sy, d.mask_sx = masks.stride()[:4]
    d.trg_sb, d.trg_sy, d.trg_sx, d.trg_sc = trg.stride()
    d.bg_layer_disp, d.max_disp, d.zbuf_scale = (float(bg_layer_disp),
                                                 float(max_disp),
                                                 float(zbuf_scale))
    out = torch.empty((), dtype=torch.float32, device=dev)
    ws, n = _workspace(dev)
    rc = _C.lib().lsi_zbuf_comp_loss_fwd(
        ctypes.byref(d), _C.ptr(imgs), _C.ptr(masks), _C.ptr(disps), _C.ptr(trg),
        _C.ptr(out), _C.ptr(ws), n, _C.stream_ptr(dev))
    _C.check(rc, 'lsi_zbuf_comp_loss_fwd')
    ctx.desc = d
    ctx.has_mask = masks is not None
    ctx.save_for_backward(imgs, masks if masks is not None else imgs.new_empty(0),
                          disps, trg)
    return out

  @staticmethod
  def backward(ctx, g):
    imgs, masks, disps, trg = ctx.saved_tensors
    masks = masks if ctx.has_mask else None
    dev = imgs.device
    d = ctx.desc
    g = g.contiguous().float()
    g_imgs = torch.empty((d.L, d.B, d.H, d.W, 3), dtype=torch.float32, device=dev)
    g_disps = torch.empty((d.L, d.B, d.H, d.W, 1), dtype=torch.float32, device=dev)
    g_masks = (torch.empty((d.L, d.B, d.H, d.W, 1), dtype=torch.float32,
                           device=dev) if masks is not None else None)
    rc = _C.lib().lsi_zbuf_comp_loss_bwd(
        ctypes.byref(d), _C.ptr(imgs), _C.ptr(masks), _C.ptr(disps), _C.ptr(trg),
        _C.ptr(g), _C.ptr(g_imgs), _C.ptr(g_masks), _C.ptr(g_disps),
        _C.stream_ptr(dev))
    _C.check(rc, 'lsi_zbuf_comp_loss_bwd')
    return g_imgs, g_masks, g_disps, None, None, None, None


def zbuffer_composition_loss(layer_imgs, layer_masks, layer_disps, trg_imgs,
                             bg_layer_disp, max_disp, zbuf_scale):
  # the target images are data (ldi_enc_dec.py:269-294): the kernels produce no
  # gradient for them, and silently dropping one would be wrong
  if torch.is_tensor(trg_imgs) and trg_imgs.requires_grad:
    raise RuntimeError('zbuffer_composition_loss: trg_imgs is not '
                       'differentiable on the HIP path (pass trg_imgs.detach())')
  return _ZbufComp.apply(_f32(layer_imgs),
                         None if layer_masks is None else _f32(layer_masks),
                         _f32(layer_disps), _f32(trg_imgs), bg_layer_disp,
                         max_disp, zbuf_scale)


class _DispReg(torch.autograd.Function):
  """lsi_disp_reg_loss_fwd / _bwd: (smoothness, decreasing) in one read of the
  disparities (reference ldi.py:33-68, loss.py:48-63)."""

  @staticmethod
  def forward(ctx, disp):
    dev = _C.require_device(disp)
    nl, b, h, w = disp.shape[:4]
    out2 = torch.empty((2,), dtype=torch.float32, device=dev)
    ws, n = _workspace(dev)
    st = disp.stride()[:4]
    rc = _C.lib().lsi_disp_reg_loss_fwd(nl, b, h, w, st[0], st[1], st[2], st[3],
                                        _C.ptr(disp), _C.ptr(out2), _C.ptr(ws),
                                        n, _C.stream_ptr(dev))
    _C.check(rc, 'lsi_disp_reg_loss_fwd')
    ctx.save_for_backward(disp)
    return out2

  @staticmethod
  def backward(ctx, g2):
    disp, = ctx.saved_tensors
    dev = disp.device
    nl, b, h, w = disp.shape[:4]
    g2 = g2.contiguous().float()
    g_disp = torch.empty((nl, b, h, w, 1), dtype=torch.float32, device=dev)
    st = disp.stride()[:4]
    rc = _C.lib().lsi_disp_reg_loss_bwd(nl, b, h, w, st[0], st[1], st[2], st[3],
                                        _C.ptr(disp), _C.ptr(g2), _C.ptr(g_disp),
                                        _C.stream_ptr(dev))
    _C.check(rc, 'lsi_disp_reg_loss_bwd')
    return g_disp.reshape(disp.shape)


def disp_regularisers(pred_disp):
  """(disp_smoothness_loss, decreasing_disp_loss) of L x B x H x W x 1."""
  out2 = _DispReg.apply(_f32(pred_disp))
  return out2[0], out2[1]


class _ViewSynth(torch.autograd.Function):
  """lsi_view_synth_loss_fwd / _bwd (reference ldi_enc_dec.py:337-357)."""

  @staticmethod
  def forward(ctx, recons, target, x_min, y_min):
    dev = _C.require_device(recons, target)
    recons = recons.contiguous()
    nl, b, ht, wt, c = recons.shape
    _, h, w, _ = target.shape
    if c != 3:
      raise ValueError('view_synthesis_loss: 3-channel images (got %d)' % c)
    out = torch.empty((), dtype=torch.float32, device=dev)
    ws, n = _workspace(dev)
    ts = target.stride()
    rc = _C.lib().lsi_view_synth_loss_fwd(
        nl, b, ht, wt, h, w, x_min, y_min, _C.ptr(recons), _C.ptr(target),
        ts[0], ts[1], ts[2], ts[3], _C.ptr(out), _C.ptr(ws), n,
        _C.stream_ptr(dev))
    _C.check(rc, 'lsi_view_synth_loss_fwd')
    ctx.save_for_backward(recons, target)
    ctx.crop = (x_min, y_min)
    return out

  @staticmethod
  def backward(ctx, g):
    recons, target = ctx.saved_tensors
    dev = recons.device
    nl, b, ht, wt, _ = recons.shape
    _, h, w, _ = target.shape
    g = g.contiguous().float()
    g_recons = torch.empty_like(recons)
    ts = target.stride()
    rc = _C.lib().lsi_view_synth_loss_bwd(
        nl, b, ht, wt, h, w, ctx.crop[0], ctx.crop[1], _C.ptr(recons),
        _C.ptr(target), ts[0], ts[1], ts[2], ts[3], _C.ptr(g), _C.ptr(g_recons),
        _C.stream_ptr(dev))
    _C.check(rc, 'lsi_view_synth_loss_bwd')
    return g_recons, None, None, None


def view_synthesis_loss(recons_splat, to_recons_img, x_min, y_min):
  return _ViewSynth.apply(_f32(recons_splat), _f32(to_recons_img), int(x_min),
                          int(y_min))


# launches of the SSIM kernels through this binding (the loss and the metric)
CALLS = {'ssim_fwd': 0, 'ssim_bwd': 0, 'ssim_eval': 0}
SSIM_C1, SSIM_C2 = 1e-4, 9e-4  # (0.01 R)^2, (0.03 R)^2 at dynamic range R = 1


def ssim_desc(recons, target, x_min, y_min, win, sigma, what):
  """The LsiSsimDesc of recons nl x B x Ht x Wt x 3 against target B x H x W x 3;
  ValueError for what the kernels would refuse with LSI_EINVAL."""
  nl, b, ht, wt, c = recons.shape
  if c != 3 or tuple(target.shape[:1] + target.shape[3:]) != (b, 3):
    raise ValueError('%s: 3-channel images of one batch size' % what)
  _, h, w, _ = target.shape
  if h % ht or w % wt:
    raise ValueError('%s: the target (%d x %d) is no integer multiple of the '
                     'rendering (%d x %d)' % (what, h, w, ht, wt))
  win = int(win)
  if win < 3 or win > 11 or win % 2 == 0:
    raise ValueError('%s: the window size is odd, 3 .. 11 (got %d)' % (what, win))
  if ht - 2 * y_min < win or wt - 2 * x_min < win:
    raise ValueError('%s: the cropped rendering (%d x %d) holds no %d x %d window'
                     % (what, ht - 2 * y_min, wt - 2 * x_min, win, win))
  d = _C.LsiSsimDesc()
  d.nl, d.B, d.Ht, d.Wt, d.H, d.W = nl, b, ht, wt, h, w
  d.x_min, d.y_min, d.win = int(x_min), int(y_min), win
  d.sigma, d.c1, d.c2 = float(sigma), SSIM_C1, SSIM_C2
  d.t_sb, d.t_sy, d.t_sx, d.t_sc = target.stride()
  return d


class _Ssim(torch.autograd.Function):
  """lsi_ssim_loss_fwd / _bwd."""

  @staticmethod
  def forward(ctx, recons, target, x_min, y_min, win, sigma):
    dev = _C.require_device(recons, target)
    recons = recons.contiguous()
    d = ssim_desc(recons, target, x_min, y_min, win, sigma,
                  'ssim_view_synthesis_loss')
    out = torch.empty((), dtype=torch.float32, device=dev)
    ws, n = _workspace(dev)
    CALLS['ssim_fwd'] += 1
    rc = _C.lib().lsi_ssim_loss_fwd(ctypes.byref(d), _C.ptr(recons),
                                    _C.ptr(target), _C.ptr(out), _C.ptr(ws), n,
                                    _C.stream_ptr(dev))
    _C.check(rc, 'lsi_ssim_loss_fwd')
    ctx.save_for_backward(recons, target)
    ctx.desc = d
    return out

  @staticmethod
  def backward(ctx, g):
    recons, target = ctx.saved_tensors
    dev = recons.device
    g = g.contiguous().float()
    g_recons = torch.empty_like(recons)
    CALLS['ssim_bwd'] += 1
    rc = _C.lib().lsi_ssim_loss_bwd(ctypes.byref(ctx.desc), _C.ptr(recons),
                                    _C.ptr(target), _C.ptr(g), _C.ptr(g_recons),
                                    _C.stream_ptr(dev))
    _C.check(rc, 'lsi_ssim_loss_bwd')
    return g_recons, None, None, None, None, None


def ssim_view_synthesis_loss(recons_splat, to_recons_img, x_min, y_min, win, sigma):
  # the target is data, as in zbuffer_composition_loss
  if torch.is_tensor(to_recons_img) and to_recons_img.requires_grad:
    raise RuntimeError('ssim_view_synthesis_loss: to_recons_img is not '
                       'differentiable on the HIP path (pass '
                       'to_recons_img.detach())')
  return _Ssim.apply(_f32(recons_splat), _f32(to_recons_img), int(x_min),
                     int(y_min), int(win), float(sigma))


def ssim_window(win, sigma):
  """lsi_ssim_window: the `win` fp32 weights the kernels use (host only)."""
  out = (ctypes.c_float * min(max(int(win), 1), 16))()
  rc = _C.lib().lsi_ssim_window(int(win), float(sigma),
                                ctypes.cast(out, ctypes.c_void_p))
  if rc != _C.LSI_OK:
    raise ValueError('ssim_window: the window size is odd, 3 .. 11 (got %d)' % win)
  return list(out)


# launches of the edge-aware smoothness kernels through this binding
CALLS.update({'edge_fwd': 0, 'edge_bwd': 0})
EDGE_EPS = 1e-7


def edge_smooth_desc(disp, guide, alpha, order, normalise, what):
  """The LsiEdgeSmoothDesc of disp L x B x H x W x 1 guided by B x H x W x 3 (all
  layers) or L x B x H x W x 3 (per layer); ValueError for what the kernels would
  refuse with LSI_EINVAL and for a guide of another shape."""
  if disp.dim() != 5 or disp.shape[4] != 1:
    raise ValueError('%s: disparities L x B x H x W x 1 (got %s)' %
                     (what, tuple(disp.shape)))
  nl, b, h, w, _ = disp.shape
  if tuple(guide.shape) == (b, h, w, 3):
    g_sl, (g_sb, g_sy, g_sx, g_sc) = 0, guide.stride()
  elif tuple(guide.shape) == (nl, b, h, w, 3):
    g_sl, g_sb, g_sy, g_sx, g_sc = guide.stride()
  else:
    raise ValueError('%s: the guide is %s or %s, 3 channels (got %s)' %
                     (what, (b, h, w, 3), (nl, b, h, w, 3), tuple(guide.shape)))
  if order not in (1, 2):
    raise ValueError('%s: the order is 1 or 2 (got %r)' % (what, order))
  if min(nl, b) < 1 or h < order + 1 or w < order + 1:
    raise ValueError('%s: order %d needs at least %d rows and columns (got %d x '
                     '%d)' % (what, order, order + 1, h, w))
  alpha = float(alpha)
  if not (alpha >= 0.0 and alpha != float('inf')):
    raise ValueError('%s: alpha is finite and >= 0 (got %r)' % (what, alpha))
  d = _C.LsiEdgeSmoothDesc()
  d.L, d.B, d.H, d.W, d.order, d.normalise = nl, b, h, w, order, int(bool(normalise))
  d.d_sl, d.d_sb, d.d_sy, d.d_sx = disp.stride()[:4]
  d.g_sl, d.g_sb, d.g_sy, d.g_sx, d.g_sc = g_sl, g_sb, g_sy, g_sx, g_sc
  d.alpha, d.eps = alpha, EDGE_EPS
  return d


class _EdgeSmooth(torch.autograd.Function):
  """lsi_edge_smooth_loss_fwd / _bwd."""

  @staticmethod
  def forward(ctx, disp, guide, alpha, order, normalise):
    dev = _C.require_device(disp, guide)
    d = edge_smooth_desc(disp, guide, alpha, order, normalise,
                         'edge_smoothness_loss')
    out = torch.empty((), dtype=torch.float32, device=dev)
    sums = torch.empty((3 * d.L * d.B,), dtype=torch.float64, device=dev)
    n = int(_C.lib().lsi_edge_smooth_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty((n,), dtype=torch.uint8, device=dev)
    CALLS['edge_fwd'] += 1
    rc = _C.lib().lsi_edge_smooth_loss_fwd(ctypes.byref(d), _C.ptr(disp),
                                           _C.ptr(guide), _C.ptr(out),
                                           _C.ptr(sums), _C.ptr(ws), n,
                                           _C.stream_ptr(dev))
    _C.check(rc, 'lsi_edge_smooth_loss_fwd')
    ctx.save_for_backward(disp, guide, sums)
    ctx.desc = d
    return out

  @staticmethod
  def backward(ctx, g):
    disp, guide, sums = ctx.saved_tensors
    dev = disp.device
    g = g.contiguous().float()
    g_disp = torch.empty(tuple(disp.shape), dtype=torch.float32, device=dev)
    CALLS['edge_bwd'] += 1
    rc = _C.lib().lsi_edge_smooth_loss_bwd(ctypes.byref(ctx.desc), _C.ptr(disp),
                                           _C.ptr(guide), _C.ptr(sums), _C.ptr(g),
                                           _C.ptr(g_disp), _C.stream_ptr(dev))
    _C.check(rc, 'lsi_edge_smooth_loss_bwd')
    return g_disp, None, None, None, None


def edge_smoothness_loss(disp, guide, alpha, order, normalise):
  """Edge-aware smoothness of disp L x B x H x W x 1 (any strides) under guide
  B x H x W x 3 or L x B x H x W x 3; the gradient is w.r.t. disp only."""
  # the guide is data, as the target of zbuffer_composition_loss
  if torch.is_tensor(guide) and guide.requires_grad:
    raise RuntimeError('edge_smoothness_loss: the guide is not differentiable '
                       'on the HIP path (pass guide.detach())')
  if isinstance(order, bool) or int(order) != order:
    raise ValueError('edge_smoothness_loss: the order is 1 or 2 (got %r)' % (order,))
  return _EdgeSmooth.apply(_f32(disp), _f32(guide), float(alpha), int(order),
                           bool(normalise))


# launches of the depth-supervision kernels through this binding
CALLS.update({'depth_sup_fwd': 0, 'depth_sup_bwd': 0})
DEPTH_SUP_MODES = {'silog': _C.LSI_DEPTH_SUP_SILOG, 'l1': _C.LSI_DEPTH_SUP_L1}


def depth_sup_desc(pred, gt, gt_scale, mode, lam, valid_above, g_min, g_max, eps,
                   what):
  """The LsiDepthSupDesc of pred P x H x W against gt P x H x W (any strides) and
  gt_scale (P floats or None); RuntimeError for a wrong shape or dtype,
  ValueError for what the kernels would refuse with LSI_EINVAL."""
  for name, t in (('pred', pred), ('gt', gt), ('gt_scale', gt_scale)):
    if t is not None and t.dtype != torch.float32:
      raise RuntimeError('%s: %s is fp32 (got %s)' % (what, name, t.dtype))
  if pred.dim() != 3 or tuple(gt.shape) != tuple(pred.shape):
    raise RuntimeError('%s: pred and gt are P x H x W, of one shape (got %s and %s)'
                       % (what, tuple(pred.shape), tuple(gt.shape)))
  p, h, w = pred.shape
  if gt_scale is not None and tuple(gt_scale.shape) != (p,):
    raise RuntimeError('%s: gt_scale holds one float per plane, %s (got %s)' %
                       (what, (p,), tuple(gt_scale.shape)))
  if mode not in DEPTH_SUP_MODES:
    raise ValueError("%s: the mode is 'silog' or 'l1' (got %r)" % (what, mode))
  if min(p, h, w) < 1:
    raise ValueError('%s: empty maps (%s)' % (what, tuple(pred.shape)))
  lam, valid_above, g_min, g_max, eps = (float(lam), float(valid_above),
                                         float(g_min), float(g_max), float(eps))
  inf = float('inf')
  if not 0.0 <= lam <= 1.0:
    raise ValueError('%s: lambda lies in [0, 1] (got %r)' % (what, lam))
  if not 0.0 <= valid_above < inf:
    raise ValueError('%s: valid_above is finite and >= 0 (got %r)' %
                     (what, valid_above))
  if not 0.0 < g_min <= g_max < inf:
    raise ValueError('%s: 0 < 1 / depth_max <= 1 / depth_min < inf (got %r, %r)' %
                     (what, g_min, g_max))
  if not 0.0 < eps < inf:
    raise ValueError('%s: eps is finite and > 0 (got %r)' % (what, eps))
  d = _C.LsiDepthSupDesc()
  d.P, d.H, d.W, d.mode = p, h, w, DEPTH_SUP_MODES[mode]
  d.p_sp, d.p_sy, d.p_sx = pred.stride()
  d.g_sp, d.g_sy, d.g_sx = gt.stride()
  d.valid_above, d.g_min, d.g_max, d.eps, d.lam = valid_above, g_min, g_max, eps, lam
  return d


class _DepthSup(torch.autograd.Function):
  """lsi_depth_sup_loss_fwd / _bwd."""

  @staticmethod
  def forward(ctx, pred, gt, gt_scale, mode, lam, valid_above, g_min, g_max, eps):
    d = depth_sup_desc(pred, gt, gt_scale, mode, lam, valid_above, g_min, g_max,
                       eps, 'depth_supervision_loss')
    dev = _C.require_device(pred, gt, gt_scale)
    if gt_scale is not None:
      gt_scale = gt_scale.contiguous()
    out = torch.empty((), dtype=torch.float32, device=dev)
    sums = torch.empty((3 * d.P,), dtype=torch.float64, device=dev)
    n = int(_C.lib().lsi_depth_sup_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty((n,), dtype=torch.uint8, device=dev)
    CALLS['depth_sup_fwd'] += 1
    rc = _C.lib().lsi_depth_sup_loss_fwd(ctypes.byref(d), _C.ptr(pred), _C.ptr(gt),
                                         _C.ptr(gt_scale), _C.ptr(out),
                                         _C.ptr(sums), _C.ptr(ws), n,
                                         _C.stream_ptr(dev))
    _C.check(rc, 'lsi_depth_sup_loss_fwd')
    ctx.save_for_backward(pred, gt, sums,
                          gt_scale if gt_scale is not None else pred.new_empty(0))
    ctx.has_scale = gt_scale is not None
    ctx.desc = d
    ctx.mark_non_differentiable(sums)
    return out, sums

  @staticmethod
  def backward(ctx, g, _):
    pred, gt, sums, gt_scale = ctx.saved_tensors
    gt_scale = gt_scale if ctx.has_scale else None
    dev = pred.device
    g = g.contiguous().float()
    g_pred = torch.empty(tuple(pred.shape), dtype=torch.float32, device=dev)
    CALLS['depth_sup_bwd'] += 1
    rc = _C.lib().lsi_depth_sup_loss_bwd(ctypes.byref(ctx.desc), _C.ptr(pred),
                                         _C.ptr(gt), _C.ptr(gt_scale), _C.ptr(sums),
                                         _C.ptr(g), _C.ptr(g_pred),
                                         _C.stream_ptr(dev))
    _C.check(rc, 'lsi_depth_sup_loss_bwd')
    return (g_pred,) + (None,) * 8


def depth_supervision_loss(pred, gt, gt_scale, mode, lam, valid_above, g_min, g_max,
                           eps, return_plane_sums=False):
  """Depth supervision of pred P x H x W (any strides, never copied) against the
  sparse ground truth gt P x H x W, gt_scale P floats or None; the gradient is
  w.r.t. pred only.  return_plane_sums: also the 3 P doubles (n_p, A_p, Q_p)
  the forward left for the backward."""
  # the ground truth is data, as the target of zbuffer_composition_loss
  for name, t in (('gt', gt), ('gt_scale', gt_scale)):
    if torch.is_tensor(t) and t.requires_grad:
      raise RuntimeError('depth_supervision_loss: %s is not differentiable on the '
                         'HIP path (pass %s.detach())' % (name, name))
  out, sums = _DepthSup.apply(pred, gt, gt_scale, mode, lam, valid_above, g_min,
                              g_max, eps)
  return (out, sums) if return_plane_sums else out


# launches of the geometric-consistency kernels through this binding
CALLS.update({'geo_cons_fwd': 0, 'geo_cons_bwd': 0})
GEO_CONS_MODES = {'ratio': _C.LSI_GEO_CONS_RATIO, 'l1': _C.LSI_GEO_CONS_L1}


def geo_cons_desc(disp, partner, mats, mode, occl_thresh, what):
  """The LsiGeoConsDesc of disp P x H x W (any strides) against partner P x H x W
  (any strides), or against its own other half when partner is None (P even,
  shift P / 2), under mats P x 4 x 4; RuntimeError for a wrong shape or dtype,
  ValueError for what the kernels would refuse with LSI_EINVAL."""
  for name, t in (('disps', disp), ('partner_disps', partner), ('mats', mats)):
    if t is not None and t.dtype != torch.float32:
      raise RuntimeError('%s: %s is fp32 (got %s)' % (what, name, t.dtype))
  if disp.dim() != 3:
    raise RuntimeError('%s: disps are P x H x W (got %s)' % (what, tuple(disp.shape)))
  p, h, w = disp.shape
  if partner is not None and tuple(partner.shape) != (p, h, w):
    raise RuntimeError('%s: disps and partner_disps are P x H x W, of one shape (got '
                       '%s and %s)' % (what, (p, h, w), tuple(partner.shape)))
  if tuple(mats.shape) != (p, 4, 4):
    raise RuntimeError('%s: mats holds one 4 x 4 matrix per plane, %s (got %s)' %
                       (what, (p, 4, 4), tuple(mats.shape)))
  if mode not in GEO_CONS_MODES:
    raise ValueError("%s: the mode is 'ratio' or 'l1' (got %r)" % (what, mode))
  if min(p, h, w) < 1:
    raise ValueError('%s: empty maps (%s)' % (what, (p, h, w)))
  if partner is None and p % 2:
    raise ValueError('%s: the paired form needs an even number of planes, the two '
                     "views' halves (got %d)" % (what, p))
  if p > 65535 or h * w >= 1 << 24 or p * h * w > 2 ** 31 - 1:
    raise ValueError('%s: at most 65535 planes of fewer than 2^24 pixels, 2^31 - 1 '
                     'pixels in all (got %s)' % (what, (p, h, w)))
  occl_thresh = float(occl_thresh)
  if not 0.0 <= occl_thresh < 1.0:
    raise ValueError('%s: occl_thresh lies in [0, 1) (got %r)' % (what, occl_thresh))
  d = _C.LsiGeoConsDesc()
  d.P, d.H, d.W, d.mode = p, h, w, GEO_CONS_MODES[mode]
  d.d_sp, d.d_sy, d.d_sx = disp.stride()
  d.e_sp, d.e_sy, d.e_sx = (disp if partner is None else partner).stride()
  d.shift, d.occl_thresh = (p // 2 if partner is None else 0), occl_thresh
  return d


class _GeoCons(torch.autograd.Function):
  """lsi_geo_cons_loss_fwd / _bwd.  partner None: the paired
  form, one gradient buffer."""

  @staticmethod
  def forward(ctx, disp, partner, mats, mode, occl_thresh, want_map):
    d = geo_cons_desc(disp, partner, mats, mode, occl_thresh,
                      'geometric_consistency_loss')
    dev = _C.require_device(disp, partner, mats)
    mats = mats.contiguous()
    e = disp if partner is None else partner
    out = torch.empty((), dtype=torch.float32, device=dev)
    sums = torch.empty((3 * d.P,), dtype=torch.float64, device=dev)
    emap = (torch.empty((d.P, d.H, d.W), dtype=torch.float32, device=dev)
            if want_map else None)
    n = int(_C.lib().lsi_geo_cons_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty((n,), dtype=torch.uint8, device=dev)
    CALLS['geo_cons_fwd'] += 1
    rc = _C.lib().lsi_geo_cons_loss_fwd(ctypes.byref(d), _C.ptr(disp), _C.ptr(e),
                                        _C.ptr(mats), _C.ptr(out), _C.ptr(sums),
                                        _C.ptr(emap), _C.ptr(ws), n,
                                        _C.stream_ptr(dev))
    _C.check(rc, 'lsi_geo_cons_loss_fwd')
    ctx.save_for_backward(disp, mats, sums,
                          partner if partner is not None else disp.new_empty(0))
    ctx.paired = partner is None
    ctx.desc = d
    if emap is None:
      emap = disp.new_empty(0)
    ctx.mark_non_differentiable(sums, emap)
    return out, sums, emap

  @staticmethod
  def backward(ctx, g, _s, _m):
    disp, mats, sums, partner = ctx.saved_tensors
    dev = disp.device
    d = ctx.desc
    g = g.contiguous().float()
    shape = (d.P, d.H, d.W)
    g_disp = torch.empty(shape, dtype=torch.float32, device=dev)
    g_partner = (None if ctx.paired else
                 torch.empty(shape, dtype=torch.float32, device=dev))
    CALLS['geo_cons_bwd'] += 1
    rc = _C.lib().lsi_geo_cons_loss_bwd(ctypes.byref(d), _C.ptr(disp),
                                        _C.ptr(disp if ctx.paired else partner),
                                        _C.ptr(mats), _C.ptr(sums), _C.ptr(g),
                                        _C.ptr(g_disp), _C.ptr(g_partner),
                                        _C.stream_ptr(dev))
    _C.check(rc, 'lsi_geo_cons_loss_bwd')
    return g_disp, g_partner, None, None, None, None


def geometric_consistency_loss(disp, partner, mats, mode, occl_thresh,
                               return_map=False, return_plane_sums=False):
  """Geometric consistency of disp P x H x W (any strides, never copied) with
  partner P x H x W, or with its own other half (partner None), under mats
  P x 4 x 4; the gradient is w.r.t. disp and partner.  return_map: also the
  per-pixel term, -1 where unscored; return_plane_sums: also the 3 P doubles
  (sum e, N_p, 0) the forward left for the backward."""
  # the cameras are constants here
  if torch.is_tensor(mats) and mats.requires_grad:
    raise RuntimeError('geometric_consistency_loss: mats is not differentiable on '
                       'the HIP path (pass mats.detach())')
  out, sums, emap = _GeoCons.apply(disp, partner, mats, mode, occl_thresh,
                                   bool(return_map))
  res = (out,) + ((emap,) if return_map else ()) + ((sums,) if return_plane_sums else ())
  return res if len(res) > 1 else out


# launches of the photometric-reprojection kernels through this binding
CALLS.update({'photo_reproj_fwd': 0, 'photo_reproj_bwd': 0})
PHOTO_MODES = {'l1': _C.LSI_PHOTO_L1, 'charb': _C.LSI_PHOTO_CHARB}


def photo_reproj_desc(tex, disp, img, mats, partner, shift, mode, occl_thresh, eps,
                      what):
  """The LsiPhotoReprojDesc of tex L x Q x H x W x C and disp L x Q x H x W (plane
  p = l Q + q) against img Q x H x W x C under mats Q x 4 x 4, partner Q x H x W
  or None (any strides); RuntimeError for a wrong shape or dtype, ValueError for
  what the kernels would refuse with LSI_EINVAL."""
  for name, t in (('layer_imgs', tex), ('layer_disps', disp), ('other_imgs', img),
                  ('mats', mats), ('partner_disps', partner)):
    if t is not None and t.dtype != torch.float32:
      raise RuntimeError('%s: %s is fp32 (got %s)' % (what, name, t.dtype))
  if tex.dim() != 5 or disp.dim() != 4 or tuple(tex.shape[:4]) != tuple(disp.shape):
    raise RuntimeError('%s: layer_imgs are L x Q x H x W x C and layer_disps L x Q x H x '
                       'W, of one shape (got %s and %s)' %
                       (what, tuple(tex.shape), tuple(disp.shape)))
  nl, nq, h, w, c = tex.shape
  p = nl * nq
  if img.dim() != 4 or tuple(img.shape[1:]) != (h, w, c):
    raise RuntimeError('%s: other_imgs are Q x H x W x C, %s (got %s)' %
                       (what, ('Q', h, w, c), tuple(img.shape)))
  q = img.shape[0]
  if nq != q:
    raise RuntimeError('%s: layer_imgs hold L layers of the Q = %d views of other_imgs '
                       '(got %s)' % (what, q, tuple(tex.shape)))
  if partner is not None and tuple(partner.shape) != (q, h, w):
    raise RuntimeError('%s: partner_disps are Q x H x W, of one shape with other_imgs, '
                       '%s (got %s)' % (what, (q, h, w), tuple(partner.shape)))
  if tuple(mats.shape) != (q, 4, 4):
    raise RuntimeError('%s: mats holds one 4 x 4 matrix per image, %s (got %s)' %
                       (what, (q, 4, 4), tuple(mats.shape)))
  if mode not in PHOTO_MODES:
    raise ValueError("%s: the mode is 'l1' or 'charb' (got %r)" % (what, mode))
  if min(p, q, h, w) < 1:
    raise ValueError('%s: empty maps (%s over %d images)' % (what, (p, h, w), q))
  if not 1 <= c <= 4:
    raise ValueError('%s: 1 to 4 channels (got %d)' % (what, c))
  if p > 65535 or h * w >= 1 << 24 or p * h * w > 2 ** 31 - 1:
    raise ValueError('%s: at most 65535 planes of fewer than 2^24 pixels, 2^31 - 1 '
                     'pixels in all (got %s)' % (what, (p, h, w)))
  if isinstance(shift, bool) or int(shift) != shift or not 0 <= shift < q:
    raise ValueError('%s: shift is an integer in [0, %d) (got %r)' % (what, q, shift))
  occl_thresh, eps = float(occl_thresh), float(eps)
  if not 0.0 <= occl_thresh < 1.0:
    raise ValueError('%s: occl_thresh lies in [0, 1) (got %r)' % (what, occl_thresh))
  if partner is None and occl_thresh > 0.0:
    raise ValueError('%s: occl_thresh > 0 needs partner_disps (got %r without)' %
                     (what, occl_thresh))
  if not 0.0 < eps < float('inf'):
    raise ValueError('%s: eps is finite and > 0 (got %r)' % (what, eps))
  d = _C.LsiPhotoReprojDesc()
  d.P, d.Q, d.H, d.W, d.C, d.mode = p, q, h, w, c, PHOTO_MODES[mode]
  d.t_sl, d.t_sq, d.t_sy, d.t_sx, d.t_sc = tex.stride()
  d.d_sl, d.d_sq, d.d_sy, d.d_sx = disp.stride()
  d.i_sq, d.i_sy, d.i_sx, d.i_sc = img.stride()
  if partner is not None:
    d.e_sq, d.e_sy, d.e_sx = partner.stride()
  d.shift, d.occl_thresh, d.eps = int(shift), occl_thresh, eps
  return d


class _PhotoReproj(torch.autograd.Function):
  """lsi_photo_reproj_loss_fwd / _bwd."""

  @staticmethod
  def forward(ctx, tex, disp, img, mats, partner, shift, mode, occl_thresh, eps,
              want_map):
    d = photo_reproj_desc(tex, disp, img, mats, partner, shift, mode, occl_thresh, eps,
                          'photometric_reprojection_loss')
    dev = _C.require_device(tex, disp, img, mats, partner)
    mats = mats.contiguous()
    out = torch.empty((), dtype=torch.float32, device=dev)
    sums = torch.empty((3 * d.P,), dtype=torch.float64, device=dev)
    emap = (torch.empty((d.P, d.H, d.W), dtype=torch.float32, device=dev)
            if want_map else None)
    n = int(_C.lib().lsi_photo_reproj_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty((n,), dtype=torch.uint8, device=dev)
    CALLS['photo_reproj_fwd'] += 1
    rc = _C.lib().lsi_photo_reproj_loss_fwd(
        ctypes.byref(d), _C.ptr(tex), _C.ptr(disp), _C.ptr(img), _C.ptr(mats),
        _C.ptr(partner), _C.ptr(out), _C.ptr(sums), _C.ptr(emap), _C.ptr(ws), n,
        _C.stream_ptr(dev))
    _C.check(rc, 'lsi_photo_reproj_loss_fwd')
    ctx.save_for_backward(tex, disp, img, mats, sums,
                          partner if partner is not None else disp.new_empty(0))
    ctx.has_partner = partner is not None
    ctx.desc = d
    if emap is None:
      emap = disp.new_empty(0)
    ctx.mark_non_differentiable(sums, emap)
    return out, sums, emap

  @staticmethod
  def backward(ctx, g, _s, _m):
    tex, disp, img, mats, sums, partner = ctx.saved_tensors
    partner = partner if ctx.has_partner else None
    dev = disp.device
    d = ctx.desc
    g = g.contiguous().float()
    need_tex, need_disp = ctx.needs_input_grad[:2]
    if not (need_tex or need_disp):
      return (None,) * 10
    g_tex = (torch.empty(tuple(tex.shape), dtype=torch.float32, device=dev)
             if need_tex else None)
    g_disp = (torch.empty(tuple(disp.shape), dtype=torch.float32, device=dev)
              if need_disp else None)
    CALLS['photo_reproj_bwd'] += 1
    rc = _C.lib().lsi_photo_reproj_loss_bwd(
        ctypes.byref(d), _C.ptr(tex), _C.ptr(disp), _C.ptr(img), _C.ptr(mats),
        _C.ptr(partner), _C.ptr(sums), _C.ptr(g), _C.ptr(g_tex), _C.ptr(g_disp),
        _C.stream_ptr(dev))
    _C.check(rc, 'lsi_photo_reproj_loss_bwd')
    return (g_tex, g_disp) + (None,) * 8


def photometric_reprojection_loss(tex, disp, img, mats, partner, shift, mode,
                                  occl_thresh, eps, return_map=False,
                                  return_plane_sums=False):
  """Backward-warp photometric loss of tex L x Q x H x W x C at disp L x Q x H x W
  (any strides, never copied; plane p = l Q + q) against img Q x H x W x C sampled
  under mats Q x 4 x 4, partner Q x H x W or None; the gradient is w.r.t. tex and
  disp.  return_map:
  also the per-pixel term, -1 where unscored; return_plane_sums: also the 3 P
  doubles (sum e, N_p, 0) the forward left for the backward."""
  # the sampled views and the cameras are constants here
  for name, t in (('other_imgs', img), ('mats', mats), ('partner_disps', partner)):
    if torch.is_tensor(t) and t.requires_grad:
      raise RuntimeError('photometric_reprojection_loss: %s is not differentiable on '
                         'the HIP path (pass %s.detach())' % (name, name))
  out, sums, emap = _PhotoReproj.apply(tex, disp, img, mats, partner, shift, mode,
                                       occl_thresh, eps, bool(return_map))
  res = (out,) + ((emap,) if return_map else ()) + ((sums,) if return_plane_sums else ())
  return res if len(res) > 1 else out


class _Compose(torch.autograd.Function):
  """lsi_compose_fwd / lsi_compose_bwd on imgs [L,N,C], masks [L,N], dmaps
  [L,N] (contiguous fp32)."""

  @staticmethod
  def forward(ctx, imgs, masks, dmaps, soft, min_disp, temp):
    dev = imgs.device
    nl, n, c = imgs.shape
    out = torch.empty((n, c), dtype=torch.float32, device=dev)
    rc = _C.lib().lsi_compose_fwd(nl, n, c, _C.ptr(imgs), _C.ptr(masks),
                                  _C.ptr(dmaps), soft, min_disp, temp,
                                  _C.ptr(out), _C.stream_ptr(dev))
    _C.check(rc, 'lsi_compose_fwd')
    ctx.save_for_backward(imgs, masks, dmaps)
    ctx.args = (soft, min_disp, temp)
    return out

  @staticmethod
  def backward(ctx, g_out):
    imgs, masks, dmaps = ctx.saved_tensors
    dev = imgs.device
    nl, n, c = imgs.shape
    # inputs that need no gradient get no work
    grads = [torch.empty_like(x) if need else None
             for x, need in zip((imgs, masks, dmaps), ctx.needs_input_grad)]
    rc = _C.lib().lsi_compose_bwd(nl, n, c, _C.ptr(imgs), _C.ptr(masks),
                                  _C.ptr(dmaps), *ctx.args,
                                  _C.ptr(_f32(g_out).contiguous()),
                                  *[_C.ptr(g) for g in grads], _C.stream_ptr(dev))
    _C.check(rc, 'lsi_compose_bwd')
    return tuple(grads) + (None, None, None)


def _refuse_grad(what, tensors):
  # an input that asks for a gradient must not lose it silently: without the
  # caller's differentiable=True the call is the forward-only one it always was
  if any(x.requires_grad for x in tensors):
    raise RuntimeError('%s on the GPU is forward-only unless it is called with '
                       'differentiable=True' % what)


def compose(imgs, masks, dmaps, soft, min_disp, depth_softmax_temp,
            differentiable=False):
  """lsi_compose_fwd (reference layers.py:29-70); with differentiable=True also
  lsi_compose_bwd: the gradients of imgs, masks and dmaps as TF differentiates
  the reference's graph."""
  _C.require_device(imgs, masks, dmaps)
  if not differentiable:
    _refuse_grad('layers.compose', (imgs, masks, dmaps))
  nl, c = imgs.shape[0], imgs.shape[-1]
  lead = tuple(imgs.shape[1:-1])
  imgs_c = _f32(imgs).reshape(nl, -1, c).contiguous()
  masks_c = _f32(masks).reshape(nl, -1).contiguous()
  dmaps_c = _f32(dmaps).reshape(nl, -1).contiguous()
  out = _Compose.apply(imgs_c, masks_c, dmaps_c, int(bool(soft)), float(min_disp),
                       float(depth_softmax_temp))
  return out.reshape(lead + (c,))


class _ComposeDepth(torch.autograd.Function):
  """lsi_compose_depth_fwd / lsi_compose_depth_bwd on masks, dmaps [L,N]."""

  @staticmethod
  def forward(ctx, masks, dmaps, bg_layer, min_disp, temp):
    dev = masks.device
    nl, n = masks.shape
    # tf.reduce_max over the relu'd maps with the background layer appended
    dmax = 0.0
    if bg_layer:
      dmax = max(float(torch.relu(dmaps).max()), min_disp)
    out = torch.empty((n,), dtype=torch.float32, device=dev)
    rc = _C.lib().lsi_compose_depth_fwd(nl, n, _C.ptr(masks), _C.ptr(dmaps),
                                        bg_layer, dmax, min_disp, temp,
                                        _C.ptr(out), _C.stream_ptr(dev))
    _C.check(rc, 'lsi_compose_depth_fwd')
    ctx.save_for_backward(masks, dmaps)
    ctx.args = (bg_layer, dmax, min_disp, temp)
    return out

  @staticmethod
  def backward(ctx, g_out):
    masks, dmaps = ctx.saved_tensors
    # the masks only select the layer (one_hot(argmax)): a zero gradient
    g_masks = torch.zeros_like(masks) if ctx.needs_input_grad[0] else None
    if not ctx.needs_input_grad[1]:
      return g_masks, None, None, None, None
    dev = masks.device
    nl, n = masks.shape
    g_dmaps = torch.empty_like(dmaps)
    rc = _C.lib().lsi_compose_depth_bwd(nl, n, _C.ptr(masks), _C.ptr(dmaps),
                                        *ctx.args, _C.ptr(_f32(g_out).contiguous()),
                                        _C.ptr(g_dmaps), _C.stream_ptr(dev))
    _C.check(rc, 'lsi_compose_depth_bwd')
    return g_masks, g_dmaps, None, None, None


def compose_depth(masks, dmaps, bg_layer, min_disp, depth_softmax_temp,
                  differentiable=False):
  """lsi_compose_depth_fwd (reference layers.py:73-115); with
  differentiable=True also lsi_compose_depth_bwd (the selected layer's
  disparity takes the gradient, the masks' is zero)."""
  _C.require_device(masks, dmaps)
  if not differentiable:
    _refuse_grad('layers.compose_depth', (masks, dmaps))
  nl = masks.shape[0]
  lead = tuple(masks.shape[1:-1])
  masks_c = _f32(masks).reshape(nl, -1).contiguous()
  dmaps_c = _f32(dmaps).reshape(nl, -1).contiguous()
  out = _ComposeDepth.apply(masks_c, dmaps_c, int(bool(bg_layer)), float(min_disp),
                            float(depth_softmax_temp))
  return out.reshape(lead + (1,))
