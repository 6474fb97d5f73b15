"""Loss functions on LDIs (mirror of the reference's lsi/loss/loss.py) plus the
view-synthesis loss the reference computes inline in ldi_enc_dec.py:337-357.

The three losses are fused HIP kernels (csrc/lsi_loss.hip, forward and
backward); tensors that do not live on a ROCm device raise, as for the
renderer -- there is no second implementation (the torch restatements the
tests check gradients against live in oracle/lsi_torch_ref.py)."""
import math

import torch



def event_prob(layer_masks):
  """Per-pixel ordered-multiplication layer probabilities (reference
  loss.py:27-45; dead code there, kept for surface parity)."""
  eps = 1e-6
  layer_masks = torch.clamp(layer_masks, eps, 1 - eps)
  log_inv_m = torch.log(1 - layer_masks)
  log_prob = torch.cumsum(log_inv_m, dim=0) - log_inv_m + torch.log(layer_masks)
  layer_probs = torch.exp(log_prob)
  escape_probs = 1 - torch.sum(layer_probs, dim=0, keepdim=True)
  return layer_probs, escape_probs


def decreasing_disp_loss(layer_disps):
  """Penalises disparities that increase from one layer to the next, with the
  nearer layer detached (reference loss.py:48-63).  On a ROCm device: the fused
  HIP kernel (lsi_disp_reg_loss_fwd)."""
  n_layers = layer_disps.shape[0]
  if n_layers == 1:
    return 0
  from lsi.loss import _hip  # pylint: disable=g-import-not-at-top
  return _hip.disp_regularisers(layer_disps)[1]


def zbuffer_composition_loss(layer_imgs, layer_masks, layer_disps, trg_imgs,
                             bg_layer_disp=0, max_disp=1, zbuf_scale=10):
  """Depth+mask weighted self-consistency loss with a white background layer
  (reference loss.py:66-115).  On a ROCm device: one fused HIP pass
  (lsi_zbuf_comp_loss_fwd / _bwd)."""
  from lsi.loss import _hip  # pylint: disable=g-import-not-at-top
  return _hip.zbuffer_composition_loss(layer_imgs, layer_masks, layer_disps,
                                       trg_imgs, bg_layer_disp, max_disp,
                                       zbuf_scale)


def area_downsample(img, ht, wt):
  """tf.image.resize_images(..., AREA) for integer reduction factors: exact box
  mean.  img: B x H x W x C."""
  b, h, w, c = img.shape
  fy, fx = h // ht, w // wt
  if fy * ht != h or fx * wt != w:
    raise ValueError('AREA resize implemented for integer factors only')
  if fy == 1 and fx == 1:
    return img
  return img.reshape(b, ht, fy, wt, fx, c).mean(dim=(2, 4))


def _py2_round(x):
  return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def view_synthesis_loss(recons_splat, to_recons_img, splat_bdry_ignore=0.05):
  """L1 view-synthesis loss of the reference's training script
  (ldi_enc_dec.py:337-357): AREA-downsample the target to the splat's size,
  mean |diff| over channels, min over layers, crop the border, mean."""
  _, _, ht, wt, _ = recons_splat.shape
  from lsi.loss import _hip  # pylint: disable=g-import-not-at-top
  return _hip.view_synthesis_loss(recons_splat, to_recons_img,
                                  _py2_round(wt * splat_bdry_ignore),
                                  _py2_round(ht * splat_bdry_ignore))


def ssim_view_synthesis_loss(recons_splat, to_recons_img, splat_bdry_ignore=0.05,
                             win=7, sigma=1.5):
  """Structural view-synthesis loss (the reference has none):
  the target AREA-downsampled and the border cropped as in
  `view_synthesis_loss`, SSIM over the win x win windows that lie inside the
  crop (Gaussian weights, sigma <= 0: box; C1 = 1e-4, C2 = 9e-4), DSSIM =
  (1 - mean_c SSIM) / 2, min over layers, mean.  One fused HIP launch each way
  (lsi_ssim_loss_fwd / _bwd); the gradient is w.r.t. recons_splat only."""
  _, _, ht, wt, _ = recons_splat.shape
  from lsi.loss import _hip  # pylint: disable=g-import-not-at-top
  return _hip.ssim_view_synthesis_loss(recons_splat, to_recons_img,
                                       _py2_round(wt * splat_bdry_ignore),
                                       _py2_round(ht * splat_bdry_ignore), win,
                                       sigma)


def edge_aware_smoothness_loss(pred_disp, guide_imgs, alpha=1.0, order=1,
                               normalise=True):
  """Edge-aware disparity smoothness (the reference has none):
  mean |d_x d| exp(-alpha mean_c |d_x G|) + the same along y, with first
  (order 1) or second (order 2) differences of the disparities pred_disp
  L x B x H x W x 1 and matching differences of the guide images, B x H x W x 3
  for all layers or L x B x H x W x 3 per layer.  normalise: every plane's
  disparities are divided by their mean (+ 1e-7), which makes the term
  independent of the disparity scale.  One fused HIP launch each way
  (lsi_edge_smooth_loss_fwd / _bwd); the gradient is w.r.t. pred_disp only."""
  from lsi.loss import _hip  # pylint: disable=g-import-not-at-top
  return _hip.edge_smoothness_loss(pred_disp, guide_imgs, alpha, order, normalise)


def _planes(t, name, what='depth_supervision_loss'):
  """[..., H, W, 1] or [..., H, W] as a P x H x W view (never a copy).  A last
  dimension of 1 is the channel from four dimensions on; three are P x H x W."""
  if t.dim() >= 4 and t.shape[-1] == 1:
    t = t[..., 0]
  if t.dim() < 2:
    raise RuntimeError('%s: %s is [..., H, W, 1] or [..., H, W] '
                       '(got %s)' % (what, name, tuple(t.shape)))
  h, w = t.shape[-2:]
  try:
    return t.view(-1, h, w)
  except RuntimeError:
    raise RuntimeError('%s: the leading dimensions of %s (%s, '
                       'strides %s) do not flatten without a copy' %
                       (what, name, tuple(t.shape), t.stride())) from None


def depth_supervision_loss(pred_disp, gt, gt_scale=None, mode='silog', lam=0.5,
                           valid_above=0., depth_min=1e-3, depth_max=80., eps=1e-6):
  """Depth supervision against sparse ground truth (the
  reference has none): predicted inverse depths pred_disp and a ground-truth
  map gt, both [..., H, W, 1] or [..., H, W] with equal leading dimensions
  (flattened to P planes as views; a last dimension of 1 is the channel from four
  dimensions on); g = gt * gt_scale[p] (P floats, or gt itself)
  is the ground truth as inverse depth, the convention of
  eval_metrics.depth_accuracy_metrics.  A pixel is scored -- by the ground truth
  alone -- when gt > valid_above and 1 / depth_max <= g <= 1 / depth_min (both in
  fp32); a NaN is a hole.  q = max(pred, eps), a NaN prediction is eps.
  mode 'silog' (Eigen et al. 2014): d = log q - log g, per plane mean(d^2) -
  lam mean(d)^2 over its scored pixels; 'l1': per plane mean |q - g|; the loss is
  the mean over the planes that hold a scored pixel, 0 if none does.  One fused
  HIP launch each way plus a one-block finish (lsi_depth_sup_loss_fwd / _bwd);
  the gradient is w.r.t. pred_disp only, 0 at pixels that are not scored or are
  clamped at eps."""
  import numpy as np  # pylint: disable=g-import-not-at-top
  from lsi.loss import _hip  # pylint: disable=g-import-not-at-top
  pred, gt = _planes(pred_disp, 'pred_disp'), _planes(gt, 'gt')
  if not (depth_min > 0 and depth_max >= depth_min):
    raise ValueError('depth_supervision_loss: 0 < depth_min <= depth_max (got %r, '
                     '%r)' % (depth_min, depth_max))
  one = np.float32(1.0)
  g_min, g_max = float(one / np.float32(depth_max)), float(one / np.float32(depth_min))
  return _hip.depth_supervision_loss(pred, gt, gt_scale, mode, lam, valid_above,
                                     g_min, g_max, eps)


def geometric_consistency_loss(disps, mats, partner_disps=None, mode='ratio',
                               occl_thresh=0., return_map=False):
  """Geometric consistency between two views' inverse depths (the
  reference has none; Godard et al. 2017, Bian et al. 2019): the differentiable
  counterpart of projection.disocclusion_mask.  disps is [..., H, W, 1] or
  [..., H, W] (flattened to P planes as a view), mats P x 4 x 4 on the device:
  mats[p] takes a pixel (x + .5, y + .5, 1, d) of plane p to its partner's frame.
  partner_disps None is the paired form: P is even and the partner of plane p is
  plane p +- P / 2 of disps itself (the trainer's buffer of 2 B views with
  mats = [src -> trg; trg -> src]); else partner_disps has disps' shape and
  plane p's partner is its plane p.  Each pixel's d is projected to (u, v, dd) in
  fp32 as the renderer does and the partner is sampled bilinearly at (u, v): s.
  The pixel is scored when everything is finite, the point lies in front of the
  partner's camera (n > 0, dd > 0) and inside the hull of its pixel centres,
  s > 0 and -- with occl_thresh > 0 -- it is not occluded: s - dd > occl_thresh
  (s + dd).  mode 'ratio': e = |dd - s| / (dd + s), scale-free in [0, 1); 'l1':
  e = |dd - s|.  Per plane the mean of e over its scored pixels; the loss is the
  mean over the planes that hold one, 0 if none does.  One fused HIP launch each
  way plus a one-block finish (lsi_geo_cons_loss_fwd / _bwd); the gradient is
  w.r.t. disps and partner_disps, the scored set and mats are constants.
  return_map: also the detached per-pixel e, P x H x W, -1 where unscored."""
  from lsi.loss import _hip  # pylint: disable=g-import-not-at-top
  what = 'geometric_consistency_loss'
  d = _planes(disps, 'disps', what)
  e = None if partner_disps is None else _planes(partner_disps, 'partner_disps', what)
  return _hip.geometric_consistency_loss(d, e, mats, mode, occl_thresh,
                                         return_map=return_map)


def _image_planes(t, name, what):
  """[..., H, W, C] as a P x H x W x C view (never a copy)."""
  if t.dim() < 3:
    raise RuntimeError('%s: %s is [..., H, W, C] (got %s)' % (what, name, tuple(t.shape)))
  h, w, c = t.shape[-3:]
  try:
    return t.view(-1, h, w, c)
  except RuntimeError:
    raise RuntimeError('%s: the leading dimensions of %s (%s, '
                       'strides %s) do not flatten without a copy' %
                       (what, name, tuple(t.shape), t.stride())) from None


def _layers_of_views(t, q, tail, name, what):
  """[..., *tail dimensions] as an L x Q x tail view (never a copy): the leading
  dimensions flatten to L Q planes, plane p = l Q + q.  The planes need not lie
  at one stride -- the layers of the network's buffer do not -- as long as the
  split into layers and views is a view."""
  if t.dim() < tail:
    raise RuntimeError('%s: %s is [..., %s] (got %s)' %
                       (what, name, 'H, W, C' if tail == 3 else 'H, W', tuple(t.shape)))
  lead = 1
  for n in t.shape[:t.dim() - tail]:
    lead *= n
  if q < 1 or lead % q:
    raise ValueError('%s: the number of sampled images divides the number of planes '
                     '(got %d planes of %s over %d images)' % (what, lead, name, q))
  try:
    return t.view((lead // q, q) + tuple(t.shape[t.dim() - tail:]))
  except RuntimeError:
    raise RuntimeError('%s: the leading dimensions of %s (%s, '
                       'strides %s) do not flatten without a copy' %
                       (what, name, tuple(t.shape), t.stride())) from None


def photometric_reprojection_loss(layer_imgs, layer_disps, other_imgs, mats,
                                  partner_disps=None, shift=0, mode='l1',
                                  occl_thresh=0., eps=1e-3, return_map=False):
  """Backward-warp photometric loss over the layers of an LDI (the
  reference has none; Garg et al. 2016, Godard et al. 2017, Zhou et al. 2017).
  layer_imgs is [..., H, W, C] with 1 <= C <= 4, layer_disps [..., H, W, 1] or
  [..., H, W] with the same leading dimensions (flattened to P planes as views);
  other_imgs [..., H, W, C] are the Q images that are sampled, mats Q x 4 x 4 on
  the device, partner_disps [..., H, W, 1] or [..., H, W] (Q planes) or None the
  inverse depths of the sampled views' visible surface (for both, a last
  dimension of 1 is the channel from four dimensions on, as in `_planes`: a
  map of width 1 needs its channel dimension).  Q divides P: plane p is
  a layer of view q = p mod Q, mats[q] takes its pixels (x + .5, y + .5, 1, d)
  to the frame of image r = (q + shift) mod Q -- L x B layers over B images with
  shift 0, the trainer's buffer of 2 B views against its own input images with
  shift B.  Each pixel's d is projected to (u, v, dd) in fp32 as the renderer
  does, image r is sampled bilinearly at (u, v), and the sample is compared with
  the pixel's own texture: mode 'l1' the mean over the channels of |tex - s|,
  'charb' of sqrt((tex - s)^2 + eps^2).  The pixel is scored when everything is
  finite, the point lies in front of that camera (n > 0, dd > 0) and inside the
  hull of its pixel centres and -- with occl_thresh > 0, which needs
  partner_disps -- it is visible there: the sample sd of partner r is > 0 and
  not sd - dd > occl_thresh (sd + dd).  Per plane the mean over its scored
  pixels; the loss is the mean over the planes that hold one, 0 if none does.
  One fused HIP launch each way plus a one-block finish
  (lsi_photo_reproj_loss_fwd / _bwd), no atomics: both directions give the same
  bits on the same inputs.  The gradient is w.r.t. layer_imgs and layer_disps;
  the scored set, the sampled images, mats and partner_disps are constants.
  return_map: also the detached per-pixel term, P x H x W, -1 where unscored."""
  from lsi.loss import _hip  # pylint: disable=g-import-not-at-top
  what = 'photometric_reprojection_loss'
  img = _image_planes(other_imgs, 'other_imgs', what)
  e = None if partner_disps is None else _planes(partner_disps, 'partner_disps', what)
  tex = _layers_of_views(layer_imgs, img.shape[0], 3, 'layer_imgs', what)
  if layer_disps.dim() >= 4 and layer_disps.shape[-1] == 1:
    layer_disps = layer_disps[..., 0]
  disp = _layers_of_views(layer_disps, img.shape[0], 2, 'layer_disps', what)
  return _hip.photometric_reprojection_loss(tex, disp, img, mats, e, shift, mode,
                                            occl_thresh, eps, return_map=return_map)
