"""The training objective of ldi_enc_dec.py, assembled from the loss kernels: each
term is written once, over groups of views (`Views`), and weighted by one table
(`loss_coefficients`).

The network's output is one buffer of 2 B LDIs (source views, then target views)
whose halves are views of it.  A loss taken on a half sends its gradient back
through a slice: autograd fills a zero tensor of the whole buffer per half and
adds them up (texture, masks, disparities: a dozen kernels over 25 - 100 MB each
per step).  Every term is a mean over the batch, so the term of the pair is twice
the mean over the 2 B LDIs: one group of 2 B views with the factor 2, one call
per term on the whole buffer, no slices.  Without such a buffer: two groups, src
-> trg and trg -> src (reference ldi_enc_dec.py:302-334: one call per direction)."""
import functools
import operator

import torch

from lsi.geometry import ldi as ldi_utils
from lsi.loss import loss

REFERENCE = ('self_cons', 'compose_splat', 'indep_splat', 'incr_depth', 'disp_smoothness')


def loss_coefficients(opts):
  """{term: factor of its scalar in the total}: the terms whose weight --<term>_wt
  is > 0, in the order they are added.  The disparities scale with max_disp: a
  term linear in them is divided by it (the smoothness term is quadratic; the
  normalised edge term and the geometric ratio are scale-free).  'ssim' multiplies
  compose_splat_wt * compose_ssim_loss + indep_splat_wt * indep_ssim_loss."""
  d = opts.max_disp
  divisors = (
      ('self_cons', 1.0), ('compose_splat', 1.0), ('indep_splat', 1.0), ('ssim', 1.0),
      ('incr_depth', d), ('disp_smoothness', d * d),
      ('edge_smooth', 1.0 if getattr(opts, 'edge_smooth_norm', True) else d),
      ('depth_sup', 1.0),
      ('geo_cons', d if getattr(opts, 'geo_cons_mode', 'ratio') == 'l1' else 1.0),
      ('photo_reproj', 1.0))
  weights = ((name, getattr(opts, name + '_wt', 0.0), div) for name, div in divisors)
  return {name: wt / div for name, wt, div in weights if wt > 0}


def _joined(parts):
  return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


class Views(object):
  """A group of views a term is evaluated on, with all a term may read for them.
  Tensors of several parts are concatenated when first read, once per step."""

  def __init__(self, ldi, own, targets, mats, host_mats, gt, partner=None, shift=0,
               factor=1.0):
    self.ldi = ldi                    # [tex, masks, disps] of the views
    self.own, self._targets, self._mats, self._host = own, targets, mats, host_mats
    self.gt, self.gt_scale = gt       # depth ground truth of the views, its scale
    # layer 0 of the partner views: the surface the other view sees.  In one
    # buffer of 2 B views, view q's partner is view q +- B = shift of the same
    # tensor, and the geometric term is given no partner.
    self.visible = (partner or ldi)[2][0]
    self.partner_disps = None if partner is None else self.visible
    self.shift, self.factor = shift, factor

  imgs = functools.cached_property(lambda self: _joined(self.own))       # the inputs
  targets = functools.cached_property(lambda self: _joined(self._targets))
  mats = functools.cached_property(lambda self: _joined(self._mats))     # device
  host_mats = functools.cached_property(lambda self: _joined(self._host))

  @property
  def sampled(self):
    """The partner views' input images: among the views' own, or the targets."""
    return self.imgs if self.shift else self.targets


def view_groups(ldi_src, ldi_trg, pair, imgs, mats, host_mats, gt=(None, None)):
  """(groups, halves): the two directions, and what the terms are taken on --
  the one group of `pair`, the network's buffer of 2 B LDIs, or the halves."""
  (src, trg), (m_trg, m_src), (h_trg, h_src), b = imgs, mats, host_mats, imgs[0].shape[0]
  half = lambda k: [None if t is None else t[k * b:(k + 1) * b] for t in gt]
  halves = [Views(ldi_src, [src], [trg], [m_trg], [h_trg], half(0), partner=ldi_trg),
            Views(ldi_trg, [trg], [src], [m_src], [h_src], half(1), partner=ldi_src)]
  if pair is None:
    return halves, halves
  # Both directions from ONE launch (and one in the backward): a batch of 2 B
  # elements with their own matrices, compared with [imgs_trg; imgs_src].  A rank
  # with 4 samples then issues 8-view launches instead of twice 4.
  return [Views(pair, [src, trg], [trg, src], [m_trg, m_src], [h_trg, h_src], gt,
                shift=b, factor=2.0)], halves


def _total(parts):
  """Sum of factor * value; a factor of 1 costs no launch."""
  return functools.reduce(operator.add, [v if f == 1.0 else f * v for f, v in parts])


def self_consistency(groups, opts):
  """ldi_enc_dec.py:269-294; --l0_self_cons: layer 0 against the input, in torch."""
  def term(g):
    if opts.l0_self_cons:
      return torch.mean(torch.abs(g.imgs - g.ldi[0][0]))
    masks = g.ldi[1] if g.ldi[1] is not None else torch.ones_like(g.ldi[2])
    return loss.zbuffer_composition_loss(
        g.ldi[0], masks, g.ldi[2], g.imgs, zbuf_scale=opts.zbuf_scale,
        bg_layer_disp=opts.bg_layer_disp, max_disp=opts.max_disp)
  return {'self_cons_loss': _total([(g.factor, term(g)) for g in groups])}


def view_synthesis(groups, opts, coef, zero):
  """View synthesis via forward splatting (ldi_enc_dec.py:296-357).  One sweep per
  group renders the per-layer AND the composed view (the reference makes four
  forward_splat calls whose per-layer splats are identical pairwise).  A term
  whose weight is 0 is the scalar zero; no render when both are."""
  kinds = [k for k in ('indep', 'compose') if k + '_splat' in coef]
  parts = {}
  for g in groups if kinds else ():
    img_i, _, img_c, _ = ldi_utils.forward_splat_both(
        g.ldi, g.mats, trg_downsampling=opts.trg_splat_downsampling,
        zbuf_scale=opts.zbuf_scale, bg_layer_disp=opts.bg_layer_disp,
        max_disp=opts.max_disp, mat_host=g.host_mats)
    for kind in kinds:
      img = {'indep': img_i, 'compose': img_c}[kind]
      parts.setdefault(kind + '_splat_loss', []).append(
          (g.factor, loss.view_synthesis_loss(img, g.targets, opts.splat_bdry_ignore)))
      if 'ssim' in coef:
        parts.setdefault(kind + '_ssim_loss', []).append(
            (g.factor, loss.ssim_view_synthesis_loss(
                img, g.targets, opts.splat_bdry_ignore, win=opts.ssim_win,
                sigma=opts.ssim_sigma)))
  return {k + n: _total(parts[k + n]) if k + n in parts else zero
          for n in ('_splat_loss', '_ssim_loss') for k in ('compose', 'indep')}


def disparity_regularisers(groups, opts, zero):
  """ldi_enc_dec.py:388-396: both from one read of each disparity tensor (fused
  HIP kernel lsi_disp_reg_loss_fwd); no ordering term for a single layer."""
  from lsi.loss import _hip as loss_hip  # pylint: disable=g-import-not-at-top
  both = [(g.factor, loss_hip.disp_regularisers(g.ldi[2])) for g in groups]
  return {'incr_depth_loss': (_total([(f, v[1]) for f, v in both])
                              if opts.n_layers > 1 else zero),
          'disp_smoothness_loss': _total([(f, v[0]) for f, v in both])}


def edge_smoothness(groups, opts):
  """DESIGN.md 4.14; no reference counterpart.  Guided by the layer's own
  texture, detached, or by the input images."""
  by_texture = opts.edge_smooth_guide == 'texture'
  return {'edge_smooth_loss': _total([(g.factor, loss.edge_aware_smoothness_loss(
      g.ldi[2], g.ldi[0].detach() if by_texture else g.imgs, alpha=opts.edge_smooth_alpha,
      order=opts.edge_smooth_order, normalise=opts.edge_smooth_norm)) for g in groups])}


def depth_supervision(groups, opts, source):
  """Of layer 0 (no reference counterpart).  The planes' ground
  truth holds the background's disparity where no object is: not scored."""
  return {'depth_sup_loss': _total([(g.factor, loss.depth_supervision_loss(
      g.ldi[2][0], g.gt, g.gt_scale, mode=opts.depth_sup_mode, lam=opts.depth_sup_lambda,
      valid_above=opts.bg_layer_disp if source == 'planes' else 0.,
      depth_min=opts.depth_sup_min, depth_max=opts.depth_sup_max)) for g in groups])}


def geometric_consistency(groups, opts):
  """Of the two views' layer 0 (no reference counterpart)."""
  def term(g):
    kw = {} if g.partner_disps is None else {'partner_disps': g.partner_disps}
    return loss.geometric_consistency_loss(
        g.ldi[2][0], g.mats, mode=opts.geo_cons_mode, occl_thresh=opts.geo_cons_occl, **kw)
  return {'geo_cons_loss': _total([(g.factor, term(g)) for g in groups])}


def photometric_reprojection(groups, opts):
  """Backward warp (no reference counterpart).  texture: all layers
  at their own disparities; image: layer 0's disparities under the view's own input
  image.  A plane samples the partner view's input image."""
  def term(g):
    tex, disps = ((g.ldi[0], g.ldi[2]) if opts.photo_reproj_what == 'texture'
                  else (g.imgs, g.ldi[2][0]))
    return loss.photometric_reprojection_loss(
        tex, disps, g.sampled, g.mats, partner_disps=g.visible.detach(), shift=g.shift,
        mode=opts.photo_reproj_mode, occl_thresh=opts.photo_reproj_occl)
  return {'photo_reproj_loss': _total([(g.factor, term(g)) for g in groups])}


def objective(groups, halves, opts, coef, depth_source=None):
  """(total, scalars) under coef = loss_coefficients(opts): the six reference
  scalars, whatever their weights, then those of the other enabled terms."""
  zero = halves[0].imgs.new_zeros(())
  s = self_consistency(halves if opts.l0_self_cons else groups, opts)
  s.update(view_synthesis(groups, opts, coef, zero))
  s.update(disparity_regularisers(groups, opts, zero))
  for name, term in (('edge_smooth', edge_smoothness),
                     ('depth_sup', functools.partial(depth_supervision, source=depth_source)),
                     ('geo_cons', geometric_consistency),
                     ('photo_reproj', photometric_reprojection)):
    if name in coef:
      s.update(term(groups, opts))
  if 'ssim' in coef:
    # the structural terms ride on the L1 terms' weights
    s['ssim_loss'] = (coef.get('compose_splat', 0.0) * s['compose_ssim_loss'] +
                      coef.get('indep_splat', 0.0) * s['indep_ssim_loss'])
  total = zero
  for name, c in coef.items():
    total = total + c * s[name + '_loss']
  logged = [n + '_loss' for n in REFERENCE] + ['total_loss'] + [
      n + '_loss' for row in coef if row not in REFERENCE
      for n in (('compose_ssim', 'indep_ssim') if row == 'ssim' else (row,))]
  s['total_loss'] = total
  return total, {k: s[k] for k in logged}
