"""View-synthesis evaluation metrics (the arithmetic of the reference's
`ldi_pred_eval.py:297-548` `define_metrics`, without the TF session / HTML
plumbing): masked L1 view-synthesis error, its dis-occlusion-restricted
variant, rendered-disparity error, and PSNR.  Metrics are returned as
(sum, normaliser) pairs; datasets are aggregated as sum(metric)/sum(norm) like
`test_utils.py:247-255`.
"""
import torch

from lsi import _C
from lsi.geometry import ldi as ldi_utils
from lsi.loss import loss as loss_utils


def _centre_mask(b, h, w, frac, device):
  x_min = loss_utils._py2_round(w * frac)
  y_min = loss_utils._py2_round(h * frac)
  m = torch.zeros((b, h, w), device=device)
  m[:, y_min:h - y_min, x_min:w - x_min] = 1.0
  return m


def render_view(ldi_src, pixel_coords, k_s, k_t, rot, t, opts):
  """The rendering the metrics score (compose_layers=True, compute_trg_disp=True:
  ldi_pred_eval.py:340-353): (recons nl x B x Ht x Wt x 3, recons_disp nl x B x
  Ht x Wt x 1)."""
  recons, _, recons_disp = ldi_utils.forward_splat(
      ldi_src, pixel_coords, k_s, k_t, rot, t, compose_layers=True,
      compute_trg_disp=True, trg_downsampling=opts.trg_splat_downsampling,
      zbuf_scale=opts.zbuf_scale, bg_layer_disp=opts.bg_layer_disp,
      max_disp=opts.max_disp)
  return recons, recons_disp


def view_synthesis_metrics(ldi_src, pixel_coords, k_s, k_t, rot, t, imgs_trg,
                           opts, valid_mask=None, disocc_mask=None,
                           gt_disp_trg=None, ssim=None, rendered=None):
  """Renders `ldi_src` into the target camera (compose_layers=True,
  compute_trg_disp=True: ldi_pred_eval.py:340-353) and accumulates the masked
  errors against `imgs_trg` (B x H x W x 3).

  opts needs: trg_splat_downsampling, zbuf_scale, bg_layer_disp, max_disp,
  splat_bdry_ignore.  valid_mask / disocc_mask / gt_disp_trg: B x H x W x 1 or
  None.  Returns a dict name -> (sum, norm) of 0-d tensors.  With ssim = (win,
  sigma) the dict also holds `ssim`, from the kernel `MetricAccumulator.add_ssim`
  runs (there is no op form of it).  `rendered`: the caller's `render_view` of
  the same arguments, scored instead of rendering here.
  """
  recons, recons_disp = rendered or render_view(ldi_src, pixel_coords, k_s, k_t, rot,
                                                t, opts)
  _, b, ht, wt, _ = recons.shape
  dev = recons.device
  target = loss_utils.area_downsample(imgs_trg, ht, wt)
  if valid_mask is None:
    valid = torch.ones((b, ht, wt), device=dev)
  else:  # "ignore pixels that might have aliasing": > 0.95 after AREA resize
    valid = (loss_utils.area_downsample(valid_mask, ht, wt)[..., 0] >
             0.95).float()
  centre = _centre_mask(b, ht, wt, opts.splat_bdry_ignore, dev) * valid
  pw = torch.min(torch.mean(torch.abs(target.unsqueeze(0) - recons), dim=4),
                 dim=0)[0] * centre
  out = {'compose_splat_loss': (pw.sum(), centre.sum())}
  mse = (((target - recons[0])**2).mean(dim=3) * centre).sum() / centre.sum()
  out['psnr'] = (10.0 * torch.log10(1.0 / mse.clamp_min(1e-20)), torch.ones(()))
  if disocc_mask is not None:
    # the reference uses the un-thresholded down-sampled mask here
    # (ldi_pred_eval.py:403-409)
    dm = loss_utils.area_downsample(disocc_mask.float(), ht, wt)[..., 0]
    out['compose_splat_loss_disocc'] = ((pw * dm).sum(), (centre * dm).sum())
  if gt_disp_trg is not None:
    gt = loss_utils.area_downsample(gt_disp_trg, ht, wt)
    pd = torch.min(torch.mean(torch.abs(gt.unsqueeze(0) - recons_disp), dim=4),
                   dim=0)[0] * centre
    out['depth_splat_loss'] = (pd.sum(), centre.sum())
    if disocc_mask is not None:
      out['depth_splat_loss_disocc'] = ((pd * dm).sum(), (centre * dm).sum())
  if ssim is not None:
    out['ssim'] = ssim_metric(recons, imgs_trg, opts.splat_bdry_ignore, *ssim)
  return out


def ssim_metric(recons, imgs_trg, splat_bdry_ignore, win=11, sigma=1.5):
  """(sum over the windows of layer 0's SSIM, number of windows) of a rendering
  nl x B x Ht x Wt x 3 against imgs_trg B x H x W x 3 as 0-d device tensors
  (lsi_eval_ssim)."""
  from lsi.nnutils import _hip_eval  # pylint: disable=g-import-not-at-top
  ht, wt = recons.shape[2:4]
  acc2 = torch.zeros((2,), dtype=torch.float64, device=recons.device)
  _hip_eval.ssim_metric(acc2, recons, imgs_trg,
                        loss_utils._py2_round(wt * splat_bdry_ignore),
                        loss_utils._py2_round(ht * splat_bdry_ignore), win, sigma)
  return acc2[0], acc2[1]


def aggregate(metric_dicts):
  """sum(metric) / sum(norm) over iterations (test_utils.py:247-255)."""
  totals = {}
  for d in metric_dicts:
    for k, (s, n) in d.items():
      a, c = totals.get(k, (0.0, 0.0))
      totals[k] = (a + float(s), c + float(n))
  return {k: a / c for k, (a, c) in totals.items() if c > 0}


def layer_prediction_metrics(ldi_src, ldi_trg, imgs_src, imgs_trg, gt, opts):
  """Per-layer texture / disparity errors of the predicted LDIs against ground
  truth (reference ldi_pred_eval.py:455-521; synthetic data only).

  ldi_*: [tex L x B x H x W x 3, masks, disps L x B x H x W x 1].
  gt: dict with src_gt_disp, trg_gt_disp (foreground, B x H x W x 1) and,
      for the background metrics, src/trg_gt_disp_bg and src/trg_gt_tex_bg.
  Foreground (layer 0): valid where the gt disparity exceeds bg_layer_disp;
  background (last layer): valid where the foreground hides the background
  (gt_disp > gt_disp_bg).  Texture errors are summed over the pixels and divided
  by 3 (the channels).  Returns name -> (sum, norm)."""
  n_layers = ldi_src[0].shape[0]
  out = {}
  v_s = (gt['src_gt_disp'] > opts.bg_layer_disp).float()
  v_t = (gt['trg_gt_disp'] > opts.bg_layer_disp).float()
  fg_tex = ((torch.abs(ldi_src[0][0] - imgs_src) * v_s).sum() / 3 +
            (torch.abs(ldi_trg[0][0] - imgs_trg) * v_t).sum() / 3)
  fg_disp = ((torch.abs(ldi_src[2][0] - gt['src_gt_disp']) * v_s).sum() +
             (torch.abs(ldi_trg[2][0] - gt['trg_gt_disp']) * v_t).sum())
  n_fg = (v_s + v_t).sum()
  out['fg_tex_error'] = (fg_tex, n_fg)
  out['fg_disp_error'] = (fg_disp, n_fg)
  if 'src_gt_disp_bg' in gt:
    b_s = (gt['src_gt_disp'] > gt['src_gt_disp_bg']).float()
    b_t = (gt['trg_gt_disp'] > gt['trg_gt_disp_bg']).float()
    bg_tex = ((torch.abs(ldi_src[0][n_layers - 1] - gt['src_gt_tex_bg']) *
               b_s).sum() / 3 +
              (torch.abs(ldi_trg[0][n_layers - 1] - gt['trg_gt_tex_bg']) *
               b_t).sum() / 3)
    bg_disp = ((torch.abs(ldi_src[2][n_layers - 1] - gt['src_gt_disp_bg']) *
                b_s).sum() +
               (torch.abs(ldi_trg[2][n_layers - 1] - gt['trg_gt_disp_bg']) *
                b_t).sum())
    n_bg = (b_s + b_t).sum()
    out['bg_tex_error'] = (bg_tex, n_bg)
    out['bg_disp_error'] = (bg_disp, n_bg)
  return out


DEPTH_KEYS = ('depth_abs_rel', 'depth_sq_rel', 'depth_rmse', 'depth_rmse_log',
              'depth_a1', 'depth_a2', 'depth_a3')
_FLT_MIN = 1.1754943508222875e-38


def garg_crop(h, w):
  """The evaluation crop of Garg et al. 2016 on an h x w image as (y0, y1, x0,
  x1), truncated as the protocol's `astype(int32)` does."""
  return (int(0.40810811 * h), int(0.99189189 * h),
          int(0.03594771 * w), int(0.96405229 * w))


def _middle_mean(values):
  """The median of a 1-d fp32 tensor as an fp64 0-d tensor: the mean of the two
  middle order statistics (torch.median returns the lower one)."""
  v = torch.sort(values)[0].double()
  n = v.numel()
  return (v[(n - 1) // 2] + v[n // 2]) / 2


def depth_accuracy_metrics(pred, gt, gt_scale=None, mask=None, crop=None,
                           valid_above=0., depth_min=1e-3, depth_max=80.,
                           median=False):
  """Depth accuracy of pred (B x H x W (x 1) inverse depth) against gt (the same
  shape; gt_scale[b] turns it into inverse depth, default 1) in torch ops, on any
  device: the definition of DESIGN.md 4.16, the arithmetic of
  `MetricAccumulator.add_depth_accuracy`.  A pixel is scored where gt >
  valid_above, inside crop = (y0, y1, x0, x1), where mask (B x H x W (x 1)) is
  non-zero and depth_min <= 1 / (gt gt_scale) <= depth_max; with `median` the
  predicted depths of an image are scaled by med(gt depth) / med(predicted
  depth) over its scored pixels first.  Returns name -> (sum over the scored
  images of the per-image figure, number of scored images) as 0-d float64
  tensors for abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 (`depth_` in front) and,
  with `median`, depth_scale."""
  b, h, w = pred.shape[:3]
  pred = pred.float().reshape(b, h, w)
  gt = gt.float().reshape(b, h, w)
  dev = pred.device
  scale = (torch.ones((b,), device=dev) if gt_scale is None else
           gt_scale.to(dev, torch.float32))
  dg = 1.0 / (gt * scale.view(b, 1, 1))
  valid = (gt > valid_above) & (dg >= depth_min) & (dg <= depth_max)
  if crop is not None:
    inside = torch.zeros((h, w), dtype=torch.bool, device=dev)
    inside[crop[0]:crop[1], crop[2]:crop[3]] = True
    valid = valid & inside
  if mask is not None:
    valid = valid & (mask.reshape(b, h, w) != 0)
  # (pred > FLT_MIN is false for a NaN: fmaxf(pred, FLT_MIN))
  floor = torch.full_like(pred, _FLT_MIN)
  dp_raw = 1.0 / torch.where(pred > _FLT_MIN, pred, floor)
  names = DEPTH_KEYS + (('depth_scale',) if median else ())
  sums = torch.zeros((len(names),), dtype=torch.float64, device=dev)
  n_img = 0
  for i in range(b):
    g, p = dg[i][valid[i]], dp_raw[i][valid[i]]
    n = g.numel()
    if n == 0:
      continue
    s = (_middle_mean(g) / _middle_mean(p)).float() if median else torch.ones((), device=dev)
    dp = (s * p).clamp(depth_min, depth_max)
    e = g - dp
    r = torch.maximum(g / dp, dp / g)
    row = [(e.abs() / g).double().sum() / n, (e * e / g).double().sum() / n,
           ((e * e).double().sum() / n).sqrt(),
           (((g.log() - dp.log())**2).double().sum() / n).sqrt()]
    row += [(r < t).double().sum() / n for t in (1.25, 1.5625, 1.953125)]
    if median:
      row.append(s.double())
    sums = sums + torch.stack(row)
    n_img += 1
  count = torch.tensor(float(n_img), dtype=torch.float64, device=dev)
  return {k: (sums[j], count) for j, k in enumerate(names)}


class MetricAccumulator(object):
  """The same metrics accumulated on the device by the fused kernels of
  csrc/lsi_eval.hip: every add_* call is one metric launch plus a one-block
  finishing kernel that adds to 16 running doubles, with no host
  synchronisation and no device-to-host copy; `sums()` reads them back in one
  copy.  `results()` is what `aggregate` gives over the op route's dicts, with
  one difference: a view without any scored cell (an empty centre) adds nothing
  to `psnr`, where the op route adds NaN.  The same sequence of calls gives the
  same 16 doubles bit for bit."""

  def __init__(self, device):
    from lsi.nnutils import _hip_eval  # pylint: disable=g-import-not-at-top
    self._hip = _hip_eval
    self.device = torch.device(device)
    self.acc = torch.zeros((_hip_eval.SLOT_COUNT,), dtype=torch.float64,
                           device=self.device)
    self._ws = None
    self.acc_ssim = None  # two doubles of their own, made by the first add_ssim
    # nine doubles of their own and a workspace, made by the first add_depth_accuracy
    self.acc_depth = None
    self._depth_ws = (None, 0)
    self._depth_median = False
    self._ones = None

  def _workspace(self):
    if self._ws is None:
      self._ws = self._hip.workspace(self.acc.device)
    return self._ws

  def reset(self):
    self.acc.zero_()
    if self.acc_ssim is not None:
      self.acc_ssim.zero_()
    if self.acc_depth is not None:
      self.acc_depth.zero_()

  def add_ssim(self, recons, imgs_trg, splat_bdry_ignore, win=11, sigma=1.5):
    """Adds the SSIM of layer 0 of a rendering (recons nl x B x Ht x Wt x 3)
    against imgs_trg B x H x W x 3 -- the sum over the win x win windows inside
    the border crop and their number -- to an accumulator of two doubles beside
    the 16 (lsi_eval_ssim).  `sums()` and `results()` carry the key `ssim` once
    this has been called."""
    _C.require_device(recons, imgs_trg)
    if self.acc_ssim is None:
      self.acc_ssim = torch.zeros((2,), dtype=torch.float64, device=self.device)
    ht, wt = recons.shape[2:4]
    self._hip.ssim_metric(self.acc_ssim, recons, imgs_trg,
                          loss_utils._py2_round(wt * splat_bdry_ignore),
                          loss_utils._py2_round(ht * splat_bdry_ignore), win, sigma)

  def add_depth_accuracy(self, pred, gt, gt_scale=None, mask=None, crop=None,
                         valid_above=0., depth_min=1e-3, depth_max=80.,
                         median=False, per_image=None):
    """`depth_accuracy_metrics` of the same arguments in the fused kernels of
    csrc/lsi_depth_metrics.hip: the per-image figures are added to nine doubles
    beside the 16 (lsi_eval_depth_metrics; 2 launches, 10 with `median`, no
    host synchronisation).  `sums()` and `results()` carry the `depth_*` keys
    once this has been called (`depth_scale` once it has been called with
    `median`).  per_image: B x 10 float64 on the device, overwritten with each
    image's seven figures, its scale, its number of scored pixels and 1."""
    _C.require_device(gt, gt_scale)
    b, h, w = pred.shape[:3]
    if self.acc_depth is None:
      self.acc_depth = torch.zeros((self._hip.DEPTH_SLOT_COUNT,), dtype=torch.float64,
                                   device=self.device)
    need = int(_C.lib().lsi_eval_depth_workspace_bytes(b, h, w, 1 if median else 0))
    if self._depth_ws[1] < need:
      self._depth_ws = self._hip.depth_workspace(self.device, b, h, w, median)
    if gt_scale is None:
      if self._ones is None or self._ones.numel() != b:
        self._ones = torch.ones((b,), dtype=torch.float32, device=self.device)
      gt_scale = self._ones
    self._depth_median = self._depth_median or bool(median)
    self._hip.depth_metrics(
        self.acc_depth, pred, gt, gt_scale, self._depth_ws[0], self._depth_ws[1],
        mask=mask, crop=crop, valid_above=valid_above, depth_min=depth_min,
        depth_max=depth_max, median=median, per_image=per_image)

  def add_rendered(self, recons, recons_disp, imgs_trg, splat_bdry_ignore,
                   valid_mask=None, disocc_mask=None, gt_disp_trg=None,
                   valid_above=None):
    """Scores an existing rendering (recons nl x B x Ht x Wt x 3, recons_disp
    nl x B x Ht x Wt x 1 or None) against imgs_trg B x H x W x 3; the masks as
    `view_synthesis_metrics` takes them, disocc_mask fp32 or bool.  With
    valid_above, valid_mask is a map (the ground-truth disparity, say) and a
    pixel is valid where it exceeds that value: the caller's
    `(map > valid_above).float()` without its two launches."""
    _C.require_device(recons, recons_disp, imgs_trg, valid_mask, gt_disp_trg)
    ht, wt = recons.shape[2:4]
    ws, n = self._workspace()
    self._hip.view_metrics(
        self.acc, ws, n, recons, recons_disp, imgs_trg,
        loss_utils._py2_round(wt * splat_bdry_ignore),
        loss_utils._py2_round(ht * splat_bdry_ignore), valid=valid_mask,
        disocc=disocc_mask, gt_disp=gt_disp_trg, valid_above=valid_above)

  def add_view_synthesis(self, ldi_src, pixel_coords, k_s, k_t, rot, t, imgs_trg,
                         opts, valid_mask=None, disocc_mask=None,
                         gt_disp_trg=None, valid_above=None, ssim=None,
                         rendered=None):
    """`view_synthesis_metrics` with the arithmetic after the render fused: the
    same forward_splat call (or the caller's, `rendered`), then `add_rendered`
    (and, with ssim = (win, sigma), `add_ssim`)."""
    recons, recons_disp = rendered or render_view(ldi_src, pixel_coords, k_s, k_t,
                                                  rot, t, opts)
    self.add_rendered(recons, recons_disp, imgs_trg, opts.splat_bdry_ignore,
                      valid_mask=valid_mask, disocc_mask=disocc_mask,
                      gt_disp_trg=gt_disp_trg, valid_above=valid_above)
    if ssim is not None:
      self.add_ssim(recons, imgs_trg, opts.splat_bdry_ignore, *ssim)

  def add_layer_prediction(self, ldi_src, ldi_trg, imgs_src, imgs_trg, gt, opts):
    """`layer_prediction_metrics` in one pass over both views."""
    _C.require_device(ldi_src[0], ldi_src[2], ldi_trg[0], ldi_trg[2], imgs_src,
                      imgs_trg)
    ws, n = self._workspace()
    self._hip.layer_metrics(self.acc, ws, n, ldi_src, ldi_trg, imgs_src, imgs_trg,
                            gt, opts.bg_layer_disp)

  def sums(self):
    """name -> (sum, norm) as Python floats, from ONE device-to-host copy (one
    more for `ssim` once `add_ssim` has been called, and one for the `depth_*`
    keys once `add_depth_accuracy` has)."""
    v = self.acc.tolist()
    slot = self._hip.SLOTS
    out = {k: (v[slot[s]], v[slot[n]]) for k, (s, n) in self._hip.METRICS.items()}
    if self.acc_ssim is not None:
      out['ssim'] = tuple(self.acc_ssim.tolist())
    if self.acc_depth is not None:
      d = self.acc_depth.tolist()
      slot = self._hip.DEPTH_SLOTS
      for k, s in self._hip.DEPTH_METRICS.items():
        if k != 'depth_scale' or self._depth_median:
          out[k] = (d[slot[s]], d[slot['IMAGES']])
    return out

  def results(self):
    """name -> sum / norm for every metric that was scored (norm > 0)."""
    return {k: s / n for k, (s, n) in self.sums().items() if n > 0}
