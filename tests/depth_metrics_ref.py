"""An fp64 NumPy restatement of the depth accuracy metrics (DESIGN.md 4.16,
include/lsi_hip.h: lsi_eval_depth_metrics) and the fixtures its tests share.

What is fp32 here is what decides a set or an order, and both are exact in the
kernel too: the ground-truth depth dg = 1 / (gt gt_scale) (one correctly rounded
product and quotient), the scored set it defines, dp_raw = 1 / fmaxf(pred,
FLT_MIN), the order statistics of both and the scale (float)(med / med).
Everything after that -- the clamp, the seven terms, the sums -- is fp64."""
import numpy as np

FLT_MIN = np.float32(1.1754943508222875e-38)
THRESHOLDS = (1.25, 1.5625, 1.953125)
COLUMNS = ('abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'a1', 'a2', 'a3', 'scale', 'n',
           'scored')
KEYS = ('depth_abs_rel', 'depth_sq_rel', 'depth_rmse', 'depth_rmse_log', 'depth_a1',
        'depth_a2', 'depth_a3')


def middle_mean(values):
  """The median of fp32 values in fp64: the two middle order statistics averaged."""
  v = np.sort(np.asarray(values, np.float32)).astype(np.float64)
  return (v[(v.size - 1) // 2] + v[v.size // 2]) / 2


def scored_set(gt, gt_scale, mask=None, crop=None, valid_above=0., depth_min=1e-3,
               depth_max=80.):
  """(V, dg): the B x H x W bool set of scored pixels and the fp32 depths."""
  gt = np.asarray(gt, np.float32).reshape(np.shape(gt)[:3])
  b, h, w = gt.shape
  scale = np.asarray(gt_scale, np.float32).reshape(b, 1, 1)
  with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
    dg = np.float32(1) / (gt * scale)
    v = (gt > np.float32(valid_above)) & (dg >= np.float32(depth_min)) & (
        dg <= np.float32(depth_max))
  if crop is not None:
    inside = np.zeros((h, w), bool)
    inside[crop[0]:crop[1], crop[2]:crop[3]] = True
    v &= inside
  if mask is not None:
    v &= np.asarray(mask).reshape(b, h, w) != 0
  return v, dg


def per_image_table(pred, gt, gt_scale, mask=None, crop=None, valid_above=0.,
                    depth_min=1e-3, depth_max=80., median=False, margin=None):
  """The B x 10 table (COLUMNS; zeros for an image without a scored pixel).  With
  `margin` also the number of pixels on which fp32 and fp64 arithmetic may
  decide differently: scored pixels whose ratio r lies within that relative
  distance of a delta threshold, and pixels with gt > valid_above whose depth
  lies within it of depth_min or depth_max."""
  v, dg = scored_set(gt, gt_scale, mask, crop, valid_above, depth_min, depth_max)
  b, h, w = v.shape
  pred = np.asarray(pred, np.float32).reshape(b, h, w)
  with np.errstate(divide='ignore', over='ignore'):
    dp_raw = np.float32(1) / np.fmax(pred, FLT_MIN)   # fmax drops a NaN, as fmaxf
  lo, hi = float(np.float32(depth_min)), float(np.float32(depth_max))
  table = np.zeros((b, len(COLUMNS)), np.float64)
  near = 0
  for i in range(b):
    if margin is not None:
      g = dg[i][np.asarray(gt, np.float32).reshape(b, h, w)[i] > np.float32(valid_above)]
      g = g.astype(np.float64)
      near += int(((np.abs(g / lo - 1) < margin) | (np.abs(g / hi - 1) < margin)).sum())
    n = int(v[i].sum())
    if n == 0:
      continue
    g32, p32 = dg[i][v[i]], dp_raw[i][v[i]]
    s = np.float32(middle_mean(g32) / middle_mean(p32)) if median else np.float32(1)
    g = g32.astype(np.float64)
    dp = np.clip(float(s) * p32.astype(np.float64), lo, hi)
    e = g - dp
    r = np.maximum(g / dp, dp / g)
    table[i, :4] = ((np.abs(e) / g).sum() / n, (e * e / g).sum() / n,
                    np.sqrt((e * e).sum() / n),
                    np.sqrt(((np.log(g) - np.log(dp))**2).sum() / n))
    table[i, 4:7] = [(r < t).sum() / n for t in THRESHOLDS]
    table[i, 7:] = (float(s), n, 1.0)
    if margin is not None:
      near += int(sum((np.abs(r / t - 1) < margin).sum() for t in THRESHOLDS))
  return (table, near) if margin is not None else table


def totals(table):
  """name -> (sum over the scored images, scored images) of a table."""
  out = {k: (table[:, j].sum(), table[:, 9].sum()) for j, k in enumerate(KEYS)}
  out['depth_scale'] = (table[:, 7].sum(), table[:, 9].sum())
  return out


def _same_side(new, old, mids):
  """Whether replacing `old` by `new` leaves the middle order statistics `mids`
  (lower, upper) what they are."""
  return ((old < mids[0]) & (new < mids[0])) | ((old > mids[1]) & (new > mids[1]))


def build_fixture(seed, shape, mask=None, crop=None, valid_above=0., depth_min=1e-3,
                  depth_max=80., median=False, empty=0.3, margin=1e-4, odd_preds=True):
  """pred, gt (B x H x W fp32, gt_scale 1): depths log-uniform over [0.5, 120] (some
  beyond the 80 cap), `empty` of the ground truth 0, predictions gt exp(N(0,
  0.3)) plus, with odd_preds, a few zero, negative, NaN and 1e-9 ones.  Pixels
  within `margin` of a depth cap or a delta threshold are redrawn until there
  are none (a prediction is redrawn on its side of the image's median, which
  therefore stays what it is)."""
  rs = np.random.RandomState(seed)
  b, h, w = shape
  draw_depth = lambda n: np.exp(rs.uniform(np.log(0.5), np.log(120.), n))
  depth = draw_depth(b * h * w).reshape(shape)
  for _ in range(100):
    bad = (np.abs(depth / depth_max - 1) < 4 * margin) | (np.abs(depth / depth_min - 1) < 4 * margin)
    if not bad.any():
      break
    depth[bad] = draw_depth(int(bad.sum()))
  gt = (1.0 / depth).astype(np.float32)
  gt[rs.rand(*shape) < empty] = 0
  pred = (gt * np.exp(0.3 * rs.randn(*shape))).astype(np.float32)
  pred[gt == 0] = rs.rand(int((gt == 0).sum())).astype(np.float32)
  if odd_preds and pred.size >= 16:
    flat = pred.reshape(-1)
    idx = rs.permutation(flat.size)[:8]
    flat[idx] = np.array([0, 0, -1, -0.25, np.nan, np.nan, 1e-9, 1e-9], np.float32)
  kw = dict(mask=mask, crop=crop, valid_above=valid_above, depth_min=depth_min,
            depth_max=depth_max)
  scale = np.ones((b,), np.float32)
  v, dg = scored_set(gt, scale, **kw)
  for _ in range(200):
    with np.errstate(divide='ignore', over='ignore'):
      dp_raw = np.float32(1) / np.fmax(pred, FLT_MIN)
    n_bad = 0
    for i in range(b):
      if not v[i].any():
        continue
      p32 = np.sort(dp_raw[i][v[i]])
      mids = (p32[(p32.size - 1) // 2], p32[p32.size // 2])
      s = np.float32(middle_mean(dg[i][v[i]]) / middle_mean(p32)) if median else np.float32(1)
      dp = np.clip(float(s) * dp_raw[i].astype(np.float64), float(np.float32(depth_min)),
                   float(np.float32(depth_max)))
      g = np.where(v[i], dg[i], 1).astype(np.float64)
      r = np.maximum(g / dp, dp / g)
      bad = v[i] & np.any([np.abs(r / t - 1) < 2 * margin for t in THRESHOLDS], axis=0)
      n_bad += int(bad.sum())
      for y, x in zip(*np.nonzero(bad)):
        for _ in range(1000):
          new = np.float32(gt[i, y, x] * np.exp(0.3 * rs.randn()))
          if not median or _same_side(np.float32(1) / new, dp_raw[i, y, x], mids):
            pred[i, y, x] = new
            break
    if n_bad == 0:
      break
  table, near = per_image_table(pred, gt, scale, median=median, margin=margin, **kw)
  assert near == 0, 'the fixture builder left %d pixels near a threshold' % near
  return pred, gt


def case_inputs(seed, shape, kw):
  """(pred, gt, metric arguments) of a test case: kw is the metric's arguments
  with `mask` 'bool' or 'f32' standing for a random mask of that type (80 %
  set) and `empty` for the builder's share of empty ground truth."""
  kw = dict(kw)
  empty = kw.pop('empty', 0.3)
  if 'mask' in kw:
    m = np.random.RandomState(seed + 1000).rand(*shape) < 0.8
    kw['mask'] = m if kw['mask'] == 'bool' else m.astype(np.float32)
  pred, gt = build_fixture(seed, shape, empty=empty, **kw)
  return pred, gt, kw
