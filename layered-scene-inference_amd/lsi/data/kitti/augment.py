"""Augmentation of KITTI stereo pairs: random crop (zoom), horizontal flip and
per-channel colour, images and cameras together.  NumPy only.

One `PairAugment` is drawn per stereo pair and shared by its two views.  The
images go through `augment_area_resize`, the restatement of the HIP kernel
lsi_augment_resize_u8 (csrc/lsi_image.hip) and the host route of the loaders:
the two return the same bits.  The cameras go through `augment_cameras`.
Ground truth (--kitti_gt_everywhere): 16-bit disparity maps
go through `sample_disparity_px`, the restatement of lsi_augment_sample_u16,
and the Velodyne projections through `augment_projection`.

  crop    window(aug, H, W) of each view, from its own shape; the output is the
          exact AREA resize of the window
  flip    output column k holds what column w - 1 - k held
  colour  tone(v) = rint(255 (v / 255) ** gamma) on the source bytes, then the
          resized value times brightness * color[c], clamped at 1
"""
import collections

import numpy as np

AugmentOptions = collections.namedtuple(
    'AugmentOptions',
    ['flip_prob', 'zoom_max', 'color_prob', 'gamma', 'brightness', 'color'])
# the last three: (lo, hi) ranges

PairAugment = collections.namedtuple(
    'PairAugment',
    ['flip', 'zoom_y', 'zoom_x', 'off_y', 'off_x', 'gamma', 'brightness', 'color'])

IDENTITY = PairAugment(False, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, (1.0, 1.0, 1.0))
N_DRAWS = 11

DEFAULTS = AugmentOptions(0.5, 1.15, 0.5, (0.8, 1.2), (0.5, 2.0), (0.8, 1.2))


def _range(v, name):
  lo, hi = (float(x) for x in v)
  if not 0 < lo <= hi or not np.isfinite(hi):
    raise ValueError('--aug_%s needs 0 < lo <= hi, got %r' % (name, (lo, hi)))
  return lo, hi


def options_from(opts):
  """AugmentOptions from the --aug_* values of `opts` (absent: the defaults)."""
  get = lambda name, default: getattr(opts, 'aug_' + name, default)
  o = AugmentOptions(
      float(get('flip_prob', DEFAULTS.flip_prob)), float(get('zoom_max', DEFAULTS.zoom_max)),
      float(get('color_prob', DEFAULTS.color_prob)), _range(get('gamma', DEFAULTS.gamma), 'gamma'),
      _range(get('brightness', DEFAULTS.brightness), 'brightness'),
      _range(get('color', DEFAULTS.color), 'color'))
  if not (0 <= o.flip_prob <= 1 and 0 <= o.color_prob <= 1):
    raise ValueError('--aug_flip_prob and --aug_color_prob are probabilities')
  if not 1 <= o.zoom_max < np.inf:
    raise ValueError('--aug_zoom_max must be >= 1 (1 = no crop), got %r' % o.zoom_max)
  return o


def sample(rng, opts):
  """One PairAugment.  Always N_DRAWS uniform numbers, in this order: flip, zoom
  y, zoom x, offset y, offset x, colour switch, gamma, brightness, three channel
  factors -- an option that is off does not shift the draws of the others."""
  u = rng.random_sample(N_DRAWS)
  lerp = lambda r, x: r[0] + float(x) * (r[1] - r[0])
  colour = bool(u[5] < opts.color_prob)
  return PairAugment(
      flip=bool(u[0] < opts.flip_prob),
      zoom_y=1.0 + float(u[1]) * (opts.zoom_max - 1.0),
      zoom_x=1.0 + float(u[2]) * (opts.zoom_max - 1.0),
      off_y=float(u[3]), off_x=float(u[4]),
      gamma=lerp(opts.gamma, u[6]) if colour else 1.0,
      brightness=lerp(opts.brightness, u[7]) if colour else 1.0,
      color=tuple(lerp(opts.color, x) for x in u[8:11]) if colour else (1.0, 1.0, 1.0))


def window(aug, H, W):
  """(y0, x0, ch, cw) of an H x W image: ch = max(1, round(H / zoom_y)), y0 =
  round(off_y (H - ch)), columns alike.  Inside the image for zoom >= 1, offsets
  in [0, 1]."""
  def axis(n, zoom, off):
    c = min(n, max(1, int(np.rint(n / zoom))))
    return int(np.rint(off * (n - c))), c
  y0, ch = axis(int(H), aug.zoom_y, aug.off_y)
  x0, cw = axis(int(W), aug.zoom_x, aug.off_x)
  return y0, x0, ch, cw


def tone_table(aug):
  """uint8[3][256]: rint(255 (v / 255) ** gamma) in float64, the same for the
  three channels.  gamma = 1 gives the identity."""
  v = np.arange(256, dtype=np.float64)
  t = np.rint(255.0 * (v / 255.0) ** float(aug.gamma)).astype(np.uint8)
  return np.ascontiguousarray(np.broadcast_to(t, (3, 256)))


def gains(aug):
  """float32[3]: brightness * color[c]."""
  return (np.float64(aug.brightness) * np.asarray(aug.color, np.float64)).astype(np.float32)


def image_params(aug, nc):
  """(table or None, gains float32[nc]) of an nc-channel image: one-channel
  images get the identity curve and gain 1; so does gamma = 1 (table None)."""
  if nc != 3:
    return None, np.ones(nc, np.float32)
  return (None if aug.gamma == 1.0 else tone_table(aug)), gains(aug)


def _axis_sums(a, n_out):
  """sum_j o[i, j] a[j] along axis 0 in int64, o[i, j] = min((i+1) n, (j+1)
  n_out) - max(i n, j n_out) where positive: a few shifted gathers, one per
  tap."""
  n = a.shape[0]
  i = np.arange(n_out, dtype=np.int64)
  lo, hi = (i * n) // n_out, -((-(i + 1) * n) // n_out)      # taps [lo, hi)
  out = np.zeros((n_out,) + a.shape[1:], np.int64)
  for t in range(int((hi - lo).max())):
    j = np.minimum(lo + t, n - 1)
    o = np.minimum((i + 1) * n, (j + 1) * n_out) - np.maximum(i * n, j * n_out)
    o = np.where(lo + t < hi, o, 0)
    out += o.reshape((-1,) + (1,) * (a.ndim - 1)) * a[j]
  return out


def augment_area_resize(img_u8, window, flip, table, gains, ho, wo):  # pylint: disable=redefined-outer-name
  """The kernel's arithmetic on one uint8 H x W x C image: int64 sums of the
  integer overlaps over the window of the tone-mapped bytes, np.float32(acc) *
  np.float32(1 / (255 ch cw)), the fp32 gain multiply, the clamp at 1, the
  mirrored store.  table: uint8[C][256] or None; gains: C floats.  Returns
  float32 ho x wo x C."""
  img = np.asarray(img_u8)
  if img.dtype != np.uint8 or img.ndim != 3:
    raise ValueError('an H x W x C uint8 image is needed')
  y0, x0, ch, cw = (int(v) for v in window)
  if not (0 <= y0 and ch >= 1 and y0 + ch <= img.shape[0] and
          0 <= x0 and cw >= 1 and x0 + cw <= img.shape[1]):
    raise ValueError('window %r leaves the %d x %d image' % (window, img.shape[0], img.shape[1]))
  nc = img.shape[2]
  win = img[y0:y0 + ch, x0:x0 + cw]
  if table is not None:
    table = np.asarray(table, np.uint8).reshape(nc, 256)
    win = np.stack([table[c][win[:, :, c]] for c in range(nc)], axis=2)
  acc = _axis_sums(win.astype(np.int64), ho)                          # ho x cw x C
  acc = _axis_sums(acc.transpose(1, 0, 2), wo).transpose(1, 0, 2)     # ho x wo x C
  scale = np.float32(1.0 / (255.0 * float(ch) * float(cw)))
  g = np.asarray(gains, np.float32).reshape(nc)
  if not (np.isfinite(g).all() and (g >= 0).all()):
    raise ValueError('gains must be finite and >= 0, got %r' % (g,))
  out = np.minimum((acc.astype(np.float32) * scale) * g, np.float32(1.0))
  if flip:
    out = out[:, ::-1]
  return np.ascontiguousarray(out, np.float32)


def sample_disparity_px(raw_u16, window, flip, ho, wo):  # pylint: disable=redefined-outer-name
  """The arithmetic of lsi_augment_sample_u16 on one H x W map of 16-bit
  disparities (value = disparity * 256, 0 = no match), and the host route of
  the loaders: output pixel (i, k) takes the pixel of the
  window under its centre, row y0 + min(((2 i + 1) ch) // (2 ho), ch - 1),
  columns alike, as float32((raw / 256.0) * (wo / float(cw))) -- pixels of the
  ho x wo image; float64, rounded once -- and lands at column wo - 1 - k under
  a flip.  Zeros stay zeros and the sign does not change: the flipped pair's
  baseline changes sign in t and the loss uses |t_x|.  The full window without
  flip gives the bits of data.load_disparity_px.  Returns float32 ho x wo x 1."""
  raw = np.asarray(raw_u16)
  if raw.ndim != 2 or raw.dtype.kind not in 'iu':
    raise ValueError('an H x W integer map is needed')
  y0, x0, ch, cw = (int(v) for v in window)
  if not (0 <= y0 and ch >= 1 and y0 + ch <= raw.shape[0] and
          0 <= x0 and cw >= 1 and x0 + cw <= raw.shape[1]):
    raise ValueError('window %r leaves the %d x %d map' % (window, raw.shape[0], raw.shape[1]))
  raw = raw.astype(np.int64)
  ys = y0 + np.minimum(((2 * np.arange(ho, dtype=np.int64) + 1) * ch) // (2 * ho), ch - 1)
  xs = x0 + np.minimum(((2 * np.arange(wo, dtype=np.int64) + 1) * cw) // (2 * wo), cw - 1)
  out = (raw[ys][:, xs] / 256.0 * (wo / float(cw))).astype(np.float32)
  if flip:
    out = out[:, ::-1]
  return np.ascontiguousarray(out[:, :, None], np.float32)


def augment_projection(mat_3x4, shape, win, flip, h, w, dtype=np.float32):
  """velodyne.velo_to_image's 3 x 4 matrix (scanner -> pixel areas of the whole
  image resized to w x h) for the augmented view, row for row what
  augment_cameras does to the intrinsics: with (y0, x0, ch, cw) = win and
  (H, W) = shape,
    row0' = row0 (W / cw) - (x0 w / cw) row2,  row1' alike with H, ch, y0, h;
    flip: row0'' = w row2 - row0'
  in float64, rounded to `dtype` once.  Row 2 -- every depth -- is untouched,
  and so are the scans: view 0 stays camera 2 = source.  The full window
  without flip returns the input bits."""
  y0, x0, ch, cw = (int(v) for v in win)
  m = np.array(mat_3x4, np.float64).reshape(3, 4)
  # (x - 0 * r is x but for the sign of a zero: an offset of 0 subtracts nothing)
  m[0] = m[0] * (shape[1] / float(cw)) - ((x0 * (w / float(cw))) * m[2] if x0 else 0.0)
  m[1] = m[1] * (shape[0] / float(ch)) - ((y0 * (h / float(ch))) * m[2] if y0 else 0.0)
  if flip:
    m[0] = w * m[2] - m[0]
  return m.astype(dtype)


def augment_cameras(k_s, k_t, rot, t, src_shape, trg_shape, win_s, win_t, flip, h, w):
  """The cameras of the augmented pair, float64; k_s, k_t, rot, t are
  data.pair_cameras' (intrinsics of the whole images resized to w x h).

  Crop: K' = diag(w / cw, h / ch, 1) T(-x0, -y0) K_orig per view, which in terms
  of k = diag(w / W, h / H, 1) K_orig is row 0 times W / cw minus x0 w / cw in
  its last entry (rows alike) -- the full window multiplies by 1 and subtracts
  0: pair_cameras' values exactly.  Flip, S = diag(-1, 1, 1): K'[0, 2] = w -
  K[0, 2], K'[0, 1] = -K[0, 1], rot' = S rot S, t' = S t; source stays source."""
  def crop(k, shape, win):
    y0, x0, ch, cw = win
    k = np.array(k, np.float64)
    k[0] *= shape[1] / float(cw)
    k[1] *= shape[0] / float(ch)
    k[0, 2] -= x0 * (w / float(cw))
    k[1, 2] -= y0 * (h / float(ch))
    if flip:
      k[0, 2] = w - k[0, 2]
      k[0, 1] = -k[0, 1]
    return k
  rot = np.array(rot, np.float64)
  t = np.array(t, np.float64)
  if flip:
    s = np.diag([-1.0, 1.0, 1.0])
    rot, t = s @ rot @ s, s @ t
  return crop(k_s, src_shape, win_s), crop(k_t, trg_shape, win_t), rot, t
