"""float32 NumPy restatement of the contact sheet of include/lsi_hip.h
(lsi_visual_pack_u8): grid, zoom, kinds, quantisation, NaN marker and the row
bytes beyond 3 x width that stay untouched.  Every operation is one float32
NumPy operation in the order the header gives, so the device's bytes must
equal these -- the tests use no tolerance."""
import numpy as np

SKIP, RGB, GRAY, LUT, ABSDIFF = 0, 1, 2, 3, 4
F = np.float32


def sheet_size(rows, cols, cell_h, cell_w, gutter):
  return rows * cell_h + (rows + 1) * gutter, cols * cell_w + (cols + 1) * gutter


def quantise(v, lo, hi):
  """(bytes, is-NaN) of an array: t = fl(fl(v - lo) inv), inv = fl(1 / fl(hi -
  lo)), clamped to [0, 1], floor(fl(fl(t 255) + 0.5))."""
  v = np.asarray(v, F)
  lo = F(lo)
  inv = F(1) / (F(hi) - lo)
  nan = np.isnan(v)
  with np.errstate(invalid='ignore'):
    t = (np.where(nan, F(0), v) - lo) * inv
  assert t.dtype == F
  t = np.minimum(np.maximum(t, F(0)), F(1))
  q = np.floor(t * F(255) + F(0.5))
  return q.astype(np.uint8), nan


def absdiff(a, b):
  """H x W x C (C = 1 or 3) -> H x W: |a0 - b0|, or ((|a0 - b0| + |a1 - b1|) +
  |a2 - b2|) fl(1/3) in that order."""
  a, b = np.asarray(a, F), np.asarray(b, F)
  with np.errstate(invalid='ignore'):
    d = np.abs(a - b)
    if d.shape[2] == 1:
      return d[..., 0]
    return ((d[..., 0] + d[..., 1]) + d[..., 2]) * (F(1) / F(3))


def item_pixels(kind, a, lo, hi, lut, nan_colour, ref=None):
  """The H x W x 3 bytes of one item at zoom 1."""
  a = np.asarray(a, F)
  if a.ndim == 2:
    a = a[..., None]
  if kind == RGB:
    q, nan = quantise(a, lo, hi)
    px, nan = q.copy(), nan.any(axis=2)
  else:
    if kind == ABSDIFF:
      ref = np.asarray(ref, F)
      v = absdiff(a, ref[..., None] if ref.ndim == 2 else ref)
    else:
      v = a[..., 0]
    q, nan = quantise(v, lo, hi)
    px = np.repeat(q[..., None], 3, axis=2) if kind == GRAY else np.asarray(lut)[q]
  px[nan] = nan_colour
  return px


class RefSheet(object):
  """The calls of lsi.visualization.SheetBuilder on host arrays."""

  def __init__(self, cols, cell_h, cell_w, gutter=2, bg=(255, 255, 255),
               nan=(255, 0, 255), lut=None):
    self.cols, self.cell_h, self.cell_w, self.gutter = cols, cell_h, cell_w, gutter
    self.bg, self.nan, self.lut = bg, nan, lut
    self.items = []

  def add(self, kind, a=None, lo=0., hi=1., zoom=None, ref=None):
    if kind != SKIP:
      h, w = np.asarray(a).shape[:2]
      fit = min(self.cell_h // h, self.cell_w // w)
      zoom = fit if zoom is None else zoom
      assert 1 <= zoom <= fit
    self.items.append((kind, a, lo, hi, zoom, ref))

  @property
  def rows(self):
    return max(1, -(-len(self.items) // self.cols))

  def size(self):
    return sheet_size(self.rows, self.cols, self.cell_h, self.cell_w, self.gutter)

  def render_into(self, buf):
    """buf: Hs x row_bytes uint8; only [:, :3 Ws] is written."""
    hs, ws = self.size()
    sheet = np.empty((hs, ws, 3), np.uint8)
    sheet[:] = self.bg
    for k, (kind, a, lo, hi, zoom, ref) in enumerate(self.items):
      if kind == SKIP:
        continue
      px = item_pixels(kind, a, lo, hi, self.lut, self.nan, ref)
      px = np.repeat(np.repeat(px, zoom, axis=0), zoom, axis=1)  # (y // zoom, x // zoom)
      y0 = self.gutter + (k // self.cols) * (self.cell_h + self.gutter)
      x0 = self.gutter + (k % self.cols) * (self.cell_w + self.gutter)
      sheet[y0:y0 + px.shape[0], x0:x0 + px.shape[1]] = px
    buf[:, :3 * ws] = sheet.reshape(hs, 3 * ws)
    return buf

  def render(self):
    hs, ws = self.size()
    return self.render_into(np.empty((hs, 3 * ws), np.uint8)).reshape(hs, ws, 3)
