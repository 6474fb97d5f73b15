"""Colour maps and the builder of a contact sheet (lsi_visual_pack_u8)."""
import ctypes

import numpy as np
import torch

from lsi import _C


def colormap(name):
  """A uint8 [256, 3] table.  'gray' is k, k, k.  'ember' is an ordered map for
  disparities and errors built from integer ramps: blue rises over the first
  quarter and falls over the second, red rises from k = 48 to 160, green from
  112 to 240, and blue returns from 192 towards white.  Its luma 77 r + 150 g +
  29 b grows with every step, so it survives a grey-scale print, and its 256
  colours are distinct."""
  k = np.arange(256, dtype=np.int64)
  if name == 'gray':
    rgb = (k, k, k)
  elif name == 'ember':
    ramp = lambda v: np.clip(v, 0, 255)
    rgb = (ramp((k - 48) * 255 // 112), ramp((k - 112) * 255 // 128),
           np.where(k < 64, 2 * k, np.where(k < 128, 2 * (128 - k), ramp((k - 192) * 4))))
  else:
    raise ValueError("unknown colour map %r ('gray', 'ember')" % (name,))
  return np.stack(rgb, axis=1).astype(np.uint8)


def sheet_size(rows, cols, cell_h, cell_w, gutter):
  """(height, width) of a sheet in pixels (lsi_visual_sheet_size)."""
  sheet = _C.LsiVisSheet(rows=rows, cols=cols, cell_h=cell_h, cell_w=cell_w,
                         gutter=gutter)
  h, w = ctypes.c_int64(), ctypes.c_int64()
  _C.check(_C.lib().lsi_visual_sheet_size(ctypes.byref(sheet), ctypes.byref(h),
                                          ctypes.byref(w)), 'lsi_visual_sheet_size')
  return h.value, w.value


class SheetBuilder(object):
  """Collects the cells of one contact sheet and packs them with one launch.

  Tensors are taken as they are -- fp32 on the builder's ROCm device, H x W x C
  (or H x W for one channel) with any non-negative strides, no copy -- and are
  referenced until `clear()`.  Cell k is row k // cols, column k % cols; the sheet
  has as many rows as the cells need.  `zoom=None` picks the largest integer
  magnification that fits the cell.  There is no CPU path."""

  def __init__(self, device, cols, cell_h, cell_w, gutter=2, bg=(255, 255, 255),
               nan=(255, 0, 255), cmap='ember'):
    self.device = torch.device(device)
    if self.device.type != 'cuda':
      raise RuntimeError('SheetBuilder needs a ROCm GPU (got device %s); there is '
                         'no CPU fallback' % (self.device,))
    if self.device.index is None:
      self.device = torch.device('cuda', torch.cuda.current_device())
    self.cols, self.cell_h, self.cell_w, self.gutter = cols, cell_h, cell_w, gutter
    self.bg, self.nan = tuple(bg), tuple(nan)
    self.lut = np.ascontiguousarray(colormap(cmap) if isinstance(cmap, str) else cmap,
                                    dtype=np.uint8)
    if self.lut.shape != (256, 3):
      raise ValueError('cmap must be a name or a uint8 [256, 3] table')
    sheet_size(1, cols, cell_h, cell_w, gutter)  # refuses a bad grid here
    self._items_host = (_C.LsiVisItem * _C.LSI_VIS_MAX_ITEMS)()
    self._items_bytes = torch.frombuffer(self._items_host, dtype=torch.uint8)
    self._items_dev = None  # allocated with the table by the first pack
    self._lut_dev = None
    self.clear()

  def clear(self):
    """Forgets the cells (and lets go of their tensors)."""
    self.names, self.ranges, self._keep = [], [], []

  def _add(self, name, kind, t, lo, hi, zoom, ref=None):
    n = len(self.names)
    if n >= _C.LSI_VIS_MAX_ITEMS:
      raise ValueError('a sheet holds at most %d cells' % _C.LSI_VIS_MAX_ITEMS)
    it = self._items_host[n]
    ctypes.memset(ctypes.byref(it), 0, ctypes.sizeof(it))
    it.kind = kind
    if kind != _C.LSI_VIS_SKIP:
      dev = _C.require_device(t, ref)
      if dev != self.device or t.dtype != torch.float32 or (
          ref is not None and ref.dtype != torch.float32):
        raise RuntimeError('%s: fp32 tensors on %s are needed (got %s on %s)' %
                           (name, self.device, t.dtype, dev))
      views = [v.unsqueeze(-1) if v.dim() == 2 else v for v in (t, ref) if v is not None]
      h, w, c = views[0].shape if views[0].dim() == 3 else (0, 0, 0)
      want_c = {_C.LSI_VIS_RGB: (3,), _C.LSI_VIS_ABSDIFF: (1, 3)}.get(kind, (1,))
      if c not in want_c or any(v.shape != views[0].shape for v in views):
        raise ValueError('%s: H x W x %s tensor(s) of one shape needed, got %s' %
                         (name, ' or '.join(map(str, want_c)),
                          [tuple(v.shape) for v in views]))
      fit = min(self.cell_h // h, self.cell_w // w) if h and w else 0
      zoom = fit if zoom is None else int(zoom)
      if zoom < 1 or zoom > fit:
        raise ValueError('%s: %d x %d at zoom %d does not fit the %d x %d cell' %
                         (name, h, w, zoom, self.cell_h, self.cell_w))
      lo32 = np.float32(lo)
      with np.errstate(divide='ignore', invalid='ignore'):
        inv = np.float32(1.0) / (np.float32(hi) - lo32)
      if not (np.isfinite(lo32) and np.isfinite(inv) and inv > 0):
        raise ValueError('%s: the range [%r, %r] is empty or not finite' % (name, lo, hi))
      it.H, it.W, it.C, it.zoom = h, w, c, zoom
      it.lo, it.inv = float(lo32), float(inv)
      it.src = views[0].data_ptr()
      it.s_y, it.s_x, it.s_c = views[0].stride()
      if ref is not None:
        it.ref = views[1].data_ptr()
        it.r_y, it.r_x, it.r_c = views[1].stride()
    self.names.append(name)
    self.ranges.append(None if kind == _C.LSI_VIS_SKIP else (float(lo), float(hi)))
    self._keep.append((t, ref))

  def add_rgb(self, name, t, lo=0., hi=1., zoom=None):
    self._add(name, _C.LSI_VIS_RGB, t, lo, hi, zoom)

  def add_gray(self, name, t, lo, hi, zoom=None):
    self._add(name, _C.LSI_VIS_GRAY, t, lo, hi, zoom)

  def add_map(self, name, t, lo, hi, zoom=None):
    """One channel through the colour map."""
    self._add(name, _C.LSI_VIS_LUT, t, lo, hi, zoom)

  def add_absdiff(self, name, a, b, hi, zoom=None):
    """|a - b| (the mean over three channels) on [0, hi] through the colour map."""
    self._add(name, _C.LSI_VIS_ABSDIFF, a, 0., hi, zoom, ref=b)

  def skip(self):
    """Leaves the next cell empty."""
    self._add('', _C.LSI_VIS_SKIP, None, 0., 1., None)

  @property
  def rows(self):
    return max(1, -(-len(self.names) // self.cols))

  def size(self):
    """(height, width) of the sheet the present cells give."""
    return sheet_size(self.rows, self.cols, self.cell_h, self.cell_w, self.gutter)

  def meta(self):
    """The layout for the legend (VisualWriter.submit)."""
    return {'rows': self.rows, 'cols': self.cols, 'cell': [self.cell_h, self.cell_w],
            'gutter': self.gutter, 'ranges': list(self.ranges)}

  def pack(self, out=None):
    """Uploads the descriptors, launches once and returns the uint8 sheet
    Hs x Ws x 3 on the device.  `out`: a sheet to fill instead of a new one --
    uint8, that shape, pixels dense, rows a multiple of 4 bytes apart, 4-byte
    aligned (an earlier result of `pack` is); with it a repeated pack allocates
    nothing.  A new sheet whose rows are not a multiple of 4 bytes is a view of
    a buffer with padded rows; the padding is never written."""
    hs, ws = self.size()
    if out is None:
      pitch = (3 * ws + 3) // 4 * 4
      buf = torch.empty((hs, pitch), dtype=torch.uint8, device=self.device)
      out = buf[:, :3 * ws].unflatten(1, (ws, 3))
    elif (out.dtype != torch.uint8 or out.device != self.device or
          tuple(out.shape) != (hs, ws, 3) or out.stride()[1:] != (3, 1)):
      raise ValueError('out must be a uint8 %d x %d x 3 sheet on %s with dense pixels' %
                       (hs, ws, self.device))
    if self._items_dev is None:
      self._items_dev = torch.empty_like(self._items_bytes, device=self.device)
      self._lut_dev = torch.from_numpy(self.lut).to(self.device)
    n = len(self.names)
    nbytes = n * ctypes.sizeof(_C.LsiVisItem)
    # (pageable source: the copy has left the host array when copy_ returns)
    self._items_dev[:nbytes].copy_(self._items_bytes[:nbytes])
    sheet = _C.LsiVisSheet(rows=self.rows, cols=self.cols, cell_h=self.cell_h,
                           cell_w=self.cell_w, gutter=self.gutter, n_items=n)
    sheet.bg[:], sheet.nan[:] = self.bg, self.nan
    rc = _C.lib().lsi_visual_pack_u8(
        ctypes.byref(sheet), ctypes.addressof(self._items_host),
        self._items_dev.data_ptr(), self._lut_dev.data_ptr(), out.data_ptr(),
        out.stride(0), _C.stream_ptr(self.device))
    _C.check(rc, 'lsi_visual_pack_u8')
    return out
