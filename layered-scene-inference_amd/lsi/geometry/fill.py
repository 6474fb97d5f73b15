"""Push-pull (pyramid) hole filling of rendered images on the device
(csrc/lsi_fill.hip).

    filled = fill_holes(img, conf)
    filled = fill_splat_holes(trg_img, trg_wts, bg_layer_disp, max_disp, zbuf_scale,
                              n_layers=L)

img: float32 N x H x W x C, C in 1 .. 4; conf: N x H x W (or N x H x W x 1), the
share of each pixel that is known, clamped to [0, 1].  Confident colour is
summed down a pyramid of 2 x 2 boxes, normalised where a box holds more than
one pixel's worth, and every pixel takes, for the share it lacks, the bilinear
up-sample of the level above; an image without any confident pixel becomes
`bg_value`.  `fill_splat_holes` reads the confidence off forward_splat's weight
sum: the canvas of weight bg_wt and value 1 is taken out of the pixel again, so
hairline cracks between magnified splats and dis-occluded bands get the colour
of what surrounds them.  All fp32 in a fixed order: a function of the inputs
alone, bit for bit.  Forward only -- it finishes pictures, it is no loss.
There is no CPU fallback; `fill_holes_ops` states the same in torch ops on any
device (the op route: the second check and the context of the measurements).
"""
import numpy as np
import torch

from lsi import _C

TILE = _C.LSI_FILL_TILE
MODES = {'conf': _C.LSI_FILL_CONF, 'splat': _C.LSI_FILL_SPLAT}


def _check(img, w):
  for name, t in (('img', img), ('conf', w)):
    if not isinstance(t, torch.Tensor):
      raise TypeError('%s must be a tensor' % name)
    if t.dtype != torch.float32:
      raise RuntimeError('fill_holes is fp32 (got %s for %s)' % (t.dtype, name))
    if not t.is_contiguous():
      raise RuntimeError('fill_holes needs a contiguous %s' % name)
  if img.dim() != 4 or not 1 <= img.shape[3] <= 4:
    raise RuntimeError('img is N x H x W x C with C in 1 .. 4, got %s' % (tuple(img.shape),))
  if tuple(w.shape) not in (tuple(img.shape[:3]), tuple(img.shape[:3]) + (1,)):
    raise RuntimeError('conf is N x H x W [x 1] = %s, got %s' %
                       (tuple(img.shape[:3]), tuple(w.shape)))
  for name, t in (('img', img), ('conf', w)):
    if not t.is_cuda:
      raise RuntimeError('fill_holes needs %s on a ROCm GPU (got device %s); there '
                         'is no CPU fallback' % (name, t.device))


def _fill(img, w, mode, bg_wt, bg_value, conf_min, out=None, workspace=None):
  _check(img, w)
  dev = _C.require_device(img, w)
  n, h, wd, c = img.shape
  lib = _C.lib()
  with torch.cuda.device(dev):
    if out is None:
      out = torch.empty_like(img)
    elif (out.shape != img.shape or out.dtype != torch.float32 or out.device != dev or
          not out.is_contiguous() or out.data_ptr() == img.data_ptr()):
      raise RuntimeError('out must be a contiguous fp32 tensor of the shape of img on its '
                         'device, and not img itself')
    if workspace is None:
      # (for a shape the library refuses the size is 0: it reports it itself)
      need = int(lib.lsi_fill_holes_workspace_bytes(n, h, wd, c))
      workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _C.check(lib.lsi_fill_holes(
        n, h, wd, c, img.data_ptr(), w.data_ptr(), mode, float(bg_wt), float(bg_value),
        float(conf_min), out.data_ptr(), workspace.data_ptr(), workspace.numel(),
        _C.stream_ptr(dev)), 'lsi_fill_holes')
  return out


def fill_holes(img, conf, conf_min=1e-3, bg_value=1.0, out=None, workspace=None):
  """img with its holes filled: N x H x W x C; module doc.  `workspace`: a uint8
  device tensor of lsi_fill_holes_workspace_bytes to reuse between calls.  3
  launches whatever the data."""
  return _fill(img, conf, _C.LSI_FILL_CONF, 0.0, bg_value, conf_min, out, workspace)


def canvas_weight(bg_layer_disp, max_disp, zbuf_scale, n_layers=1):
  """The weight of the canvas under a composed rendering of `n_layers` layers,
  as forward_splat derives it: every layer is splatted onto a canvas of
  lsi_bg_weight and the canvases are summed (fp32)."""
  bg_wt = np.float32(_C.bg_weight(bg_layer_disp, max_disp, zbuf_scale))
  total = np.float32(0)
  for _ in range(int(n_layers)):
    total = np.float32(total + bg_wt)
  return float(total)


def fill_splat_holes(trg_img, trg_wts, bg_layer_disp, max_disp, zbuf_scale,
                     conf_min=1e-3, n_layers=1, out=None, workspace=None):
  """The composed rendering 1 x B x H x W x C of forward_splat with the canvas
  taken out and the holes filled; trg_wts: its weight sums 1 x B x H x W x 1.
  bg_layer_disp, max_disp, zbuf_scale: what the rendering was made with, and
  n_layers the number of layers it composed (`canvas_weight`: the canvas weight
  is derived as forward_splat derives it).  An unreached pixel whose weight
  differs from that by rounding has a share of 1e-7: below any useful conf_min."""
  if trg_img.dim() != 5 or trg_img.shape[0] != 1 or trg_wts.dim() != 5:
    raise RuntimeError('fill_splat_holes takes the 1 x B x H x W x C outputs of a composed '
                       'forward_splat, got %s and %s' %
                       (tuple(trg_img.shape), tuple(trg_wts.shape)))
  bg_wt = canvas_weight(bg_layer_disp, max_disp, zbuf_scale, n_layers)
  filled = _fill(trg_img[0], trg_wts[0], _C.LSI_FILL_SPLAT, bg_wt, 1.0, conf_min,
                 None if out is None else out[0], workspace)
  return filled.unsqueeze(0) if out is None else out


def splat_confidence(trg_wts, bg_layer_disp, max_disp, zbuf_scale, conf_min=1e-3, n_layers=1):
  """c0 of LSI_FILL_SPLAT in torch ops: the share of every pixel of a rendering
  that came from the layers (1 - it is the hole)."""
  bg_wt = torch.tensor(canvas_weight(bg_layer_disp, max_disp, zbuf_scale, n_layers),
                       dtype=torch.float32, device=trg_wts.device)
  c = torch.where(trg_wts > bg_wt, (trg_wts - bg_wt) / trg_wts, torch.zeros_like(trg_wts))
  return torch.where(c < conf_min, torch.zeros_like(c), c)


def _push_ops(v):
  h, w = v.shape[1:3]
  v = torch.nn.functional.pad(v, (0, 0, 0, w % 2, 0, h % 2))
  s = ((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + (v[:, 1::2, 0::2] + v[:, 1::2, 1::2]))
  sc = s[..., -1:]
  over = sc > 1
  div = torch.where(over, sc, torch.ones_like(sc))
  return torch.cat([torch.where(over, s[..., :-1] / div, s[..., :-1]),
                    torch.where(over, torch.ones_like(sc), sc)], dim=-1)


def _upsample_ops(f, h, w):
  hu, wu = f.shape[1:3]
  y = torch.arange(h, device=f.device)
  x = torch.arange(w, device=f.device)
  cy, cx = y >> 1, x >> 1
  ny = (cy + (y & 1) * 2 - 1).clamp(0, hu - 1)
  nx = (cx + (x & 1) * 2 - 1).clamp(0, wu - 1)
  g = lambda iy, ix: f[:, iy][:, :, ix]
  return ((9.0 * g(cy, cx) + 3.0 * g(cy, nx)) + (3.0 * g(ny, cx) + g(ny, nx))) * 0.0625


def fill_holes_ops(img, conf, conf_min=1e-3, bg_value=1.0, mode='conf', bg_wt=0.0):
  """`fill_holes` (mode 'conf') or the filling of `fill_splat_holes` (mode
  'splat', conf = the weight sums, bg_wt the canvas weight) in torch ops on the
  tensors' device: the same definition, a dozen ops per level."""
  img, w = img.float(), conf.float().reshape(img.shape[:3])
  zero = torch.zeros_like(w)
  if MODES[mode] == _C.LSI_FILL_CONF:
    c = torch.where(w > 0, w.clamp(max=1.0), zero)
    p = img * c.unsqueeze(-1)
  else:
    c = torch.where(w > bg_wt, (w - bg_wt) / w, zero)
    p = img - ((1.0 - c) * bg_value).unsqueeze(-1)
  c = torch.where(c < conf_min, zero, c)
  p = torch.where((c == 0).unsqueeze(-1), torch.zeros_like(p), p)
  levels = [torch.cat([p, c.unsqueeze(-1)], dim=-1)]
  while tuple(levels[-1].shape[1:3]) != (1, 1):
    levels.append(_push_ops(levels[-1]))
  top = levels[-1]
  pos = top[..., -1:] > 0
  f = torch.where(pos, top[..., :-1] / torch.where(pos, top[..., -1:],
                                                   torch.ones_like(top[..., -1:])),
                  torch.full_like(top[..., :-1], bg_value))
  for v in levels[-2::-1]:
    f = v[..., :-1] + (1.0 - v[..., -1:]) * _upsample_ops(f, v.shape[1], v.shape[2])
  return f
