"""LiDAR scans rasterised into depth maps on the device: a scatter with a
z-buffer and an optional occlusion filter (csrc/lsi_lidar.hip, DESIGN.md
section 4.19).

    depth = rasterize_points(points, first, count, mats, h, w)

points: float32 [N, 4] (x y z reflectance; scan b is rows first[b] ..
first[b] + count[b]) or [B, Nmax, 4] (first may be None: b Nmax); mats: float32
[B, V, 12] or [B, V, 3, 4], V = 1 or 2 views per scan.  The result is
B x V x h x w x 1 float32, 0 where no point landed: per pixel the smallest
Z = row 2 of the matrix applied to the point, over the points with
z_min <= Z <= z_max whose (X / Z, Y / Z) falls inside [0, w) x [0, h); with
`inverse` 1 / Z.  All fp32 in a fixed order: the result is a function of the
inputs alone, bit for bit, whatever the order of the points.  With
occl_window = (wy, wx) != (0, 0) a pixel is emptied when the nearest depth of
its (2 wy + 1) x (2 wx + 1) neighbourhood times occl_ratio is still nearer than
it: background returns seen through a foreground edge, because the scanner does
not sit where the camera does.  Not differentiable -- it produces data.  There is
no CPU fallback; `rasterize_points_ops` states the same in torch ops on any
device (the op route: context for the measurements, not the yardstick).
"""
import ctypes

import numpy as np
import torch

from lsi import _C

# the finishing kernel's LDS tile (rows, columns): sizes around it are where its
# halo and its edge handling can go wrong
TILE = (_C.LSI_LIDAR_TILE_H, _C.LSI_LIDAR_TILE_W)


def _scans(points, first, count):
  """(points as [N, 4], first and count as int64 / int32 NumPy arrays)."""
  if not isinstance(points, torch.Tensor):
    raise TypeError('points must be a tensor')
  if points.dim() not in (2, 3) or points.shape[-1] != 4:
    raise RuntimeError('points are [N, 4] or [B, Nmax, 4], got %s' % (tuple(points.shape),))
  host = lambda v: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else
                    np.asarray(v))
  count = host(count).astype(np.int32).reshape(-1)
  if points.dim() == 3:
    if first is None:
      first = np.arange(points.shape[0], dtype=np.int64) * points.shape[1]
    if count.shape[0] != points.shape[0]:
      raise RuntimeError('%d counts for %d scans' % (count.shape[0], points.shape[0]))
  elif first is None:
    raise RuntimeError('first may be None only with points [B, Nmax, 4]')
  first = host(first).astype(np.int64).reshape(-1)
  if first.shape != count.shape:
    raise RuntimeError('first %s and count %s differ' % (first.shape, count.shape))
  return points.reshape(-1, 4), first, count


def _mats(mats, b):
  if mats.dim() == 4 and tuple(mats.shape[2:]) == (3, 4):
    mats = mats.reshape(mats.shape[0], mats.shape[1], 12)
  if mats.dim() != 3 or mats.shape[0] != b or mats.shape[2] != 12:
    raise RuntimeError('mats are [B, V, 12] or [B, V, 3, 4] with B = %d, got %s' %
                       (b, tuple(mats.shape)))
  return mats


def rasterize_points(points, first, count, mats, h, w, z_min=1e-3, z_max=80.,
                     occl_window=(0, 0), occl_ratio=1.0, inverse=False):
  """B x V x h x w x 1 depth (or inverse depth) maps of the scans; module doc.
  first, count: sequences, NumPy arrays or tensors (a device tensor is read
  back: the grid is sized on the host).  3 launches whatever the data."""
  for name, t in (('points', points), ('mats', mats)):
    if isinstance(t, torch.Tensor) and not t.is_cuda:
      raise RuntimeError(
          'rasterize_points needs %s on a ROCm GPU (got device %s); there is no '
          'CPU fallback' % (name, t.device))
  flat, first, count = _scans(points, first, count)
  dev = _C.require_device(flat, mats)
  if flat.dtype != torch.float32 or mats.dtype != torch.float32:
    raise RuntimeError('rasterize_points is fp32 (got %s, %s)' % (flat.dtype, mats.dtype))
  b = count.shape[0]
  mats = _mats(mats, b).contiguous()
  v = mats.shape[1]
  flat = flat.contiguous()
  h, w, win_y, win_x = int(h), int(w), int(occl_window[0]), int(occl_window[1])
  desc = (_C.LsiScanDesc * max(b, 1))()
  for k in range(b):
    desc[k].first, desc[k].n = int(first[k]), int(count[k])
  lib = _C.lib()
  with torch.cuda.device(dev):
    desc_dev = torch.frombuffer(desc, dtype=torch.uint8).to(dev)
    out = torch.empty((b, v, h, w, 1), dtype=torch.float32, device=dev)
    # (for arguments the library refuses the size is 0: it reports them itself)
    need = int(lib.lsi_lidar_workspace_bytes(b, v, h, w, win_y, win_x))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _C.check(lib.lsi_lidar_rasterize(
        b, v, h, w, ctypes.addressof(desc), desc_dev.data_ptr(),
        flat.data_ptr() if flat.numel() else None, flat.shape[0], mats.data_ptr(),
        float(z_min), float(z_max), win_y, win_x, float(occl_ratio),
        _C.LSI_LIDAR_INVERSE if inverse else 0, out.data_ptr(), ws.data_ptr(),
        ws.numel(), _C.stream_ptr(dev)), 'lsi_lidar_rasterize')
  return out


def rasterize_points_ops(points, first, count, mats, h, w, z_min=1e-3, z_max=80.,
                         occl_window=(0, 0), occl_ratio=1.0, inverse=False):
  """`rasterize_points` in torch ops on the points' device: the same
  definition, one scan and view at a time."""
  flat, first, count = _scans(points, first, count)
  b = count.shape[0]
  mats = _mats(mats, b)
  v = mats.shape[1]
  h, w = int(h), int(w)
  win_y, win_x = int(occl_window[0]), int(occl_window[1])
  dev = flat.device
  inf = float('inf')
  z_min, z_max = (torch.tensor(t, dtype=torch.float32, device=dev) for t in (z_min, z_max))
  zbuf = torch.full((b, v, h * w), inf, dtype=torch.float32, device=dev)
  for k in range(b):
    p = flat[int(first[k]):int(first[k]) + int(count[k])].float()
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    for j in range(v):
      m = mats[k, j].float()
      big_x, big_y, big_z = (((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) +
                             m[4 * r + 3] for r in range(3))
      col, row = big_x / big_z, big_y / big_z
      keep = ((big_z >= z_min) & (big_z <= z_max) & (col >= 0) & (col < w) &
              (row >= 0) & (row < h))
      idx = row[keep].floor().long() * w + col[keep].floor().long()
      zbuf[k, j].scatter_reduce_(0, idx, big_z[keep], 'amin', include_self=True)
  zbuf = zbuf.view(b, v, h, w)
  full = torch.isfinite(zbuf)
  if win_y > 0 or win_x > 0:
    # (max_pool2d pads with -inf: the clipped window's minimum of the non-empty)
    mn = -torch.nn.functional.max_pool2d(-zbuf, (2 * win_y + 1, 2 * win_x + 1), stride=1,
                                         padding=(win_y, win_x))
    full = full & ~(mn * torch.tensor(occl_ratio, dtype=torch.float32, device=dev) < zbuf)
  val = 1.0 / zbuf if inverse else zbuf
  return torch.where(full, val, torch.zeros_like(val)).unsqueeze(-1)
