"""The LiDAR rasteriser's definition (include/lsi_hip.h) restated
in float32 NumPy: the yardstick of tests/test_lidar_cpu.py and
tests/test_lidar_gpu.py.  Every product, sum and quotient is a float32 operation
of its own (NumPy never contracts), in the order the definition gives; the
z-buffer is np.minimum.at and the window minimum a brute-force loop."""
import numpy as np

F = np.float32


def project(pts, mat, h, w, z_min, z_max):
  """(row, col, Z) of the points of one scan that one view keeps."""
  pts = np.asarray(pts, F).reshape(-1, 4)
  m = np.asarray(mat, F).reshape(12)
  x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
  with np.errstate(all='ignore'):
    big = [((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3]
           for r in range(3)]
    assert all(b.dtype == F for b in big)
    keep = (big[2] >= F(z_min)) & (big[2] <= F(z_max))
    u = big[0] / big[2]
    v = big[1] / big[2]
    keep &= (u >= F(0)) & (u < F(w)) & (v >= F(0)) & (v < F(h))
  u, v, depth = u[keep], v[keep], big[2][keep]
  return np.floor(v).astype(np.int64), np.floor(u).astype(np.int64), depth


def zbuffer(pts, mat, h, w, z_min, z_max):
  """h x w float32: the smallest Z per pixel, +inf where no point lands."""
  row, col, depth = project(pts, mat, h, w, z_min, z_max)
  buf = np.full((h, w), np.inf, F)
  np.minimum.at(buf, (row, col), depth)
  return buf


def window_min(buf, win_y, win_x):
  """The minimum of buf over [r - win_y, r + win_y] x [c - win_x, c + win_x]
  clipped to the image (empty pixels are +inf and never win)."""
  h, w = buf.shape
  out = np.empty_like(buf)
  for r in range(h):
    r0, r1 = max(r - win_y, 0), min(r + win_y, h - 1) + 1
    for c in range(w):
      out[r, c] = buf[r0:r1, max(c - win_x, 0):min(c + win_x, w - 1) + 1].min()
  return out


def finish(buf, win_y=0, win_x=0, ratio=1.0, inverse=False):
  """The output map of one z-buffer: the filter, then depth or 1 / depth, 0 where
  empty.  Also returns the number of pixels the filter removed."""
  full = np.isfinite(buf)
  removed = 0
  if win_y > 0 or win_x > 0:
    with np.errstate(all='ignore'):
      drop = full & (window_min(buf, win_y, win_x) * F(ratio) < buf)
    removed = int(drop.sum())
    full = full & ~drop
  safe = np.where(full, buf, F(1))
  val = (F(1) / safe) if inverse else safe
  assert val.dtype == F
  return np.where(full, val, F(0)).astype(F), removed


def rasterize(points, first, count, mats, h, w, z_min=1e-3, z_max=80.,
              occl_window=(0, 0), occl_ratio=1.0, inverse=False, stats=None):
  """B x V x h x w x 1 float32.  points [N, 4] or [B, Nmax, 4]; first None with
  the latter.  stats: a dict that receives 'removed' and 'kept' (pixels)."""
  points = np.asarray(points, F)
  if first is None:
    first = np.arange(points.shape[0]) * points.shape[1]
  flat = points.reshape(-1, 4)
  mats = np.asarray(mats, F).reshape(len(count), -1, 12)
  b, v = mats.shape[:2]
  out = np.zeros((b, v, h, w, 1), F)
  removed = kept = 0
  for i in range(b):
    scan = flat[int(first[i]):int(first[i]) + int(count[i])]
    for j in range(v):
      buf = zbuffer(scan, mats[i, j], h, w, z_min, z_max)
      out[i, j, :, :, 0], r = finish(buf, occl_window[0], occl_window[1], occl_ratio, inverse)
      removed += r
      kept += int((out[i, j] != 0).sum())
  if stats is not None:
    stats['removed'], stats['kept'] = removed, kept
  return out
