"""KITTI raw Velodyne scans and the matrix that takes them into an image: the
ground truth of the depth evaluation of Eigen et al. 2014 and Garg et al. 2016
(lsi.geometry.lidar rasterises the points).

A scan is `velodyne_points/data/N.bin`: float32 quadruples x y z reflectance in
the scanner's frame (x forward, y left, z up, metres).  `calib_velo_to_cam.txt`
holds the rigid motion R, T into the frame of camera 0; `calib_cam_to_cam.txt`
holds the rectifying rotation R_rect_00 and the projections P_rect_0x of the
rectified cameras.  A point lands in camera x at

    (X, Y, Z)^T = P_rect_0x [R_rect_00 0; 0 1] [R T; 0 1] (x, y, z, 1)^T,

at KITTI's pixel coordinate (X / Z, Y / Z), which puts integers at pixel
centres.

Pixel convention.  `velo_to_image` folds the resize to h x w and the choice of
the pixel a coordinate belongs to into rows 0 and 1, so that floor(X' / Z) is
directly the column (and floor(Y' / Z) the row) of the h x w pixel whose area
holds the point:

    row0' = (w / W0) (row0 + (0.5 - origin) row2),   row1' alike with h / H0.

With origin = 0 a native-size point goes to round-half-up of its KITTI
coordinate: pixel i covers [i - 0.5, i + 0.5).  origin = 1 is the widely copied
"- 1" of the monodepth evaluation script (`round(x) - 1`, its authors' remnant
of MATLAB's 1-based indices): every point one pixel further up and left.
"""
import os

import numpy as np

from lsi.data.kitti.data import read_calib_file


def load_scan(path):
  """The scan as [n, 4] float32 (x, y, z, reflectance)."""
  size = os.path.getsize(path)
  if size % 16 != 0:
    raise ValueError('%s is no Velodyne scan: %d bytes is not a multiple of the '
                     '16 bytes of a point' % (path, size))
  return np.fromfile(path, dtype='<f4').astype(np.float32, copy=False).reshape(-1, 4)


def read_velo_calib(path):
  """(R 3 x 3, T 3) of calib_velo_to_cam.txt, float64."""
  calib = read_calib_file(path)
  for key, n in (('R', 9), ('T', 3)):
    if not isinstance(calib.get(key), np.ndarray) or calib[key].size != n:
      raise ValueError('%s: no %s with %d numbers' % (path, key, n))
  return calib['R'].reshape(3, 3), calib['T'].reshape(3)


def velo_to_image(calib_cam, calib_velo, cam, src_shape, h, w, origin=0.0,
                  dtype=np.float32):
  """The 3 x 4 float32 (`dtype`) matrix from scanner coordinates to the h x w image of
  rectified camera `cam` (2 or 3), composed in float64 (module doc).
  calib_cam: read_calib_file of calib_cam_to_cam.txt; calib_velo: (R, T) of
  read_velo_calib; src_shape: (H0, W0, ...) of the camera's native image."""
  rot, trans = calib_velo
  velo = np.eye(4)
  velo[:3, :3] = np.asarray(rot, np.float64).reshape(3, 3)
  velo[:3, 3] = np.asarray(trans, np.float64).reshape(3)
  rect = np.eye(4)
  rect[:3, :3] = np.asarray(calib_cam['R_rect_00'], np.float64).reshape(3, 3)
  proj = np.asarray(calib_cam['P_rect_0%d' % cam], np.float64).reshape(3, 4)
  m = proj @ rect @ velo
  m[0] = (w / float(src_shape[1])) * (m[0] + (0.5 - origin) * m[2])
  m[1] = (h / float(src_shape[0])) * (m[1] + (0.5 - origin) * m[2])
  return m.astype(dtype)
