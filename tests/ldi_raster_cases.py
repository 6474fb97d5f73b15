"""The inputs test_ldi_raster_cpu.py and test_ldi_raster_gpu.py share: LDIs with
invalid texels, coinciding layers and a mask, and per item three source-to-target
matrices -- the identity, a rectified shift, a general pose with forward motion
(up to about 2 x magnification) and a mirrored view among them.  The restatement
of a case is computed once (`reference`) and read only."""
import functools

import numpy as np

import ldi_raster_ref as R

F = np.float32
SHAPES = {'small': (2, 2, 9, 13, 11, 17),       # L, B, H, W, Ht, Wt
          'big': (2, 2, 20, 37, 24, 40)}        # 1480 texels per view: 6 workgroups, ragged
V = 3
DISP_MIN = 0.05

# name: shape, layout, mask, edge_ratio, merge_ratio, max_extent, cull_back
CASES = {
    'small-packed': ('small', 'packed', False, 0.0, 0.0, 32, False),
    'small-planar-mask-cut-merge': ('small', 'planar', True, 0.8, 0.95, 32, False),
    'big-packed-mask-cut': ('big', 'packed', True, 0.8, 0.0, 32, False),
    'big-planar-merge': ('big', 'planar', False, 0.0, 0.95, 32, False),
    'big-packed-extent2': ('big', 'packed', False, 0.0, 0.0, 2, False),
    'small-planar-mask-extent2': ('small', 'planar', True, 0.8, 0.0, 2, False),
    'big-packed-mask-cull': ('big', 'packed', True, 0.8, 0.0, 32, True),
    'small-packed-cull': ('small', 'packed', False, 0.0, 0.95, 32, True),
}
MIRRORED = (1, 0)         # (item, view) of the mirrored matrix
IDENTITY = (0, 0)
GENERAL = (0, 2)


def intrinsics(h, w):
  return np.array([[0.58 * w, 0, w / 2.0], [0, 0.58 * w, h / 2.0], [0, 0, 1]], np.float64)


def rotation(yaw, pitch, roll):
  cy, sy, cp, sp, cr, sr = (np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch),
                            np.cos(roll), np.sin(roll))
  ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
  rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
  rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
  return rz @ rx @ ry


def pose_matrix(h, w, ht, wt, rot, t):
  """pad(K_t) [R t; 0 1] pad(K_s^-1) with K_t the source intrinsics scaled to
  the target size: what forward_projection_matrix and render_views build."""
  k = intrinsics(h, w)
  kt = np.diag([wt / float(w), ht / float(h), 1.0]) @ k
  pad = lambda m: np.block([[m, np.zeros((3, 1))], [np.zeros((1, 3)), np.ones((1, 1))]])
  ext = np.eye(4)
  ext[:3, :3], ext[:3, 3] = rot, t
  return (pad(kt) @ ext @ pad(np.linalg.inv(k))).astype(F)


def matrices(h, w, ht, wt):
  """B x V x 4 x 4 for B = 2."""
  eye = np.eye(3)
  mirror = np.array([[-wt / float(w), 0, wt, 0], [0, ht / float(h), 0, 0], [0, 0, 1, 0],
                     [0, 0, 0, 1]], F)
  return np.stack([
      np.stack([np.eye(4, dtype=F),
                pose_matrix(h, w, ht, wt, eye, [-0.3, 0, 0]),
                pose_matrix(h, w, ht, wt, rotation(0.05, -0.03, 0.08), [0.06, -0.04, -0.8])]),
      np.stack([mirror,
                pose_matrix(h, w, ht, wt, rotation(-0.04, 0.02, -0.05), [-0.1, 0.05, -0.6]),
                pose_matrix(h, w, ht, wt, eye, [0.25, 0, 0])])])


def ldi(shape, seed=0):
  """tex L x B x H x W x 3, mask L x B x H x W, disp L x B x H x W: layer 1
  equals layer 0 on half of the texels (the lowest id must win there, and
  merge_ratio merges them) and lies behind it elsewhere; NaN, inf and
  below-disp_min texels in both layers."""
  nl, nb, h, w = SHAPES[shape][:4]
  rs = np.random.RandomState(seed)
  tex = rs.rand(nl, nb, h, w, 3).astype(F)
  disp = (0.25 + 0.35 * rs.rand(nl, nb, h, w)).astype(F)
  same = rs.rand(nb, h, w) < 0.5
  disp[1] = np.where(same, disp[0], (disp[0] * F(0.5) + F(0.02) * disp[1]).astype(F))
  bad = rs.rand(nl, nb, h, w)
  disp[bad < 0.03] = np.nan
  disp[(bad >= 0.03) & (bad < 0.05)] = np.inf
  disp[(bad >= 0.05) & (bad < 0.08)] = 0.01      # below DISP_MIN
  mask = rs.rand(nl, nb, h, w).astype(F)
  mask[rs.rand(nl, nb, h, w) < 0.02] = np.nan
  return tex, mask, disp


def inputs(name):
  shape, layout, use_mask, edge_ratio, merge_ratio, max_extent, cull = CASES[name]
  nl, nb, h, w, ht, wt = SHAPES[shape]
  tex, mask, disp = ldi(shape)
  par = dict(disp_min=DISP_MIN, mask_min=0.3, edge_ratio=edge_ratio, merge_ratio=merge_ratio,
             max_extent=max_extent, bg_value=0.75, cull_back=cull)
  return dict(tex=tex, mask=mask if use_mask else None, disp=disp, M=matrices(h, w, ht, wt),
              ht=ht, wt=wt, layout=layout, par=par)


@functools.lru_cache(maxsize=None)
def reference(name):
  c = inputs(name)
  return R.raster(c['tex'], c['mask'], c['disp'], c['M'], c['ht'], c['wt'], **c['par'])


def magnifying_matrix():
  """2.5 x with shear and sub-pixel offsets, for a single fully valid layer."""
  return np.array([[2.5, 0.3, 0.37, 0], [0.2, 2.5, 0.21, 0], [0, 0, 1, 0], [0, 0, 0, 1]], F)


def interior(count):
  """(y0, y1, x0, x1) of the largest rectangle of rows and columns of `count`
  (Ht x Wt) that are covered throughout: the rows and columns whose every pixel
  between the first and last such column / row is covered."""
  full = count > 0
  rows = np.nonzero(full.any(1))[0]
  cols = np.nonzero(full.any(0))[0]
  y0, y1, x0, x1 = rows[0], rows[-1], cols[0], cols[-1]
  while not full[y0:y1 + 1, x0:x1 + 1].all():      # shrink the worst side
    sides = {'y0': full[y0, x0:x1 + 1].mean(), 'y1': full[y1, x0:x1 + 1].mean(),
             'x0': full[y0:y1 + 1, x0].mean(), 'x1': full[y0:y1 + 1, x1].mean()}
    worst = min(sides, key=sides.get)
    if worst == 'y0':
      y0 += 1
    elif worst == 'y1':
      y1 -= 1
    elif worst == 'x0':
      x0 += 1
    else:
      x1 -= 1
  return y0, y1, x0, x1
