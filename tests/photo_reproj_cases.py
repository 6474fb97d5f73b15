"""Inputs and references shared by tests/test_photo_reproj_cpu.py (which holds
the inputs to their conditions, from restatement (a) alone) and
tests/test_photo_reproj_gpu.py (which runs the kernels on them).

Poses, cameras and the disparity recipe are those of tests/test_geo_cons_gpu.py
(restated here, so that the CPU tests import no GPU test module):
focal 0.9 W, 'rect' / 'general' / 'yaw60' / 'yaw180' / 'same'; the first half of
the Q views is projected with the forward matrix, the second with the inverse of
the same pose, shift = Q / 2 (the paired buffer) -- or, in the two-tensor form,
every view with the forward matrix and shift 0.  Plane p = l Q + q is layer l of
view q: layer 0 is the 0.4 k / 256 surface, layer l lies behind it at 1 - l / 5
of its disparity.  The partner is layer 0 of the sampled views (in the two-tensor
form a surface of its own).  Planted per plane of 100 pixels or more, at distinct
pixels: d = 0, NaN and negative, one NaN texture value, one NaN image value per
image plane, and -- in layer 0 of the first half's views -- a 3 x 3 patch at a
third of its disparity: the point lies well behind the partner's surface.
Textures and images are smooth colour ramps plus integer noise, over 256."""
import functools
import os
import sys

import numpy as np
import torch

import photo_reproj_ref as ref

UPSTREAM = 2.5
OCCL = 0.2
EPS = 1e-3

# name: P, Q, H, W, C
SHAPES = {
    'a': (4, 2, 13, 37, 3),     # two layers, ragged rows, one block per plane
    'b': (2, 2, 40, 150, 3),    # several blocks per plane, waves straddle row ends
    'c': (16, 8, 9, 17, 3),     # the training plane count
    'd': (2, 2, 1, 1, 3),       # one pixel
    'e': (2, 2, 24, 72, 1),     # one channel
    'f': (2, 2, 13, 37, 4),     # four channels
    'p': (4, 2, 13, 37, 3),     # a's values in one packed RGBD buffer, img at x-stride 2
    't': (4, 2, 13, 37, 3),     # a's shape, the two-tensor form: shift 0, a partner of its own
}
VALUES = {'p': 'a'}
TWO_TENSORS = ('t',)
EMPTY_POSES = ('yaw60', 'yaw180')
# (shape, pose, mode, occl_thresh).  Every shape sees both poses, one with the
# occlusion rule and one without (which pose gets it alternates with the shape),
# and the modes alternate every other shape, so that each pairing of mode and
# threshold occurs; the rows after that add the pairings a shape misses that
# way where the shape is there for the partner (c: the training plane count, f:
# four channels, t: the two-tensor form, a), the one pixel and the empty poses.
RUNS = ([(n, pose, ref.MODES[(i // 2 + j) % 2], OCCL * ((i + j + 1) % 2))
         for i, n in enumerate('abcefpt') for j, pose in enumerate(('rect', 'general'))] +
        [('a', 'rect', 'charb', OCCL), ('a', 'general', 'l1', OCCL),
         ('c', 'general', 'charb', OCCL), ('f', 'general', 'l1', OCCL),
         ('t', 'rect', 'l1', OCCL), ('t', 'general', 'charb', OCCL),
         ('d', 'same', 'l1', 0.0), ('d', 'same', 'charb', OCCL),
         ('d', 'rect', 'l1', 0.0), ('a', 'yaw60', 'l1', 0.0),
         ('c', 'yaw180', 'charb', OCCL), ('t', 'yaw60', 'charb', OCCL)])
assert len(set(RUNS)) == len(RUNS)

POSES = {
    'same': ((0, 0, 0), (0, 0, 0)),
    'rect': ((0, 0, 0), (-0.54, 0, 0)),
    'general': ((2, -4, 3), (0.3, -0.1, 0.25)),
    'yaw60': ((0, 60, 0), (0, 0, 0)),
    'yaw180': ((0, 180, 0), (0, 0, 0)),
}


def _rotation(deg):
  rx, ry, rz = np.deg2rad(np.asarray(deg, np.float64))
  cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
  Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
  Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
  Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
  return (Rz @ Ry @ Rx).astype(np.float32)


@functools.lru_cache(maxsize=None)
def matrices(h, w, pose):
  """(forward, inverse) 4 x 4 fp32 of the pose between two 0.9 W cameras (host
  code only: lsi.geometry.projection)."""
  pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                     'layered-scene-inference_amd')
  if pkg not in sys.path:
    sys.path.insert(0, pkg)
  from lsi.geometry import projection
  deg, t = POSES[pose]
  if pose == 'same':
    # exactly I (K I K^-1 in fp32 is I only to an ulp, and one pixel is scored
    # only at u = v = 0.5 exactly)
    return np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
  k = torch.tensor([[[0.9 * w, 0, w / 2.0], [0, 0.9 * w, h / 2.0], [0, 0, 1]]],
                   dtype=torch.float32)
  rot = torch.from_numpy(_rotation(deg))[None]
  t = torch.tensor(t, dtype=torch.float32).reshape(1, 3, 1)
  fwd = projection.forward_projection_matrix(k, k, rot, t)
  inv = projection.inverse_projection_matrix(k, k, rot, t)
  return fwd[0].numpy().copy(), inv[0].numpy().copy()


@functools.lru_cache(maxsize=None)
def make_inputs(name, pose):
  """(T, D, I, M, E, shift, patch) fp32 NumPy (patch: bool P x H x W)."""
  two = name in TWO_TENSORS
  p, q, h, w, c = SHAPES[name]
  rng = np.random.RandomState(sum(map(ord, VALUES.get(name, name))) + 29)
  yy, xx = np.mgrid[0:h, 0:w]

  def surface(n):
    k = np.stack([150 + 25 * np.sin(0.2 * xx + 0.5 * i) + 20 * np.cos(0.3 * yy) +
                  rng.randint(-6, 7, (h, w)) for i in range(n)])
    return (0.4 * np.round(k) / 256).astype(np.float32)

  def colours(n, phase):
    k = np.stack([np.stack([128 + 60 * np.sin(0.15 * xx + 0.4 * i + ch + phase) +
                            50 * np.cos(0.2 * yy - 0.3 * ch) + rng.randint(-8, 9, (h, w))
                            for ch in range(c)], axis=-1) for i in range(n)])
    return (np.round(k) / 256).astype(np.float32)

  layer0 = surface(q)
  D = np.concatenate([(layer0 * np.float32(1.0 - l / 5.0)).astype(np.float32)
                      for l in range(p // q)])
  E = surface(q) if two else None
  T, I = colours(p, 0.0), colours(q, 0.1)
  fwd, inv = matrices(h, w, pose)
  if two:
    M, shift = np.stack([fwd] * q), 0
  else:
    M, shift = np.stack([fwd] * (q // 2) + [inv] * (q // 2)), q // 2
  patch = np.zeros((p, h, w), bool)
  if h * w >= 100:
    for pl in range(p):
      idx = rng.permutation(h * w)
      D[pl].flat[idx[:3]] = (0.0, np.nan, -0.25)
      T[pl].reshape(-1, c)[idx[3], pl % c] = np.nan
      if pl < q:
        I[pl].reshape(-1, c)[idx[4], pl % c] = np.nan
        if two:
          E[pl].flat[idx[5:7]] = (np.nan, 0.0)
      if pl < (q if two else q // 2):   # layer 0 (of the first half's views)
        y0, x0 = h // 2 - 1, w // 2 - 1
        patch[pl, y0:y0 + 3, x0:x0 + 3] = True
    D = np.where(patch, (0.4 * np.floor(D * 640 / 3) / 256).astype(np.float32), D)
  if not two:
    E = D[:q].copy()              # layer 0 of the views: the visible surface
  return T, D, I, M.astype(np.float32), E, shift, patch


@functools.lru_cache(maxsize=None)
def case_reference(name, pose, mode, occl):
  """Reference of a run, computed once and shared (read-only): restatement (a)
  with the gradient of loss * UPSTREAM, and (b)'s own fp32 errors against it."""
  T, D, I, M, E, shift, patch = make_inputs(name, pose)
  l, gT, gD, sums, emap, sc = ref.loss_and_grad(T, D, I, M, E, shift, mode, occl, EPS,
                                                UPSTREAM)
  t = torch.from_numpy
  l32, t32, d32 = ref.loss_and_grad_ops(t(T), t(D), t(I), t(M), t(E), shift, mode, occl,
                                        EPS, UPSTREAM)
  tmax, dmax = np.abs(gT).max(), np.abs(gD).max()
  terr, derr = np.abs(t32 - gT).max(), np.abs(d32 - gD).max()
  return {'loss': l, 'gT': gT, 'gD': gD, 'sums': sums, 'map': emap, 'scored': sc,
          'tmax': tmax, 'dmax': dmax, 'patch': patch,
          'loss_err32': abs(l32 - l) / abs(l) if l else abs(l32),
          'gT_err32': float(terr / tmax) if tmax else float(terr),
          'gD_err32': float(derr / dmax) if dmax else float(derr)}


def lattice_inputs():
  """The quarter-pixel lattice: M = I with M[0][3] = 8, d multiples of 1/32 up to
  2 (u on the quarter-pixel lattice, weights multiples of 1/4), colours multiples
  of 1/8 below 2, one channel: every sample a multiple of 1/128, every e too; in
  l1 mode nothing rounds, in any order."""
  p, q, h, w = 2, 2, 13, 37
  rng = np.random.RandomState(3)
  D = (rng.randint(1, 65, (p, h, w)) / 32.0).astype(np.float32)
  T = (rng.randint(0, 16, (p, h, w, 1)) / 8.0).astype(np.float32)
  I = (rng.randint(0, 16, (q, h, w, 1)) / 8.0).astype(np.float32)
  M = np.tile(np.eye(4, dtype=np.float32), (q, 1, 1))
  M[:, 0, 3] = 8.0
  return T, D, I, M
