"""Camera paths through a stereo pair (host only: float64 NumPy, cast to fp32).

    k, rot, t = interpolate_cameras(k_s, k_t, rot, t, s)

(k_t, rot, t) is the target camera of a pair as the data loaders give it --
intrinsics B x 3 x 3, rotation B x 3 x 3 and translation B x 3 x 1 of the
source -> target motion -- and k_s the source intrinsics.  For every scalar of
`s` the camera at that fraction of the motion:

    k(s) = (1 - s) k_s + s k_t,   R(s) = exp(s log R),   t(s) = s t

s = 0 is the source camera (R = I, t = 0), s = 1 exactly (k_t, rot, t), bit
for bit after the cast; values outside [0, 1] extrapolate.  The rotation goes
through its axis and angle, so R(a) R(b) = R(a + b); R = I is handled exactly.
Returns CPU float32 tensors K x B x 3 x 3, K x B x 3 x 3, K x B x 3 x 1.
"""
import numpy as np
import torch


def _host(x):
  if isinstance(x, torch.Tensor):
    x = x.detach().cpu().numpy()
  return np.asarray(x)


def axis_angle(rot):
  """(unit axis [3], angle in [0, pi]) of a 3 x 3 rotation, float64; the axis of
  the identity is (0, 0, 1) with angle exactly 0."""
  r = np.asarray(rot, np.float64)
  v = 0.5 * np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
  sin, cos = np.linalg.norm(v), 0.5 * (np.trace(r) - 1.0)
  if sin == 0.0 and cos > 0.0:
    return np.array([0.0, 0.0, 1.0]), 0.0
  angle = np.arctan2(sin, cos)
  if sin > 1e-6:
    return v / sin, angle
  # close to pi the antisymmetric part vanishes: R + I = 2 a a^T there
  sym = 0.5 * (r + np.eye(3))
  j = int(np.argmax(np.diag(sym)))
  a = sym[j] / np.sqrt(sym[j, j])
  if np.dot(a, v) < 0:
    a = -a
  return a / np.linalg.norm(a), angle


def rotation(axis, angle):
  """Rodrigues: the rotation by `angle` about the unit `axis`, float64."""
  x, y, z = axis
  k = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
  return np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * np.matmul(k, k)


def interpolate_cameras(k_s, k_t, rot, t, s):
  """Module doc.  s: a scalar or a sequence of K scalars."""
  k_s, k_t, rot, t = _host(k_s), _host(k_t), _host(rot), _host(t)
  b = rot.shape[0]
  if k_s.shape != (b, 3, 3) or k_t.shape != (b, 3, 3) or rot.shape != (b, 3, 3) or \
      t.shape != (b, 3, 1):
    raise ValueError('cameras are B x 3 x 3 (k_s, k_t, rot) and B x 3 x 1 (t), got %s' %
                     ([x.shape for x in (k_s, k_t, rot, t)],))
  s = np.atleast_1d(np.asarray(s, np.float64))
  if s.ndim != 1 or not np.isfinite(s).all():
    raise ValueError('s is a finite scalar or a sequence of them')
  f32 = lambda x: np.asarray(x, np.float32)
  logs = [axis_angle(rot[i]) for i in range(b)]
  ks, rots, ts = [], [], []
  for v in s:
    if v == 1.0:          # the inputs themselves, whatever the cast of a product gives
      ks.append(f32(k_t)), rots.append(f32(rot)), ts.append(f32(t))
      continue
    ks.append(f32((1.0 - v) * k_s.astype(np.float64) + v * k_t.astype(np.float64)))
    rots.append(f32(np.stack([rotation(axis, v * angle) for axis, angle in logs])))
    ts.append(f32(v * t.astype(np.float64)))
  as_t = lambda xs: torch.from_numpy(np.ascontiguousarray(np.stack(xs)))
  return as_t(ks), as_t(rots), as_t(ts)
