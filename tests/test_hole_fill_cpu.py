"""The push-pull hole filler's definition (tests/hole_fill_ref.py, the float32
restatement the kernel is held to in test_hole_fill_gpu.py) on cases with known
answers, the camera paths of lsi.geometry.trajectory, and what `fill_holes`
refuses before it looks for a device.  No GPU."""
import numpy as np
import pytest
import torch

import hole_fill_ref as R

F = np.float32


def rand_img(rs, n, h, w, c):
  return rs.rand(n, h, w, c).astype(F)


# --- the definition -------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (1, 1, 7, 3), (2, 5, 3, 4), (3, 33, 65, 3)])
def test_full_confidence_returns_the_image_bitwise(shape):
  img = rand_img(np.random.RandomState(0), *shape)
  out = R.fill(img, np.ones(shape[:3], F))
  assert out.dtype == F and np.array_equal(out.view(np.uint32), img.view(np.uint32))
  # a confidence above 1 is clamped
  assert np.array_equal(R.fill(img, np.full(shape[:3], 3.5, F)), img)


@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (1, 1, 7, 3), (2, 5, 3, 4), (1, 33, 65, 3)])
def test_all_holes_give_the_background_value(shape):
  img = rand_img(np.random.RandomState(1), *shape)
  for bg in (1.0, 0.25):
    out = R.fill(img, np.zeros(shape[:3], F), bg_value=bg)
    assert out.shape == shape and (out == F(bg)).all()
  # negative and NaN confidences are holes as well
  w = np.full(shape[:3], -1.0, F)
  w[0, 0, 0] = np.nan
  assert (R.fill(img, w) == F(1)).all()


@pytest.mark.parametrize('shape,at', [((1, 1, 1, 3), (0, 0)), ((1, 1, 7, 3), (0, 5)),
                                      ((1, 5, 3, 3), (4, 1)), ((1, 33, 65, 3), (32, 64)),
                                      ((1, 33, 65, 3), (7, 20))])
def test_one_confident_pixel_colours_everything(shape, at):
  img = rand_img(np.random.RandomState(2), *shape)
  colour = np.array([0.2, 0.7, 0.4], F)
  img[0, at[0], at[1]] = colour
  for conf in (1.0, 0.3):
    w = np.zeros(shape[:3], F)
    w[0, at[0], at[1]] = conf
    out = R.fill(img, w)
    assert np.abs(out - colour).max() <= 1e-6, (shape, at, conf)


@pytest.mark.parametrize('shape', [(1, 1, 7, 3), (2, 5, 3, 4), (2, 33, 65, 3)])
def test_constant_colour_survives_any_confidence_pattern(shape):
  rs = np.random.RandomState(3)
  colour = rs.rand(shape[3]).astype(F)
  img = np.broadcast_to(colour, shape).copy()
  w = (rs.rand(*shape[:3]) * (rs.rand(*shape[:3]) > 0.5)).astype(F)
  w[:, 0, 0] = 0.5                                    # no image without any confidence
  out = R.fill(img, w)
  assert np.abs(out - colour).max() <= 1e-6


def test_hand_worked_4x4():
  """One channel; pixel (0, 0) = 1 with confidence 1, pixel (3, 3) = 4 with
  confidence 0.5 (p = 2), holes elsewhere.
    level 1 (2 x 2): p = [[1, 0], [0, 2]], c = [[1, 0], [0, 0.5]]
    level 2 (1 x 1): S_p = 3, S_c = 1.5 > 1: p = 2, c = 1; F_2 = 2
    F_1 = p_1 + (1 - c_1) 2 = [[1, 2], [2, 3]] = 1 + i + j
    the up-sample of a linear map with clamped borders: U = 1 + a[y] + a[x],
    a = [0, 0.25, 0.75, 1]; F_0 = U in the holes, 1 + 0 U at (0, 0) and
    2 + 0.5 * 3 = 3.5 at (3, 3).  Every number is a short dyadic fraction: exact."""
  img = np.full((1, 4, 4, 1), 9.0, F)
  w = np.zeros((1, 4, 4), F)
  img[0, 0, 0, 0], w[0, 0, 0] = 1.0, 1.0
  img[0, 3, 3, 0], w[0, 3, 3] = 4.0, 0.5
  want = np.array([[1.00, 1.25, 1.75, 2.00],
                   [1.25, 1.50, 2.00, 2.25],
                   [1.75, 2.00, 2.50, 2.75],
                   [2.00, 2.25, 2.75, 3.50]], F)
  p, c = R.level0(img, w)
  l1 = R.push(np.concatenate([p, c[..., None]], -1))
  assert np.array_equal(l1[0, :, :, 0], F([[1, 0], [0, 2]]))
  assert np.array_equal(l1[0, :, :, 1], F([[1, 0], [0, 0.5]]))
  assert np.array_equal(R.push(l1)[0, 0, 0], F([2, 1]))
  assert np.array_equal(R.fill(img, w)[0, :, :, 0], want)


@pytest.mark.parametrize('mode', [R.CONF, R.SPLAT])
def test_nan_and_inf_in_holes_do_not_leak(mode):
  rs = np.random.RandomState(4)
  img = rand_img(rs, 2, 33, 65, 3)
  hole = rs.rand(2, 33, 65) > 0.5
  img[hole] = np.where(rs.rand(int(hole.sum()), 3) > 0.5, np.nan, np.inf).astype(F)
  img[0, 0, 0], hole[0, 0, 0] = -np.inf, True
  if mode == R.CONF:
    w = np.where(hole, 0, rs.rand(2, 33, 65)).astype(F)
    out = R.fill(img, w)
  else:       # a hole of a rendering: nothing but the canvas weight
    w = np.where(hole, 1e-7, 0.5 + rs.rand(2, 33, 65)).astype(F)
    out = R.fill(img, w, mode, bg_wt=1e-7)
  assert np.isfinite(out).all() and out.min() >= -1e-6 and out.max() <= 1 + 1e-6


@pytest.mark.parametrize('shape', [(1, 1, 1, 2), (1, 1, 7, 3), (2, 5, 3, 4), (2, 33, 65, 3)])
def test_sizes_against_a_scalar_restatement(shape):
  """The vectorised restatement against the definition written pixel by pixel."""
  rs = np.random.RandomState(5)
  n, h, w, c = shape
  img = rand_img(rs, *shape)
  conf = (rs.rand(n, h, w) * (rs.rand(n, h, w) > 0.5)).astype(F)
  got = R.fill(img, conf, conf_min=0.05, bg_value=0.5)
  for b in range(n):
    c0 = np.where(conf[b] > 0, np.minimum(conf[b], F(1)), F(0)).astype(F)
    c0[c0 < F(0.05)] = 0
    lv = [np.concatenate([np.where(c0[..., None] == 0, F(0), img[b] * c0[..., None]),
                          c0[..., None]], -1).astype(F)]
    while lv[-1].shape[:2] != (1, 1):
      v = lv[-1]
      hh, ww = v.shape[:2]
      nxt = np.zeros(((hh + 1) // 2, (ww + 1) // 2, c + 1), F)
      for y in range(nxt.shape[0]):
        for x in range(nxt.shape[1]):
          g = lambda yy, xx: v[yy, xx] if yy < hh and xx < ww else np.zeros(c + 1, F)
          s = (g(2 * y, 2 * x) + g(2 * y, 2 * x + 1)) + (g(2 * y + 1, 2 * x) + g(2 * y + 1, 2 * x + 1))
          nxt[y, x] = np.append(s[:c] / s[c], F(1)) if s[c] > 1 else s
      lv.append(nxt)
    f = lv[-1][:, :, :c] / lv[-1][:, :, c:] if lv[-1][0, 0, c] > 0 else np.full((1, 1, c), 0.5, F)
    for v in lv[-2::-1]:
      hh, ww = v.shape[:2]
      hu, wu = f.shape[:2]
      nf = np.zeros((hh, ww, c), F)
      for y in range(hh):
        cy = y >> 1
        ny = min(max(cy + (1 if y & 1 else -1), 0), hu - 1)
        for x in range(ww):
          cx = x >> 1
          nx = min(max(cx + (1 if x & 1 else -1), 0), wu - 1)
          u = ((F(9) * f[cy, cx] + F(3) * f[cy, nx]) + (F(3) * f[ny, cx] + f[ny, nx])) * F(0.0625)
          nf[y, x] = v[y, x, :c] + (F(1) - v[y, x, c]) * u
      f = nf
    assert np.array_equal(got[b].view(np.uint32), f.astype(F).view(np.uint32)), (shape, b)


def test_splat_mode_recovers_a_covered_foreground():
  """A canvas of value 1 and weight bg_wt under a foreground that reached the
  pixels with a large weight: img = (fg lw + bg_wt) / (lw + bg_wt).  Where it is
  covered the foreground comes back; where nothing landed (img = 1, w = bg_wt)
  the filler puts foreground colours, not the canvas."""
  rs = np.random.RandomState(6)
  bg_wt = 1e-6
  fg = (0.1 + 0.5 * rs.rand(2, 33, 65, 3)).astype(F)      # below 0.6: the canvas is 1
  cover = (rs.rand(2, 33, 65) > 0.4).astype(F)
  img, wts = R.splat_canvas(fg, cover, bg_wt, scale=3.0)
  assert (img[cover == 0] == 1).all() and (wts[cover == 0] == F(bg_wt)).all()
  out = R.fill(img, wts, R.SPLAT, bg_wt=bg_wt)
  assert np.abs(out - fg)[cover == 1].max() <= 2e-6
  assert out[cover == 0].max() <= 0.6 + 1e-6 and out[cover == 0].min() >= 0.1 - 1e-6
  # a thin cover: c0 = lw / (lw + bg_wt) = 1 / 2 leaves the same colour after the canvas
  # has been taken out, and the other half is filled in from the neighbours
  img2, wts2 = R.splat_canvas(fg, cover, bg_wt, scale=bg_wt)
  p, c = R.level0(img2, wts2, R.SPLAT, bg_wt=bg_wt)
  assert np.abs(c[cover == 1] - 0.5).max() <= 1e-6
  assert np.abs(p - 0.5 * fg)[cover == 1].max() <= 1e-6


def test_conf_min_threshold():
  img = np.full((1, 1, 4, 1), 0.5, F)
  w = np.array([[[0.25, 0.0999, 0.1, 0.0]]], F)
  p, c = R.level0(img, w, conf_min=0.1)
  assert np.array_equal(c, F([[[0.25, 0, 0.1, 0]]]))
  assert np.array_equal(p[..., 0], F([[[0.125, 0, F(0.5) * F(0.1), 0]]]))
  p, c = R.level0(img, w, conf_min=0.0)
  assert np.array_equal(c, w)
  # SPLAT: the share (w - bg_wt) / w is what is compared
  wts = np.array([[[2.0, 1.05, 1.0, 0.5]]], F)
  p, c = R.level0(img, wts, R.SPLAT, conf_min=0.1, bg_wt=1.0)
  assert np.array_equal(c, F([[[0.5, 0, 0, 0]]]))
  assert np.array_equal(p[..., 0], F([[[0.0, 0, 0, 0]]]))    # 0.5 - (1 - 0.5) 1
  # and a thresholded pixel takes its neighbours' colour like any other hole
  img[0, 0, 1] = 100.0
  assert np.abs(R.fill(img, w, conf_min=0.1) - 0.5).max() <= 1e-6


# --- camera paths ---------------------------------------------------------------------
def cameras(rs, b=2, identity=False):
  from lsi.geometry import trajectory as T
  k = lambda: np.array([[100 + 10 * rs.rand(), 0, 48 + rs.rand()],
                        [0, 100 + 10 * rs.rand(), 32 + rs.rand()], [0, 0, 1]], F)
  k_s, k_t = np.stack([k() for _ in range(b)]), np.stack([k() for _ in range(b)])
  rot = []
  for _ in range(b):
    axis = rs.randn(3)
    rot.append(np.eye(3) if identity else T.rotation(axis / np.linalg.norm(axis), 0.3 * rs.rand()))
  return k_s, k_t, np.stack(rot).astype(F), rs.randn(b, 3, 1).astype(F)


def test_interpolate_cameras_end_points():
  from lsi.geometry import trajectory as T
  k_s, k_t, rot, t = cameras(np.random.RandomState(7))
  k, r, tt = T.interpolate_cameras(torch.from_numpy(k_s), k_t, rot, torch.from_numpy(t),
                                   [0.0, 1.0, 0.5, -0.5])
  assert k.dtype == r.dtype == tt.dtype == torch.float32
  assert tuple(k.shape) == (4, 2, 3, 3) and tuple(r.shape) == (4, 2, 3, 3)
  assert tuple(tt.shape) == (4, 2, 3, 1)
  # s = 0: the source camera, the identity pose
  assert np.array_equal(k[0].numpy(), k_s)
  assert np.array_equal(r[0].numpy(), np.broadcast_to(np.eye(3, dtype=F), (2, 3, 3)))
  assert (tt[0].numpy() == 0).all()
  # s = 1: the inputs, bit for bit
  for got, want in ((k[1], k_t), (r[1], rot), (tt[1], t)):
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
  assert np.allclose(k[2].numpy(), 0.5 * (k_s + k_t), atol=1e-5)
  assert np.allclose(tt[3].numpy(), -0.5 * t, atol=1e-6)
  # a scalar s
  assert tuple(T.interpolate_cameras(k_s, k_t, rot, t, 0.25)[1].shape) == (1, 2, 3, 3)
  with pytest.raises(ValueError):
    T.interpolate_cameras(k_s, k_t, rot, t[:, :, 0], [0.5])


@pytest.mark.parametrize('s', [0.0, 0.25, 0.5, 1.5, -0.5])
def test_rotations_compose_along_the_path(s):
  from lsi.geometry import trajectory as T
  k_s, k_t, rot, t = cameras(np.random.RandomState(8), b=3)
  _, r, _ = T.interpolate_cameras(k_s, k_t, rot, t, [s, 1.0 - s])
  prod = np.matmul(r[0].numpy().astype(np.float64), r[1].numpy().astype(np.float64))
  assert np.abs(prod - rot).max() <= 1e-6
  for m in r[0].numpy().astype(np.float64):
    assert np.abs(np.matmul(m, m.T) - np.eye(3)).max() <= 1e-6 and np.linalg.det(m) > 0.999


def test_identity_rotation_is_exact_and_half_turns_work():
  from lsi.geometry import trajectory as T
  k_s, k_t, rot, t = cameras(np.random.RandomState(9), identity=True)
  _, r, _ = T.interpolate_cameras(k_s, k_t, rot, t, [-0.5, 0.0, 0.3, 1.0, 1.5])
  assert np.array_equal(r.numpy(), np.broadcast_to(np.eye(3, dtype=F), (5, 2, 3, 3)))
  # a rotation by pi: the axis comes from the symmetric part
  half = T.rotation(np.array([0.6, 0.0, 0.8]), np.pi)
  axis, angle = T.axis_angle(half)
  assert abs(angle - np.pi) < 1e-9 and np.abs(np.abs(axis) - [0.6, 0.0, 0.8]).max() < 1e-9
  assert np.abs(np.matmul(T.rotation(axis, 0.5 * angle), T.rotation(axis, 0.5 * angle)) -
                half).max() < 1e-9


# --- refusals that need no device ---------------------------------------------------
def test_fill_holes_refuses_before_it_looks_for_a_device(built_lib):
  from lsi.geometry import fill
  img, conf = torch.rand(1, 8, 8, 3), torch.rand(1, 8, 8)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    fill.fill_holes(img, conf)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    fill.fill_splat_holes(img[None], conf[None, ..., None], 1e-3, 0.4, 50.)
  with pytest.raises(RuntimeError, match='contiguous'):
    fill.fill_holes(torch.rand(1, 8, 3, 8).permute(0, 1, 3, 2), conf)
  with pytest.raises(RuntimeError, match='contiguous'):
    fill.fill_holes(img, torch.rand(1, 8, 16)[:, :, ::2])
  with pytest.raises(RuntimeError, match='C in 1 .. 4'):
    fill.fill_holes(torch.rand(1, 8, 8, 5), conf)
  with pytest.raises(RuntimeError, match='fp32'):
    fill.fill_holes(img.double(), conf)
  with pytest.raises(RuntimeError, match='N x H x W'):
    fill.fill_holes(img, torch.rand(1, 8, 7))
  with pytest.raises(TypeError):
    fill.fill_holes(img.numpy(), conf)


def test_library_refuses_shapes_before_any_launch(built_lib):
  """Host answers of the two entry points: no pointer is touched."""
  from lsi import _C
  lib = _C.lib()
  one = 64                                         # non-NULL, never dereferenced
  call = lambda n, h, w, c, ptrs=(one, one, one, one), mode=0, bg_wt=0., bg=1., cm=1e-3, nb=1 << 40: \
      lib.lsi_fill_holes(n, h, w, c, ptrs[0], ptrs[1], mode, bg_wt, bg, cm, ptrs[2], ptrs[3], nb, None)
  size = lib.lsi_fill_holes_workspace_bytes
  for dims in ((0, 8, 8, 3), (65536, 8, 8, 3), (1, 0, 8, 3), (1, 8, -1, 3), (1, 8, 8, 0),
               (1, 8, 8, 5), (1, 2048, 2048, 3), (1, 32, 32 * 2561, 1), (4, 8192, 8193, 1)):
    assert size(*dims) == 0 and call(*dims) == -1, dims
  assert call(1, 8, 8, 3, mode=2) == -1 and call(1, 8, 8, 3, cm=-1.0) == -1
  assert call(1, 8, 8, 3, bg=float('inf')) == -1 and call(1, 8, 8, 3, cm=float('nan')) == -1
  assert call(1, 8, 8, 3, mode=1, bg_wt=-1.0) == -1
  # what is taken: the limit holds 1024 x 1024 and more
  for dims in ((1, 1, 1, 1), (1, 1024, 1024, 4), (2, 1024, 1536, 3), (8, 256, 768, 3)):
    assert size(*dims) >= 16, dims
    for miss in range(4):
      assert call(*dims, ptrs=[None if k == miss else one for k in range(4)]) == -2, (dims, miss)
    assert call(*dims, nb=size(*dims) - 1) == -3, dims
  # the pushed levels 1 .. 5 and F_5: 8 x 256 x 768 x 3
  lv = [(256 >> l) * (768 >> l) for l in range(1, 6)]
  assert size(8, 256, 768, 3) == 8 * 4 * (4 * sum(lv) + 3 * lv[-1])
  assert size(1, 1, 1, 1) == 16


# --- the op route on the host -----------------------------------------------------------
@pytest.mark.parametrize('mode', ['conf', 'splat'])
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (1, 1, 7, 3), (2, 5, 3, 4), (2, 33, 65, 3)])
def test_ops_statement_agrees_with_the_restatement(built_lib, shape, mode):
  from lsi.geometry import fill
  rs = np.random.RandomState(10)
  img = rand_img(rs, *shape)
  conf = (rs.rand(*shape[:3]) * (rs.rand(*shape[:3]) > 0.5)).astype(F)
  if mode == 'conf':
    img[conf == 0] = np.nan
    want = R.fill(img, conf, conf_min=0.05, bg_value=0.75)
    got = fill.fill_holes_ops(torch.from_numpy(img), torch.from_numpy(conf), conf_min=0.05,
                              bg_value=0.75)
  else:
    img, wts = R.splat_canvas(img, conf, 1e-6, scale=2.0)
    want = R.fill(img, wts, R.SPLAT, bg_wt=1e-6)
    got = fill.fill_holes_ops(torch.from_numpy(img), torch.from_numpy(wts)[..., None],
                              mode='splat', bg_wt=1e-6)
  assert got.dtype == torch.float32 and np.abs(got.numpy() - want).max() <= 1e-6
