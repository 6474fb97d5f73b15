"""tests/sampling_ref.py, the fp64 restatement that test_sampling_exact_gpu.py
holds the sampling kernels to, pinned on the CPU: its values to the oracle
(oracle/lsi_oracle.py, fp32), its closed-form gradients to fp64 autograd of the
torch restatement (oracle/lsi_torch_ref.py), both by exact equality -- every
case is on the quarter lattice (or built from powers of two), where each
product and sum is exact in fp32 and fp64 alike.  Every case also proves what
it says about itself (how many points touch the border, lie outside, sit on a
pixel's edge, collide, get clamped), measured with the restatement alone.

Neither reference defines a non-finite coordinate for every operation
(lsi_oracle.bilinear_taps and the torch code index with it): there the
comparison moves such points far outside the image, looks at the finite points
of the per-point results, and at all of the image / source gradients, which a
point far outside and a non-finite one both leave alone."""
import numpy as np
import pytest
import torch

import lsi_oracle as O
import lsi_torch_ref as TR
import sampling_ref as R

ALL = list(R.SHAPES)
FAR = -100.0      # wholly outside every image here, on the lattice


def _f32(a):
  return np.asarray(a, np.float32)


def _finite_coords(cs):
  co = cs.coords.copy()
  co[~R.finite_points(cs)] = FAR
  return co


def _eq(name, got, want, where=None):
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape, (name, got.shape, want.shape)
  if where is not None:
    where = np.broadcast_to(where, got.shape)
    got, want = got[where], want[where]
  bad = np.flatnonzero(got != want)
  assert bad.size == 0, '%s: %d of %d differ, first got %r want %r' % (
      name, bad.size, got.size, got.flat[bad[0]], want.flat[bad[0]])


@pytest.mark.parametrize('name', ALL)
def test_values_equal_the_oracle(name):
  cs, r = R.case(name), R.expected(name, 'float32')
  fin = R.finite_points(cs)
  img, vals, co = _f32(cs.img), _f32(cs.vals), _f32(cs.coords)
  _eq('bilinear', _f32(r['bilinear']), O.bilinear(img, co))
  _eq('splat', _f32(r['splat']), O.splat(vals, co, img))
  ims, wts = O.bilinear_taps(img, _f32(_finite_coords(cs)))
  _eq('taps', _f32(r['taps']), np.stack(ims), fin[None, ..., None])
  _eq('wts', _f32(r['wts']), np.stack(wts), fin[None, ..., None])
  # the non-finite points sample nothing
  assert not r['taps'][:, ~fin].any() and not r['bilinear'][~fin].any()
  assert np.isfinite(r['wts'][:, fin]).all()


@pytest.mark.parametrize('name', list(R.SCATTER))
def test_scatter_add_equals_the_oracle(name):
  (init, idx, upd, g), (out, g_init, g_upd) = R.scatter_case(name)
  _eq('out', _f32(out), O.batch_scatter_add_tensor(init, idx, upd))
  _eq('row 1', _f32(out[1]), O.scatter_add_tensor(init[1], idx[1][:, None], upd[1]))
  ti = torch.tensor(init, requires_grad=True)
  tu = torch.tensor(upd, requires_grad=True)
  got = ti.scatter_add(1, torch.tensor(idx, dtype=torch.int64), tu)
  _eq('out, torch', out, got.detach().numpy())
  got.backward(torch.tensor(g))
  _eq('g_init', g_init, ti.grad.numpy())
  _eq('g_upd', g_upd, tu.grad.numpy())
  assert np.abs(out).max() < 2 ** 20 and (out == np.round(out)).all()
  sh = R.SCATTER[name]
  assert idx.shape == (R.SCATTER_B, sh.n) and init.shape == (R.SCATTER_B, sh.p)
  if sh.one:     # the collision case: every update of a row goes to one place
    assert sh.n == 700 and all(len(set(row)) == 1 for row in idx.tolist())
    assert (np.abs(out - init).sum(1) == np.abs(upd.sum(1))).all()


@pytest.mark.parametrize('name', ALL)
def test_gradients_equal_fp64_autograd(name):
  cs, r = R.case(name), R.expected(name, 'float64')
  fin = R.finite_points(cs)[..., None]
  T = lambda a: torch.tensor(np.asarray(a, np.float64))
  leaf = lambda a: T(a).requires_grad_(True)
  co = _finite_coords(cs)

  i64, c64 = leaf(cs.img), leaf(co)
  out = TR.bilinear(i64, c64)
  _eq('bilinear', r['bilinear'], out.detach().numpy(), fin)
  out.backward(T(cs.g_vals))
  _eq('bilinear g_imgs', r['bilinear_g_imgs'], i64.grad.numpy())
  _eq('bilinear g_coords', r['bilinear_g_coords'], c64.grad.numpy(), fin)

  for tag in ('t', 'w', 'tw'):
    i64, c64 = leaf(cs.img), leaf(co)
    ims, wts = TR.bilinear_taps(i64, c64)
    loss = 0
    if 't' in tag:
      loss = loss + sum((a * T(g)).sum() for a, g in zip(ims, cs.g_taps))
    if 'w' in tag:
      loss = loss + sum((a * T(g)).sum() for a, g in zip(wts, cs.g_wts))
    gi, gc = torch.autograd.grad(loss, [i64, c64], allow_unused=True)
    # (the taps do not depend on the coordinates, nor the weights on the image)
    gi = np.zeros(cs.img.shape) if gi is None else gi.numpy()
    gc = np.zeros(co.shape) if gc is None else gc.numpy()
    _eq('taps g_imgs ' + tag, r['taps_g_imgs_' + tag], gi)
    _eq('taps g_coords ' + tag, r['taps_g_coords_' + tag], gc, fin)

  s64, c64, n64 = leaf(cs.vals), leaf(co), leaf(cs.img)
  out = TR.splat(s64, c64, n64)
  _eq('splat', r['splat'], out.detach().numpy())
  out.backward(T(cs.g_img))
  _eq('splat g_src', r['splat_g_src'], s64.grad.numpy(), fin)
  _eq('splat g_coords', r['splat_g_coords'], c64.grad.numpy(), fin)
  _eq('splat g_init', r['splat_g_init'], n64.grad.numpy())

  # a non-finite point: zero gradients of its own
  for key in ('bilinear_g_coords', 'taps_g_coords_tw', 'splat_g_coords', 'splat_g_src'):
    assert not r[key][~fin[..., 0]].any(), key


@pytest.mark.parametrize('name', ALL)
def test_the_device_answer_is_determined_to_the_last_bit(name):
  """Every result is a multiple of 1/16 below 2^16 (2^20 sixteenths): fp32 holds
  it, and every partial sum on the way to it, exactly, in any order.  The clamp
  case is built from 2^-10: multiples of 2^-10 below 2^13."""
  scale, bound = (16.0, 2.0 ** 20) if name in R.EXACT16 else (2.0 ** 10, 2.0 ** 23)
  for dtype in ('float32', 'float64'):
    for key, a in R.expected(name, dtype).items():
      a = a[np.isfinite(a)] * scale          # (the undefined weights are NaN)
      assert (a == np.round(a)).all(), (key, dtype)
      assert np.abs(a).max(initial=0) < bound, (key, dtype, np.abs(a).max())
      if key != 'wts':
        assert a.size == R.expected(name, dtype)[key].size, key
  cs = R.case(name)
  for a in (cs.img, cs.vals, cs.coords, cs.g_img, cs.g_vals, cs.g_taps, cs.g_wts):
    assert np.array_equal(_f32(a).astype(np.float64), a, equal_nan=True)
  # no partial sum of an accumulation leaves fp32 either: bounded by the sum of
  # the magnitudes of everything one batch item can add to one place
  for most in (np.abs(cs.vals).sum((1, 2)), np.abs(cs.g_vals).sum((1, 2)),
               np.abs(cs.g_taps).sum((0, 2, 3))):
    assert scale * (most.max() + 8) < 2.0 ** 24


@pytest.mark.parametrize('name', ALL)
def test_cases_are_what_they_claim(name):
  cs = R.case(name)
  sh = cs.shape
  d = R.describe(cs.coords, *sh.img)
  assert d['points'] == sh.pts[0] * sh.pts[1]
  fin = R.finite_points(cs)
  if sh.kind in ('lattice', 'hostile'):
    q = cs.coords[fin & (np.abs(cs.coords) < 1e8).all(-1)] * 4
    assert (q == np.round(q)).all()
    assert q[:, 0].min() >= -8 and q[:, 0].max() <= 4 * (sh.img[1] + 2)
    assert q[:, 1].min() >= -8 and q[:, 1].max() <= 4 * (sh.img[0] + 2)
    if sh.b * d['points'] >= 255:
      assert d['border'] >= 0.10 and d['outside'] >= 0.05, d
      assert d['on_border'] > 0 and d['on_centre'] > 0, d
      for i in range(1, sh.b):      # items are drawn independently
        assert not np.array_equal(cs.coords[0], cs.coords[i])
  if sh.kind == 'lattice':
    assert d['nonfinite'] == 0
  if sh.kind == 'hostile':
    flat = cs.coords.reshape(-1, 2)
    with np.errstate(invalid='ignore'):
      hostile = ~np.isfinite(flat) | (np.abs(flat) >= 1e9)
    assert hostile.any(1).sum() >= R.HOSTILE_SHARE * len(flat)
    assert hostile.any(1).sum() < 0.2 * len(flat)
    assert hostile.all(1).any() and (hostile[:, 0] & ~hostile[:, 1]).any()
    assert (hostile[:, 1] & ~hostile[:, 0]).any()
    for axis in (0, 1):
      col = flat[:, axis]
      assert np.isnan(col).any()
      for v in R.HOSTILE_VALUES[1:]:
        assert (col == np.float32(v)).any(), (axis, v)
    assert d['nonfinite'] > 0
  if sh.kind in ('centre', 'corner'):
    assert d['points'] == 2000 and d['distinct'] == 1 and sh.b == 1
    one = R.splat(np.ones((1, 1, 1, 1)), cs.coords[:, :1, :1], np.zeros((1,) + sh.img + (1,)))
    hit = one[one != 0]
    if sh.kind == 'centre':
      assert hit.tolist() == [1.0]
    else:
      assert hit.tolist() == [0.25] * 4
  if sh.kind == 'clamp':
    assert d['clamped'] > 0 and d['kept_small'] > 0, d
    # ... from either side, on either axis, and some of each at the border
    frac = cs.coords - np.floor(cs.coords)
    for axis in (0, 1):
      got = set(np.unique(frac[..., axis]).tolist())
      assert got == {0.5, 0.5 + 2.0 ** -10, 0.5 + 2.0 ** -9, 0.5 - 2.0 ** -10,
                     0.5 - 2.0 ** -9}, got
    assert d['border'] > 0
    # a dropped corner adds nothing, a kept one all of it: one point, by hand
    for f, want in ((2.0 ** -10, [1 - 2.0 ** -10]), (2.0 ** -9, [1 - 2.0 ** -9, 2.0 ** -9])):
      co = np.array([[[[2.5 + f, 1.5]]]])
      one = R.splat(np.ones((1, 1, 1, 1)), co, np.zeros((1, 4, 6, 1)))
      assert one[0, 1, 2:4, 0].tolist() == (want + [0.0])[:2] and one.sum() == sum(want)
      g_src, g_co, _ = R.splat_grad(np.ones((1, 1, 1, 1)), co, np.ones((1, 4, 6, 1)))
      assert g_src.item() == sum(want)
      assert g_co[0, 0, 0].tolist() == [-1.0 + len(want) - 1, -sum(want)]


def test_the_cases_cover_the_shapes():
  sh = [s for s in R.SHAPES.values() if s.kind == 'lattice']
  assert {s.pts[0] * s.pts[1] for s in sh} == {1, 255, 256, 257, 513}
  assert {s.img for s in sh} == {(1, 1), (1, 7), (9, 1), (9, 13)}
  assert {s.c for s in sh} == {1, 3, 5} and {s.b for s in sh} >= {1, 3}
  assert R.SHAPES[R.STRIDES].b == 3
  assert {(s.n, s.p) for s in R.SCATTER.values()} == {
      (n, p) for n in (1, 257, 700) for p in (1, 5)}


def test_arbitrary_coordinates():
  """Off the lattice nothing is exact: fp64 autograd within 1e-12, the fp32
  oracle within its own rounding -- at most four terms of four products of
  values below 1 each, 16 roundings of 2^-24: 1e-6 -- per output, and per
  unit weight of what collects on a canvas pixel (a few dozen points)."""
  rs = np.random.RandomState(77)
  b, h, w, c, hp, wp = 2, 9, 13, 3, 19, 27
  img, vals = rs.rand(b, h, w, c), rs.rand(b, hp, wp, c)
  co = np.stack([rs.uniform(-2, w + 2, (b, hp, wp)),
                 rs.uniform(-2, h + 2, (b, hp, wp))], -1)
  co = co.astype(np.float32).astype(np.float64)
  g_vals, g_img = rs.rand(b, hp, wp, c), rs.rand(b, h, w, c)
  near = lambda name, got, want, tol: np.testing.assert_allclose(
      got, want, rtol=tol, atol=tol, err_msg=name)
  f = _f32
  near('bilinear', R.bilinear(f(img), f(co)), O.bilinear(f(img), f(co)), 1e-6)
  near('splat', R.splat(f(vals), f(co), f(img)), O.splat(f(vals), f(co), f(img)), 4e-5)
  taps, wts = R.bilinear_taps(f(img), f(co))
  ims_o, wts_o = O.bilinear_taps(f(img), f(co))
  _eq('taps', f(taps), np.stack(ims_o))
  near('wts', wts, np.stack(wts_o), 1e-6)
  T = lambda a: torch.tensor(a, requires_grad=True)
  i64, c64, s64, n64 = T(img), T(co), T(vals), T(img)
  out = TR.bilinear(i64, c64)
  near('bilinear, fp64', R.bilinear(img, co), out.detach().numpy(), 1e-12)
  out.backward(torch.tensor(g_vals))
  gi, gc = R.bilinear_grad(img, co, g_vals)
  near('bilinear g_imgs', gi, i64.grad.numpy(), 1e-12)
  near('bilinear g_coords', gc, c64.grad.numpy(), 1e-12)
  out = TR.splat(s64, T(co), n64)
  near('splat, fp64', R.splat(vals, co, img), out.detach().numpy(), 1e-12)
  c64 = T(co)
  TR.splat(s64, c64, n64).backward(torch.tensor(g_img))
  gs, gc, gn = R.splat_grad(vals, co, g_img)
  near('splat g_src', gs, s64.grad.numpy(), 1e-12)
  near('splat g_coords', gc, c64.grad.numpy(), 1e-12)
  near('splat g_init', gn, n64.grad.numpy(), 0)


def test_a_nonfinite_point_changes_nothing_else():
  """The hostile case against the same case with its non-finite points moved
  far outside: identical everywhere but in the undefined weights."""
  name, = R.HOSTILE
  cs = R.case(name)
  fin = R.finite_points(cs)
  r = R.expected(name, 'float32')
  co = _f32(_finite_coords(cs))
  _eq('bilinear', r['bilinear'], R.bilinear(cs.img, co))
  _eq('splat', r['splat'], R.splat(cs.vals, co, cs.img))
  taps, wts = R.bilinear_taps(cs.img, co)
  _eq('taps', r['taps'], taps)
  _eq('wts', r['wts'], wts, fin[None, ..., None])
  gi, gc = R.bilinear_grad(cs.img, co, cs.g_vals)
  _eq('g_imgs', r['bilinear_g_imgs'], gi)
  _eq('g_coords', r['bilinear_g_coords'], gc)   # far outside: zero as well
  gi, gc = R.bilinear_taps_grad(cs.img.shape, co, cs.g_taps, cs.g_wts)
  _eq('taps g_imgs', r['taps_g_imgs_tw'], gi)
  _eq('taps g_coords', r['taps_g_coords_tw'], gc, fin[..., None])
  gs, gc, _ = R.splat_grad(cs.vals, co, cs.g_img)
  _eq('splat g_src', r['splat_g_src'], gs)
  _eq('splat g_coords', r['splat_g_coords'], gc)
