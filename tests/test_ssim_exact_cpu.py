"""tests/ssim_exact_ref.py -- the float32 restatement that the SSIM kernels are
held to with `==` (tests/test_ssim_exact_gpu.py) -- is the definition: against the
fp64 op restatement of tests/ssim_ref.py under the bars of tests/test_ssim_gpu.py,
against anchors worked by hand, and the tile and stride arithmetic of every case
is what the case claims.  No GPU.

Bars (those of tests/test_ssim_gpu.py, with the fp32 op restatement's own error
measured on the same inputs): loss |l - l64| <= max(4 x |l32 - l64|, 2e-6 |l64|);
gradient max |g - g64| <= max(4 x max |g32 - g64|, 1e-5 max |g64|); d per window
and layer max |d - d64| <= max(4 x max |d32 - d64|, 2e-6 max |d64|) -- the loss's
bar, one window at a time.  Loss and gradient are compared where the fp64
restatement's best and second-best layer are >= MIN_GAP apart in every window
(otherwise fp64 may choose another layer: then d alone is compared, per layer)."""
import functools

import numpy as np
import pytest
import torch

import ssim_exact_ref as X
import ssim_ref

F = np.float32
LOSS_RTOL, GRAD_RTOL, SLACK = 2e-6, 1e-5, 4.0     # tests/test_ssim_gpu.py
MIN_GAP = 1e-4

# the cases whose fp64 gap is >= MIN_GAP: loss and gradient are compared there
# (a condition on the inputs, their seeds found on the CPU).  The others hold
# ties on purpose; stride_single's 2049 windows of 9 pixels have no seed with
# every gap that wide.
GAPPED = set(X.CASES) - set(X.TIE_CASES) - {'stride_single'}


@functools.lru_cache(maxsize=None)
def fp64(name):
  """Loss, gradient and d of the op restatement in fp64 and in fp32."""
  case = X.CASES[name]
  recons, target = (torch.from_numpy(a.copy()) for a in X.inputs(name))
  args = (case.x_min, case.y_min, case.win, case.sigma)
  out = {}
  for dt in (torch.float64, torch.float32):
    r = recons.to(dt).clone().requires_grad_(True)
    l = ssim_ref.loss(r, target.to(dt), *args)
    (l * case.upstream).backward()
    d = ssim_ref.dssim_maps(recons.to(dt), target.to(dt), *args)
    out[dt] = (float(l.detach()), r.grad.double().numpy(), d.double().numpy())
  gap = ssim_ref.best_gap(recons.double(), target.double(), *args)
  return {'64': out[torch.float64], '32': out[torch.float32], 'gap': gap}


def restated_loss(r):
  """The float the device returns if its fp64 sum were exact."""
  lo, hi = X.interval(r['loss_partials'], r['windows'])
  ends = X.float32_ends(lo, hi)
  return sorted(ends)[0], ends


@pytest.mark.parametrize('name', list(X.CASES))
def test_conditions_under_which_equality_is_owed(name):
  r = X.restated(name)
  w = r['watch']
  print('ssim exact %s: smallest non-zero intermediate %.3g, finite %s' %
        (name, w.min_nonzero, w.finite))
  assert w.finite
  assert w.min_nonzero >= X.TINY          # no subnormal anywhere
  # the (m + 1) 2^-53 bound of the fp64 sums needs partial sums of one sign
  assert X.same_sign(r['loss_partials']) and X.same_sign(r['metric_partials'])
  assert np.isfinite(r['grad']).all()
  case = X.CASES[name]
  inside = np.zeros(r['grad'].shape[2:4], bool)
  inside[case.y_min:case.ht - case.y_min, case.x_min:case.wt - case.x_min] = True
  assert (r['grad'][:, :, ~inside] == 0).all()
  assert r['loss_partials'].size == r['metric_partials'].size
  # the interval of the fp64 sum rounds to a single float in every case here
  # (two would be legitimate; the device test admits either end)
  _, ends = restated_loss(r)
  assert len(ends) == 1


@pytest.mark.parametrize('name', list(X.CASES))
def test_restatement_against_the_fp64_definition(name):
  r, ref = X.restated(name), fp64(name)
  l64, g64, d64 = ref['64']
  l32, g32, d32 = ref['32']
  d_err, d_err32 = np.abs(r['d'] - d64).max(), np.abs(d32 - d64).max()
  d_bar = max(SLACK * d_err32, LOSS_RTOL * np.abs(d64).max())
  print('ssim exact %s: gap %.3g | d err restatement %.3g op fp32 %.3g bar %.3g' %
        (name, ref['gap'], d_err, d_err32, d_bar))
  assert d_err <= d_bar
  assert (ref['gap'] >= MIN_GAP) == (name in GAPPED), ref['gap']
  if name not in GAPPED:
    return
  l, _ = restated_loss(r)
  l_err, l_bar = abs(l - l64), max(SLACK * abs(l32 - l64), LOSS_RTOL * abs(l64))
  scale = np.abs(g64).max()
  g_err = np.abs(r['grad'] - g64).max() / scale
  g_bar = max(SLACK * np.abs(g32 - g64).max() / scale, GRAD_RTOL)
  print('ssim exact %s: loss err %.3g (relative %.3g) bar %.3g | grad err %.3g op fp32 '
        '%.3g bar %.3g' % (name, l_err, l_err / abs(l64), l_bar, g_err,
                           np.abs(g32 - g64).max() / scale, g_bar))
  assert l_err <= l_bar
  assert g_err <= g_bar
  # the metric: the same sum of layer 0's mean SSIM
  case = X.CASES[name]
  recons, target = (torch.from_numpy(a.copy()) for a in X.inputs(name))
  args = (case.x_min, case.y_min, case.win, case.sigma)
  s64, n64 = ssim_ref.metric(recons.double(), target.double(), *args)
  s32, _ = ssim_ref.metric(recons, target, *args)
  s = float(r['metric_partials'].astype(np.float64).sum())
  print('ssim exact %s: metric sum err %.3g op fp32 %.3g' %
        (name, abs(s - s64) / abs(s64), abs(s32 - s64) / abs(s64)))
  assert n64 == r['windows']
  assert abs(s - s64) <= max(SLACK * abs(s32 - s64), LOSS_RTOL * abs(s64))


@pytest.mark.parametrize('name', X.TIE_CASES)
def test_tie_cases_hold_ties(name):
  r = X.restated(name)
  tied = int((r['ties'] > 1).sum())
  two = np.sort(r['d'], axis=0)[:2]
  ulps = X.ulps_apart(two[0], two[1])
  near = int(((ulps >= 1) & (ulps <= 16)).sum())
  print('ssim exact %s: %d of %d windows tied (%d three ways), %d with the two best '
        'layers 1 .. 16 ulps apart' % (name, tied, r['ties'].size,
                                       int((r['ties'] > 2).sum()), near))
  assert tied > 0
  # near ties are built into `ties` alone (layer 1 one ulp from layer 0); the
  # value cases tie exactly or not at all, so only `tied` is held for them
  if name == 'ties':
    assert near > 0 and int((r['ties'] == 3).sum()) > 0 and int((r['ties'] == 2).sum()) > 0
    # windows of all three kinds receive gradient in the layers at the minimum
    assert (np.abs(r['grad']).reshape(3, -1).max(axis=1) > 0).all()


# ---------------------------------------------------------------------------
# anchors that can be checked by hand
# ---------------------------------------------------------------------------
def _rng_images(seed, b, ht, wt, f):
  rs = np.random.RandomState(seed)
  return rs.rand(b, ht * f, wt * f, 3).astype(F)


@pytest.mark.parametrize('f', [1, 2])
def test_identical_images_score_zero_exactly(f):
  target = _rng_images(2, 2, 14, 19, f)
  t = X.area(target, 14, 19, X.Watch())
  r = X.restate(t[None], target, 1, 2, 5, 1.5)
  # numerator and denominator have the same bits
  assert (r['d'] == 0.0).all() and (r['s_mean'] == 1.0).all()
  assert float(X.interval(r['loss_partials'], r['windows'])[1]) == 0.0
  # ... so the partial sums are whole numbers and their fp64 sum is exact
  assert float(r['metric_partials'].astype(np.float64).sum()) == r['windows']
  lo, hi = X.interval(r['metric_partials'])
  assert lo <= r['windows'] <= hi
  # the gradient at the minimum: zero at the gradient's usual bar, 1e-5 of the
  # largest entry these images have 0.05 away from it -- not exactly zero
  rs = np.random.RandomState(3)
  off = X.restate((t + rs.uniform(-0.05, 0.05, t.shape)).astype(F)[None], target, 1, 2, 5,
                  1.5)
  print('ssim exact identical f=%d: largest |gradient| %.3g (%.3g with noise of 0.05)' %
        (f, np.abs(r['grad']).max(), np.abs(off['grad']).max()))
  assert np.abs(r['grad']).max() <= GRAD_RTOL * np.abs(off['grad']).max()


def test_black_images_score_zero_exactly():
  r = X.restated('values_black')
  assert (r['d'] == 0.0).all() and (r['ties'] == 2).all()
  assert (r['loss_partials'] == 0.0).all()
  assert float(r['metric_partials'].astype(np.float64).sum()) == r['windows']
  assert r['windows'] == 2 * 22 * 39
  assert (r['grad'] == 0.0).all()                # A = 0 and x = y = 0


def test_a_layer_that_loses_everywhere_has_no_gradient():
  rs = np.random.RandomState(5)
  target = _rng_images(5, 1, 12, 17, 1)
  good = (target + rs.uniform(-0.02, 0.02, target.shape)).astype(F)
  bad = (target + rs.uniform(-0.3, 0.3, target.shape)).astype(F)
  r = X.restate(np.stack([bad, good]), target, 1, 1, 3, 0.0)
  assert (r['d'][0] > r['d'][1]).all() and (r['ties'] == 1).all()
  assert (r['grad'][0] == 0.0).all() and np.abs(r['grad'][1]).max() > 0
  alone = X.restate(good[None], target, 1, 1, 3, 0.0)
  assert np.array_equal(r['grad'][1], alone['grad'][0])


def test_tied_layers_share_the_gradient():
  rs = np.random.RandomState(6)
  target = _rng_images(6, 2, 13, 16, 1)
  x = (target + rs.uniform(-0.05, 0.05, target.shape)).astype(F)
  one = X.restate(x[None], target, 0, 1, 7, 1.5)
  two = X.restate(np.stack([x, x]), target, 0, 1, 7, 1.5)
  assert (two['ties'] == 2).all()
  # halving is exact: every product and sum of the gradient scales with it
  assert np.array_equal(two['grad'][0], two['grad'][1])
  assert np.array_equal(two['grad'][0] * F(2), one['grad'][0])
  three = X.restate(np.stack([x, x, x]), target, 0, 1, 7, 1.5)
  assert (three['ties'] == 3).all()
  assert np.array_equal(three['grad'][0], three['grad'][1])
  assert np.array_equal(three['grad'][0], three['grad'][2])
  # 1/3 is not exact: up = (gs / 3) / 6 rounds twice more than gs / 6
  err = np.abs(three['grad'].astype(np.float64).sum(axis=0) - one['grad'][0]).max()
  assert err <= GRAD_RTOL * np.abs(one['grad']).max()
  assert np.array_equal(one['loss_partials'], two['loss_partials'])


def test_one_window_is_its_own_loss():
  for name in ('one_window_n3', 'one_window_n11', 'one_window_n3_crop',
               'one_window_n11_crop'):
    r = X.restated(name)
    assert r['windows'] == 1 and r['d'].shape == (1, 1, 1, 1)
    assert X.float32_ends(*X.interval(r['loss_partials'], 1)) == {float(r['d'].ravel()[0])}
    # one non-zero partial sum: the fp64 sums are exact, the metric is S widened
    assert int((r['loss_partials'] != 0).sum()) == 1
    assert r['metric_partials'][0, 0] == r['s_mean'].ravel()[0]
    assert int((r['metric_partials'] != 0).sum()) == 1


def test_per_thread_sums_follow_the_tile_assignment():
  """Windows numbered by powers of two small enough for exact fp32 sums: the
  partial sum of block g, thread t is the sum over its windows, by hand."""
  b, hv, wv = 3, 18, 35
  vals = np.arange(b * hv * wv, dtype=F).reshape(b, hv, wv)     # < 2^24: exact
  got = X.thread_partials(vals, X.Watch())
  assert got.shape == (12, 256)
  want = np.zeros((12, 256), np.float64)
  for i in range(b):
    for v in range(hv):
      for u in range(wv):
        tile = (i * 2 + v // 16) * 2 + u // 32
        want[tile, ((v % 16) * 32 + u % 32) % 256] += vals[i, v, u]
  assert np.array_equal(got, want)
  # past MAXBLK tiles: block 0 adds tile 2048 to tile 0
  vals = np.arange(2049, dtype=F).reshape(2049, 1, 1)
  got = X.thread_partials(vals, X.Watch())
  assert got.shape == (2048, 256) and got[0, 0] == 2048 and got[1, 0] == 1
  assert got[:, 1:].sum() == 0 and got.sum() == 2049 * 2048 / 2


# ---------------------------------------------------------------------------
# the tile and stride arithmetic of each case, from its shapes
# ---------------------------------------------------------------------------
def geo(name):
  c = X.CASES[name]
  return X.geometry(c.nl, c.b, c.ht, c.wt, c.x_min, c.y_min, c.win)


def test_constants_are_the_kernels():
  import os
  from conftest import PKG
  with open(os.path.join(PKG, 'csrc', 'lsi_ssim.hip')) as f:
    src = f.read()
  with open(os.path.join(PKG, 'csrc', 'lsi_reduce.h')) as f:
    red = f.read()
  assert 'using FwdGeo = Geo<%d, %d>;' % (X.FWD_WX, X.FWD_WY) in src
  assert 'constexpr int PX = %d, PY = %d;' % (X.BWD_PX, X.BWD_PY) in src
  assert 'constexpr int MAXBLK = %d;' % X.MAXBLK in red
  assert 'constexpr int TPB = %d;' % X.TPB in red


def test_geometry_of_the_cases():
  g = geo('seams_n11')
  assert (g['Hv'], g['Wv']) == (18, 35)
  assert (g['fwd_ty'], g['fwd_tx'], g['fwd_last']) == (2, 2, (2, 3))   # ragged last
  assert (g['bwd_ty'], g['bwd_tx'], g['bwd_last']) == (4, 2, (6, 15))
  for n in (3, 5, 7, 9, 11):           # every window size crosses tile seams both ways
    for name in ('seams_n%d' % n, 'seams_n%d_box' % n):
      g = geo(name)
      assert g['fwd_ty'] == 2 and g['fwd_tx'] == 2 and g['bwd_tiles'] == 2 * 4 * 2
      assert g['zero_rows'] == [] and g['zero_cols'] == []
      assert X.CASES[name].win == n
  for name in ('one_window_n3', 'one_window_n11', 'one_window_n3_crop',
               'one_window_n11_crop'):
    g = geo(name)
    assert (g['Hv'], g['Wv'], g['fwd_tiles']) == (1, 1, 1)
  # deep_crop: the crop (rows 9 .. 15, columns 33 .. 41) lies inside backward tile
  # (1, 1); every other tile takes the zero branch, rows 0 and 3 and columns 0 and
  # 2 among them
  g = geo('deep_crop')
  c = X.CASES['deep_crop']
  assert c.y_min >= X.BWD_PY and c.x_min >= X.BWD_PX
  assert (g['Hv'], g['Wv']) == (5, 7)
  assert (g['bwd_ty'], g['bwd_tx']) == (4, 3)
  assert g['zero_rows'] == [0, 2, 3] and g['zero_cols'] == [0, 2]
  assert 1 not in g['zero_rows'] and 1 not in g['zero_cols']     # the centre tile
  # crop_5pct: the trainer's rounding of 0.05
  c = X.CASES['crop_5pct']
  assert (ssim_ref.py2_round(c.wt * 0.05), ssim_ref.py2_round(c.ht * 0.05)) == (5, 2)
  # the stride loops: more than MAXBLK tiles in BOTH kernels
  g = geo('stride_single')
  assert g['fwd_tiles'] == g['bwd_tiles'] == 2049 > X.MAXBLK
  assert g['fwd_grid'] == g['bwd_grid'] == X.MAXBLK       # block 0 takes two
  g = geo('stride_multi')
  assert (g['fwd_ty'], g['fwd_tx'], g['bwd_ty'], g['bwd_tx']) == (1, 3, 1, 3)
  assert g['fwd_tiles'] == g['bwd_tiles'] == 2100 > X.MAXBLK
  second = [(t, t + X.MAXBLK) for t in range(2100 - X.MAXBLK)]
  assert len(second) == 52                                 # blocks 0 .. 51
  for first, nxt in second:            # another image and another tile column
    assert first // 3 != nxt // 3 and first % 3 != nxt % 3
  assert g['fwd_last'] == (1, 4) and g['bwd_last'] == (3, 6)
  # the rest: one pass, no zero branch
  for name in X.CASES:
    if not name.startswith(('stride', 'deep')):
      g = geo(name)
      assert g['fwd_tiles'] <= X.MAXBLK and g['bwd_tiles'] <= X.MAXBLK
      assert g['zero_rows'] == [] and g['zero_cols'] == []


def test_every_case_of_the_list_is_present():
  c = X.CASES
  assert {c[n].win for n in c if n.startswith('seams')} == {3, 5, 7, 9, 11}
  assert all(c['seams_n%d_box' % n].sigma == 0.0 and c['seams_n%d' % n].sigma == 1.5
             for n in (3, 5, 7, 9, 11))
  assert {c[n].nl for n in c if n.startswith('layers')} == {1, 5, 8}
  assert {(c[n].fy, c[n].fx) for n in c if n.startswith('factors')} == {(1, 2), (3, 1),
                                                                       (4, 4)}
  assert sum(c[n].chw for n in c) == 1
  assert sorted({c[n].upstream for n in c}) == [1.0 / 3.0, 2.5]
  assert sum(n.startswith('values') for n in c) == 5
  # what the value cases claim about their inputs
  recons, target = X.inputs('values_lattice255')
  k = np.round(target.astype(np.float64) * 255)
  assert np.array_equal(target, (k.astype(F) / F(255)).astype(F)) and len(np.unique(k)) == 256
  recons, _ = X.inputs('values_out_of_range')
  assert recons.min() == F(-0.25) and recons.max() == F(1.25)
  recons, target = X.inputs('values_saturated_patch')
  assert (recons[:, :, 8:20, 16:28] == 1.0).all()
  recons, target = X.inputs('values_constant_patch')
  assert (recons[:, :, 8:20, 16:28] == 0.5).all()
  recons, _ = X.inputs('ties')
  half = 37 // 2
  assert np.array_equal(recons[0, :, :, :half], recons[1, :, :, :half])
  assert np.array_equal(recons[0, :, :, :half], recons[2, :, :, :half])
  moved = X.ulps_apart(recons[0, :, :, half:], recons[1, :, :, half:])
  assert set(np.unique(moved)) == {0, 1}
  assert moved.reshape(-1, 3)[::5].min() == 1 and moved.sum() == 3 * len(moved.reshape(-1, 3)[::5])


# ---------------------------------------------------------------------------
# `==` sees what the float bars cannot
# ---------------------------------------------------------------------------
def _restate_with(monkeypatch, name, passes):
  case = X.CASES[name]
  monkeypatch.setattr(X, '_pass', passes)
  return X.restate(*X.inputs(name), case.x_min, case.y_min, case.win, case.sigma,
                   case.upstream)


def test_equality_sees_the_summation_order_and_one_tap(monkeypatch):
  """The same arithmetic with every pass summed k descending, and with the last
  tap of the back-convolution off by one float32 step: both stay far inside the
  bars of tests/test_ssim_gpu.py and both change the gradient's bits."""
  name = 'seams_n7'
  want, ref = X.restated(name), fp64(name)
  real = X._pass

  def descending(v, g, axis, out_len, watch, flip=False):
    n = len(g)
    s = np.zeros(v.shape[:axis] + (out_len,) + v.shape[axis + 1:], F)
    for k in reversed(range(n)):
      sl = [slice(None)] * v.ndim
      sl[axis] = slice(k, k + out_len)
      s = s + (g[n - 1 - k] if flip else g[k]) * v[tuple(sl)]
    return s

  def one_tap(v, g, axis, out_len, watch, flip=False):
    if flip:
      g = g.copy()
      g[0] = np.nextafter(g[0], F(1))
    return real(v, g, axis, out_len, watch, flip)

  scale = np.abs(ref['64'][1]).max()
  bar = max(SLACK * np.abs(ref['32'][1] - ref['64'][1]).max() / scale, GRAD_RTOL)
  for what, passes in (('descending', descending), ('one tap', one_tap)):
    got = _restate_with(monkeypatch, name, passes)
    changed = int((got['grad'] != want['grad']).sum())
    err = np.abs(got['grad'] - ref['64'][1]).max() / scale
    print('ssim exact %s, %s: %d of %d gradient elements change, error to fp64 %.3g '
          '(bar %.3g)' % (name, what, changed, want['grad'].size, err, bar))
    assert err <= bar                    # the float bar passes it ...
    assert changed > want['grad'].size // 10   # ... equality does not
