"""The LiDAR rasteriser on the device (csrc/lsi_lidar.hip) against
the float32 NumPy restatement tests/lidar_ref.py: every comparison is on the
float32 bits of every element (np.array_equal on the uint32 views).  The
definition fixes the order of every operation and the z-buffer is an exact
minimum, so nothing depends on the order threads arrive in and no tolerance is
needed or given.

The clouds are two fronto-parallel sheets of points with a little depth noise,
spread a tenth of the image beyond its borders, seen through K [I | t]: all
coordinates are ordinary numbers far from the denormals.  One point in twenty
is on the near sheet, so whether a far pixel has a near one in its window -- and
is removed -- depends on the window's exact extent.  The far sheet reaches
past z_max, so the upper bound drops points in every case."""
import functools

import numpy as np
import pytest
import torch

import lidar_ref as R

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 16, 64          # the finishing kernel's LDS tile (lidar.TILE)
Z_MAX = 14.25


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def view_mats(h, w, v=2):
  f = np.float32(w / 2.0)
  out = []
  for j in range(v):
    out.append(np.array([[f, 0, w / 2.0, -0.4 * f * j], [0, f * 1.1, h / 2.0, 0.07 * j],
                         [0.002 * j, 0, 1, 0.01 * j]], np.float32).reshape(12))
  return np.stack(out)


def cloud(seed, n, h, w, near=6.0, far=14.0, share=0.05):
  rs = np.random.RandomState(seed)
  z = np.where(rs.rand(n) < share, near, far) + rs.uniform(0, 0.5, n)
  u = rs.uniform(-0.1 * w, 1.1 * w, n)
  v = rs.uniform(-0.1 * h, 1.1 * h, n)
  f = w / 2.0
  pts = np.stack([(u - w / 2.0) * z / f, (v - h / 2.0) * z / (1.1 * f), z, rs.rand(n)], 1)
  return pts.astype(np.float32)


def run(dev, pts, first, count, mats, h, w, **kw):
  from lsi.geometry import lidar
  out = lidar.rasterize_points(torch.from_numpy(np.array(pts)).to(dev), first, count,
                               torch.from_numpy(np.array(mats)).to(dev), h, w, **kw)
  torch.cuda.synchronize()
  assert out.dtype == torch.float32 and out.is_contiguous()
  return out.cpu().numpy()


def assert_same(got, want, what):
  assert got.shape == want.shape, (what, got.shape, want.shape)
  a, b = got.view(np.uint32), want.view(np.uint32)
  bad = np.argwhere(a != b)
  assert len(bad) == 0, '%s: %d of %d elements differ, first at %s: %r vs %r' % (
      what, len(bad), a.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


# --- 1. ragged batches, depth and inverse --------------------------------------------
@functools.lru_cache(maxsize=None)
def packed_case():
  """B = 3, V = 2 in packed form: scans of 0, 1 and 257 points whose first points
  are at 7, 265 and 3 -- no multiple of the block size -- with NaN rows between
  them that belong to no scan."""
  h, w = 20, 70
  flat = np.full((270, 4), np.nan, np.float32)
  flat[3:260] = cloud(11, 257, h, w)
  flat[265] = (0.3, -0.2, 7.0, 0.5)
  first, count = [7, 265, 3], [0, 1, 257]
  mats = np.stack([view_mats(h, w)] * 3)
  mats[1, :, 3] += 2.0                                    # every scan its own matrices
  flat.setflags(write=False)
  return flat, first, count, mats, h, w


@pytest.mark.parametrize('inverse', [False, True])
def test_packed_ragged_batch(dev, inverse):
  flat, first, count, mats, h, w = packed_case()
  kw = dict(z_max=Z_MAX, inverse=inverse)
  want = R.rasterize(flat, first, count, mats, h, w, **kw)
  assert not want[0].any() and (want[1] != 0).sum() == 2 and (want[2, 0] != 0).sum() > 50
  assert_same(run(dev, flat, first, count, mats, h, w, **kw), want, 'packed')


@functools.lru_cache(maxsize=None)
def padded_case():
  """[B, Nmax, 4] with first = None: 20 000 and 19 999 points at 48 x 160 (2.6
  points per pixel and view: every pixel is contended), NaN past the count."""
  h, w = 48, 160
  pts = np.stack([cloud(21, 20000, h, w), cloud(22, 20000, h, w)])
  pts[1, 19999:] = np.nan
  mats = np.stack([view_mats(h, w)] * 2)
  pts.setflags(write=False)
  return pts, [20000, 19999], mats, h, w


@functools.lru_cache(maxsize=None)
def padded_want(window, ratio, inverse):
  pts, count, mats, h, w = padded_case()
  stats = {}
  want = R.rasterize(pts, None, count, mats, h, w, z_max=Z_MAX, occl_window=window,
                     occl_ratio=ratio, inverse=inverse, stats=stats)
  want.setflags(write=False)
  return want, stats


@pytest.mark.parametrize('inverse', [False, True])
def test_padded_batch(dev, inverse):
  pts, count, mats, h, w = padded_case()
  want, stats = padded_want((0, 0), 1.0, inverse)
  assert stats['kept'] > 0.5 * want.size
  got = run(dev, pts, None, count, mats, h, w, z_max=Z_MAX, inverse=inverse)
  assert_same(got, want, 'padded')
  # the same scans through explicit descriptors, as counts on the device
  got = run(dev, pts.reshape(-1, 4), [0, 20000], torch.tensor(count, dtype=torch.int32, device=dev),
            mats, h, w, z_max=Z_MAX, inverse=inverse)
  assert_same(got, want, 'padded, explicit first')


def test_no_points_at_all(dev):
  from lsi.geometry import lidar
  mats = torch.from_numpy(np.stack([view_mats(9, 11)] * 2)).to(dev)
  for pts in (torch.zeros((0, 4), device=dev), torch.full((8, 4), float('nan'), device=dev)):
    out = lidar.rasterize_points(pts, [0, 0], [0, 0], mats, 9, 11, occl_window=(1, 1))
    assert out.shape == (2, 2, 9, 11, 1) and not out.any()


# --- 2. the filter -------------------------------------------------------------------
@pytest.mark.parametrize('ratio', [1.0, 1.25])
@pytest.mark.parametrize('window', [(0, 3), (2, 0), (8, 8)])
def test_occlusion_filter(dev, window, ratio):
  pts, count, mats, h, w = padded_case()
  for inverse in (False, True):
    want, stats = padded_want(window, ratio, inverse)
    # the comparison cannot pass on an untouched or an all-empty map
    assert stats['removed'] >= 1 and stats['kept'] >= 1, stats
    got = run(dev, pts, None, count, mats, h, w, z_max=Z_MAX, occl_window=window,
              occl_ratio=ratio, inverse=inverse)
    assert_same(got, want, 'filter %s %s' % (window, ratio))
  print(window, ratio, stats)


@pytest.mark.parametrize('size', [(TILE_H - 1, TILE_W - 1), (TILE_H + 1, TILE_W + 1),
                                  (TILE_H - 1, TILE_W + 1), (TILE_H + 1, TILE_W - 1),
                                  (2 * TILE_H + 1, 2 * TILE_W + 1), (3, 5)])
def test_sizes_around_the_tile(dev, size):
  from lsi.geometry import lidar
  assert lidar.TILE == (TILE_H, TILE_W)
  h, w = size
  pts = cloud(31 + h, 3 * h * w, h, w, share=0.05 if h * w > 100 else 0.4)[None]
  mats = view_mats(h, w)[None]
  for window, ratio in (((0, 0), 1.0), ((8, 8), 1.25), ((2, 3), 1.25), ((1, 8), 1.0)):
    stats = {}
    want = R.rasterize(pts, None, [pts.shape[1]], mats, h, w, z_max=Z_MAX, occl_window=window,
                       occl_ratio=ratio, stats=stats)
    assert stats['kept'] >= 1 and (window == (0, 0) or stats['removed'] >= 1), (window, stats)
    got = run(dev, pts, None, [pts.shape[1]], mats, h, w, z_max=Z_MAX, occl_window=window,
              occl_ratio=ratio)
    assert_same(got, want, '%s window %s' % (size, window))


# --- 3. contention -------------------------------------------------------------------
@pytest.mark.parametrize('patch', [1, 2])
def test_contended_pixels_keep_the_minimum(dev, patch):
  """4096 points of distinct depths on one pixel, and on a 2 x 2 patch."""
  h, w = 32, 64
  m = np.array([[64, 0, 32, 0], [0, 64, 16, 0], [0, 0, 1, 0]], np.float32).reshape(1, 1, 12)
  rs = np.random.RandomState(40 + patch)
  z = (4 + np.arange(4096) * 2.0 ** -10).astype(np.float32)        # distinct, exact
  rs.shuffle(z)
  # u = 64 x / z + 32: x / z = 1 / 128 or 3 / 128 is the middle of column 32 or 33
  cell = rs.randint(0, patch, (2, 4096))
  pts = np.zeros((1, 4096, 4), np.float32)
  pts[0, :, 0] = z * ((2 * cell[0] + 1) / 128.0)
  pts[0, :, 1] = z * ((2 * cell[1] + 1) / 128.0)
  pts[0, :, 2] = z
  want = R.rasterize(pts, None, [4096], m, h, w)
  filled = np.argwhere(want[0, 0, :, :, 0])
  assert len(filled) == patch * patch
  for r, c in filled:
    on = (cell[1] == r - 16) & (cell[0] == c - 32)
    assert on.sum() > 900 // (patch * patch) and want[0, 0, r, c, 0] == z[on].min()
  assert_same(run(dev, pts, None, [4096], m, h, w), want, 'contention')
  assert_same(run(dev, pts, None, [4096], m, h, w, inverse=True),
              R.rasterize(pts, None, [4096], m, h, w, inverse=True), 'contention, inverse')


# --- 4. checks that need no oracle ---------------------------------------------------
def test_invariant_under_a_permutation_of_the_points(dev):
  pts, count, mats, h, w = padded_case()
  kw = dict(z_max=Z_MAX, occl_window=(2, 2), occl_ratio=1.25)
  a = run(dev, pts[:1], None, count[:1], mats[:1], h, w, **kw)
  perm = np.random.RandomState(50).permutation(count[0])
  b = run(dev, pts[:1, perm], None, count[:1], mats[:1], h, w, **kw)
  c = run(dev, pts[:1, ::-1], None, count[:1], mats[:1], h, w, **kw)
  assert_same(b, a, 'permuted')
  assert_same(c, a, 'reversed')
  assert (a != 0).any()


def test_view_0_of_two_is_the_single_view(dev):
  pts, count, mats, h, w = padded_case()
  for kw in (dict(z_max=Z_MAX), dict(z_max=Z_MAX, occl_window=(1, 2), occl_ratio=1.1,
                                     inverse=True)):
    two = run(dev, pts, None, count, mats, h, w, **kw)
    for j in range(2):
      one = run(dev, pts, None, count, mats[:, j:j + 1], h, w, **kw)
      assert_same(one[:, 0], two[:, j], 'view %d' % j)
    assert not np.array_equal(two[:, 0], two[:, 1])


# --- 5. the op route -----------------------------------------------------------------
def test_op_route_equals_the_kernel_on_the_device(dev):
  from lsi.geometry import lidar
  flat, first, count, mats, h, w = packed_case()
  pts, pcount, pmats, ph, pw = padded_case()
  for args, kw in (((flat, first, count, mats, h, w), dict(z_max=Z_MAX)),
                   ((flat, first, count, mats, h, w), dict(z_max=Z_MAX, inverse=True,
                                                           occl_window=(1, 1), occl_ratio=1.25)),
                   ((pts, None, pcount, pmats, ph, pw), dict(z_max=Z_MAX)),
                   ((pts, None, pcount, pmats, ph, pw), dict(z_max=Z_MAX, inverse=True,
                                                             occl_window=(2, 3), occl_ratio=1.25))):
    t = [torch.from_numpy(np.array(args[0])).to(dev), args[1], args[2],
         torch.from_numpy(args[3]).to(dev), args[4], args[5]]
    ops = lidar.rasterize_points_ops(*t, **kw)
    hip = lidar.rasterize_points(*t, **kw)
    assert ops.device == hip.device and ops.shape == hip.shape
    assert_same(ops.cpu().numpy(), hip.cpu().numpy(), 'op route %s' % (kw,))


# --- 6. the evaluation ---------------------------------------------------------------
PLANE_DEPTH = 10.0


def _kitti_batch(seed, bs=2, h=128, w=128):
  """A KITTI-shaped batch as ldi_enc_dec.KittiBatches hands it on (CPU tensors),
  with the three velodyne outputs: points on the plane Z = PLANE_DEPTH of the
  camera frame, the second scan shorter and NaN-padded."""
  rs = np.random.RandomState(seed)
  f = w / 2.0
  k = np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1]], np.float32)
  n = 6000
  pts = np.full((bs, n, 4), np.nan, np.float32)
  counts = np.array([n, n - 1500], np.int32)
  for b in range(bs):
    u, v = rs.uniform(0, w, counts[b]), rs.uniform(0, h, counts[b])
    pts[b, :counts[b], 0] = (u - w / 2.0) * PLANE_DEPTH / f
    pts[b, :counts[b], 1] = (v - h / 2.0) * PLANE_DEPTH / f
    pts[b, :counts[b], 2] = PLANE_DEPTH
    pts[b, :counts[b], 3] = 0.5
  mats = np.zeros((bs, 2, 3, 4), np.float32)
  mats[:, :, :, :3] = k
  mats[:, 1, 0, 3] = -0.5 * f                              # the target camera's offset
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
  return (t(rs.rand(bs, h, w, 3).astype(np.float32)), t(rs.rand(bs, h, w, 3).astype(np.float32)),
          t(np.stack([k] * bs)), t(np.stack([k] * bs)), t(np.stack([np.eye(3, dtype=np.float32)] * bs)),
          t(np.tile(np.array([[-0.5], [0], [0]], np.float32), (bs, 1, 1))),
          t(pts), t(counts), t(mats.reshape(bs, 2, 12)))


def _evaluate(tmp_path, monkeypatch, replay, recording, name, batches, *extra):
  """ldi_pred_eval.Tester.test on `batches`, the network's forward pass pinned by
  tests/test_visuals_gpu.py's Replay (it is not reproducible from run to run)."""
  import ldi_enc_dec as script
  import ldi_pred_eval as ev
  opts = script.apply_dataset_overrides(ev.build_parser().parse_args(
      ['--dataset', 'kitti', '--kitti_procedural', 'true', '--batch_size', '2', '--n_layers', '2',
       '--img_height', '128', '--img_width', '128', '--num_eval_iter', '2', '--random_weights',
       'true', '--checkpoint_dir', str(tmp_path), '--exp_name', name, '--eval_depth', 'true',
       '--kitti_dl_velodyne', 'true'] + list(extra)))
  restore = ev.Tester.restore

  def pinned_restore(self):
    restore(self)
    model = self.trainer.model
    self.trainer.model = lambda *a: replay('model', model(*a))

  replay.start(recording)
  monkeypatch.setattr(ev.Tester, 'restore', pinned_restore)
  try:
    return ev.Tester(opts).test(batches=batches)
  finally:
    monkeypatch.undo()


def test_evaluation_scores_both_views_against_the_scans(tmp_path, dev, monkeypatch):
  from test_visuals_gpu import Replay
  from lsi.nnutils import eval_metrics
  batches = [_kitti_batch(60), _kitti_batch(61)]
  replay = Replay()
  runs = {}
  runs['false'] = _evaluate(tmp_path, monkeypatch, replay, True, 'ops', batches,
                            '--device_metrics', 'false')
  assert len(replay.tape['model']) == 2
  runs['true'] = _evaluate(tmp_path, monkeypatch, replay, False, 'fused', batches,
                           '--device_metrics', 'true')
  keys = eval_metrics.DEPTH_KEYS
  assert set(keys) <= set(runs['true']) and set(runs['true']) == set(runs['false'])
  # by hand: the restatement's maps, scored by add_depth_accuracy, in the order
  # the evaluation scores them (source view, then target view, batch by batch)
  acc = eval_metrics.MetricAccumulator(dev)
  for batch, (ldi_src, ldi_trg) in zip(batches, replay.tape['model']):
    gt = R.rasterize(batch[6].numpy(), None, batch[7].numpy(), batch[8].numpy(), 128, 128,
                     z_min=1e-3, z_max=80., inverse=True)
    filled = gt[gt != 0]
    assert filled.size > 0.15 * gt.size and np.all(filled == np.float32(1 / PLANE_DEPTH))
    for view, ldi in enumerate((ldi_src, ldi_trg)):
      acc.add_depth_accuracy(ldi[2][0], torch.from_numpy(gt[:, view].copy()).to(dev), None,
                             valid_above=0., depth_min=1e-3, depth_max=80.)
  hand = acc.results()
  for k in keys:
    got, want = runs['true'][k], runs['false'][k]
    print('%s: %.12g (op route %.12g, by hand %.12g)' % (k, got, want, hand[k]))
    assert np.isfinite(got)
    assert got == hand[k], k
    # the tolerance of tests/test_depth_metrics_gpu.py for the two routes
    if k in ('depth_a1', 'depth_a2', 'depth_a3'):
      assert abs(got - want) <= 1e-12, k
    else:
      assert abs(got - want) <= 1e-5 * abs(want), k
  # a window and an origin reach the rasteriser: with a one-depth plane nothing is
  # occluded, so the figures stay what they were
  same = _evaluate(tmp_path, monkeypatch, replay, False, 'window', batches, '--device_metrics',
                   'true', '--lidar_occl_window', '2', '2', '--lidar_occl_ratio', '1.25')
  assert all(same[k] == runs['true'][k] for k in keys)
  with pytest.raises(ValueError, match='pick'):
    _evaluate(tmp_path, monkeypatch, replay, False, 'both', batches, '--device_metrics', 'true',
              '--kitti_dl_disparities_px', 'true')
