"""The fused depth accuracy metrics (csrc/lsi_depth_metrics.hip) and
MetricAccumulator.add_depth_accuracy on top of them, against the fp64 NumPy
restatement in tests/depth_metrics_ref.py and the op route of
lsi.nnutils.eval_metrics.

Shapes are the smallest at which each part can go wrong: one pixel; 3 x 20 x 28
(560 pixels: three blocks per image, no multiple of 64); 2 x 64 x 96 with a crop
at odd offsets and a mask; one 256 x 768 image, which reaches the cap of 64
blocks per image.  (One pixel with median scaling is image 2 of the median
fixtures: its figures are zero up to rounding.)

Tolerances.  n_b, the scored flags and the scale s_b (fp32 bits) are equal: the
scored set and the order statistics are exact.  The delta shares are equal
where the restatement finds no scored pixel within 1e-4 relative of a threshold
or a depth cap: the fixture builder guarantees it, the fixtures made by hand are
redrawn until it holds, and every test asserts it.  abs_rel, sq_rel, rmse and
rmse_log agree within 1e-5 relative: the terms are non-negative, so a sum's
relative error is bounded by the per-term error -- about ten roundings of at
most 2.5 ulp (logf, the divisions), 1.5e-6 -- plus the fp32 per-thread
accumulation of at most 12 terms (7e-7); 1e-5 leaves several times that."""
import functools
import os

import numpy as np
import pytest
import torch

import depth_metrics_ref as R

pytestmark = pytest.mark.gpu

DELTAS = ('depth_a1', 'depth_a2', 'depth_a3')


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


CASES = {
    'one_pixel': ((1, 1, 1), dict(empty=0., depth_max=150.)),
    'three_blocks': ((3, 20, 28), dict()),
    'three_blocks_median': ((3, 20, 28), dict(median=True)),
    'crop_bool_mask_median': ((2, 64, 96), dict(crop=(5, 51, 7, 90), mask='bool', median=True)),
    'crop_f32_mask_cap40': ((2, 64, 96), dict(crop=(5, 51, 7, 90), mask='f32', depth_max=40.)),
    'block_cap': ((1, 256, 768), dict()),
    'block_cap_median': ((1, 256, 768), dict(median=True)),
}


@functools.lru_cache(maxsize=None)
def case(name):
  """(pred, gt, kwargs, table) of a case, computed once and left unchanged."""
  shape, kw = CASES[name]
  pred, gt, kw = R.case_inputs(sorted(CASES).index(name) + 200, shape, kw)
  table, near = R.per_image_table(pred, gt, np.ones((shape[0],), np.float32),
                                  margin=1e-4, **kw)
  assert near == 0          # what makes equal delta shares a fair demand
  for a in (pred, gt, table):
    a.setflags(write=False)
  return pred, gt, kw, table


def run(dev, pred, gt, kw, acc=None, scale=None):
  """One add_depth_accuracy call; returns (accumulator, per-image table)."""
  from lsi.nnutils import eval_metrics
  acc = acc or eval_metrics.MetricAccumulator(dev)
  b = pred.shape[0]
  per_image = torch.full((b, 10), -1.0, dtype=torch.float64, device=dev)
  tkw = {k: (torch.tensor(v, device=dev) if k == 'mask' else v) for k, v in kw.items()}
  acc.add_depth_accuracy(
      torch.tensor(pred, device=dev)[..., None], torch.tensor(gt, device=dev)[..., None],
      None if scale is None else torch.tensor(scale, device=dev), per_image=per_image, **tkw)
  return acc, per_image.cpu().numpy()


def check_table(got, want, floors=None):
  """floors: row -> absolute allowance of that image's four sums (see
  test_median_scale_is_the_exact_order_statistic); every other row is held to
  1e-5 relative.  The delta shares are equal: every caller has asserted that
  the restatement finds no pixel near a threshold or a cap."""
  assert np.array_equal(got[:, 8:], want[:, 8:])           # n_b, scored
  assert np.array_equal(got[:, 7].astype(np.float32).view(np.uint32),
                        want[:, 7].astype(np.float32).view(np.uint32))  # s_b, bit for bit
  assert np.isfinite(got).all()
  for i in range(got.shape[0]):
    floor = (floors or {}).get(i, 0.)
    for j in range(4):
      print('image %d %s: %.12g (restatement %.12g, rel %.3g)' % (
          i, R.COLUMNS[j], got[i, j], want[i, j],
          abs(got[i, j] - want[i, j]) / max(abs(want[i, j]), 1e-300)))
      assert abs(got[i, j] - want[i, j]) <= 1e-5 * abs(want[i, j]) + floor * (1, 80, 80, 1)[j], (
          i, R.COLUMNS[j])
    for j in range(4, 7):
      assert got[i, j] == want[i, j], (i, R.COLUMNS[j], got[i, j], want[i, j])


def sequential_sum(tables, acc0=None):
  """What the finishing kernel leaves in the 9 doubles: the scored rows added
  one by one, images in index order, calls in call order."""
  acc = np.zeros(9) if acc0 is None else acc0.copy()
  for t in tables:
    for row in t:
      if row[9]:
        acc[:8] += row[:8]
        acc[8] += 1.0
  return acc


# --- 1. the per-image table ----------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_per_image_table_matches_the_restatement(dev, name):
  pred, gt, kw, want = case(name)
  acc, got = run(dev, pred, gt, kw)
  check_table(got, want)
  assert np.array_equal(acc.acc_depth.cpu().numpy(), sequential_sum([got]))
  if name.startswith('block_cap'):
    assert want[0, 8] > 64 * 256      # more scored pixels than one round of the blocks


def test_pixel_disparities_and_a_scale_per_image(dev):
  """gt_scale: the maps of the three_blocks case as pixel disparities of three
  cameras (powers of two, so the products are exact) give the same table."""
  pred, gt, kw, want = case('three_blocks_median')
  f = np.array([64., 128., 32.], np.float32)
  _, got = run(dev, pred, gt * f[:, None, None], kw, scale=1 / f)
  check_table(got, want)


# --- 2. median scaling --------------------------------------------------------------
def _median_batch(seed):
  """Eight 20 x 28 images, one per case of the select; gt_scale 1, depth caps
  [1e-3, 80], no odd predictions except where the case asks for them.  Returns
  (pred, gt, table with median scaling, table without, pixels near a threshold
  or a cap in either)."""
  h, w = 20, 28
  pred, gt = R.build_fixture(seed, (8, h, w), median=True, odd_preds=False)
  pred, gt = pred.copy(), gt.copy()
  rs = np.random.RandomState(seed + 1)
  v, _ = R.scored_set(gt, np.ones(8, np.float32))

  def parity(i, odd):
    if (int(v[i].sum()) % 2 == 1) != odd:
      y, x = [a[0] for a in np.nonzero(v[i])]
      gt[i, y, x] = 0
  parity(0, True)                                   # 0: an odd count
  parity(1, False)                                  # 1: an even count
  keep = np.nonzero(v[2])
  one = gt[2, keep[0][5], keep[1][5]]
  gt[2] = 0
  gt[2, keep[0][5], keep[1][5]] = one               # 2: exactly one scored pixel
  gt[3] = 0                                         # 3: none
  gt[4][gt[4] > 0] = 0.125
  pred[4] = 0.25                                    # 4: all values equal
  lv = np.exp(np.linspace(np.log(0.02), np.log(1.5), 16)).astype(np.float32)
  gt[5] = np.where(gt[5] > 0, lv[rs.randint(0, 16, (h, w))], 0)
  pred[5] = lv[rs.randint(0, 16, (h, w))]           # 5: many ties, 16 levels
  zero = rs.rand(h, w) < 0.3                        # 6: dp_raw spans > 30 binades
  pred[6][zero] = 0
  pred[6][rs.rand(h, w) < 0.05] = np.nan
  pred[6][rs.rand(h, w) < 0.05] = -1.0
  pred[7][rs.rand(h, w) < 0.6] = 0                  # 7: more than half zero
  scale = np.ones(8, np.float32)
  table, near = R.per_image_table(pred, gt, scale, median=True, margin=1e-4)
  plain, near_plain = R.per_image_table(pred, gt, scale, median=False, margin=1e-4)
  return pred, gt, table, plain, near + near_plain


@functools.lru_cache(maxsize=None)
def median_batch():
  """The first of the fixtures above (by seed) in which the restatement finds
  no pixel within 1e-4 relative of a threshold or a cap, with the median
  scaling and without: the edits that make the cases cannot be guarded by the
  builder, so the whole fixture is redrawn instead."""
  for seed in range(77, 577):
    pred, gt, table, plain, near = _median_batch(seed)
    if near == 0:
      break
  assert near == 0
  for a in (pred, gt, table, plain):
    a.setflags(write=False)
  return pred, gt, table, plain


@functools.lru_cache(maxsize=None)
def bad_predictions():
  """One image of zero, negative, NaN, tiny and infinite predictions against
  the ground truth of the first image of median_batch() with none near a
  threshold: (pred, gt, {median: table})."""
  h, w = 20, 28
  kinds = np.array([0, -2.5, np.nan, 1e-9, np.inf, -np.inf, -0.0], np.float32)
  bad = np.tile(kinds, h * w // 7 + 1)[:h * w].reshape(1, h, w)
  one = np.ones(1, np.float32)
  for i in range(8):
    gt = median_batch()[1][i:i + 1]
    tables = {m: R.per_image_table(bad, gt, one, median=m, margin=1e-4) for m in (False, True)}
    if tables[False][0][0, 8] > 0 and tables[False][1] == 0 and tables[True][1] == 0:
      break
  assert tables[False][1] == 0 and tables[True][1] == 0 and tables[False][0][0, 8] > 0
  return bad, gt, {m: t[0] for m, t in tables.items()}


def test_median_scale_is_the_exact_order_statistic(dev):
  """The scale is the restatement's bit for bit.  Where the scaled prediction
  equals the true depth up to rounding (images 2 and 4: one scored pixel; all
  values equal) the restatement's own figures are rounding residue of s_b dp_raw,
  1e-8 and less, and a relative bound says nothing: those two images' figures may
  differ by 2^-19 --
  an ulp of dp relative to dg and an ulp of each logf at log(80) -- times the
  depth cap for the two figures that carry a length."""
  pred, gt, want, _ = median_batch()
  n = want[:, 8]
  assert n[0] % 2 == 1 and n[1] % 2 == 0 and n[1] > 0 and n[2] == 1 and n[3] == 0
  assert want[7, 7] < 1e-30 and want[6, 7] > 1e-3    # a tiny scale; an ordinary one
  acc, got = run(dev, pred, gt, dict(median=True))
  for i in range(8):
    print('image %d: n %d, s_b %.9g (restatement %.9g)' % (i, got[i, 8], got[i, 7], want[i, 7]))
  check_table(got, want, floors={2: 2.0**-19, 4: 2.0**-19})
  assert not got[3].any()                            # the image without ground truth
  a = acc.acc_depth.cpu().numpy()
  assert np.array_equal(a, sequential_sum([got])) and a[8] == 7
  assert np.isfinite(a).all()
  # alone, the empty image leaves the accumulator as it is
  acc2, got2 = run(dev, pred[3:4], gt[3:4], dict(median=True), acc=acc)
  assert not got2.any() and np.array_equal(acc2.acc_depth.cpu().numpy(), a)


# --- 3. robustness ------------------------------------------------------------------
def test_bad_predictions_give_finite_metrics(dev):
  """Zero, negative, NaN and infinite predictions are huge (or zero) finite
  depths: the figures are the restatement's, and no NaN reaches the sums."""
  pred, gt, _, want = median_batch()
  acc, got = run(dev, pred, gt, dict())
  check_table(got, want)
  bad, gt1, tables = bad_predictions()
  for median in (False, True):
    acc, got_bad = run(dev, bad, gt1, dict(median=median), acc=acc)
    check_table(got_bad, tables[median])
  assert np.isfinite(acc.acc_depth.cpu().numpy()).all()


# --- 4. accumulation ----------------------------------------------------------------
def test_accumulation_is_ordered_and_reproducible(dev):
  from lsi.nnutils import eval_metrics
  calls = [case('three_blocks_median'), case('crop_bool_mask_median'), case('three_blocks')]

  def sequence():
    acc, tables = eval_metrics.MetricAccumulator(dev), []
    for pred, gt, kw, _ in calls[:2]:
      tables.append(run(dev, pred, gt, kw, acc=acc)[1])
    return acc, tables
  acc, tables = sequence()
  nine = acc.acc_depth.cpu().numpy()
  assert np.array_equal(nine, sequential_sum(tables))
  sums = acc.sums()
  for j, k in enumerate(R.KEYS + ('depth_scale',)):
    assert sums[k] == (nine[j], nine[8]), k
  assert nine[8] == 5
  again = sequence()[0].acc_depth.cpu().numpy()
  assert np.array_equal(again.view(np.uint64), nine.view(np.uint64))
  acc.reset()
  assert not acc.acc_depth.cpu().numpy().any() and not acc.acc.cpu().numpy().any()
  # without a median call there is no depth_scale; before any call no depth key
  fresh = eval_metrics.MetricAccumulator(dev)
  assert not any(k.startswith('depth_a') or k.startswith('depth_r') for k in fresh.sums())
  run(dev, *calls[2][:3], acc=fresh)
  assert set(R.KEYS) <= set(fresh.sums()) and 'depth_scale' not in fresh.sums()


def test_results_match_the_op_route(dev):
  from lsi.nnutils import eval_metrics
  acc, dicts = eval_metrics.MetricAccumulator(dev), []
  for name in ('three_blocks_median', 'crop_bool_mask_median'):
    pred, gt, kw, _ = case(name)
    run(dev, pred, gt, kw, acc=acc)
    tkw = {k: (torch.tensor(v, device=dev) if k == 'mask' else v) for k, v in kw.items()}
    dicts.append(eval_metrics.depth_accuracy_metrics(
        torch.tensor(pred, device=dev)[..., None], torch.tensor(gt, device=dev)[..., None], **tkw))
  got, want = acc.results(), eval_metrics.aggregate(dicts)
  assert set(got) == set(want) == set(R.KEYS + ('depth_scale',))
  for k in want:
    print('%s: %.12g (op route %.12g)' % (k, got[k], want[k]))
    if k in DELTAS:
      assert abs(got[k] - want[k]) <= 1e-12, k
    else:
      assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), k


# --- 5. no host synchronisation, a launch count that ignores the data ----------------
def _depth_kernels(dev, pred, gt, kw):
  from torch.profiler import profile, ProfilerActivity
  from lsi.nnutils import eval_metrics
  acc = eval_metrics.MetricAccumulator(dev)
  p, g = torch.tensor(pred, device=dev), torch.tensor(gt, device=dev)
  acc.add_depth_accuracy(p, g, **kw)            # allocations and code loading
  torch.cuda.synchronize()
  before = torch.cuda.get_sync_debug_mode()
  with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    torch.cuda.set_sync_debug_mode('error')     # a synchronising torch call raises
    try:
      acc.add_depth_accuracy(p, g, **kw)
    finally:
      torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
  on_device = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA')]
  assert not [n for n in on_device if 'memcpy' in n.lower()], on_device
  return sorted(n for n in on_device if 'depth_' in n)


def test_no_synchronisation_and_a_fixed_launch_count(dev):
  pred, gt, _, _ = case('three_blocks')
  empty = np.zeros_like(gt)
  for kw, count in ((dict(), 2), (dict(median=True), 10)):
    full = _depth_kernels(dev, pred, gt, kw)
    none = _depth_kernels(dev, pred, empty, kw)
    print(kw, full)
    assert len(full) == count and len(none) == count, (full, none)


# --- 6. errors -----------------------------------------------------------------------
def test_errors(dev):
  from lsi.nnutils import eval_metrics
  pred, gt, _, _ = case('three_blocks')
  acc = eval_metrics.MetricAccumulator(dev)
  p, g = torch.tensor(pred, device=dev), torch.tensor(gt, device=dev)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    acc.add_depth_accuracy(torch.tensor(pred), g)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    acc.add_depth_accuracy(p, g, mask=torch.ones(3, 20, 28))
  with pytest.raises(ValueError, match='x 1'):
    acc.add_depth_accuracy(p, g[:, :19])
  with pytest.raises(RuntimeError, match='code -1'):
    acc.add_depth_accuracy(p, g, crop=(0, 21, 0, 28))
  with pytest.raises(RuntimeError, match='code -1'):
    acc.add_depth_accuracy(p, g, depth_min=0.)
  assert not acc.acc_depth.cpu().numpy().any()
  # bf16 predictions are converted
  acc.add_depth_accuracy(p.bfloat16(), g)
  want = R.per_image_table(p.bfloat16().float().cpu().numpy(), gt, np.ones(3, np.float32))
  got = acc.sums()
  for j, k in enumerate(R.KEYS[:4]):
    assert abs(got[k][0] - want[:, j].sum()) <= 1e-5 * want[:, j].sum(), k


# --- 7. end to end -------------------------------------------------------------------
def _eval_argv(tmp_path, *extra):
  return ['--dataset', 'synthetic', '--synth_scene', 'planes', '--batch_size', '2',
          '--n_layers', '2', '--img_height', '128', '--img_width', '128',
          '--n_obj_max', '2', '--num_eval_iter', '2', '--random_weights', 'true',
          '--checkpoint_dir', str(tmp_path)] + list(extra)


def _run_tester(tmp_path, monkeypatch, replay, recording, name, *extra):
  """ldi_pred_eval.Tester as main() runs it, with the network's forward pass and
  forward_splat pinned by tests/test_visuals_gpu.py's Replay (neither is
  reproducible from run to run; its docstring has the figures): the results,
  which are also the keys of results.txt."""
  import ldi_enc_dec as script
  import ldi_pred_eval as ev
  from lsi.nnutils import eval_metrics
  opts = script.apply_dataset_overrides(ev.build_parser().parse_args(
      _eval_argv(tmp_path, '--exp_name', name, *extra)))
  opts.debug_synth_texture = False
  opts.synth_dl_eval_data = True
  restore, splat = ev.Tester.restore, eval_metrics.ldi_utils.forward_splat

  def pinned_restore(self):
    restore(self)
    model = self.trainer.model
    self.trainer.model = lambda *a: replay('model', model(*a))

  replay.start(recording)
  monkeypatch.setattr(ev.Tester, 'restore', pinned_restore)
  monkeypatch.setattr(eval_metrics.ldi_utils, 'forward_splat',
                      lambda *a, **k: replay('splat', splat(*a, **k)))
  try:
    results = ev.Tester(opts).test()
  finally:
    monkeypatch.undo()
  lines = open(os.path.join(str(tmp_path), name, 'results', 'results.txt')).read().splitlines()
  assert [l.split(' : ')[0] for l in lines] == sorted(results)
  assert all(np.isfinite(float(l.split(' : ')[1])) for l in lines)
  return results


def test_eval_script_scores_depth_on_both_routes(tmp_path, dev, monkeypatch):
  from test_visuals_gpu import Replay
  replay = Replay()
  plain = _run_tester(tmp_path, monkeypatch, replay, True, 'plain')
  assert len(plain) == 9 and not set(R.KEYS) & set(plain)
  assert len(replay.tape['model']) == 2 and len(replay.tape['splat']) == 4
  runs = {}
  for route in ('false', 'true'):
    runs[route] = res = _run_tester(tmp_path, monkeypatch, replay, False, 'depth_' + route,
                                    '--eval_depth', 'true', '--device_metrics', route)
    assert set(res) == set(plain) | set(R.KEYS)
    assert replay.pos == {'model': 1, 'splat': 3}     # the calls a run without the flag makes
  for k in R.KEYS:
    got, want = runs['true'][k], runs['false'][k]
    print('%s: %.12g (op route %.12g)' % (k, got, want))
    if k in DELTAS:
      # (the per-image shares are equal -- counts over counts; their fp64 sum over
      # the images is associated differently on the two routes: the last bit)
      assert abs(got - want) <= 1e-12, k
    else:
      assert abs(got - want) <= 1e-5 * abs(want), k
  for k in plain:                        # the keys that existed before are what they were
    print('%s: %.12g (without --eval_depth %.12g)' % (k, runs['false'][k], plain[k]))
    assert runs['false'][k] == plain[k], k
  med = _run_tester(tmp_path, monkeypatch, replay, False, 'median', '--eval_depth', 'true',
                    '--depth_median_scale', 'true', '--device_metrics', 'true')
  assert set(med) == set(plain) | set(R.KEYS) | {'depth_scale'} and med['depth_scale'] > 0
