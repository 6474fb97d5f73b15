"""The fused evaluation kernels (csrc/lsi_eval.hip) and the MetricAccumulator on
top of them, against the NumPy restatement in oracle/lsi_oracle.py and the op
route of lsi.nnutils.eval_metrics.  The kernels are driven directly with random
arrays: nothing is rendered except in the end-to-end test.

Tolerances (those tests/test_sampling_gpu.py applies to the same quantities):
sums within 2e-4 relative (1e-4 for the layer metrics), integer-valued
normalisers equal, dis-occlusion-weighted normalisers within 1e-5 relative,
PSNR within 0.05 dB of 10 log10(1 / mse) evaluated in fp64."""
import math
import os
import types

import numpy as np
import pytest
import torch

import lsi_oracle as O
from conftest import golden

pytestmark = pytest.mark.gpu

VIEW_KEYS = ('compose_splat_loss', 'compose_splat_loss_disocc', 'depth_splat_loss',
             'depth_splat_loss_disocc')
DM_NORMS = ('compose_splat_loss_disocc', 'depth_splat_loss_disocc')
LAYER_KEYS = ('fg_tex_error', 'fg_disp_error', 'bg_tex_error', 'bg_disp_error')


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def T(x, dev):
  return None if x is None else torch.tensor(x, device=dev)


def f32(a):
  return np.asarray(a, np.float32)


def view_inputs(seed, b=2, nl=1, ht=12, wt=20, fy=1, fx=1, valid=True,
                disocc='f32', depth=True):
  """Random arrays for one rendered view.  The valid mask has a band of zeros
  whose edges cut through the fy x fx blocks, so the 0.95 threshold decides."""
  rs = np.random.RandomState(seed)
  h, w = fy * ht, fx * wt
  d = {'recons': f32(rs.rand(nl, b, ht, wt, 3)),
       'recons_disp': f32(0.4 * rs.rand(nl, b, ht, wt, 1)) if depth else None,
       'target': f32(rs.rand(b, h, w, 3)),
       'gt_disp': f32(0.4 * rs.rand(b, h, w, 1)) if depth else None,
       'valid': None, 'disocc': None}
  if valid:
    v = np.ones((b, h, w, 1), np.float32)
    v[:, h // 3:h // 3 + max(3, h // 5)] = 0      # rows: an odd first row
    v[:, :, w // 2 + 1:w // 2 + 4] = 0            # columns: three wide, odd start
    v[0, -1, -1] = 0
    d['valid'] = v
  if disocc:
    m = rs.rand(b, h, w, 1) > 0.6
    d['disocc'] = m if disocc == 'bool' else f32(m)
  return d


def oracle_view(d, bdry):
  """The oracle's (sum, norm) pairs and the fp64 PSNR of the same arrays (None
  when no cell is scored)."""
  want = O.eval_view_synthesis_metrics(d['recons'], d['recons_disp'], d['target'],
                                       bdry, d['valid'], d['disocc'], d['gt_disp'])
  _, b, ht, wt, _ = d['recons'].shape
  tgt = O.area_downsample(d['target'], ht, wt)
  centre = np.zeros((b, ht, wt), np.float64)
  x_min, y_min = O.py2_round(wt * bdry), O.py2_round(ht * bdry)
  centre[:, y_min:ht - y_min, x_min:wt - x_min] = 1
  if d['valid'] is not None:
    centre *= O.area_downsample(d['valid'], ht, wt)[..., 0] > np.float32(0.95)
  assert centre.sum() == want['compose_splat_loss'][1]
  psnr = None
  if centre.sum() > 0:
    se = ((tgt.astype(np.float64) - d['recons'][0].astype(np.float64))**2).mean(-1)
    psnr = 10.0 * math.log10(1.0 / ((se * centre).sum() / centre.sum()))
  return want, psnr


def add(acc, d, bdry, dev, **kw):
  acc.add_rendered(T(d['recons'], dev), T(d['recons_disp'], dev), T(d['target'], dev),
                   bdry, valid_mask=T(d['valid'], dev), disocc_mask=T(d['disocc'], dev),
                   gt_disp_trg=T(d['gt_disp'], dev), **kw)


def check_sums(got, want, keys, sum_tol=2e-4):
  """got, want: name -> (sum, norm); every key of `keys` that `want` lacks must
  be exactly (0, 0) in `got`."""
  for k in keys:
    gs, gn = got[k]
    if k not in want:
      assert gs == 0.0 and gn == 0.0, (k, gs, gn)
      continue
    ws, wn = want[k]
    print('%s: sum %.9g (want %.9g)  norm %.9g (want %.9g)' % (k, gs, ws, gn, wn))
    assert abs(gs - ws) <= sum_tol * abs(ws), (k, gs, ws)
    if k in DM_NORMS:
      assert abs(gn - wn) <= 1e-5 * abs(wn), (k, gn, wn)
    else:
      assert gn == wn, (k, gn, wn)


def check_view(acc, wants, psnrs):
  """The accumulator against the sum of the oracle's results of its calls."""
  total = {}
  for w in wants:
    for k, (s, n) in w.items():
      a, c = total.get(k, (0.0, 0.0))
      total[k] = (a + s, c + n)
  got = acc.sums()
  check_sums(got, total, VIEW_KEYS)
  scored = [p for p in psnrs if p is not None]
  print('psnr: %r (want %r)' % (got['psnr'], scored))
  assert got['psnr'][1] == len(scored)
  if scored:
    assert abs(got['psnr'][0] / len(scored) - sum(scored) / len(scored)) <= 0.05
  else:
    assert got['psnr'][0] == 0.0
  for k in LAYER_KEYS:
    assert got[k] == (0.0, 0.0), k


def run_view_case(dev, bdry, **kw):
  from lsi.nnutils import eval_metrics
  d = view_inputs(**kw)
  acc = eval_metrics.MetricAccumulator(dev)
  add(acc, d, bdry, dev)
  want, psnr = oracle_view(d, bdry)
  check_view(acc, [want], [psnr])
  return acc, want


# --- 1. view metrics against the oracle --------------------------------------
@pytest.mark.parametrize('bdry', [0.1, 0.0])
@pytest.mark.parametrize('fy,fx', [(1, 1), (2, 2), (2, 4), (4, 2)])
def test_view_metrics_factors_and_crop(dev, fy, fx, bdry):
  _, want = run_view_case(dev, bdry, seed=3, fy=fy, fx=fx)
  assert set(want) == set(VIEW_KEYS)
  # the valid band removes cells, the dis-occlusion mask weights the rest
  assert 0 < want['compose_splat_loss_disocc'][1] < want['compose_splat_loss'][1]
  assert want['compose_splat_loss'][1] < 2 * 12 * 20


@pytest.mark.parametrize('depth', [False, True])
@pytest.mark.parametrize('disocc', [None, 'f32', 'bool'])
@pytest.mark.parametrize('valid', [False, True])
def test_view_metrics_optional_inputs(dev, valid, disocc, depth):
  """Every subset of the optional inputs; the slots of an absent metric stay 0."""
  _, want = run_view_case(dev, 0.1, seed=4, fy=2, fx=2, valid=valid, disocc=disocc,
                          depth=depth)
  assert ('depth_splat_loss' in want) == depth
  assert ('compose_splat_loss_disocc' in want) == bool(disocc)
  assert ('depth_splat_loss_disocc' in want) == bool(depth and disocc)


def test_view_metrics_min_over_two_layers(dev):
  d = view_inputs(seed=6, nl=2, fy=2, fx=2)
  one = dict(d, recons=d['recons'][:1], recons_disp=d['recons_disp'][:1])
  _, want = run_view_case(dev, 0.1, seed=6, nl=2, fy=2, fx=2)
  # the min over the layers matters: layer 0 alone scores worse
  assert want['compose_splat_loss'][0] < 0.95 * oracle_view(one, 0.1)[0]['compose_splat_loss'][0]
  assert want['depth_splat_loss'][0] < 0.95 * oracle_view(one, 0.1)[0]['depth_splat_loss'][0]


def test_view_metrics_valid_from_a_thresholded_map(dev):
  """valid_above: the kernel thresholds the map itself, as the caller's
  (map > valid_above).float() would."""
  from lsi.nnutils import eval_metrics
  d = view_inputs(seed=7, fy=2, fx=2)
  gt = d['gt_disp'].copy()
  gt[:, :7] = 0.01
  gt[:, :, 11:14] = 0.05                          # equal to the threshold: invalid
  d['gt_disp'] = gt
  d['valid'] = f32(gt > np.float32(0.05))
  want, psnr = oracle_view(d, 0.1)
  acc = eval_metrics.MetricAccumulator(dev)
  acc.add_rendered(T(d['recons'], dev), T(d['recons_disp'], dev), T(d['target'], dev),
                   0.1, valid_mask=T(gt, dev), disocc_mask=T(d['disocc'], dev),
                   gt_disp_trg=T(gt, dev), valid_above=0.05)
  check_view(acc, [want], [psnr])
  assert want['compose_splat_loss'][1] < 2 * 8 * 16


def test_view_metrics_without_a_scored_cell_adds_no_psnr(dev):
  d = view_inputs(seed=8, fy=2, fx=2)
  d['valid'] = np.zeros_like(d['valid'])
  from lsi.nnutils import eval_metrics
  acc = eval_metrics.MetricAccumulator(dev)
  add(acc, d, 0.1, dev)
  want, psnr = oracle_view(d, 0.1)
  assert psnr is None
  assert acc.sums()['psnr'] == (0.0, 0.0)
  assert acc.sums()['compose_splat_loss'] == (0.0, 0.0)
  assert 'psnr' not in acc.results() and 'compose_splat_loss' not in acc.results()


# --- 2. grid-stride and block edges ------------------------------------------
def test_view_metrics_partial_block(dev):
  run_view_case(dev, 0.1, seed=9, b=1, ht=7, wt=37, fy=2, fx=2)


def test_view_metrics_more_cells_than_the_grid(dev):
  # 589 824 cells > MAXBLK * 256 = 524 288: the grid-stride loop wraps
  run_view_case(dev, 0.1, seed=10, b=1, ht=512, wt=1152)


# --- 3. accumulation and reproducibility --------------------------------------
def test_accumulation_reproducibility_and_reset(dev, monkeypatch):
  from lsi.nnutils import eval_metrics
  cases = [view_inputs(seed=20, fy=2, fx=2),
           view_inputs(seed=21, fy=2, fx=2, valid=False, disocc='bool'),
           view_inputs(seed=22, b=1, ht=9, wt=15, fy=2, fx=4)]
  accs = [eval_metrics.MetricAccumulator(dev) for _ in range(2)]
  for acc in accs:
    for d in cases:
      add(acc, d, 0.1, dev)
  wants, psnrs = zip(*[oracle_view(d, 0.1) for d in cases])
  check_view(accs[0], wants, psnrs)
  a, b = [acc.acc.cpu().numpy() for acc in accs]
  assert a.tobytes() == b.tobytes()
  # the op route on the same renderings (its render replaced by the arrays)
  opts = types.SimpleNamespace(trg_splat_downsampling=1, zbuf_scale=50, max_disp=1,
                               bg_layer_disp=1e-3, splat_bdry_ignore=0.1)
  dicts = []
  for d in cases:
    monkeypatch.setattr(eval_metrics.ldi_utils, 'forward_splat',
                        lambda *a, _d=d, **k: (T(_d['recons'], dev), None,
                                               T(_d['recons_disp'], dev)))
    dicts.append(eval_metrics.view_synthesis_metrics(
        None, None, None, None, None, None, T(d['target'], dev), opts,
        valid_mask=T(d['valid'], dev), disocc_mask=T(d['disocc'], dev),
        gt_disp_trg=T(d['gt_disp'], dev)))
  agg = eval_metrics.aggregate(dicts)
  res = accs[0].results()
  assert set(res) == set(agg)
  for k in agg:
    print('%s: %.9g (op route %.9g)' % (k, res[k], agg[k]))
    if k == 'psnr':
      assert abs(res[k] - agg[k]) <= 0.05
    else:
      assert abs(res[k] - agg[k]) <= 2e-4 * abs(agg[k]), k
  accs[0].reset()
  assert not accs[0].acc.cpu().numpy().any()
  assert accs[0].results() == {}


# --- 4. layer metrics -----------------------------------------------------------
def layer_inputs(nl=2, b=2, h=16, w=24):
  rs = np.random.RandomState(5)
  ldis = [[f32(rs.rand(nl, b, h, w, 3)), None, f32(0.4 * rs.rand(nl, b, h, w, 1))]
          for _ in range(2)]
  imgs = [f32(rs.rand(b, h, w, 3)) for _ in range(2)]
  gt = {}
  for side in ('src', 'trg'):
    gt[side + '_gt_disp'] = f32(0.4 * rs.rand(b, h, w, 1))
    gt[side + '_gt_disp_bg'] = f32(0.4 * rs.rand(b, h, w, 1))
    gt[side + '_gt_tex_bg'] = f32(rs.rand(b, h, w, 3))
  return ldis, imgs, gt


@pytest.mark.parametrize('layout', ['contiguous', 'no_bg', 'permuted'])
def test_layer_metrics_against_the_oracle(dev, layout):
  from lsi.nnutils import eval_metrics
  opts = types.SimpleNamespace(bg_layer_disp=0.05)
  ldis, imgs, gt = layer_inputs()
  want = O.eval_layer_prediction_metrics(ldis[0], ldis[1], imgs[0], imgs[1], gt,
                                         opts.bg_layer_disp)
  if layout == 'no_bg':
    gt = {k: v for k, v in gt.items() if not k.endswith('_bg')}
    want = {k: v for k, v in want.items() if k.startswith('fg_')}
  dev_ldis = [[T(l[0], dev), None, T(l[2], dev)] for l in ldis]
  if layout == 'permuted':
    # channels-first storage (a convolution's output) viewed as L x B x H x W x 3
    for l in dev_ldis:
      l[0] = l[0].permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)
      assert not l[0].is_contiguous()
  acc = eval_metrics.MetricAccumulator(dev)
  acc.add_layer_prediction(dev_ldis[0], dev_ldis[1], T(imgs[0], dev), T(imgs[1], dev),
                           {k: T(v, dev) for k, v in gt.items()}, opts)
  got = acc.sums()
  check_sums(got, want, LAYER_KEYS, sum_tol=1e-4)
  assert 0 < want['fg_tex_error'][1] < 2 * 2 * 16 * 24
  for k in VIEW_KEYS + ('psnr',):
    assert got[k] == (0.0, 0.0), k
  assert set(acc.results()) == set(want)


# --- 5. dis-occlusion mask -------------------------------------------------------
def test_disocclusion_mask_golden(dev):
  from lsi.geometry import projection
  g = golden('disocclusion.npz')
  got = projection.disocclusion_mask(T(g['disps_src'], dev), T(g['disps_trg'], dev),
                                     None, T(g['M'], dev), fused=True)
  assert got.dtype == torch.float32 and tuple(got.shape) == g['mask'].shape
  assert np.array_equal(got.cpu().numpy(), g['mask'])


def _general_pose(b, h, w):
  from lsi.geometry import projection
  k = torch.tensor([[0.58 * w, 0, w / 2.0], [0, 0.58 * w, h / 2.0], [0, 0, 1.0]])
  rots, ts = [], []
  for i in range(b):
    ax, ay, az = [math.radians(a) for a in ((2.0, -3.0, 1.5), (-1.0, 2.5, -2.0))[i % 2]]
    rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)],
                   [0, math.sin(ax), math.cos(ax)]])
    ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0],
                   [-math.sin(ay), 0, math.cos(ay)]])
    rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0],
                   [0, 0, 1]])
    rots.append(f32(rz @ ry @ rx))
    ts.append(f32([[0.3], [-0.1], [0.2]]) * (1 if i % 2 == 0 else -1))
  ks = k.unsqueeze(0).repeat(b, 1, 1)
  return projection.forward_projection_matrix(ks, ks, torch.tensor(np.stack(rots)),
                                              torch.tensor(np.stack(ts)))


def test_disocclusion_mask_general_pose(dev):
  from lsi.geometry import projection
  from lsi.nnutils import helpers
  b, h, w, thresh = 2, 24, 40, 1e-2
  rs = np.random.RandomState(12)
  ds, dt = [f32(0.4 * rs.rand(b, h, w, 1)) for _ in range(2)]
  mat = _general_pose(b, h, w)
  # pixels whose decision lies within rounding of the threshold: the oracle alone
  u, v, d2 = O.project(mat.numpy(), ds[..., 0], 1.0)
  samp = O.bilinear(dt, np.stack([u, v], axis=-1))[..., 0]
  with np.errstate(all='ignore'):
    near = np.abs(np.abs(d2 - samp) - np.float32(thresh)) <= 1e-6
  assert near.mean() <= 0.005
  pc = helpers.pixel_coords(b, h, w, device=dev)
  args = (T(ds, dev), T(dt, dev))
  want = projection.disocclusion_mask(*args, pc, mat.to(dev), thresh=thresh)
  got = projection.disocclusion_mask(*args, pc, mat.to(dev), thresh=thresh, fused=True)
  want, got = want.cpu().numpy()[..., 0], got.cpu().numpy()[..., 0]
  ref = O.disocclusion_mask(ds, dt, mat.numpy(), thresh)[..., 0]
  assert 0.02 < ref.mean() < 0.98 and (ref[:, 1:-1, 1:-1] == 0).any()  # both outcomes
  assert np.array_equal(got[~near], want[~near])
  # other source points than the grid: the op route serves
  off = pc + torch.tensor([0.25, -0.25, 0.0], device=dev)
  assert np.array_equal(
      projection.disocclusion_mask(*args, off, mat.to(dev), thresh=thresh,
                                   fused=True).cpu().numpy(),
      projection.disocclusion_mask(*args, off, mat.to(dev), thresh=thresh).cpu().numpy())


# --- 6. no host synchronisation ---------------------------------------------------
def test_adds_do_not_synchronise(dev):
  from lsi.nnutils import eval_metrics
  if not hasattr(torch.cuda, 'set_sync_debug_mode'):
    pytest.skip('torch.cuda.set_sync_debug_mode is not available in this torch build')
  d = view_inputs(seed=30, fy=2, fx=2, disocc='bool')
  dv = {k: T(v, dev) for k, v in d.items()}
  ldis, imgs, gt = layer_inputs()
  dev_ldis = [[T(l[0], dev), None, T(l[2], dev)] for l in ldis]
  dev_imgs = [T(i, dev) for i in imgs]
  dev_gt = {k: T(v, dev) for k, v in gt.items()}
  opts = types.SimpleNamespace(bg_layer_disp=0.05)
  acc = eval_metrics.MetricAccumulator(dev)
  acc._workspace()
  torch.cuda.synchronize()
  before = torch.cuda.get_sync_debug_mode()
  torch.cuda.set_sync_debug_mode('error')
  try:
    acc.add_rendered(dv['recons'], dv['recons_disp'], dv['target'], 0.1,
                     valid_mask=dv['valid'], disocc_mask=dv['disocc'],
                     gt_disp_trg=dv['gt_disp'])
    acc.add_layer_prediction(dev_ldis[0], dev_ldis[1], dev_imgs[0], dev_imgs[1],
                             dev_gt, opts)
  finally:
    torch.cuda.set_sync_debug_mode(before)
  res = acc.results()
  assert set(res) == set(VIEW_KEYS + LAYER_KEYS + ('psnr',))


# --- 7. end to end ------------------------------------------------------------------
def _eval_argv(tmp_path):
  return ['--dataset', 'synthetic', '--synth_scene', 'planes', '--batch_size', '1',
          '--n_layers', '2', '--img_height', '128', '--img_width', '128',
          '--n_obj_max', '2', '--num_eval_iter', '2', '--random_weights', 'true',
          '--checkpoint_dir', str(tmp_path)]


def test_tester_device_metrics_match_the_op_route(tmp_path, dev):
  import ldi_enc_dec as script
  import ldi_pred_eval as ev
  from lsi.nnutils import eval_metrics
  opts = script.apply_dataset_overrides(ev.build_parser().parse_args(_eval_argv(tmp_path)))
  opts.debug_synth_texture = False
  opts.synth_dl_eval_data = True
  tester = ev.Tester(opts)
  tester.restore()
  batches = [tester.trainer.data_loader.forward(opts.batch_size) for _ in range(2)]
  dicts = []
  for b in batches:
    dicts += tester.eval_batch(batch=b)
  want = eval_metrics.aggregate(dicts)
  acc = eval_metrics.MetricAccumulator(tester.trainer.device)
  for b in batches:
    assert tester.eval_batch(batch=b, acc=acc) == []
  got = acc.results()
  assert set(got) == set(want) and len(want) == 9
  for k in want:
    print('%s: %.9g (op route %.9g)' % (k, got[k], want[k]))
    if k == 'psnr':
      assert abs(got[k] - want[k]) <= 0.05
    else:
      assert abs(got[k] - want[k]) <= 2e-4 * abs(want[k]), k


def test_eval_script_device_metrics_writes_the_same_keys(tmp_path, dev):
  import ldi_pred_eval as ev
  ev.main(_eval_argv(tmp_path) + ['--exp_name', 'run', '--device_metrics', 'true'])
  # (apply_dataset_overrides: the run's directory is <checkpoint_dir>/<exp_name>)
  lines = open(os.path.join(str(tmp_path), 'run', 'results', 'results.txt')).read().splitlines()
  # the keys and the format of the op route's file (test_eval_script_writes_results)
  assert [l.split(' : ')[0] for l in lines] == sorted(VIEW_KEYS + LAYER_KEYS + ('psnr',))
  for l in lines:
    assert np.isfinite(float(l.split(' : ')[1])), l


# --- 8. errors ------------------------------------------------------------------------
def test_errors(dev):
  from lsi.nnutils import eval_metrics
  d = view_inputs(seed=40, fy=2, fx=2)
  acc = eval_metrics.MetricAccumulator(dev)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    acc.add_rendered(torch.tensor(d['recons']), None, torch.tensor(d['target']), 0.1)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    acc.add_rendered(T(d['recons'], dev), None, T(d['target'], dev), 0.1,
                     disocc_mask=torch.tensor(d['disocc']))
  with pytest.raises((ValueError, RuntimeError), match='multiple|invalid shape'):
    acc.add_rendered(T(d['recons'], dev), None, T(d['target'][:, :23], dev), 0.1)
  ldis, imgs, gt = layer_inputs()
  opts = types.SimpleNamespace(bg_layer_disp=0.05)
  dev_ldis = [[T(l[0], dev), None, T(l[2], dev)] for l in ldis]
  dev_gt = {k: T(v, dev) for k, v in gt.items() if not k.endswith('_gt_tex_bg')}
  with pytest.raises(ValueError, match='all of'):
    acc.add_layer_prediction(dev_ldis[0], dev_ldis[1], T(imgs[0], dev), T(imgs[1], dev),
                             dev_gt, opts)
  cpu_ldis = [[torch.tensor(l[0]), None, torch.tensor(l[2])] for l in ldis]
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    acc.add_layer_prediction(cpu_ldis[0], cpu_ldis[1], torch.tensor(imgs[0]),
                             torch.tensor(imgs[1]),
                             {k: torch.tensor(v) for k, v in gt.items()}, opts)
  assert not acc.acc.cpu().numpy().any()          # nothing was added
  # the C entry points refuse the same before any launch
  from lsi import _C
  from lsi.nnutils import _hip_eval
  ws, n = _hip_eval.workspace(dev)
  r, t = T(d['recons'], dev), T(d['target'], dev)
  args = lambda h: (1, 2, 12, 20, h, 40, 2, 1, r.data_ptr(), None, t.data_ptr(),
                    *t.stride(), None, None, None, 0, 0.0, acc.acc.data_ptr(),
                    ws.data_ptr(), n, None)
  assert _C.lib().lsi_eval_view_metrics(*args(23)) == -1
  assert _C.lib().lsi_eval_view_metrics(*args(24)[:8], None, *args(24)[9:]) == -1
  assert _C.lib().lsi_eval_view_metrics(*args(24)[:-2], 8, None) == -1
  assert _C.lib().lsi_disocclusion_mask(1, 4, 4, 4, 4, None, None, None, 0.01, None,
                                        None) == -1
