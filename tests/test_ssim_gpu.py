"""The fused SSIM view-synthesis loss and metric (csrc/lsi_ssim.hip) against the
fp64 restatement of its definition (tests/ssim_ref.py).

Bars.  fp32 arithmetic itself misses the project's usual bars here (2e-6
relative on a loss, 1e-5 of the largest entry on a gradient) through the
E_xx - mu_x^2 cancellation, so every comparison first measures the error of the
fp32 op restatement against fp64 on the same inputs and allows the kernels
max(4 x that error, the usual bar): the factor 4 covers a different summation
order (tile-wise separable passes, fp64 partial sums) on top of the
cancellation both share.  The yardstick is always the fp64 restatement.

Condition on the inputs (not a tolerance: no window is left out): on the fp64
restatement the smallest gap between the best and the second-best layer over
all windows is >= 1e-4.  The seeds were picked on the CPU for that: with them the
gap is >= 1e-3, more than thirty times the largest per-window fp32 error of d
that the op restatement shows on these inputs (<= 3e-5), so the kernels and the
yardstick choose the same layer everywhere."""
import functools
import sys

import numpy as np
import pytest
import torch

import ssim_ref
from conftest import PKG

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_RTOL, SLACK = 2e-6, 1e-5, 4.0
MIN_GAP = 1e-4

# name: nl, B, Ht, Wt, factor, (x_min, y_min), win, sigma, seed
CASES = {
    'a': (3, 2, 23, 37, 2, (2, 1), 7, 1.5, 6),    # ragged tiles, in-kernel resize
    'b': (1, 2, 40, 70, 1, (0, 0), 11, 1.5, 1),   # several tiles, largest halo
    'c': (3, 1, 19, 45, 2, (3, 2), 3, 0.0, 1),    # box window, short window grid
    'd': (2, 2, 40, 70, 1, (4, 4), 11, 1.5, 8),   # min over layers, largest halo
    'e': (4, 2, 33, 50, 2, (3, 3), 7, 1.5, 2),    # training layer count
    'f': (1, 1, 11, 11, 1, (0, 0), 11, 1.5, 1),   # exactly one window
}


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def make_inputs(name, seed=None, amps=None):
  """(recons nl x B x Ht x Wt x 3, target B x H x W x 3) fp32 on the CPU.  The
  target: a smooth sinusoid plus uniform noise of +-0.075, clamped to [0, 1], one
  corner patch constant (zero variance: only C2 is left in the denominator).
  Layer l: the down-sampled target plus noise of amplitude 0.02 inside the blocks
  where ((x nl) // Wt + (2 y) // Ht) % nl == l and 0.12 elsewhere, so the best
  layer changes across the image at sharp borders.  amps = per-layer constant
  amplitudes instead."""
  nl, b, ht, wt, f, (x_min, y_min), win, _, case_seed = CASES[name]
  rng = np.random.RandomState(case_seed if seed is None else seed)
  h, w = ht * f, wt * f
  yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
  target = np.zeros((b, h, w, 3))
  for i in range(b):
    for c in range(3):
      target[i, :, :, c] = 0.5 + 0.3 * np.sin(
          2 * np.pi * ((1.0 + 0.5 * c) * xx / w + (0.75 + 0.25 * i) * yy / h) + c + i)
  target = np.clip(target + rng.uniform(-0.075, 0.075, target.shape), 0.0, 1.0)
  # (one whole window inside the crop, at most half the image each way)
  target[:, :min(f * (y_min + win), h // 2), :min(f * (x_min + win), w // 2)] = 0.5
  target = torch.from_numpy(target.astype(np.float32))
  t = ssim_ref.area(target, ht, wt).numpy()
  ys, xs = np.mgrid[0:ht, 0:wt]
  block = ((xs * nl) // wt + (2 * ys) // ht) % nl
  recons = np.zeros((nl, b, ht, wt, 3), np.float32)
  for l in range(nl):
    amp = np.where(block == l, 0.02, 0.12) if amps is None else np.full(block.shape,
                                                                          amps[l])
    noise = rng.uniform(-1.0, 1.0, (b, ht, wt, 3)) * amp[None, :, :, None]
    recons[l] = (t + noise).astype(np.float32)
  return torch.from_numpy(recons), target


def reference(recons, target, x_min, y_min, win, sigma, upstream=2.5):
  """Loss and gradient of (loss * upstream) from the op restatement in fp64 and
  in fp32, on the CPU, and the fp32 restatement's own errors."""
  out = {}
  for dt in (torch.float64, torch.float32):
    r = recons.to(dt).clone().requires_grad_(True)
    l = ssim_ref.loss(r, target.to(dt), x_min, y_min, win, sigma)
    (l * upstream).backward()
    out[dt] = (float(l.detach()), r.grad.double())
  l64, g64 = out[torch.float64]
  l32, g32 = out[torch.float32]
  return {'loss': l64, 'grad': g64,
          'loss_err32': abs(l32 - l64) / abs(l64),
          'grad_err32': float((g32 - g64).abs().max() / g64.abs().max())}


@functools.lru_cache(maxsize=None)
def case_reference(name):
  """Inputs and reference of a case, computed once and shared (read-only)."""
  recons, target = make_inputs(name)
  _, _, _, _, _, (x_min, y_min), win, sigma, _ = CASES[name]
  ref = reference(recons, target, x_min, y_min, win, sigma)
  ref['gap'] = ssim_ref.best_gap(recons.double(), target.double(), x_min, y_min, win,
                                 sigma)
  ref['recons'], ref['target'] = recons, target
  return ref


def kernel(recons, target, x_min, y_min, win, sigma, dev, upstream=2.5):
  """(loss, gradient of loss * upstream) from the HIP kernels."""
  from lsi.loss import _hip
  r = recons.to(dev).requires_grad_(True)
  l = _hip.ssim_view_synthesis_loss(r, target.to(dev), x_min, y_min, win, sigma)
  (l * upstream).backward()
  return l.detach(), r.grad


def check(tag, l, g, ref):
  """Prints the measured errors, then holds them against the bars."""
  loss_err = abs(float(l) - ref['loss']) / abs(ref['loss'])
  grad_err = float((g.cpu().double() - ref['grad']).abs().max() /
                   ref['grad'].abs().max())
  loss_bar = max(SLACK * ref['loss_err32'], LOSS_RTOL)
  grad_bar = max(SLACK * ref['grad_err32'], GRAD_RTOL)
  print('ssim %s: loss err kernel %.3g restatement %.3g bar %.3g | grad err kernel '
        '%.3g restatement %.3g bar %.3g' % (tag, loss_err, ref['loss_err32'], loss_bar,
                                            grad_err, ref['grad_err32'], grad_bar))
  assert loss_err <= loss_bar, (tag, loss_err, loss_bar)
  assert grad_err <= grad_bar, (tag, grad_err, grad_bar)


def outside_crop_is_zero(g, x_min, y_min):
  g = g.cpu()
  ht, wt = g.shape[2:4]
  inside = torch.zeros((ht, wt), dtype=torch.bool)
  inside[y_min:ht - y_min, x_min:wt - x_min] = True
  return bool((g[:, :, ~inside] == 0.0).all())


@pytest.mark.parametrize('name', sorted(CASES))
def test_forward_and_gradient(name, dev):
  ref = case_reference(name)
  _, _, _, _, _, (x_min, y_min), win, sigma, _ = CASES[name]
  assert ref['gap'] >= MIN_GAP, ref['gap']
  l, g = kernel(ref['recons'], ref['target'], x_min, y_min, win, sigma, dev)
  assert bool(torch.isfinite(g).all())
  check(name, l, g, ref)
  assert outside_crop_is_zero(g, x_min, y_min)
  if name == 'f':
    hv = ref['recons'].shape[2] - win + 1
    assert hv == 1                                   # exactly one window


def test_public_wrapper_derives_the_crop(dev):
  """loss.ssim_view_synthesis_loss: the crop from splat_bdry_ignore as
  view_synthesis_loss derives it (0.05 of 37 x 23 rounds to case a's 2, 1)."""
  from lsi.loss import loss
  ref = case_reference('a')
  assert (ssim_ref.py2_round(37 * 0.05), ssim_ref.py2_round(23 * 0.05)) == (2, 1)
  l = loss.ssim_view_synthesis_loss(ref['recons'].to(dev), ref['target'].to(dev),
                                    splat_bdry_ignore=0.05, win=7, sigma=1.5)
  l2, _ = kernel(ref['recons'], ref['target'], 2, 1, 7, 1.5, dev)
  assert torch.equal(l, l2)


def test_exact_ties_split_the_gradient(dev):
  """Case a with layer 1 equal to layer 0 and layer 2 worse everywhere."""
  _, _, _, _, _, (x_min, y_min), win, sigma, _ = CASES['a']
  recons, target = make_inputs('a', amps=(0.02, 0.02, 0.12))
  recons[1] = recons[0]
  d = ssim_ref.dssim_maps(recons.double(), target.double(), x_min, y_min, win, sigma)
  assert float((d[2] - d[0]).min()) >= MIN_GAP      # worse in every window
  ref = reference(recons[:1], target, x_min, y_min, win, sigma)
  l, g = kernel(recons, target, x_min, y_min, win, sigma, dev)
  assert torch.equal(g[0], g[1])
  assert float(g[0].abs().max()) > 0
  assert bool((g[2] == 0.0).all())
  check('ties', l, (g[0] + g[1]).unsqueeze(0), ref)


def test_strided_target_gives_the_same_bits(dev):
  from lsi.loss import _hip
  ref = case_reference('a')
  recons, target = ref['recons'].to(dev), ref['target'].to(dev)
  chw = target.permute(0, 3, 1, 2).contiguous()     # stored channels-first
  view = chw.permute(0, 2, 3, 1)                    # viewed as B x H x W x 3
  assert not view.is_contiguous() and torch.equal(view, target)
  a = _hip.ssim_view_synthesis_loss(recons, target, 2, 1, 7, 1.5)
  b = _hip.ssim_view_synthesis_loss(recons, view, 2, 1, 7, 1.5)
  assert torch.equal(a, b)


def test_reproducible(dev):
  ref = case_reference('e')
  _, _, _, _, _, (x_min, y_min), win, sigma, _ = CASES['e']
  runs = [kernel(ref['recons'], ref['target'], x_min, y_min, win, sigma, dev)
          for _ in range(2)]
  assert torch.equal(runs[0][0], runs[1][0])
  assert torch.equal(runs[0][1], runs[1][1])


def test_refusals(dev):
  from lsi.loss import _hip
  ref = case_reference('a')
  recons, target = ref['recons'].to(dev), ref['target'].to(dev)
  before = dict(_hip.CALLS)
  with pytest.raises(ValueError, match='window'):    # 23 - 2 * 9 = 5 rows < 7
    _hip.ssim_view_synthesis_loss(recons, target, 2, 9, 7, 1.5)
  with pytest.raises(ValueError, match='odd'):
    _hip.ssim_view_synthesis_loss(recons, target, 2, 1, 4, 1.5)
  with pytest.raises(RuntimeError, match='not differentiable'):
    _hip.ssim_view_synthesis_loss(recons, target.clone().requires_grad_(True), 2, 1,
                                  7, 1.5)
  assert _hip.CALLS == before                        # nothing was launched
  torch.cuda.synchronize()


def test_metric_accumulates_beside_the_sixteen_slots(dev):
  from lsi.nnutils import eval_metrics
  acc = eval_metrics.MetricAccumulator(dev)
  assert 'ssim' not in acc.sums() and 'ssim' not in acc.results()
  want_sum, want_sum32, want_n = 0.0, 0.0, 0.0
  for name, times in (('b', 2), ('f', 1)):
    ref = case_reference(name)
    s, n = ssim_ref.metric(ref['recons'].double(), ref['target'].double(), 0, 0, 11, 1.5)
    s32, _ = ssim_ref.metric(ref['recons'], ref['target'], 0, 0, 11, 1.5)
    for _ in range(times):
      acc.add_ssim(ref['recons'].to(dev), ref['target'].to(dev), 0.0, win=11,
                   sigma=1.5)
      want_sum, want_sum32, want_n = want_sum + s, want_sum32 + s32, want_n + n
  sums = acc.sums()
  got_sum, got_n = sums.pop('ssim')
  assert got_n == want_n == 2 * 2 * 30 * 60 + 1     # the exact window count
  # the bar of the loss: max(4 x the fp32 restatement's error, 2e-6 relative)
  err = abs(got_sum - want_sum) / abs(want_sum)
  err32 = abs(want_sum32 - want_sum) / abs(want_sum)
  print('ssim metric: sum %.9g want %.9g err kernel %.3g restatement %.3g' %
        (got_sum, want_sum, err, err32))
  assert err <= max(SLACK * err32, LOSS_RTOL)
  assert len(sums) == 9 and all(v == (0.0, 0.0) for v in sums.values())
  assert abs(acc.results()['ssim'] - got_sum / got_n) <= 1e-15
  acc.reset()
  assert acc.sums()['ssim'] == (0.0, 0.0)
  # two identical images: 1
  img = case_reference('b')['target'].to(dev)
  acc.add_ssim(img.unsqueeze(0), img, 0.0)
  assert abs(acc.results()['ssim'] - 1.0) <= 1e-6


# ---------------------------------------------------------------------------
# the training script
# ---------------------------------------------------------------------------
def _trainer(tmp_path, **kw):
  # 128 x 256: the smallest image the U-Net takes (H and W divisible by 128)
  sys.path.insert(0, PKG)
  import ldi_enc_dec as script
  args = ['--dataset', 'kitti', '--kitti_procedural', 'true', '--batch_size', '2',
          '--n_layers', '2', '--img_height', '128', '--img_width', '256', '--num_iter',
          '8', '--log_freq', '1', '--checkpoint_dir', str(tmp_path), '--bf16', 'false']
  for k, v in kw.items():
    args += ['--' + k, str(v)]
  opts = script.apply_dataset_overrides(script.build_parser().parse_args(args))
  torch.manual_seed(0)
  np.random.seed(0)
  tr = script.Trainer(opts)
  tr.setup()
  return tr


SIX = {'self_cons_loss', 'compose_splat_loss', 'indep_splat_loss', 'incr_depth_loss',
       'disp_smoothness_loss', 'total_loss'}


def test_default_step_makes_no_ssim_call(tmp_path, dev):
  from lsi.loss import _hip
  tr = _trainer(tmp_path)
  before = dict(_hip.CALLS)
  _, scalars = tr.train_step()
  torch.cuda.synchronize()
  assert set(scalars) == SIX
  assert _hip.CALLS == before


def test_step_with_ssim_terms(tmp_path, dev, monkeypatch):
  from lsi.loss import _hip, loss
  tr = _trainer(tmp_path, ssim_wt=0.85)
  o = tr.opts
  seen = []
  real = loss.ssim_view_synthesis_loss

  def spy(img, target, bdry, win, sigma):
    seen.append((img.detach().cpu(), target.detach().cpu(), bdry, win, sigma))
    return real(img, target, bdry, win=win, sigma=sigma)

  monkeypatch.setattr(loss, 'ssim_view_synthesis_loss', spy)
  before = dict(_hip.CALLS)
  staged, _ = tr.stage(tr.feed())
  total, scalars = tr.compute_losses(staged)
  assert set(scalars) == SIX | {'compose_ssim_loss', 'indep_ssim_loss'}
  assert _hip.CALLS['ssim_fwd'] - before['ssim_fwd'] == len(seen)
  # paired: one call per term on the 2 B views, twice the mean; else one per
  # direction and term, summed.  Per-layer rendering first, composed second.
  assert len(seen) in (2, 4)
  scale = 2.0 if len(seen) == 2 else 1.0
  want = {'indep_ssim_loss': [0.0, 0.0], 'compose_ssim_loss': [0.0, 0.0]}
  for i, (img, target, bdry, win, sigma) in enumerate(seen):
    assert (bdry, win, sigma) == (o.splat_bdry_ignore, 7, 1.5)
    ht, wt = img.shape[2:4]
    crop = ssim_ref.py2_round(wt * bdry), ssim_ref.py2_round(ht * bdry)
    key = 'indep_ssim_loss' if i % 2 == 0 else 'compose_ssim_loss'
    assert img.shape[0] == (o.n_layers if i % 2 == 0 else 1)
    l64 = float(ssim_ref.loss(img.double(), target.double(), *crop, win, sigma))
    l32 = float(ssim_ref.loss(img, target, *crop, win, sigma))
    want[key][0] += scale * l64
    want[key][1] += scale * abs(l32 - l64)
  for key, (l64, err32) in want.items():
    err = abs(float(scalars[key].detach()) - l64) / l64
    bar = max(SLACK * err32 / l64, LOSS_RTOL)
    print('ssim trainer %s: %.9g want %.9g err %.3g restatement %.3g bar %.3g' %
          (key, float(scalars[key].detach()), l64, err, err32 / l64, bar))
    assert err <= bar, (key, err, bar)
  parts = (o.self_cons_wt * scalars['self_cons_loss'] +
           o.compose_splat_wt * scalars['compose_splat_loss'] +
           o.indep_splat_wt * scalars['indep_splat_loss'] +
           (o.incr_depth_wt / o.max_disp) * scalars['incr_depth_loss'] +
           (o.disp_smoothness_wt / o.max_disp ** 2) * scalars['disp_smoothness_loss'] +
           o.ssim_wt * (o.compose_splat_wt * scalars['compose_ssim_loss'] +
                        o.indep_splat_wt * scalars['indep_ssim_loss']))
  assert abs(float(total) - float(parts)) <= 1e-5 * abs(float(parts))
  # the structural terms alone reach the network's first convolution
  first = next(p for n, p in tr.model.named_parameters() if p.dim() == 4)
  g, = torch.autograd.grad(scalars['compose_ssim_loss'] + scalars['indep_ssim_loss'],
                           first)
  assert bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
  assert _hip.CALLS['ssim_bwd'] - before['ssim_bwd'] == len(seen)


def test_captured_graph_step_reproduces_the_eager_scalars(tmp_path, dev):
  runs = {}
  for mode in ('false', 'true'):
    tr = _trainer(tmp_path / mode, ssim_wt=0.85, hip_graph=mode)
    batch = tr.feed()
    tr.feed = lambda batch=batch: batch
    for _ in range(5):           # 3 eager warm-up steps, the capture, one replay
      _, scalars = tr.train_step()
    torch.cuda.synchronize()
    runs[mode] = {k: float(v) for k, v in scalars.items()}
    if mode == 'true':
      assert tr._graph is not None
  for k in ('compose_ssim_loss', 'indep_ssim_loss', 'total_loss'):
    a, b = runs['false'][k], runs['true'][k]
    assert np.isfinite(b) and b > 0
    # (MIOpen's weight gradients are not run-to-run deterministic: the bar of
    # tests/test_train_gpu.py for the same comparison)
    assert abs(a - b) <= 2e-2 * abs(a), (k, runs)


# ---------------------------------------------------------------------------
# the evaluation script
# ---------------------------------------------------------------------------
def test_eval_ssim_on_both_metric_routes(tmp_path, dev):
  """--eval_ssim adds `ssim` to the results of the op route and of
  --device_metrics; both run lsi_eval_ssim on the same renderings."""
  sys.path.insert(0, PKG)
  import ldi_enc_dec as script
  import ldi_pred_eval as ev
  from lsi.loss import _hip
  from lsi.nnutils import eval_metrics
  argv = ['--dataset', 'synthetic', '--synth_scene', 'planes', '--batch_size', '1',
          '--n_layers', '2', '--img_height', '128', '--img_width', '128',
          '--n_obj_max', '2', '--num_eval_iter', '1', '--random_weights', 'true',
          '--checkpoint_dir', str(tmp_path)]
  res = {}
  for ssim in ('false', 'true'):
    opts = script.apply_dataset_overrides(
        ev.build_parser().parse_args(argv + ['--eval_ssim', ssim]))
    opts.debug_synth_texture = False
    opts.synth_dl_eval_data = True
    torch.manual_seed(0)
    np.random.seed(0)
    tester = ev.Tester(opts)
    tester.restore()
    batch = tester.trainer.data_loader.forward(opts.batch_size)
    before = _hip.CALLS['ssim_eval']
    ops = eval_metrics.aggregate(tester.eval_batch(batch=batch))
    acc = eval_metrics.MetricAccumulator(tester.trainer.device)
    assert tester.eval_batch(batch=batch, acc=acc) == []
    res[ssim] = (ops, acc.results())
    # two views per route
    assert _hip.CALLS['ssim_eval'] - before == (4 if ssim == 'true' else 0)
  assert 'ssim' not in res['false'][0] and 'ssim' not in res['false'][1]
  ops, fused = res['true']
  assert set(ops) == set(fused) == set(res['false'][0]) | {'ssim'}
  print('eval ssim: op route %.9g, device metrics %.9g' % (ops['ssim'], fused['ssim']))
  assert -1.0 <= fused['ssim'] <= 1.0
  # the two routes render separately: the bar of the same comparison for the
  # other metrics (tests/test_eval_fused_gpu.py)
  assert abs(ops['ssim'] - fused['ssim']) <= 2e-4 * abs(ops['ssim'])
