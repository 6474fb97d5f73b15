"""The SSIM kernels (csrc/lsi_ssim.hip) against the float32 restatement of their
own arithmetic, tests/ssim_exact_ref.py: the gradient with `==` on every element,
the loss and the metric inside the interval that the device's fp64 sum of the
restated per-thread fp32 partial sums may round to ("Held to exact
tests").  No tolerance anywhere.  tests/test_ssim_exact_cpu.py holds the
restatement to the fp64 definition and checks, from the shapes, that the cases
reach the paths they are named after: the tile stride loops of both kernels
(more than 2048 tiles), the backward's zero branch, ragged tiles, every window
size, exact ties and near ties of the best layer."""
import numpy as np
import pytest
import torch

import ssim_exact_ref as X

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def device_inputs(name, dev):
  case = X.CASES[name]
  recons, target = (torch.from_numpy(a.copy()).to(dev) for a in X.inputs(name))
  if case.chw:                      # stored channels-first, viewed as B x H x W x 3
    target = target.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert not target.is_contiguous()
  return recons, target


def kernel(name, dev):
  """(loss, gradient of loss * upstream, the metric's two doubles)."""
  from lsi.loss import _hip
  from lsi.nnutils import _hip_eval
  case = X.CASES[name]
  recons, target = device_inputs(name, dev)
  args = (case.x_min, case.y_min, case.win, case.sigma)
  r = recons.clone().requires_grad_(True)
  l = _hip.ssim_view_synthesis_loss(r, target, *args)
  (l * case.upstream).backward()
  acc2 = torch.zeros((2,), dtype=torch.float64, device=dev)
  _hip_eval.ssim_metric(acc2, recons, target, *args)
  return l.detach(), r.grad, acc2


def assert_gradient_equal(name, got, want):
  """By value (the sign of a zero is not compared); the first differing element
  with both values and its backward tile."""
  got = got.cpu().numpy()
  assert got.shape == want.shape and got.dtype == want.dtype == F
  diff = got != want
  if diff.any():
    idx = tuple(int(i) for i in np.argwhere(diff)[0])
    b, ty, tx, tile = X.bwd_tile_of(idx, want.shape)
    grid = X.geometry(*[X.CASES[name][i] for i in (0, 1, 2, 3, 6, 7, 8)])['bwd_grid']
    pytest.fail('%s: %d of %d gradient elements differ; first at (l, b, y, x, c) = %s: '
                'kernel %r (0x%08x) restatement %r (0x%08x); backward tile %d (image %d, '
                'tile row %d, tile column %d), block %d, pass %d'
                % (name, int(diff.sum()), diff.size, idx, float(got[idx]),
                   int(got[idx].view(np.uint32)), float(want[idx]),
                   int(want[idx].view(np.uint32)), tile, b, ty, tx, tile % grid,
                   tile // grid))


def assert_loss_in_interval(name, l, r):
  lo, hi = X.interval(r['loss_partials'], r['windows'])
  ends = X.float32_ends(lo, hi)
  print('ssim exact %s: loss %.9g, allowed %s' % (name, float(l), sorted(ends)))
  assert l.dtype == torch.float32 and float(l) in ends, (name, float(l), sorted(ends))


def assert_metric_in_interval(name, acc2, r, calls=1):
  """The fp64 sum within (m + 1) 2^-53 relative per call, the count with ==."""
  got_sum, got_n = acc2.tolist()
  lo, hi = X.interval(r['metric_partials'])
  print('ssim exact %s: metric sum %.17g in [%.17g, %.17g], count %d' %
        (name, got_sum, calls * float(lo), calls * float(hi), got_n))
  assert got_n == calls * r['windows']
  assert calls * lo <= got_sum <= calls * hi, (name, got_sum, float(lo), float(hi))


@pytest.mark.parametrize('name', list(X.CASES))
def test_gradient_loss_and_metric(name, dev):
  r = X.restated(name)
  l, g, acc2 = kernel(name, dev)
  assert bool(torch.isfinite(g).all())
  assert_gradient_equal(name, g, r['grad'])
  assert_loss_in_interval(name, l, r)
  assert_metric_in_interval(name, acc2, r)
  if r['windows'] == 1:     # the loss is d bit for bit, the metric the mean S widened
    assert float(l) == float(r['d'].ravel()[0])
    assert acc2.tolist() == [float(r['s_mean'].ravel()[0]), 1.0]
  # twice: the same bits
  l2, g2, acc2b = kernel(name, dev)
  assert torch.equal(l, l2) and torch.equal(g, g2) and torch.equal(acc2, acc2b)


def test_metric_reads_layer_zero_of_any(dev):
  """A 3-layer recons scores as its layer 0 alone; two calls accumulate; the 16
  slots of the accumulator stay untouched."""
  from lsi.nnutils import _hip_eval, eval_metrics
  name = 'ties'
  case, r = X.CASES[name], X.restated(name)
  recons, target = device_inputs(name, dev)
  assert recons.shape[0] == 3 and not torch.equal(recons[0], recons[2])
  args = (case.x_min, case.y_min, case.win, case.sigma)
  three = torch.zeros((2,), dtype=torch.float64, device=dev)
  one = torch.zeros((2,), dtype=torch.float64, device=dev)
  _hip_eval.ssim_metric(three, recons, target, *args)
  _hip_eval.ssim_metric(one, recons[:1], target, *args)
  assert torch.equal(three, one)
  assert_metric_in_interval(name, three, r)
  first = three.clone()
  _hip_eval.ssim_metric(three, recons, target, *args)
  assert torch.equal(three, first + first)           # s + s and n + n are exact
  assert_metric_in_interval(name, three, r, calls=2)
  # through the accumulator (crop 0 there: the restatement of that call)
  acc = eval_metrics.MetricAccumulator(dev)
  acc.add_ssim(recons, target, 0.0, win=case.win, sigma=case.sigma)
  acc.add_ssim(recons, target, 0.0, win=case.win, sigma=case.sigma)
  sums = acc.sums()
  got_sum, got_n = sums.pop('ssim')
  r0 = X.restate(*X.inputs(name), 0, 0, case.win, case.sigma, gradient=False)
  lo, hi = X.interval(r0['metric_partials'])
  assert got_n == 2 * r0['windows'] and 2 * lo <= got_sum <= 2 * hi
  assert len(sums) == 9 and all(v == (0.0, 0.0) for v in sums.values())
  assert bool((acc.acc == 0).all()) and acc.acc.numel() == _hip_eval.SLOT_COUNT == 16
