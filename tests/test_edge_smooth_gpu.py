"""The fused edge-aware disparity smoothness loss (csrc/lsi_edge_smooth.hip)
against the fp64 restatement of its definition (tests/edge_smooth_ref.py,
DESIGN.md 4.14).

Bars, the project's own (tests/test_ssim_gpu.py): every comparison first
measures the error of the fp32 op restatement against fp64 on the same inputs
and allows the kernels max(4 x that error, the usual bar) -- 2e-6 relative on a
loss, 1e-5 of the largest entry on a gradient; the factor 4 covers a different
summation order.  The yardstick is always the fp64 restatement.

Condition on the inputs (not a tolerance: nothing is left out): every stencil
value of the fp64 restatement is exactly 0 or at least 1/256 in magnitude.  It
holds by construction -- the disparities are multiples of 1/256 -- so the
kernels and the yardstick take the same sign everywhere; the zeros (a constant
patch, a constant plane, chance) are part of the test: sign(0) = 0."""
import functools
import sys

import numpy as np
import pytest
import torch

import edge_smooth_ref as ref
from conftest import PKG

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_RTOL, SLACK = 2e-6, 1e-5, 4.0
ALPHA, UPSTREAM = 10.0, 2.5

# name: L, B, H, W, per-layer guide, orders
CASES = {
    'a': (3, 2, 13, 37, False, (1, 2)),    # ragged rows
    'b': (2, 3, 40, 150, True, (1, 2)),    # several blocks per plane
    'c': (4, 8, 9, 17, False, (1, 2)),     # 32 planes, the training plane count
    'd': (1, 1, 2, 3, False, (1,)),        # one row of y-, two columns of x-differences
    'e': (2, 2, 3, 70, True, (1, 2)),      # order 2: exactly one row of y-stencils
}
RUNS = [(n, o, norm) for n in sorted(CASES) for o in CASES[n][5]
        for norm in (False, True)]


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def make_inputs(name):
  """(disp L x B x H x W x 1, guide B x H x W x 3 or L x B x H x W x 3) fp32 on the
  CPU.  Disparities k / 256, k in [13, 256]; a constant quarter-plane patch in
  plane (0, 0); for L > 1 plane (1, 0) entirely constant.  Guide: a smooth
  sinusoid plus uniform noise of +-0.2, clamped to [0, 1], its right half
  quantised to {0, 1/2, 1} (exact zero image gradients)."""
  nl, b, h, w, per_layer, _ = CASES[name]
  rng = np.random.RandomState(sum(map(ord, name)))
  disp = rng.randint(13, 257, (nl, b, h, w, 1)).astype(np.float64) / 256.0
  disp[0, 0, :max(h // 2, 1), :max(w // 2, 1)] = 77.0 / 256.0
  if nl > 1:
    disp[1, 0] = 101.0 / 256.0
  lead = (nl, b) if per_layer else (1, b)
  yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
  guide = np.zeros(lead + (h, w, 3))
  for l in range(lead[0]):
    for i in range(b):
      for c in range(3):
        guide[l, i, :, :, c] = 0.5 + 0.3 * np.sin(
            2 * np.pi * ((1.0 + 0.5 * c) * xx / w + (0.75 + 0.25 * i) * yy / h)
            + c + i + 2 * l)
  guide = np.clip(guide + rng.uniform(-0.2, 0.2, guide.shape), 0.0, 1.0)
  guide[..., w // 2:, :] = np.round(guide[..., w // 2:, :] * 2.0) / 2.0
  if not per_layer:
    guide = guide[0]
  return (torch.from_numpy(disp.astype(np.float32)),
          torch.from_numpy(guide.astype(np.float32)))


def reference(disp, guide, alpha, order, normalise):
  """Loss and gradient of (loss * UPSTREAM) from the restatement in fp64 and in
  fp32, on the CPU, and the fp32 restatement's own errors."""
  out = {}
  for dt in (torch.float64, torch.float32):
    l, g = ref.loss_and_grad(disp.to(dt), guide.to(dt), alpha, order, normalise,
                             UPSTREAM)
    out[dt] = (float(l), g.double())
  l64, g64 = out[torch.float64]
  l32, g32 = out[torch.float32]
  return {'loss': l64, 'grad': g64,
          'loss_err32': abs(l32 - l64) / abs(l64),
          'grad_err32': float((g32 - g64).abs().max() / g64.abs().max())}


@functools.lru_cache(maxsize=None)
def case_reference(name, order, normalise):
  """Reference of a run, computed once and shared (read-only)."""
  disp, guide = make_inputs(name)
  r = reference(disp, guide, ALPHA, order, normalise)
  r['stencil'] = ref.min_nonzero_stencil(disp.double(), guide.double(), order)
  return r


def kernel(disp, guide, alpha, order, normalise, dev):
  """(loss, gradient of loss * UPSTREAM w.r.t. disp) from the HIP kernels; disp
  and guide may be device views."""
  from lsi.loss import _hip
  d = disp.to(dev).detach().requires_grad_(True)
  l = _hip.edge_smoothness_loss(d, guide.to(dev), alpha, order, normalise)
  (l * UPSTREAM).backward()
  return l.detach(), d.grad


def check(tag, l, g, r):
  """Prints the measured errors, then holds them against the bars."""
  loss_err = abs(float(l) - r['loss']) / abs(r['loss'])
  grad_err = float((g.cpu().double() - r['grad']).abs().max() / r['grad'].abs().max())
  loss_bar = max(SLACK * r['loss_err32'], LOSS_RTOL)
  grad_bar = max(SLACK * r['grad_err32'], GRAD_RTOL)
  print('edge %s: loss err kernel %.3g restatement %.3g bar %.3g | grad err kernel '
        '%.3g restatement %.3g bar %.3g' % (tag, loss_err, r['loss_err32'], loss_bar,
                                            grad_err, r['grad_err32'], grad_bar))
  assert loss_err <= loss_bar, (tag, loss_err, loss_bar)
  assert grad_err <= grad_bar, (tag, grad_err, grad_bar)


@pytest.mark.parametrize('name,order,normalise', RUNS)
def test_forward_and_gradient(name, order, normalise, dev):
  r = case_reference(name, order, normalise)
  smallest, zeros = r['stencil']
  print('edge %s order %d: smallest non-zero stencil %.3g, %.1f %% exact zeros' %
        (name, order, smallest, 100 * zeros))
  assert smallest >= 1.0 / 256.0 and (zeros > 0.0 or name == 'd')
  disp, guide = make_inputs(name)
  l, g = kernel(disp, guide, ALPHA, order, normalise, dev)
  assert g.shape == disp.shape and bool(torch.isfinite(g).all())
  check('%s o%d n%d' % (name, order, normalise), l, g, r)
  if CASES[name][0] > 1:
    assert bool((g[1, 0] == 0.0).all())          # the wholly constant plane
    assert float(g[0, 0].abs().max()) > 0.0
  if name == 'd':
    assert disp.shape[2] - order == 1 and disp.shape[3] - order == 2
  if name == 'e' and order == 2:
    assert disp.shape[2] - order == 1


def test_public_wrapper(dev):
  from lsi.loss import loss
  disp, guide = make_inputs('a')
  got = loss.edge_aware_smoothness_loss(disp.to(dev), guide.to(dev), alpha=ALPHA)
  l, _ = kernel(disp, guide, ALPHA, 1, True, dev)
  assert torch.equal(got, l)


@pytest.mark.parametrize('order', [1, 2])
def test_reproducible(order, dev):
  disp, guide = make_inputs('b')
  runs = [kernel(disp, guide, ALPHA, order, True, dev) for _ in range(2)]
  assert torch.equal(runs[0][0], runs[1][0])
  assert torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize('order', [1, 2])
def test_strided_inputs_give_the_same_bits(order, dev):
  disp, guide = make_inputs('a')
  disp, guide = disp.to(dev), guide.to(dev)
  want = kernel(disp, guide, ALPHA, order, True, dev)
  # channel 1 of an L x B x H x W x 2 tensor
  two = torch.stack([torch.full_like(disp[..., 0], 7.0), disp[..., 0]], dim=-1)
  view = two[..., 1:]
  assert not view.is_contiguous() and torch.equal(view, disp)
  got = kernel(view, guide, ALPHA, order, True, dev)
  assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
  # a guide stored channels-first, viewed as B x H x W x 3
  chw = guide.permute(0, 3, 1, 2).contiguous()
  gview = chw.permute(0, 2, 3, 1)
  assert not gview.is_contiguous() and torch.equal(gview, guide)
  got = kernel(disp, gview, ALPHA, order, True, dev)
  assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
  # the shared guide expanded to L x B x ...: as a stride-0 view and as a copy
  expanded = guide.unsqueeze(0).expand(disp.shape[0], -1, -1, -1, -1)
  for g5 in (expanded, expanded.contiguous()):
    got = kernel(disp, g5, ALPHA, order, True, dev)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_alpha_zero_is_the_unweighted_mean(dev):
  disp, guide = make_inputs('a')
  sx, sy, _, _ = ref.stencils(disp.double(), guide.double(), 1)
  want = float(sx.abs().mean() + sy.abs().mean())
  r = reference(disp, guide, 0.0, 1, False)
  assert abs(r['loss'] - want) <= 1e-14 * want
  l, g = kernel(disp, guide, 0.0, 1, False, dev)
  check('alpha 0', l, g, r)
  assert abs(float(l) - want) <= max(SLACK * r['loss_err32'], LOSS_RTOL) * want


def test_refusals(dev):
  from lsi.loss import _hip
  disp, guide = make_inputs('a')
  disp, guide = disp.to(dev), guide.to(dev)
  before = dict(_hip.CALLS)
  with pytest.raises(ValueError, match='rows'):              # 2 rows < 3
    _hip.edge_smoothness_loss(disp[:, :, :2], guide[:, :2], ALPHA, 2, True)
  with pytest.raises(ValueError, match='order'):
    _hip.edge_smoothness_loss(disp, guide, ALPHA, 3, True)
  with pytest.raises(ValueError, match='alpha'):
    _hip.edge_smoothness_loss(disp, guide, -1.0, 1, True)
  with pytest.raises(ValueError, match='guide'):             # batch 1 against 2
    _hip.edge_smoothness_loss(disp, guide[:1], ALPHA, 1, True)
  with pytest.raises(ValueError, match='guide'):             # 4 channels
    _hip.edge_smoothness_loss(disp, torch.cat([guide, guide[..., :1]], -1), ALPHA, 1,
                              True)
  with pytest.raises(RuntimeError, match='not differentiable'):
    _hip.edge_smoothness_loss(disp, guide.clone().requires_grad_(True), ALPHA, 1, True)
  assert _hip.CALLS == before                                # nothing was launched
  torch.cuda.synchronize()


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


def test_default_step_makes_no_edge_call(tmp_path, dev):
  from lsi.loss import _hip
  tr = _trainer(tmp_path)
  before = dict(_hip.CALLS)
  _, scalars = tr.train_step()
  torch.cuda.synchronize()
  assert set(scalars) == SIX
  assert _hip.CALLS == before


@pytest.mark.parametrize('guide_kind', ['image', 'texture'])
def test_step_with_the_edge_term(guide_kind, tmp_path, dev, monkeypatch):
  from lsi.loss import _hip, loss
  tr = _trainer(tmp_path, edge_smooth_wt=0.1, edge_smooth_alpha=10,
                edge_smooth_guide=guide_kind)
  o = tr.opts
  seen = []
  real = loss.edge_aware_smoothness_loss

  def spy(disp, guide, alpha, order, normalise):
    seen.append((disp.detach().cpu(), guide.detach().cpu(), guide.requires_grad,
                 alpha, order, normalise))
    return real(disp, guide, alpha=alpha, order=order, normalise=normalise)

  monkeypatch.setattr(loss, 'edge_aware_smoothness_loss', spy)
  before = dict(_hip.CALLS)
  staged, _ = tr.stage(tr.feed())
  total, scalars = tr.compute_losses(staged)
  assert set(scalars) == SIX | {'edge_smooth_loss'}
  assert _hip.CALLS['edge_fwd'] - before['edge_fwd'] == len(seen)
  # paired: one call on the 2 B views, twice the mean; else one per view, summed
  assert len(seen) in (1, 2)
  scale = 2.0 if len(seen) == 1 else 1.0
  l64, err32 = 0.0, 0.0
  for disp, guide, guide_grad, alpha, order, normalise in seen:
    assert (alpha, order, normalise) == (10.0, 1, True)
    assert not guide_grad                  # no gradient path through the guide
    assert disp.shape[0] == o.n_layers and disp.shape[2:] == (128, 256, 1)
    assert guide.dim() == (5 if guide_kind == 'texture' else 4)
    assert guide.shape[-4:] == disp.shape[1:4] + (3,)
    a = float(ref.loss(disp.double(), guide.double(), alpha, order, normalise))
    b = float(ref.loss(disp, guide, alpha, order, normalise))
    l64 += scale * a
    err32 += scale * abs(b - a)
  got = float(scalars['edge_smooth_loss'].detach())
  err, bar = abs(got - l64) / l64, max(SLACK * err32 / l64, LOSS_RTOL)
  print('edge trainer (%s): %.9g want %.9g err %.3g restatement %.3g bar %.3g' %
        (guide_kind, got, l64, err, err32 / l64, bar))
  assert err <= bar, (err, bar)
  parts = (o.self_cons_wt * scalars['self_cons_loss'] +
           o.compose_splat_wt * scalars['compose_splat_loss'] +
           o.indep_splat_wt * scalars['indep_splat_loss'] +
           (o.incr_depth_wt / o.max_disp) * scalars['incr_depth_loss'] +
           (o.disp_smoothness_wt / o.max_disp ** 2) * scalars['disp_smoothness_loss'] +
           o.edge_smooth_wt * scalars['edge_smooth_loss'])
  assert abs(float(total) - float(parts)) <= 1e-5 * abs(float(parts))
  # the term alone reaches the network's first convolution
  first = next(p for n, p in tr.model.named_parameters() if p.dim() == 4)
  g, = torch.autograd.grad(scalars['edge_smooth_loss'], first, retain_graph=True)
  assert bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
  assert _hip.CALLS['edge_bwd'] - before['edge_bwd'] == len(seen)
  # ... and, whatever guides it, not the predicted textures
  pair = getattr(tr.model, 'pair_ldi', None)
  if pair is not None and pair[0].requires_grad:
    g_tex, = torch.autograd.grad(scalars['edge_smooth_loss'], pair[0],
                                 retain_graph=True, allow_unused=True)
    assert g_tex is None or float(g_tex.abs().max()) == 0.0


def test_unnormalised_term_is_divided_by_max_disp(tmp_path, dev):
  tr = _trainer(tmp_path, edge_smooth_wt=0.1, edge_smooth_norm='false',
                edge_smooth_order=2)
  o = tr.opts
  staged, _ = tr.stage(tr.feed())
  total, s = tr.compute_losses(staged)
  parts = (o.self_cons_wt * s['self_cons_loss'] +
           o.compose_splat_wt * s['compose_splat_loss'] +
           o.indep_splat_wt * s['indep_splat_loss'] +
           (o.incr_depth_wt / o.max_disp) * s['incr_depth_loss'] +
           (o.disp_smoothness_wt / o.max_disp ** 2) * s['disp_smoothness_loss'] +
           (o.edge_smooth_wt / o.max_disp) * s['edge_smooth_loss'])
  assert float(s['edge_smooth_loss']) > 0
  assert abs(float(total) - float(parts)) <= 1e-5 * abs(float(parts))


def test_captured_graph_step_reproduces_the_eager_scalars(tmp_path, dev):
  runs = {}
  for mode in ('false', 'true'):
    tr = _trainer(tmp_path / mode, edge_smooth_wt=0.1, edge_smooth_alpha=10,
                  hip_graph=mode)
    batch = tr.feed()
    tr.feed = lambda batch=batch: batch
    for _ in range(5):           # 3 eager warm-up steps, the capture, one replay
      _, scalars = tr.train_step()
    torch.cuda.synchronize()
    runs[mode] = {k: float(v) for k, v in scalars.items()}
    if mode == 'true':
      assert tr._graph is not None
  for k in ('edge_smooth_loss', 'total_loss'):
    a, b = runs['false'][k], runs['true'][k]
    assert np.isfinite(b) and b > 0
    # (MIOpen's weight gradients are not run-to-run deterministic: the bar of
    # tests/test_train_gpu.py for the same comparison)
    assert abs(a - b) <= 2e-2 * abs(a), (k, runs)
