"""The fused sparse depth-supervision loss (csrc/lsi_depth_sup.hip) against the
fp64 restatement of its definition (tests/depth_sup_ref.py).

Bars, the project's own (tests/test_edge_smooth_gpu.py): every comparison first
measures the error of the fp32 op restatement against fp64 on the same inputs
and allows the kernels max(4 x that error, the usual bar) -- 2e-6 relative on a
loss, 1e-5 of the largest entry on a gradient; the factor 4 covers a different
summation order.  The yardstick is always the fp64 restatement.

Condition on the inputs (not a tolerance: nothing is left out): gt, gt_scale
(powers of two >= 1) and pred are such that g and pred are multiples of 1/256,
so in l1 mode every e_i of a free pixel is exactly 0 or at least 1/256 in
magnitude and the kernels and the yardstick take the same sign; the zeros
(planted pred == g) are part of the test: sign(0) = 0.  Which pixels are scored
is decided in fp32 by both sides from exactly representable values.

Shapes a - g are the issue's; h and i are added because none of a - g has rows
whose base is 16-byte aligned: h (W = 72) takes the 16-byte loads and stores,
i (W = 70 in rows of stride 72) the 16-byte loads with a ragged row end."""
import ctypes
import functools
import sys

import numpy as np
import pytest
import torch

import depth_sup_ref as ref
from conftest import PKG

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_RTOL, SLACK = 2e-6, 1e-5, 4.0
UPSTREAM = 2.5
EPS = 1e-6
G_MIN = float(np.float32(1.0) / np.float32(80.0))
G_MAX = float(np.float32(1.0) / np.float32(1e-3))
KW = dict(valid_above=0.0, g_min=G_MIN, g_max=G_MAX, eps=EPS)
SCALES = (2.0, 1.0, 4.0)
EINVAL, ENULL, EWORKSPACE = -1, -2, -3

# name: P, H, W
SHAPES = {
    'a': (3, 13, 37),     # ragged rows, one block per plane
    'b': (2, 40, 150),    # several blocks per plane
    'c': (8, 9, 17),      # the training plane count
    'd': (1, 1, 1),       # one pixel, scored
    'e': (4, 5, 70),      # plane 1 empty, plane 2 one pixel, plane 3 at 5 %
    'f': (3, 13, 37),     # a's values: pred planes apart, gt at x-stride 2
    'g': (3, 13, 37),     # all planes empty
    'h': (2, 24, 72),     # aligned rows: 16-byte loads and stores, 2 blocks per plane
    'i': (4, 5, 70),      # e's values in rows of stride 72: 16-byte loads, ragged end
}
VALUES = {'f': 'a', 'i': 'e'}    # layouts of another shape's values
RUNS = [(n, m, lam, (i + j + k) % 2 == 1)
        for i, n in enumerate(sorted(SHAPES)) for j, m in enumerate(ref.MODES)
        for k, lam in enumerate((0.0, 0.5, 1.0))]


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def make_inputs(name, scaled):
  """(pred P x H x W, gt P x H x W, gt_scale P or None) fp32 NumPy.  pred and gt
  are k / 256, k in [13, 256].  Planted per plane (planes of 16 pixels or more),
  at distinct random pixels: ground-truth holes 0, NaN, 1/1024 (below g_min at
  every scale) and 4096 (above g_max); at scored pixels predictions 0, -1/2, NaN
  and exactly eps; two pixels with pred == g."""
  name = VALUES.get(name, name)
  p, h, w = SHAPES[name]
  n = h * w
  rng = np.random.RandomState(sum(map(ord, name)) + 7 * scaled)
  gt = (rng.randint(13, 257, (p, n)) / 256.0).astype(np.float32)
  pred = (rng.randint(13, 257, (p, n)) / 256.0).astype(np.float32)
  scale = (np.array([SCALES[i % 3] for i in range(p)], np.float32) if scaled
           else None)
  if n == 1:
    gt[:], pred[:] = 100.0 / 256, 50.0 / 256
  for pl in range(p if n >= 16 else 0):
    idx = rng.permutation(n)
    gt[pl, idx[:4]] = (0.0, np.nan, 1.0 / 1024, 4096.0)
    pred[pl, idx[4:8]] = (0.0, -0.5, np.nan, np.float32(EPS))
    pred[pl, idx[8:10]] = gt[pl, idx[8:10]] * (scale[pl] if scaled else 1.0)
    one = idx[10]
    # planes that are emptied keep their unscorable plants
    keep = ~((gt[pl] >= 13.0 / 256) & (gt[pl] <= 1.0))
    if name == 'g' or (name == 'e' and pl in (1, 2)):
      gt[pl] = np.where(keep, gt[pl], 0.0)
      if name == 'e' and pl == 2:
        gt[pl, one] = 100.0 / 256
    elif name == 'e' and pl == 3:
      gt[pl] = np.where(keep | (rng.uniform(size=n) < 0.05), gt[pl], 0.0)
  return pred.reshape(p, h, w), gt.reshape(p, h, w), scale


@functools.lru_cache(maxsize=None)
def case_reference(name, mode, lam, scaled):
  """Reference of a run, computed once and shared (read-only): loss and gradient
  of (loss * UPSTREAM) in fp64, the plane sums, which pixels are scored / free,
  and the fp32 op restatement's own errors."""
  pred, gt, scale = make_inputs(name, scaled)
  l64, g64, sums = ref.loss_and_grad(pred, gt, scale, mode, lam, upstream=UPSTREAM,
                                     **KW)
  t = lambda a: None if a is None else torch.from_numpy(a)
  l32, g32 = ref.loss_and_grad_ops(t(pred), t(gt), t(scale), mode, lam,
                                   upstream=UPSTREAM, **KW)
  ok, g = ref.scored(gt, scale, KW['valid_above'], G_MIN, G_MAX)
  q, above = ref.clamp(pred, EPS)
  gmax = np.abs(g64).max()
  return {'loss': l64, 'grad': g64, 'sums': sums, 'ok': ok, 'free': ok & above,
          'e': np.where(ok, q.astype(np.float64) - g, 0.0),
          'loss_err32': abs(l32 - l64) / abs(l64) if l64 else abs(l32),
          'grad_err32': float(np.abs(g32 - g64).max() / gmax) if gmax else
                        float(np.abs(g32).max())}


def same(a, b):
  """torch.equal with NaN equal to NaN (the inputs hold planted NaNs)."""
  return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def on_device(name, scaled, dev):
  """The inputs on the device in the layout the shape asks for."""
  pred, gt, scale = (None if a is None else torch.from_numpy(a).to(dev)
                     for a in make_inputs(name, scaled))
  p, h, w = pred.shape
  if name == 'f':
    # layer 0 of a P x L x H x W buffer (L = 3): the planes lie apart
    buf = torch.full((p, 3, h, w), 7.0, device=dev)
    buf[:, 0] = pred
    pview = buf[:, 0]
    wide = torch.full((p, h, 2 * w), 7.0, device=dev)
    wide[:, :, ::2] = gt
    gview = wide[:, :, ::2]
    assert pview.stride() == (3 * h * w, w, 1) and gview.stride() == (2 * h * w, 2 * w, 2)
    assert same(pview, pred) and same(gview, gt) and not pview.is_contiguous()
    pred, gt = pview, gview
  if name == 'i':
    views = []
    for t in (pred, gt):
      buf = torch.full((p, h, 72), 7.0, device=dev)
      buf[:, :, :w] = t
      views.append(buf[:, :, :w])
      assert views[-1].stride() == (h * 72, 72, 1) and same(views[-1], t)
    pred, gt = views
  return pred, gt, scale


def kernel(pred, gt, scale, mode, lam):
  """(loss, gradient of loss * UPSTREAM w.r.t. pred, plane sums) from the HIP
  kernels; pred and gt may be device views."""
  from lsi.loss import _hip
  x = pred.detach().requires_grad_(True)
  l, sums = _hip.depth_supervision_loss(x, gt, scale, mode, lam, KW['valid_above'],
                                        G_MIN, G_MAX, EPS, return_plane_sums=True)
  g, = torch.autograd.grad(l * UPSTREAM, x)
  return l.detach(), g, sums


def check(tag, l, g, r):
  """Prints the measured errors, then holds them against the bars."""
  l, g = float(l), g.cpu().double().numpy()
  gmax = np.abs(r['grad']).max()
  loss_err = abs(l - r['loss']) / abs(r['loss']) if r['loss'] else abs(l)
  grad_err = float(np.abs(g - r['grad']).max() / gmax) if gmax else float(np.abs(g).max())
  loss_bar = max(SLACK * r['loss_err32'], LOSS_RTOL)
  grad_bar = max(SLACK * r['grad_err32'], GRAD_RTOL)
  print('depth_sup %s: loss %.9g err kernel %.3g restatement %.3g bar %.3g | grad err '
        'kernel %.3g restatement %.3g bar %.3g' %
        (tag, l, loss_err, r['loss_err32'], loss_bar, grad_err, r['grad_err32'],
         grad_bar))
  assert loss_err <= loss_bar, (tag, loss_err, loss_bar)
  assert grad_err <= grad_bar, (tag, grad_err, grad_bar)


def test_the_inputs_hold_what_they_should():
  for name in sorted(SHAPES):
    for scaled in (False, True):
      pred, gt, scale = make_inputs(name, scaled)
      assert pred.shape == gt.shape == SHAPES[name]
      ok, g = ref.scored(gt, scale, 0.0, G_MIN, G_MAX)
      n = ok.reshape(ok.shape[0], -1).sum(1)
      if name == 'd':
        assert n.tolist() == [1]
        continue
      for pl in range(pred.shape[0]):
        assert (gt[pl] == 0).any() and np.isnan(gt[pl]).any()
        with np.errstate(invalid='ignore'):
          assert ((gt[pl] > 0) & (g[pl] < G_MIN)).any() and (g[pl] > G_MAX).any()
        for planted in (pred[pl] == 0, pred[pl] < 0, np.isnan(pred[pl]),
                        pred[pl] == np.float32(EPS)):
          assert planted.any()
          if VALUES.get(name, name) not in ('e', 'g') or (name in 'ei' and pl == 0):
            assert (planted & ok[pl]).sum() == 1      # at a scored pixel
      if VALUES.get(name, name) == 'e':
        assert n[1] == 0 and n[2] == 1 and 0.02 * 350 <= n[3] <= 0.09 * 350
        assert n[0] == 350 - 4
      elif name == 'g':
        assert not n.any()
      else:
        assert (n == ok[0].size - 4).all()
      # g and pred on the 1/256 lattice; pred == g planted at scored pixels
      fin = np.isfinite(pred) & (pred > 0.01)
      assert (pred[fin] * 256 == np.round(pred[fin] * 256)).all()
      assert (g[ok] * 256 == np.round(g[ok] * 256)).all()
      if name != 'g':
        assert ((pred == g) & ok).sum() >= 2


@pytest.mark.parametrize('name,mode,lam,scaled', RUNS)
def test_forward_and_gradient(name, mode, lam, scaled, dev):
  r = case_reference(name, mode, lam, scaled)
  pred, gt, scale = on_device(name, scaled, dev)
  l, g, sums = kernel(pred, gt, scale, mode, lam)
  assert g.shape == pred.shape and g.is_contiguous()
  assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(l))
  assert bool(torch.isfinite(sums).all())
  sums = sums.cpu().numpy().reshape(-1, 3)
  # the counts exactly, the sums to the forward's bar
  assert np.array_equal(sums[:, 0], r['sums'][:, 0])
  scale_ = np.abs(r['sums'][:, 1:]).max()
  if scale_:
    err = np.abs(sums[:, 1:] - r['sums'][:, 1:]).max() / scale_
    assert err <= max(SLACK * r['loss_err32'], LOSS_RTOL), err
  else:
    assert not sums[:, 1:].any()
  gc = g.cpu().numpy()
  # pixels that are not scored, or are clamped at eps: exactly 0
  assert not gc[~r['free']].any()
  if mode == 'l1':
    # the lattice: every free e is 0 or at least 1/256; sign(0) = 0 exactly
    e = r['e'][r['free']]
    assert ((e == 0) | (np.abs(e) >= 1.0 / 256)).all()
    zero = r['free'] & (r['e'] == 0)
    assert name in 'dg' or zero.sum() >= 2
    assert not gc[zero].any()
    assert (np.sign(gc) == np.sign(np.where(r['free'], r['e'], 0.0))).all()
  if name == 'g':
    assert float(l) == 0.0 and not gc.any()        # S = 0: exactly nothing
  if VALUES.get(name, name) == 'e':
    assert sums[:, 0].tolist()[1:3] == [0.0, 1.0] and not gc[1].any()
  check('%s %s lam %g scale %d' % (name, mode, lam, scaled), l, g, r)


@pytest.mark.parametrize('name', ['f', 'i'])
@pytest.mark.parametrize('mode', ref.MODES)
def test_strided_inputs_give_the_same_bits(name, mode, dev):
  pred, gt, scale = on_device(name, True, dev)
  want = kernel(pred.contiguous(), gt.contiguous(), scale, mode, 0.5)
  got = kernel(pred, gt, scale, mode, 0.5)
  for a, b in zip(got, want):
    assert torch.equal(a, b)
  # layer 0 of the trainer's buffer: L x B x H x W x 1 with the channel innermost
  p, h, w = pred.shape
  rgbd = torch.full((p, h, w, 2, 4), 7.0, device=dev)
  rgbd[:, :, :, 0, 3] = pred
  view = rgbd.permute(3, 0, 1, 2, 4)[0, ..., 3]
  assert view.stride() == (h * w * 8, w * 8, 8) and same(view, pred)
  got = kernel(view, gt, scale, mode, 0.5)
  for a, b in zip(got, want):
    assert torch.equal(a, b)


@pytest.mark.parametrize('mode', ref.MODES)
def test_reproducible(mode, dev):
  pred, gt, scale = on_device('b', True, dev)
  runs = [kernel(pred, gt, scale, mode, 0.5) for _ in range(2)]
  for a, b in zip(*runs):
    assert torch.equal(a, b)


def test_public_wrapper(dev):
  from lsi.loss import loss
  pred, gt, scale = on_device('a', True, dev)
  for mode in ref.MODES:
    want, g_want, _ = kernel(pred, gt, scale, mode, 0.5)
    # [..., H, W, 1] with two leading dimensions: 1 x 3 planes
    x = pred[None, ..., None].clone().requires_grad_(True)
    got = loss.depth_supervision_loss(x, gt[None, ..., None], scale, mode=mode)
    assert torch.equal(got.detach(), want)
    (got * UPSTREAM).backward()
    assert x.grad.shape == x.shape and torch.equal(x.grad[0, ..., 0], g_want)
  # the defaults: silog, lambda 1/2, 1e-3 .. 80 m, eps 1e-6
  got = loss.depth_supervision_loss(pred, gt)
  want, _, _ = kernel(pred, gt, None, 'silog', 0.5)
  assert torch.equal(got, want)
  # valid_above is the ground truth's own: everything at or below 1/2 is a hole
  got = loss.depth_supervision_loss(pred, gt, valid_above=0.5)
  want = ref.loss(*make_inputs('a', True)[:2], None, 'silog', 0.5, 0.5, G_MIN, G_MAX,
                  EPS)
  assert abs(float(got) - want) <= 1e-5 * want


def test_refusals_come_in_order_and_launch_nothing(dev):
  from lsi import _C
  from lsi.loss import _hip
  lib = _C.lib()
  pred, gt, scale = on_device('a', True, dev)
  d = _hip.depth_sup_desc(pred, gt, scale, 'silog', 0.5, 0.0, G_MIN, G_MAX, EPS, 't')
  n = int(lib.lsi_depth_sup_workspace_bytes(ctypes.byref(d)))
  assert n == (3 * 3 * 1 + 3) * 8
  out = torch.full((), -7.0, device=dev)
  sums = torch.full((9,), -7.0, dtype=torch.float64, device=dev)
  ws = torch.full((n // 8,), -7.0, dtype=torch.float64, device=dev)
  g_loss = torch.full((), UPSTREAM, device=dev)
  g_pred = torch.full(pred.shape, -7.0, device=dev)
  ptr = _C.ptr

  def fwd(desc, p=pred, g=gt, o=out, s=sums, w=ws, nbytes=n):
    return lib.lsi_depth_sup_loss_fwd(ctypes.byref(desc), ptr(p), ptr(g), ptr(scale),
                                      ptr(o), ptr(s), ptr(w), nbytes, None)

  def bwd(desc, p=pred, g=gt, s=sums, gl=g_loss, gp=g_pred):
    return lib.lsi_depth_sup_loss_bwd(ctypes.byref(desc), ptr(p), ptr(g), ptr(scale),
                                      ptr(s), ptr(gl), ptr(gp), None)

  def bad(**kw):
    b = _hip.depth_sup_desc(pred, gt, scale, 'silog', 0.5, 0.0, G_MIN, G_MAX, EPS, 't')
    for k, v in kw.items():
      setattr(b, k, v)
    return b

  for kw in (dict(mode=2), dict(P=0), dict(H=-1), dict(g_min=0.0),
             dict(g_max=G_MIN / 2), dict(valid_above=-1.0), dict(eps=0.0),
             dict(lam=1.5), dict(lam=float('nan')), dict(g_max=float('inf'))):
    b = bad(**kw)
    assert lib.lsi_depth_sup_workspace_bytes(ctypes.byref(b)) == 0, kw
    # a bad descriptor first: before the NULL pointer and the short workspace
    assert fwd(b, p=None, nbytes=0) == EINVAL and bwd(b, p=None) == EINVAL, kw
  # then a NULL pointer, before the short workspace
  for null in ('p', 'g', 'o', 's', 'w'):
    assert fwd(d, **{null: None}, nbytes=0) == ENULL, null
  for null in ('p', 'g', 's', 'gl', 'gp'):
    assert bwd(d, **{null: None}) == ENULL, null
  # then the workspace
  assert fwd(d, nbytes=n - 1) == EWORKSPACE
  torch.cuda.synchronize()
  # nothing was launched: no output was touched
  for t in (out, sums, ws, g_pred):
    assert bool((t == -7.0).all())
  # ... and the same arguments, complete, run (gt_scale may be NULL)
  assert fwd(d) == 0 and bwd(d) == 0
  assert lib.lsi_depth_sup_loss_fwd(ctypes.byref(d), ptr(pred), ptr(gt), None, ptr(out),
                                    ptr(sums), ptr(ws), n, None) == 0
  torch.cuda.synchronize()
  assert bool(torch.isfinite(g_pred).all()) and float(out) > 0


def test_capture_in_a_graph_and_replay_on_new_values(dev):
  """Forward and backward at shape a, recorded in one graph on one stream, then
  replayed on other values: bit for bit what the eager calls give."""
  from lsi.loss import _hip
  first = on_device('a', True, dev)
  other = on_device('a', False, dev)        # other values (another seed), no NaN lost
  scale = first[2]
  for mode in ref.MODES:
    pred_s = first[0].clone().requires_grad_(True)
    gt_s = first[1].clone()

    def step():
      l = _hip.depth_supervision_loss(pred_s, gt_s, scale, mode, 0.5, 0.0, G_MIN,
                                      G_MAX, EPS)
      g, = torch.autograd.grad(l * UPSTREAM, pred_s)
      return l, g

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      step()                                  # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
      l_s, g_s = step()
    with torch.no_grad():
      pred_s.copy_(other[0])
      gt_s.copy_(other[1])
    graph.replay()
    torch.cuda.synchronize()
    l, g, _ = kernel(other[0], other[1], scale, mode, 0.5)
    assert torch.equal(l_s, l) and torch.equal(g_s, g)
    assert not torch.equal(g, kernel(first[0], first[1], scale, mode, 0.5)[1])


# ---------------------------------------------------------------------------
# the training script
# ---------------------------------------------------------------------------
def _trainer(tmp_path, *extra):
  # 128 x 128, one pair: the smallest planar-scene run of tests/test_train_gpu.py
  sys.path.insert(0, PKG)
  import ldi_enc_dec as script
  argv = ['--dataset', 'synthetic', '--synth_scene', 'planes', '--batch_size', '1',
          '--n_layers', '2', '--img_height', '128', '--img_width', '128',
          '--n_obj_max', '2', '--checkpoint_dir', str(tmp_path), '--bf16', 'false',
          '--log_freq', '1000000', '--save_latest_freq', '1000000',
          '--checkpoint_freq', '1000000'] + list(extra)
  opts = script.apply_dataset_overrides(script.build_parser().parse_args(argv))
  torch.manual_seed(0)
  np.random.seed(0)
  tr = script.Trainer(opts)
  tr.setup()
  return tr


SIX = {'self_cons_loss', 'compose_splat_loss', 'indep_splat_loss', 'incr_depth_loss',
       'disp_smoothness_loss', 'total_loss'}


def test_training_steps_with_the_term(tmp_path, dev, monkeypatch):
  from lsi.loss import _hip, loss
  tr = _trainer(tmp_path, '--depth_sup_wt', '1')
  o = tr.opts
  seen = []
  real = loss.depth_supervision_loss

  def spy(pred, gt, gt_scale=None, **kw):
    seen.append((pred.detach().cpu().numpy(), gt.detach().cpu().numpy(), gt_scale, kw,
                 pred.shape, pred.stride(), pred.data_ptr()))
    return real(pred, gt, gt_scale, **kw)

  monkeypatch.setattr(loss, 'depth_supervision_loss', spy)
  before = dict(_hip.CALLS)
  staged, _ = tr.stage(tr.feed())
  assert len(staged) == 5 and staged[4].shape == (2, 128, 128, 1)
  total, scalars = tr.compute_losses(staged)
  assert set(scalars) == SIX | {'depth_sup_loss'}
  got = float(scalars['depth_sup_loss'].detach())
  assert np.isfinite(got) and got > 0
  assert _hip.CALLS['depth_sup_fwd'] - before['depth_sup_fwd'] == len(seen)
  # paired: one call on the 2 B views, twice the mean; else one per view, summed
  assert len(seen) in (1, 2)
  factor = 2.0 if len(seen) == 1 else 1.0
  pair = getattr(tr.model, 'pair_ldi', None)
  want = err32 = 0.0
  for pred, gt, gt_scale, kw, shape, stride, data_ptr in seen:
    assert gt_scale is None
    assert kw == dict(mode='silog', lam=0.5, valid_above=o.bg_layer_disp,
                      depth_min=1e-3, depth_max=80.0)
    assert shape == (2 // len(seen), 128, 128, 1)
    if pair is not None and len(seen) == 1:
      # layer 0 of the network's own buffer: a view, not a copy
      assert data_ptr == pair[2].data_ptr() and stride == pair[2][0].stride()
    args = (pred[..., 0], gt[..., 0], None, 'silog', 0.5, o.bg_layer_disp, G_MIN, G_MAX,
            EPS)
    a = ref.loss(*args)
    t = torch.from_numpy
    b = float(ref.loss_ops(t(args[0]), t(args[1]), *args[2:]))
    want += factor * a
    err32 += factor * abs(b - a)
    ok, _ = ref.scored(args[1], None, o.bg_layer_disp, G_MIN, G_MAX)
    assert ok.sum() > 0
  err, bar = abs(got - want) / want, max(SLACK * err32 / want, LOSS_RTOL)
  print('depth_sup trainer: %.9g want %.9g err %.3g restatement %.3g bar %.3g' %
        (got, want, err, err32 / want, bar))
  assert err <= bar, (err, bar)
  parts = (o.self_cons_wt * scalars['self_cons_loss'] +
           o.compose_splat_wt * scalars['compose_splat_loss'] +
           o.indep_splat_wt * scalars['indep_splat_loss'] +
           (o.incr_depth_wt / o.max_disp) * scalars['incr_depth_loss'] +
           (o.disp_smoothness_wt / o.max_disp ** 2) * scalars['disp_smoothness_loss'] +
           o.depth_sup_wt * scalars['depth_sup_loss'])
  assert abs(float(total) - float(parts)) <= 1e-5 * abs(float(parts))
  # the term alone reaches the layer-0 disparity head
  head = tr.model.ldi_tex_disp.pixelwise_pred.preds[0].conv.weight
  g, = torch.autograd.grad(scalars['depth_sup_loss'], head, retain_graph=True)
  assert bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
  assert _hip.CALLS['depth_sup_bwd'] - before['depth_sup_bwd'] == len(seen)
  # two whole steps: the term is logged, finite and positive
  for _ in range(2):
    total, scalars = tr.train_step()
    assert all(np.isfinite(float(v)) for v in scalars.values())
    assert float(scalars['depth_sup_loss']) > 0
  assert bool(torch.isfinite(head.grad).all()) and float(head.grad.abs().sum()) > 0


class _Batches(object):
  """A loader that hands on one prepared batch."""

  def __init__(self, batch):
    self.batch = batch

  def forward(self, bs):
    assert bs == self.batch[0].shape[0]
    return self.batch


@pytest.mark.parametrize('source', ['px', 'velodyne'])
def test_kitti_ground_truth_is_staged_as_the_evaluation_forms_it(source, tmp_path, dev):
  """No KITTI files are at hand: a KITTI-shaped batch (tests/test_lidar_gpu.py: scans
  on the plane Z = 10) goes through feed, stage and compute_losses of a trainer
  on procedural KITTI pairs whose loader is replaced."""
  sys.path.insert(0, PKG)
  import ldi_enc_dec as script
  from lsi.geometry import lidar
  from test_lidar_gpu import PLANE_DEPTH, _kitti_batch
  argv = ['--dataset', 'kitti', '--kitti_procedural', 'true', '--batch_size', '2',
          '--n_layers', '2', '--img_height', '128', '--img_width', '128', '--bf16',
          'false', '--checkpoint_dir', str(tmp_path), '--depth_sup_mode', 'l1',
          '--depth_sup_max', '50']
  opts = script.apply_dataset_overrides(script.build_parser().parse_args(argv))
  tr = script.Trainer(opts)
  tr.setup()
  # (with files this is what --depth_sup_wt 1 --kitti_dl_... true sets up)
  opts.depth_sup_wt, tr.depth_sup_source = 1.0, source
  batch = _kitti_batch(62)
  k_s, k_t, trans = batch[2], batch[3], batch[5]
  pts, counts, mats = batch[6:9]
  inv = lidar.rasterize_points(pts.to(dev), None, counts, mats.to(dev), 128, 128,
                               z_min=1e-3, z_max=50.0, inverse=True)
  want_gt = torch.cat([inv[:, 0], inv[:, 1]], dim=0)          # 2 B x H x W x 1
  filled = want_gt > 0
  assert 0.05 < float(filled.float().mean()) < 0.6
  assert bool((want_gt[filled] == np.float32(1.0) / np.float32(PLANE_DEPTH)).all())
  if source == 'px':
    # the same maps as pixel disparities d = f_x |t_x| / depth: the last two outputs
    f_t = float(k_s[0, 0, 0]) * abs(float(trans[0, 0, 0]))
    px = (want_gt * f_t).cpu()
    batch = batch[:6] + (px[:2], px[2:])
    want_scale = torch.cat([1.0 / (k_s[:, 0, 0] * trans[:, 0, 0].abs()),
                            1.0 / (k_t[:, 0, 0] * trans[:, 0, 0].abs())]).float()
  tr.data_loader = _Batches(batch)
  fed = tr.feed()
  assert len(fed) == 7 and fed[6][0] == source
  staged, _ = tr.stage(fed)
  if source == 'px':
    assert len(staged) == 6
    assert torch.equal(staged[4], px.to(dev)) and torch.equal(staged[5].cpu(), want_scale)
  else:
    assert len(staged) == 5 and torch.equal(staged[4], want_gt)
  total, scalars = tr.compute_losses(staged)
  got = float(scalars['depth_sup_loss'].detach())
  pair = tr.model.pair_ldi
  assert pair is not None
  pred = pair[2][0, ..., 0].detach().cpu().numpy()
  gt = staged[4][..., 0].cpu().numpy()
  scale = staged[5].cpu().numpy() if source == 'px' else None
  g_min = float(np.float32(1.0) / np.float32(50.0))
  # one call on the 2 B planes, times 2
  want = 2.0 * ref.loss(pred, gt, scale, 'l1', 0.5, 0.0, g_min, G_MAX, EPS)
  ok, g = ref.scored(gt, scale, 0.0, g_min, G_MAX)
  assert ok.sum() == int(filled.sum()) and np.abs(g[ok] - 0.1).max() <= 1e-6
  print('depth_sup trainer (%s): %.9g want %.9g' % (source, got, want))
  assert want > 0 and abs(got - want) <= LOSS_RTOL * want
  # a batch without ground truth under a positive weight is an error that names
  # the three sources
  tr.data_loader = _Batches(batch[:6])
  with pytest.raises(ValueError, match='--kitti_dl_velodyne'):
    tr.feed()


def _pin_network(tr, pair):
  """The trainer's network pass replaced by a recorded output (2 B LDIs)."""
  b = pair[2].shape[1] // 2
  half = lambda t, k: None if t is None else t[:, k * b:(k + 1) * b]

  def forward(imgs_src, imgs_trg):
    tr.model.pair_ldi = list(pair)
    return [half(t, 0) for t in pair], [half(t, 1) for t in pair]

  tr.train_model = forward


def test_weight_zero_is_the_step_without_the_flag(tmp_path, dev):
  """`--depth_sup_wt 0` against no flag at all: same seeds, same batch, the
  step's loss bit for bit, and no extra loader output, staged tensor or launch.

  The network pass is pinned to one recorded output for both runs, because two
  fresh runs of this project WITHOUT the flag do not agree bit for bit to begin
  with: measured on the MI355X, three identical fp32 runs of this configuration
  gave total_loss 4.131279468536377 / 4.1312918663024902 / 4.131291389465332 (and
  disp_smoothness_loss 2.4980776 / 2.4980774 / 2.4980774: the predicted
  disparities themselves differ), bf16 runs likewise.  Everything the flag could
  touch -- feed, stage, every loss kernel, the renderer, the total -- runs for
  real in both."""
  from lsi.loss import _hip
  runs = []
  pair = None
  for i, extra in enumerate(((), ('--depth_sup_wt', '0'), ())):
    tr = _trainer(tmp_path / str(i), *extra)
    assert tr.opts.depth_sup_wt == 0.0 and tr.depth_sup_source is None
    before = dict(_hip.CALLS)
    batch = tr.feed()
    assert len(batch) == 6                  # no extra loader output
    staged, _ = tr.stage(batch)
    assert len(staged) == 4
    if pair is None:
      with torch.no_grad():
        tr.train_model(staged[0], staged[1])
      pair = [None if t is None else t.detach().clone() for t in tr.model.pair_ldi]
    _pin_network(tr, pair)
    total, scalars = tr.compute_losses(staged)
    assert set(scalars) == SIX and _hip.CALLS == before
    runs.append((total.detach().clone(), [t.clone() for t in staged],
                 {k: float(torch.as_tensor(v).detach()) for k, v in scalars.items()}))
    print('depth_sup weight 0, run %d (%s): %s' % (i, ' '.join(extra) or 'no flag',
                                                   runs[-1][2]))
  # the same batch went in ...
  for a, b in zip(runs[0][1], runs[1][1]):
    assert torch.equal(a, b)
  # ... and the same loss came out
  assert torch.equal(runs[0][0], runs[1][0]), (runs[0][2], runs[1][2])
  assert float(runs[0][0]) > 0
