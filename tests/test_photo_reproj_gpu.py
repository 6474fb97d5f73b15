"""The fused backward-warp photometric loss (csrc/lsi_photo_reproj.hip) against
the restatement of its definition (tests/photo_reproj_ref.py (a)).

Bars, the project's own (tests/test_geo_cons_gpu.py): every comparison first
measures the error of the fp32 op restatement (b) against (a) on the same
inputs, on the CPU, and allows the kernels max(4 x that error, the usual bar) --
2e-6 relative on a loss, 1e-5 of the largest entry on each gradient.  The scored
count per plane and where the map is -1 are compared exactly: both sides form
u, v, dd, the samples and the partner's sample in fp32, operation for operation.

Inputs, poses and the conditions they meet: tests/photo_reproj_cases.py, held
from the restatement alone in tests/test_photo_reproj_cpu.py.  Shape p holds a's
values in one packed P x H x W x 4 buffer (tex = [..., :3], disp = [..., 3]) with
the images at x-stride 2 in padded rows; shape t is the two-tensor form.

The trainer tests run at 128 x 256, the smallest size the U-Net takes.
Figures measured on an MI355X are in DESIGN.md 4.23."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import photo_reproj_cases as cases
import photo_reproj_ref as ref
from conftest import PKG
from photo_reproj_cases import EPS, OCCL, UPSTREAM

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_RTOL, SLACK = 2e-6, 1e-5, 4.0
EINVAL, ENULL, EWORKSPACE = -1, -2, -3


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def same(a, b):
  """torch.equal with NaN equal to NaN (the inputs hold planted NaNs)."""
  return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def on_device(name, pose, dev):
  """(T, D, I, M, E, shift) on the device in the layout the shape asks for."""
  T, D, I, M, E, shift, _ = cases.make_inputs(name, pose)
  T, D, I, M, E = (torch.from_numpy(a).to(dev) for a in (T, D, I, M, E))
  p, h, w, c = T.shape
  if name == 'p':
    rgbd = torch.full((p, h, w, 4), 7.0, device=dev)
    rgbd[..., :3], rgbd[..., 3] = T, D
    tview, dview = rgbd[..., :3], rgbd[..., 3]
    wide = torch.full((I.shape[0], h, 2 * w + 2, c), 7.0, device=dev)
    wide[:, :, :2 * w:2] = I
    iview = wide[:, :, :2 * w:2]
    assert tview.stride() == (4 * h * w, 4 * w, 4, 1) and dview.stride() == (4 * h * w, 4 * w, 4)
    assert iview.stride() == (h * (2 * w + 2) * c, (2 * w + 2) * c, 2 * c, 1)
    assert same(tview, T) and same(dview, D) and same(iview, I)
    T, D, I = tview, dview, iview
  return T, D, I, M, E, shift


def kernel(T, D, I, M, E, shift, mode, occl, want=(True, True)):
  """(loss, gradient of loss * UPSTREAM w.r.t. T, w.r.t. D, plane sums, map) from
  the HIP kernels; T, D, I and E may be device views.  T is P x H x W x C, D is
  P x H x W: split into layers of the Q views here (a view)."""
  from lsi.loss import _hip
  q = I.shape[0]
  x = T.view((-1, q) + tuple(T.shape[1:])).detach().requires_grad_(want[0])
  y = D.view((-1, q) + tuple(D.shape[1:])).detach().requires_grad_(want[1])
  l, emap, sums = _hip.photometric_reprojection_loss(
      x, y, I, M, E, shift, mode, occl, EPS, return_map=True, return_plane_sums=True)
  g = torch.autograd.grad(l * UPSTREAM, [t for t, k in zip((x, y), want) if k])
  g = list(g)
  gT = g.pop(0).reshape(T.shape) if want[0] else None
  gD = g.pop(0).reshape(D.shape) if want[1] else None
  return l.detach(), gT, gD, sums, emap


def check(tag, l, gT, gD, r):
  """Prints the measured errors, then holds them against the bars."""
  l = float(l)
  loss_err = abs(l - r['loss']) / abs(r['loss']) if r['loss'] else abs(l)
  loss_bar = max(SLACK * r['loss_err32'], LOSS_RTOL)
  print('photo_reproj %s: loss %.9g err kernel %.3g restatement %.3g bar %.3g' %
        (tag, l, loss_err, r['loss_err32'], loss_bar))
  assert loss_err <= loss_bar, (tag, loss_err, loss_bar)
  for which, got, want, scale, err32 in (('tex', gT, r['gT'], r['tmax'], r['gT_err32']),
                                         ('disp', gD, r['gD'], r['dmax'], r['gD_err32'])):
    if got is None:
      continue
    err = np.abs(got.cpu().double().numpy() - want).max()
    err = float(err / scale) if scale else float(err)
    bar = max(SLACK * err32, GRAD_RTOL)
    print('photo_reproj %s: %s gradient err kernel %.3g restatement %.3g bar %.3g' %
          (tag, which, err, err32, bar))
    assert err <= bar, (tag, which, err, bar)


@pytest.mark.parametrize('name,pose,mode,occl', cases.RUNS)
def test_forward_and_gradient(name, pose, mode, occl, dev):
  r = cases.case_reference(name, pose, mode, occl)
  T, D, I, M, E, shift = on_device(name, pose, dev)
  l, gT, gD, sums, emap = kernel(T, D, I, M, E, shift, mode, occl)
  assert gT.shape == T.shape and gD.shape == D.shape
  assert bool(torch.isfinite(gT).all()) and bool(torch.isfinite(gD).all())
  assert bool(torch.isfinite(l)) and bool(torch.isfinite(sums).all())
  sums = sums.cpu().numpy().reshape(-1, 3)
  # the counts exactly, the sums to the forward's bar, the spare untouched
  assert np.array_equal(sums[:, 1], r['sums'][:, 1])
  assert not sums[:, 2].any()
  scale_ = np.abs(r['sums'][:, 0]).max()
  if scale_:
    err = np.abs(sums[:, 0] - r['sums'][:, 0]).max() / scale_
    assert err <= max(SLACK * r['loss_err32'], LOSS_RTOL), err
  else:
    assert not sums[:, 0].any()
  emap = emap.cpu().numpy()
  # -1 exactly where unscored; the scored values to a few fp32 ulps
  assert np.array_equal(emap == -1.0, ~r['scored'])
  assert np.abs(emap - r['map']).max() <= 4e-7 * max(1.0, np.abs(r['map']).max())
  if not r['scored'].any():
    assert float(l) == 0.0
    assert not gT.cpu().numpy().any() and not gD.cpu().numpy().any()
  # a gradient entry is exactly 0 where the restatement's is
  assert not gT.cpu().numpy()[r['gT'] == 0].any()
  assert not gD.cpu().numpy()[r['gD'] == 0].any()
  check('%s %s %s occl %g' % (name, pose, mode, occl), l, gT, gD, r)


@pytest.mark.parametrize('mode', ref.MODES)
def test_strided_inputs_give_the_same_bits(mode, dev):
  """The per-lane route (any stride) against the whole-line route (tex's last two
  strides (C, 1)): loss, sums, map and both gradients bit for bit."""
  T, D, I, M, E, shift = on_device('p', 'general', dev)
  assert T.stride()[-2:] == (4, 1)
  want = kernel(T.contiguous(), D.contiguous(), I.contiguous(), M, E, shift, mode, OCCL)
  got = kernel(T, D, I, M, E, shift, mode, OCCL)
  for a, b in zip(got, want):
    assert torch.equal(a, b)
  # the network's own layout: L x 2 B x H x W x 4 views of a 2 B x H x W x L x 4
  # buffer, the partner layer 0 of it
  from lsi.loss import _hip
  T, D, I, M, E, shift = on_device('a', 'rect', dev)
  p, h, w, c = T.shape
  q = I.shape[0]
  buf = torch.full((q, h, w, p // q, 4), 7.0, device=dev)
  pred = buf.permute(3, 0, 1, 2, 4)
  pred[..., :3], pred[..., 3] = T.view(p // q, q, h, w, c), D.view(p // q, q, h, w)
  tex, disp = pred[..., :3], pred[..., 3]
  assert tex.stride() == (4, h * w * 8, w * 8, 8, 1) and same(disp[0], E)
  want = kernel(T, D, I, M, E, shift, mode, OCCL)
  x, y = tex.detach().requires_grad_(True), disp.detach().requires_grad_(True)
  l, emap, sums = _hip.photometric_reprojection_loss(
      x, y, I, M, disp[0].detach(), shift, mode, OCCL, EPS, return_map=True,
      return_plane_sums=True)
  gx, gy = torch.autograd.grad(l * UPSTREAM, [x, y])
  assert gx.is_contiguous() and gy.is_contiguous()
  for a, b in zip((l.detach(), gx.reshape(T.shape), gy.reshape(D.shape), sums, emap), want):
    assert torch.equal(a, b)


def test_either_gradient_alone(dev):
  T, D, I, M, E, shift = on_device('b', 'general', dev)
  both = kernel(T, D, I, M, E, shift, 'charb', OCCL)
  only_t = kernel(T, D, I, M, E, shift, 'charb', OCCL, want=(True, False))
  only_d = kernel(T, D, I, M, E, shift, 'charb', OCCL, want=(False, True))
  assert torch.equal(only_t[1], both[1]) and only_t[2] is None
  assert torch.equal(only_d[2], both[2]) and only_d[1] is None
  assert torch.equal(only_t[0], both[0]) and torch.equal(only_d[0], both[0])


def test_quarter_pixel_lattice_is_exact(dev):
  T, D, I, M = cases.lattice_inputs()
  l, gT, gD, sums, emap, sc = ref.loss_and_grad(T, D, I, M, None, 1, 'l1')
  assert 0.1 * sc.size < sc.sum() < sc.size
  # the lattice: the restatement's sums are the same in fp32 and in fp64
  e = np.where(sc, emap, np.float32(0.0))
  s32 = np.array([np.cumsum(e[i].ravel(), dtype=np.float32)[-1] for i in range(2)])
  assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), sums[:, 0])
  assert np.array_equal(e * 128, np.round(e * 128)) and e.max() > 0
  t = lambda a: torch.from_numpy(a).to(dev)
  lk, _, _, ksums, kmap = kernel(t(T), t(D), t(I), t(M), None, 1, 'l1', 0.0)
  assert np.array_equal(ksums.cpu().numpy().reshape(-1, 3), sums)
  assert np.array_equal(kmap.cpu().numpy(), emap)
  assert float(lk) == float(np.float32(l))


@pytest.mark.parametrize('mode', ref.MODES)
def test_both_directions_are_reproducible(mode, dev):
  """No atomics either way: loss, sums, map and both gradients bit for bit."""
  for name in ('b', 'p'):
    args = on_device(name, 'general', dev)
    runs = [kernel(*args, mode, OCCL) for _ in range(2)]
    for a, b in zip(*runs):
      assert torch.equal(a, b)
    assert float(runs[0][1].abs().sum()) > 0 and float(runs[0][2].abs().sum()) > 0


def test_public_wrapper(dev):
  from lsi.loss import loss
  T, D, I, M, E, shift = on_device('a', 'general', dev)
  p, h, w, c = T.shape
  q = I.shape[0]
  for mode in ref.MODES:
    want, gT_want, gD_want, _, map_want = kernel(T, D, I, M, E, shift, mode, OCCL)
    # leading dimensions L x Q, the disparities with their channel
    x = T.view(p // q, q, h, w, c).clone().requires_grad_(True)
    y = D.view(p // q, q, h, w, 1).clone().requires_grad_(True)
    got, emap = loss.photometric_reprojection_loss(
        x, y, I, M, partner_disps=E[..., None], shift=shift, mode=mode,
        occl_thresh=OCCL, eps=EPS, return_map=True)
    assert torch.equal(got.detach(), want) and torch.equal(emap, map_want)
    assert not emap.requires_grad and emap.shape == (p, h, w)
    (got * UPSTREAM).backward()
    assert x.grad.shape == x.shape and y.grad.shape == y.shape
    assert torch.equal(x.grad.reshape(T.shape), gT_want)
    assert torch.equal(y.grad.reshape(D.shape), gD_want)
  # the defaults: l1, shift 0, no partner, no occlusion rule, eps 1e-3, no map
  got = loss.photometric_reprojection_loss(T, D, I, M)
  assert torch.equal(got, kernel(T, D, I, M, None, 0, 'l1', 0.0)[0])
  got = loss.photometric_reprojection_loss(T, D, I, M, mode='charb')
  assert torch.equal(got, kernel(T, D, I, M, None, 0, 'charb', 0.0)[0])
  # a constant texture: the disparities alone take a gradient
  y = D.clone().requires_grad_(True)
  loss.photometric_reprojection_loss(T, y, I, M, shift=shift).backward()
  assert float(y.grad.abs().sum()) > 0


def test_refusals_come_in_order_and_launch_nothing(dev):
  from lsi import _C
  from lsi.loss import _hip
  lib = _C.lib()
  T, D, I, M, E, shift = on_device('t', 'rect', dev)
  T5, D4 = T.view(2, 2, 13, 37, 3), D.view(2, 2, 13, 37)
  make = lambda: _hip.photo_reproj_desc(T5, D4, I, M, E, 0, 'l1', 0.2, EPS, 't')
  d = make()
  n = int(lib.lsi_photo_reproj_workspace_bytes(ctypes.byref(d)))
  assert n == (3 * 4 * 1 + 4) * 8
  out = torch.full((), -7.0, device=dev)
  sums = torch.full((12,), -7.0, dtype=torch.float64, device=dev)
  ws = torch.full((n // 8,), -7.0, dtype=torch.float64, device=dev)
  emap = torch.full(D.shape, -7.0, device=dev)
  g_loss = torch.full((), UPSTREAM, device=dev)
  g_t = torch.full(T.shape, -7.0, device=dev)
  g_d = torch.full(D.shape, -7.0, device=dev)
  ptr = _C.ptr

  def fwd(desc, t=T, dd=D, i=I, m=M, e=E, o=out, s=sums, w=ws, nbytes=n):
    return lib.lsi_photo_reproj_loss_fwd(ctypes.byref(desc), ptr(t), ptr(dd), ptr(i),
                                         ptr(m), ptr(e), ptr(o), ptr(s), ptr(emap),
                                         ptr(w), nbytes, None)

  def bwd(desc, t=T, dd=D, i=I, m=M, e=E, s=sums, gl=g_loss, gt=g_t, gd=g_d):
    return lib.lsi_photo_reproj_loss_bwd(ctypes.byref(desc), ptr(t), ptr(dd), ptr(i),
                                         ptr(m), ptr(e), ptr(s), ptr(gl), ptr(gt),
                                         ptr(gd), None)

  def bad(**kw):
    b = make()
    for k, v in kw.items():
      setattr(b, k, v)
    return b

  for kw in (dict(mode=2), dict(P=0), dict(H=-1), dict(C=5), dict(Q=3), dict(P=65536),
             dict(H=4096, W=4096), dict(shift=2), dict(shift=-1), dict(occl_thresh=1.0),
             dict(occl_thresh=float('nan')), dict(eps=0.0)):
    b = bad(**kw)
    assert lib.lsi_photo_reproj_workspace_bytes(ctypes.byref(b)) == 0, kw
    # a bad descriptor first: before the NULL pointer and the short workspace
    assert fwd(b, t=None, nbytes=0) == EINVAL and bwd(b, t=None) == EINVAL, kw
  # then a NULL pointer, before the short workspace
  for null in ('t', 'dd', 'i', 'm', 'e', 'o', 's', 'w'):
    assert fwd(d, **{null: None}, nbytes=0) == ENULL, null
  for null in ('t', 'dd', 'i', 'm', 'e', 's', 'gl'):
    assert bwd(d, **{null: None}) == ENULL, null
  assert bwd(d, gt=None, gd=None) == ENULL
  # then the workspace
  assert fwd(d, nbytes=n - 1) == EWORKSPACE
  torch.cuda.synchronize()
  # nothing was launched: no output was touched
  for t in (out, sums, ws, emap, g_t, g_d):
    assert bool((t == -7.0).all())
  # ... and the same arguments, complete, run; either gradient may be left out
  assert fwd(d) == 0 and bwd(d, gt=None) == 0
  torch.cuda.synchronize()
  assert bool((g_t == -7.0).all()) and bool(torch.isfinite(g_d).all())
  assert bwd(d, gd=None) == 0
  torch.cuda.synchronize()
  assert bool(torch.isfinite(g_t).all())
  assert float(out) > 0 and float(g_t.abs().sum()) > 0 and float(g_d.abs().sum()) > 0
  # without the rule the partner may be NULL
  assert fwd(bad(occl_thresh=0.0), e=None) == 0 and bwd(bad(occl_thresh=0.0), e=None) == 0
  torch.cuda.synchronize()


def test_capture_in_a_graph_and_replay_on_new_values(dev):
  """Forward and backward at shape a, recorded in one graph on a side stream, then
  replayed on other values: loss and gradients bit for bit the eager call's."""
  from lsi.loss import _hip
  first = on_device('a', 'general', dev)
  other = on_device('a', 'rect', dev)          # other values and other cameras
  shift = first[5]
  split = lambda t, q=first[2].shape[0]: t.view((-1, q) + tuple(t.shape[1:]))
  for mode in ref.MODES:
    t_s = split(first[0]).clone().requires_grad_(True)
    d_s = split(first[1]).clone().requires_grad_(True)
    i_s, m_s, e_s = first[2].clone(), first[3].clone(), first[4].clone()

    def step():
      l = _hip.photometric_reprojection_loss(t_s, d_s, i_s, m_s, e_s, shift, mode, OCCL,
                                             EPS)
      gt, gd = torch.autograd.grad(l * UPSTREAM, [t_s, d_s])
      return l, gt, gd

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      step()                                    # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
      l_s, gt_s, gd_s = step()
    with torch.no_grad():
      t_s.copy_(split(other[0]))
      d_s.copy_(split(other[1]))
      for dst, src in ((i_s, other[2]), (m_s, other[3]), (e_s, other[4])):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    l, gT, gD, _, _ = kernel(*other, mode, OCCL)
    assert torch.equal(l_s, l)
    assert torch.equal(gt_s.reshape(gT.shape), gT) and torch.equal(gd_s.reshape(gD.shape), gD)
    assert not torch.equal(gD, kernel(*first, mode, OCCL)[2])


# ---------------------------------------------------------------------------
# the training script
# ---------------------------------------------------------------------------
def _trainer(tmp_path, *extra):
  sys.path.insert(0, PKG)
  import ldi_enc_dec as script
  argv = ['--dataset', 'kitti', '--kitti_procedural', 'true', '--batch_size', '2',
          '--n_layers', '2', '--img_height', '128', '--img_width', '256', '--bf16',
          'false', '--checkpoint_dir', str(tmp_path), '--log_freq', '1000000',
          '--save_latest_freq', '1000000', '--checkpoint_freq', '1000000'] + list(extra)
  opts = script.apply_dataset_overrides(script.build_parser().parse_args(argv))
  torch.manual_seed(0)
  np.random.seed(0)
  tr = script.Trainer(opts)
  tr.setup()
  return tr


SIX = {'self_cons_loss', 'compose_splat_loss', 'indep_splat_loss', 'incr_depth_loss',
       'disp_smoothness_loss', 'total_loss'}


def _flagless_total(o, s):
  return (o.self_cons_wt * s['self_cons_loss'] +
          o.compose_splat_wt * s['compose_splat_loss'] +
          o.indep_splat_wt * s['indep_splat_loss'] +
          (o.incr_depth_wt / o.max_disp) * s['incr_depth_loss'] +
          (o.disp_smoothness_wt / o.max_disp ** 2) * s['disp_smoothness_loss'])


@pytest.mark.parametrize('what,paired,mode', [('texture', 'true', 'l1'),
                                              ('texture', 'false', 'charb'),
                                              ('image', 'true', 'charb')])
def test_ten_training_steps_with_the_term(what, paired, mode, tmp_path, dev):
  from lsi.loss import _hip, loss
  tr = _trainer(tmp_path, '--photo_reproj_wt', '0.5', '--photo_reproj_mode', mode,
                '--photo_reproj_what', what, '--paired_splat', paired)
  o = tr.opts
  assert o.photo_reproj_occl == 0.2
  before = dict(_hip.CALLS)
  staged, _ = tr.stage(tr.feed())
  total, scalars = tr.compute_losses(staged)
  assert set(scalars) == SIX | {'photo_reproj_loss'}
  n_calls = 1 if paired == 'true' else 2
  assert _hip.CALLS['photo_reproj_fwd'] - before['photo_reproj_fwd'] == n_calls
  # the term again, through the public function on the network's own buffer
  pair = tr.model.pair_ldi
  b = o.batch_size
  assert pair is not None and pair[0].shape == (2, 2 * b, 128, 256, 3)
  imgs_src, imgs_trg, mat_trg, mat_src = staged[:4]
  imgs2 = torch.cat([imgs_src, imgs_trg])
  kw = dict(mode=mode, occl_thresh=0.2)
  with torch.no_grad():
    if what == 'image':
      again, emap = loss.photometric_reprojection_loss(
          imgs2, pair[2][0], imgs2, torch.cat([mat_trg, mat_src]),
          partner_disps=pair[2][0].detach(), shift=b, return_map=True, **kw)
      again = 2.0 * again
    elif paired == 'true':
      again, emap = loss.photometric_reprojection_loss(
          pair[0], pair[2], imgs2, torch.cat([mat_trg, mat_src]),
          partner_disps=pair[2][0].detach(), shift=b, return_map=True, **kw)
      again = 2.0 * again
    else:
      l_s, emap = loss.photometric_reprojection_loss(
          pair[0][:, :b], pair[2][:, :b], imgs_trg, mat_trg,
          partner_disps=pair[2][0, b:].detach(), return_map=True, **kw)
      again = l_s + loss.photometric_reprojection_loss(
          pair[0][:, b:], pair[2][:, b:], imgs_src, mat_src,
          partner_disps=pair[2][0, :b].detach(), **kw)
  assert torch.equal(again, scalars['photo_reproj_loss'].detach())
  assert float(again) > 0 and float((emap >= 0).float().mean()) > 0.25
  parts = _flagless_total(o, scalars) + o.photo_reproj_wt * scalars['photo_reproj_loss']
  assert abs(float(total) - float(parts)) <= 1e-5 * abs(float(parts))
  # the term alone reaches the disparities of both views, finitely -- and, by
  # texture, every layer's texture; by image, layer 0's disparities only
  g_tex, g_disp = torch.autograd.grad(scalars['photo_reproj_loss'], [pair[0], pair[2]],
                                      retain_graph=True, allow_unused=True)
  assert bool(torch.isfinite(g_disp).all())
  assert float(g_disp[0, :b].abs().sum()) > 0 and float(g_disp[0, b:].abs().sum()) > 0
  if what == 'image':
    assert g_tex is None and not bool(g_disp[1].any())
  else:
    assert bool(torch.isfinite(g_tex).all()) and float(g_disp[1].abs().sum()) > 0
    assert float(g_tex[0].abs().sum()) > 0 and float(g_tex[1].abs().sum()) > 0
  assert _hip.CALLS['photo_reproj_bwd'] - before['photo_reproj_bwd'] == n_calls
  # ten whole steps on one batch: finite throughout, and the loss goes down
  batch = tr.feed()
  tr.feed = lambda batch=batch: batch
  log = []
  for _ in range(10):
    total, scalars = tr.train_step()
    log.append({k: float(v) for k, v in scalars.items()})
    assert all(np.isfinite(v) for v in log[-1].values()), log[-1]
  for p in tr.model.parameters():
    assert p.grad is None or bool(torch.isfinite(p.grad).all())
  print('photo_reproj trainer %s paired=%s %s: total %s | term %s' %
        (what, paired, mode, ' '.join('%.5g' % s['total_loss'] for s in log),
         ' '.join('%.5g' % s['photo_reproj_loss'] for s in log)))
  assert log[-1]['total_loss'] < log[0]['total_loss']


def test_the_term_without_the_splat_terms(tmp_path, dev):
  """With both splat weights at 0 the paired splat builds no matrices: the term
  builds its own."""
  from lsi.loss import loss
  tr = _trainer(tmp_path, '--photo_reproj_wt', '0.5', '--indep_splat_wt', '0',
                '--compose_splat_wt', '0')
  staged, _ = tr.stage(tr.feed())
  total, scalars = tr.compute_losses(staged)
  pair = tr.model.pair_ldi
  b = tr.opts.batch_size
  with torch.no_grad():
    again = 2.0 * loss.photometric_reprojection_loss(
        pair[0], pair[2], torch.cat([staged[0], staged[1]]),
        torch.cat([staged[2], staged[3]]), partner_disps=pair[2][0].detach(), shift=b,
        occl_thresh=0.2)
  assert torch.equal(again, scalars['photo_reproj_loss'].detach()) and float(again) > 0
  assert float(scalars['compose_splat_loss']) == 0.0 == float(scalars['indep_splat_loss'])
  parts = _flagless_total(tr.opts, scalars) + 0.5 * scalars['photo_reproj_loss']
  assert abs(float(total) - float(parts)) <= 1e-5 * abs(float(parts))


def _pin_network(tr, pair):
  """The trainer's network pass replaced by a recorded output (2 B LDIs)."""
  b = pair[2].shape[1] // 2
  half = lambda t, k: None if t is None else t[:, k * b:(k + 1) * b]

  def forward(imgs_src, imgs_trg):
    tr.model.pair_ldi = list(pair)
    return [half(t, 0) for t in pair], [half(t, 1) for t in pair]

  tr.train_model = forward


def test_weight_zero_is_the_step_without_the_flag(tmp_path, dev):
  """`--photo_reproj_wt 0` against no flag at all: the same keys, the step's loss
  bit for bit, no launch of the term.  The network pass is pinned to one recorded
  output for the runs, as in tests/test_geo_cons_gpu.py: two fresh runs of the
  network do not agree bit for bit to begin with."""
  from lsi.loss import _hip
  runs = []
  pair = None
  for i, extra in enumerate(((), ('--photo_reproj_wt', '0', '--photo_reproj_mode', 'charb',
                                  '--photo_reproj_occl', '0.3', '--photo_reproj_what',
                                  'image'), ())):
    tr = _trainer(tmp_path / str(i), *extra)
    assert tr.opts.photo_reproj_wt == 0.0
    before = dict(_hip.CALLS)
    staged, _ = tr.stage(tr.feed())
    assert len(staged) == 4
    if pair is None:
      with torch.no_grad():
        tr.train_model(staged[0], staged[1])
      pair = [None if t is None else t.detach().clone() for t in tr.model.pair_ldi]
    _pin_network(tr, pair)
    total, scalars = tr.compute_losses(staged)
    assert set(scalars) == SIX
    assert _hip.CALLS['photo_reproj_fwd'] == before['photo_reproj_fwd']
    runs.append((total.detach().clone(), [t.clone() for t in staged],
                 {k: float(torch.as_tensor(v).detach()) for k, v in scalars.items()}))
  for a, b in zip(runs[0][1], runs[1][1]):
    assert torch.equal(a, b)
  # flagless, weight 0, flagless again: the pinned step is itself reproducible,
  # and the weight-0 step is that step
  for k in (1, 2):
    assert torch.equal(runs[0][0], runs[k][0]), (runs[0][2], runs[k][2])
    assert runs[0][2] == runs[k][2]
  assert float(runs[0][0]) > 0
