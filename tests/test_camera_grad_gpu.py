"""The camera gradient of forward_splat on the MI355X: dL/dM from the backward
kernels (lsi_splat_bwd_m / lsi_splat_bwd_both_m), carried to k_s, k_t, rot, t
and focal_disps, against fp64 autograd of the reference's op graph
(oracle/lsi_torch_ref.py, M built from the cameras in fp64 torch here).

Bar, as tests/test_full_size_gpu.py: the kernels' error against fp64 is at
most twice that of the same op graph run in fp32 (what the reference's own
autodiff computes), plus a floor of 1e-6 of the largest entry."""
import math

import numpy as np
import pytest
import torch

import lsi_torch_ref as TR

pytestmark = pytest.mark.gpu

S, BG, MD, ZB = 0.5, 1e-3, 0.4, 50.0


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def _rodrigues(a):
  """B x 3 axis-angle -> B x 3 x 3 rotations."""
  z = torch.zeros_like(a[:, 0])
  k = torch.stack([torch.stack([z, -a[:, 2], a[:, 1]], -1),
                   torch.stack([a[:, 2], z, -a[:, 0]], -1),
                   torch.stack([-a[:, 1], a[:, 0], z], -1)], 1)
  return torch.linalg.matrix_exp(k)


def _cameras(b, h, w, general, seed):
  """KITTI-like intrinsics; rectified stereo (identity rotation, x baseline)
  or a general pose (small rotation, 3-D translation)."""
  g = torch.Generator().manual_seed(seed)
  f = 0.58 * w
  k = torch.tensor([[f, 0.0, w / 2], [0.0, f, h / 2], [0.0, 0.0, 1.0]]).repeat(b, 1, 1)
  if general:
    rot = _rodrigues(0.02 * (torch.rand((b, 3), generator=g) - 0.5))
    t = torch.tensor([[-0.5], [0.02], [0.03]]) + 0.02 * torch.rand((b, 3, 1), generator=g)
  else:
    rot = torch.eye(3).repeat(b, 1, 1)
    t = torch.tensor([[-0.532], [0.0], [0.0]]).repeat(b, 1, 1)
  return [x.to(torch.float32) for x in (k, k.clone(), rot, t)]


def _ldi(nl, b, h, w, seed, mask=True):
  g = torch.Generator().manual_seed(seed)
  tex = torch.rand((nl, b, h, w, 3), generator=g)
  # smooth disparity fields, layers front to back
  base = torch.rand((nl * b, 1, h // 4, w // 4), generator=g)
  field = torch.nn.functional.interpolate(base, size=(h, w), mode='bilinear',
                                          align_corners=False)
  scale = torch.tensor([(nl - l) / nl for l in range(nl)]).view(nl, 1, 1, 1, 1)
  disp = (MD * (0.2 + 0.75 * field.reshape(nl, b, h, w, 1)) * scale).contiguous()
  msk = (0.3 + 0.7 * torch.rand((nl, b, h, w, 1), generator=g)) if mask else None
  return tex, msk, disp


def _mat64(k_s, k_t, rot, t, focal=None):
  """pad(K_t) [R t; 0 1] pad(K_s^-1) (reference projection.py:71-86) in the
  dtype of the inputs; focal_disps folded into row 3 (ldi.py:130-143:
  D + f = (q3 + f q2) / q2)."""
  b = k_s.shape[0]
  dt = k_s.dtype
  eye = torch.eye(4, dtype=dt).repeat(b, 1, 1)
  kt = torch.cat([torch.cat([k_t, torch.zeros((b, 3, 1), dtype=dt)], 2), eye[:, 3:]], 1)
  ks = torch.cat([torch.cat([torch.linalg.inv(k_s), torch.zeros((b, 3, 1), dtype=dt)], 2),
                  eye[:, 3:]], 1)
  e = torch.cat([torch.cat([rot, t], 2), eye[:, 3:]], 1)
  m = kt @ e @ ks
  if focal is not None:
    f = focal.reshape(b, 1)
    m = torch.cat([m[:, :3], (m[:, 3] + f * m[:, 2])[:, None]], 1)
  return m


def _cotangents(shape_l, shape_c, seed):
  g = torch.Generator().manual_seed(seed)
  return torch.rand(shape_l, generator=g), torch.rand(shape_c, generator=g)


def _loss(outs, ci, cc):
  """A loss that reaches every output: images by random weights, the
  composed weights through a log."""
  if len(outs) == 4:
    img, _, img_c, wts_c = outs
    return ((img * ci.to(img)).sum() + (img_c * cc.to(img)).sum() +
            1e-3 * torch.log(wts_c).sum())
  img, wts = outs[:2]
  return (img * ci.to(img)).sum() + 1e-3 * torch.log(wts).sum()


def _ref_grads(tex, mask, disp, cams, focal, compose, dtype, ci, cc):
  """Autograd of the reference's op graph in `dtype` w.r.t. the cameras."""
  leaves = [c.to(dtype).clone().requires_grad_(True) for c in cams]
  f = focal.to(dtype).clone().requires_grad_(True) if focal is not None else None
  m = _mat64(*leaves, focal=f)
  d = disp.to(dtype)
  if f is not None:
    d = d - f.view(1, -1, 1, 1, 1)
  msk = torch.ones_like(d) if mask is None else mask.to(dtype)
  t = tex.to(dtype)
  if compose == 'both':
    img, wts, _ = TR.forward_splat(t, msk, d, m, S, BG, MD, ZB, False)
    img_c, wts_c, _ = TR.forward_splat(t, msk, d, m, S, BG, MD, ZB, True)
    outs = (img, wts, img_c, wts_c)
  else:
    outs = TR.forward_splat(t, msk, d, m, S, BG, MD, ZB, compose)
  _loss(outs, ci, cc).backward()
  return [x.grad.double() for x in leaves] + ([f.grad.double()] if f is not None else [])


def _check(name, got, g64, g32):
  scale = float(g64.abs().max()) + 1e-30
  err = float((got.double() - g64).abs().max())
  err32 = float((g32 - g64).abs().max())
  print('%s: |kernel - fp64| %.2e, |fp32 graph - fp64| %.2e (of %.2e)'
        % (name, err, err32, scale))
  assert bool(torch.isfinite(got).all()), name
  assert err <= 2.0 * err32 + 1e-6 * scale, (name, err, err32, scale)


def _kernel_camera_grads(dev, tex, mask, disp, cams, focal, compose, ci, cc):
  from lsi.geometry import ldi
  leaves = [c.clone().requires_grad_(True) for c in cams]
  f = focal.clone().requires_grad_(True) if focal is not None else None
  src = [tex.to(dev), None if mask is None else mask.to(dev), disp.to(dev)]
  outs = ldi.forward_splat(src, None, *leaves, focal_disps=f, compose_layers=compose,
                           trg_downsampling=S, bg_layer_disp=BG, max_disp=MD,
                           zbuf_scale=ZB)
  _loss(outs, ci, cc).backward()
  return [x.grad for x in leaves] + ([f.grad] if f is not None else [])


@pytest.mark.parametrize('compose', [True, False])
@pytest.mark.parametrize('stream', ['1', '0'])
def test_rectified_camera_grads(dev, monkeypatch, stream, compose):
  """Rectified pairs (the STREAM forward; the streamed backward with
  LSI_BWD_STREAM=1, the gather kernel's unit-normaliser branch with 0): every
  camera gets its gradient, rows 2 and 3 and M[1][0], M[1][3] included."""
  from lsi import _C
  from lsi.geometry import ldi, projection
  monkeypatch.setenv('LSI_BWD_STREAM', stream)
  nl, b, h, w = 2, 2, 32, 256
  tex, mask, disp = _ldi(nl, b, h, w, 11)
  cams = _cameras(b, h, w, False, 5)
  m = projection.forward_projection_matrix(*cams)
  assert ldi.plan_key((nl, b, h, w), S, MD, m)[0] == _C.LSI_PATH_STREAM
  nlo = 1 if compose else nl
  ci, cc = _cotangents((nlo, b, int(h * S), int(w * S), 3), (1,), 21)
  got = _kernel_camera_grads(dev, tex, mask, disp, cams, None, compose, ci, cc)
  g64 = _ref_grads(tex, mask, disp, cams, None, compose, torch.float64, ci, cc)
  g32 = _ref_grads(tex, mask, disp, cams, None, compose, torch.float32, ci, cc)
  for name, a, r64, r32 in zip(('k_s', 'k_t', 'rot', 't'), got, g64, g32):
    _check(name, a.cpu(), r64, r32)


@pytest.mark.parametrize('compose', [True, False])
def test_general_pose_camera_and_focal_grads(dev, compose):
  """General poses with a mask and focal_disps (the TILE forward, the gather
  backward's general branch)."""
  nl, b, h, w = 3, 2, 32, 64
  tex, mask, disp = _ldi(nl, b, h, w, 12)
  cams = _cameras(b, h, w, True, 6)
  focal = torch.tensor([0.05, -0.03]).view(b, 1, 1, 1)
  nlo = 1 if compose else nl
  ci, cc = _cotangents((nlo, b, int(h * S), int(w * S), 3), (1,), 22)
  got = _kernel_camera_grads(dev, tex, mask, disp, cams, focal, compose, ci, cc)
  g64 = _ref_grads(tex, mask, disp, cams, focal, compose, torch.float64, ci, cc)
  g32 = _ref_grads(tex, mask, disp, cams, focal, compose, torch.float32, ci, cc)
  for name, a, r64, r32 in zip(('k_s', 'k_t', 'rot', 't', 'focal_disps'), got, g64, g32):
    _check(name, a.cpu(), r64, r32)


def _matrix_grad(dev, tex, mask, disp, mat, call, path, ci, cc, stream=None):
  from lsi.geometry import ldi
  m = mat.clone().requires_grad_(True)
  src = [tex.to(dev), None if mask is None else mask.to(dev), disp.to(dev)]
  kw = dict(trg_downsampling=S, bg_layer_disp=BG, max_disp=MD, zbuf_scale=ZB, path=path)
  if call == 'both':
    outs = ldi.forward_splat_both(src, m, **kw)
  else:
    outs = ldi.forward_splat_matrix(src, m, compose_layers=call, **kw)
  _loss(outs, ci, cc).backward()
  return m.grad


def _ref_matrix_grad(tex, mask, disp, mat, call, dtype, ci, cc):
  m = mat.to(dtype).clone().requires_grad_(True)
  msk = torch.ones_like(disp, dtype=dtype) if mask is None else mask.to(dtype)
  t, d = tex.to(dtype), disp.to(dtype)
  if call == 'both':
    img, wts, _ = TR.forward_splat(t, msk, d, m, S, BG, MD, ZB, False)
    img_c, wts_c, _ = TR.forward_splat(t, msk, d, m, S, BG, MD, ZB, True)
    outs = (img, wts, img_c, wts_c)
  else:
    outs = TR.forward_splat(t, msk, d, m, S, BG, MD, ZB, call)
  _loss(outs, ci, cc).backward()
  return m.grad.double()


@pytest.mark.parametrize('call', [True, False, 'both'])
@pytest.mark.parametrize('path', ['tile', 'atomic', 'stream'])
def test_src2trg_matrix_grad(dev, monkeypatch, path, call):
  """forward_splat_matrix (compose True / False) and forward_splat_both with a
  src2trg_mat that requires grad, on each backward kernel."""
  nl, b, h, w = 2, 2, 32, 128
  general = path != 'stream'
  tex, mask, disp = _ldi(nl, b, h, w, 13, mask=general)
  mat = _mat64(*_cameras(b, h, w, general, 7)).to(torch.float32)
  monkeypatch.setenv('LSI_BWD_STREAM', '1')
  nlo = 1 if call is True else nl
  ci, cc = _cotangents((nlo, b, int(h * S), int(w * S), 3), (1, b, int(h * S), int(w * S), 3), 23)
  got = _matrix_grad(dev, tex, mask, disp, mat, call, path, ci, cc)
  g64 = _ref_matrix_grad(tex, mask, disp, mat, call, torch.float64, ci, cc)
  g32 = _ref_matrix_grad(tex, mask, disp, mat, call, torch.float32, ci, cc)
  _check('M %s %s' % (path, call), got.cpu(), g64, g32)


def test_full_size_cfg3_matrix_grad(dev, monkeypatch):
  """BASELINE config 3's shape (4 layers, 256 x 768, the training call
  forward_splat_both on RGBD pixels), three batch elements: the streamed and
  the gather backward against fp64."""
  import bench
  nl, h, w, _, _, cams, md, bg = bench.WORKLOADS['cfg3']
  assert (md, bg) == (MD, BG)
  tex, disp, mat = bench.make_inputs(nl, 3, h, w, cams, md, 77, torch.device('cpu'))
  ci, cc = _cotangents((nl, 3, h // 2, w // 2, 3), (1, 3, h // 2, w // 2, 3), 24)
  from lsi.geometry import ldi
  grads = {}
  for stream in ('1', '0'):
    monkeypatch.setenv('LSI_BWD_STREAM', stream)
    pred = torch.cat([tex, disp], dim=-1).to(dev)
    m = mat.clone().requires_grad_(True)
    outs = ldi.forward_splat_both([pred[..., 0:3], None, pred[..., 3:4]], m,
                                  trg_downsampling=S, bg_layer_disp=BG, max_disp=MD,
                                  zbuf_scale=ZB)
    _loss(outs, ci, cc).backward()
    grads[stream] = m.grad.cpu()
    del outs, pred
  g64 = _ref_matrix_grad(tex, None, disp, mat, 'both', torch.float64, ci, cc)
  g32 = _ref_matrix_grad(tex, None, disp, mat, 'both', torch.float32, ci, cc)
  for stream, g in grads.items():
    _check('cfg3 M stream=%s' % stream, g, g64, g32)


@pytest.mark.parametrize('path', ['tile', 'stream'])
def test_nonfinite_disparities_drop_out_of_the_matrix_grad(dev, monkeypatch, path):
  """Dropped (non-finite) pixels contribute 0: g_M is finite and that of the
  same LDI whose pixels there are masked out instead."""
  monkeypatch.setenv('LSI_BWD_STREAM', '1')
  nl, b, h, w = 2, 2, 32, 128
  tex, mask, disp = _ldi(nl, b, h, w, 14)
  mat = _mat64(*_cameras(b, h, w, path != 'stream', 8)).to(torch.float32)
  g = torch.Generator().manual_seed(9)
  bad = torch.rand(disp.shape, generator=g) < 0.02
  vals = torch.tensor([float('nan'), float('inf'), -float('inf')])
  disp_bad = disp.clone()
  disp_bad[bad] = vals[torch.randint(0, 3, (int(bad.sum()),), generator=g)]
  mask_drop = torch.where(bad, torch.zeros_like(mask), mask)
  ci, cc = _cotangents((1, b, h // 2, w // 2, 3), (1,), 25)
  g_bad = _matrix_grad(dev, tex, mask, disp_bad, mat, True, path, ci, cc)
  g_drop = _matrix_grad(dev, tex, mask_drop, disp, mat, True, path, ci, cc)
  assert bool(torch.isfinite(g_bad).all())
  np.testing.assert_allclose(g_bad.cpu().numpy(), g_drop.cpu().numpy(), rtol=1e-5,
                             atol=1e-6 * float(g_drop.abs().max()))


@pytest.mark.parametrize('stream', ['1', '0'])
@pytest.mark.parametrize('call', [True, 'both'])
def test_other_gradients_unchanged_and_grad_m_reproducible(dev, monkeypatch, stream, call):
  """Requesting g_M leaves g_tex, g_disp and g_mask bitwise as they were, on
  both backward kernels; two runs give bitwise the same g_M.  (The forward
  runs with LSI_DETERMINISTIC so that every backward sees the same outputs;
  the backward kernels use no atomics either way.)"""
  from lsi.geometry import ldi
  monkeypatch.setenv('LSI_BWD_STREAM', stream)
  nl, b, h, w = 2, 2, 64, 256
  tex, mask, disp = _ldi(nl, b, h, w, 15)
  mat = _mat64(*_cameras(b, h, w, False, 9)).to(torch.float32)
  ci, cc = _cotangents((1 if call is True else nl, b, h // 2, w // 2, 3),
                       (1, b, h // 2, w // 2, 3), 26)
  res = []
  for want_m in (False, True, True):
    t = tex.to(dev).requires_grad_(True)
    d = disp.to(dev).requires_grad_(True)
    k = mask.to(dev).requires_grad_(True)
    m = mat.clone().requires_grad_(want_m)
    kw = dict(trg_downsampling=S, bg_layer_disp=BG, max_disp=MD, zbuf_scale=ZB,
              deterministic=True)
    outs = (ldi.forward_splat_both([t, k, d], m, **kw) if call == 'both' else
            ldi.forward_splat_matrix([t, k, d], m, compose_layers=True, **kw))
    _loss(outs, ci, cc).backward()
    res.append((t.grad.cpu(), d.grad.cpu(), k.grad.cpu(),
                m.grad.cpu() if want_m else None))
  for i in range(3):
    assert torch.equal(res[0][i], res[1][i]) and torch.equal(res[0][i], res[2][i]), i
  assert torch.equal(res[1][3], res[2][3])


def test_pose_refinement_converges(dev):
  """End to end: a smooth textured plane seen from a target camera; the pose
  starts ~2 target pixels off in translation plus a small roll.  Adam on t and
  rot alone, driven by the photometric loss through forward_splat, brings the
  mean reprojection error of the plane's pixels down at least 10x."""
  from lsi.geometry import ldi
  h = w = 64
  f = 0.8 * w
  k = torch.tensor([[[f, 0.0, w / 2], [0.0, f, h / 2], [0.0, 0.0, 1.0]]])
  ys, xs = torch.meshgrid(torch.arange(h) + 0.5, torch.arange(w) + 0.5, indexing='ij')
  tex = torch.stack([
      0.5 + 0.25 * torch.sin(2 * math.pi * xs / 29 + 0.3) + 0.2 * torch.cos(2 * math.pi * ys / 23),
      0.5 + 0.3 * torch.sin(2 * math.pi * (xs + ys) / 37),
      0.5 + 0.3 * torch.cos(2 * math.pi * (xs - 0.5 * ys) / 31)], -1)[None, None]
  disp = (0.4 + 0.1 * xs / w + 0.05 * ys / h)[None, None, ..., None]
  src = [tex.to(dev), None, disp.to(dev)]
  kw = dict(trg_downsampling=1, bg_layer_disp=1e-3, max_disp=1.0, zbuf_scale=10.0)
  rot_true = torch.eye(3)[None]
  t_true = torch.tensor([[[-0.2], [0.0], [0.0]]])
  with torch.no_grad():
    target, _ = ldi.forward_splat(src, None, k, k, rot_true, t_true, **kw)
  p = torch.stack([xs, ys, torch.ones_like(xs), disp[0, 0, ..., 0]], -1).double()

  def reproj(rot, t):
    from lsi.geometry import projection
    def uv(r, tt):
      m = projection.forward_projection_matrix(k, k, r, tt)[0].double()
      q = p @ m.T
      return q[..., :2] / q[..., 2:3]
    return float((uv(rot, t) - uv(rot_true, t_true)).norm(dim=-1).mean())

  rot = _rodrigues(torch.tensor([[0.0, 0.0, 0.015]])).clone().requires_grad_(True)
  t = (t_true + torch.tensor([[[2.0], [1.0], [0.0]]]) / (f * 0.45)).requires_grad_(True)
  e0 = reproj(rot.detach(), t.detach())
  assert 1.5 < e0 < 4.0, e0
  opt = torch.optim.Adam([t, rot], lr=3e-3)
  border = 6
  for _ in range(120):
    opt.zero_grad()
    img, _ = ldi.forward_splat(src, None, k, k, rot, t, **kw)
    loss = ((img - target)[:, :, border:-border, border:-border] ** 2).mean()
    loss.backward()
    assert rot.grad is not None and t.grad is not None
    opt.step()
  e1 = reproj(rot.detach(), t.detach())
  print('pose refinement: mean reprojection error %.3f -> %.4f px' % (e0, e1))
  assert e1 * 10 <= e0, (e0, e1)
