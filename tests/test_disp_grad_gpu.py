"""The gradient of forward_splat's target disparity (compute_trg_disp=True) on
the MI355X: lsi_splat_bwd_disp, through both backward kernels, against fp64
autograd of the reference's op graph (ldi.py:129-171) restated below.

Bar, as tests/test_camera_grad_gpu.py: the kernels' error against fp64 is at
most twice that of the same op graph run in fp32 (what the reference's own
autodiff computes), plus a floor of the largest entry: 1e-6 there, 1e-4 here
(the target disparity is a ratio of two canvases that the forward kernels sum
in their own order: the general-pose divisions show it).  Per-pixel
gradients are compared where a pixel's floor / clamp / clip decisions come
out the same in fp32 and fp64 (lsi_oracle.decisions_are_robust)."""
import ctypes

import numpy as np
import pytest
import torch

import lsi_oracle as O
import lsi_torch_ref as TR

pytestmark = pytest.mark.gpu

MD, ZB = 0.4, 10.0


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


# ---------------------------------------------------------------------------
# the oracle: ldi.py:129-171 in torch, composed with amax (TF's reduce_max
# gradient: an even split among tied layers)
# ---------------------------------------------------------------------------
def oracle_splat(tex, mask, disp, mat, s, bg_layer_disp, compose, max_disp=MD,
                 zbuf_scale=ZB):
  nl, b, h, w, c = tex.shape
  dt = tex.dtype
  ht, wt = int(h * s), int(w * s)
  bg = TR.zbuffer_weights(torch.tensor(bg_layer_disp / max_disp, dtype=dt), zbuf_scale)
  xs = (torch.arange(w, dtype=dt) + 0.5).view(1, 1, w).expand(b, h, w)
  ys = (torch.arange(h, dtype=dt) + 0.5).view(1, h, 1).expand(b, h, w)
  imgs, wtss, dsps = [], [], []
  for l in range(nl):
    p = torch.stack([xs, ys, torch.ones_like(xs), disp[l, ..., 0]], -1)
    q = torch.einsum('bhwk,bjk->bhwj', p, mat.to(dt))
    uv = TR.divide_safe(q[..., 0:2], q[..., 2:3]) * s
    dd = TR.divide_safe(q[..., 3:4], q[..., 2:3])
    pw = TR.zbuffer_weights(dd / max_disp, zbuf_scale)
    if mask is not None:
      pw = pw * mask[l]
    imgs.append(TR.splat(tex[l] * pw, uv, torch.ones((b, ht, wt, c), dtype=dt) * bg))
    wtss.append(TR.splat(pw, uv, torch.ones((b, ht, wt, 1), dtype=dt) * bg))
    dsps.append(TR.splat(dd * pw, uv, torch.zeros((b, ht, wt, 1), dtype=dt)))
  img, wts, dsp = torch.stack(imgs), torch.stack(wtss), torch.stack(dsps)
  dsp = TR.divide_safe(dsp, wts)
  if compose:
    img = img.sum(0, keepdim=True)
    wts = wts.sum(0, keepdim=True)
    dsp = dsp.amax(0, keepdim=True)
  return TR.divide_safe(img, wts), wts, dsp


def _oracle_grads(tex, mask, disp, mat, s, bg, compose, dtype, loss_fn):
  def leaf(x):
    return x.detach().to(dtype).clone().requires_grad_(True)

  leaves = {'tex': leaf(tex), 'disp': leaf(disp), 'M': leaf(mat)}
  if mask is not None:
    leaves['mask'] = leaf(mask)
  outs = oracle_splat(leaves['tex'], leaves.get('mask'), leaves['disp'], leaves['M'],
                      s, bg, compose)
  loss_fn(*outs).backward()
  return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double()
          for k, v in leaves.items()}


def _kernel_grads(dev, tex, mask, disp, mat, s, bg, compose, loss_fn, path='auto',
                  packed=False, deterministic=False):
  from lsi.geometry import ldi
  if packed:
    pred = torch.cat([tex, disp], -1).to(dev).requires_grad_(True)
    t, d = pred[..., 0:3], pred[..., 3:4]
  else:
    t = tex.to(dev).requires_grad_(True)
    d = disp.to(dev).requires_grad_(True)
  k = mask.to(dev).requires_grad_(True) if mask is not None else None
  m = mat.clone().requires_grad_(True)
  img, wts, dsp = ldi.forward_splat_matrix(
      [t, k, d], m, compose_layers=compose, compute_trg_disp=True, trg_downsampling=s,
      bg_layer_disp=bg, max_disp=MD, zbuf_scale=ZB, path=path,
      deterministic=deterministic)
  loss_fn(img, wts, dsp).backward()
  if packed:
    g = {'tex': pred.grad[..., 0:3], 'disp': pred.grad[..., 3:4]}
  else:
    g = {'tex': t.grad, 'disp': d.grad}
  if k is not None:
    g['mask'] = k.grad
  g['M'] = m.grad
  return {n: v.detach().cpu() for n, v in g.items()}


def _check(name, got, g64, g32, where=None):
  got, g64, g32 = got.double(), g64.double(), g32.double()
  if where is not None:
    got, g64, g32 = got * where, g64 * where, g32 * where
  scale = float(g64.abs().max()) + 1e-30
  err = float((got - g64).abs().max())
  err32 = float((g32 - g64).abs().max())
  print('%s: |kernel - fp64| %.2e, |fp32 graph - fp64| %.2e (of %.2e)'
        % (name, err, err32, scale))
  assert bool(torch.isfinite(got).all()), name
  assert err <= 2.0 * err32 + 1e-4 * scale, (name, err, err32, scale)


def _firm(mat, disp, s):
  """B x H x W robust-decision masks per layer: L x B x H x W x 1."""
  ht, wt = int(disp.shape[2] * s), int(disp.shape[3] * s)
  return torch.tensor(np.stack([O.decisions_are_robust(mat.numpy(), disp[l, ..., 0].numpy(),
                                                       s, ht, wt, MD)
                                for l in range(disp.shape[0])])[..., None])


def _compare(got, g64, g32, mat, disp, s, names, tag):
  firm = _firm(mat, disp, s).double()
  assert firm.mean() > 0.9, float(firm.mean())
  for n in names:
    if n == 'M':
      _check('%s %s' % (tag, n), got[n], g64[n], g32[n])
    else:
      _check('%s %s' % (tag, n), got[n], g64[n], g32[n], firm)


def _cams_rectified(b, h, w, seed):
  g = torch.Generator().manual_seed(seed)
  mats = []
  for _ in range(b):
    m = torch.eye(4)
    m[0, 0] = 1.0 + 0.05 * (float(torch.rand((), generator=g)) - 0.5)
    m[0, 2] = 2.0 * (float(torch.rand((), generator=g)) - 0.5)
    m[0, 3] = -0.3 * w
    m[1, 2] = 0.5 * (float(torch.rand((), generator=g)) - 0.5)
    mats.append(m)
  return torch.stack(mats)


def _cams_general(b, h, w, seed):
  """K [R t] K^-1 with a small rotation and a 3-D translation."""
  g = torch.Generator().manual_seed(seed)
  f = 0.58 * w
  k = torch.tensor([[f, 0.0, w / 2, 0.0], [0.0, f, h / 2, 0.0], [0.0, 0.0, 1.0, 0.0],
                    [0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)
  mats = []
  for _ in range(b):
    a = 0.02 * (torch.rand(3, generator=g, dtype=torch.float64) - 0.5)
    sk = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]],
                      dtype=torch.float64)
    e = torch.eye(4, dtype=torch.float64)
    e[:3, :3] = torch.linalg.matrix_exp(sk)
    e[:3, 3] = torch.tensor([-0.5, 0.02, 0.03], dtype=torch.float64) + \
        0.02 * torch.rand(3, generator=g, dtype=torch.float64)
    mats.append(k @ e @ torch.linalg.inv(k))
  return torch.stack(mats).to(torch.float32)


def _ldi(nl, b, h, w, seed, mask=True, zero_mask=0.1):
  g = torch.Generator().manual_seed(seed)
  tex = torch.rand((nl, b, h, w, 3), generator=g)
  base = torch.rand((nl * b, 1, max(h // 4, 1), max(w // 4, 1)), generator=g)
  field = torch.nn.functional.interpolate(base, size=(h, w), mode='bilinear',
                                          align_corners=False)
  scale = torch.tensor([(nl - l) / nl for l in range(nl)]).view(nl, 1, 1, 1, 1)
  disp = (MD * (0.2 + 0.75 * field.reshape(nl, b, h, w, 1)) * scale).contiguous()
  msk = None
  if mask:
    msk = 0.3 + 0.7 * torch.rand((nl, b, h, w, 1), generator=g)
    msk[torch.rand(msk.shape, generator=g) < zero_mask] = 0.0
  return tex, msk, disp


def _coef(shape, seed):
  g = torch.Generator().manual_seed(seed)
  return torch.rand(shape, generator=g) - 0.3


def _dsp_loss(c):
  return lambda img, wts, dsp: (dsp * c.to(dsp)).sum()


# ---------------------------------------------------------------------------
def test_disparity_output_is_differentiable(dev):
  """The gradient that used to be missing: torch.autograd.grad of a loss on
  the target disparity alone w.r.t. the source disparities and masks."""
  from lsi.geometry import ldi
  nl, b, h, w, s, bg = 2, 2, 16, 32, 0.5, 0.2
  tex, mask, disp = _ldi(nl, b, h, w, 1)
  mat = _cams_general(b, h, w, 2)
  c = _coef((1, b, int(h * s), int(w * s), 1), 3)
  d = disp.to(dev).requires_grad_(True)
  k = mask.to(dev).requires_grad_(True)
  _, _, dsp = ldi.forward_splat_matrix([tex.to(dev), k, d], mat, compose_layers=True,
                                       compute_trg_disp=True, trg_downsampling=s,
                                       bg_layer_disp=bg, max_disp=MD, zbuf_scale=ZB)
  gd, gk = torch.autograd.grad((dsp * c.to(dev)).sum(), [d, k])
  got = {'disp': gd.cpu(), 'mask': gk.cpu()}
  g64 = _oracle_grads(tex, mask, disp, mat, s, bg, True, torch.float64, _dsp_loss(c))
  g32 = _oracle_grads(tex, mask, disp, mat, s, bg, True, torch.float32, _dsp_loss(c))
  _compare(got, g64, g32, mat, disp, s, ('disp', 'mask'), 'grad')


@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('bg', [0.0, 0.2])
@pytest.mark.parametrize('compose', [True, False])
@pytest.mark.parametrize('stream', ['1', '0'])
def test_rectified_against_fp64(dev, monkeypatch, stream, compose, bg, packed):
  """Rectified pairs (the STREAM forward when composed; the streamed backward
  with LSI_BWD_STREAM=1, the gather kernel with 0), RGBD pixels and separate
  tensors, bg_layer_disp 0 (W' = 1e-8 on empty cells) and 0.2."""
  from lsi import _C
  from lsi.geometry import ldi
  monkeypatch.setenv('LSI_BWD_STREAM', stream)
  nl, b, h, w, s = 3, 2, 24, 256, 0.5
  tex, _, disp = _ldi(nl, b, h, w, 10 + packed, mask=False)
  mat = _cams_rectified(b, h, w, 4)
  if compose:
    assert ldi.plan_key((nl, b, h, w), s, MD, mat)[0] == _C.LSI_PATH_STREAM
  nlo = 1 if compose else nl
  c = _coef((nlo, b, int(h * s), int(w * s), 1), 5)
  got = _kernel_grads(dev, tex, None, disp, mat, s, bg, compose, _dsp_loss(c),
                      packed=packed)
  assert bool((got['tex'] == 0).all())
  g64 = _oracle_grads(tex, None, disp, mat, s, bg, compose, torch.float64, _dsp_loss(c))
  g32 = _oracle_grads(tex, None, disp, mat, s, bg, compose, torch.float32, _dsp_loss(c))
  _compare(got, g64, g32, mat, disp, s, ('disp', 'M'),
           'rect stream=%s compose=%s bg=%s packed=%s' % (stream, compose, bg, packed))


@pytest.mark.parametrize('s', [1.0, 0.5, 0.25])
@pytest.mark.parametrize('bg', [0.0, 0.2])
@pytest.mark.parametrize('compose', [True, False])
@pytest.mark.parametrize('path', ['tile', 'atomic'])
def test_general_pose_against_fp64(dev, path, compose, bg, s):
  """General poses with a mask (zeros included) on the tile and atomic
  forwards: the gather backward's general branch."""
  nl, b, h, w = 3, 2, 16, 48
  tex, mask, disp = _ldi(nl, b, h, w, 20)
  mat = _cams_general(b, h, w, 6)
  nlo = 1 if compose else nl
  c = _coef((nlo, b, int(h * s), int(w * s), 1), 7)
  got = _kernel_grads(dev, tex, mask, disp, mat, s, bg, compose, _dsp_loss(c), path=path)
  assert bool((got['tex'] == 0).all())
  g64 = _oracle_grads(tex, mask, disp, mat, s, bg, compose, torch.float64, _dsp_loss(c))
  g32 = _oracle_grads(tex, mask, disp, mat, s, bg, compose, torch.float32, _dsp_loss(c))
  _compare(got, g64, g32, mat, disp, s, ('disp', 'mask', 'M'),
           'general %s compose=%s bg=%s s=%s' % (path, compose, bg, s))


@pytest.mark.parametrize('general', [False, True])
def test_camera_and_focal_grads(dev, general):
  """k_s, k_t, rot, t and focal_disps receive the disparity's share (through
  forward_splat, the matrix built by differentiable torch ops)."""
  from lsi.geometry import ldi
  nl, b, h, w, s, bg = 2, 2, 16, 64, 0.5, 0.2
  tex, mask, disp = _ldi(nl, b, h, w, 30, mask=general)
  g = torch.Generator().manual_seed(8)
  f = 0.58 * w
  k = torch.tensor([[f, 0.0, w / 2], [0.0, f, h / 2], [0.0, 0.0, 1.0]]).repeat(b, 1, 1)
  if general:
    a = 0.02 * (torch.rand((b, 3), generator=g) - 0.5)
    z = torch.zeros(b)
    rot = torch.linalg.matrix_exp(torch.stack([
        torch.stack([z, -a[:, 2], a[:, 1]], -1), torch.stack([a[:, 2], z, -a[:, 0]], -1),
        torch.stack([-a[:, 1], a[:, 0], z], -1)], 1))
    t = torch.tensor([[-0.5], [0.02], [0.03]]) + 0.02 * torch.rand((b, 3, 1), generator=g)
  else:
    rot = torch.eye(3).repeat(b, 1, 1)
    t = torch.tensor([[-0.5], [0.0], [0.0]]).repeat(b, 1, 1)
  cams = [k, k.clone(), rot, t]
  focal = torch.tensor([0.03, -0.02]).view(b, 1, 1, 1)
  c = _coef((1, b, int(h * s), int(w * s), 1), 9)

  leaves = [x.clone().requires_grad_(True) for x in cams]
  fl = focal.clone().requires_grad_(True)
  src = [tex.to(dev), None if mask is None else mask.to(dev), disp.to(dev)]
  _, _, dsp = ldi.forward_splat(src, None, *leaves, focal_disps=fl, compute_trg_disp=True,
                                trg_downsampling=s, bg_layer_disp=bg, max_disp=MD,
                                zbuf_scale=ZB)
  (dsp * c.to(dev)).sum().backward()
  got = [x.grad for x in leaves] + [fl.grad]

  def ref(dtype):
    lv = [x.to(dtype).clone().requires_grad_(True) for x in cams]
    ff = focal.to(dtype).clone().requires_grad_(True)
    bb = lv[0].shape[0]
    eye = torch.eye(4, dtype=dtype).repeat(bb, 1, 1)
    kt = torch.cat([torch.cat([lv[1], torch.zeros((bb, 3, 1), dtype=dtype)], 2), eye[:, 3:]], 1)
    ks = torch.cat([torch.cat([torch.linalg.inv(lv[0]), torch.zeros((bb, 3, 1), dtype=dtype)],
                              2), eye[:, 3:]], 1)
    e = torch.cat([torch.cat([lv[2], lv[3]], 2), eye[:, 3:]], 1)
    m = kt @ e @ ks
    m = torch.cat([m[:, :3], (m[:, 3] + ff.reshape(bb, 1) * m[:, 2])[:, None]], 1)
    d = disp.to(dtype) - ff.view(1, -1, 1, 1, 1)
    _, _, dd = oracle_splat(tex.to(dtype), None if mask is None else mask.to(dtype), d, m,
                            s, bg, True)
    (dd * c.to(dtype)).sum().backward()
    return [x.grad.double() for x in lv] + [ff.grad.double()]

  g64, g32 = ref(torch.float64), ref(torch.float32)
  for name, a, r64, r32 in zip(('k_s', 'k_t', 'rot', 't', 'focal_disps'), got, g64, g32):
    _check('%s general=%s' % (name, general), a.cpu(), r64, r32)


@pytest.mark.parametrize('compose', [True, False])
@pytest.mark.parametrize('stream', ['1', '0'])
def test_mixed_loss_is_the_sum_of_the_separate_backwards(dev, monkeypatch, stream, compose):
  """img, wts and dsp terms in one loss: the gradients are the sum of the
  three backwards run one term at a time (deterministic forwards: the same
  outputs each time)."""
  monkeypatch.setenv('LSI_BWD_STREAM', stream)
  nl, b, h, w, s, bg = 3, 2, 24, 256, 0.5, 0.2
  tex, _, disp = _ldi(nl, b, h, w, 40, mask=False)
  mat = _cams_rectified(b, h, w, 11)
  nlo = 1 if compose else nl
  ci = _coef((nlo, b, h // 2, w // 2, 3), 12)
  cw = _coef((nlo, b, h // 2, w // 2, 1), 13)
  cd = _coef((nlo, b, h // 2, w // 2, 1), 14)
  terms = [lambda i, wt, d: (i * ci.to(i)).sum(),
           lambda i, wt, d: 1e-2 * (torch.log(wt) * cw.to(wt)).sum(),
           lambda i, wt, d: (d * cd.to(d)).sum()]
  sep = [_kernel_grads(dev, tex, None, disp, mat, s, bg, compose, f, deterministic=True)
         for f in terms]
  both = _kernel_grads(dev, tex, None, disp, mat, s, bg, compose,
                       lambda i, wt, d: sum(f(i, wt, d) for f in terms), deterministic=True)
  for n in ('tex', 'disp', 'M'):
    want = sep[0][n] + sep[1][n] + sep[2][n]
    scale = float(want.abs().max())
    err = float((both[n] - want).abs().max())
    assert err <= 1e-5 * scale, (n, err, scale)


@pytest.mark.parametrize('route', ['stream', 'gather', 'tile'])
def test_ties_split_evenly(dev, monkeypatch, route):
  """Exact ties: layer 1 duplicates layer 0 (every cell they reach is a 2-way
  tie) and a masked-out band leaves cells that no layer reaches (all layers
  at 0: an L-way tie).  TF's reduce_max gradient splits evenly, so the two
  duplicated layers get the same gradient, half of what one layer alone
  would get."""
  monkeypatch.setenv('LSI_BWD_STREAM', '0' if route == 'gather' else '1')
  nl, b, h, w, s, bg = 3, 1, 16, 128, 0.5, 0.2
  tex, mask, disp = _ldi(nl, b, h, w, 50, mask=(route == 'tile'), zero_mask=0.0)
  tex[1], disp[1] = tex[0], disp[0]
  if mask is not None:
    mask[1] = mask[0]
    mask[:, :, 4:8] = 0.0     # rows no layer renders
  mat = _cams_general(b, h, w, 15) if route == 'tile' else _cams_rectified(b, h, w, 15)
  c = _coef((1, b, h // 2, w // 2, 1), 16)
  got = _kernel_grads(dev, tex, mask, disp, mat, s, bg, True, _dsp_loss(c))
  scale = float(got['disp'].abs().max())
  assert float((got['disp'][0] - got['disp'][1]).abs().max()) <= 1e-5 * scale
  g64 = _oracle_grads(tex, mask, disp, mat, s, bg, True, torch.float64, _dsp_loss(c))
  g32 = _oracle_grads(tex, mask, disp, mat, s, bg, True, torch.float32, _dsp_loss(c))
  _compare(got, g64, g32, mat, disp, s, ('disp', 'M') + (('mask',) if mask is not None else ()),
           'ties %s' % route)
  # one of the duplicated layers alone receives twice the share
  one = _kernel_grads(dev, tex[[0, 2]], None if mask is None else mask[[0, 2]],
                      disp[[0, 2]], mat, s, bg, True, _dsp_loss(c))
  scale = float(one['disp'].abs().max())
  assert float((2 * got['disp'][0] - one['disp'][0]).abs().max()) <= 1e-4 * scale


@pytest.mark.parametrize('route', ['stream', 'gather', 'tile'])
def test_nonfinite_disparities_give_zero_gradient(dev, monkeypatch, route):
  monkeypatch.setenv('LSI_BWD_STREAM', '0' if route == 'gather' else '1')
  nl, b, h, w, s, bg = 2, 2, 16, 128, 0.5, 0.2
  tex, mask, disp = _ldi(nl, b, h, w, 60, mask=(route == 'tile'))
  mat = _cams_general(b, h, w, 17) if route == 'tile' else _cams_rectified(b, h, w, 17)
  g = torch.Generator().manual_seed(18)
  bad = torch.rand(disp.shape, generator=g) < 0.03
  vals = torch.tensor([float('nan'), float('inf'), -float('inf')])
  disp[bad] = vals[torch.randint(0, 3, (int(bad.sum()),), generator=g)]
  c = _coef((1, b, h // 2, w // 2, 1), 19)
  got = _kernel_grads(dev, tex, mask, disp, mat, s, bg, True, _dsp_loss(c))
  for n, v in got.items():
    assert bool(torch.isfinite(v).all()), n
  assert bool((got['disp'][bad] == 0).all())
  assert float(got['disp'][~bad].abs().max()) > 0


def test_agrees_with_the_generic_route(dev):
  """Coordinates that require grad take _forward_splat_coords (differentiable
  torch ops + lsi_splat_generic).  Where every pixel has weight > 0 the two
  routes give the same gradients."""
  from lsi.geometry import ldi
  nl, b, h, w, s, bg = 2, 2, 16, 48, 0.5, 0.2
  tex, mask, disp = _ldi(nl, b, h, w, 70, zero_mask=0.0)
  k = torch.tensor([[30.0, 0.0, 24.0], [0.0, 30.0, 8.0], [0.0, 0.0, 1.0]]).repeat(b, 1, 1)
  rot = torch.eye(3).repeat(b, 1, 1)
  t = torch.tensor([[-0.3], [0.01], [0.02]]).repeat(b, 1, 1)
  c = _coef((1, b, h // 2, w // 2, 1), 21)
  ys, xs = torch.meshgrid(torch.arange(h) + 0.5, torch.arange(w) + 0.5, indexing='ij')
  grid = torch.stack([xs, ys, torch.ones_like(xs)], -1)[None].repeat(b, 1, 1, 1)
  res = []
  for coords in (None, grid.to(dev).requires_grad_(True)):
    d = disp.to(dev).requires_grad_(True)
    m = mask.to(dev).requires_grad_(True)
    _, _, dsp = ldi.forward_splat([tex.to(dev), m, d], coords, k, k, rot, t,
                                  compute_trg_disp=True, trg_downsampling=s,
                                  bg_layer_disp=bg, max_disp=MD, zbuf_scale=ZB)
    (dsp * c.to(dev)).sum().backward()
    res.append((d.grad.cpu(), m.grad.cpu()))
  for a, g_, n in zip(res[0], res[1], ('disp', 'mask')):
    scale = float(g_.abs().max())
    bad = (a - g_).abs() > 1e-3 * scale
    assert float(bad.float().mean()) < 0.01, (n, float(bad.float().mean()))


def test_mask_gradient_diverges_from_the_generic_route_as_tf(dev):
  """Pinned divergence: a landed pixel of mask 0 gets the mask
  gradient TF gives, c * D * zbuf * gS (the oracle's), while the generic
  route's where(pw != 0, ...) gives it 0."""
  from lsi.geometry import ldi
  nl, b, h, w, s, bg = 1, 1, 16, 48, 0.5, 0.2
  tex, mask, disp = _ldi(nl, b, h, w, 71, zero_mask=0.0)
  mask[:, :, 6:10, 10:30] = 0.0
  zero = (mask == 0)
  k = torch.tensor([[30.0, 0.0, 24.0], [0.0, 30.0, 8.0], [0.0, 0.0, 1.0]])[None]
  rot, t = torch.eye(3)[None], torch.tensor([[[-0.3], [0.0], [0.0]]])
  c = _coef((1, b, h // 2, w // 2, 1), 22)
  ys, xs = torch.meshgrid(torch.arange(h) + 0.5, torch.arange(w) + 0.5, indexing='ij')
  grid = torch.stack([xs, ys, torch.ones_like(xs)], -1)[None]
  res = []
  for coords in (None, grid.to(dev).requires_grad_(True)):
    m = mask.to(dev).requires_grad_(True)
    _, _, dsp = ldi.forward_splat([tex.to(dev), m, disp.to(dev)], coords, k, k, rot, t,
                                  compute_trg_disp=True, trg_downsampling=s,
                                  bg_layer_disp=bg, max_disp=MD, zbuf_scale=ZB)
    (dsp * c.to(dev)).sum().backward()
    res.append(m.grad.cpu())
  fused, generic = res
  # (the generic route keeps the weight canvas' share there, drops the rest)
  diff = (fused - generic)[zero]
  assert float(diff.abs().max()) > 1e-3 * float(fused.abs().max())
  scale = float(fused.abs().max())
  assert float((fused - generic)[~zero].abs().max()) <= 1e-3 * scale
  from lsi.geometry import projection
  mat = projection.forward_projection_matrix(k, k, rot, t)
  g64 = _oracle_grads(tex, mask, disp, mat, s, bg, True, torch.float64, _dsp_loss(c))
  g32 = _oracle_grads(tex, mask, disp, mat, s, bg, True, torch.float32, _dsp_loss(c))
  _compare({'mask': fused}, g64, g32, mat, disp, s, ('mask',), 'divergence')


def test_full_size_cfg3(dev, monkeypatch):
  """BASELINE config 3's shape (4 layers, 256 x 768, s = 0.5, composed, RGBD
  pixels), one batch element: the streamed and the gather backward against
  fp64."""
  import bench
  nl, h, w, _, _, cams, md, bg = bench.WORKLOADS['cfg3']
  assert md == MD
  tex, disp, mat = bench.make_inputs(nl, 1, h, w, cams, md, 78, torch.device('cpu'))
  c = _coef((1, 1, h // 2, w // 2, 1), 23)
  got = {}
  for stream in ('1', '0'):
    monkeypatch.setenv('LSI_BWD_STREAM', stream)
    got[stream] = _kernel_grads(dev, tex, None, disp, mat, 0.5, bg, True, _dsp_loss(c),
                                packed=True)
  g64 = _oracle_grads(tex, None, disp, mat, 0.5, bg, True, torch.float64, _dsp_loss(c))
  g32 = _oracle_grads(tex, None, disp, mat, 0.5, bg, True, torch.float32, _dsp_loss(c))
  for stream, g in got.items():
    _compare(g, g64, g32, mat, disp, 0.5, ('disp', 'M'), 'cfg3 stream=%s' % stream)


@pytest.mark.parametrize('compose', [False, True])
@pytest.mark.parametrize('route', ['stream', 'gather', 'tile'])
def test_reproducible(dev, monkeypatch, route, compose):
  """Repeated backwards of one forward: per-layer output bitwise the same;
  composed (the per-layer canvases are rendered again, in no fixed order) the
  same to rounding."""
  from lsi.geometry import ldi
  monkeypatch.setenv('LSI_BWD_STREAM', '0' if route == 'gather' else '1')
  nl, b, h, w, s, bg = 3, 2, 24, 256, 0.5, 0.2
  tex, mask, disp = _ldi(nl, b, h, w, 80, mask=(route == 'tile'))
  mat = _cams_general(b, h, w, 24) if route == 'tile' else _cams_rectified(b, h, w, 24)
  c = _coef((1 if compose else nl, b, h // 2, w // 2, 1), 25)
  t = tex.to(dev).requires_grad_(True)
  d = disp.to(dev).requires_grad_(True)
  k = mask.to(dev).requires_grad_(True) if mask is not None else None
  m = mat.clone().requires_grad_(True)
  _, _, dsp = ldi.forward_splat_matrix([t, k, d], m, compose_layers=compose,
                                       compute_trg_disp=True, trg_downsampling=s,
                                       bg_layer_disp=bg, max_disp=MD, zbuf_scale=ZB)
  loss = (dsp * c.to(dev)).sum()
  leaves = [x for x in (d, k, m) if x is not None]
  runs = [torch.autograd.grad(loss, leaves, retain_graph=True) for _ in range(3)]
  for i in range(len(leaves)):
    if compose:
      scale = float(runs[0][i].abs().max())
      for r in runs[1:]:
        assert float((r[i] - runs[0][i]).abs().max()) <= 1e-4 * scale, i
    else:
      assert torch.equal(runs[0][i], runs[1][i]) and torch.equal(runs[0][i], runs[2][i]), i


class _CountingLib(object):
  def __init__(self, lib, names):
    self._lib, self._names = lib, names

  def __getattr__(self, name):
    self._names.append(name)
    return getattr(self._lib, name)


@pytest.mark.parametrize('grad_m', [False, True])
@pytest.mark.parametrize('route', ['stream', 'tile'])
def test_no_disparity_gradient_no_change(dev, monkeypatch, route, grad_m):
  """compute_trg_disp=True with the disparity left out of the loss: the
  backward calls lsi_splat_bwd / lsi_splat_bwd_m as before (no new entry),
  and its gradients are bitwise what that entry gives for the same forward
  outputs."""
  from lsi import _C
  from lsi.geometry import ldi
  nl, b, h, w, s, bg = 3, 2, 24, 256, 0.5, 0.2
  tex, mask, disp = _ldi(nl, b, h, w, 90, mask=(route == 'tile'))
  mat = _cams_general(b, h, w, 26) if route == 'tile' else _cams_rectified(b, h, w, 26)
  ci = _coef((1, b, h // 2, w // 2, 3), 27)
  t = tex.to(dev).requires_grad_(True)
  d = disp.to(dev).requires_grad_(True)
  k = mask.to(dev).requires_grad_(True) if mask is not None else None
  m = mat.clone().requires_grad_(grad_m)
  img, wts, dsp = ldi.forward_splat_matrix([t, k, d], m, compose_layers=True,
                                           compute_trg_disp=True, trg_downsampling=s,
                                           bg_layer_disp=bg, max_disp=MD, zbuf_scale=ZB)
  assert dsp.requires_grad
  node = img.grad_fn
  desc = _C.LsiSplatDesc.from_buffer_copy(node.desc)
  saved = [x.detach() for x in node.saved_tensors]
  names = []
  real = _C.lib()
  monkeypatch.setattr(_C, 'lib', lambda: _CountingLib(real, names))
  ((img * ci.to(dev)).sum() + 1e-2 * torch.log(wts).sum()).backward()
  monkeypatch.undo()
  assert not [n for n in names if 'disp' in n], names
  assert ('lsi_splat_bwd_m' if grad_m else 'lsi_splat_bwd') in names, names
  # the same call by hand on the saved forward outputs
  tx, mk, dp, mt, im, wt = saved[:6]
  mk = mk if k is not None else None
  g_img = (ci.expand(im.shape).contiguous()).to(dev)
  g_wts = torch.full_like(wt, 1e-2) / wt   # (what log's backward computes)
  g_tex, g_disp = torch.empty_like(tx), torch.empty_like(dp)
  g_mask = torch.empty_like(mk) if mk is not None else None
  lib = _C.lib()
  if grad_m:
    desc.flags |= _C.LSI_GRAD_M
  g_m = torch.empty((b, 4, 4), device=dev) if grad_m else None
  nbytes = int(lib.lsi_splat_bwd_workspace_bytes(ctypes.byref(desc)))
  ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
  args = [_C.ptr(tx), _C.ptr(dp), _C.ptr(mk), _C.ptr(mt), _C.ptr(im), _C.ptr(wt),
          _C.ptr(g_img), _C.ptr(g_wts), _C.ptr(g_tex), _C.ptr(g_disp), _C.ptr(g_mask)]
  if grad_m:
    rc = lib.lsi_splat_bwd_m(ctypes.byref(desc), *args, _C.ptr(g_m), _C.ptr(ws), nbytes,
                             _C.stream_ptr(dev))
  else:
    rc = lib.lsi_splat_bwd(ctypes.byref(desc), *args, _C.ptr(ws), nbytes, _C.stream_ptr(dev))
  _C.check(rc, 'lsi_splat_bwd')
  torch.cuda.synchronize()
  assert torch.equal(t.grad, g_tex) and torch.equal(d.grad, g_disp)
  if k is not None:
    assert torch.equal(k.grad, g_mask)
  if grad_m:
    assert torch.equal(m.grad.to(dev), g_m)


def test_depth_refinement_converges(dev):
  """End to end: the source disparities of a one-layer LDI are optimised so
  that the rendered target disparity matches a given map (rendered from the
  true disparities); the loss falls at least 100x."""
  from lsi.geometry import ldi
  h, w = 32, 64
  ys, xs = torch.meshgrid(torch.arange(h) + 0.5, torch.arange(w) + 0.5, indexing='ij')
  true = (0.2 + 0.02 * torch.sin(xs / 7.0) + 0.012 * torch.cos(ys / 5.0))[None, None, ..., None]
  tex = torch.full((1, 1, h, w, 3), 0.5)
  mat = torch.eye(4)[None]
  mat[0, 0, 3] = -20.0          # x shift of 20 px per unit disparity
  kw = dict(compose_layers=True, compute_trg_disp=True, trg_downsampling=1,
            bg_layer_disp=0.0, max_disp=MD, zbuf_scale=ZB)
  with torch.no_grad():
    _, _, target = ldi.forward_splat_matrix([tex.to(dev), None, true.to(dev)], mat, **kw)
  est = torch.full_like(true, 0.2).to(dev).requires_grad_(True)
  opt = torch.optim.Adam([est], lr=3e-3)
  band = slice(8, w - 16)

  def loss_of():
    _, _, dsp = ldi.forward_splat_matrix([tex.to(dev), None, est], mat, **kw)
    return ((dsp - target)[:, :, :, band] ** 2).mean()

  l0 = float(loss_of())
  for _ in range(150):
    opt.zero_grad()
    loss = loss_of()
    loss.backward()
    opt.step()
  l1 = float(loss_of())
  print('depth refinement: loss %.3e -> %.3e' % (l0, l1))
  assert l1 * 100 <= l0, (l0, l1)
