"""lsi_compose_bwd, lsi_compose_depth_bwd and lsi_render_planes_bwd on the GPU
against the fp64 autograd of oracle/lsi_torch_ref.py.

Kinks: fp32 and fp64 can fall on different sides of a floor or an arg-max, so a
pixel gets ZERO upstream gradient on both sides where (fp64 oracle, before the
kernel runs) some plane's x or y lies within 1e-3 of an integer or, in hard
modes, the two largest probabilities differ by < 1e-4; at most 5 % of the
pixels may be left out.

Tolerance: per compared tensor, e_ref = error of the same torch restatement run
in fp32 on the CPU against its fp64 run, and the kernel's error against fp64,
both max abs / fp64 max |gradient|; the kernel must stay within 4 e_ref + 1e-6
(4: the atomics' other summation order; 1e-6: fp32 round-off of the largest
element)."""
import ctypes

import numpy as np
import pytest
import torch

import lsi_torch_ref as TR
import layers_grad_ref as R
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def _check(name, got, want64, ref32, against=None):
  """`against`: another fp32 result to compare `got` with instead of fp64."""
  scale = float(want64.abs().max())
  assert scale > 0, name
  e_ref = float((ref32.double() - want64).abs().max()) / scale
  base = want64 if against is None else against.detach().cpu().double()
  e_k = float((got.detach().cpu().double() - base).abs().max()) / scale
  print('%-28s e_kernel %.3g  e_ref %.3g  ratio %.2f' %
        (name, e_k, e_ref, e_k / max(e_ref, 1e-30)))
  assert e_k <= 4 * e_ref + 1e-6, (name, e_k, e_ref)


def _leaf(x, dev):
  return x.detach().float().to(dev).requires_grad_(True)


def _left_out(keep):
  share = 1.0 - float(keep.double().mean())
  print('left out: %d of %d pixels (%.2f %%)' % (int((~keep).sum()), keep.numel(),
                                                 100 * share))
  assert share <= 0.05
  return share


def _grads(fn, inputs, gs, dtype):
  xs = [x.detach().to(dtype).clone().requires_grad_(True) for x in inputs]
  outs = fn(*xs)
  outs = outs if isinstance(outs, tuple) else (outs,)
  pairs = [(o, g.to(dtype)) for o, g in zip(outs, gs) if g is not None]
  return torch.autograd.grad([o for o, _ in pairs], xs, [g for _, g in pairs],
                             allow_unused=True)


# ---------------------------------------------------------------------------
# 1. compose / compose_depth on the reference's planar_transform outputs
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def stored_layers():
  g = golden('layers.npz')
  return [torch.tensor(g[k], dtype=torch.float64)
          for k in ('p_out_imgs', 'p_out_masks', 'p_out_dmaps')]


def _gap_keep(masks, dsel, min_disp, temp):
  p, _ = R.probs(masks, dsel, min_disp, temp)
  top = torch.sort(p, 0)[0]
  return ((top[-1] - top[-2]) >= 1e-4)


@pytest.mark.parametrize('soft,min_disp,temp', [(False, 0.2, 0.4), (False, 1e-6, 1),
                                                (True, 1e-3, 0.4)])
def test_compose_against_the_oracle(dev, stored_layers, soft, min_disp, temp):
  from lsi.geometry import layers
  imgs, masks, dmaps = stored_layers
  assert imgs.shape[1] * imgs.shape[2] * imgs.shape[3] == 640
  g = torch.tensor(np.random.RandomState(11).randn(*imgs.shape[1:]))
  if not soft:
    keep = _gap_keep(masks, dmaps, min_disp, temp)
    assert _left_out(keep) == 0
    g = g * keep
  fn = lambda a, b, c: TR.compose(a, b, c, soft, min_disp, temp)
  want = _grads(fn, (imgs, masks, dmaps), (g,), torch.float64)
  ref = _grads(fn, (imgs, masks, dmaps), (g,), torch.float32)
  xs = [_leaf(x, dev) for x in (imgs, masks, dmaps)]
  out = layers.compose(*xs, soft=soft, min_disp=min_disp, depth_softmax_temp=temp,
                       differentiable=True)
  out.backward(g.float().to(dev))
  _check('g_imgs', xs[0].grad, want[0], ref[0])
  if soft:
    _check('g_masks', xs[1].grad, want[1], ref[1])
    _check('g_dmaps', xs[2].grad, want[2], ref[2])
  else:
    assert not xs[1].grad.any() and not xs[2].grad.any()


@pytest.mark.parametrize('bg_layer', [False, True])
@pytest.mark.parametrize('min_disp,temp', [(0.2, 0.4), (1e-3, 0.4)])
def test_compose_depth_against_the_oracle(dev, stored_layers, bg_layer, min_disp, temp):
  from lsi.geometry import layers
  _, masks, dmaps = stored_layers
  g = torch.tensor(np.random.RandomState(12).randn(*dmaps.shape[1:]))
  d = torch.relu(dmaps)
  dsel = max(float(d.max()), min_disp) - d if bg_layer else dmaps
  keep = _gap_keep(masks, dsel, min_disp, temp)
  _left_out(keep)
  g = g * keep
  fn = lambda a, b: TR.compose_depth(a, b, bg_layer, min_disp, temp)
  want = _grads(fn, (masks, dmaps), (g,), torch.float64)
  ref = _grads(fn, (masks, dmaps), (g,), torch.float32)
  xs = [_leaf(x, dev) for x in (masks, dmaps)]
  out = layers.compose_depth(*xs, bg_layer=bg_layer, min_disp=min_disp,
                             depth_softmax_temp=temp, differentiable=True)
  out.backward(g.float().to(dev))
  _check('g_dmaps', xs[1].grad, want[1], ref[1])
  assert not xs[0].grad.any()


# ---------------------------------------------------------------------------
# 2. known answers
# ---------------------------------------------------------------------------
def test_known_answers_on_eight_pixels(dev):
  from lsi.geometry import layers
  min_disp, temp = 0.2, 0.4
  rs = np.random.RandomState(13)
  imgs = torch.tensor(rs.rand(2, 1, 8, 3))
  masks = torch.tensor(0.2 + 0.7 * rs.rand(2, 1, 8, 1))
  dmaps = torch.tensor(0.3 + 0.4 * rs.rand(2, 1, 8, 1))
  dmaps[0, 0, 0] = -0.1         # pixel 0: layer 0 behind the camera
  dmaps[1, 0, 1] = 0.0          # pixel 1: layer 1 at d == 0
  masks[0, 0, 2] = 0.0          # pixel 2: layer 0 transparent
  masks[:, 0, 3] = 0.0          # pixel 3: both transparent, the background wins
  dmaps[:, 0, 4] = 0.05         # pixel 4: both behind the background, it wins
  g = torch.tensor(rs.randn(1, 8, 3))
  gd = torch.tensor(rs.randn(1, 8, 1))
  for soft in (True, False):
    want = R.compose_closed(imgs, masks, dmaps, g, soft, min_disp, temp)
    ref = R.compose_closed(imgs.float(), masks.float(), dmaps.float(), g.float(), soft,
                           min_disp, temp)
    xs = [_leaf(x, dev) for x in (imgs, masks, dmaps)]
    layers.compose(*xs, soft=soft, min_disp=min_disp,
                   depth_softmax_temp=temp, differentiable=True).backward(g.float().to(dev))
    gi, gm, gdm = [x.grad.cpu() for x in xs]
    assert bool(torch.isfinite(gi).all() and torch.isfinite(gm).all() and
                torch.isfinite(gdm).all())
    _check('g_imgs soft=%d' % soft, gi, want[0], ref[0])
    if soft:
      _check('g_masks', gm, want[1], ref[1])
      _check('g_dmaps', gdm, want[2], ref[2])
      assert float(gdm[0, 0, 0]) == 0 and float(gdm[1, 0, 1]) == 0   # d <= 0
      assert float(gdm[1, 0, 0]) != 0
      # mask == 0: the finite g_z / 1e-8 (g_z itself carries p ~ 1e-8)
      assert float(gm[0, 0, 2]) != 0 and float(want[1][0, 0, 2]) != 0
    else:
      assert not gm.any() and not gdm.any()
      # the background wins pixels 3 and 4: nothing reaches the layers
      assert not gi[:, 0, 3:5].any()
      # elsewhere exactly one layer takes g unchanged
      assert torch.equal(gi[:, 0, :3].sum(0), g.float()[0, :3])
  xs = [_leaf(x, dev) for x in (masks, dmaps)]
  layers.compose_depth(*xs, bg_layer=False, min_disp=min_disp,
                       depth_softmax_temp=temp, differentiable=True).backward(gd.float().to(dev))
  gdm = xs[1].grad.cpu()
  want = R.compose_depth_closed(masks, dmaps, gd, False, min_disp, temp)
  assert torch.equal(gdm, want.float())       # a selection of g
  assert not gdm[:, 0, 3:5].any()             # the background won
  # requires_grad=False: no gradient, no work
  a, b, c = [x.float().to(dev) for x in (imgs, masks, dmaps)]
  b.requires_grad_(True)
  layers.compose(a, b, c, soft=True, min_disp=min_disp,
                 depth_softmax_temp=temp, differentiable=True).sum().backward()
  assert a.grad is None and c.grad is None and b.grad is not None
  # without differentiable=True the calls stay the forward-only ones they were
  with pytest.raises(RuntimeError, match='differentiable=True'):
    layers.compose(a, b, c, soft=True)
  with pytest.raises(RuntimeError, match='differentiable=True'):
    layers.compose_depth(b, c)


# ---------------------------------------------------------------------------
# 3. the fused renderer against the oracle
# ---------------------------------------------------------------------------
def _desc(tex, hom, hw, soft, min_disp, temp):
  from lsi import _C
  d = _C.LsiSceneDesc()
  d.B, d.V, d.P = hom.shape[:3]
  d.Hs, d.Ws = tex.shape[2:4]
  d.H, d.W = hw
  d.n_box, d.soft, d.min_disp, d.temp = d.P, int(soft), min_disp, temp
  d.outputs = _C.LSI_SCENE_IMG | _C.LSI_SCENE_DISP
  return d


def _render(tex, hom, dmat, hw, soft, min_disp, temp):
  """lsi_render_planes / _bwd on explicit matrices (what layers.render_planes
  calls after plane_homographies)."""
  from lsi.geometry import layers
  return layers._RenderPlanes.apply(tex, hom, dmat,
                                    _desc(tex, hom, hw, soft, min_disp, temp))


def _upstream(seed, keep, which):
  rs = np.random.RandomState(seed)
  k = keep.unsqueeze(-1)
  g_img = torch.tensor(rs.randn(*keep.shape, 3)) * k
  g_disp = torch.tensor(rs.randn(*keep.shape, 1)) * k
  return (g_img if which != 'disp' else None, g_disp if which != 'img' else None)


@pytest.mark.parametrize('soft,min_disp,temp', [(False, 0.2, 0.4), (True, 1e-3, 0.4)])
@pytest.mark.parametrize('hw', [(16, 20), (5, 77)])
@pytest.mark.parametrize('npl', [2, 3, 6, 10])
def test_render_planes_against_the_oracle(dev, npl, hw, soft, min_disp, temp):
  tex, hom, dmat = R.scene(SEED_OF(npl, hw), 2, 2, npl, 12, 20, *hw)
  keep = R.kink_keep(tex, hom, dmat, hw, not soft, min_disp, temp)
  _left_out(keep)
  fn = lambda a, b, c: R.fused_oracle(a, b, c, hw, soft, min_disp, temp)
  xs = [_leaf(x, dev) for x in (tex, hom, dmat)]
  outs = _render(*xs, hw, soft, min_disp, temp)
  for which in ('img', 'disp', 'both'):
    gs = _upstream(21, keep, which)
    want = _grads(fn, (tex, hom, dmat), gs, torch.float64)
    ref = _grads(fn, (tex, hom, dmat), gs, torch.float32)
    pairs = [(o, g.float().to(dev)) for o, g in zip(outs, gs) if g is not None]
    got = torch.autograd.grad([o for o, _ in pairs], xs, [g for _, g in pairs],
                              retain_graph=True)
    for name, gt, wt, rf in zip(('g_tex', 'g_hom', 'g_dmat'), got, want, ref):
      if wt is None or not wt.any():
        # the disparity output reaches the plane disparities only, the hard
        # image the textures and homographies only
        assert (which == 'disp' and name != 'g_dmat') or \
            (which == 'img' and not soft and name == 'g_dmat'), (name, which)
        assert not gt.any(), (name, which)
        continue
      _check('%s <- %s' % (name, which), gt, wt, rf)
      if name == 'g_tex':
        _check('g_masks <- %s' % which, gt[..., 3], wt[..., 3], rf[..., 3]) \
            if wt[..., 3].any() else None


def SEED_OF(npl, hw):
  """Seeds checked on the CPU: the oracle alone leaves out 0.9 - 4.2 %."""
  return 100 + npl + hw[0]


# ---------------------------------------------------------------------------
# 4. the fused route against the op route
# ---------------------------------------------------------------------------
def _op_route(tex, hom, dmat, hw, soft, min_disp, temp):
  """transform_pts -> divide_safe -> bilinear -> trg_disp_maps' product ->
  compose / compose_depth, per world and view (every op differentiable)."""
  from lsi.geometry import homography, layers, sampling
  from lsi.nnutils import helpers
  h, w = hw
  nb, nv, npl = hom.shape[:3]
  pcs = helpers.pixel_coords(1, h, w, device=tex.device)[0][None].expand(npl, h, w, 3)
  imgs, disps = [], []
  for b in range(nb):
    for v in range(nv):
      q = helpers.transform_pts(pcs, hom[b, v].reshape(npl, 3, 3))
      both = sampling.bilinear_wrapper(tex[b], homography.normalize_homogeneous(q))
      prod = dmat[b, v].reshape(npl, 1, 1, 3) * pcs
      dm = (prod[..., 0:1] + prod[..., 1:2]) + prod[..., 2:3]
      imgs.append(layers.compose(both[..., :3], both[..., 3:4], dm, soft=soft,
                                 min_disp=min_disp, depth_softmax_temp=temp, differentiable=True))
      disps.append(layers.compose_depth(both[..., 3:4], dm, bg_layer=False,
                                        min_disp=min_disp, depth_softmax_temp=temp,
                                        differentiable=True))
  return (torch.stack(imgs).reshape(nb, nv, h, w, 3),
          torch.stack(disps).reshape(nb, nv, h, w, 1))


@pytest.mark.parametrize('soft,min_disp,temp', [(False, 0.2, 0.4), (True, 1e-3, 0.4)])
def test_fused_route_equals_the_op_route(dev, soft, min_disp, temp):
  hw = (16, 20)
  tex, hom, dmat = R.scene(SEED_OF(3, hw), 2, 2, 3, 12, 20, *hw)
  keep = R.kink_keep(tex, hom, dmat, hw, not soft, min_disp, temp)
  _left_out(keep)
  gs = _upstream(22, keep, 'both')
  fn = lambda a, b, c: R.fused_oracle(a, b, c, hw, soft, min_disp, temp)
  want = _grads(fn, (tex, hom, dmat), gs, torch.float64)
  ref = _grads(fn, (tex, hom, dmat), gs, torch.float32)
  res = []
  for route in (_render, _op_route):
    xs = [_leaf(x, dev) for x in (tex, hom, dmat)]
    outs = route(*xs, hw, soft, min_disp, temp)
    torch.autograd.backward(outs, [g.float().to(dev) for g in gs])
    res.append((outs, [x.grad for x in xs]))
  assert torch.equal(res[0][0][0], res[1][0][0]) and torch.equal(res[0][0][1], res[1][0][1])
  for name, a, b, wt, rf in zip(('g_tex', 'g_hom', 'g_dmat'), res[0][1], res[1][1],
                                want, ref):
    _check('%s fused vs op route' % name, a, wt, rf, against=b)


# ---------------------------------------------------------------------------
# 5. hostile homographies
# ---------------------------------------------------------------------------
def _hostile():
  rs = np.random.RandomState(17)
  nb, nv, npl, hs, ws, h, w = 2, 2, 6, 24, 40, 32, 64
  tex = rs.rand(nb, npl, hs, ws, 4)
  tex[..., 3] = tex[..., 3] > 0.3
  hom = np.tile(np.array([ws / w, 0, 0, 0, hs / h, 0, 0, 0, 1.0]), (nb, nv, npl, 1))
  hom += 0.05 * rs.randn(*hom.shape) * (hom != 0)
  hom[..., [2, 5]] = 0.3 + 0.2 * rs.rand(nb, nv, npl, 2)
  dmat = np.tile(np.array([0, 0, 0.4]), (nb, nv, npl, 1))
  dmat[..., 2] += 0.1 * rs.rand(nb, nv, npl)
  hom[0, 0, 0, 6:] = [0, 0, -1]                 # behind the camera
  dmat[0, 0, 0] = [0, 0, -0.5]
  hom[0, 0, 1, 6:] = [0, 0, 0]                  # q2 == 0 everywhere
  hom[0, 1, 0, 6:] = [1, 0, -32.5]              # q2 == 0 on the column x = 32.5
  hom[0, 1, 1, :3] = [1e6, 0, 1e9]              # far outside
  hom[1, :, :, :] = 0                           # a world no view sees
  hom[1, :, :, 2] = -1e4
  hom[1, :, :, 8] = 1
  return [torch.tensor(x) for x in (tex, hom, dmat)], (h, w)


def test_hostile_homographies(dev):
  (tex, hom, dmat), hw = _hostile()
  soft, min_disp, temp = True, 0.2, 0.4
  keep = R.kink_keep(tex, hom, dmat, hw, False, min_disp, temp)
  print('left out: %.2f %%' % (100 - 100 * float(keep.double().mean())))
  gs = _upstream(23, keep, 'both')
  fn = lambda a, b, c: R.fused_oracle(a, b, c, hw, soft, min_disp, temp)
  want = _grads(fn, (tex, hom, dmat), gs, torch.float64)
  ref = _grads(fn, (tex, hom, dmat), gs, torch.float32)
  res = []
  for route in (_render, _op_route):
    xs = [_leaf(x, dev) for x in (tex, hom, dmat)]
    outs = route(*xs, hw, soft, min_disp, temp)
    torch.autograd.backward(outs, [g.float().to(dev) for g in gs])
    res.append(xs[0].grad)
  assert bool(torch.isfinite(res[0]).all())
  _check('g_tex fused vs op route', res[0], want[0], ref[0], against=res[1])
  _check('g_tex', res[0], want[0], ref[0])
  # planes the forward samples as 0 everywhere: plane (0, 1) (q2 == 0 in view 0,
  # far outside in view 1) and the whole of world 1
  assert not res[0][0, 1].any() and not res[0][1].any()
  assert res[0][0, 2].any()
  # non-finite entries in two planes: the call succeeds and the other planes'
  # texture gradients are those of a scene where these two are merely unseen
  # (both sample mask 0 and colour 0 at the same disparities)
  bad, unseen = hom.clone(), hom.clone()
  bad[0, 0, 4, 2] = float('nan')
  bad[0, 1, 4, 0] = float('inf')
  bad[0, :, 5, 8] = float('nan')
  unseen[0, :, 4:6] = hom[1, 0, 0]
  got = []
  for hm in (bad, unseen):
    xs = [x.float().to(dev) for x in (tex, hm, dmat)]
    xs[0].requires_grad_(True)
    outs = _render(*xs, hw, soft, min_disp, temp)       # raises unless LSI_OK
    torch.autograd.backward(outs, [g.float().to(dev) for g in gs])
    got.append(xs[0].grad)
  assert not got[0][0, 4:6].any()
  others = [0, 1, 2, 3]
  scale = float(got[1].abs().max())
  diff = float((got[0][0, others] - got[1][0, others]).abs().max())
  print('other planes: max |diff| %.3g of %.3g' % (diff, scale))
  # the same per-pixel products, summed by the atomics in another order
  assert diff <= 1e-6 * scale
  assert torch.equal(got[0][1], got[1][1])


# ---------------------------------------------------------------------------
# 6. reproducibility and contracts
# ---------------------------------------------------------------------------
def test_reproducibility_and_contracts(dev):
  from lsi import _C
  from lsi.geometry import layers
  hw = (5, 77)
  tex, hom, dmat = [x.float().to(dev) for x in R.scene(31, 2, 2, 6, 12, 20, *hw)]
  d = _desc(tex, hom, hw, True, 0.2, 0.4)
  rs = np.random.RandomState(32)
  g_img = torch.tensor(rs.randn(2, 2, *hw, 3), dtype=torch.float32, device=dev)
  g_disp = torch.tensor(rs.randn(2, 2, *hw, 1), dtype=torch.float32, device=dev)
  need = int(_C.lib().lsi_render_planes_bwd_workspace_bytes(ctypes.byref(d)))
  assert need == 2 * 2 * 2 * 6 * 12 * 4
  runs = []
  for fill in (0.0, 1.5):
    g_tex = torch.full_like(tex, fill)
    g_hom = torch.full_like(hom, float('nan'))
    g_dmat = torch.full_like(dmat, float('nan'))
    ws = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=dev)
    rc = _C.lib().lsi_render_planes_bwd(
        ctypes.byref(d), _C.ptr(tex), _C.ptr(hom), _C.ptr(dmat), _C.ptr(g_img),
        _C.ptr(g_disp), _C.ptr(g_tex), _C.ptr(g_hom), _C.ptr(g_dmat), _C.ptr(ws),
        need + 64, _C.stream_ptr(dev))
    assert rc == 0
    assert bool((ws[need:] == 0xAB).all())            # the tail is not touched
    runs.append((g_tex, g_hom, g_dmat))
  assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
  assert bool(torch.isfinite(runs[0][1]).all() and torch.isfinite(runs[0][2]).all())
  # accumulated into what was there
  scale = float(runs[0][0].abs().max())
  assert scale > 0
  assert float((runs[1][0] - 1.5 - runs[0][0]).abs().max()) <= 1e-6 * max(scale, 1.5)
  # outputs that are not asked for: no workspace needed, the others unchanged
  g_tex = torch.zeros_like(tex)
  rc = _C.lib().lsi_render_planes_bwd(
      ctypes.byref(d), _C.ptr(tex), _C.ptr(hom), _C.ptr(dmat), _C.ptr(g_img), None,
      _C.ptr(g_tex), None, None, None, 0, _C.stream_ptr(dev))
  assert rc == 0 and g_tex.any()
  # the room outputs are forward-only
  eye = torch.eye(3, device=dev).expand(1, 1, 2, 3, 3)
  args = [torch.rand(1, 2, 8, 8, 3, device=dev, requires_grad=True),
          torch.rand(1, 2, 8, 8, 1, device=dev), eye, eye, eye,
          torch.zeros(1, 1, 2, 3, 1, device=dev),
          torch.tensor([0., 0., 1.], device=dev).expand(1, 1, 2, 1, 3),
          -torch.ones(1, 1, 2, 1, 1, device=dev), (8, 8)]
  with pytest.raises(RuntimeError, match='forward-only'):
    layers.render_planes(*args, n_box=1)
  assert len(layers.render_planes(*[a.detach() if torch.is_tensor(a) else a
                                    for a in args], n_box=1)) == 4
  img, disp = layers.render_planes(*args)
  img.sum().backward()
  assert args[0].grad is not None and args[0].grad.any()


# ---------------------------------------------------------------------------
# 7. fitting through the renderer
# ---------------------------------------------------------------------------
def _fit_scene(dev):
  n = 32
  yy, xx = torch.meshgrid(torch.linspace(0, 1, n), torch.linspace(0, 1, n), indexing='ij')
  def texture(ph):
    rgb = torch.stack([0.5 + 0.4 * torch.sin(6 * xx + ph), 0.5 + 0.4 * torch.cos(5 * yy - ph),
                       0.5 + 0.4 * torch.sin(4 * (xx + yy) + 2 * ph)], -1)
    r2 = (xx - 0.5) ** 2 + (yy - 0.5) ** 2
    return torch.cat([rgb, torch.sigmoid(40 * (0.12 + 0.05 * ph - r2))[..., None]], -1)
  tex = torch.stack([texture(0.3), texture(1.1)])[None].to(dev)       # 1 x 2 x 32 x 32 x 4
  k = torch.tensor([[n, 0, n / 2.0], [0, n, n / 2.0], [0, 0, 1.0]], device=dev)
  rot = torch.eye(3, device=dev).expand(1, 2, 1, 3, 3)
  t = torch.tensor([[0.0, 0, 0], [0.08, -0.03, 0.02]], device=dev).reshape(1, 2, 1, 3, 1)
  n_hat = torch.tensor([[0.0, 0, 1], [0.1, 0, 1]], device=dev).reshape(1, 1, 2, 1, 3)
  a = torch.tensor([-2.0, -3.0], device=dev).reshape(1, 1, 2, 1, 1)
  return tex, k, rot, t, n_hat, a


def _render_fit(tex, k, rot, t, n_hat, a):
  from lsi.geometry import layers
  kk = k[None, None, None]
  return layers.render_planes(tex, None, kk, kk, rot, t, n_hat, a, (32, 32), soft=True,
                              min_disp=0.1, depth_softmax_temp=0.4)[0]


def _adam(params, loss_fn, lr, project=None):
  opt = torch.optim.Adam(params, lr=lr)
  losses = []
  for _ in range(20):
    opt.zero_grad()
    loss = loss_fn()
    loss.backward()
    opt.step()
    if project is not None:
      project()
    losses.append(float(loss.detach()))
  print('loss: first %.5g, last %.5g' % (losses[0], losses[-1]))
  assert all(np.isfinite(losses))
  assert losses[-1] < losses[0]
  return losses


def test_textures_fit_through_render_planes(dev):
  tex, k, rot, t, n_hat, a = _fit_scene(dev)
  target = _render_fit(tex, k, rot, t, n_hat, a)
  assert not target.requires_grad
  mine = (0.5 * torch.ones_like(tex)).requires_grad_(True)
  # (colours and masks live in [0, 1]: a negative mask has no log-probability)
  losses = _adam([mine], lambda: ((_render_fit(mine, k, rot, t, n_hat, a) - target) ** 2).mean(),
                 0.05, project=lambda: mine.data.clamp_(0, 1))
  assert losses[-1] < 0.5 * losses[0]


def test_planes_fit_through_plane_homographies(dev):
  tex, k, rot, t, n_hat, a = _fit_scene(dev)
  target = _render_fit(tex, k, rot, t, n_hat, a)
  n2 = (n_hat + torch.tensor([0.05, -0.04, 0.0], device=dev)).requires_grad_(True)
  a2 = (a * 1.1).requires_grad_(True)
  _adam([n2, a2], lambda: ((_render_fit(tex, k, rot, t, n2, a2) - target) ** 2).mean(), 2e-3)
  assert n2.grad.any() and a2.grad.any()
