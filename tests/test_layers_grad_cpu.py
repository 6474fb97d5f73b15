"""The gradients of compose, compose_depth and the fused planar renderer,
without a GPU: the closed form of DESIGN section 4.9 (what the kernels
implement) equals the fp64 autograd of the oracle's op graph, and the new
entries refuse bad arguments before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import lsi_torch_ref as TR
import layers_grad_ref as R
from conftest import golden

RTOL = 1e-9   # fp64 round-off of two evaluation orders


def _close(got, want, what):
  scale = float(want.abs().max())
  err = float((got - want).abs().max())
  print('%s: max |diff| %.3g of max |grad| %.3g' % (what, err, scale))
  assert scale > 0, what
  assert err <= RTOL * scale, what


def _layers():
  g = golden('layers.npz')
  return [torch.tensor(g[k], dtype=torch.float64)
          for k in ('p_out_imgs', 'p_out_masks', 'p_out_dmaps')]


@pytest.mark.parametrize('soft,min_disp,temp', [(False, 0.2, 0.4), (False, 1e-6, 1),
                                                (True, 1e-3, 0.4)])
def test_compose_closed_form_is_the_oracles_autograd(soft, min_disp, temp):
  imgs, masks, dmaps = [x.requires_grad_(True) for x in _layers()]
  g = torch.tensor(np.random.RandomState(1).randn(*imgs.shape[1:]))
  out = TR.compose(imgs, masks, dmaps, soft, min_disp, temp)
  want = torch.autograd.grad(out, (imgs, masks, dmaps), g, allow_unused=True)
  got = R.compose_closed(imgs.detach(), masks.detach(), dmaps.detach(), g, soft,
                         min_disp, temp)
  _close(got[0], want[0], 'g_imgs')
  if soft:
    _close(got[1], want[1], 'g_masks')
    _close(got[2], want[2], 'g_dmaps')
  else:     # one_hot(argmax): no path to the masks and disparities
    for gt, wt in zip(got[1:], want[1:]):
      assert not gt.any() and (wt is None or not wt.any())


@pytest.mark.parametrize('bg_layer', [False, True])
def test_compose_depth_closed_form_is_the_oracles_autograd(bg_layer):
  _, masks, dmaps = _layers()
  dmaps = (dmaps - 0.05 * (dmaps < 0.3)).requires_grad_(True)   # some d <= 0
  masks.requires_grad_(True)
  g = torch.tensor(np.random.RandomState(2).randn(*dmaps.shape[1:]))
  out = TR.compose_depth(masks, dmaps, bg_layer, 1e-3, 0.4)
  want = torch.autograd.grad(out, (masks, dmaps), g, allow_unused=True)
  got = R.compose_depth_closed(masks.detach(), dmaps.detach(), g, bg_layer, 1e-3, 0.4)
  assert want[0] is None or not want[0].any()
  _close(got, want[1], 'g_dmaps')


@pytest.mark.parametrize('soft,min_disp,temp', [(False, 0.2, 0.4), (True, 1e-3, 0.4)])
@pytest.mark.parametrize('which', ['img', 'disp', 'both'])
def test_fused_closed_form_is_the_oracles_autograd(soft, min_disp, temp, which):
  hw = (7, 9)
  tex, hom, dmat = R.scene(5, 2, 2, 3, 6, 8, *hw)
  dmat[0, 0, 0, 2] = -0.2                                        # a plane with d <= 0
  tex, hom, dmat = [x.requires_grad_(True) for x in (tex, hom, dmat)]
  rs = np.random.RandomState(3)
  g_img = torch.tensor(rs.randn(2, 2, *hw, 3)) if which != 'disp' else None
  g_disp = torch.tensor(rs.randn(2, 2, *hw, 1)) if which != 'img' else None
  both = R.fused_oracle(tex, hom, dmat, hw, soft, min_disp, temp)
  outs = [o for o, g in zip(both, (g_img, g_disp)) if g is not None]
  want = torch.autograd.grad(outs, (tex, hom, dmat),
                             [g for g in (g_img, g_disp) if g is not None],
                             allow_unused=True)
  got = R.fused_closed(tex.detach(), hom.detach(), dmat.detach(), hw, soft, min_disp,
                       temp, g_img, g_disp)
  for name, gt, wt in zip(('g_tex', 'g_hom', 'g_dmat'), got, want):
    if wt is None or not wt.any():
      assert not gt.any(), name
    else:
      _close(gt, wt, name)
  if which != 'disp':
    assert got[0].any() and got[1].any()
  assert got[2].any() or (which == 'img' and not soft)


def _desc(_C, **kw):
  d = _C.LsiSceneDesc()
  d.B, d.V, d.P, d.Hs, d.Ws, d.H, d.W = 2, 2, 3, 8, 8, 20, 20
  d.n_box, d.soft, d.min_disp, d.temp, d.outputs = 3, 1, 0.2, 0.4, 1 | 2
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def test_render_planes_bwd_argument_errors_before_any_launch(built_lib):
  from lsi import _C
  lib = _C.lib()
  need = lib.lsi_render_planes_bwd_workspace_bytes(ctypes.byref(_desc(_C)))
  # one partial of 12 floats per workgroup (2 per view of 400 pixels) and plane
  assert need == 2 * 2 * 2 * 3 * 12 * 4
  assert lib.lsi_render_planes_bwd_workspace_bytes(None) == 0
  assert lib.lsi_render_planes_bwd_workspace_bytes(ctypes.byref(_desc(_C, P=17))) == 0
  some = 256     # a non-NULL, aligned address that is never read: every call
  # below is refused by the argument checks
  def call(d, tex=some, hom=some, dmat=some, g_img=some, g_disp=some, g_tex=some,
           g_hom=some, g_dmat=some, ws=some, ws_bytes=need):
    return lib.lsi_render_planes_bwd(ctypes.byref(d) if d is not None else None, tex,
                                     hom, dmat, g_img, g_disp, g_tex, g_hom, g_dmat,
                                     ws, ws_bytes, None)
  assert call(None) == -2                                      # LSI_ENULL
  for bad in (dict(P=0), dict(P=17), dict(B=0), dict(V=-1), dict(Hs=0), dict(W=0),
              dict(H=-3), dict(outputs=0), dict(outputs=16), dict(outputs=1 | 4),
              dict(outputs=2 | 8), dict(outputs=15), dict(Hs=8192, Ws=8192)):
    assert call(_desc(_C, **bad)) == -1, bad                   # LSI_EINVAL
  d = _desc(_C)
  assert call(d, tex=None) == -2
  assert call(d, hom=None) == -2
  assert call(d, dmat=None) == -2
  assert call(d, g_img=None, g_disp=None) == -2                # not both
  assert call(d, tex=260) == -1                                # RGBA texel alignment
  assert call(d, ws=None) == -2
  assert call(d, ws_bytes=need - 1) == -3                      # LSI_EWORKSPACE
  assert call(d, g_tex=None, g_dmat=None, ws_bytes=0) == -3    # g_hom alone needs it
  # nothing asked for: no work, no launch
  assert call(d, g_tex=None, g_hom=None, g_dmat=None, ws=None, ws_bytes=0) == 0


def test_compose_bwd_argument_errors_before_any_launch(built_lib):
  from lsi import _C
  lib = _C.lib()
  some = 256
  def comp(L=2, N=8, C=3, imgs=some, masks=some, dmaps=some, temp=0.4, g_out=some,
           g_imgs=some, g_masks=some, g_dmaps=some):
    return lib.lsi_compose_bwd(L, N, C, imgs, masks, dmaps, 1, 0.2, temp, g_out,
                               g_imgs, g_masks, g_dmaps, None)
  for bad in (dict(L=0), dict(N=0), dict(N=-4), dict(C=0), dict(temp=0.0)):
    assert comp(**bad) == -1, bad
  for bad in ('imgs', 'masks', 'dmaps', 'g_out'):
    assert comp(**{bad: None}) == -2, bad
  assert comp(g_imgs=None, g_masks=None, g_dmaps=None) == 0    # nothing asked for
  def depth(L=2, N=8, masks=some, dmaps=some, temp=0.4, g_out=some, g_dmaps=some):
    return lib.lsi_compose_depth_bwd(L, N, masks, dmaps, 1, 0.5, 0.2, temp, g_out,
                                     g_dmaps, None)
  for bad in (dict(L=0), dict(N=0), dict(temp=0.0)):
    assert depth(**bad) == -1, bad
  for bad in ('masks', 'dmaps', 'g_out', 'g_dmaps'):
    assert depth(**{bad: None}) == -2, bad


def test_differentiable_calls_have_no_cpu_path(built_lib):
  from lsi.geometry import layers
  x = torch.rand(2, 4, 4, 3, requires_grad=True)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    layers.compose(x, torch.rand(2, 4, 4, 1), torch.rand(2, 4, 4, 1))
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    layers.compose_depth(torch.rand(2, 4, 4, 1), torch.rand(2, 4, 4, 1, requires_grad=True))
