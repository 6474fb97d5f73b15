"""The fused loss and composition kernels (csrc/lsi_loss.hip) at the shapes,
layouts and values training feeds them, against the fp64 torch restatements of
the reference's op graphs (oracle/lsi_torch_ref.py) run on the device on the
same fp32 values.

tests/test_loss_gpu.py checks the same bars on the golden fixtures (a block or
two per kernel, contiguous tensors).  Here: the 2 B = 8 view pair buffer at
256 x 768 (several passes of every grid-stride loop, 2048 partials in
finish_kernel), the trainer's stride-4 RGBD views, planar and permuted inputs,
block and grid-cap edges, the view-synthesis loss at the training crop and
downsampling, and the edge values of each operation.

Bars: loss scalars 2e-6 relative, gradients 1e-5 of the
largest reference entry, compose 1e-6 absolute, hard selections exact.  Where
the inputs are quantised (dyadic), that is so the kernel's fp32 differences are
exact: a sign or a minimum that decides a gradient is then the same in fp32 and
fp64, and exact zeros and ties come up on their own.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOSS_RTOL = 2e-6        # scalar bar: fp32 per pixel, fp64 partial sums
GRAD_RTOL = 1e-5        # gradient bar, relative to the largest reference entry
COMPOSE_ATOL = 1e-6     # soft compose bar (winning |log p| <= 7 here)
# hard selections: pixels whose two largest fp64 probabilities are within this
# relative gap (32 fp32 ulps of 1) may pick either layer in fp32 ...
HARD_TIE_MARGIN = 32 * 2.0 ** -23
# ... and there are at most this many of them per million pixels
HARD_NEAR_TIES_PER_M = 200

TPB, MAXBLK = 256, 2048          # lsi_loss.hip: threads per block, grid cap
GRID_CAP = TPB * MAXBLK          # 524288 threads: the second pass starts above
PAIR = (8, 256, 768)             # 2 B views x H x W of the trainer's pair buffer
SPLAT = (128, 384)               # the splat at trg_splat_downsampling = 0.5
BDRY = 0.1                       # splat_bdry_ignore: x_min = 38, y_min = 13
MAX_DISP = 0.4                   # KITTI max_disp (ldi_enc_dec.py)
BG_DISP = 1e-3                   # KITTI bg_layer_disp
ZBUF = 50.0                      # zbuf_scale default
MIN_DISP, TEMP = 1e-3, 1.0       # compose: min_disp of the goldens, default temp


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def _TR():
  import lsi_torch_ref as TR
  return TR


def f32(x):
  """A Python float at the value the kernel sees (fp32 argument)."""
  return float(np.float32(x))


def _gen(dev, seed):
  g = torch.Generator(device=dev)
  g.manual_seed(seed)
  return g


def _leaf64(t):
  return t.detach().double().requires_grad_(True)


def _scalar_close(got, want, rtol=LOSS_RTOL, what=''):
  got, want = [float(v.detach()) if torch.is_tensor(v) else float(v)
               for v in (got, want)]
  assert abs(got - want) <= rtol * abs(want), (what, got, want)


def _close(got, want, rtol=GRAD_RTOL, what=''):
  got, want = got.detach().double(), want.detach().double()
  assert got.shape == want.shape, (what, got.shape, want.shape)
  scale = float(want.abs().max()) if want.numel() else 0.0
  err = float((got - want).abs().max()) if want.numel() else 0.0
  assert err <= rtol * scale, (what, err, scale)


def _close_split(got, want, sel, what=''):
  """The gradient bar on the pixels `sel` and on the rest separately (the
  pixels with S ~ 0 carry gradients ~1e8 x the others')."""
  sel = sel.expand_as(want)
  for part, name in ((sel, 'S=0'), (~sel, 'rest')):
    if bool(part.any()):
      _close(got[part], want[part], what='%s[%s]' % (what, name))


# ---------------------------------------------------------------------------
# 1. self-consistency loss: lsi_zbuf_comp_loss_fwd / _bwd
# ---------------------------------------------------------------------------
def _disparities(shape, g, dev, md):
  """[-0.2, 1.2] x max_disp (negative and above-max values included), 5 %
  exactly 0 and 5 % exactly max_disp (x = 1: the clip passes the gradient)."""
  u = torch.rand(shape, generator=g, device=dev)
  d = (u * 1.4 - 0.2) * md
  k = torch.rand(shape, generator=g, device=dev)
  d = torch.where(k < 0.05, torch.zeros_like(d), d)
  return torch.where((k >= 0.05) & (k < 0.10), torch.full_like(d, md), d)


# name, L, B, H, W, layout, masks, target, zbuf_scale, bg_layer_disp
ZBUF_CASES = [
    ('px255', 2, 3, 5, 17, 'rgbd', 'random', 'contig', ZBUF, BG_DISP),
    ('px256', 2, 2, 8, 16, 'rgbd', 'random', 'contig', ZBUF, BG_DISP),
    ('px257', 3, 1, 1, 257, 'planar', 'random', 'chw', ZBUF, BG_DISP),
    ('gridcap', 2, 2, 256, 1024, 'rgbd', 'random', 'contig', ZBUF, BG_DISP),
    ('gridcap+1', 2, 1, 3, 174763, 'rgbd', 'random', 'contig', ZBUF, BG_DISP),
    ('pair_L4_trainer', 4) + PAIR + ('rgbd', 'ones', 'cat', ZBUF, BG_DISP),
    ('pair_L2_trainer', 2) + PAIR + ('rgbd', 'ones', 'cat', ZBUF, BG_DISP),
    ('pair_L1_trainer', 1) + PAIR + ('rgbd', 'ones', 'cat', ZBUF, BG_DISP),
    ('pair_L4_contig_nomask_z10', 4) + PAIR + ('contig', None, 'contig', 10.0,
                                               BG_DISP),
    ('pair_L2_planar_expand_chw', 2) + PAIR + ('planar', 'expand', 'chw', ZBUF,
                                               BG_DISP),
    ('pair_L2_S0_z10', 2) + PAIR + ('contig', 'random', 'contig', 10.0, 0.0),
    ('pair_L4_S0_z50', 4) + PAIR + ('rgbd', 'random', 'chw', ZBUF, 0.0),
]


def _zbuf_inputs(dev, seed, L, B, H, W, layout, mask_kind, trg_kind):
  """The kernel's inputs as the layout makes them: (imgs, masks, mask leaf,
  disps, trg, imgs' gradient getter, disps' gradient getter, the pixels whose
  masks are all 0).  In the RGBD layout imgs and disps are views of one leaf,
  and the getters read their gradients back from it."""
  g = _gen(dev, seed)
  if layout == 'rgbd':     # LdiPredictor: one L x B x H x W x 4 buffer
    base = torch.empty((L, B, H, W, 4), device=dev)
    base[..., 0:3] = torch.rand((L, B, H, W, 3), generator=g, device=dev)
    base[..., 3:4] = _disparities((L, B, H, W, 1), g, dev, MAX_DISP)
    base.requires_grad_(True)
    imgs, disps = base[..., 0:3], base[..., 3:4]
    assert imgs.stride()[3] == 4 and disps.stride()[3] == 4
    g_imgs, g_disps = lambda: base.grad[..., 0:3], lambda: base.grad[..., 3:4]
  elif layout == 'planar':  # conv-output style: channels-first, permuted
    imgs = torch.rand((L, B, 3, H, W), generator=g, device=dev).permute(
        0, 1, 3, 4, 2).requires_grad_(True)
    disps = _disparities((L, B, 1, H, W), g, dev, MAX_DISP).permute(
        0, 1, 3, 4, 2).requires_grad_(True)
    assert not imgs.is_contiguous()
    g_imgs, g_disps = lambda: imgs.grad, lambda: disps.grad
  else:
    imgs = torch.rand((L, B, H, W, 3), generator=g, device=dev).requires_grad_(True)
    disps = _disparities((L, B, H, W, 1), g, dev, MAX_DISP).requires_grad_(True)
    g_imgs, g_disps = lambda: imgs.grad, lambda: disps.grad
  zero_px = torch.zeros((1, B, H, W, 1), dtype=torch.bool, device=dev)
  m_leaf = None
  if mask_kind is None:
    masks = None
  elif mask_kind == 'ones':   # the trainer's torch.ones_like(disp)
    masks = m_leaf = torch.ones((L, B, H, W, 1), device=dev).requires_grad_(True)
  elif mask_kind == 'expand':  # stride 0 along the layers
    m_leaf = torch.rand((1, B, H, W, 1), generator=g, device=dev).requires_grad_(True)
    masks = m_leaf.expand(L, B, H, W, 1)
  else:                       # [0, 1], exact 0s and 1s, 3 % of pixels all 0
    m = torch.rand((L, B, H, W, 1), generator=g, device=dev)
    k = torch.rand((L, B, H, W, 1), generator=g, device=dev)
    m = torch.where(k < 0.1, torch.zeros_like(m), m)
    m = torch.where((k >= 0.1) & (k < 0.2), torch.ones_like(m), m)
    zero_px = torch.rand((1, B, H, W, 1), generator=g, device=dev) < 0.03
    masks = m_leaf = torch.where(zero_px, torch.zeros_like(m), m).requires_grad_(True)
  if trg_kind == 'chw':
    trg = torch.rand((B, 3, H, W), generator=g, device=dev).permute(0, 2, 3, 1)
  elif trg_kind == 'cat':     # torch.cat([imgs_src, imgs_trg])
    half = max(B // 2, 1)
    trg = torch.cat([torch.rand((half, H, W, 3), generator=g, device=dev),
                     torch.rand((B - half, H, W, 3), generator=g, device=dev)])
  else:
    trg = torch.rand((B, H, W, 3), generator=g, device=dev)
  return imgs, masks, m_leaf, disps, trg, g_imgs, g_disps, zero_px


@pytest.mark.parametrize('case', ZBUF_CASES, ids=[c[0] for c in ZBUF_CASES])
def test_zbuffer_loss_forward_and_gradients_match_fp64(case, dev):
  """Scalar and the gradients of imgs, masks and disps.  With bg_layer_disp = 0
  the pixels whose masks are all 0 have S = 0 (divide_safe's 1e-8 path): their
  mask gradients are ~1e8 x the others', so the bar is applied to them and to
  the rest separately."""
  from lsi.loss import loss
  TR = _TR()
  name, L, B, H, W, layout, mask_kind, trg_kind, zs, bg = case
  imgs, masks, m_leaf, disps, trg, g_imgs, g_disps, zero_px = _zbuf_inputs(
      dev, sum(map(ord, name)), L, B, H, W, layout, mask_kind, trg_kind)
  got = loss.zbuffer_composition_loss(imgs, masks, disps, trg, bg_layer_disp=bg,
                                      max_disp=MAX_DISP, zbuf_scale=zs)
  (2.0 * got).backward()

  oi, od = _leaf64(imgs), _leaf64(disps)
  om_leaf = None if m_leaf is None else _leaf64(m_leaf)
  if mask_kind is None:
    om = torch.ones_like(od)
  elif mask_kind == 'expand':
    om = om_leaf.expand(L, B, H, W, 1)
  else:
    om = om_leaf
  want = TR.zbuffer_composition_loss(oi, om, od, trg.double(),
                                     bg_layer_disp=f32(bg),
                                     max_disp=f32(MAX_DISP), zbuf_scale=zs)
  (2.0 * want).backward()
  _scalar_close(got, want, what='loss')
  _close(g_imgs(), oi.grad, what='imgs')
  _close(g_disps(), od.grad, what='disps')
  if m_leaf is not None:
    _close_split(m_leaf.grad, om_leaf.grad, zero_px, what='masks')
  if bg == 0.0 and mask_kind == 'random':
    assert bool(zero_px.any())                 # the S = 0 path was taken
  # the planted x = 1 disparities get the clip's gradient (where it is not
  # negligible: a layer that takes all the weight has el - cost ~ 0)
  at_max = ((disps.detach() == f32(MAX_DISP)) &
            (od.grad.abs() > 1e-3 * od.grad.abs().max()))
  if L > 1 and B * H * W >= GRID_CAP:
    assert bool(at_max.any())
  assert bool((g_disps()[at_max] != 0).all())


# ---------------------------------------------------------------------------
# 2. disparity regularisers: lsi_disp_reg_loss_fwd / _bwd
# ---------------------------------------------------------------------------
def _dyadic(shape, g, dev):
  """k / 4096: every fp32 difference of these is exact."""
  return torch.randint(0, 4096, shape, generator=g, device=dev).float() / 4096


def _disp_view(dev, L, B, H, W, layout, values):
  """(leaf, disp, grad getter): `values` as the stride-4 disparity view of an
  RGBD buffer or as a contiguous tensor."""
  if layout == 'rgbd':
    base = torch.rand((L, B, H, W, 4), device=dev)
    base[..., 3:4] = values
    base.requires_grad_(True)
    d = base[..., 3:4]
    return d, lambda: base.grad[..., 3:4]
  d = values.clone().requires_grad_(True)
  return d, lambda: d.grad


def _regs(d):
  from lsi.geometry import ldi
  from lsi.loss import loss
  return ldi.disp_smoothness_loss(d), loss.decreasing_disp_loss(d)


DISP_CASES = [
    ('pair_L2_rgbd', 2) + PAIR + ('rgbd',),
    ('pair_L4_rgbd', 4) + PAIR + ('rgbd',),
    ('pair_L4_contig', 4) + PAIR + ('contig',),
    ('pair_L1_rgbd', 1) + PAIR + ('rgbd',),
    ('ragged_rgbd', 3, 2, 37, 53, 'rgbd'),
    ('ragged_contig', 3, 2, 37, 53, 'contig'),
]


@pytest.mark.parametrize('case', DISP_CASES, ids=[c[0] for c in DISP_CASES])
def test_disparity_regularisers_match_fp64(case, dev):
  """Both scalars and the disparity gradient.  Every fourth row of layer l + 1
  repeats layer l (relu'(0) = 0 of the decreasing loss); the dyadic values give
  exact-zero second differences by themselves (abs'(0) = 0)."""
  from lsi.loss import _hip
  TR = _TR()
  name, L, B, H, W, layout = case
  g = _gen(dev, 11 + len(name))
  v = _dyadic((L, B, H, W, 1), g, dev)
  for l in range(1, L):
    v[l, :, ::4] = v[l - 1, :, ::4]
  d, gd = _disp_view(dev, L, B, H, W, layout, v)
  smooth, decr = _regs(d)
  if L == 1:
    assert decr == 0                                   # loss.py:58
    assert float(_hip.disp_regularisers(d)[1].detach()) == 0.0  # kernel
  (0.7 * smooth + 1.3 * decr).backward()
  o = _leaf64(d)
  w_smooth, w_decr = TR.disp_smoothness_loss(o), TR.decreasing_disp_loss(o)
  (0.7 * w_smooth + 1.3 * w_decr).backward()
  _scalar_close(smooth, w_smooth, what='smoothness')
  if L > 1:
    _scalar_close(decr, w_decr, what='decreasing')
  _close(gd(), o.grad, what='disp')


def test_disparity_regularisers_on_piecewise_linear_fields(dev):
  """Full-size sawtooth ramps (period 64 along x, linear along y), layers 0
  and 1 equal, layer 2 farther.  The second differences are exactly 0 except
  across the kinks and every increase is exactly 0, so (TF: abs'(0) =
  relu'(0) = 0) the gradient is exactly 0 at columns 2-61 of each period,
  and matches the oracle at the kinks.  A pure ramp gives exact zeros."""
  TR = _TR()
  L, (B, H, W) = 3, PAIR
  y = torch.arange(H, device=dev, dtype=torch.float32).view(1, 1, H, 1, 1)
  x = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, 1, W, 1)
  for period in (64, W):
    ramp = ((x % period) * 2.0 ** -11 + y * 2.0 ** -10).expand(1, B, H, W, 1)
    v = torch.cat([ramp, ramp, ramp - 0.25])
    for layout in ('rgbd', 'contig'):
      d, gd = _disp_view(dev, L, B, H, W, layout, v)
      smooth, decr = _regs(d)
      assert float(decr.detach()) == 0.0, layout
      (smooth + decr).backward()
      far = ((x % 64) >= 2) & ((x % 64) < 62)
      assert float(gd().masked_select(far).abs().max()) == 0.0, layout
      if period == W:
        assert float(smooth.detach()) == 0.0, layout
        assert float(gd().abs().max()) == 0.0, layout
      else:
        o = _leaf64(d)
        (TR.disp_smoothness_loss(o) + TR.decreasing_disp_loss(o)).backward()
        _scalar_close(smooth, TR.disp_smoothness_loss(o), what=layout)
        _close(gd(), o.grad, what=layout)


@pytest.mark.parametrize('hw', [(3, 3), (3, 4), (4, 3), (4, 4)])
def test_disparity_regularisers_tiny_images(hw, dev):
  """At H, W in {3, 4} every term of the smoothness loss exists."""
  TR = _TR()
  H, W = hw
  v = _dyadic((3, 2, H, W, 1), _gen(dev, H * 10 + W), dev)
  d, gd = _disp_view(dev, 3, 2, H, W, 'rgbd', v)
  smooth, decr = _regs(d)
  (smooth + 2.0 * decr).backward()
  o = _leaf64(d)
  w_smooth, w_decr = TR.disp_smoothness_loss(o), TR.decreasing_disp_loss(o)
  (w_smooth + 2.0 * w_decr).backward()
  _scalar_close(smooth, w_smooth, what='smoothness')
  _scalar_close(decr, w_decr, what='decreasing')
  _close(gd(), o.grad, what='disp')


@pytest.mark.parametrize('hw', [(1, 1), (1, 5), (2, 5), (5, 1), (5, 2), (2, 2)])
def test_disparity_smoothness_drops_empty_terms(hw, dev):
  """H or W < 3: the reference's reduce_mean of an empty second difference is
  NaN; the kernel counts that term as 0 and takes no gradient from it
  (DESIGN 4.5).  No trainer shape gets there."""
  TR = _TR()
  H, W = hw
  v = _dyadic((2, 2, H, W, 1), _gen(dev, H * 10 + W), dev)
  d, gd = _disp_view(dev, 2, 2, H, W, 'contig', v)
  smooth, decr = _regs(d)
  (smooth + decr).backward()
  o = _leaf64(d)
  assert bool(torch.isnan(TR.disp_smoothness_loss(o.detach())))
  dx, dy = TR.gradient(o)
  terms = [t.abs().mean() for t in TR.gradient(dx) + TR.gradient(dy) if t.numel()]
  w_smooth = sum(terms) if terms else o.sum() * 0.0
  w_decr = TR.decreasing_disp_loss(o)
  (w_smooth + w_decr).backward()
  assert bool(torch.isfinite(smooth))
  if terms:
    _scalar_close(smooth, w_smooth, what='smoothness')
  else:
    assert float(smooth.detach()) == 0.0
  _scalar_close(decr, w_decr, what='decreasing')
  _close(gd(), o.grad, what='disp')


# ---------------------------------------------------------------------------
# 3. view-synthesis loss: lsi_view_synth_loss_fwd / _bwd
# ---------------------------------------------------------------------------
def _vs_inputs(dev, seed, nl, B, Ht, Wt, fy, fx, pad=1):
  """Dyadic recons (k / 1024) and target (k / 256): the AREA box means of
  power-of-two factors and every |recons - target| are exact in fp32, so the
  layer minimum is the same in fp32 and fp64 and ties are real ties.  With
  pad > 1 the target is the top-left crop of a pad x larger buffer."""
  g = _gen(dev, seed)
  recons = torch.randint(0, 1024, (nl, B, Ht, Wt, 3), generator=g,
                         device=dev).float() / 1024
  big = torch.randint(0, 256, (B, Ht * fy * pad, Wt * fx * pad, 3), generator=g,
                      device=dev).float() / 256
  return recons, big[:, :Ht * fy, :Wt * fx]


def _assert_zero_outside(gr, y_min, x_min):
  """The cropped border rows and columns get exactly no gradient."""
  _, _, ht, wt, _ = gr.shape
  out = gr.detach().clone()
  out[:, :, y_min:ht - y_min, x_min:wt - x_min] = 0
  assert float(out.abs().max()) == 0.0


def _vs_check(recons_leaf, recons, target, bdry):
  """Scalar and recons gradient against the fp64 oracle with TF's even split
  of the gradient among tied layers; returns the kernel's gradient."""
  from lsi.loss import loss
  TR = _TR()
  got = loss.view_synthesis_loss(recons, target, bdry)
  (3.0 * got).backward()
  o = _leaf64(recons_leaf)
  ov = o if o.shape == recons.shape else o.permute(0, 1, 3, 4, 2)
  want = TR.view_synthesis_loss_even_ties(ov, target.double(), bdry)
  (3.0 * want).backward()
  _scalar_close(got, want, what='loss')
  gr = recons_leaf.grad
  _close(gr, o.grad, what='recons')
  return got, gr


@pytest.mark.parametrize('nl', [1, 2, 4])
def test_view_synthesis_loss_at_the_training_shape(nl, dev):
  """nl x 8 x 128 x 384 against 8 x 256 x 768, bdry 0.1 (x_min 38, y_min 13):
  nl = 1 the composed splat, 2 and 4 the per-layer one."""
  B, (Ht, Wt) = PAIR[0], SPLAT
  recons, target = _vs_inputs(dev, nl, nl, B, Ht, Wt, 2, 2)
  recons.requires_grad_(True)
  _, gr = _vs_check(recons, recons, target, BDRY)
  x_min, y_min = 38, 13
  inner = gr[:, :, y_min:Ht - y_min, x_min:Wt - x_min]
  _assert_zero_outside(gr, y_min, x_min)
  assert bool((inner[:, :, 0] != 0).any()) and bool((inner[:, :, :, 0] != 0).any())


# name, nl, B, Ht, Wt, fy, fx, bdry
VS_FACTOR_CASES = [
    ('fy2_fx4', 2, 2, 48, 40, 2, 4, BDRY),
    ('fy4_fx2', 3, 2, 40, 48, 4, 2, BDRY),
    ('factor1', 2, 2, 64, 80, 1, 1, BDRY),
    ('quarter', 2, 2, 64, 192, 4, 4, BDRY),
    ('crop0', 2, 3, 32, 48, 2, 2, 0.0),
]


@pytest.mark.parametrize('case', VS_FACTOR_CASES, ids=[c[0] for c in VS_FACTOR_CASES])
def test_view_synthesis_loss_area_factors(case, dev):
  """AREA factors fy != fx, 1 and 4 (trg_splat_downsampling 0.25), crop 0.  The
  target is a crop of a 4 x larger buffer (strided rows, and a factor taken
  along the wrong axis reads real, wrong pixels)."""
  name, nl, B, Ht, Wt, fy, fx, bdry = case
  recons, target = _vs_inputs(dev, len(name), nl, B, Ht, Wt, fy, fx, pad=4)
  assert not target.is_contiguous()
  recons.requires_grad_(True)
  _vs_check(recons, recons, target, bdry)


def test_view_synthesis_loss_noncontiguous_recons(dev):
  """A planar (permuted) recons: the wrapper's .contiguous() and the layout of
  the gradient it hands back."""
  nl, B, Ht, Wt = 2, 2, 64, 96
  g = _gen(dev, 5)
  leaf = (torch.randint(0, 1024, (nl, B, 3, Ht, Wt), generator=g, device=dev)
          .float() / 1024).requires_grad_(True)
  recons = leaf.permute(0, 1, 3, 4, 2)
  assert not recons.is_contiguous()
  target = torch.randint(0, 256, (B, 2 * Ht, 2 * Wt, 3), generator=g,
                         device=dev).float() / 256
  _vs_check(leaf, recons, target, BDRY)


def test_view_synthesis_loss_crop_rounds_half_up(dev):
  """Wt * bdry = 2.5 and Ht * bdry = 4.5: Python 2's round (the reference)
  gives 3 and 5, Python 3's gives 2 and 4.  The crop is checked against those
  hand-worked bounds, not the oracle's py2_round."""
  from lsi.loss import loss
  nl, B, Ht, Wt, bdry = 2, 2, 36, 20, 0.125
  x_min, y_min = 3, 5
  assert (round(Wt * bdry), round(Ht * bdry)) == (2, 4)
  recons, target = _vs_inputs(dev, 7, nl, B, Ht, Wt, 2, 2)
  recons.requires_grad_(True)
  got = loss.view_synthesis_loss(recons, target, bdry)
  got.backward()
  r = recons.detach().double()
  tgt = target.double().reshape(B, Ht, 2, Wt, 2, 3).mean(dim=(2, 4))
  pw = (tgt.unsqueeze(0) - r).abs().mean(dim=4).min(dim=0)[0]
  want = pw[:, y_min:Ht - y_min, x_min:Wt - x_min].mean()
  _scalar_close(got, want, what='loss')
  gr = recons.grad
  inner = gr[:, :, y_min:Ht - y_min, x_min:Wt - x_min]
  _assert_zero_outside(gr, y_min, x_min)
  for edge in (inner[:, :, 0], inner[:, :, -1], inner[:, :, :, 0], inner[:, :, :, -1]):
    assert bool((edge != 0).any())


def test_view_synthesis_loss_rejects_bad_crops_and_factors(dev):
  from lsi.loss import loss
  r = torch.rand((1, 1, 4, 4, 3), device=dev)
  with pytest.raises(RuntimeError):        # x_min = y_min = 2: no pixel left
    float(loss.view_synthesis_loss(r, torch.rand((1, 8, 8, 3), device=dev), 0.5))
  with pytest.raises(RuntimeError):        # 6 x 8 onto 4 x 4: factor 1.5 in y
    float(loss.view_synthesis_loss(r, torch.rand((1, 6, 8, 3), device=dev), 0.0))
  with pytest.raises(RuntimeError):        # 8 x 10 onto 4 x 4: factor 2.5 in x
    float(loss.view_synthesis_loss(r, torch.rand((1, 8, 10, 3), device=dev), 0.0))


def test_view_synthesis_loss_ties_at_the_training_shape(dev):
  """Exact ties of 2, 3 and 4 of 4 layers planted in known pixels of a full
  input: TF splits the gradient evenly, so each tied layer gets g / k.  Checked
  against the even-split oracle everywhere, and, as in test_loss_gpu.py,
  against torch.min's oracle by the tied groups' sum and their equal split.
  Ties planted in the crop get exactly zero gradient."""
  from lsi.loss import loss
  TR = _TR()
  nl, B, (Ht, Wt) = 4, PAIR[0], SPLAT
  recons, target = _vs_inputs(dev, 3, nl, B, Ht, Wt, 2, 2)
  tgt = target.reshape(B, Ht, 2, Wt, 2, 3).mean(dim=(2, 4))   # exact
  rows, cols = slice(40, 48), slice(100, 200)
  near = tgt.clone()
  near[..., 0] += 2.0 ** -10                      # l1 = 2^-10 / 3: the minimum
  far = tgt + 0.5
  groups = [(0, (0, 1)), (1, (1, 2, 3)), (2, (0, 1, 2, 3))]
  for b, layers in groups:
    for l in range(nl):
      src = near if l in layers else far
      recons[l, b, rows, cols] = src[b, rows, cols]
  recons[:, 3, 0:8] = near[3, 0:8]                # a 4-way tie in the crop
  recons.requires_grad_(True)
  got, gr = _vs_check(recons, recons, target, BDRY)
  gr = gr.detach().double()
  o = _leaf64(recons)
  (3.0 * TR.view_synthesis_loss(o, target.double(), BDRY)).backward()
  for b, layers in groups:
    k = len(layers)
    mine = gr[list(layers), b, rows, cols]
    theirs = o.grad[list(layers), b, rows, cols]
    _close(mine.sum(0), theirs.sum(0), what='tie group of %d' % k)
    assert bool((mine[0] != 0).any())
    for i in range(1, k):
      assert torch.equal(mine[i], mine[0]), (k, i)
    _close(mine[0] * k, theirs.sum(0), what='even split of %d' % k)
  _assert_zero_outside(gr, 13, 38)


# ---------------------------------------------------------------------------
# 4. compose / compose_depth: lsi_compose_fwd, lsi_compose_depth_fwd
# ---------------------------------------------------------------------------
COMPOSE_SHAPE = (3, 4, 256, 768)   # L, B, H, W: N = 786432 > GRID_CAP


def _compose_inputs(dev, seed, C):
  """Layer 0 in front everywhere (mask >= 0.05, disparity >= 0.25) so that the
  winning log-probabilities stay small; the other layers with negative (relu)
  and zero disparities and zero masks.  Planted: all-zero disparities (the
  1e-8 path: the background layer wins) in batch 0, rows 0-7; layer 1 a
  duplicate of layer 0's mask and disparity (an exact tie; the layers behind
  them get negative disparities) in batch 1, rows 0-15."""
  L, B, H, W = COMPOSE_SHAPE
  g = _gen(dev, seed)
  imgs = torch.rand((L, B, H, W, C), generator=g, device=dev)
  masks = 0.05 + 0.95 * torch.rand((L, B, H, W, 1), generator=g, device=dev)
  k = torch.rand((L, B, H, W, 1), generator=g, device=dev)
  masks = torch.where(k < 0.1, torch.ones_like(masks), masks)
  masks[1:] = torch.where(k[1:] > 0.85, torch.zeros_like(masks[1:]), masks[1:])
  dmaps = 0.25 + 0.75 * torch.rand((L, B, H, W, 1), generator=g, device=dev)
  u = torch.rand((L, B, H, W, 1), generator=g, device=dev)
  dmaps[1:] = torch.where(u[1:] < 0.15, -0.2 * u[1:], dmaps[1:])
  dmaps[1:] = torch.where((u[1:] >= 0.15) & (u[1:] < 0.2),
                          torch.zeros_like(u[1:]), dmaps[1:])
  dmaps[:, 0, 0:8] = 0.0
  masks[1, 1, 0:16], dmaps[1, 1, 0:16] = masks[0, 1, 0:16], dmaps[0, 1, 0:16]
  dmaps[2:, 1, 0:16] = -0.1
  return imgs, masks, dmaps


def _selection_probs(masks, dmaps, depth, bg_layer, min_disp, temp):
  """fp64 soft_z_buffering probabilities of compose / compose_depth's
  selection (layers.py:29-115), background layer last."""
  TR = _TR()
  nl = masks.shape[0]
  dmaps = torch.relu(dmaps)
  bg = torch.ones_like(dmaps[:1]) * min_disp
  masks = torch.cat([masks, torch.ones_like(masks[:1])])
  dmaps = torch.cat([dmaps, bg])
  if depth and bg_layer:
    dmaps = torch.cat([torch.max(dmaps) - dmaps[0:nl], bg])
  return TR.soft_z_buffering(masks, dmaps, temp)


def _check_hard(got, want, probs):
  """Exact equality except where the fp64 oracle's two largest probabilities
  are within HARD_TIE_MARGIN (but not equal: exact ties must pick the first);
  those pixels are counted and bounded."""
  top = probs.topk(2, dim=0).values
  gap = (top[0] - top[1]) / top[0]
  near = (gap > 0) & (gap <= HARD_TIE_MARGIN)
  n = near.numel()
  assert int(near.sum()) <= HARD_NEAR_TIES_PER_M * n / 1e6, int(near.sum())
  want = want.float()
  keep = ~near.expand_as(want)
  assert torch.equal(got[keep], want[keep]), int((got[keep] != want[keep]).sum())


@pytest.mark.parametrize('soft', [False, True], ids=['hard', 'soft'])
@pytest.mark.parametrize('C', [1, 3, 4])
def test_compose_beyond_the_grid_cap(C, soft, dev):
  from lsi.geometry import layers
  TR = _TR()
  imgs, masks, dmaps = _compose_inputs(dev, 20 + C, C)
  got = layers.compose(imgs, masks, dmaps, soft=soft, min_disp=MIN_DISP,
                       depth_softmax_temp=TEMP)
  m64, d64 = masks.double(), dmaps.double()
  want = TR.compose(imgs.double(), m64, d64, soft=soft, min_disp=f32(MIN_DISP),
                    depth_softmax_temp=f32(TEMP))
  # the planted pixels: the background (white) wins where every disparity is 0
  assert bool((want[0, 0:8] == 1.0).all())
  if soft:
    err = float((got.double() - want).abs().max())
    assert err <= COMPOSE_ATOL, err
  else:
    _check_hard(got, want, _selection_probs(m64, d64, False, False,
                                            f32(MIN_DISP), f32(TEMP)))
    # the duplicate pair: the first layer wins the exact tie
    dup = (slice(1, 2), slice(0, 16))
    assert torch.equal(got[dup], imgs[0][dup])


@pytest.mark.parametrize('bg_layer', [False, True], ids=['no_bg', 'bg'])
def test_compose_depth_beyond_the_grid_cap(bg_layer, dev):
  from lsi.geometry import layers
  TR = _TR()
  _, masks, dmaps = _compose_inputs(dev, 30 + bg_layer, 1)
  got = layers.compose_depth(masks, dmaps, bg_layer=bg_layer, min_disp=MIN_DISP,
                             depth_softmax_temp=TEMP)
  m64, d64 = masks.double(), dmaps.double()
  want = TR.compose_depth(m64, d64, bg_layer=bg_layer, min_disp=f32(MIN_DISP),
                          depth_softmax_temp=f32(TEMP))
  _check_hard(got, want, _selection_probs(m64, d64, True, bg_layer,
                                          f32(MIN_DISP), f32(TEMP)))
  if not bg_layer:
    assert bool((got[0, 0:8] == f32(MIN_DISP)).all())   # background wins
    assert torch.equal(got[1, 0:16], dmaps[0, 1, 0:16])  # first of the tie


# ---------------------------------------------------------------------------
# 5. reproducibility at the pair shape
# ---------------------------------------------------------------------------
def test_loss_reductions_are_bitwise_reproducible(dev):
  """Fixed reduction order, fp64 partials (lsi_loss.hip header): three
  forward calls, one of them on a side stream, give the same bits; two
  backward calls give the same gradients."""
  from lsi.loss import loss
  L, (B, H, W) = 4, PAIR
  imgs, masks, _, disps, trg, _, _, _ = _zbuf_inputs(dev, 1, L, B, H, W, 'rgbd',
                                                     'random', 'contig')
  recons, target = _vs_inputs(dev, 2, L, B, SPLAT[0], SPLAT[1], 2, 2)
  recons.requires_grad_(True)
  fns = {
      'zbuf': (lambda: loss.zbuffer_composition_loss(
          imgs, masks, disps, trg, bg_layer_disp=BG_DISP, max_disp=MAX_DISP,
          zbuf_scale=ZBUF), (imgs, masks, disps)),
      'regs': (lambda: torch.stack(_regs(disps)), (disps,)),
      'vs': (lambda: loss.view_synthesis_loss(recons, target, BDRY), (recons,)),
  }
  side = torch.cuda.Stream(device=dev)
  for name, (fn, inputs) in fns.items():
    a, b = fn(), fn()
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      c = fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    assert torch.equal(a, b) and torch.equal(a, c), name
    w = torch.ones_like(a)
    g1 = torch.autograd.grad(a, inputs, w)
    g2 = torch.autograd.grad(b, inputs, w)
    for x, y in zip(g1, g2):
      assert torch.equal(x, y), name
