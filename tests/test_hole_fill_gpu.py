"""The push-pull hole filler (csrc/lsi_fill.hip) through lsi.geometry.fill,
against the float32 NumPy restatement tests/hole_fill_ref.py: the comparison is
`np.array_equal` on the bit patterns, no tolerance.  The
torch-op statement of the same definition agrees to 1e-6."""
import numpy as np
import pytest
import torch

import hole_fill_ref as R

pytestmark = pytest.mark.gpu
F = np.float32

# N, H, W, C: one pixel; a row; smaller than a tile; one tile exactly; a tile
# edge plus one (halos, ragged tiles); an even and an odd level-5 map
SHAPES = [(1, 1, 1, 1), (1, 1, 7, 3), (2, 5, 3, 4), (1, 32, 32, 3), (3, 33, 65, 3),
          (2, 64, 96, 4), (1, 96, 160, 1)]
PATTERNS = ('random', 'band', 'isolated', 'one_image')
BG_WT = 1e-6


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def confidence(rs, pattern, n, h, w):
  """N x H x W in [0, 1]: 0 in the holes, fractional and full confidence elsewhere."""
  c = np.where(rs.rand(n, h, w) > 0.5, 1.0, 0.05 + 0.95 * rs.rand(n, h, w)).astype(F)
  if pattern == 'random':
    c[rs.rand(n, h, w) < 0.5] = 0
  elif pattern == 'band':            # 40 columns and 40 rows wide, across tile edges
    c[:, :, max(w // 2 - 20, 0):w // 2 + 20] = 0
    if n > 1:
      c[1:, max(h // 2 - 20, 0):h // 2 + 20, :] = 0
  elif pattern == 'isolated':
    c[:, 0::3, 1::4] = 0
    c[:, h - 1, w - 1] = 0
  else:                              # every pixel of the last image and no other
    c[n - 1] = 0
  return c


_CASES = {}


def case(shape, pattern, mode):
  """(img, w, want): computed once, shared, never written to."""
  key = (shape, pattern, mode)
  if key not in _CASES:
    n, h, w, c = shape
    rs = np.random.RandomState(31 * sum(shape) + 7 * PATTERNS.index(pattern) + mode)
    conf = confidence(rs, pattern, n, h, w)
    img = rs.rand(n, h, w, c).astype(F)
    if mode == R.CONF:
      bad = np.array([np.nan, np.inf, -np.inf, 1e30], F)      # what a hole may hold
      img[conf == 0] = bad[rs.randint(0, 4, (int((conf == 0).sum()), c))]
      wts = conf
      want = R.fill(img, wts, R.CONF, conf_min=0.1, bg_value=0.75)
    else:
      img, wts = R.splat_canvas(img, conf, BG_WT, scale=2.0)
      want = R.fill(img, wts, R.SPLAT, conf_min=1e-3, bg_value=1.0, bg_wt=BG_WT)
    for a in (img, wts, want):
      a.setflags(write=False)
    _CASES[key] = (img, wts, want)
  return _CASES[key]


def run(dev, img, wts, mode, **kw):
  from lsi.geometry import fill
  ti, tw = torch.tensor(img, device=dev), torch.tensor(wts, device=dev)
  if mode == R.CONF:
    return fill.fill_holes(ti, tw, conf_min=0.1, bg_value=0.75, **kw)
  return fill._fill(ti, tw, fill.MODES['splat'], BG_WT, 1.0, 1e-3, **kw)


def assert_bits(got, want, what):
  got = got.cpu().numpy()
  assert got.dtype == F and got.shape == want.shape
  same = got.view(np.uint32) == want.view(np.uint32)
  if not same.all():
    bad = np.argwhere(~same)
    k = tuple(bad[0])
    pytest.fail('%s: %d of %d values differ; first at %s: got %r, want %r' %
                (what, len(bad), same.size, k, got[k], want[k]))


@pytest.mark.parametrize('mode', [R.CONF, R.SPLAT], ids=['conf', 'splat'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bit_exact_against_the_restatement(dev, shape, mode):
  for pattern in PATTERNS:
    img, wts, want = case(shape, pattern, mode)
    assert np.isfinite(want).all()
    assert_bits(run(dev, img, wts, mode), want, '%s %s' % (shape, pattern))


def test_full_confidence_and_no_confidence(dev):
  from lsi.geometry import fill
  rs = np.random.RandomState(11)
  img = torch.tensor(rs.rand(2, 33, 65, 3).astype(F), device=dev)
  assert torch.equal(fill.fill_holes(img, torch.ones(2, 33, 65, device=dev)), img)
  none = fill.fill_holes(img, torch.zeros(2, 33, 65, 1, device=dev), bg_value=0.25)
  assert bool((none == 0.25).all())


def test_out_workspace_and_repeat(dev):
  """`out` and `workspace` are used as given, nothing beyond them is written, a
  repeated call allocates nothing and gives the same bits."""
  from lsi import _C
  from lsi.geometry import fill
  shape = (3, 33, 65, 3)
  img, wts, want = case(shape, 'random', R.CONF)
  need = int(_C.lib().lsi_fill_holes_workspace_bytes(*shape))
  lv = [(-(-33 >> l)) * (-(-65 >> l)) for l in range(1, 6)]
  assert need == 3 * 4 * (4 * sum(lv) + 3 * lv[-1])
  ws = torch.full((64 + need + 64,), 0xAB, dtype=torch.uint8, device=dev)
  buf = torch.full((16 + want.size + 16,), -7.0, device=dev)
  out = buf[16:16 + want.size].view(shape)
  ti, tw = torch.tensor(img, device=dev), torch.tensor(wts, device=dev)
  got = fill.fill_holes(ti, tw, conf_min=0.1, bg_value=0.75, out=out, workspace=ws[64:64 + need])
  assert got is out
  assert_bits(out, want, 'out=')
  assert bool((buf[:16] == -7).all() and (buf[-16:] == -7).all())
  assert bool((ws[:64] == 0xAB).all() and (ws[-64:] == 0xAB).all())
  torch.cuda.synchronize()
  before = torch.cuda.memory_allocated(dev)
  fill.fill_holes(ti, tw, conf_min=0.1, bg_value=0.75, out=out, workspace=ws[64:64 + need])
  assert torch.cuda.memory_allocated(dev) == before
  assert_bits(out, want, 'repeat')
  with pytest.raises(RuntimeError, match='workspace'):
    fill.fill_holes(ti, tw, out=out, workspace=ws[64:64 + need - 4])
  with pytest.raises(RuntimeError, match='not img itself'):
    fill.fill_holes(ti, tw, out=ti)


def test_over_limit_shape_is_refused_without_a_launch(dev):
  """64 x 64 pixels at level 5 do not fit the middle kernel's LDS: the error code
  comes back and `out` keeps its bytes."""
  from lsi import _C
  from lsi.geometry import fill
  lib = _C.lib()
  assert lib.lsi_fill_holes_workspace_bytes(1, 2048, 2048, 1) == 0
  assert lib.lsi_fill_holes_workspace_bytes(1, 1024, 1024, 4) > 0
  img = torch.zeros(1, 2048, 2048, 1, device=dev)
  out = torch.full_like(img, -7.0)
  ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
  rc = lib.lsi_fill_holes(1, 2048, 2048, 1, img.data_ptr(), img.data_ptr(), 0, 0., 1., 1e-3,
                          out.data_ptr(), ws.data_ptr(), ws.numel(), _C.stream_ptr(dev))
  assert rc == -1
  torch.cuda.synchronize()
  assert bool((out == -7).all())
  with pytest.raises(RuntimeError, match='code -1'):
    fill.fill_holes(img, img[..., 0])


@pytest.mark.parametrize('mode', ['conf', 'splat'])
def test_ops_statement_agrees(dev, mode):
  from lsi.geometry import fill
  shape = (3, 33, 65, 3)
  img, wts, want = case(shape, 'random', R.SPLAT if mode == 'splat' else R.CONF)
  ti, tw = torch.tensor(img, device=dev), torch.tensor(wts, device=dev)
  if mode == 'conf':                  # (the holes hold NaN and Inf: selected away here too)
    got = fill.fill_holes(ti, tw, conf_min=0.1, bg_value=0.75)
    ops = fill.fill_holes_ops(ti, tw, conf_min=0.1, bg_value=0.75)
  else:
    got = fill._fill(ti, tw, fill.MODES['splat'], BG_WT, 1.0, 1e-3)
    ops = fill.fill_holes_ops(ti, tw, conf_min=1e-3, bg_value=1.0, mode='splat', bg_wt=BG_WT)
  assert_bits(got, want, 'kernel')
  err = float((got - ops).abs().max())
  print('max |kernel - ops| = %.3g' % err)
  assert err <= 1e-6
  # on the host as well: the op route runs anywhere
  cpu = fill.fill_holes_ops(ti.cpu(), tw.cpu(), **(
      dict(conf_min=0.1, bg_value=0.75) if mode == 'conf' else
      dict(conf_min=1e-3, bg_value=1.0, mode='splat', bg_wt=BG_WT)))
  assert float((got.cpu() - cpu).abs().max()) <= 1e-6


def test_fill_splat_holes_on_a_rendering(dev):
  """forward_splat's composed outputs, magnified so that cracks open: the wrapper
  derives the canvas weight itself, leaves no canvas in the holes and keeps the
  covered pixels."""
  from lsi import _C
  from lsi.geometry import fill, ldi
  rs = np.random.RandomState(12)
  nl, b, h, w = 2, 2, 33, 65
  tex = torch.tensor((0.1 + 0.5 * rs.rand(nl, b, h, w, 3)).astype(F), device=dev)
  disp = torch.tensor((0.05 + 0.3 * rs.rand(nl, b, h, w, 1)).astype(F), device=dev)
  k = np.array([[60., 0, w / 2], [0, 60., h / 2], [0, 0, 1]], F)
  k_t = k.copy()
  k_t[0, 0] = k_t[1, 1] = 150.                                  # magnified 2.5 times
  cams = [torch.tensor(np.stack([x] * b)) for x in
          (k, k_t, np.eye(3, dtype=F), np.array([[0.3], [0.1], [0.]], F))]
  kw = dict(bg_layer_disp=1e-3, max_disp=0.4, zbuf_scale=50.)
  img, wts = ldi.forward_splat([tex, None, disp], None, *cams, compose_layers=True,
                               trg_downsampling=1, **kw)
  filled = fill.fill_splat_holes(img, wts, n_layers=nl, **kw)
  assert tuple(filled.shape) == (1, b, h, w, 3)
  bg_wt = fill.canvas_weight(n_layers=nl, **kw)                 # both layers' canvases
  assert bg_wt == 2 * _C.bg_weight(**kw)
  want = R.fill(img[0].cpu().numpy(), wts[0, ..., 0].cpu().numpy(), R.SPLAT, bg_wt=bg_wt)
  assert_bits(filled[0], want, 'rendering')
  conf = fill.splat_confidence(wts, n_layers=nl, **kw)[0, ..., 0]
  hole = conf == 0
  assert 0.02 < float(hole.float().mean()) < 0.9                # cracks did open
  assert float(img[0][hole].min()) > 0.99                       # ... and show the canvas
  # none of it is left (p0 = img - (1 - c0) cancels to 2 ulp of 1 over c0 >= 1e-3)
  assert float(filled[0][hole].max()) <= 0.6 + 1e-3
  solid = conf > 0.999
  assert float((filled[0] - img[0])[solid].abs().max()) <= 1e-3
