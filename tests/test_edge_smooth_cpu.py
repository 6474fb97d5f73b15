"""The edge-aware disparity smoothness loss, the parts that need
no GPU: the restatement of tests/edge_smooth_ref.py against examples worked by
hand and against gradcheck, header / binding / exports agree, the entries refuse
bad arguments before any launch, the workspace follows its formula, and the
Python surface exists (no CPU path, five trainer flags).

The hand examples: order 1 on a 2 x 3 plane; order 2 on a 3 x 3 plane, the
smallest it accepts (H, W >= order + 1).  alpha = ln 2 and a guide whose mean
absolute differences are (half-)integers make every weight a power of 2."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

from conftest import PKG, ROOT

import edge_smooth_ref as ref

NEW = ('lsi_edge_smooth_workspace_bytes', 'lsi_edge_smooth_loss_fwd',
       'lsi_edge_smooth_loss_bwd')
EINVAL, ENULL, EWORKSPACE = -1, -2, -3     # include/lsi_hip.h
LN2 = math.log(2.0)
R = 2.0 ** -0.5


def _plane(d, g):
  """disp 1 x 1 x H x W x 1 and guide 1 x H x W x 3 (fp64) from nested lists; the
  guide's channels are g x (1/2, 1, 3/2): mean_c |dG| = |dg|."""
  d = torch.tensor(d, dtype=torch.float64)[None, None, :, :, None]
  g = torch.tensor(g, dtype=torch.float64)[None, :, :, None] * torch.tensor(
      [0.5, 1.0, 1.5], dtype=torch.float64)
  return d, g


def test_order_1_by_hand():
  d, g = _plane([[1, 2, 4], [3, 3, 8]], [[0, 1, 1], [2, 1, 4]])
  # sx = [-1 -2; 0 -5], ex = [1 0; 1 3]: A = 1/2 + 2 + 0 + 5/8
  # sy = [-2 -1 -4],    ey = [2 0 3]:    B = 2/4 + 1 + 4/8
  a, b, s = ref.plane_sums(d, g, LN2, 1)
  assert abs(float(a) - 3.125) <= 1e-14 and abs(float(b) - 2.0) <= 1e-14
  assert float(s) == 21.0
  want = 3.125 / 4 + 2.0 / 3            # H (W - 1) = 4, (H - 1) W = 3
  l, grad = ref.loss_and_grad(d, g, LN2, 1, False)
  assert abs(float(l) - want) <= 1e-14
  # d[0,0]: +sign(sx[0,0]) wx / 4 + sign(sy[0,0]) wy / 3
  assert abs(float(grad[0, 0, 0, 0, 0]) - (-0.5 / 4 - 0.25 / 3)) <= 1e-14
  # d[1,1]: +sign(sx[1,1]) / 8 / 4, -sign(sx[1,0]) = 0, -sign(sy[0,1]) 1 / 3
  assert abs(float(grad[0, 0, 1, 1, 0]) - (-0.125 / 4 + 1.0 / 3)) <= 1e-14
  k = 1.0 / (21.0 / 6 + 1e-7)
  l, grad_n = ref.loss_and_grad(d, g, LN2, 1, True)
  assert abs(float(l) - k * want) <= 1e-14
  # the quotient rule: k grad - k^2 / N * want, everywhere
  assert float((grad_n - (k * grad - k * k / 6 * want)).abs().max()) <= 1e-14


def test_order_2_by_hand():
  d, g = _plane([[1, 2, 4], [3, 3, 8], [6, 4, 9]], [[0, 1, 1], [2, 1, 4], [2, 3, 0]])
  # sx = [1; 5; 7], ex = [1/2; 1; 1]:  A = 2^-1/2 + 5/2 + 7/2
  # sy = [1 0 -3],  ey = [1 1 1/2]:    B = 1/2 + 0 + 3 2^-1/2
  a, b, s = ref.plane_sums(d, g, LN2, 2)
  assert abs(float(a) - (R + 6.0)) <= 1e-14 and abs(float(b) - (0.5 + 3 * R)) <= 1e-14
  assert float(s) == 40.0
  want = (R + 6.0) / 3 + (0.5 + 3 * R) / 3
  l, grad = ref.loss_and_grad(d, g, LN2, 2, False)
  assert abs(float(l) - want) <= 1e-14
  # the centre: -2 sign(sx[1,1]) / 2 / 3 - 2 sign(sy[1,1]) = 0
  assert abs(float(grad[0, 0, 1, 1, 0]) - (-2 * 0.5 / 3)) <= 1e-14
  # d[2,2]: +sign(sx[2,1]) / 2 / 3 + sign(sy[1,2]) 2^-1/2 / 3
  assert abs(float(grad[0, 0, 2, 2, 0]) - (0.5 / 3 - R / 3)) <= 1e-14
  k = 1.0 / (40.0 / 9 + 1e-7)
  assert abs(float(ref.loss(d, g, LN2, 2, True)) - k * want) <= 1e-14


def test_per_layer_guide_and_plane_mean():
  """Two layers with their own guides are the mean of the two planes' terms."""
  d0, g0 = _plane([[1, 2, 4], [3, 3, 8]], [[0, 1, 1], [2, 1, 4]])
  d1, g1 = _plane([[2, 2, 1], [5, 1, 1]], [[1, 1, 0], [0, 2, 2]])
  d, g = torch.cat([d0, d1], 0), torch.stack([g0, g1], 0)
  for norm in (False, True):
    want = 0.5 * (ref.loss(d0, g0, LN2, 1, norm) + ref.loss(d1, g1, LN2, 1, norm))
    assert abs(float(ref.loss(d, g, LN2, 1, norm) - want)) <= 1e-14


@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('normalise', [False, True])
def test_gradcheck_of_the_restatement(order, normalise):
  gen = torch.Generator().manual_seed(5)
  # distinct multiples of 1/64 plus a sub-grid offset: no stencil is near zero
  d = (torch.randperm(2 * 2 * 5 * 6, generator=gen).double().reshape(2, 2, 5, 6, 1)
       + 13.0) / 64.0
  d = d + 1e-3 * torch.rand(d.shape, dtype=torch.float64, generator=gen)
  g = torch.rand((2, 2, 5, 6, 3), dtype=torch.float64, generator=gen)
  smallest, zeros = ref.min_nonzero_stencil(d, g, order)
  assert smallest > 1e-4 and zeros == 0.0
  d.requires_grad_(True)
  assert torch.autograd.gradcheck(
      lambda t: ref.loss(t, g, 3.0, order, normalise), (d,), eps=1e-6, atol=1e-7)


def _desc(_C, **kw):
  d = _C.LsiEdgeSmoothDesc()
  d.L, d.B, d.H, d.W, d.order, d.normalise = 2, 3, 16, 24, 1, 1
  d.d_sl, d.d_sb, d.d_sy, d.d_sx = 3 * 16 * 24, 16 * 24, 24, 1
  d.g_sl, d.g_sb, d.g_sy, d.g_sx, d.g_sc = 0, 16 * 24 * 3, 24 * 3, 3, 1
  d.alpha, d.eps = 10.0, 1e-7
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def test_header_binding_and_exports_agree(built_lib):
  from lsi import _C
  with open(os.path.join(ROOT, 'include', 'lsi_hip.h')) as f:
    h = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
  assert re.search(r'#define LSI_VERSION 100\b', h)
  handle = ctypes.CDLL(built_lib)
  n_params = {}
  for n in NEW:
    m = re.search(r'(?:int|size_t)\s+%s\s*\(([^)]*)\)\s*;' % n, h)
    assert m, n
    n_params[n] = len(m.group(1).split(','))
    assert n in _C.SIGNATURES, n
    res, args = _C.SIGNATURES[n]
    assert len(args) == n_params[n], n
    assert res is (ctypes.c_size_t if n.endswith('_bytes') else ctypes.c_int)
    assert hasattr(handle, n), n
  assert n_params == {'lsi_edge_smooth_workspace_bytes': 1,
                      'lsi_edge_smooth_loss_fwd': 8, 'lsi_edge_smooth_loss_bwd': 7}
  # the struct: 6 int32, 9 int64, 2 float -- no padding
  m = re.search(r'typedef struct LsiEdgeSmoothDesc \{(.*?)\} LsiEdgeSmoothDesc;', h,
                flags=re.S)
  fields = re.findall(r'\b([A-Za-z_0-9]+)\s*[,;]', m.group(1))
  assert fields == [f[0] for f in _C.LsiEdgeSmoothDesc._fields_]
  assert fields == ['L', 'B', 'H', 'W', 'order', 'normalise', 'd_sl', 'd_sb', 'd_sy',
                    'd_sx', 'g_sl', 'g_sb', 'g_sy', 'g_sx', 'g_sc', 'alpha', 'eps']
  assert ctypes.sizeof(_C.LsiEdgeSmoothDesc) == 6 * 4 + 9 * 8 + 2 * 4
  assert _C.LsiEdgeSmoothDesc.d_sl.offset == 24
  assert _C.LsiEdgeSmoothDesc.g_sl.offset == 56
  assert _C.LsiEdgeSmoothDesc.alpha.offset == 96


def test_argument_errors_are_reported_before_any_launch(built_lib):
  from lsi import _C
  lib = _C.lib()
  big = 1 << 30
  p = ctypes.c_void_p(16)     # never dereferenced: every call below is refused

  def calls(d, a=p, b=p, c=p, e=p, ws=p, nbytes=big):
    r = ctypes.byref(d) if d is not None else None
    return (lib.lsi_edge_smooth_loss_fwd(r, a, b, c, e, ws, nbytes, None),
            lib.lsi_edge_smooth_loss_bwd(r, a, b, c, e, ws, None))

  assert calls(None) == (EINVAL,) * 2
  assert lib.lsi_edge_smooth_workspace_bytes(None) == 0
  for bad in (dict(order=0), dict(order=3), dict(order=-1),
              dict(H=1), dict(W=1),                      # order 1 needs 2
              dict(order=2, H=2), dict(order=2, W=2),    # order 2 needs 3
              dict(alpha=-1.0), dict(alpha=float('inf')), dict(alpha=float('nan')),
              dict(L=0), dict(B=-1), dict(H=0), dict(W=-4)):
    d = _desc(_C, **bad)
    assert calls(d) == (EINVAL,) * 2, bad
    assert lib.lsi_edge_smooth_workspace_bytes(ctypes.byref(d)) == 0, bad
  # a bad descriptor wins over a NULL pointer, a NULL pointer over the workspace
  assert calls(_desc(_C, order=3), a=None, nbytes=0) == (EINVAL,) * 2
  d = _desc(_C)
  for null in ('a', 'b', 'c', 'e', 'ws'):
    assert calls(d, **{null: None}, nbytes=0) == (ENULL,) * 2, null
  short = int(lib.lsi_edge_smooth_workspace_bytes(ctypes.byref(d))) - 1
  # (the backward takes no workspace: with these arguments it would launch)
  assert lib.lsi_edge_smooth_loss_fwd(ctypes.byref(d), p, p, p, p, p, short,
                                      None) == EWORKSPACE
  # the smallest planes are valid: the refusal is the NULL pointer's
  assert calls(_desc(_C, H=2, W=2), a=None) == (ENULL,) * 2
  assert calls(_desc(_C, order=2, H=3, W=3, alpha=0.0), a=None) == (ENULL,) * 2


def test_workspace_formula(built_lib):
  from lsi import _C
  lib = _C.lib()
  # (3 L B bpp + L B) doubles, bpp = min(max(ceil(H W / 1024), 1), 256)
  for (nl, b, h, w) in ((1, 1, 2, 3), (2, 3, 16, 24), (3, 2, 32, 32), (3, 2, 32, 33),
                        (4, 8, 256, 768), (1, 2, 600, 900)):
    bpp = min(max(-(-h * w // 1024), 1), 256)
    d = _desc(_C, L=nl, B=b, H=h, W=w)
    assert lib.lsi_edge_smooth_workspace_bytes(ctypes.byref(d)) == \
        (3 * nl * b * bpp + nl * b) * 8, (nl, b, h, w)
  assert min(max(-(-32 * 33 // 1024), 1), 256) == 2
  assert min(max(-(-600 * 900 // 1024), 1), 256) == 256


def test_no_cpu_path(built_lib):
  from lsi.loss import _hip, loss
  disp, guide = torch.rand(2, 1, 8, 8, 1), torch.rand(1, 8, 8, 3)
  before = dict(_hip.CALLS)
  assert before.keys() >= {'edge_fwd', 'edge_bwd'}
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    loss.edge_aware_smoothness_loss(disp, guide)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    _hip.edge_smoothness_loss(disp, guide, 1.0, 2, False)
  with pytest.raises(RuntimeError, match='not differentiable'):
    _hip.edge_smoothness_loss(disp, guide.clone().requires_grad_(True), 1.0, 1, True)
  assert _hip.CALLS == before


def test_descriptor_from_tensors():
  """edge_smooth_desc reads the strides of views and refuses what the kernels
  would (it touches no device)."""
  sys.path.insert(0, PKG)
  from lsi.loss import _hip
  two = torch.zeros(2, 3, 5, 7, 2)
  chw = torch.zeros(3, 3, 5, 7).permute(0, 2, 3, 1)
  d = _hip.edge_smooth_desc(two[..., 1:], chw, 2.0, 2, True, 't')
  assert (d.L, d.B, d.H, d.W, d.order, d.normalise) == (2, 3, 5, 7, 2, 1)
  assert (d.d_sl, d.d_sb, d.d_sy, d.d_sx) == (210, 70, 14, 2)
  assert (d.g_sl, d.g_sb, d.g_sy, d.g_sx, d.g_sc) == (0, 105, 7, 1, 35)
  assert d.alpha == 2.0 and abs(d.eps - 1e-7) < 1e-14
  d = _hip.edge_smooth_desc(two[..., :1], torch.zeros(2, 3, 5, 7, 3), 0.0, 1, False, 't')
  assert (d.g_sl, d.g_sb, d.g_sy, d.g_sx, d.g_sc) == (315, 105, 21, 3, 1)
  disp = two[..., :1]
  for guide, alpha, order in ((torch.zeros(2, 5, 7, 3), 1.0, 1),      # batch
                              (torch.zeros(3, 5, 7, 4), 1.0, 1),      # channels
                              (torch.zeros(3, 3, 5, 7, 3), 1.0, 1),   # layers
                              (torch.zeros(3, 5, 7, 3), -1.0, 1),
                              (torch.zeros(3, 5, 7, 3), float('nan'), 1),
                              (torch.zeros(3, 5, 7, 3), 1.0, 3)):
    with pytest.raises(ValueError):
      _hip.edge_smooth_desc(disp, guide, alpha, order, True, 't')
  with pytest.raises(ValueError, match='rows'):
    _hip.edge_smooth_desc(torch.zeros(1, 1, 2, 7, 1), torch.zeros(1, 2, 7, 3), 1.0, 2,
                          True, 't')


def test_flags_and_their_defaults():
  sys.path.insert(0, PKG)
  import ldi_enc_dec
  o = ldi_enc_dec.build_parser().parse_args([])
  assert (o.edge_smooth_wt, o.edge_smooth_alpha, o.edge_smooth_order,
          o.edge_smooth_norm, o.edge_smooth_guide) == (0.0, 1.0, 1, True, 'image')
  o = ldi_enc_dec.build_parser().parse_args(
      ['--edge_smooth_wt', '0.1', '--edge_smooth_alpha', '10', '--edge_smooth_order',
       '2', '--edge_smooth_norm', 'false', '--edge_smooth_guide', 'texture'])
  assert (o.edge_smooth_wt, o.edge_smooth_alpha, o.edge_smooth_order,
          o.edge_smooth_norm, o.edge_smooth_guide) == (0.1, 10.0, 2, False, 'texture')
  with pytest.raises(SystemExit):
    ldi_enc_dec.build_parser().parse_args(['--edge_smooth_guide', 'depth'])
