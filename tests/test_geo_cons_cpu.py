"""The geometric-consistency loss, the parts that need no GPU:
the restatements of tests/geo_cons_ref.py against a 2 x 3 example worked by hand
and against central differences, the fp32 op restatement against the NumPy one,
header / binding / exports agree, the entries refuse bad arguments before any
launch and in the stated order, the workspace follows its formula, and the
Python surface exists (no CPU path, refusals, three trainer flags).

The hand example: one plane of 2 x 3 against one partner plane (shift 0), M = I
with M[0][3] = 1, so u = x + .5 + d, v = y + .5, n = 1, dd = d: a pixel samples
its own row of E at x + d.

    D = [[1/2, 1, 1/2], [1/4, NaN, 0]]     E = [[1, 2, 4], [1/2, 1/4, 0]]

    (0,0)  x' = 1/2   s = (1 + 2) / 2 = 3/2     dd = 1/2
    (0,1)  x' = 2     s = 4 (x1 = 3 is outside: weight and mask 0)   dd = 1
    (0,2)  u = 3 > W - 1/2: not scored
    (1,0)  x' = 1/4   s = 3/4 1/2 + 1/4 1/4 = 7/16   dd = 1/4
    (1,1)  NaN: not scored     (1,2)  d = 0: dd = 0 and s = 0: not scored

N = 3, dd < s everywhere (sign -1), du/dd = ddd/dd = 1, ds/du = E[x1] - E[x0]
= 1, -4 (the outside tap's mask is 0), -1/4.
l1:    e = 1, 3, 3/16; loss = 67/48; dD = (-1 + ds/du) (-1)(-1) ... = (-1 + 1,
       -1 - 4, -1 - 1/4) / 3; dE = +c_k / 3.
ratio: e = 1/2, 3/5, 3/11; de/ds = 2 dd / b^2 = 1/4, 2/25, 128/121; de/ddd =
       -2 s / b^2 = -3/4, -8/25, -224/121; dD = (de/ddd + de/ds ds/du) / 3 =
       -1/6, -16/75, -256/363."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

import geo_cons_ref as ref

NEW = ('lsi_geo_cons_workspace_bytes', 'lsi_geo_cons_loss_fwd',
       'lsi_geo_cons_loss_bwd')
EINVAL, ENULL, EWORKSPACE = -1, -2, -3     # include/lsi_hip.h
NAN = float('nan')
HAND_D = np.array([[[0.5, 1.0, 0.5], [0.25, NAN, 0.0]]], np.float32)
HAND_E = np.array([[[1.0, 2.0, 4.0], [0.5, 0.25, 0.0]]], np.float32)
HAND_M = np.eye(4, dtype=np.float32)[None].copy()
HAND_M[0, 0, 3] = 1.0
HAND_SCORED = np.array([[[1, 1, 0], [1, 0, 0]]], bool)


def test_l1_by_hand():
  l, gD, gE, sums, emap, sc = ref.loss_and_grad(HAND_D, HAND_E, HAND_M, 0, 'l1')
  assert np.array_equal(sc, HAND_SCORED)
  assert sums.tolist() == [[1 + 3 + 3 / 16, 3.0, 0.0]]
  assert l == (1 + 3 + 3 / 16) / 3
  assert np.array_equal(emap, np.array([[[1, 3, -1], [3 / 16, -1, -1]]], np.float32))
  want = np.array([[[0.0, -5.0, 0.0], [-1.25, 0.0, 0.0]]]) / 3
  assert np.abs(gD - want).max() <= 1e-15
  want = np.array([[[0.5, 0.5, 1.0], [0.75, 0.25, 0.0]]]) / 3
  assert np.abs(gE - want).max() <= 1e-15
  # an upstream factor scales the gradients
  _, g2, e2, _, _, _ = ref.loss_and_grad(HAND_D, HAND_E, HAND_M, 0, 'l1', upstream=2.5)
  assert np.abs(g2 - 2.5 * gD).max() <= 1e-15 and np.abs(e2 - 2.5 * gE).max() <= 1e-15


def test_ratio_by_hand():
  l, gD, gE, sums, emap, sc = ref.loss_and_grad(HAND_D, HAND_E, HAND_M, 0, 'ratio')
  assert np.array_equal(sc, HAND_SCORED) and sums[0, 1] == 3.0
  assert abs(l - (1 / 2 + 3 / 5 + 3 / 11) / 3) <= 1e-15
  want = np.array([[[-1 / 6, -16 / 75, 0.0], [-256 / 363, 0.0, 0.0]]])
  assert np.abs(gD - want).max() <= 1e-15
  want = np.array([[[1 / 24, 1 / 24, 2 / 75], [32 / 121, 32 / 363, 0.0]]])
  assert np.abs(gE - want).max() <= 1e-15
  assert np.array_equal(emap, np.array([[[1 / 2, 3 / 5, -1], [3 / 11, -1, -1]]],
                                       np.float32))


def test_sign_of_zero_is_zero_and_the_paired_form_adds_both():
  # two planes, each the other's partner, identity: dd == s everywhere
  D = (np.arange(1, 13, dtype=np.float32) / 16).reshape(1, 3, 4)
  D = np.concatenate([D, D])
  M = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
  for mode in ref.MODES:
    l, gD, gE, sums, emap, sc = ref.loss_and_grad(D, D, M, 1, mode, paired=True)
    assert sc.all() and l == 0.0 and not gD.any() and not emap.any()
  # one pixel moved: its own term and, through the tap, the partner's
  D2 = D.copy()
  D2[0, 1, 2] += 0.25
  l, gD, gE, _, _, _ = ref.loss_and_grad(D2, D2, M, 1, 'l1', paired=True)
  assert l == 0.25 / 12
  want = np.zeros(D.shape)
  # plane 0 (dd > s): +1 own, -1 at the partner's tap; plane 1 (dd < s): -1 own,
  # +1 at the tap, which is the moved pixel: 2 / (12 * 2) there, -2 / 24 on plane 1
  want[0, 1, 2], want[1, 1, 2] = 2 / 24, -2 / 24
  assert np.abs(gD - want).max() <= 1e-16 and gD is gE


def _scene(p, h, w, seed, general):
  """A smooth paired scene off the lattice: P / 2 views and their partners."""
  rng = np.random.RandomState(seed)
  yy, xx = np.mgrid[0:h, 0:w]
  D = np.stack([0.2 + 0.05 * np.sin(0.3 * xx + i) + 0.04 * np.cos(0.4 * yy - i) +
                0.01 * rng.uniform(size=(h, w)) for i in range(p)]).astype(np.float32)
  M = np.tile(np.eye(4, dtype=np.float32), (p, 1, 1))
  half = p // 2
  M[:half, 0, 3], M[half:, 0, 3] = -7.3, 7.3
  if general:
    M[:, 0, 1], M[:, 1, 0], M[:, 2, 3], M[:, 1, 3] = 0.02, -0.015, 0.3, 0.9
    M[:, 3, 0] = 1e-4
  return D, M


@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('general', [False, True])
def test_gradient_against_central_differences(mode, general):
  p, h, w = 4, 7, 11
  D, M = _scene(p, h, w, 5, general)
  rng = np.random.RandomState(11)
  E = (D[::-1] * rng.uniform(0.8, 1.25, D.shape)).astype(np.float32)
  l, gD, gE, sums, _, sc = ref.loss_and_grad(D, E, M, 2, mode, occl_thresh=0.15)
  assert 0.4 * sc.size < sc.sum() < sc.size
  # fp64 throughout reproduces the loss of the fp32-formed values closely
  l64 = ref.loss_frozen(D, E, M, 2, mode, sc)
  assert abs(l64 - l) <= 2e-5 * l
  hstep = 1e-6
  worst = 0.0
  for which, g in (('D', gD), ('E', gE)):
    for idx in zip(*np.unravel_index(rng.permutation(D.size)[:60], D.shape)):
      a, b = D.astype(np.float64), E.astype(np.float64)
      t = a if which == 'D' else b
      t[idx] += hstep
      up = ref.loss_frozen(a, b, M, 2, mode, sc)
      t[idx] -= 2 * hstep
      dn = ref.loss_frozen(a, b, M, 2, mode, sc)
      worst = max(worst, abs((up - dn) / (2 * hstep) - g[idx]))
  # fp32 u, v (an ulp of 16 is 1e-6) against fp64 positions: 1e-4 of the largest
  # entry; a wrong term is off by the entry itself
  scale = max(np.abs(gD).max(), np.abs(gE).max())
  print('geo_cons central differences %s general=%d: worst %.3g of %.3g' %
        (mode, general, worst, scale))
  assert worst <= 1e-4 * scale


@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('paired', [False, True])
def test_the_two_restatements_agree(mode, paired):
  p, h, w = 4, 9, 13
  D, M = _scene(p, h, w, 3, True)
  E = D if paired else (D[::-1] * 1.1).astype(np.float32)
  D[0, 2, 3], D[1, 4, 4], D[2, 0, 0] = NAN, 0.0, -0.25
  l, gD, gE, sums, _, sc = ref.loss_and_grad(D, E, M, 2, mode, 0.2, 2.5, paired=paired)
  t = torch.from_numpy
  l32, sc32 = ref.loss_ops(t(D), t(E), t(M), 2, mode, 0.2, return_scored=True)
  assert np.array_equal(sc32.numpy(), sc)
  assert not sc[0, 2, 3] and not sc[1, 4, 4] and not sc[2, 0, 0]
  l32, g32, e32 = ref.loss_and_grad_ops(t(D), t(E), t(M), 2, mode, 0.2, 2.5,
                                        paired=paired)
  assert abs(l32 - l) <= 1e-6 * l
  scale = max(np.abs(gD).max(), np.abs(gE).max())
  assert np.isfinite(g32).all() and np.isfinite(e32).all()
  assert np.abs(g32 - gD).max() <= 2e-5 * scale
  assert np.abs(e32 - gE).max() <= 2e-5 * scale
  assert not gD[~sc & ~np.isfinite(D)].any()


def test_empty_planes_leave_the_mean():
  D, M = _scene(4, 6, 9, 1, False)
  E = (D[::-1] * 1.1).astype(np.float32)
  l, _, _, sums, _, sc = ref.loss_and_grad(D, E, M, 2, 'ratio')
  assert (sums[:, 1] > 0).all()
  # plane 1 looks away (n < 0), plane 3 has no partner values
  M2, E2 = M.copy(), E.copy()
  M2[1, 2, 2] = -1.0
  E2[(3 + 2) % 4] = 0.0
  l2, gD, gE, sums2, emap, sc2 = ref.loss_and_grad(D, E2, M2, 2, 'ratio')
  assert sums2[1].tolist() == [0, 0, 0] and sums2[3].tolist() == [0, 0, 0]
  assert np.array_equal(sums2[[0, 2]], sums[[0, 2]])
  assert abs(l2 - (sums[0, 0] / sums[0, 1] + sums[2, 0] / sums[2, 1]) / 2) <= 1e-16
  assert not gD[1].any() and not gD[3].any() and (emap[1] == -1).all()
  # nothing scored anywhere: 0, and zero gradients
  M3 = M.copy()
  M3[:, 2, 2] = -1.0
  l3, gD, gE, sums3, emap, sc3 = ref.loss_and_grad(D, E, M3, 2, 'l1')
  assert l3 == 0.0 and not sc3.any() and not gD.any() and not gE.any()
  t = torch.from_numpy
  l32, g32, e32 = ref.loss_and_grad_ops(t(D), t(E), t(M3), 2, 'l1')
  assert l32 == 0.0 and not g32.any() and not e32.any()


def test_the_occlusion_rule():
  # identity, one plane each: dd = d, s = E
  D = np.full((1, 2, 4), 0.25, np.float32)
  E = np.array([[[0.25, 0.3, 0.375, 0.5], [0.75, 0.2, 0.125, 0.376]]], np.float32)
  M = np.eye(4, dtype=np.float32)[None]
  # s - dd > t (s + dd) with t = 1/5: occluded from s > 3/8 on (3/8 itself: equal)
  _, _, _, _, _, sc = ref.loss_and_grad(D, E, M, 0, 'ratio', occl_thresh=0.2)
  assert sc.tolist() == [[[True, True, True, False], [False, True, True, False]]]
  # nearer than the partner's surface is never an occlusion; threshold 0: no rule
  _, _, _, _, _, sc = ref.loss_and_grad(D, E, M, 0, 'ratio', occl_thresh=0.0)
  assert sc.all()
  l, gD, gE, sums, emap, _ = ref.loss_and_grad(D, E, M, 0, 'l1', occl_thresh=0.2)
  assert sums[0, 1] == 5 and emap[0, 0, 3] == -1 and gD[0, 0, 3] == 0 == gE[0, 0, 3]


# ---------------------------------------------------------------------------
# the library and the Python surface
# ---------------------------------------------------------------------------
def _desc(_C, **kw):
  d = _C.LsiGeoConsDesc()
  d.P, d.H, d.W, d.mode = 2, 13, 37, 0
  d.d_sp, d.d_sy, d.d_sx = 13 * 37, 37, 1
  d.e_sp, d.e_sy, d.e_sx = 13 * 37, 37, 1
  d.shift, d.occl_thresh = 1, 0.0
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def test_header_binding_and_exports_agree(built_lib):
  from lsi import _C
  with open(os.path.join(ROOT, 'include', 'lsi_hip.h')) as f:
    h = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
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
  assert n_params == {'lsi_geo_cons_workspace_bytes': 1, 'lsi_geo_cons_loss_fwd': 10,
                      'lsi_geo_cons_loss_bwd': 9}
  assert re.search(r'#define LSI_GEO_CONS_RATIO 0\b', h)
  assert re.search(r'#define LSI_GEO_CONS_L1 1\b', h)
  assert (_C.LSI_GEO_CONS_RATIO, _C.LSI_GEO_CONS_L1) == (0, 1)
  # the struct: 4 int32, 6 int64, 1 int32, 1 float -- no padding
  m = re.search(r'typedef struct LsiGeoConsDesc \{(.*?)\} LsiGeoConsDesc;', h, flags=re.S)
  fields = re.findall(r'\b([A-Za-z_0-9]+)\s*[,;]', m.group(1))
  assert fields == [f[0] for f in _C.LsiGeoConsDesc._fields_]
  assert fields == ['P', 'H', 'W', 'mode', 'd_sp', 'd_sy', 'd_sx', 'e_sp', 'e_sy', 'e_sx',
                    'shift', 'occl_thresh']
  assert ctypes.sizeof(_C.LsiGeoConsDesc) == 4 * 4 + 6 * 8 + 4 + 4
  assert _C.LsiGeoConsDesc.d_sp.offset == 16 and _C.LsiGeoConsDesc.shift.offset == 64
  from lsi.loss import loss
  assert callable(loss.geometric_consistency_loss)


def test_argument_errors_are_reported_before_any_launch(built_lib):
  from lsi import _C
  lib = _C.lib()
  big = 1 << 30
  p = ctypes.c_void_p(16)     # never dereferenced: every call below is refused

  def calls(d, disp=p, partner=p, m=p, a=p, b=p, g=p, nbytes=big):
    r = ctypes.byref(d) if d is not None else None
    # fwd: out_loss, plane_sums, out_map (may be NULL), workspace;
    # bwd: plane_sums, g_loss, g_disp, g_partner (may be NULL)
    return (lib.lsi_geo_cons_loss_fwd(r, disp, partner, m, a, b, None, g, nbytes, None),
            lib.lsi_geo_cons_loss_bwd(r, disp, partner, m, a, b, g, None, None))

  assert calls(None) == (EINVAL,) * 2
  assert lib.lsi_geo_cons_workspace_bytes(None) == 0
  for bad in (dict(mode=2), dict(mode=-1), dict(P=0), dict(H=0), dict(W=-3),
              dict(P=65536), dict(H=4096, W=4096), dict(P=200, H=4095, W=4096),
              dict(shift=-1), dict(shift=2), dict(occl_thresh=-0.1),
              dict(occl_thresh=1.0), dict(occl_thresh=NAN)):
    d = _desc(_C, **bad)
    assert calls(d) == (EINVAL,) * 2, bad
    assert lib.lsi_geo_cons_workspace_bytes(ctypes.byref(d)) == 0, bad
  # a bad descriptor wins over a NULL pointer, a NULL pointer over the workspace
  assert calls(_desc(_C, mode=7), disp=None, nbytes=0) == (EINVAL,) * 2
  d = _desc(_C)
  for null in ('disp', 'partner', 'm', 'a', 'b', 'g'):
    assert calls(d, **{null: None}, nbytes=0) == (ENULL,) * 2, null
  short = int(lib.lsi_geo_cons_workspace_bytes(ctypes.byref(d))) - 1
  assert short > 0
  # (the backward takes no workspace: with these arguments it would launch)
  assert lib.lsi_geo_cons_loss_fwd(ctypes.byref(d), p, p, p, p, p, None, p, short,
                                   None) == EWORKSPACE
  assert lib.lsi_geo_cons_loss_fwd(ctypes.byref(d), p, p, p, p, p, p, p, short,
                                   None) == EWORKSPACE
  # the edges of the ranges are valid: the refusal is the NULL pointer's
  for edge in (dict(mode=1), dict(P=1, H=1, W=1, shift=0), dict(P=65535, H=1, W=1),
               dict(H=1, W=(1 << 24) - 1), dict(shift=0), dict(occl_thresh=0.999)):
    assert calls(_desc(_C, **edge), disp=None) == (ENULL,) * 2, edge


def test_workspace_formula(built_lib):
  from lsi import _C
  lib = _C.lib()
  # (3 P bpp + P) doubles; a block covers r = max(ceil(1024 / W), ceil(H / 256))
  # rows, bpp = ceil(H / r)
  want = {}
  for (p, h, w) in ((2, 1, 1), (2, 13, 37), (2, 40, 150), (8, 9, 17), (2, 24, 72),
                    (8, 256, 768), (2, 375, 1242), (2, 3000, 8)):
    r = max(-(-1024 // w), -(-h // 256))
    bpp = -(-h // r)
    want[(p, h, w)] = bpp
    d = _desc(_C, P=p, H=h, W=w)
    assert lib.lsi_geo_cons_workspace_bytes(ctypes.byref(d)) == \
        (3 * p * bpp + p) * 8, (p, h, w)
  # the GPU tests' shapes: one block per plane, and several
  assert want[(2, 13, 37)] == 1 and want[(2, 40, 150)] == 6
  assert want[(8, 256, 768)] == 128 and want[(2, 3000, 8)] == 24


def test_no_cpu_path_and_python_side_refusals(built_lib):
  from lsi.loss import _hip, loss
  d = torch.rand(4, 8, 8, 1) + 0.1
  m = torch.eye(4).repeat(4, 1, 1)
  before = dict(_hip.CALLS)
  assert before.keys() >= {'geo_cons_fwd', 'geo_cons_bwd'}
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    loss.geometric_consistency_loss(d, m)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    loss.geometric_consistency_loss(d[..., 0], m, partner_disps=d[..., 0], mode='l1',
                                    occl_thresh=0.2, return_map=True)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    _hip.geometric_consistency_loss(d[..., 0], None, m, 'ratio', 0.0)
  # dtype
  with pytest.raises(RuntimeError, match='fp32'):
    loss.geometric_consistency_loss(d.double(), m)
  with pytest.raises(RuntimeError, match='fp32'):
    loss.geometric_consistency_loss(d, m.double())
  with pytest.raises(RuntimeError, match='fp32'):
    loss.geometric_consistency_loss(d, m, partner_disps=d.half())
  # shape
  with pytest.raises(RuntimeError, match='one shape'):
    loss.geometric_consistency_loss(d, m, partner_disps=d[:2])
  with pytest.raises(RuntimeError, match='per plane'):
    loss.geometric_consistency_loss(d, m[:2])
  with pytest.raises(RuntimeError, match='per plane'):
    loss.geometric_consistency_loss(d, torch.eye(4))
  with pytest.raises(RuntimeError, match='H, W'):
    loss.geometric_consistency_loss(torch.rand(8), m)
  buf = torch.rand(3, 4, 8, 8, 1)
  with pytest.raises(RuntimeError, match='without a copy'):
    loss.geometric_consistency_loss(buf[:, :2], torch.eye(4).repeat(6, 1, 1))
  # the cameras are constants
  with pytest.raises(RuntimeError, match='not differentiable'):
    loss.geometric_consistency_loss(d, m.clone().requires_grad_(True))
  # what the entries would refuse
  with pytest.raises(ValueError, match='even'):
    loss.geometric_consistency_loss(d[:3], m[:3])
  for kw in (dict(mode='l2'), dict(occl_thresh=-0.1), dict(occl_thresh=1.0),
             dict(occl_thresh=NAN)):
    with pytest.raises(ValueError):
      loss.geometric_consistency_loss(d, m, **kw)
  assert _hip.CALLS == before


def test_descriptor_from_tensors():
  """geo_cons_desc reads the strides of views (it touches no device)."""
  sys.path.insert(0, PKG)
  from lsi.loss import _hip, loss
  buf = torch.zeros(3, 4, 5, 7, 1)            # L x 2 B x H x W x 1
  d0 = loss._planes(buf[0], 'disps', 'geometric_consistency_loss')
  m = torch.zeros(4, 4, 4)
  d = _hip.geo_cons_desc(d0, None, m, 'ratio', 0.0, 't')
  assert (d.P, d.H, d.W, d.mode, d.shift) == (4, 5, 7, 0, 2)
  assert (d.d_sp, d.d_sy, d.d_sx) == (35, 7, 1) == (d.e_sp, d.e_sy, d.e_sx)
  e = torch.zeros(4, 5, 14)[:, :, ::2]
  d = _hip.geo_cons_desc(d0, e, m, 'l1', 0.25, 't')
  assert (d.mode, d.shift, d.occl_thresh) == (1, 0, 0.25)
  assert (d.e_sp, d.e_sy, d.e_sx) == (70, 14, 2)


def test_flags_and_their_defaults():
  sys.path.insert(0, PKG)
  import ldi_enc_dec
  o = ldi_enc_dec.build_parser().parse_args([])
  assert (o.geo_cons_wt, o.geo_cons_mode, o.geo_cons_occl) == (0.0, 'ratio', 0.0)
  o = ldi_enc_dec.build_parser().parse_args(
      ['--geo_cons_wt', '0.5', '--geo_cons_mode', 'l1', '--geo_cons_occl', '0.2'])
  assert (o.geo_cons_wt, o.geo_cons_mode, o.geo_cons_occl) == (0.5, 'l1', 0.2)
  with pytest.raises(SystemExit):
    ldi_enc_dec.build_parser().parse_args(['--geo_cons_mode', 'huber'])
