"""The sparse depth-supervision loss, the parts that need no
GPU: the fp64 restatement of tests/depth_sup_ref.py against a 1 x 2 x 3 example
worked by hand and against central differences, the fp32 op restatement against
it, header / binding / exports agree, the entries refuse bad arguments before
any launch and in the stated order, the workspace follows its formula, and the
Python surface exists (no CPU path, RuntimeError for a wrong dtype or shape,
five trainer flags).

The hand example (eps = 2^-10, valid_above = 0, g in [1/80, 1000]), u = ln 2:

    gt   = [[1, 1/2, 0], [1/4, NaN, 2]]      scored: 1, 1/2, 1/4, 2   (n = 4)
    pred = [[2, 1/2, 3], [1,   5,   0]]      q at gt = 2: eps (clamped)

silog: d = (1, 0, 2, -11) u, A = -8 u, Q = 126 u^2, D = 31.5 u^2 - lam 4 u^2.
At lam = 1/2: 2 lam A / n^2 = -u / 2, so the gradient is (d_i / 2 + u / 2) / q_i
= u / 2, u, 3 u / 2 at the three free pixels, 0 at the clamped one.
l1: |e| = (1, 0, 3/4, 2 - 2^-10), loss = (3.75 - 2^-10) / 4, gradient 1/4, 0
(sign(0)), 1/4, and 0 at the clamped pixel."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

import depth_sup_ref as ref

NEW = ('lsi_depth_sup_workspace_bytes', 'lsi_depth_sup_loss_fwd',
       'lsi_depth_sup_loss_bwd')
EINVAL, ENULL, EWORKSPACE = -1, -2, -3     # include/lsi_hip.h
U = math.log(2.0)
NAN = float('nan')
HAND_GT = np.array([[[1.0, 0.5, 0.0], [0.25, NAN, 2.0]]], np.float32)
HAND_PRED = np.array([[[2.0, 0.5, 3.0], [1.0, 5.0, 0.0]]], np.float32)
HAND_KW = dict(valid_above=0.0, g_min=1.0 / 80, g_max=1000.0, eps=2.0 ** -10)


def test_silog_by_hand():
  for lam in (0.0, 0.5, 1.0):
    l, g, sums = ref.loss_and_grad(HAND_PRED, HAND_GT, None, 'silog', lam, **HAND_KW)
    assert sums[0, 0] == 4.0
    assert abs(sums[0, 1] + 8 * U) <= 1e-14 and abs(sums[0, 2] - 126 * U * U) <= 1e-12
    assert abs(l - (31.5 - 4 * lam) * U * U) <= 1e-13
  l, g, _ = ref.loss_and_grad(HAND_PRED, HAND_GT, None, 'silog', 0.5, **HAND_KW)
  want = np.array([[[0.5 * U, U, 0.0], [1.5 * U, 0.0, 0.0]]])
  assert np.abs(g - want).max() <= 1e-14
  # the hole, the NaN and the clamped pixel: exactly 0
  assert g[0, 0, 2] == 0.0 and g[0, 1, 1] == 0.0 and g[0, 1, 2] == 0.0
  # gt_scale: 4 gt' = gt
  l2, g2, _ = ref.loss_and_grad(HAND_PRED, HAND_GT / 4, np.array([4.0]), 'silog', 0.5,
                                **HAND_KW)
  assert l2 == l and np.array_equal(g2, g)
  # an upstream gradient scales the gradient
  _, g3, _ = ref.loss_and_grad(HAND_PRED, HAND_GT, None, 'silog', 0.5, upstream=2.5,
                               **HAND_KW)
  assert np.abs(g3 - 2.5 * want).max() <= 1e-14


def test_l1_by_hand():
  l, g, sums = ref.loss_and_grad(HAND_PRED, HAND_GT, None, 'l1', 0.5, **HAND_KW)
  assert sums[0, 0] == 4.0 and sums[0, 1] == 3.75 - 2.0 ** -10 and sums[0, 2] == 0.0
  assert l == (3.75 - 2.0 ** -10) / 4
  assert np.array_equal(g, np.array([[[0.25, 0.0, 0.0], [0.25, 0.0, 0.0]]]))


def test_validity_is_the_ground_truths_alone():
  gt = np.array([[[0.3, 0.2, 0.5, 1.0 / 100, 2000.0, NAN, float('inf'), -1.0]]],
                np.float32)
  ok, _ = ref.scored(gt, None, 0.2, 1.0 / 80, 1000.0)
  # 0.2 is not above valid_above; 1/100 < g_min; 2000 > g_max
  assert ok.tolist() == [[[True, False, True, False, False, False, False, False]]]
  ok, g = ref.scored(gt, np.array([2.0]), 0.0, 1.0 / 80, 1000.0)
  assert ok.tolist() == [[[True, True, True, True, False, False, False, False]]]
  assert g[0, 0, 3] == np.float32(1.0 / 100) * np.float32(2.0)


def test_empty_planes_leave_the_mean():
  """Two planes, the second without a scored pixel: S = 1, the first plane's term;
  none scored: loss 0 and gradient 0."""
  gt = np.concatenate([HAND_GT, np.zeros_like(HAND_GT)], 0)
  pred = np.concatenate([HAND_PRED, HAND_PRED], 0)
  for mode in ref.MODES:
    l1, g1, _ = ref.loss_and_grad(HAND_PRED, HAND_GT, None, mode, 0.5, **HAND_KW)
    l2, g2, sums = ref.loss_and_grad(pred, gt, None, mode, 0.5, **HAND_KW)
    assert l2 == l1 and np.array_equal(g2[0], g1[0]) and not g2[1].any()
    assert sums[1].tolist() == [0.0, 0.0, 0.0]
    l0, g0, _ = ref.loss_and_grad(pred, 0 * gt, None, mode, 0.5, **HAND_KW)
    assert l0 == 0.0 and not g0.any()
    t = lambda a: torch.from_numpy(a)
    lo, go = ref.loss_and_grad_ops(t(pred), t(0 * gt), None, mode, 0.5, **HAND_KW)
    assert lo == 0.0 and not go.any()


def _random_case(seed, p=3, h=5, w=7):
  rng = np.random.RandomState(seed)
  gt = rng.uniform(0.05, 1.0, (p, h, w)).astype(np.float32)
  gt[rng.uniform(size=gt.shape) < 0.4] = 0.0
  gt[0, 0, 0], gt[1, 2, 3] = NAN, 5000.0
  gt[2] = 0.0
  gt[2, 1, 1] = 0.5
  pred = rng.uniform(0.05, 1.0, (p, h, w)).astype(np.float32)
  pred[0, 1, 1], pred[1, 0, 0], pred[1, 1, 1] = 0.0, NAN, -1.0
  return pred, gt, np.array([0.5, 1.0, 2.0], np.float32)


@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('lam', [0.0, 0.5, 1.0])
def test_gradient_against_central_differences(mode, lam):
  pred, gt, scale = _random_case(3)
  kw = dict(valid_above=0.0, g_min=1.0 / 80, g_max=1000.0, eps=1e-6)
  l, g, sums = ref.loss_and_grad(pred, gt, scale, mode, lam, upstream=2.5, **kw)
  assert sums[:, 0].min() == 1.0 and np.isfinite(g).all() and l > 0
  ok, g32 = ref.scored(gt, scale, kw['valid_above'], kw['g_min'], kw['g_max'])
  # (l1: no scored prediction sits on the kink)
  assert np.abs(ref.clamp(pred, kw['eps'])[0] - g32)[ok].min() > 1e-3
  # the restatement takes fp32 predictions: difference it in fp64 through its
  # own arithmetic, on the pixels it says carry a gradient and on the others
  def f(q):
    return _loss64(q, gt, scale, mode, lam, **kw)
  step = 1e-6
  num = np.zeros_like(g)
  base = pred.astype(np.float64)
  # (a prediction of 0, NaN or -1 is eps: so is -1, a step away from the clamp)
  base[~ref.clamp(pred, kw['eps'])[1]] = -1.0
  for idx in np.ndindex(*pred.shape):
    hi, lo = base.copy(), base.copy()
    hi[idx] += step
    lo[idx] -= step
    num[idx] = 2.5 * (f(hi) - f(lo)) / (2 * step)
  # clamped predictions (0, NaN, -1) sit strictly inside the clamp: 0 both ways
  assert np.abs(num - g).max() <= 1e-7 * max(np.abs(g).max(), 1.0)
  for idx in ((0, 1, 1), (1, 0, 0), (1, 1, 1)):
    assert g[idx] == 0.0 and num[idx] == 0.0
  assert g[~ok].max() == 0.0 and g[~ok].min() == 0.0


def _loss64(pred64, gt, scale, mode, lam, valid_above, g_min, g_max, eps):
  """The definition on fp64 predictions (the restatement's own takes fp32)."""
  ok, g32 = ref.scored(gt, scale, valid_above, g_min, g_max)
  q = np.maximum(pred64, float(np.float32(eps)))
  g = np.where(ok, g32, 1.0).astype(np.float64)
  q = np.where(ok, q, 1.0)
  n = ok.reshape(ok.shape[0], -1).sum(1).astype(np.float64)
  has = n > 0
  nn = np.where(has, n, 1.0)
  flat = lambda a: a.reshape(a.shape[0], -1).sum(1)
  if mode == 'silog':
    d = np.log(q) - np.log(g)
    terms = flat(d * d) / nn - lam * (flat(d) / nn) ** 2
  else:
    terms = flat(np.abs(q - g)) / nn
  return float(terms[has].sum() / has.sum())


@pytest.mark.parametrize('mode', ref.MODES)
def test_the_two_restatements_agree(mode):
  pred, gt, scale = _random_case(4)
  kw = dict(valid_above=0.0, g_min=1.0 / 80, g_max=1000.0, eps=1e-6)
  l64, g64, _ = ref.loss_and_grad(pred, gt, scale, mode, 0.5, upstream=2.5, **kw)
  assert abs(l64 - _loss64(np.nan_to_num(pred.astype(np.float64)), gt, scale, mode,
                           0.5, **kw)) <= 1e-14
  t = torch.from_numpy
  l32, g32 = ref.loss_and_grad_ops(t(pred), t(gt), t(scale), mode, 0.5, upstream=2.5,
                                   **kw)
  assert abs(l32 - l64) <= 1e-5 * l64
  assert np.abs(g32 - g64).max() <= 1e-5 * np.abs(g64).max()
  assert np.array_equal(g32 == 0.0, g64 == 0.0)


def _desc(_C, **kw):
  d = _C.LsiDepthSupDesc()
  d.P, d.H, d.W, d.mode = 4, 16, 24, 0
  d.p_sp, d.p_sy, d.p_sx = 16 * 24, 24, 1
  d.g_sp, d.g_sy, d.g_sx = 16 * 24, 24, 1
  d.valid_above, d.g_min, d.g_max, d.eps, d.lam = 0.0, 1.0 / 80, 1000.0, 1e-6, 0.5
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
  assert n_params == {'lsi_depth_sup_workspace_bytes': 1, 'lsi_depth_sup_loss_fwd': 9,
                      'lsi_depth_sup_loss_bwd': 8}
  assert re.search(r'#define LSI_DEPTH_SUP_SILOG 0\b', h)
  assert re.search(r'#define LSI_DEPTH_SUP_L1 1\b', h)
  assert (_C.LSI_DEPTH_SUP_SILOG, _C.LSI_DEPTH_SUP_L1) == (0, 1)
  # the struct: 4 int32, 6 int64, 5 float, 1 int32 -- no padding
  m = re.search(r'typedef struct LsiDepthSupDesc \{(.*?)\} LsiDepthSupDesc;', h,
                flags=re.S)
  fields = re.findall(r'\b([A-Za-z_0-9]+)\s*[,;]', m.group(1))
  assert fields == [f[0] for f in _C.LsiDepthSupDesc._fields_]
  assert fields == ['P', 'H', 'W', 'mode', 'p_sp', 'p_sy', 'p_sx', 'g_sp', 'g_sy',
                    'g_sx', 'valid_above', 'g_min', 'g_max', 'eps', 'lam', 'reserved']
  assert ctypes.sizeof(_C.LsiDepthSupDesc) == 4 * 4 + 6 * 8 + 5 * 4 + 4
  assert _C.LsiDepthSupDesc.p_sp.offset == 16
  assert _C.LsiDepthSupDesc.valid_above.offset == 64


def test_argument_errors_are_reported_before_any_launch(built_lib):
  from lsi import _C
  lib = _C.lib()
  big = 1 << 30
  p = ctypes.c_void_p(16)     # never dereferenced: every call below is refused

  def calls(d, pred=p, gt=p, scale=p, a=p, b=p, c=p, nbytes=big):
    r = ctypes.byref(d) if d is not None else None
    # fwd: out_loss, plane_sums, workspace; bwd: plane_sums, g_loss, g_pred
    return (lib.lsi_depth_sup_loss_fwd(r, pred, gt, scale, a, b, c, nbytes, None),
            lib.lsi_depth_sup_loss_bwd(r, pred, gt, scale, a, b, c, None))

  inf, nan = float('inf'), float('nan')
  assert calls(None) == (EINVAL,) * 2
  assert lib.lsi_depth_sup_workspace_bytes(None) == 0
  for bad in (dict(mode=2), dict(mode=-1), dict(P=0), dict(H=0), dict(W=-3),
              dict(g_min=0.0), dict(g_min=-1.0), dict(g_max=1.0 / 81),
              dict(valid_above=-0.5), dict(eps=0.0), dict(eps=-1e-6),
              dict(lam=-0.01), dict(lam=1.01),
              dict(valid_above=inf), dict(g_min=nan), dict(g_max=inf), dict(eps=inf),
              dict(eps=nan), dict(lam=nan), dict(valid_above=nan),
              dict(H=1 << 16, W=1 << 15)):
    d = _desc(_C, **bad)
    assert calls(d) == (EINVAL,) * 2, bad
    assert lib.lsi_depth_sup_workspace_bytes(ctypes.byref(d)) == 0, bad
  # a bad descriptor wins over a NULL pointer, a NULL pointer over the workspace
  assert calls(_desc(_C, mode=7), pred=None, nbytes=0) == (EINVAL,) * 2
  d = _desc(_C)
  for null in ('pred', 'gt', 'a', 'b', 'c'):
    assert calls(d, **{null: None}, nbytes=0) == (ENULL,) * 2, null
  short = int(lib.lsi_depth_sup_workspace_bytes(ctypes.byref(d))) - 1
  assert short > 0
  # only gt_scale may be NULL: the refusal is then the workspace's
  # (the backward takes no workspace: with these arguments it would launch)
  assert lib.lsi_depth_sup_loss_fwd(ctypes.byref(d), p, p, None, p, p, p, short,
                                    None) == EWORKSPACE
  assert lib.lsi_depth_sup_loss_fwd(ctypes.byref(d), p, p, p, p, p, p, short,
                                    None) == EWORKSPACE
  # the edges of the ranges are valid: the refusal is the NULL pointer's
  for edge in (dict(lam=0.0), dict(lam=1.0), dict(g_max=1.0 / 80), dict(mode=1),
               dict(P=1, H=1, W=1)):
    assert calls(_desc(_C, **edge), pred=None) == (ENULL,) * 2, edge


def test_workspace_formula(built_lib):
  from lsi import _C
  lib = _C.lib()
  # (3 P bpp + P) doubles; a block covers r = max(ceil(1024 / W), ceil(H / 256))
  # rows, bpp = ceil(H / r)
  want = {}
  for (p, h, w) in ((1, 1, 1), (3, 13, 37), (2, 40, 150), (8, 9, 17), (4, 5, 70),
                    (8, 256, 768), (2, 375, 1242), (1, 3000, 8)):
    r = max(-(-1024 // w), -(-h // 256))
    bpp = -(-h // r)
    want[(p, h, w)] = bpp
    d = _desc(_C, P=p, H=h, W=w)
    assert lib.lsi_depth_sup_workspace_bytes(ctypes.byref(d)) == \
        (3 * p * bpp + p) * 8, (p, h, w)
  # the GPU tests' shapes: one block per plane, and several
  assert want[(3, 13, 37)] == 1 and want[(2, 40, 150)] == 6
  assert want[(8, 256, 768)] == 128 and want[(1, 3000, 8)] == 24


def test_no_cpu_path_and_python_side_refusals(built_lib):
  from lsi.loss import _hip, loss
  pred, gt = torch.rand(2, 8, 8, 1) + 0.1, torch.rand(2, 8, 8, 1) + 0.1
  before = dict(_hip.CALLS)
  assert before.keys() >= {'depth_sup_fwd', 'depth_sup_bwd'}
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    loss.depth_supervision_loss(pred, gt)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    loss.depth_supervision_loss(pred[..., 0], gt[..., 0], torch.ones(2), mode='l1')
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    _hip.depth_supervision_loss(pred[..., 0], gt[..., 0], None, 'silog', 0.5, 0.0,
                                1.0 / 80, 1000.0, 1e-6)
  # dtype
  with pytest.raises(RuntimeError, match='fp32'):
    loss.depth_supervision_loss(pred.double(), gt)
  with pytest.raises(RuntimeError, match='fp32'):
    loss.depth_supervision_loss(pred, gt.half())
  with pytest.raises(RuntimeError, match='fp32'):
    loss.depth_supervision_loss(pred, gt, torch.ones(2, dtype=torch.float64))
  # shape
  with pytest.raises(RuntimeError, match='one shape'):
    loss.depth_supervision_loss(pred, gt[:1])
  with pytest.raises(RuntimeError, match='one shape'):
    loss.depth_supervision_loss(pred, gt[:, :4])
  with pytest.raises(RuntimeError, match='per plane'):
    loss.depth_supervision_loss(pred, gt, torch.ones(3))
  with pytest.raises(RuntimeError, match='H, W'):
    loss.depth_supervision_loss(torch.rand(8), torch.rand(8))
  # leading dimensions that do not flatten as a view
  buf = torch.rand(3, 4, 8, 8, 1)
  with pytest.raises(RuntimeError, match='without a copy'):
    loss.depth_supervision_loss(buf[:, :2], torch.rand(3, 2, 8, 8, 1))
  # the ground truth is data
  with pytest.raises(RuntimeError, match='not differentiable'):
    loss.depth_supervision_loss(pred, gt.clone().requires_grad_(True))
  # what the entries would refuse
  for kw in (dict(mode='l2'), dict(lam=1.5), dict(lam=-0.1), dict(valid_above=-1.0),
             dict(depth_min=0.0), dict(depth_min=2.0, depth_max=1.0), dict(eps=0.0),
             dict(lam=float('nan')), dict(depth_max=float('inf'))):
    with pytest.raises(ValueError):
      loss.depth_supervision_loss(pred, gt, **kw)
  assert _hip.CALLS == before


def test_descriptor_from_tensors():
  """depth_sup_desc reads the strides of views (it touches no device); the
  public wrapper flattens the leading dimensions as views."""
  sys.path.insert(0, PKG)
  from lsi.loss import _hip, loss
  buf = torch.zeros(3, 4, 5, 7, 1)            # L x B x H x W x 1
  pred = loss._planes(buf[0], 'pred')
  assert pred.shape == (4, 5, 7) and pred.data_ptr() == buf.data_ptr()
  gt = torch.zeros(4, 5, 14)[:, :, ::2]
  d = _hip.depth_sup_desc(pred, gt, torch.ones(4), 'l1', 0.25, 0.2, 1.0 / 80, 1000.0,
                          1e-6, 't')
  assert (d.P, d.H, d.W, d.mode) == (4, 5, 7, 1)
  assert (d.p_sp, d.p_sy, d.p_sx) == (35, 7, 1)
  assert (d.g_sp, d.g_sy, d.g_sx) == (70, 14, 2)
  assert d.lam == 0.25 and d.valid_above == np.float32(0.2)
  assert d.g_min == np.float32(1.0 / 80) and d.g_max == 1000.0
  assert d.eps == np.float32(1e-6)
  # layer 1 of a packed RGBD buffer: x-stride 4
  rgbd = torch.zeros(2, 4, 5, 7, 4)
  view = loss._planes(rgbd[1, ..., 3:], 'pred')
  d = _hip.depth_sup_desc(view, gt, None, 'silog', 0.5, 0.0, 1.0 / 80, 1000.0, 1e-6,
                          't')
  assert (d.p_sp, d.p_sy, d.p_sx) == (140, 28, 4) and d.mode == 0
  assert view.data_ptr() == rgbd.data_ptr() + 4 * (4 * 5 * 7 * 4 + 3)
  # both 5-D and 4-D inputs: [..., H, W, 1] and [..., H, W]
  assert loss._planes(torch.zeros(2, 3, 5, 7, 1), 'x').shape == (6, 5, 7)
  assert loss._planes(torch.zeros(2, 3, 5, 7), 'x').shape == (6, 5, 7)
  assert loss._planes(torch.zeros(5, 7), 'x').shape == (1, 5, 7)
  # three dimensions are P x H x W, also where W = 1
  assert loss._planes(torch.zeros(3, 5, 1), 'x').shape == (3, 5, 1)


def test_g_min_and_g_max_are_fp32_quotients(monkeypatch):
  """1 / depth_max and 1 / depth_min are formed once, in fp32."""
  from lsi.loss import _hip, loss
  seen = {}

  def spy(pred, gt, gt_scale, mode, lam, valid_above, g_min, g_max, eps):
    seen.update(g_min=g_min, g_max=g_max, eps=eps, mode=mode, lam=lam,
                valid_above=valid_above)
    return None

  monkeypatch.setattr(_hip, 'depth_supervision_loss', spy)
  loss.depth_supervision_loss(torch.zeros(1, 2, 2), torch.zeros(1, 2, 2))
  assert seen['g_min'] == float(np.float32(1.0) / np.float32(80.0))
  assert seen['g_max'] == float(np.float32(1.0) / np.float32(1e-3))
  assert (seen['mode'], seen['lam'], seen['valid_above'], seen['eps']) == \
      ('silog', 0.5, 0.0, 1e-6)


def test_flags_and_their_defaults():
  sys.path.insert(0, PKG)
  import ldi_enc_dec
  o = ldi_enc_dec.build_parser().parse_args([])
  assert (o.depth_sup_wt, o.depth_sup_mode, o.depth_sup_lambda, o.depth_sup_min,
          o.depth_sup_max) == (0.0, 'silog', 0.5, 1e-3, 80.0)
  o = ldi_enc_dec.build_parser().parse_args(
      ['--depth_sup_wt', '0.5', '--depth_sup_mode', 'l1', '--depth_sup_lambda',
       '0.85', '--depth_sup_min', '1', '--depth_sup_max', '50'])
  assert (o.depth_sup_wt, o.depth_sup_mode, o.depth_sup_lambda, o.depth_sup_min,
          o.depth_sup_max) == (0.5, 'l1', 0.85, 1.0, 50.0)
  with pytest.raises(SystemExit):
    ldi_enc_dec.build_parser().parse_args(['--depth_sup_mode', 'berhu'])


def test_ground_truth_sources():
  """A positive weight names its three sources when the configuration has none."""
  sys.path.insert(0, PKG)
  import ldi_enc_dec as script

  def source(*argv):
    o = script.apply_dataset_overrides(script.build_parser().parse_args(
        ['--depth_sup_wt', '1'] + list(argv)))
    return script.depth_sup_source(o)

  assert source('--dataset', 'synthetic', '--synth_scene', 'planes') == 'planes'
  assert source('--dataset', 'synthetic', '--synth_scene', 'planes_batched') == 'planes'
  assert source('--dataset', 'kitti', '--kitti_dl_disparities_px', 'true') == 'px'
  assert source('--dataset', 'kitti', '--kitti_dl_velodyne', 'true') == 'velodyne'
  for argv in (('--dataset', 'synthetic'),
               ('--dataset', 'kitti'),
               ('--dataset', 'kitti', '--kitti_procedural', 'true',
                '--kitti_dl_velodyne', 'true'),
               ('--dataset', 'kitti', '--kitti_dl_velodyne', 'true',
                '--kitti_dl_disparities_px', 'true')):
    with pytest.raises(ValueError) as e:
      source(*argv)
    for name in ('planes', '--kitti_dl_disparities_px', '--kitti_dl_velodyne'):
      assert name in str(e.value), argv
  # the trainer refuses such a configuration before it builds a loader
  o = script.apply_dataset_overrides(script.build_parser().parse_args(
      ['--depth_sup_wt', '1', '--dataset', 'synthetic', '--cpu', 'true']))
  tr = script.Trainer.__new__(script.Trainer)
  tr.opts = o
  with pytest.raises(ValueError, match='--kitti_dl_velodyne'):
    tr.define_data_loader()


def test_staging_of_the_kitti_ground_truth():
  """feed() picks the loader outputs by source, stage() forms [gt_src; gt_trg] and
  gt_scale = 1 / (f_x |t_x|) as Evaluator.eval_depth does (no device needed for
  the disparity maps)."""
  sys.path.insert(0, PKG)
  import ldi_enc_dec as script
  o = script.apply_dataset_overrides(script.build_parser().parse_args(
      ['--depth_sup_wt', '1', '--dataset', 'kitti', '--kitti_dl_disparities_px', 'true']))
  tr = script.Trainer.__new__(script.Trainer)
  tr.opts, tr.depth_sup_source = o, script.depth_sup_source(o)
  b, h, w = 2, 4, 6
  gen = torch.Generator().manual_seed(1)
  k_s = torch.tensor([[[700.0, 0, 3], [0, 700.0, 2], [0, 0, 1]]]).repeat(b, 1, 1)
  k_t = k_s.clone()
  k_t[:, 0, 0] = 721.5
  trans = torch.tensor([[[-0.54], [0.0], [0.0]]]).repeat(b, 1, 1)
  six = [torch.rand(b, h, w, 3, generator=gen), torch.rand(b, h, w, 3, generator=gen),
         k_s, k_t, torch.eye(3).repeat(b, 1, 1), trans]
  d_s, d_t = torch.rand(b, h, w, 1, generator=gen), torch.rand(b, h, w, 1, generator=gen)
  # (with --kitti_dl_disparities the batch also carries that flag's two maps)
  for batch in (six + [d_s, d_t], six + [d_s * 0, d_t * 0, d_s, d_t]):
    out = tr._depth_sup_outputs(batch)
    assert out[0] == 'px' and out[1] is d_s and out[2] is d_t
    gt2, scale2 = tr._stage_depth_sup(out, k_s, k_t, trans, lambda t: t)
    assert torch.equal(gt2, torch.cat([d_s, d_t], 0))
    t_x = trans[:, 0, 0].abs()
    assert torch.equal(scale2, torch.cat([(1.0 / (k_s[:, 0, 0] * t_x)).float(),
                                          (1.0 / (k_t[:, 0, 0] * t_x)).float()]))
  with pytest.raises(ValueError, match='planes'):
    tr._depth_sup_outputs(six)
  tr.depth_sup_source = 'planes'
  fourteen = six + [torch.zeros(1)] * 2 + [d_s, d_s * 2, d_t, d_t * 2] + [torch.zeros(1)] * 2
  out = tr._depth_sup_outputs(fourteen)
  assert out[0] == 'planes' and out[1] is d_s and out[2] is d_t
  gt2, = tr._stage_depth_sup(out, k_s, k_t, trans, lambda t: t)
  assert torch.equal(gt2, torch.cat([d_s, d_t], 0))
  tr.depth_sup_source = 'velodyne'
  nine = six + [torch.zeros(b, 8, 4), torch.zeros(b, dtype=torch.int32), torch.zeros(b, 2, 12)]
  out = tr._depth_sup_outputs(nine)
  assert out[0] == 'velodyne' and out[1] is nine[6] and out[3] is nine[8]
