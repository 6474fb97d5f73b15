"""The fused geometric-consistency loss (csrc/lsi_geo_cons.hip) against the
restatement of its definition (tests/geo_cons_ref.py (a)).

Bars, the project's own (tests/test_depth_sup_gpu.py): every comparison first
measures the error of the fp32 op restatement (b) against (a) on the same
inputs, on the CPU, and allows the kernels max(4 x that error, the usual bar) --
2e-6 relative on a loss, 1e-5 of the largest entry on a gradient.  The scored
count per plane and where the map is -1 are compared exactly: both sides form
u, v, dd and s in fp32, operation for operation.

Poses: cameras with focal 0.9 W and a centred principal point; the first half of
a paired buffer is projected with projection.forward_projection_matrix, the
second with inverse_projection_matrix of the same pose, so the halves are true
inverses.  'rect' is the rectified baseline t = (-0.54, 0, 0), 'general' the
rotation (2, -4, 3) degrees with t = (0.3, -0.1, 0.25), 'yaw60' and 'yaw180'
look away: all planes empty.  Disparities are 0.4 k / 256 on a smooth surface
with noise.  Condition on the inputs, asserted from the restatement alone
(nothing is left out of a comparison): every non-empty case scores between 0.5
and 1.0 of its pixels, the empty cases none.  The one-pixel shape scores only
where u = v = 0.5 exactly, so its non-empty pose is the identity.

The trainer tests run at 128 x 256, the smallest size the other trainer tests
use: the U-Net refuses sizes that are not multiples of 128 (64 x 192 raises
"encoder_decoder_unet needs H and W divisible by 128")."""
import ctypes
import functools
import sys

import numpy as np
import pytest
import torch

import geo_cons_ref as ref
from conftest import PKG

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_RTOL, SLACK = 2e-6, 1e-5, 4.0
UPSTREAM = 2.5
OCCL = 0.2
EINVAL, ENULL, EWORKSPACE = -1, -2, -3

# name: P, H, W
SHAPES = {
    'a': (2, 13, 37),     # ragged rows, one block per plane
    'b': (2, 40, 150),    # several blocks per plane
    'c': (8, 9, 17),      # the training plane count
    'd': (2, 1, 1),       # one pixel
    'e': (2, 24, 72),     # 16-byte-aligned rows
    'f': (2, 13, 37),     # a's values: layer 0 of P x 3 x H x W, partner at x-stride 2
    'g': (2, 13, 37),     # a's values, the two-tensor form
}
VALUES = {'f': 'a', 'g': 'a'}
TWO_TENSORS = ('f', 'g')
EMPTY_POSES = ('yaw60', 'yaw180')
# (shape, pose, mode, occl_thresh)
RUNS = ([(n, pose, ref.MODES[(i + j) % 2], OCCL * ((i + j // 2) % 2))
         for i, n in enumerate('abcefg') for j, pose in enumerate(('rect', 'general'))] +
        [('a', 'rect', 'l1', OCCL), ('a', 'rect', 'ratio', 0.0),
         ('d', 'same', 'ratio', 0.0), ('d', 'same', 'l1', OCCL),
         ('d', 'rect', 'ratio', 0.0), ('a', 'yaw60', 'ratio', 0.0),
         ('c', 'yaw180', 'l1', OCCL), ('g', 'yaw60', 'l1', 0.0)])


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def _rotation(deg):
  rx, ry, rz = np.deg2rad(np.asarray(deg, np.float64))
  cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
  Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
  Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
  Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
  return (Rz @ Ry @ Rx).astype(np.float32)


POSES = {
    'same': ((0, 0, 0), (0, 0, 0)),
    'rect': ((0, 0, 0), (-0.54, 0, 0)),
    'general': ((2, -4, 3), (0.3, -0.1, 0.25)),
    'yaw60': ((0, 60, 0), (0, 0, 0)),
    'yaw180': ((0, 180, 0), (0, 0, 0)),
}


@functools.lru_cache(maxsize=None)
def matrices(h, w, pose):
  """(forward, inverse) 4 x 4 fp32 of the pose between two 0.9 W cameras."""
  sys.path.insert(0, PKG)
  from lsi.geometry import projection
  deg, t = POSES[pose]
  if pose == 'same':
    # exactly I (K I K^-1 in fp32 is I only to an ulp, and one pixel is scored
    # only at u = v = 0.5 exactly)
    return np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
  k = torch.tensor([[[0.9 * w, 0, w / 2.0], [0, 0.9 * w, h / 2.0], [0, 0, 1]]],
                   dtype=torch.float32)
  rot = torch.from_numpy(_rotation(deg))[None]
  t = torch.tensor(t, dtype=torch.float32).reshape(1, 3, 1)
  fwd = projection.forward_projection_matrix(k, k, rot, t)
  inv = projection.inverse_projection_matrix(k, k, rot, t)
  return fwd[0].numpy().copy(), inv[0].numpy().copy()


@functools.lru_cache(maxsize=None)
def make_inputs(name, pose):
  """(D, E or None, M, shift, patch) fp32 NumPy; E None: the paired form.  D and E
  are 0.4 k / 256 on a smooth surface.  Planted per plane of 100 pixels or more,
  at distinct pixels: d = 0, NaN and negative in D and -- in the two-tensor form --
  a NaN and a 0 in E (in the paired form D's own are the partner's); and, in the
  first view's planes, a 3 x 3 patch of D at a third of its disparity: its partner
  is 3 x nearer."""
  two = name in TWO_TENSORS
  name = VALUES.get(name, name)
  p, h, w = SHAPES[name]
  rng = np.random.RandomState(sum(map(ord, name)) + 13)
  yy, xx = np.mgrid[0:h, 0:w]

  def surface(n):
    k = np.stack([150 + 25 * np.sin(0.2 * xx + 0.5 * i) + 20 * np.cos(0.3 * yy) +
                  rng.randint(-6, 7, (h, w)) for i in range(n)])
    return (0.4 * np.round(k) / 256).astype(np.float32)

  D = surface(p)
  E = surface(p) if two else None
  fwd, inv = matrices(h, w, pose)
  if two:
    M, shift = np.stack([fwd] * p), 0
  else:
    M, shift = np.stack([fwd] * (p // 2) + [inv] * (p // 2)), p // 2
  patch = np.zeros((p, h, w), bool)
  if h * w >= 100:
    for pl in range(p):
      idx = rng.permutation(h * w)
      D[pl].flat[idx[:3]] = (0.0, np.nan, -0.25)
      if two:
        E[pl].flat[idx[3:5]] = (np.nan, 0.0)
      if two or pl < p // 2:      # (not where a paired partner's patch would land)
        y0, x0 = h // 2 - 1, w // 2 - 1
        patch[pl, y0:y0 + 3, x0:x0 + 3] = True
    D = np.where(patch, (0.4 * np.floor(D * 640 / 3) / 256).astype(np.float32), D)
  return D, E, M.astype(np.float32), shift, patch


@functools.lru_cache(maxsize=None)
def case_reference(name, pose, mode, occl):
  """Reference of a run, computed once and shared (read-only): restatement (a)
  with the gradient of loss * UPSTREAM, and (b)'s own errors against it."""
  D, E, M, shift, patch = make_inputs(name, pose)
  paired = E is None
  l, gD, gE, sums, emap, sc = ref.loss_and_grad(D, D if paired else E, M, shift, mode,
                                                occl, UPSTREAM, paired=paired)
  t = torch.from_numpy
  l32, g32, e32 = ref.loss_and_grad_ops(t(D), t(D if paired else E), t(M), shift, mode,
                                        occl, UPSTREAM, paired=paired)
  gmax = max(np.abs(gD).max(), np.abs(gE).max())
  gerr = max(np.abs(g32 - gD).max(), np.abs(e32 - gE).max())
  return {'loss': l, 'gD': gD, 'gE': gE, 'sums': sums, 'map': emap, 'scored': sc,
          'gmax': gmax, 'patch': patch,
          'loss_err32': abs(l32 - l) / abs(l) if l else abs(l32),
          'grad_err32': float(gerr / gmax) if gmax else float(gerr)}


def same(a, b):
  """torch.equal with NaN equal to NaN (the inputs hold planted NaNs)."""
  return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def on_device(name, pose, dev):
  """The inputs on the device in the layout the shape asks for."""
  D, E, M, shift, _ = make_inputs(name, pose)
  D, M = torch.from_numpy(D).to(dev), torch.from_numpy(M).to(dev)
  E = None if E is None else torch.from_numpy(E).to(dev)
  p, h, w = D.shape
  if name == 'f':
    # layer 0 of a P x L x H x W buffer (L = 3): the planes lie apart; the
    # partner at x-stride 2 in rows of 2 W + 2: its rows do not follow one another
    buf = torch.full((p, 3, h, w), 7.0, device=dev)
    buf[:, 0] = D
    dview = buf[:, 0]
    wide = torch.full((p, h, 2 * w + 2), 7.0, device=dev)
    wide[:, :, :2 * w:2] = E
    eview = wide[:, :, :2 * w:2]
    assert dview.stride() == (3 * h * w, w, 1)
    assert eview.stride() == (h * (2 * w + 2), 2 * w + 2, 2)
    assert same(dview, D) and same(eview, E) and not dview.is_contiguous()
    D, E = dview, eview
  return D, E, M


def kernel(D, E, M, mode, occl):
  """(loss, gradient of loss * UPSTREAM w.r.t. D, w.r.t. E or None, plane sums,
  map) from the HIP kernels; D and E may be device views."""
  from lsi.loss import _hip
  x = D.detach().requires_grad_(True)
  y = None if E is None else E.detach().requires_grad_(True)
  l, emap, sums = _hip.geometric_consistency_loss(x, y, M, mode, occl, return_map=True,
                                                  return_plane_sums=True)
  g = torch.autograd.grad(l * UPSTREAM, [x] if y is None else [x, y])
  return l.detach(), g[0], (None if y is None else g[1]), sums, emap


def check(tag, l, gD, gE, r):
  """Prints the measured errors, then holds them against the bars."""
  l = float(l)
  loss_err = abs(l - r['loss']) / abs(r['loss']) if r['loss'] else abs(l)
  gerr = np.abs(gD.cpu().double().numpy() - r['gD']).max()
  if gE is not None:
    gerr = max(gerr, np.abs(gE.cpu().double().numpy() - r['gE']).max())
  grad_err = float(gerr / r['gmax']) if r['gmax'] else float(gerr)
  loss_bar = max(SLACK * r['loss_err32'], LOSS_RTOL)
  grad_bar = max(SLACK * r['grad_err32'], GRAD_RTOL)
  print('geo_cons %s: loss %.9g err kernel %.3g restatement %.3g bar %.3g | grad err '
        'kernel %.3g restatement %.3g bar %.3g' %
        (tag, l, loss_err, r['loss_err32'], loss_bar, grad_err, r['grad_err32'],
         grad_bar))
  assert loss_err <= loss_bar, (tag, loss_err, loss_bar)
  assert grad_err <= grad_bar, (tag, grad_err, grad_bar)


def test_the_inputs_hold_what_they_should():
  for name, pose, mode, occl in RUNS:
    r = case_reference(name, pose, mode, occl)
    D, E, M, shift, patch = make_inputs(name, pose)
    sc = r['scored']
    frac = sc.mean()
    print('geo_cons inputs %s %s %s occl %g: scored %.3f' % (name, pose, mode, occl, frac))
    if pose in EMPTY_POSES or (name == 'd' and pose == 'rect'):
      assert not sc.any() and r['loss'] == 0.0
      continue
    assert 0.5 <= frac <= 1.0, (name, pose, frac)
    assert (r['sums'][:, 1] > 0).all()
    if name == 'd':
      assert sc.all()
      continue
    for pl in range(D.shape[0]):
      with np.errstate(invalid='ignore'):
        assert (D[pl] == 0).any() and np.isnan(D[pl]).any() and (D[pl] < 0).any()
        if E is not None:
          assert (E[pl] == 0).any() and np.isnan(E[pl]).any()
    with np.errstate(invalid='ignore'):
      assert not sc[~(D > 0)].any()
    # the patch: its partner is about 3 x nearer -- scored without the rule, not
    # scored under it
    without = case_reference(name, pose, mode, 0.0)['scored']
    assert (without & patch).sum() >= patch.sum() // 2
    if occl > 0:
      # (a patch pixel that lands next to a planted 0 of the partner samples less)
      assert (without & ~sc & patch).sum() >= patch.sum() // 2


@pytest.mark.parametrize('name,pose,mode,occl', RUNS)
def test_forward_and_gradient(name, pose, mode, occl, dev):
  r = case_reference(name, pose, mode, occl)
  D, E, M = on_device(name, pose, dev)
  l, gD, gE, sums, emap = kernel(D, E, M, mode, occl)
  assert gD.shape == D.shape and gD.is_contiguous()
  assert (gE is None) == (E is None)
  assert bool(torch.isfinite(gD).all()) and bool(torch.isfinite(l))
  assert gE is None or bool(torch.isfinite(gE).all())
  assert bool(torch.isfinite(sums).all())
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
    assert float(l) == 0.0 and not gD.cpu().numpy().any()
    assert gE is None or not gE.cpu().numpy().any()
  # a gradient entry is exactly 0 where the restatement's is
  got = gD.cpu().numpy()
  assert not got[r['gD'] == 0].any()
  if gE is not None:
    assert not gE.cpu().numpy()[r['gE'] == 0].any()
  check('%s %s %s occl %g' % (name, pose, mode, occl), l, gD, gE, r)


@pytest.mark.parametrize('mode', ref.MODES)
def test_strided_inputs_give_the_same_bits(mode, dev):
  D, E, M = on_device('f', 'general', dev)
  want = kernel(D.contiguous(), E.contiguous(), M, mode, OCCL)
  got = kernel(D, E, M, mode, OCCL)
  for k in (0, 3, 4):                 # loss, plane sums, map
    assert torch.equal(got[k], want[k])
  # layer 0 of the trainer's paired buffer: L x 2 B x H x W x 1 in a packed buffer
  D, _, M = on_device('a', 'rect', dev)
  p, h, w = D.shape
  rgbd = torch.full((p, h, w, 2, 4), 7.0, device=dev)
  rgbd[:, :, :, 0, 3] = D
  view = rgbd.permute(3, 0, 1, 2, 4)[0, ..., 3]
  assert view.stride() == (h * w * 8, w * 8, 8) and same(view, D)
  want = kernel(D, None, M, mode, 0.0)
  got = kernel(view, None, M, mode, 0.0)
  for k in (0, 3, 4):
    assert torch.equal(got[k], want[k])


def test_identity_with_equal_halves_is_exactly_zero(dev):
  D = make_inputs('b', 'rect')[0].copy()
  D[1] = D[0]
  M = torch.eye(4, device=dev).repeat(2, 1, 1)
  # not scored: the three planted pixels of a plane and the neighbours whose
  # zero-weight tap is the planted NaN (0 * NaN is NaN, as in lsi_bilinear_fwd)
  sc = ref.loss_and_grad(D, D, M.cpu().numpy(), 1, 'l1', OCCL, paired=True)[5]
  assert 40 * 150 - 7 <= sc[0].sum() <= 40 * 150 - 3 and np.array_equal(sc[0], sc[1])
  D = torch.from_numpy(D).to(dev)
  for mode in ref.MODES:
    l, g, _, sums, emap = kernel(D, None, M, mode, OCCL)
    sums = sums.cpu().numpy().reshape(-1, 3)
    assert float(l) == 0.0 and not g.cpu().numpy().any()
    assert (sums[:, 1] == sc[0].sum()).all() and not sums[:, 0].any()
    emap = emap.cpu().numpy()
    assert np.array_equal(emap == -1, ~sc) and not emap[sc].any()


def test_quarter_pixel_lattice_is_exact(dev):
  """M = I with M[0][3] = 8, d and E multiples of 1/32 up to 2: u lies on the
  quarter-pixel lattice, the weights are multiples of 1/4, every e a multiple of
  2^-9 below 2: in l1 mode nothing rounds, in any order."""
  p, h, w = 2, 13, 37
  rng = np.random.RandomState(3)
  D = (rng.randint(1, 65, (p, h, w)) / 32.0).astype(np.float32)
  M = np.tile(np.eye(4, dtype=np.float32), (p, 1, 1))
  M[:, 0, 3] = 8.0
  l, gD, _, sums, emap, sc = ref.loss_and_grad(D, D, M, 1, 'l1', paired=True)
  assert 0.1 * sc.size < sc.sum() < sc.size
  # the lattice: the restatement's sums are the same in fp32 and in fp64
  e = np.where(sc, emap, np.float32(0.0))
  s32 = np.array([np.cumsum(e[i].ravel(), dtype=np.float32)[-1] for i in range(p)])
  assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), sums[:, 0])
  assert np.array_equal(e * 512, np.round(e * 512))
  t = lambda a: torch.from_numpy(a).to(dev)
  lk, g, _, ksums, kmap = kernel(t(D), None, t(M), 'l1', 0.0)
  assert np.array_equal(ksums.cpu().numpy().reshape(-1, 3), sums)
  assert np.array_equal(kmap.cpu().numpy(), emap)
  assert float(lk) == float(np.float32(l))


@pytest.mark.parametrize('mode', ref.MODES)
def test_forward_is_reproducible(mode, dev):
  D, E, M = on_device('b', 'general', dev)
  runs = [kernel(D, E, M, mode, OCCL) for _ in range(2)]
  for k in (0, 3, 4):                 # loss, plane sums, map: bit for bit
    assert torch.equal(runs[0][k], runs[1][k])
  # the backward adds with atomics: held to the gradient's bar
  r = case_reference('b', 'general', mode, OCCL)
  for run in runs:
    check('b general %s again' % mode, run[0], run[1], run[2], r)


def test_public_wrapper(dev):
  from lsi.loss import loss
  D, _, M = on_device('a', 'general', dev)
  for mode in ref.MODES:
    want, g_want, _, _, map_want = kernel(D, None, M, mode, OCCL)
    # [..., H, W, 1] with two leading dimensions: 1 x 2 planes
    x = D[None, ..., None].clone().requires_grad_(True)
    got, emap = loss.geometric_consistency_loss(x, M, mode=mode, occl_thresh=OCCL,
                                                return_map=True)
    assert torch.equal(got.detach(), want) and torch.equal(emap, map_want)
    assert not emap.requires_grad
    (got * UPSTREAM).backward()
    assert x.grad.shape == x.shape
    r = case_reference('a', 'general', mode, OCCL)
    check('a general %s wrapper' % mode, got.detach(), x.grad[0, ..., 0], None, r)
  # the defaults: ratio, no occlusion rule, no map
  got = loss.geometric_consistency_loss(D, M)
  assert torch.equal(got, kernel(D, None, M, 'ratio', 0.0)[0])
  # the two-tensor form
  D, E, M = on_device('g', 'rect', dev)
  got = loss.geometric_consistency_loss(D, M, partner_disps=E, mode='l1')
  assert torch.equal(got, kernel(D, E, M, 'l1', 0.0)[0])


def test_refusals_come_in_order_and_launch_nothing(dev):
  from lsi import _C
  from lsi.loss import _hip
  lib = _C.lib()
  D, E, M = on_device('g', 'rect', dev)
  d = _hip.geo_cons_desc(D, E, M, 'ratio', 0.0, 't')
  n = int(lib.lsi_geo_cons_workspace_bytes(ctypes.byref(d)))
  assert n == (3 * 2 * 1 + 2) * 8
  out = torch.full((), -7.0, device=dev)
  sums = torch.full((6,), -7.0, dtype=torch.float64, device=dev)
  ws = torch.full((n // 8,), -7.0, dtype=torch.float64, device=dev)
  emap = torch.full(D.shape, -7.0, device=dev)
  g_loss = torch.full((), UPSTREAM, device=dev)
  g_d = torch.full(D.shape, -7.0, device=dev)
  g_e = torch.full(D.shape, -7.0, device=dev)
  ptr = _C.ptr

  def fwd(desc, p=D, e=E, m=M, o=out, s=sums, w=ws, nbytes=n):
    return lib.lsi_geo_cons_loss_fwd(ctypes.byref(desc), ptr(p), ptr(e), ptr(m), ptr(o),
                                     ptr(s), ptr(emap), ptr(w), nbytes, None)

  def bwd(desc, p=D, e=E, m=M, s=sums, gl=g_loss, gd=g_d):
    return lib.lsi_geo_cons_loss_bwd(ctypes.byref(desc), ptr(p), ptr(e), ptr(m), ptr(s),
                                     ptr(gl), ptr(gd), ptr(g_e), None)

  def bad(**kw):
    b = _hip.geo_cons_desc(D, E, M, 'ratio', 0.0, 't')
    for k, v in kw.items():
      setattr(b, k, v)
    return b

  for kw in (dict(mode=2), dict(P=0), dict(H=-1), dict(P=65536), dict(H=4096, W=4096),
             dict(shift=2), dict(shift=-1), dict(occl_thresh=1.0),
             dict(occl_thresh=float('nan'))):
    b = bad(**kw)
    assert lib.lsi_geo_cons_workspace_bytes(ctypes.byref(b)) == 0, kw
    # a bad descriptor first: before the NULL pointer and the short workspace
    assert fwd(b, p=None, nbytes=0) == EINVAL and bwd(b, p=None) == EINVAL, kw
  # then a NULL pointer, before the short workspace
  for null in ('p', 'e', 'm', 'o', 's', 'w'):
    assert fwd(d, **{null: None}, nbytes=0) == ENULL, null
  for null in ('p', 'e', 'm', 's', 'gl', 'gd'):
    assert bwd(d, **{null: None}) == ENULL, null
  # then the workspace
  assert fwd(d, nbytes=n - 1) == EWORKSPACE
  torch.cuda.synchronize()
  # nothing was launched, nothing zero-filled: no output was touched
  for t in (out, sums, ws, emap, g_d, g_e):
    assert bool((t == -7.0).all())
  # ... and the same arguments, complete, run
  assert fwd(d) == 0 and bwd(d) == 0
  torch.cuda.synchronize()
  assert bool(torch.isfinite(g_d).all()) and bool(torch.isfinite(g_e).all())
  assert float(out) > 0 and float(g_d.abs().sum()) > 0 and float(g_e.abs().sum()) > 0


def test_capture_in_a_graph_and_replay_on_new_values(dev):
  """Forward and backward at shape a, recorded in one graph on one stream, then
  replayed on other values: the loss bit for bit what the eager call gives, the
  gradient (atomics) to its bar."""
  from lsi.loss import _hip
  first = on_device('a', 'general', dev)
  other = on_device('a', 'rect', dev)        # other values and other cameras
  for mode in ref.MODES:
    d_s = first[0].clone().requires_grad_(True)
    m_s = first[2].clone()

    def step():
      l = _hip.geometric_consistency_loss(d_s, None, m_s, mode, OCCL)
      g, = torch.autograd.grad(l * UPSTREAM, d_s)
      return l, g

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      step()                                  # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
      l_s, g_s = step()
    with torch.no_grad():
      d_s.copy_(other[0])
      m_s.copy_(other[2])
    graph.replay()
    torch.cuda.synchronize()
    l, g, _, _, _ = kernel(other[0], None, other[2], mode, OCCL)
    assert torch.equal(l_s, l)
    check('a rect %s replayed' % mode, l_s, g_s, None,
          case_reference('a', 'rect', mode, OCCL))
    assert not torch.equal(g, kernel(first[0], None, first[2], mode, OCCL)[1])


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


@pytest.mark.parametrize('paired,mode', [('true', 'ratio'), ('false', 'l1')])
def test_ten_training_steps_with_the_term(paired, mode, tmp_path, dev):
  from lsi.loss import _hip, loss
  tr = _trainer(tmp_path, '--geo_cons_wt', '0.5', '--geo_cons_mode', mode,
                '--geo_cons_occl', '0.2', '--paired_splat', paired)
  o = tr.opts
  before = dict(_hip.CALLS)
  staged, _ = tr.stage(tr.feed())
  total, scalars = tr.compute_losses(staged)
  assert set(scalars) == SIX | {'geo_cons_loss'}
  n_calls = 1 if paired == 'true' else 2
  assert _hip.CALLS['geo_cons_fwd'] - before['geo_cons_fwd'] == n_calls
  # the term again, through the public function on the network's own buffer
  pair = tr.model.pair_ldi
  b = o.batch_size
  assert pair is not None and pair[2].shape == (2, 2 * b, 128, 256, 1)
  mat_trg, mat_src = staged[2], staged[3]
  kw = dict(mode=mode, occl_thresh=0.2)
  with torch.no_grad():
    if paired == 'true':
      again, emap = loss.geometric_consistency_loss(
          pair[2][0], torch.cat([mat_trg, mat_src]), return_map=True, **kw)
      again = 2.0 * again
    else:
      l_s, emap = loss.geometric_consistency_loss(
          pair[2][0, :b], mat_trg, partner_disps=pair[2][0, b:], return_map=True, **kw)
      again = l_s + loss.geometric_consistency_loss(
          pair[2][0, b:], mat_src, partner_disps=pair[2][0, :b], **kw)
  assert torch.equal(again, scalars['geo_cons_loss'].detach())
  assert float(again) > 0 and float((emap >= 0).float().mean()) > 0.5
  wt = o.geo_cons_wt / o.max_disp if mode == 'l1' else o.geo_cons_wt
  parts = _flagless_total(o, scalars) + wt * scalars['geo_cons_loss']
  assert abs(float(total) - float(parts)) <= 1e-5 * abs(float(parts))
  # the term alone reaches the layer-0 disparities of both views, finitely
  g, = torch.autograd.grad(scalars['geo_cons_loss'], pair[2], retain_graph=True)
  assert bool(torch.isfinite(g).all())
  assert float(g[0, :b].abs().sum()) > 0 and float(g[0, b:].abs().sum()) > 0
  assert not bool(g[1].any())
  assert _hip.CALLS['geo_cons_bwd'] - before['geo_cons_bwd'] == n_calls
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
  print('geo_cons trainer paired=%s %s: total %s | term %s' %
        (paired, mode, ' '.join('%.5g' % s['total_loss'] for s in log),
         ' '.join('%.5g' % s['geo_cons_loss'] for s in log)))
  assert log[-1]['total_loss'] < log[0]['total_loss']


def test_the_term_without_the_splat_terms(tmp_path, dev):
  """With both splat weights at 0 the paired splat builds no matrices: the term
  builds its own."""
  from lsi.loss import loss
  tr = _trainer(tmp_path, '--geo_cons_wt', '0.5', '--indep_splat_wt', '0',
                '--compose_splat_wt', '0')
  staged, _ = tr.stage(tr.feed())
  total, scalars = tr.compute_losses(staged)
  pair = tr.model.pair_ldi
  with torch.no_grad():
    again = 2.0 * loss.geometric_consistency_loss(pair[2][0],
                                                  torch.cat([staged[2], staged[3]]))
  assert torch.equal(again, scalars['geo_cons_loss'].detach()) and float(again) > 0
  assert float(scalars['compose_splat_loss']) == 0.0 == float(scalars['indep_splat_loss'])
  parts = _flagless_total(tr.opts, scalars) + 0.5 * scalars['geo_cons_loss']
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
  """`--geo_cons_wt 0` against no flag at all: the same keys, the step's loss bit
  for bit, no launch of the term.  The network pass is pinned to one recorded
  output for the runs, as in tests/test_depth_sup_gpu.py: two fresh runs of the
  network do not agree bit for bit to begin with."""
  from lsi.loss import _hip
  runs = []
  pair = None
  for i, extra in enumerate(((), ('--geo_cons_wt', '0', '--geo_cons_mode', 'l1',
                                  '--geo_cons_occl', '0.3'), ())):
    tr = _trainer(tmp_path / str(i), *extra)
    assert tr.opts.geo_cons_wt == 0.0
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
    assert _hip.CALLS['geo_cons_fwd'] == before['geo_cons_fwd']
    runs.append((total.detach().clone(), [t.clone() for t in staged],
                 {k: float(torch.as_tensor(v).detach()) for k, v in scalars.items()}))
  for a, b in zip(runs[0][1], runs[1][1]):
    assert torch.equal(a, b)
  assert torch.equal(runs[0][0], runs[1][0]), (runs[0][2], runs[1][2])
  assert runs[0][2] == runs[1][2] and float(runs[0][0]) > 0
