"""The backward-warp photometric loss, the parts that need no
GPU: restatement (a) of tests/photo_reproj_ref.py against a 1 x 2 example worked
by hand and -- formed in fp64 -- against the fp64 autograd gradient of
restatement (b) on every run of the GPU tests, the conditions those runs' inputs
must meet (from (a) alone), the entries refuse bad arguments before any launch
and in the stated order, the workspace follows its formula, and the Python
surface exists (no CPU path, refusals, four trainer flags).

The hand example: one plane of 1 x 2 with two channels against one image
(shift 0), M = I with M[0][3] = 1, so u = x + .5 + d, v = .5, n = 1, dd = d.

    D = [1/2, 1/4]   T = [(2, 1), (5, 5)]   I = [(1, 4), (2, 0)]

    (0,0)  x' = 1/2   s = ((1 + 2) / 2, (4 + 0) / 2) = (3/2, 2)   tex - s = (1/2, -1)
    (0,1)  u = 7/4 > W - 1/2: not scored

N = 1.  l1: e = (1/2 + 1) / 2 = 3/4; dT = (1, -1) / 2; ds/du = I[x1] - I[x0] =
(1, -4), du/dd = 1, dD = -(1/2) (1 * 1 + (-1)(-4)) = -5/2.  charb: e = (sqrt(1/4 +
eps^2) + sqrt(1 + eps^2)) / 2, psi' = (1/2) / sqrt(1/4 + eps^2), -1 / sqrt(1 +
eps^2)."""
import ctypes
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

import photo_reproj_cases as cases
import photo_reproj_ref as ref

EINVAL, ENULL, EWORKSPACE = -1, -2, -3     # include/lsi_hip.h
NAN = float('nan')
HAND_T = np.array([[[[2.0, 1.0], [5.0, 5.0]]]], np.float32)
HAND_D = np.array([[[0.5, 0.25]]], np.float32)
HAND_I = np.array([[[[1.0, 4.0], [2.0, 0.0]]]], np.float32)
HAND_M = np.eye(4, dtype=np.float32)[None].copy()
HAND_M[0, 0, 3] = 1.0


def test_l1_by_hand():
  l, gT, gD, sums, emap, sc = ref.loss_and_grad(HAND_T, HAND_D, HAND_I, HAND_M)
  assert sc.tolist() == [[[True, False]]]
  assert sums.tolist() == [[0.75, 1.0, 0.0]] and l == 0.75
  assert np.array_equal(emap, np.array([[[0.75, -1.0]]], np.float32))
  assert np.array_equal(gT, np.array([[[[0.5, -0.5], [0.0, 0.0]]]]))
  assert np.array_equal(gD, np.array([[[-2.5, 0.0]]]))
  # an upstream factor scales the gradients
  _, t2, d2, _, _, _ = ref.loss_and_grad(HAND_T, HAND_D, HAND_I, HAND_M, upstream=2.5)
  assert np.array_equal(t2, 2.5 * gT) and np.array_equal(d2, 2.5 * gD)


def test_charbonnier_by_hand():
  eps = float(np.float32(0.25))
  l, gT, gD, sums, emap, sc = ref.loss_and_grad(HAND_T, HAND_D, HAND_I, HAND_M,
                                                mode='charb', eps=0.25)
  a, b = np.sqrt(0.25 + eps * eps), np.sqrt(1.0 + eps * eps)
  assert sc.tolist() == [[[True, False]]] and sums[0, 1] == 1.0
  assert abs(l - (a + b) / 2) <= 1e-15
  want = np.array([[[[0.5 / a / 2, -1.0 / b / 2], [0.0, 0.0]]]])
  assert np.abs(gT - want).max() <= 1e-15
  assert abs(gD[0, 0, 0] + 0.5 * (0.5 / a * 1.0 + (-1.0 / b) * -4.0)) <= 1e-15
  assert gD[0, 0, 1] == 0.0


def test_sign_of_zero_is_zero_and_non_finite_colours_are_not_scored():
  T, D, I, M = HAND_T.copy(), HAND_D.copy(), HAND_I.copy(), HAND_M
  T[0, 0, 0] = (1.5, 1.0)                      # channel 0 equals its sample
  l, gT, gD, _, _, sc = ref.loss_and_grad(T, D, I, M)
  assert sc[0, 0, 0] and l == 0.5
  assert gT[0, 0, 0].tolist() == [0.0, -0.5] and gD[0, 0, 0] == -2.0
  for where in ('tex', 'img'):
    T2, I2 = T.copy(), I.copy()
    if where == 'tex':
      T2[0, 0, 0, 1] = NAN
    else:
      I2[0, 0, 1, 0] = np.inf
    l, gT, gD, sums, emap, sc = ref.loss_and_grad(T2, D, I2, M)
    assert not sc.any() and l == 0.0 and not gT.any() and not gD.any()
    assert (emap == -1).all() and not sums.any()


def test_the_occlusion_rule_and_the_index_rule():
  # identity, two layers of one view: dd = d, sd = E; layer 1 lies behind
  T = np.zeros((2, 2, 4, 1), np.float32)
  I = np.ones((1, 2, 4, 1), np.float32)
  D = np.stack([np.full((2, 4), 0.25, np.float32), np.full((2, 4), 0.125, np.float32)])
  E = np.array([[[0.25, 0.3, 0.375, 0.5], [0.75, 0.2, 0.125, 0.376]]], np.float32)
  M = np.eye(4, dtype=np.float32)[None]
  _, _, _, sums, _, sc = ref.loss_and_grad(T, D, I, M, E, 0, 'l1', 0.2)
  # s - dd > t (s + dd) with t = 1/5: dd = 1/4 is hidden from s > 3/8 on, dd = 1/8
  # from s > 3/16 on
  assert sc[0].tolist() == [[True, True, True, False], [False, True, True, False]]
  assert sc[1].tolist() == [[False, False, False, False], [False, False, True, False]]
  assert sums[:, 1].tolist() == [5.0, 1.0]
  # threshold 0: no rule, the partner is not read
  _, _, _, _, _, sc = ref.loss_and_grad(T, D, I, M, None, 0, 'l1', 0.0)
  assert sc.all()
  # plane p uses matrix p mod Q and image (p mod Q + shift) mod Q
  T = np.zeros((4, 1, 1, 1), np.float32)
  D = np.full((4, 1, 1), 0.5, np.float32)
  I = np.array([3.0, 5.0], np.float32).reshape(2, 1, 1, 1)
  M = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
  M[1, 2, 2] = -1.0                             # view 1 looks away
  l, _, _, sums, emap, _ = ref.loss_and_grad(T, D, I, M, None, 1)
  assert emap.ravel().tolist() == [5.0, -1.0, 5.0, -1.0] and l == 5.0
  assert sums[:, 1].tolist() == [1.0, 0.0, 1.0, 0.0]
  l, _, _, _, emap, _ = ref.loss_and_grad(T, D, I, M, None, 0)
  assert emap.ravel().tolist() == [3.0, -1.0, 3.0, -1.0] and l == 3.0


@pytest.mark.parametrize('name,pose,mode,occl', cases.RUNS)
def test_analytic_gradient_equals_autograd_in_double(name, pose, mode, occl):
  """(a) formed in fp64 against (b) run in double, on every run of the GPU tests:
  the same scored set, the loss, and both gradients to 1e-10 of the largest
  entry.  Both take sign(0) = 0 and the one-sided tap derivative (floor has
  gradient 0)."""
  T, D, I, M, E, shift, _ = cases.make_inputs(name, pose)
  l, gT, gD, _, _, sc = ref.loss_and_grad(T, D, I, M, E, shift, mode, occl, cases.EPS,
                                          cases.UPSTREAM, dtype=np.float64)
  t = lambda a: torch.from_numpy(a).double()
  _, sc_ops = ref.loss_ops(t(T), t(D), t(I), t(M), t(E), shift, mode, occl, cases.EPS,
                           return_scored=True)
  assert np.array_equal(sc_ops.numpy(), sc)
  l_ops, t_ops, d_ops = ref.loss_and_grad_ops(t(T), t(D), t(I), t(M), t(E), shift, mode,
                                              occl, cases.EPS, cases.UPSTREAM)
  assert abs(l_ops - l) <= 1e-12 * max(abs(l), 1.0)
  assert np.isfinite(t_ops).all() and np.isfinite(d_ops).all()
  for got, want in ((t_ops, gT), (d_ops, gD)):
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print('photo_reproj %s %s %s occl %g: gradient max %.3g, (a) - autograd %.3g' %
          (name, pose, mode, occl, scale, err))
    assert err <= 1e-10 * scale
    # nothing reaches a pixel that is not scored
    unscored = ~(sc[..., None] if got.ndim == 4 else sc)
    assert not got[np.broadcast_to(unscored, got.shape)].any()


def test_the_inputs_hold_what_they_should():
  for name, pose, mode, occl in cases.RUNS:
    r = cases.case_reference(name, pose, mode, occl)
    T, D, I, M, E, shift, patch = cases.make_inputs(name, pose)
    sc = r['scored']
    frac = sc.mean()
    print('photo_reproj inputs %s %s %s occl %g: scored %.3f, (b) fp32 errors loss %.3g '
          'gT %.3g gD %.3g' % (name, pose, mode, occl, frac, r['loss_err32'],
                               r['gT_err32'], r['gD_err32']))
    if pose in cases.EMPTY_POSES or (name == 'd' and pose == 'rect'):
      assert not sc.any() and r['loss'] == 0.0
      assert not r['gT'].any() and not r['gD'].any() and not r['sums'].any()
      continue
    assert 0.5 <= frac <= 1.0, (name, pose, frac)
    assert (r['sums'][:, 1] > 0).all()
    if name == 'd':
      assert sc.all()
      continue
    c = T.shape[-1]
    for pl in range(D.shape[0]):
      with np.errstate(invalid='ignore'):
        assert (D[pl] == 0).any() and np.isnan(D[pl]).any() and (D[pl] < 0).any()
      assert np.isnan(T[pl]).sum() == 1
    for pl in range(I.shape[0]):
      assert np.isnan(I[pl]).sum() == 1
    with np.errstate(invalid='ignore'):
      assert not sc[~(D > 0)].any()
      assert not sc[np.isnan(T).any(-1)].any()
    assert patch.sum() == 9 * (I.shape[0] if name in cases.TWO_TENSORS
                               else I.shape[0] // 2)
    # the patch lies about 3 x deeper than the partner's surface: scored without
    # the rule -- every patch pixel that is not itself planted, but for those whose
    # taps touch the image's planted NaN -- and dropped, by at least half, under it
    without = cases.case_reference(name, pose, mode, 0.0)['scored']
    with np.errstate(invalid='ignore'):
      clean = patch & (D > 0) & np.isfinite(T).all(-1)
    samples = ref.forward(T, D, I, M, E, shift, 0.0)['s']
    nan_tap = ~np.all([np.isfinite(s_c) for s_c in samples], axis=0)
    assert clean.sum() >= patch.sum() - patch.sum() // 9
    assert not (clean & ~without & ~nan_tap).any()
    assert (without & patch).sum() >= (patch.sum() + 1) // 2
    if occl > 0:
      assert (without & ~sc & patch).sum() >= (patch.sum() + 1) // 2
    print('photo_reproj inputs %s %s: patch %d, scored at 0 %d, dropped at %g %s' %
          (name, pose, patch.sum(), (without & patch).sum(), occl,
           (without & ~sc & patch).sum() if occl > 0 else '-'))
    assert c == cases.SHAPES[name][4]


# ---------------------------------------------------------------------------
# the library and the Python surface
# ---------------------------------------------------------------------------
def _desc(_C, **kw):
  d = _C.LsiPhotoReprojDesc()
  d.P, d.Q, d.H, d.W, d.C, d.mode = 4, 2, 13, 37, 3, 0
  d.t_sl, d.t_sq, d.t_sy, d.t_sx, d.t_sc = 2 * 13 * 37 * 3, 13 * 37 * 3, 37 * 3, 3, 1
  d.d_sl, d.d_sq, d.d_sy, d.d_sx = 2 * 13 * 37, 13 * 37, 37, 1
  d.i_sq, d.i_sy, d.i_sx, d.i_sc = 13 * 37 * 3, 37 * 3, 3, 1
  d.e_sq, d.e_sy, d.e_sx = 13 * 37, 37, 1
  d.shift, d.occl_thresh, d.eps = 1, 0.0, 1e-3
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def test_header_binding_and_exports_agree(built_lib):
  from lsi import _C
  handle = ctypes.CDLL(built_lib)
  want = {'lsi_photo_reproj_workspace_bytes': 1, 'lsi_photo_reproj_loss_fwd': 12,
          'lsi_photo_reproj_loss_bwd': 11}
  for n, n_params in want.items():
    assert n in _C.SIGNATURES and hasattr(handle, n), n
    res, args = _C.SIGNATURES[n]
    assert len(args) == n_params, n
    assert res is (ctypes.c_size_t if n.endswith('_bytes') else ctypes.c_int)
  assert (_C.LSI_PHOTO_L1, _C.LSI_PHOTO_CHARB) == (0, 1)
  assert [f[0] for f in _C.LsiPhotoReprojDesc._fields_] == [
      'P', 'Q', 'H', 'W', 'C', 'mode', 't_sl', 't_sq', 't_sy', 't_sx', 't_sc', 'd_sl',
      'd_sq', 'd_sy', 'd_sx', 'i_sq', 'i_sy', 'i_sx', 'i_sc', 'e_sq', 'e_sy', 'e_sx',
      'shift', 'occl_thresh', 'eps', 'reserved']
  # 6 int32, 16 int64, int32, 2 float, int32 -- no padding
  assert ctypes.sizeof(_C.LsiPhotoReprojDesc) == 6 * 4 + 16 * 8 + 4 * 4
  assert _C.LsiPhotoReprojDesc.t_sl.offset == 24 and _C.LsiPhotoReprojDesc.shift.offset == 152
  from lsi.loss import loss
  assert callable(loss.photometric_reprojection_loss)


def test_argument_errors_are_reported_before_any_launch(built_lib):
  from lsi import _C
  lib = _C.lib()
  big = 1 << 30
  p = ctypes.c_void_p(16)     # never dereferenced: every call below is refused

  def calls(d, tex=p, disp=p, img=p, m=p, partner=p, a=p, b=p, g=p, nbytes=big):
    r = ctypes.byref(d) if d is not None else None
    # fwd: out_loss, plane_sums, out_map (may be NULL), workspace;
    # bwd: plane_sums, g_loss, g_tex, g_disp (either may be NULL)
    return (lib.lsi_photo_reproj_loss_fwd(r, tex, disp, img, m, partner, a, b, None, g,
                                          nbytes, None),
            lib.lsi_photo_reproj_loss_bwd(r, tex, disp, img, m, partner, a, b, g, None,
                                          None))

  assert calls(None) == (EINVAL,) * 2
  assert lib.lsi_photo_reproj_workspace_bytes(None) == 0
  for bad in (dict(mode=2), dict(mode=-1), dict(P=0), dict(Q=0), dict(H=0), dict(W=-3),
              dict(C=0), dict(C=5), dict(P=65536, Q=1), dict(P=3), dict(Q=3),
              dict(H=4096, W=4096), dict(P=200, H=4095, W=4096), dict(shift=-1),
              dict(shift=2), dict(occl_thresh=-0.1), dict(occl_thresh=1.0),
              dict(occl_thresh=NAN), dict(eps=0.0), dict(eps=-1.0), dict(eps=NAN),
              dict(eps=float('inf'))):
    d = _desc(_C, **bad)
    assert calls(d) == (EINVAL,) * 2, bad
    assert lib.lsi_photo_reproj_workspace_bytes(ctypes.byref(d)) == 0, bad
  # a bad descriptor wins over a NULL pointer, a NULL pointer over the workspace
  assert calls(_desc(_C, mode=7), tex=None, nbytes=0) == (EINVAL,) * 2
  d = _desc(_C)
  for null in ('tex', 'disp', 'img', 'm', 'a', 'b'):
    assert calls(d, **{null: None}, nbytes=0) == (ENULL,) * 2, null
  # the workspace (fwd) and a gradient to write (bwd: both NULL here)
  assert calls(d, g=None, nbytes=0) == (ENULL,) * 2
  # without a partner only at occl_thresh 0 -- where the refusal is the next one
  assert calls(_desc(_C, occl_thresh=0.2), partner=None, nbytes=0) == (ENULL,) * 2
  short = int(lib.lsi_photo_reproj_workspace_bytes(ctypes.byref(d))) - 1
  assert short > 0
  # (the backward takes no workspace: with these arguments it would launch)
  for partner in (p, None):
    assert lib.lsi_photo_reproj_loss_fwd(ctypes.byref(d), p, p, p, p, partner, p, p, None,
                                         p, short, None) == EWORKSPACE
  # the edges of the ranges are valid: the refusal is the NULL pointer's
  for edge in (dict(mode=1), dict(P=1, Q=1, H=1, W=1, shift=0), dict(P=65535, Q=1, H=1,
                                                                     W=1, shift=0),
               dict(H=1, W=(1 << 24) - 1), dict(C=1), dict(C=4), dict(shift=0),
               dict(occl_thresh=0.999), dict(eps=1e-30)):
    assert calls(_desc(_C, **edge), tex=None) == (ENULL,) * 2, edge


def test_workspace_formula(built_lib):
  from lsi import _C
  lib = _C.lib()
  # (3 P bpp + P) doubles; a block covers r = max(ceil(1024 / W), ceil(H / 256))
  # rows, bpp = ceil(H / r): lsi_reduce.h's rule, the geo-cons grid
  want = {}
  for (p, q, h, w) in ((2, 2, 1, 1), (4, 2, 13, 37), (2, 2, 40, 150), (16, 8, 9, 17),
                       (2, 2, 24, 72), (16, 8, 256, 768), (2, 1, 375, 1242),
                       (2, 2, 3000, 8)):
    r = max(-(-1024 // w), -(-h // 256))
    bpp = -(-h // r)
    want[(p, h, w)] = bpp
    for c in (1, 3, 4):
      d = _desc(_C, P=p, Q=q, H=h, W=w, C=c, shift=0)
      assert lib.lsi_photo_reproj_workspace_bytes(ctypes.byref(d)) == \
          (3 * p * bpp + p) * 8, (p, h, w)
      g = _C.LsiGeoConsDesc()
      g.P, g.H, g.W = p, h, w
      assert lib.lsi_geo_cons_workspace_bytes(ctypes.byref(g)) == (3 * p * bpp + p) * 8
  assert want[(4, 13, 37)] == 1 and want[(2, 40, 150)] == 6
  assert want[(16, 256, 768)] == 128 and want[(2, 3000, 8)] == 24


def test_no_cpu_path_and_python_side_refusals(built_lib):
  from lsi.loss import _hip, loss
  fn = loss.photometric_reprojection_loss
  tex = torch.rand(2, 4, 8, 8, 3)
  d = torch.rand(2, 4, 8, 8, 1) + 0.1
  img = torch.rand(4, 8, 8, 3)
  m = torch.eye(4).repeat(4, 1, 1)
  before = dict(_hip.CALLS)
  assert before.keys() >= {'photo_reproj_fwd', 'photo_reproj_bwd'}
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    fn(tex, d, img, m)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    fn(tex.view(8, 8, 8, 3), d[..., 0], img, m, partner_disps=d[0], shift=2,
       mode='charb', occl_thresh=0.2, eps=1e-2, return_map=True)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    _hip.photometric_reprojection_loss(tex, d[..., 0], img, m, None, 0, 'l1', 0.0, 1e-3)
  # dtype
  for kw in (dict(tex=tex.double()), dict(d=d.half()), dict(img=img.double()),
             dict(m=m.double())):
    a = dict(tex=tex, d=d, img=img, m=m)
    a.update(kw)
    with pytest.raises(RuntimeError, match='fp32'):
      fn(a['tex'], a['d'], a['img'], a['m'])
  with pytest.raises(RuntimeError, match='fp32'):
    fn(tex, d, img, m, partner_disps=d[0].double())
  # shape
  with pytest.raises(RuntimeError, match='one shape'):
    fn(tex, d[:1], img, m)
  with pytest.raises(RuntimeError, match='other_imgs are'):
    fn(tex, d, img[..., :2], m)
  with pytest.raises(RuntimeError, match='per image'):
    fn(tex, d, img, m[:2])
  with pytest.raises(RuntimeError, match='partner_disps are'):
    fn(tex, d, img, m, partner_disps=d[0, :2])
  with pytest.raises(RuntimeError, match='H, W, C'):
    fn(torch.rand(8, 3), d, img, m)
  buf = torch.rand(3, 4, 8, 8, 3)
  with pytest.raises(RuntimeError, match='without a copy'):
    fn(buf.permute(1, 0, 2, 3, 4), d, img, m)
  # the sampled views and the cameras are constants
  for kw in (dict(img=img.clone().requires_grad_(True)),
             dict(m=m.clone().requires_grad_(True))):
    a = dict(img=img, m=m)
    a.update(kw)
    with pytest.raises(RuntimeError, match='not differentiable'):
      fn(tex, d, a['img'], a['m'])
  with pytest.raises(RuntimeError, match='not differentiable'):
    fn(tex, d, img, m, partner_disps=d[0].clone().requires_grad_(True))
  # what the entries would refuse
  with pytest.raises(ValueError, match='divides'):
    fn(tex.view(8, 8, 8, 3)[:7], d.view(8, 8, 8, 1)[:7], img, m)
  with pytest.raises(ValueError, match='needs partner_disps'):
    fn(tex, d, img, m, occl_thresh=0.2)
  with pytest.raises(ValueError, match='channels'):
    fn(torch.rand(4, 8, 8, 5), d[0], torch.rand(4, 8, 8, 5), m)
  for kw in (dict(mode='l2'), dict(occl_thresh=-0.1), dict(occl_thresh=1.0),
             dict(occl_thresh=NAN), dict(shift=4), dict(shift=-1), dict(shift=0.5),
             dict(eps=0.0), dict(eps=NAN)):
    with pytest.raises(ValueError):
      fn(tex, d, img, m, partner_disps=d[0], **kw)
  assert _hip.CALLS == before


def test_descriptor_from_tensors():
  """photo_reproj_desc reads the strides of views (it touches no device): the
  network's buffer holds the L layers' RGBD side by side per pixel."""
  sys.path.insert(0, PKG)
  from lsi.loss import _hip, loss
  what = 'photometric_reprojection_loss'
  buf = torch.zeros(4, 5, 7, 2, 4)              # 2 B x H x W x L x 4
  pred = buf.permute(3, 0, 1, 2, 4)             # L x 2 B x H x W x 4
  tex = loss._layers_of_views(pred[..., :3], 4, 3, 'layer_imgs', what)
  disp = loss._layers_of_views(pred[..., 3], 4, 2, 'layer_disps', what)
  img = torch.zeros(4, 5, 14, 3)[:, :, ::2]
  m = torch.zeros(4, 4, 4)
  d = _hip.photo_reproj_desc(tex, disp, img, m, disp[0], 2, 'charb', 0.25, 1e-2, 't')
  assert (d.P, d.Q, d.H, d.W, d.C, d.mode, d.shift) == (8, 4, 5, 7, 3, 1, 2)
  assert (d.t_sl, d.t_sq, d.t_sy, d.t_sx, d.t_sc) == (4, 280, 56, 8, 1)
  assert (d.d_sl, d.d_sq, d.d_sy, d.d_sx) == (4, 280, 56, 8)
  assert (d.i_sq, d.i_sy, d.i_sx, d.i_sc) == (210, 42, 6, 1)
  assert (d.e_sq, d.e_sy, d.e_sx) == (280, 56, 8)
  assert (d.occl_thresh, abs(d.eps - 1e-2) < 1e-9) == (0.25, True)
  # flat planes split into layers of views
  t = loss._layers_of_views(torch.zeros(8, 5, 7, 3), 4, 3, 'layer_imgs', what)
  assert t.shape == (2, 4, 5, 7, 3) and t.stride() == (420, 105, 21, 3, 1)


def test_flags_and_their_defaults():
  sys.path.insert(0, PKG)
  import ldi_enc_dec
  parse = ldi_enc_dec.build_parser().parse_args
  o = parse([])
  assert (o.photo_reproj_wt, o.photo_reproj_mode, o.photo_reproj_occl,
          o.photo_reproj_what) == (0.0, 'l1', 0.2, 'texture')
  o = parse(['--photo_reproj_wt', '0.5', '--photo_reproj_mode', 'charb',
             '--photo_reproj_occl', '0', '--photo_reproj_what', 'image'])
  assert (o.photo_reproj_wt, o.photo_reproj_mode, o.photo_reproj_occl,
          o.photo_reproj_what) == (0.5, 'charb', 0.0, 'image')
  for bad in (['--photo_reproj_mode', 'huber'], ['--photo_reproj_what', 'depth'],
              ['--photo_reproj_wt', 'much']):
    with pytest.raises(SystemExit):
      parse(bad)
  text = ldi_enc_dec.build_parser().format_help()
  assert 'projected into the other view' in ' '.join(text.split())
