"""The per-plane reduction of csrc/lsi_reduce.h (plane_store_partials,
plane_finish_kernel) held to exact values through both losses that use it:
lsi_edge_smooth_loss_fwd and lsi_depth_sup_loss_fwd, at the smallest shapes
that reach more than 64 planes (a second trip of the loop over the terms, five
rounds of the 16 waves), more than 64 partial sums per plane (a lane adds two)
and the cap of 256 (a lane adds four).  No tolerance, nothing left out.

Conditions on the inputs (checked below on the CPU):

* Edge-smooth runs at order 1 with alpha = 0, so every weight is expf(-0) = 1
  whatever the guide, on disparities k / 256, k in [13, 256].  Depth-sup runs in
  l1 mode without gt_scale on pred and gt that are multiples of 1/64 in
  [1/64, 1]: inside [g_min, g_max] = [1/80, 1000] and above eps; a hole is a
  ground truth of 0.  Every difference, every per-thread fp32 sum and every fp64
  sum is then exact, and the expected plane sums are integer arithmetic in
  NumPy divided once by a power of two.
* bpp, the partial sums per plane, is asserted from the workspace byte count
  (3 planes bpp + planes doubles), so a change of the grid policy fails here
  instead of quietly un-testing a branch.
* "Many planes" (65): every plane's term is dyadic with few bits, so the sum of
  the terms is exact in any order and the loss is that sum divided once and
  rounded once to fp32.  Edge-smooth un-normalised at H = W = 2: nx = H (W - 1)
  = ny = (H - 1) W = 2.  Depth-sup: a plane's count n_p of scored pixels is a
  power of two and A_p is on the lattice; plane 21 has no scored pixel,
  contributes 0 and is not counted: S = 64, not 65.
* At most two planes: the loss is the kernel's own expression on the exact
  sums in Python float64 (IEEE, as the device's), rounded once to fp32 --
  k_p (A_p / nx + B_p / ny) summed and divided by the planes, with k_p =
  1 / (S_p / N + eps) or 1; A_p / n_p summed and divided by the planes.  A sum of
  two doubles does not depend on the tree."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (puts the package on sys.path)

pytestmark = pytest.mark.gpu

G_MIN = float(np.float32(1.0) / np.float32(80.0))
G_MAX = float(np.float32(1.0) / np.float32(1e-3))
EPS = 1e-6

# name: (L, B, H, W), bpp
EDGE = {
    'many planes': ((5, 13, 2, 2), 1),
    'one past a wave': ((1, 2, 260, 256), 65),
    'at the cap': ((1, 1, 520, 512), 256),     # 260 blocks' worth: capped, a 5th pixel
}
# name: (P, H, W), bpp
DSUP = {
    'many planes': ((65, 2, 4), 1),
    'one past a wave': ((2, 65, 1024), 65),    # 1 row per block
    'at the cap': ((1, 512, 1024), 256),       # 2 rows per block
}
EMPTY = 21   # the plane of DSUP['many planes'] without a scored pixel


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def f32(x):
  return float(np.float32(x))


def bpp_of(ws_bytes, planes):
  doubles, rest = divmod(ws_bytes, 8)
  bpp, rest2 = divmod(doubles - planes, 3 * planes)
  assert rest == 0 and rest2 == 0, (ws_bytes, planes)
  return bpp


# ---------------------------------------------------------------------------
# edge-smooth
# ---------------------------------------------------------------------------
def edge_inputs(name):
  """(disp L x B x H x W x 1 fp32, the exact plane sums [planes, 3] float64)."""
  shape, _ = EDGE[name]
  k = np.random.RandomState(sum(map(ord, name))).randint(13, 257, shape).astype(np.int64)
  disp = (k / 256.0).astype(np.float32)
  assert np.array_equal(disp.astype(np.float64) * 256, k)          # on the lattice
  a = np.abs(k[..., :, :-1] - k[..., :, 1:]).sum((-1, -2))
  b = np.abs(k[..., :-1, :] - k[..., 1:, :]).sum((-1, -2))
  sums = np.stack([a, b, k.sum((-1, -2))], -1).reshape(-1, 3)
  assert sums.max() < 2 ** 53
  return torch.from_numpy(disp[..., None]), sums / 256.0


def edge_forward(disp, normalise, dev):
  """(loss, plane sums [planes, 3], bpp, the descriptor) of
  lsi_edge_smooth_loss_fwd at order 1, alpha 0."""
  from lsi import _C
  from lsi.loss import _hip
  nl, b, h, w, _ = disp.shape
  disp = disp.to(dev)
  guide = torch.zeros((b, h, w, 3), device=dev)
  d = _hip.edge_smooth_desc(disp, guide, 0.0, 1, normalise, 'test')
  n = int(_C.lib().lsi_edge_smooth_workspace_bytes(ctypes.byref(d)))
  out = torch.full((), float('nan'), device=dev)
  sums = torch.full((3 * nl * b,), float('nan'), dtype=torch.float64, device=dev)
  ws = torch.full((n // 8,), float('nan'), dtype=torch.float64, device=dev)
  rc = _C.lib().lsi_edge_smooth_loss_fwd(ctypes.byref(d), _C.ptr(disp), _C.ptr(guide),
                                         _C.ptr(out), _C.ptr(sums), _C.ptr(ws), n,
                                         _C.stream_ptr(dev))
  assert rc == 0
  return float(out), sums.cpu().numpy().reshape(-1, 3), bpp_of(n, nl * b), d


@pytest.mark.parametrize('normalise', [False, True])
@pytest.mark.parametrize('name', sorted(EDGE))
def test_edge_smooth(name, normalise, dev):
  (nl, b, h, w), bpp = EDGE[name]
  planes = nl * b
  disp, want = edge_inputs(name)
  loss, sums, got_bpp, d = edge_forward(disp, normalise, dev)
  assert got_bpp == bpp
  assert np.array_equal(sums, want)
  n, nx, ny = float(h * w), float(h * (w - 1)), float((h - 1) * w)
  if planes > 2:
    if normalise:
      return                      # the terms are not dyadic: the sums alone
    assert nx == 2.0 and ny == 2.0
    terms = want[:, 0] / nx + want[:, 1] / ny
    assert np.array_equal(terms * 512, np.round(terms * 512))       # dyadic
    assert loss == f32(float(terms.sum()) / float(planes))
    return
  t = 0.0
  for s in want.tolist():
    kp = 1.0 / (s[2] / n + float(d.eps)) if normalise else 1.0
    t += kp * (s[0] / nx + s[1] / ny)
  assert loss == f32(t / float(planes))


# ---------------------------------------------------------------------------
# depth-sup
# ---------------------------------------------------------------------------
def dsup_inputs(name):
  """(pred, gt P x H x W fp32, the exact plane sums [P, 3] float64)."""
  (p, h, w), _ = DSUP[name]
  rng = np.random.RandomState(sum(map(ord, name)) + 1)
  kp = rng.randint(1, 65, (p, h * w)).astype(np.int64)
  kg = rng.randint(1, 65, (p, h * w)).astype(np.int64)
  if name == 'many planes':
    for pl in range(p):          # 1, 2, 4 or 8 scored pixels; none in plane EMPTY
      kg[pl, (0 if pl == EMPTY else 1 << (pl % 4)):] = 0
  else:
    kg[rng.uniform(size=kg.shape) < 0.1] = 0                        # holes
  pred, gt = (kp / 64.0).astype(np.float32), (kg / 64.0).astype(np.float32)
  assert np.array_equal(pred.astype(np.float64) * 64, kp)          # on the lattice
  assert np.array_equal(gt.astype(np.float64) * 64, kg)
  ok = kg > 0
  assert pred.min() > EPS and G_MIN <= gt[ok].min() and gt.max() <= G_MAX
  sums = np.stack([ok.sum(1), np.where(ok, np.abs(kp - kg), 0).sum(1) / 64.0,
                   np.zeros(p)], -1).astype(np.float64)
  return (torch.from_numpy(pred.reshape(p, h, w)),
          torch.from_numpy(gt.reshape(p, h, w)), sums)


@pytest.mark.parametrize('name', sorted(DSUP))
def test_depth_sup(name, dev):
  from lsi import _C
  from lsi.loss import _hip
  (p, h, w), bpp = DSUP[name]
  pred, gt, want = dsup_inputs(name)
  pred, gt = pred.to(dev), gt.to(dev)
  d = _hip.depth_sup_desc(pred, gt, None, 'l1', 0.5, 0.0, G_MIN, G_MAX, EPS, 'test')
  assert bpp_of(int(_C.lib().lsi_depth_sup_workspace_bytes(ctypes.byref(d))), p) == bpp
  loss, sums = _hip.depth_supervision_loss(pred, gt, None, 'l1', 0.5, 0.0, G_MIN,
                                           G_MAX, EPS, return_plane_sums=True)
  assert np.array_equal(sums.cpu().numpy().reshape(-1, 3), want)
  n, a = want[:, 0], want[:, 1]
  if p > 2:
    scored = n > 0
    assert scored.sum() == 64 and not scored[EMPTY] and scored[64]
    assert set(n[scored].tolist()) == {1.0, 2.0, 4.0, 8.0}          # powers of two
    terms = np.where(scored, a / np.maximum(n, 1.0), 0.0)
    assert np.array_equal(terms * 512, np.round(terms * 512))       # dyadic
    assert float(loss) == f32(float(terms.sum()) / 64.0)
    return
  assert (n > 0).all()
  assert float(loss) == f32(sum(ai / ni for ai, ni in zip(a.tolist(), n.tolist())) /
                            float(p))
