"""forward_splat and its gradients restated in plain NumPy (fp64 by default),
from the formulas of oracle/lsi_torch_ref.py -- no autograd -- and the lattice
scenes on which fp32 arithmetic of the splat is exact.

TEST INFRASTRUCTURE ONLY.  tests/test_splat_lattice_cpu.py holds this file to
fp64 autograd of the op graph and proves what EXACT claims;
tests/test_splat_lattice_gpu.py holds the HIP kernels to this file.

The lattice: zbuf_scale = 0 (every z-buffer weight exp(0) = 1; a positive
bg_layer_disp gives a background weight of exactly 1), max_disp = 0.5,
textures multiples of 1/8 in [0, 1], disparities multiples of 1/64, masks
powers of two in [1/8, 2] or 0, matrix offsets multiples of 1/4, m03 in
{16, 32}, s in {0.5, 1}.  Projected coordinates are then multiples of 1/8,
bilinear weights multiples of 1/64 -- each 0 or far above the 1e-3 gate -- and
every floor / clamp decision is the same in fp32 and fp64.  The weight canvas
is a sum of such dyadic terms: exact in fp32 in ANY order.

Forward, per source pixel p = (l, b, y, x) with X = x + .5, Y = y + .5:
  q_j = m_j0 X + m_j1 Y + m_j2 + m_j3 d,  n = q_2 (+1e-8 where 0)
  u = s q_0 / n, v = s q_1 / n, dd = q_3 / n
  pw = zw(dd / max_disp) * mask,  zw(r) = exp((clip(r,0,1) - .5) zbuf) [r > 0]
  corner k in (x0,y0) (x1,y0) (x0,y1) (x1,y1): w_k = wx_a wy_b [w_k > 1e-3],
  wx_0 = (1 - fx)[x0 inside], wx_1 = fx [x0 + 1 inside], cell = clamped corner
  canvases per layer: CI = bg + sum tex pw w_k, CW = bg + sum pw w_k,
  CD = sum dd pw w_k;   a pixel whose u, v or dd is not finite adds nothing
  (the build's definition: oracle/lsi_oracle.py forward_splat).
  per layer: img = CI / CW, wts = CW, dsp = CD / CW (divide_safe);
  composed: img = sum CI / sum CW, wts = sum CW, dsp = max_l dsp_l.
Backward: the chain rule through exactly these formulas; the max over layers
splits its gradient evenly among exactly tied layers (TF's reduce_max, what
test_disp_grad_gpu.oracle_splat uses).  grads() can also evaluate the same
multilinear expression with every factor replaced by its absolute value and
every subtraction by an addition: that is A, the sum of the absolute values of
all the terms that make up an element -- the yardstick of its rounding error.
"""
import collections
import functools

import numpy as np

MAX_DISP = 0.5

Scene = collections.namedtuple(
    'Scene', 'kind tex mask disp mat s bg_layer_disp max_disp zbuf_scale')

FWD_Q = ('img', 'wts', 'dsp')
GRAD_Q = ('g_tex', 'g_mask', 'g_disp', 'g_M')

# (scene kind, mode) -> the quantities that are exact in fp32 besides `wts`,
# which is exact on every scene.  mode: 'layer' (compose_layers=False),
# 'compose', 'both' (forward_splat_both: no disparity output).  Data, proven by
# tests/test_splat_lattice_cpu.py, asserted with torch.equal on the GPU.
#   shift: per layer one constant disparity k/64 with m03 = 64, integer
#     offsets, s = 1, no mask: a source pixel lands on one cell with weight 1,
#     a cell's weight is 1 or 2, every quotient divides by a power of two.
#     Composed, its layers shift differently and a cell can weigh 3: not exact.
#   shift_compose: all layers of an item share one shift: per layer 1 or 2,
#     composed L or 2L -- a power of two, and the composed outputs exact, only
#     where L is one (exact() drops the composed claims for L = 3 and 9).
#   g_M is NOT claimed, although the fp32 op graph happens to give it exactly:
#     it sums L*H*W terms of step 2^-14 whose absolute values add up to 1e5,
#     far beyond 2^24 steps, so its bits depend on the order of the reduction.
#     It is held to the rounding bound like everywhere else.
_ALL = frozenset(('img', 'dsp', 'g_tex', 'g_mask', 'g_disp'))
EXACT = {
    ('shift', 'layer'): _ALL,
    ('shift_compose', 'layer'): _ALL,
    ('shift_compose', 'compose'): _ALL,
    ('shift_compose', 'both'): _ALL - {'dsp'},
}

KINDS = ('quarter', 'rowmix', 'anypose', 'shift', 'shift_compose', 'leaving',
         'dropped', 'crowded', 'no_background')


# Worst |g32 - g64| / (2^-24 A) of the reference op graph run in fp32 (torch,
# oracle/lsi_torch_ref.py), over backward_cases() and every mode: measured and
# pinned by tests/test_splat_lattice_cpu.py (it fails if a measured value
# exceeds its pin or falls below half of it).  The GPU bound K derives from it.
REF_RATIO = {'g_tex': 3.6, 'g_mask': 3.4, 'g_disp': 3.6, 'g_M': 9.0}

# Roundings (units of 2^-24 relative to A; a v_rcp_f32 counts 2) on the
# longest chain of the backward kernels -- tests/test_splat_lattice_gpu.py
# spells the count out.  K = min(this, 4 * REF_RATIO).
CHAIN = {'g_tex': 9, 'g_mask': 20, 'g_disp': 28, 'g_M': 44}


def bound_k(name):
  return min(float(CHAIN[name]), 4.0 * REF_RATIO[name])


SMALL_SHAPES = ((2, 2, 12, 20), (1, 1, 1, 1), (3, 1, 7, 13))
STREAM_SHAPES = ((2, 2, 8, 132), (3, 1, 18, 260), (2, 1, 6, 516), (9, 1, 6, 256),
                 (1, 1, 2, 4))
BWD_STREAM_SHAPES = ((3, 2, 24, 256), (2, 1, 10, 68))
STREAM_KINDS = ('quarter', 'rowmix', 'shift_compose', 'leaving', 'dropped',
                'crowded', 'no_background')


def scales(kind, shape):
  """The target scales a (kind, shape) is rendered at."""
  h, w = shape[2:]
  if kind in ('shift', 'shift_compose', 'anypose') or h % 2 or w % 2:
    return (1.0,)
  return (0.5, 1.0)


def small_cases():
  """(kind, shape, s, mask): the any-pose and rowband routes."""
  out = []
  for shape in SMALL_SHAPES:
    kinds = KINDS if shape == SMALL_SHAPES[0] else ('quarter', 'dropped', 'shift')
    for kind in kinds:
      for s in scales(kind, shape):
        for mask in ((False,) if kind.startswith('shift') else (True, False)):
          out.append((kind, shape, s, mask, 0))
  return out


def stream_cases():
  """(kind, shape, s, mask): what the stream path accepts (W % 4 = 0, no
  x or disparity term in rows 1 and 2)."""
  out = []
  for shape in STREAM_SHAPES:
    kinds = STREAM_KINDS if shape == STREAM_SHAPES[0] else (
        'quarter', 'shift_compose', 'dropped', 'crowded')
    for kind in kinds:
      s = scales(kind, shape)[0]
      for mask in ((False,) if kind.startswith('shift') else (False, True)):
        out.append((kind, shape, s, mask, 0))
  return out


def backward_cases():
  out = [c for c in small_cases() if c[1] == SMALL_SHAPES[0] and
         (c[3] or c[0] in ('quarter', 'shift', 'shift_compose', 'dropped'))]
  out += [c for c in small_cases() if c[1] == SMALL_SHAPES[2] and c[0] != 'shift']
  for shape in BWD_STREAM_SHAPES:
    for kind in ('quarter', 'shift_compose', 'dropped', 'leaving'):
      for mask in ((False,) if kind != 'quarter' else (False, True)):
        out.append((kind, shape, scales(kind, shape)[0], mask, 0))
  return out


def exact(sc, mode):
  """The quantities the GPU test compares with torch.equal (besides wts)."""
  nl = sc.tex.shape[0]
  if mode != 'layer' and nl & (nl - 1):
    return frozenset()
  return EXACT.get((sc.kind, mode), frozenset())


# ---------------------------------------------------------------------------
# scenes: seeded, cached, read-only
# ---------------------------------------------------------------------------
def _freeze(a):
  if a is not None:
    a.setflags(write=False)
  return a


@functools.lru_cache(maxsize=None)
def scene(kind, shape=(2, 2, 12, 20), s=1.0, mask=True, seed=0):
  """kind in KINDS; shape = (L, B, H, W).  float32 arrays, all on the lattice."""
  nl, b, h, w = shape
  rs = np.random.RandomState(1000 * KINDS.index(kind) + 7 * seed + nl + 3 * b + h * w)
  tex = rs.randint(0, 9, (nl, b, h, w, 3)) / 8.0
  disp = rs.randint(1, 33, (nl, b, h, w, 1)) / 64.0
  msk = None
  if mask and kind not in ('shift', 'shift_compose'):
    msk = 2.0 ** rs.randint(-3, 2, (nl, b, h, w, 1))
    msk[rs.rand(nl, b, h, w, 1) < 0.1] = 0.0
  mat = np.tile(np.eye(4), (b, 1, 1))
  bg = 0.25
  for i in range(b):
    m = mat[i]
    m[0, 2] = rs.randint(-8, 5) / 4.0
    m[1, 2] = rs.randint(-6, 7) / 4.0
    m[0, 3] = 16.0 if i % 2 == 0 else 32.0
  if kind == 'rowmix':
    mat[:, 0, 1] = 0.25 / s      # (x s: a multiple of 1/8 on half-integer rows)
  elif kind == 'anypose':
    for i in range(b):
      mat[i, 1, 3] = 16.0 if i % 2 == 0 else -16.0  # disparity moves rows
      mat[i, 1, 0] = 0.5 * (i % 2)
      mat[i, 2, 2] = 2.0
      mat[i, 0, 0] = mat[i, 1, 1] = 2.0             # (so u, v still span the target)
      mat[i, 0, 2] *= 2.0
      mat[i, 1, 2] *= 2.0
  elif kind in ('shift', 'shift_compose'):
    assert s == 1.0
    for i in range(b):
      mat[i, 0, 2] = float(rs.randint(-3, 2))
      mat[i, 1, 2] = float(rs.randint(-2, 3))
      mat[i, 0, 3] = 64.0
    k = rs.randint(1, 9, (nl, b))                   # per layer and item: k / 64
    if kind == 'shift_compose':
      k[:] = k[:1]
    disp = np.broadcast_to((k / 64.0)[:, :, None, None, None], (nl, b, h, w, 1)).copy()
  elif kind == 'leaving':
    # most pixels project left of the target; some land at x in (-1, 0): their
    # left corners are clamped onto column 0 with weight 0
    mat[:, 0, 2] = -(w + 2.75)
    mat[:, 0, 3] = 32.0
    mat[:, 1, 2] = -2.25
  elif kind == 'dropped':
    r = rs.rand(nl, b, h, w, 1)
    odd = (0.0, -0.25, 0.75, np.nan, np.inf, -np.inf)
    for j, val in enumerate(odd):
      disp[(r >= 0.03 * j) & (r < 0.03 * (j + 1))] = val
    if disp.size >= 12:   # (every odd value, whatever the seed and the shape)
      flat = disp.reshape(-1)
      pos = rs.permutation(flat.size)[:12]
      flat[pos] = np.array(odd + odd)
  elif kind == 'crowded':
    mat[:, 0, 0] = 0.0       # a row's pixels meet in the cells its disparities name
    mat[:, 1, 1] = 0.5       # and two source rows in one target row
    mat[:, 0, 2] = 1.25
    mat[:, 1, 2] = 0.25
    mat[:, 0, 3] = 16.0
    disp = rs.randint(4, 7, (nl, b, h, w, 1)) / 64.0
  elif kind == 'no_background':
    bg = 0.0
    mat[:, 0, 2] = -(w // 2 + 0.25)   # the right half of the target stays empty
  f32 = lambda a: _freeze(None if a is None else np.ascontiguousarray(a, np.float32))
  return Scene(kind, f32(tex), f32(msk), f32(disp), f32(mat), float(s), bg, MAX_DISP, 0.0)


def out_shapes(sc, mode):
  nl, b, h, w, c = sc.tex.shape
  ht, wt = int(h * sc.s), int(w * sc.s)
  per, one = (nl, b, ht, wt), (1, b, ht, wt)
  if mode == 'layer':
    return {'img': per + (c,), 'wts': per + (1,), 'dsp': per + (1,)}
  if mode == 'compose':
    return {'img_c': one + (c,), 'wts_c': one + (1,), 'dsp_c': one + (1,)}
  assert mode == 'both'
  return {'img': per + (c,), 'wts': per + (1,), 'img_c': one + (c,), 'wts_c': one + (1,)}


@functools.lru_cache(maxsize=None)
def upstream(sc_key, mode, only=None):
  """Upstream gradients of a loss linear in the outputs: multiples of 1/4 in
  [-1, 1], zeros included (a third of them).  sc_key: scene()'s arguments.
  only: a tuple of output names -- the others get no gradient."""
  sc = scene(*sc_key)
  rs = np.random.RandomState(len(mode) + 11 * KINDS.index(sc.kind))
  g = {}
  for name, shp in out_shapes(sc, mode).items():
    v = rs.randint(-4, 5, shp) / 4.0
    v[rs.rand(*shp) < 0.25] = 0.0
    if only is None or name in only:
      g[name] = _freeze(v.astype(np.float32))
  return g


# ---------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------
def _safe(den, dt):
  return den + dt(1e-8) * (den == 0)


def _geometry(sc, dt):
  """Per source pixel [L,B,H,W]: u, v, dd, n, zw, dzw, ok; per corner
  [L,B,H,W,4]: w, dw/du, dw/dv, flat cell index into [L*B*Ht*Wt]."""
  nl, b, h, w, _ = sc.tex.shape
  ht, wt = int(h * sc.s), int(w * sc.s)
  m = sc.mat.astype(dt)
  d = sc.disp[..., 0].astype(dt)
  X = (np.arange(w) + 0.5).astype(dt)[None, None, None, :]
  Y = (np.arange(h) + 0.5).astype(dt)[None, None, :, None]
  e = lambda j, k: m[None, :, j, k, None, None]
  with np.errstate(all='ignore'):
    q = [e(j, 0) * X + e(j, 1) * Y + e(j, 2) + e(j, 3) * d for j in range(4)]
    n = _safe(q[2], dt)
    u, v, dd = q[0] / n * dt(sc.s), q[1] / n * dt(sc.s), q[3] / n
    ok = np.isfinite(u) & np.isfinite(v) & np.isfinite(dd) & np.isfinite(d)
    u, v, dd, d = [np.where(ok, a, dt(0)) for a in (u, v, dd, d)]
    n = np.where(ok, n, dt(1))
  r = dd / dt(sc.max_disp)
  zw = np.exp((np.clip(r, 0, 1) - dt(0.5)) * dt(sc.zbuf_scale)).astype(dt) * (r > 0) * ok
  dzw = zw * dt(sc.zbuf_scale) / dt(sc.max_disp) * ((r >= 0) & (r <= 1))
  zw, dzw = zw.astype(dt), dzw.astype(dt)

  def axis(c, size):
    x = c - dt(0.5)
    x0 = np.floor(x)
    f = x - x0
    in0 = ((x0 >= 0) & (x0 <= size - 1)).astype(dt)
    in1 = ((x0 + 1 >= 0) & (x0 + 1 <= size - 1)).astype(dt)
    wgt = [(dt(1) - f) * in0, f * in1]
    dw = [-in0, in1]
    cell = [np.clip(x0, 0, size - 1).astype(np.int64),
            np.clip(x0 + 1, 0, size - 1).astype(np.int64)]
    return wgt, dw, cell

  wx, dwx, cx = axis(u, wt)
  wy, dwy, cy = axis(v, ht)
  lb = (np.arange(nl)[:, None] * b + np.arange(b)[None, :])[:, :, None, None] * (ht * wt)
  wk, du, dv, idx = [], [], [], []
  for by, ax in ((0, 0), (0, 1), (1, 0), (1, 1)):
    wgt = wx[ax] * wy[by]
    gate = ((wgt > dt(1e-3)) & ok).astype(dt)
    wk.append(wgt * gate)
    du.append(dwx[ax] * wy[by] * gate)
    dv.append(wx[ax] * dwy[by] * gate)
    idx.append(lb + cy[by] * wt + cx[ax])
  st = lambda a: np.stack(a, -1)
  return dict(u=u, v=v, dd=dd, n=n, d=d, zw=zw, dzw=dzw, ok=ok, X=X, Y=Y,
              w=st(wk), du=st(du), dv=st(dv), idx=st(idx), ht=ht, wt=wt)


def _scatter(idx, val, size, dt):
  """sum of val into cells idx: [..., 4] or [..., 4, C] -> [size] / [size, C]."""
  out = np.zeros((size,) + val.shape[idx.ndim:], dt)
  np.add.at(out, idx.reshape(-1), val.reshape((-1,) + val.shape[idx.ndim:]))
  return out


def render(sc, dtype=np.float64):
  """Everything the forward computes, per layer and composed, in `dtype`:
  img, wts, dsp [L,B,Ht,Wt,C]; img_c, wts_c, dsp_c [1,...]; the canvases; and
  per layer and cell `count`, the number of contributions of positive weight,
  and `touched`, the number of pixels with a corner there, dropped ones too."""
  dt = np.dtype(dtype).type
  nl, b, h, w, c = sc.tex.shape
  g = _geometry(sc, dt)
  ht, wt = g['ht'], g['wt']
  tex = sc.tex.astype(dt)
  mask = np.ones((nl, b, h, w), dt) if sc.mask is None else sc.mask[..., 0].astype(dt)
  pw = g['zw'] * mask
  upd = pw[..., None] * g['w']                              # [L,B,H,W,4]
  size = nl * b * ht * wt
  bgw = np.exp(dt(-0.5) * dt(sc.zbuf_scale)) * dt(sc.bg_layer_disp > 0)
  bgw = dt(bgw)
  shp = (nl, b, ht, wt)
  CW = (_scatter(g['idx'], upd, size, dt) + bgw).reshape(shp + (1,))
  CI = (_scatter(g['idx'], upd[..., None] * tex[..., None, :], size, dt) +
        bgw).reshape(shp + (c,))
  CD = _scatter(g['idx'], upd * g['dd'][..., None], size, dt).reshape(shp + (1,))
  count = _scatter(g['idx'], (upd > 0).astype(np.float64), size,
                   np.float64).reshape(shp).astype(np.int64)
  touched = _scatter(g['idx'], np.ones(upd.shape), size, np.float64).reshape(shp)
  res = dict(CI=CI, CW=CW, CD=CD, count=count, touched=touched.astype(np.int64),
             bg=bgw, geom=g, pw=pw)
  res['img'], res['wts'], res['dsp'] = CI / _safe(CW, dt), CW, CD / _safe(CW, dt)
  wc = CW.sum(0, keepdims=True)
  res['wts_c'] = wc
  res['img_c'] = CI.sum(0, keepdims=True) / _safe(wc, dt)
  res['dsp_c'] = res['dsp'].max(0, keepdims=True)
  return res


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------
def grads(sc, G, dtype=np.float64, absolute=False, fwd=None):
  """Gradients of sum_o <G[o], o> over the outputs named in G (any of img,
  wts, dsp, img_c, wts_c, dsp_c; arrays of the outputs' shapes) with respect
  to tex, mask, disp and the matrices: g_tex, g_mask, g_disp, g_M.
  absolute=True: A, the same expression over absolute values (module doc)."""
  dt = np.dtype(dtype).type
  f = fwd if fwd is not None else render(sc, dtype)
  g = f['geom']
  nl, b, h, w, c = sc.tex.shape
  ht, wt = g['ht'], g['wt']
  ab = np.abs if absolute else (lambda a: a)
  sg = dt(1) if absolute else dt(-1)
  shp = (nl, b, ht, wt)
  zero = lambda ch: np.zeros((1, 1, 1, 1, ch), dt)
  get = lambda k, ch: ab(np.asarray(G[k]).astype(dt)) if G.get(k) is not None else zero(ch)
  Gi, Gw, Gd = get('img', c), get('wts', 1), get('dsp', 1)
  Gic, Gwc, Gdc = get('img_c', c), get('wts_c', 1), get('dsp_c', 1)
  Wl, Wc = _safe(f['CW'], dt), _safe(f['wts_c'], dt)
  img, dsp, img_c = ab(f['img']), ab(f['dsp']), ab(f['img_c'])
  tie = (f['dsp'] == f['dsp_c']).astype(dt)
  share = tie / tie.sum(0, keepdims=True)
  dI = Gi / Wl + Gic / Wc
  dW = (Gw + sg * ((Gi * img).sum(-1, keepdims=True) / Wl) + sg * (Gd * dsp / Wl) +
        Gwc + sg * ((Gic * img_c).sum(-1, keepdims=True) / Wc) +
        sg * (share * Gdc * dsp / Wl))
  dD = Gd / Wl + share * Gdc / Wl
  dI = np.broadcast_to(dI, shp + (c,)).reshape(-1, c)
  dW = np.broadcast_to(dW, shp + (1,)).reshape(-1)
  dD = np.broadcast_to(dD, shp + (1,)).reshape(-1)

  idx, wk = g['idx'], g['w']
  du, dv = ab(g['du']), ab(g['dv'])
  tex = ab(sc.tex.astype(dt))
  mask = np.ones((nl, b, h, w), dt) if sc.mask is None else sc.mask[..., 0].astype(dt)
  dd, u, v = ab(g['dd']), ab(g['u']), ab(g['v'])
  pw = ab(f['pw'])
  zw = g['zw']
  gI, gW, gD = dI[idx], dW[idx], dD[idx]                   # [L,B,H,W,4(,C)]
  a = (tex[..., None, :] * gI).sum(-1) + gW + dd[..., None] * gD
  S = (wk * a).sum(-1)
  g_tex = pw[..., None] * (wk[..., None] * gI).sum(-2)
  g_mask = zw * S
  Lu = pw * (du * a).sum(-1)
  Lv = pw * (dv * a).sum(-1)
  Ld = pw * (wk * gD).sum(-1) + ab(g['dzw']) * ab(mask) * S
  n = g['n']
  s = dt(sc.s)
  Lq = [s * Lu / ab(n), s * Lv / ab(n),
        sg * ((u * Lu + v * Lv + dd * Ld) / ab(n)), Ld / ab(n)]
  ok = g['ok']
  Lq = [np.where(ok, x, dt(0)) for x in Lq]
  m = ab(sc.mat.astype(dt))
  g_disp = sum(Lq[j] * m[None, :, j, 3, None, None] for j in range(4))
  ones = np.ones((nl, b, h, w), dt)
  p = [g['X'] * ones, g['Y'] * ones, ones, ab(g['d'])]
  g_M = np.stack([np.stack([(Lq[j] * p[k]).sum((0, 2, 3)) for k in range(4)], -1)
                  for j in range(4)], -2)                  # [B,4,4]
  out = dict(g_tex=g_tex, g_disp=g_disp[..., None], g_M=g_M)
  out['g_mask'] = g_mask[..., None]
  return out


def evaluate(sc, G, dtype=np.float64):
  """(forward dict, gradients, A) for upstream gradients G."""
  f = render(sc, dtype)
  return f, grads(sc, G, dtype, fwd=f), grads(sc, G, dtype, absolute=True, fwd=f)


def lattice_step(terms):
  """The largest power of two that divides every value in `terms` (fp64)."""
  t = np.abs(np.asarray(terms, np.float64).ravel())
  t = t[t != 0]
  if t.size == 0:
    return 1.0
  for k in range(-8, 80):
    sc_ = t * 2.0 ** k
    if np.all(sc_ == np.rint(sc_)):
      return 2.0 ** -k
  raise AssertionError('not dyadic')
