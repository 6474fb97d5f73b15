"""lsi.geometry.sampling restated in NumPy, and the cases its kernels are held to.

The four operations of the reference's sampling.py:41-313 -- bilinear gather,
its compose=False form (four taps, four weights), bilinear splat, batched
scatter-add -- and their gradients in closed form, as TensorFlow differentiates
that op graph: floor, clip, equal and the `w > 1e-3` mask carry no gradient,
d wt_x0/dx = -1 and d wt_x1/dx = +1, gathered taps scatter their gradient into
the image, `init` passes its gradient through.  Nothing here calls the code
under test, the oracle or the torch restatement; tests/test_sampling_ref_cpu.py
pins this file to both of those.

Precision.  A coordinate is data of the precision it is given in (fp32 on the
device and in the oracle, fp64 in the autograd restatement), and the coordinate
stage -- x = u - 0.5, floor, x0 + 1, the two differences that are the weights --
is carried out in that precision, as the reference does.  On the lattice the
cases below use it is exact in either; at |u| = 1e9 it is not (x0 + 1 == x0 in
fp32) and the fp32 answer is the definition for fp32 coordinates.  Everything
after it (products, sums, scatters) is fp64.

A non-finite coordinate (NaN or +-Inf in x or y) samples 0, adds nothing, gets a
zero coordinate gradient and sends nothing into an image or source gradient.
The compose=False weights of such a point are not defined (NaN here).

Point and tap order: taps 00, 01, 10, 11 = (x0,y0), (x0,y1), (x1,y0), (x1,y1);
splat corners tl, tr, bl, br = (x0,y0), (x1,y0), (x0,y1), (x1,y1).
"""
import collections
import functools

import numpy as np

F64 = np.float64
TAPS = ((0, 0), (0, 1), (1, 0), (1, 1))      # (ix, iy) of the gather's taps
CORNERS = ((0, 0), (1, 0), (0, 1), (1, 1))   # (ix, iy) of the splat's corners
CLAMP = 1e-3                                  # sampling.py:218-222


class _Stage(object):
  """Per point ([B, N] each): the un-masked weights w[axis][0|1], the border
  masks v[axis][0|1], the clipped cells c[axis][0|1] (int64) and `ok`."""

  def __init__(self, coords, h, w):
    c = np.asarray(coords)
    if c.dtype != np.float32:
      c = c.astype(F64)
    dt = c.dtype.type
    b = c.shape[0]
    xy = c.reshape(b, -1, 2) - dt(0.5)
    self.ok = np.isfinite(xy).all(axis=-1)
    self.w, self.v, self.c = [], [], []
    with np.errstate(all='ignore'):
      for axis, size in ((0, w), (1, h)):
        x = xy[..., axis]
        x0 = np.floor(x)
        x1 = x0 + dt(1)
        x0s = np.minimum(np.maximum(x0, dt(0)), dt(size - 1))
        x1s = np.minimum(np.maximum(x1, dt(0)), dt(size - 1))
        wts = [(x1 - x).astype(F64), (x - x0).astype(F64)]
        val = [(x0 == x0s).astype(F64), (x1 == x1s).astype(F64)]
        # a non-finite point: no weight, no valid tap, cell 0
        self.w.append([np.where(self.ok, a, 0.0) for a in wts])
        self.v.append([np.where(self.ok, a, 0.0) for a in val])
        self.c.append([np.where(self.ok, a, 0).astype(np.int64) for a in (x0s, x1s)])
    self.width = w
    self.rows = np.arange(b)[:, None]

  def idx(self, ix, iy):
    return self.c[0][ix] + self.c[1][iy] * self.width


def _flat(a, c=None):
  a = np.asarray(a, F64)
  return a.reshape(a.shape[0], -1, a.shape[-1] if c is None else c)


# ---------------------------------------------------------------------------
# bilinear gather (sampling.py:41-123)
# ---------------------------------------------------------------------------
def bilinear(imgs, coords):
  """imgs [B,Hs,Ws,C], coords [B,Ht,Wt,2] -> [B,Ht,Wt,C] (fp64)."""
  b, hs, ws, c = imgs.shape
  s = _Stage(coords, hs, ws)
  flat = _flat(imgs)
  out = np.zeros((b, s.ok.shape[1], c))
  for ix, iy in TAPS:
    wgt = s.v[0][ix] * s.v[1][iy] * s.w[0][ix] * s.w[1][iy]
    out += wgt[..., None] * flat[s.rows, s.idx(ix, iy)]
  return out.reshape(coords.shape[:-1] + (c,))


def bilinear_grad(imgs, coords, g_out):
  """-> (g_imgs [B,Hs,Ws,C], g_coords [B,Ht,Wt,2])."""
  b, hs, ws, c = imgs.shape
  s = _Stage(coords, hs, ws)
  flat, g = _flat(imgs), _flat(g_out)
  g_imgs = np.zeros_like(flat)
  gxy = [np.zeros(s.ok.shape), np.zeros(s.ok.shape)]
  for ix, iy in TAPS:
    m = s.v[0][ix] * s.v[1][iy]
    idx = s.idx(ix, iy)
    np.add.at(g_imgs, (s.rows, idx), (m * s.w[0][ix] * s.w[1][iy])[..., None] * g)
    ga = (g * flat[s.rows, idx]).sum(-1)
    gxy[0] += (2 * ix - 1) * m * s.w[1][iy] * ga
    gxy[1] += (2 * iy - 1) * m * s.w[0][ix] * ga
  return g_imgs.reshape(imgs.shape), np.stack(gxy, -1).reshape(coords.shape)


# ---------------------------------------------------------------------------
# bilinear, compose=False (sampling.py:124-130)
# ---------------------------------------------------------------------------
def bilinear_taps(imgs, coords):
  """-> (taps [4,B,Ht,Wt,C]: border-masked, wts [4,B,Ht,Wt,1]: un-masked; NaN
  at a non-finite point)."""
  b, hs, ws, c = imgs.shape
  s = _Stage(coords, hs, ws)
  flat = _flat(imgs)
  taps, wts = [], []
  for ix, iy in TAPS:
    m = s.v[0][ix] * s.v[1][iy]
    taps.append(m[..., None] * flat[s.rows, s.idx(ix, iy)])
    wts.append(np.where(s.ok, s.w[0][ix] * s.w[1][iy], np.nan))
  lead = coords.shape[:-1]
  return (np.stack(taps).reshape((4,) + lead + (c,)),
          np.stack(wts).reshape((4,) + lead + (1,)))


def bilinear_taps_grad(img_shape, coords, g_taps=None, g_wts=None):
  """-> (g_imgs, g_coords); an absent incoming gradient counts as zero."""
  b, hs, ws, c = img_shape
  s = _Stage(coords, hs, ws)
  g_imgs = np.zeros((b, hs * ws, c))
  gxy = [np.zeros(s.ok.shape), np.zeros(s.ok.shape)]
  for k, (ix, iy) in enumerate(TAPS):
    if g_taps is not None:
      m = s.v[0][ix] * s.v[1][iy]
      gt = np.asarray(g_taps[k], F64).reshape(b, -1, c)
      np.add.at(g_imgs, (s.rows, s.idx(ix, iy)), m[..., None] * gt)
    if g_wts is not None:
      gw = np.asarray(g_wts[k], F64).reshape(b, -1)
      gxy[0] += (2 * ix - 1) * s.w[1][iy] * gw
      gxy[1] += (2 * iy - 1) * s.w[0][ix] * gw
  return g_imgs.reshape(img_shape), np.stack(gxy, -1).reshape(coords.shape)


# ---------------------------------------------------------------------------
# splat (sampling.py:171-254)
# ---------------------------------------------------------------------------
def _corner_weights(s):
  """Masked axis weights, the four clamped corner weights and their keep masks."""
  ax = [[s.w[a][i] * s.v[a][i] for i in (0, 1)] for a in (0, 1)]
  raw = [ax[0][ix] * ax[1][iy] for ix, iy in CORNERS]
  kept = [(r > CLAMP).astype(F64) for r in raw]
  return ax, [r * k for r, k in zip(raw, kept)], kept, raw


def splat(src, coords, init):
  """src [B,Hs,Ws,C] to coords [B,Hs,Ws,2] on top of init [B,Ht,Wt,C]."""
  b, ht, wt, c = init.shape
  s = _Stage(coords, ht, wt)
  _, wk, _, _ = _corner_weights(s)
  out = _flat(init).copy()
  v = _flat(src)
  for k, (ix, iy) in enumerate(CORNERS):
    np.add.at(out, (s.rows, s.idx(ix, iy)), wk[k][..., None] * v)
  return out.reshape(init.shape)


def splat_grad(src, coords, g_out):
  """-> (g_src, g_coords, g_init)."""
  b, ht, wt, c = g_out.shape
  s = _Stage(coords, ht, wt)
  ax, wk, kept, _ = _corner_weights(s)
  v, g = _flat(src), _flat(g_out)
  g_src = np.zeros_like(v)
  gxy = [np.zeros(s.ok.shape), np.zeros(s.ok.shape)]
  for k, (ix, iy) in enumerate(CORNERS):
    gk = g[s.rows, s.idx(ix, iy)]
    g_src += wk[k][..., None] * gk
    gw = kept[k] * (v * gk).sum(-1)
    gxy[0] += gw * (2 * ix - 1) * s.v[0][ix] * ax[1][iy]
    gxy[1] += gw * (2 * iy - 1) * s.v[1][iy] * ax[0][ix]
  return (g_src.reshape(src.shape), np.stack(gxy, -1).reshape(coords.shape),
          np.asarray(g_out, F64).copy())


# ---------------------------------------------------------------------------
# scatter-add (sampling.py:257-313)
# ---------------------------------------------------------------------------
def batch_scatter_add(init, idx, upd):
  """init [B,P] + the updates [B,N] added at idx [B,N]; duplicates add."""
  out = np.asarray(init, F64).copy()
  np.add.at(out, (np.arange(out.shape[0])[:, None], np.asarray(idx, np.int64)),
            np.asarray(upd, F64))
  return out


def batch_scatter_add_grad(idx, g_out):
  """-> (g_init, g_upd)."""
  g = np.asarray(g_out, F64)
  return g.copy(), g[np.arange(g.shape[0])[:, None], np.asarray(idx, np.int64)]


# ---------------------------------------------------------------------------
# What a case is made of, measured with the definitions above alone
# ---------------------------------------------------------------------------
def describe(coords, h, w):
  """Shares of the points of `coords` against an h x w image or canvas."""
  s = _Stage(coords, h, w)
  m = np.stack([s.v[0][ix] * s.v[1][iy] for ix, iy in TAPS])
  c = np.asarray(coords, F64).reshape(s.ok.shape + (2,))
  with np.errstate(all='ignore'):
    on_border = s.ok & (c == np.floor(c)).any(-1)            # a pixel's edge
    on_centre = s.ok & (c - 0.5 == np.floor(c - 0.5)).any(-1)  # where floor jumps
  _, _, kept, raw = _corner_weights(s)
  raw, kept = np.stack(raw), np.stack(kept)
  n = float(s.ok.size)
  return dict(
      points=int(s.ok.shape[1]),
      border=((m == 0).any(0) & s.ok).sum() / n,   # some tap off the image
      outside=((m == 0).all(0) & s.ok).sum() / n,  # every tap off the image
      on_border=int(on_border.sum()), on_centre=int(on_centre.sum()),
      nonfinite=int((~s.ok).sum()),
      clamped=int(((raw > 0) & (kept == 0)).sum()),
      kept_small=int(((raw > 0) & (raw < 2 * CLAMP) & (kept == 1)).sum()),
      distinct=int(len(np.unique(c[s.ok].reshape(-1, 2), axis=0))))


# ---------------------------------------------------------------------------
# The cases: integer values in [-8, 8], coordinates on the quarter lattice
# ---------------------------------------------------------------------------
# img: the sampled image of the gathers and the canvas of the splat, pts: the
# grid of points (the gathers' targets, the splat's sources).
Shape = collections.namedtuple('Shape', 'b c img pts seed kind')

SHAPES = collections.OrderedDict((s_.kind + '-b%d-c%d-%dx%d-%dx%d' % (
    (s_.b, s_.c) + s_.img + s_.pts), s_) for s_ in (
        Shape(1, 1, (1, 1), (1, 1), 1, 'lattice'),
        Shape(3, 3, (1, 1), (1, 257), 2, 'lattice'),
        Shape(1, 3, (1, 7), (1, 255), 3, 'lattice'),
        Shape(3, 1, (1, 7), (19, 27), 4, 'lattice'),
        Shape(3, 5, (9, 1), (16, 16), 5, 'lattice'),
        Shape(1, 1, (9, 1), (1, 257), 6, 'lattice'),
        Shape(3, 1, (9, 13), (1, 255), 7, 'lattice'),
        Shape(1, 5, (9, 13), (16, 16), 8, 'lattice'),
        Shape(3, 3, (9, 13), (1, 257), 9, 'lattice'),
        Shape(3, 5, (9, 13), (19, 27), 10, 'lattice'),
        Shape(6, 3, (9, 13), (1, 257), 11, 'lattice'),   # the wrapper's 2 x 3
        Shape(3, 3, (9, 13), (19, 27), 12, 'hostile'),
        Shape(1, 3, (9, 13), (40, 50), 13, 'centre'),    # 2000 points, one place
        Shape(1, 3, (9, 13), (40, 50), 14, 'corner'),
        Shape(3, 3, (9, 13), (19, 27), 15, 'clamp'),
    ))
LATTICE = [k for k, s_ in SHAPES.items() if s_.kind == 'lattice']
HOSTILE = [k for k, s_ in SHAPES.items() if s_.kind == 'hostile']
COLLIDE = [k for k, s_ in SHAPES.items() if s_.kind in ('centre', 'corner')]
CLAMPED = [k for k, s_ in SHAPES.items() if s_.kind == 'clamp']
EXACT16 = LATTICE + HOSTILE + COLLIDE      # every result is a multiple of 1/16
STRIDES = 'lattice-b3-c5-9x13-19x27'       # run again with item 1 alone

HOSTILE_VALUES = (np.nan, np.inf, -np.inf, 1e9, -1e9, 3e38, -3e38)
HOSTILE_SHARE = 0.10

Case = collections.namedtuple(
    'Case', 'name shape img vals coords g_img g_vals g_taps g_wts')


def _ints(rs, *shape):
  return rs.randint(-8, 9, shape).astype(F64)


@functools.lru_cache(maxsize=None)
def case(name):
  """The operands of one case (fp64 arrays holding fp32-exact values):
    img    [B,H,W,C]      image to sample / canvas to splat onto (init)
    vals   [B,Hp,Wp,C]    the splat's source
    coords [B,Hp,Wp,2]
    g_img  [B,H,W,C]      gradient arriving at the splat's output
    g_vals [B,Hp,Wp,C]    gradient arriving at the gather's output
    g_taps [4,B,Hp,Wp,C], g_wts [4,B,Hp,Wp,1]   ... at the compose=False outputs
  Shared between tests: never written to."""
  sh = SHAPES[name]
  rs = np.random.RandomState(1000 + sh.seed)
  (h, w), (hp, wp), b, c = sh.img, sh.pts, sh.b, sh.c
  if sh.kind in ('centre', 'corner'):
    off = 0.5 if sh.kind == 'centre' else 0.0
    coords = np.empty((b, hp, wp, 2))
    coords[..., 0], coords[..., 1] = 4 + off, 3 + off
  elif sh.kind == 'clamp':
    # one axis 2^-10 (dropped) or 2^-9 (kept) away from a pixel centre, from
    # either side; the other axis on a pixel centre
    frac = np.array([2.0 ** -10, 2.0 ** -9, 1 - 2.0 ** -10, 1 - 2.0 ** -9])
    cell = np.stack([rs.randint(-1, w + 1, (b, hp, wp)),
                     rs.randint(-1, h + 1, (b, hp, wp))], -1) + 0.5
    axis = rs.randint(0, 2, (b, hp, wp))
    coords = cell + np.eye(2)[axis] * frac[rs.randint(0, 4, (b, hp, wp))][..., None]
  else:
    coords = np.stack([rs.randint(-8, 4 * (w + 2) + 1, (b, hp, wp)),
                       rs.randint(-8, 4 * (h + 2) + 1, (b, hp, wp))], -1) / 4.0
  if sh.kind == 'hostile':
    n = b * hp * wp
    pick = rs.choice(n, int(np.ceil(HOSTILE_SHARE * n)), replace=False)
    flat = coords.reshape(-1, 2)
    where = rs.randint(0, 3, len(pick))            # x, y, both
    value = np.array(HOSTILE_VALUES)[rs.randint(0, len(HOSTILE_VALUES), (len(pick), 2))]
    flat[pick[where != 1], 0] = value[where != 1, 0]
    flat[pick[where != 0], 1] = value[where != 0, 1]
  coords = coords.astype(np.float32).astype(F64)
  arrays = (_ints(rs, b, h, w, c), _ints(rs, b, hp, wp, c), coords,
            _ints(rs, b, h, w, c), _ints(rs, b, hp, wp, c),
            _ints(rs, 4, b, hp, wp, c), _ints(rs, 4, b, hp, wp, 1))
  for a in arrays:
    a.setflags(write=False)
  return Case(name, sh, *arrays)


def item(cs, i):
  """Batch item i of a case on its own (the stride check)."""
  cut = lambda a, ax: np.take(a, [i], axis=ax)
  return cs._replace(img=cut(cs.img, 0), vals=cut(cs.vals, 0),
                     coords=cut(cs.coords, 0), g_img=cut(cs.g_img, 0),
                     g_vals=cut(cs.g_vals, 0), g_taps=cut(cs.g_taps, 1),
                     g_wts=cut(cs.g_wts, 1))


def finite_points(cs):
  """[B,Hp,Wp] bool."""
  return np.isfinite(cs.coords).all(-1)


@functools.lru_cache(maxsize=None)
def expected(name, dtype='float32', only=None):
  """Every forward value and gradient of a case, from coordinates of `dtype`;
  `only`: batch item to run alone.  Shared between tests: never written to."""
  cs = case(name) if only is None else item(case(name), only)
  co = cs.coords.astype(dtype)
  r = {}
  r['bilinear'] = bilinear(cs.img, co)
  r['bilinear_g_imgs'], r['bilinear_g_coords'] = bilinear_grad(cs.img, co, cs.g_vals)
  r['taps'], r['wts'] = bilinear_taps(cs.img, co)
  for tag, gt, gw in (('t', cs.g_taps, None), ('w', None, cs.g_wts),
                      ('tw', cs.g_taps, cs.g_wts)):
    r['taps_g_imgs_' + tag], r['taps_g_coords_' + tag] = bilinear_taps_grad(
        cs.img.shape, co, gt, gw)
  r['splat'] = splat(cs.vals, co, cs.img)
  r['splat_g_src'], r['splat_g_coords'], r['splat_g_init'] = splat_grad(
      cs.vals, co, cs.g_img)
  for a in r.values():
    a.setflags(write=False)
  return r


# scatter-add: (N, P, seed, everything to one index)
ScatterShape = collections.namedtuple('ScatterShape', 'n p seed one')
SCATTER = collections.OrderedDict(
    ('n%d-p%d%s' % (s_.n, s_.p, '-one' if s_.one else ''), s_) for s_ in (
        ScatterShape(1, 1, 1, False), ScatterShape(1, 5, 2, False),
        ScatterShape(257, 1, 3, False), ScatterShape(257, 5, 4, False),
        ScatterShape(700, 1, 5, False), ScatterShape(700, 5, 6, False),
        ScatterShape(700, 5, 7, True)))
SCATTER_B = 3


@functools.lru_cache(maxsize=None)
def scatter_case(name):
  """(init [B,P], idx [B,N] int32, upd [B,N], g_out [B,P]) and the expected
  (out, g_init, g_upd)."""
  sh = SCATTER[name]
  rs = np.random.RandomState(2000 + sh.seed)
  idx = rs.randint(0, sh.p, (SCATTER_B, sh.n)).astype(np.int32)
  if sh.one:
    idx[:] = np.array([3, 0, 4], np.int32)[:, None]
  init, upd, g = (_ints(rs, SCATTER_B, sh.p), _ints(rs, SCATTER_B, sh.n),
                  _ints(rs, SCATTER_B, sh.p))
  want = (batch_scatter_add(init, idx, upd),) + batch_scatter_add_grad(idx, g)
  for a in (init, idx, upd, g) + want:
    a.setflags(write=False)
  return (init, idx, upd, g), want
