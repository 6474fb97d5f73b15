"""Semi-global matching on a census cost, restated in NumPy (int64 throughout)
from the definition in DESIGN.md section 4.17: what csrc/lsi_sgm.hip is held to
bit for bit.  The loops run over the positions of a path; the other image axis
and the disparities are vectorised."""
import numpy as np

BIG = 1 << 40
COST_OUT = 62


def grey(img):
  """uint8 [..., C] -> int64 [...]."""
  img = np.asarray(img).astype(np.int64)
  if img.shape[-1] == 1:
    return img[..., 0]
  assert img.shape[-1] == 3
  return (77 * img[..., 0] + 150 * img[..., 1] + 29 * img[..., 2] + 128) >> 8


def census(g):
  """H x W grey -> H x W x 62 bits (0 / 1): neighbour < centre over the 9 x 7
  window without the centre, neighbour coordinates clamped."""
  h, w = g.shape
  pad = np.pad(g, ((3, 3), (4, 4)), mode='edge')
  bits = []
  for dy in range(-3, 4):
    for dx in range(-4, 5):
      if dy == 0 and dx == 0:
        continue
      bits.append(pad[3 + dy:3 + dy + h, 4 + dx:4 + dx + w] < g)
  return np.stack(bits, axis=-1).astype(np.int64)


def cost_volume(cen_a, cen_m, D):
  """C[y, x, d] = hamming(cen_a[y, x], cen_m[y, x - d]), 62 where x - d < 0."""
  h, w, _ = cen_a.shape
  c = np.full((h, w, D), COST_OUT, np.int64)
  for d in range(min(D, w)):
    c[:, d:, d] = (cen_a[:, d:] != cen_m[:, :w - d]).sum(-1)
  return c


def _step(prev, c, p1, p2):
  """prev, c: N x D.  One step of the recurrence."""
  m = prev.min(axis=1, keepdims=True)
  down = np.full_like(prev, BIG)
  down[:, 1:] = prev[:, :-1] + p1          # L(d - 1) + P1
  up = np.full_like(prev, BIG)
  up[:, :-1] = prev[:, 1:] + p1            # L(d + 1) + P1
  return c + np.minimum(np.minimum(prev, down), np.minimum(up, m + p2)) - m


def path_costs(c, dy, dx, p1, p2):
  """L_r over the whole image for r = (dy, dx)."""
  h, w, _ = c.shape
  L = np.empty_like(c)
  if dy == 0:
    xs = range(w) if dx > 0 else range(w - 1, -1, -1)
    for i, x in enumerate(xs):
      L[:, x] = c[:, x] if i == 0 else _step(L[:, x - dx], c[:, x], p1, p2)
    return L
  ys = range(h) if dy > 0 else range(h - 1, -1, -1)
  for i, y in enumerate(ys):
    if i == 0:
      L[y] = c[y]
      continue
    prev = L[y - dy]
    if dx == 0:
      L[y] = _step(prev, c[y], p1, p2)
    elif dx > 0:                           # the previous pixel is (y - dy, x - 1)
      L[y, 0] = c[y, 0]
      if w > 1:
        L[y, 1:] = _step(prev[:-1], c[y, 1:], p1, p2)
    else:                                  # ... (y - dy, x + 1)
      L[y, w - 1] = c[y, w - 1]
      if w > 1:
        L[y, :-1] = _step(prev[1:], c[y, :-1], p1, p2)
  return L


def directions(paths):
  dirs = [(0, 1), (0, -1), (1, 0), (-1, 0)]
  if paths == 8:
    dirs += [(1, 1), (1, -1), (-1, 1), (-1, -1)]
  return dirs


def aggregate(c, p1, p2, paths, stats=None):
  s = np.zeros_like(c)
  for dy, dx in directions(paths):
    L = path_costs(c, dy, dx, p1, p2)
    if stats is not None:
      stats['max_path_cost'] = max(stats.get('max_path_cost', 0), int(L.max()))
    s += L
  return s


def winner(s, uniq, stats=None):
  """S (H x W x D) -> (d0, acceptable, q)."""
  h, w, D = s.shape
  d0 = s.argmin(axis=2)                    # the first minimum
  best = np.take_along_axis(s, d0[..., None], 2)[..., 0]
  d = np.arange(D)[None, None, :]
  far = np.abs(d - d0[..., None]) > 1
  s2 = np.where(far, s, BIG).min(axis=2)
  ok = (100 * best <= uniq * s2) & (d0 > 0)
  inner = (d0 > 0) & (d0 < D - 1)
  sm = np.take_along_axis(s, np.clip(d0 - 1, 0, D - 1)[..., None], 2)[..., 0]
  sp = np.take_along_axis(s, np.clip(d0 + 1, 0, D - 1)[..., None], 2)[..., 0]
  den = sm - 2 * best + sp
  use = inner & (den > 0)
  num = (sm - sp) * 128
  safe = np.where(use, den, 1)
  off = np.where(use, np.sign(num) * (np.abs(num) // safe), 0)   # C's truncation
  if stats is not None:
    stats['argmin_ties'] = stats.get('argmin_ties', 0) + int(
        ((s == best[..., None]).sum(2) > 1).sum())
    # den = (sm - best) + (sp - best) and sm > best for a FIRST argmin: den = 0
    # cannot occur; the tie that does reach the division is sp == best (off = 128)
    stats['den_zero'] = stats.get('den_zero', 0) + int((inner & (den == 0)).sum())
    stats['tie_next'] = stats.get('tie_next', 0) + int((inner & (sp == best)).sum())
  return d0, ok, 256 * d0 + off


def one_view(img_a, img_m, D, p1, p2, paths, uniq, stats=None):
  """The matcher on one image (H x W x C) against the other, as a left view."""
  c = cost_volume(census(grey(img_a)), census(grey(img_m)), D)
  return winner(aggregate(c, p1, p2, paths, stats), uniq, stats)


def sgm_pair(left, right, D=128, p1=10, p2=120, paths=8, uniq=95, lr_max=1, stats=None):
  """left, right: H x W x C uint8.  Returns the two uint16 maps."""
  left, right = np.asarray(left), np.asarray(right)
  assert left.shape == right.shape and left.dtype == np.uint8 == right.dtype
  h, w = left.shape[:2]
  dl, okl, ql = one_view(left, right, D, p1, p2, paths, uniq, stats)
  # the right view: the same matcher on the mirrored, swapped pair
  dr, okr, qr = [v[:, ::-1] for v in
                 one_view(right[:, ::-1], left[:, ::-1], D, p1, p2, paths, uniq, stats)]
  keep_l, keep_r = okl.copy(), okr.copy()
  if lr_max >= 0:
    x = np.arange(w)[None, :].repeat(h, 0)
    y = np.arange(h)[:, None].repeat(w, 1)
    xr = x - dl
    inside = xr >= 0
    xr = np.clip(xr, 0, w - 1)
    keep_l &= inside & okr[y, xr] & (np.abs(dr[y, xr] - dl) <= lr_max)
    xl = x + dr
    inside = xl <= w - 1
    xl = np.clip(xl, 0, w - 1)
    keep_r &= inside & okl[y, xl] & (np.abs(dl[y, xl] - dr) <= lr_max)
  out_l = np.where(keep_l, ql, 0)
  out_r = np.where(keep_r, qr, 0)
  assert out_l.max(initial=0) < 65536 and out_r.max(initial=0) < 65536
  assert out_l.min(initial=0) >= 0 and out_r.min(initial=0) >= 0
  return out_l.astype(np.uint16), out_r.astype(np.uint16)


def sgm_batch(left, right, **kw):
  """B x H x W x C uint8 pairs -> two B x H x W uint16 arrays."""
  outs = [sgm_pair(l, r, **kw) for l, r in zip(left, right)]
  return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


# -- scenes ---------------------------------------------------------------------
def step_scene(seed, h=64, w=128, c=1):
  """White noise with the integer disparity map 3 / 11 (central block) / 7
  (lower left block); the right image is the z-buffered forward warp of the left
  (the larger disparity wins), unhit pixels fresh noise.  Returns left, right
  (H x W x C uint8), the disparity map and the mask of the left pixels whose warp
  target kept them."""
  rs = np.random.RandomState(seed)
  left = rs.randint(0, 256, (h, w, c)).astype(np.uint8)
  disp = np.full((h, w), 3, np.int64)
  disp[h // 4:3 * h // 4, w // 3:2 * w // 3] = 11
  disp[h // 2:h, 0:w // 4] = 7
  right = rs.randint(0, 256, (h, w, c)).astype(np.uint8)
  owner = np.full((h, w), -1, np.int64)    # the disparity that owns a right pixel
  for d in sorted(set(disp.ravel().tolist())):   # ascending: larger overwrites
    ys, xs = np.nonzero((disp == d))
    xt = xs - d
    ok = xt >= 0
    right[ys[ok], xt[ok]] = left[ys[ok], xs[ok]]
    owner[ys[ok], xt[ok]] = d
  ys, xs = np.indices((h, w))
  xt = xs - disp
  visible = (xt >= 0) & (owner[ys, np.clip(xt, 0, w - 1)] == disp)
  return left, right, disp, visible


def noise_pair(seed, b, h, w, c):
  """A batch of step scenes (sizes of any kind): B x H x W x C."""
  ls, rs_ = [], []
  for i in range(b):
    l, r, _, _ = step_scene(1000 * seed + i, h, w, c)
    ls.append(l)
    rs_.append(r)
  return np.stack(ls), np.stack(rs_)


def block_pair(seed, b, h, w, c):
  """Values in {0, 255} constant over 8-pixel blocks, the right image the left
  shifted by 2: long constant runs, so that ties of the argmin and den = 0
  occur."""
  rs = np.random.RandomState(seed)
  coarse = rs.randint(0, 2, (b, (h + 7) // 8, (w + 7) // 8, 1)) * 255
  left = np.repeat(np.repeat(coarse, 8, 1), 8, 2)[:, :h, :w].astype(np.uint8)
  left = np.repeat(left, c, 3)
  right = np.roll(left, -2, axis=2)
  return np.ascontiguousarray(left), np.ascontiguousarray(right)


def shift_pair(seed, b, h, w, c, shift):
  """Noise, the right image the left one shifted by `shift` columns: left pixels
  at x >= shift match at exactly that disparity."""
  rs = np.random.RandomState(seed)
  wide = rs.randint(0, 256, (b, h, w + shift, c)).astype(np.uint8)
  return np.ascontiguousarray(wide[:, :, :w]), np.ascontiguousarray(wide[:, :, shift:])
