"""The geometric-consistency loss (include/lsi_hip.h) restated
twice:

(a) in NumPy -- `loss_and_grad`: the projection (u, v, dd), the sample s, the
    scored set and sign(dd - s) are formed in fp32, operation for operation as
    the definition orders them; magnitudes, sums and the analytic gradient are
    fp64 on those fp32 values widened.  The yardstick of
    tests/test_geo_cons_gpu.py.  `loss_frozen` is the same loss in fp64
    throughout with the scored set handed in: what central differences are
    taken of.
(b) in fp32 torch ops with autograd -- `loss_and_grad_ops`: elementwise
    sequential-k products, index gathers, no library sampler; CPU or device.  It
    measures what fp32 costs on the same inputs and is the bench's context row.

D and E are P x H x W, M is P x 4 x 4; plane p's partner is plane
(p + shift) mod P of E.  The paired form: E = D, shift = P / 2, and the gradient
w.r.t. E is added to that w.r.t. D."""
import numpy as np
import torch

MODES = ('ratio', 'l1')


def project(D, M, dtype=np.float32):
  """q0, q1, n, q3, nden, u, v, dd of every pixel, each operation rounded in
  `dtype` on its own, in mrow's order."""
  D = np.asarray(D, dtype)
  M = np.asarray(M, dtype)
  p, h, w = D.shape
  half = dtype(0.5)
  px = (np.arange(w, dtype=dtype) + half)[None, None, :]
  py = (np.arange(h, dtype=dtype) + half)[None, :, None]
  m = lambda j, k: M[:, j, k][:, None, None]
  with np.errstate(all='ignore'):
    q = []
    for j in range(4):
      acc = px * m(j, 0) + py * m(j, 1)
      acc = acc + dtype(1.0) * m(j, 2)
      acc = acc + D * m(j, 3)
      q.append(acc.astype(dtype))
    n = q[2]
    nden = (n + dtype(1e-8) * (n == 0).astype(dtype)).astype(dtype)
    u, v, dd = q[0] / nden, q[1] / nden, q[3] / nden
  return q[0], q[1], n, q[3], nden, u, v, dd


def taps(u, v, h, w, dtype=np.float32):
  """taps_of and tap_weights: indices (y, x) of the four taps 00, 01, 10, 11
  (01 is x0, y1), their weights c, and the pieces the gradient needs."""
  half, one = dtype(0.5), dtype(1.0)
  with np.errstate(all='ignore'):
    x, y = u - half, v - half
    ok = np.isfinite(x) & np.isfinite(y)
    x, y = np.where(ok, x, 0).astype(dtype), np.where(ok, y, 0).astype(dtype)
    x0, y0 = np.floor(x), np.floor(y)
    x1, y1 = x0 + one, y0 + one
    xm, ym = dtype(w - 1), dtype(h - 1)
    x0s, x1s = np.clip(x0, 0, xm), np.clip(x1, 0, xm)
    y0s, y1s = np.clip(y0, 0, ym), np.clip(y1, 0, ym)
    t = dict(wx0=x1 - x, wx1=x - x0, wy0=y1 - y, wy1=y - y0,
             vx0=(x0 == x0s).astype(dtype), vx1=(x1 == x1s).astype(dtype),
             vy0=(y0 == y0s).astype(dtype), vy1=(y1 == y1s).astype(dtype))
    t['ok'] = ok
    t['idx'] = [(y0s.astype(np.int64), x0s.astype(np.int64)),
                (y1s.astype(np.int64), x0s.astype(np.int64)),
                (y0s.astype(np.int64), x1s.astype(np.int64)),
                (y1s.astype(np.int64), x1s.astype(np.int64))]
    t['c'] = [t['vx0'] * t['vy0'] * t['wx0'] * t['wy0'],
              t['vx0'] * t['vy1'] * t['wx0'] * t['wy1'],
              t['vx1'] * t['vy0'] * t['wx1'] * t['wy0'],
              t['vx1'] * t['vy1'] * t['wx1'] * t['wy1']]
  return t


def partner_planes(p, shift):
  return (np.arange(p) + shift) % p


def forward32(D, E, M, shift, occl_thresh):
  """Everything the definition forms in fp32: a dict with the projection, the
  taps, the tap values e[k], the sample s and the scored set."""
  D, E = np.asarray(D, np.float32), np.asarray(E, np.float32)
  p, h, w = D.shape
  q0, q1, n, q3, nden, u, v, dd = project(D, M)
  t = taps(u, v, h, w)
  r = partner_planes(p, shift)[:, None, None]
  ev = [E[r, iy, ix] for iy, ix in t['idx']]
  with np.errstate(all='ignore'):
    s = t['c'][0] * ev[0]
    for k in range(1, 4):
      s = s + t['c'][k] * ev[k]
    s = np.where(t['ok'], s, np.float32(0.0)).astype(np.float32)
    f = np.isfinite
    scored = (f(D) & f(u) & f(v) & f(dd) & (n > 0) & (dd > 0) &
              (u >= np.float32(0.5)) & (u <= np.float32(w) - np.float32(0.5)) &
              (v >= np.float32(0.5)) & (v <= np.float32(h) - np.float32(0.5)) &
              (s > 0))
    if occl_thresh > 0:
      scored &= ~(s - dd > np.float32(occl_thresh) * (s + dd))
    sign = np.sign(np.where(scored, dd - s, np.float32(0.0))).astype(np.float64)
  return dict(q0=q0, q1=q1, q3=q3, nden=nden, u=u, v=v, dd=dd, s=s, t=t, ev=ev,
              scored=scored, sign=sign, r=r)


def _terms(e, scored):
  """(loss, sums P x 3 = sum e, N, 0, per-pixel g = dloss/de) of per-pixel e."""
  p = scored.shape[0]
  e = np.where(scored, e, 0.0)
  n = scored.reshape(p, -1).sum(1).astype(np.float64)
  sums = np.zeros((p, 3))
  sums[:, 0], sums[:, 1] = e.reshape(p, -1).sum(1), n
  has = n > 0
  s = float(has.sum())
  if s == 0:
    return 0.0, sums, np.zeros(scored.shape)
  nn = np.where(has, n, 1.0)
  loss = float(np.where(has, sums[:, 0] / nn, 0.0).sum() / s)
  return loss, sums, np.where(scored, 1.0 / (nn * s)[:, None, None], 0.0)


def loss_and_grad(D, E, M, shift, mode='ratio', occl_thresh=0.0, upstream=1.0,
                  paired=False):
  """(loss, gradient of upstream * loss w.r.t. D, w.r.t. E, plane sums P x 3, map
  P x H x W fp32 with -1 where unscored, scored set).  paired: E is D, and the
  one gradient returned (twice) is the sum of both."""
  assert mode in MODES
  D32 = np.asarray(D, np.float32)
  p, h, w = D32.shape
  f = forward32(D, E, M, shift, occl_thresh)
  sc, t = f['scored'], f['t']
  w64 = lambda a: np.where(sc, a, 1.0).astype(np.float64)
  dd, s = w64(f['dd']), w64(f['s'])
  e = np.abs(dd - s)
  if mode == 'ratio':
    e = e / (dd + s)
  loss, sums, g = _terms(e, sc)
  emap = np.where(sc, e, -1.0).astype(np.float32)
  g = g * float(upstream)
  if mode == 'ratio':
    k = 2.0 * f['sign'] / ((dd + s) * (dd + s))
    e_dd, e_s = k * s, -k * dd
  else:
    e_dd, e_s = f['sign'], -f['sign']
  M64 = np.asarray(M, np.float32).astype(np.float64)
  m3 = lambda j: M64[:, j, 3][:, None, None]
  nden = w64(f['nden'])
  rn2 = 1.0 / (nden * nden)
  u_d = (m3(0) * nden - w64(f['q0']) * m3(2)) * rn2
  v_d = (m3(1) * nden - w64(f['q1']) * m3(2)) * rn2
  dd_d = (m3(3) * nden - w64(f['q3']) * m3(2)) * rn2
  T = {k: t[k].astype(np.float64) for k in ('wx0', 'wx1', 'wy0', 'wy1', 'vx0', 'vx1',
                                            'vy0', 'vy1')}
  with np.errstate(invalid='ignore'):
    ev = [np.where(sc, a, 0.0).astype(np.float64) for a in f['ev']]
  s_u = (T['vx1'] * (T['vy0'] * T['wy0'] * ev[2] + T['vy1'] * T['wy1'] * ev[3]) -
         T['vx0'] * (T['vy0'] * T['wy0'] * ev[0] + T['vy1'] * T['wy1'] * ev[1]))
  s_v = (T['vy1'] * (T['vx0'] * T['wx0'] * ev[1] + T['vx1'] * T['wx1'] * ev[3]) -
         T['vy0'] * (T['vx0'] * T['wx0'] * ev[0] + T['vx1'] * T['wx1'] * ev[2]))
  gD = np.where(sc, g * (e_dd * dd_d + e_s * (s_u * u_d + s_v * v_d)), 0.0)
  gE = np.zeros((p, h, w))
  r = np.broadcast_to(f['r'], sc.shape)
  for k in range(4):
    iy, ix = t['idx'][k]
    c = np.where(sc, t['c'][k].astype(np.float64), 0.0)
    np.add.at(gE, (r[sc], iy[sc], ix[sc]), (g * e_s * c)[sc])
  if paired:
    gD = gE = gD + gE
  return loss, gD, gE, sums, emap, sc


def loss_frozen(D, E, M, shift, mode, scored):
  """The loss in fp64 throughout, over the scored set handed in."""
  D, E = np.asarray(D, np.float64), np.asarray(E, np.float64)
  p, h, w = D.shape
  _, _, _, _, _, u, v, dd = project(D, np.asarray(M, np.float64), np.float64)
  t = taps(u, v, h, w, np.float64)
  r = partner_planes(p, shift)[:, None, None]
  s = sum(t['c'][k] * E[r, t['idx'][k][0], t['idx'][k][1]] for k in range(4))
  dd, s = np.where(scored, dd, 1.0), np.where(scored, s, 1.0)
  e = np.abs(dd - s)
  if mode == 'ratio':
    e = e / (dd + s)
  return _terms(e, scored)[0]


# ---------------------------------------------------------------------------
# (b) fp32 torch ops
# ---------------------------------------------------------------------------
def _project_ops(d, m, px, py):
  """mrow on flat pixels: d, px, py [N], m [N, 4, 4] -> q0, q1, n, q3."""
  q = []
  for j in range(4):
    acc = px * m[:, j, 0] + py * m[:, j, 1]
    acc = acc + 1.0 * m[:, j, 2]
    acc = acc + d * m[:, j, 3]
    q.append(acc)
  return q


def _sample_ops(Ef, base, u, v, h, w):
  """The bilinear sample of the flat partner planes Ef at (u, v): base [N] is the
  flat offset of each pixel's partner plane.  Masks and floors are constants."""
  x, y = u - 0.5, v - 0.5
  x0, y0 = torch.floor(x).detach(), torch.floor(y).detach()
  x1, y1 = x0 + 1.0, y0 + 1.0
  x0s, x1s = x0.clamp(0, w - 1), x1.clamp(0, w - 1)
  y0s, y1s = y0.clamp(0, h - 1), y1.clamp(0, h - 1)
  wx0, wx1, wy0, wy1 = x1 - x, x - x0, y1 - y, y - y0
  vx0, vx1 = (x0 == x0s).to(u.dtype), (x1 == x1s).to(u.dtype)
  vy0, vy1 = (y0 == y0s).to(u.dtype), (y1 == y1s).to(u.dtype)
  at = lambda ys, xs: Ef[base + ys.long() * w + xs.long()]
  s = vx0 * vy0 * wx0 * wy0 * at(y0s, x0s)
  s = s + vx0 * vy1 * wx0 * wy1 * at(y1s, x0s)
  s = s + vx1 * vy0 * wx1 * wy0 * at(y0s, x1s)
  s = s + vx1 * vy1 * wx1 * wy1 * at(y1s, x1s)
  return s


def loss_ops(D, E, M, shift, mode='ratio', occl_thresh=0.0, return_scored=False):
  """The same graph in torch ops of D's dtype, differentiable w.r.t. D and E.
  One pass without a graph decides which pixels are scored; the graph is then
  built over those pixels alone (index gathers), so that nothing that is not
  scored -- a NaN, an Inf -- can reach a gradient."""
  assert mode in MODES
  p, h, w = D.shape
  dev, dt = D.device, D.dtype
  ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev),
                          indexing='ij')
  plane = torch.arange(p, device=dev)[:, None, None].expand(p, h, w).reshape(-1)
  px = (xs.to(dt) + 0.5).expand(p, h, w).reshape(-1)
  py = (ys.to(dt) + 0.5).expand(p, h, w).reshape(-1)
  base = ((plane + shift) % p) * (h * w)
  Df, Ef = D.reshape(-1), E.reshape(-1)

  def run(sel):
    d, m = Df[sel], M[plane[sel]]
    q0, q1, n, q3 = _project_ops(d, m, px[sel], py[sel])
    nden = n + 1e-8 * (n == 0).to(dt)
    u, v, dd = q0 / nden, q1 / nden, q3 / nden
    fin = torch.isfinite(u) & torch.isfinite(v)
    s = _sample_ops(Ef, base[sel], torch.where(fin, u, torch.zeros_like(u)),
                    torch.where(fin, v, torch.zeros_like(v)), h, w)
    return d, n, u, v, dd, s, fin

  with torch.no_grad():
    every = torch.arange(p * h * w, device=dev)
    d, n, u, v, dd, s, fin = run(every)
    scored = (torch.isfinite(d) & fin & torch.isfinite(dd) & (n > 0) & (dd > 0) &
              (u >= 0.5) & (u <= w - 0.5) & (v >= 0.5) & (v <= h - 0.5) & (s > 0))
    if occl_thresh > 0:
      scored &= ~(s - dd > occl_thresh * (s + dd))
    sel = torch.nonzero(scored)[:, 0]
  if sel.numel() == 0:
    out = (Df * 0.0).nan_to_num().sum() + (Ef * 0.0).nan_to_num().sum()
    return (out, scored.reshape(p, h, w)) if return_scored else out
  _, _, _, _, dd, s, _ = run(sel)
  e = (dd - s).abs()
  if mode == 'ratio':
    e = e / (dd + s)
  sums = torch.zeros(p, dtype=dt, device=dev).index_add(0, plane[sel], e)
  n = torch.zeros(p, dtype=dt, device=dev).index_add(0, plane[sel], torch.ones_like(e))
  has = n > 0
  terms = torch.where(has, sums / torch.where(has, n, torch.ones_like(n)),
                      torch.zeros_like(n))
  out = terms.sum() / has.sum().to(dt)
  return (out, scored.reshape(p, h, w)) if return_scored else out


def loss_and_grad_ops(D, E, M, shift, mode='ratio', occl_thresh=0.0, upstream=1.0,
                      paired=False):
  """(loss, gradient of upstream * loss w.r.t. D, w.r.t. E) from `loss_ops` by
  autograd, as float / fp64 arrays.  paired: E is ignored, D serves as both."""
  D = D.detach().clone().requires_grad_(True)
  E = D if paired else E.detach().clone().requires_grad_(True)
  l = loss_ops(D, E, M, shift, mode, occl_thresh)
  (l * upstream).backward()
  gD = D.grad.double().cpu().numpy()
  gE = gD if paired else E.grad.double().cpu().numpy()
  return float(l.detach()), gD, gE
