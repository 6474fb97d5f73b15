"""The backward-warp photometric loss (include/lsi_hip.h)
restated twice:

(a) in NumPy -- `loss_and_grad`: the projection (u, v, dd), the samples s_c, the
    partner's sample sd and the scored set are formed in `dtype` (fp32: as the
    kernel does, operation for operation as the definition orders them);
    magnitudes, sums and the analytic gradient are fp64 on those values widened.
    The yardstick of tests/test_photo_reproj_gpu.py.  With dtype = fp64 the same
    code is the loss in fp64 throughout: what (b) run in double must reproduce,
    gradient included.
(b) in torch ops with autograd -- `loss_and_grad_ops`: elementwise sequential-k
    products, index gathers, no library sampler; CPU or device, fp32 or fp64.  In
    fp32 it measures what fp32 costs on the same inputs and is the bench's
    context row.

T is P x H x W x C, D is P x H x W, I is Q x H x W x C, M is Q x 4 x 4, E is
Q x H x W or None; plane p uses q = p mod Q, M[q] and plane r = (q + shift) mod Q
of I and E.  The projection and the taps are tests/geo_cons_ref.py's."""
import numpy as np
import torch

import geo_cons_ref as geo

MODES = ('l1', 'charb')


def forward(T, D, I, M, E, shift, occl_thresh, dtype=np.float32):
  """Everything the definition forms in `dtype`: a dict with the projection, the
  taps, the tap values iv[c][k], the samples s[c] and the scored set."""
  T, D, I = np.asarray(T, dtype), np.asarray(D, dtype), np.asarray(I, dtype)
  p, h, w, nc = T.shape
  nq = I.shape[0]
  assert p % nq == 0 and 0 <= shift < nq and D.shape == (p, h, w)
  q = np.arange(p) % nq
  Mp = np.asarray(M, dtype)[q]
  q0, q1, n, q3, nden, u, v, dd = geo.project(D, Mp, dtype)
  t = geo.taps(u, v, h, w, dtype)
  r = ((q + shift) % nq)[:, None, None]
  zero = dtype(0.0)

  def sample(values):
    with np.errstate(all='ignore'):
      s = t['c'][0] * values[0]
      for k in range(1, 4):
        s = s + t['c'][k] * values[k]
      return np.where(t['ok'], s, zero).astype(dtype)

  iv = [[I[r, iy, ix, c] for iy, ix in t['idx']] for c in range(nc)]
  s = [sample(iv[c]) for c in range(nc)]
  with np.errstate(all='ignore'):
    f = np.isfinite
    half = dtype(0.5)
    scored = (f(D) & f(u) & f(v) & f(dd) & (n > 0) & (dd > 0) &
              (u >= half) & (u <= dtype(w) - half) & (v >= half) & (v <= dtype(h) - half))
    for c in range(nc):
      scored &= f(T[..., c]) & f(s[c])
    if occl_thresh > 0:
      assert E is not None
      E = np.asarray(E, dtype)
      sd = sample([E[r, iy, ix] for iy, ix in t['idx']])
      scored &= (sd > 0) & ~(sd - dd > dtype(occl_thresh) * (sd + dd))
  return dict(q0=q0, q1=q1, nden=nden, u=u, v=v, dd=dd, s=s, iv=iv, t=t, scored=scored,
              Mp=Mp, T=T)


def loss_and_grad(T, D, I, M, E=None, shift=0, mode='l1', occl_thresh=0.0, eps=1e-3,
                  upstream=1.0, dtype=np.float32):
  """(loss, gradient of upstream * loss w.r.t. T, w.r.t. D, plane sums P x 3, map
  P x H x W fp32 with -1 where unscored, scored set)."""
  assert mode in MODES
  f = forward(T, D, I, M, E, shift, occl_thresh, dtype)
  sc, t = f['scored'], f['t']
  nc = f['T'].shape[-1]
  eps = float(np.float32(eps))
  w64 = lambda a, fill=1.0: np.where(sc, a, fill).astype(np.float64)
  df = [w64(f['T'][..., c], 0.0) - w64(f['s'][c], 0.0) for c in range(nc)]
  e = np.zeros(sc.shape)
  for c in range(nc):
    e = e + (np.sqrt(df[c] * df[c] + eps * eps) if mode == 'charb' else np.abs(df[c]))
  e = e / float(nc)
  loss, sums, g = geo._terms(e, sc)
  emap = np.where(sc, e, -1.0).astype(np.float32)
  g = g * float(upstream)
  if mode == 'charb':
    psi = [df[c] / np.sqrt(df[c] * df[c] + eps * eps) for c in range(nc)]
  else:
    psi = [np.sign(df[c]) for c in range(nc)]
  M64 = f['Mp'].astype(np.float64)
  m3 = lambda j: M64[:, j, 3][:, None, None]
  nden = w64(f['nden'])
  rn2 = 1.0 / (nden * nden)
  u_d = (m3(0) * nden - w64(f['q0']) * m3(2)) * rn2
  v_d = (m3(1) * nden - w64(f['q1']) * m3(2)) * rn2
  K = {k: t[k].astype(np.float64) for k in ('wx0', 'wx1', 'wy0', 'wy1', 'vx0', 'vx1',
                                            'vy0', 'vy1')}
  gT = np.zeros(f['T'].shape)
  su, sv = np.zeros(sc.shape), np.zeros(sc.shape)
  for c in range(nc):
    with np.errstate(invalid='ignore'):
      ev = [np.where(sc, a, 0.0).astype(np.float64) for a in f['iv'][c]]
    s_u = (K['vx1'] * (K['vy0'] * K['wy0'] * ev[2] + K['vy1'] * K['wy1'] * ev[3]) -
           K['vx0'] * (K['vy0'] * K['wy0'] * ev[0] + K['vy1'] * K['wy1'] * ev[1]))
    s_v = (K['vy1'] * (K['vx0'] * K['wx0'] * ev[1] + K['vx1'] * K['wx1'] * ev[3]) -
           K['vy0'] * (K['vx0'] * K['wx0'] * ev[0] + K['vx1'] * K['wx1'] * ev[2]))
    gT[..., c] = np.where(sc, g * psi[c] / nc, 0.0)
    su, sv = su + psi[c] * s_u, sv + psi[c] * s_v
  gD = np.where(sc, -(g / nc) * (su * u_d + sv * v_d), 0.0)
  return loss, gT, gD, sums, emap, sc


# ---------------------------------------------------------------------------
# (b) torch ops
# ---------------------------------------------------------------------------
def loss_ops(T, D, I, M, E=None, shift=0, mode='l1', occl_thresh=0.0, eps=1e-3,
             return_scored=False):
  """The same graph in torch ops of T's dtype, differentiable w.r.t. T and D.  One
  pass without a graph decides which pixels are scored; the graph is then built
  over those pixels alone (index gathers), so that nothing that is not scored --
  a NaN, an Inf -- can reach a gradient."""
  assert mode in MODES
  p, h, w, nc = T.shape
  nq = I.shape[0]
  dev, dt = T.device, T.dtype
  eps = float(np.float32(eps))
  ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev),
                          indexing='ij')
  plane = torch.arange(p, device=dev)[:, None, None].expand(p, h, w).reshape(-1)
  px = (xs.to(dt) + 0.5).expand(p, h, w).reshape(-1)
  py = (ys.to(dt) + 0.5).expand(p, h, w).reshape(-1)
  view = plane % nq
  base = ((view + shift) % nq) * (h * w)
  Df, Tf = D.reshape(-1), T.reshape(-1, nc)
  If = [I[..., c].reshape(-1) for c in range(nc)]
  Ef = None if E is None else E.reshape(-1)

  def run(sel):
    d, m = Df[sel], M[view[sel]]
    q0, q1, n, q3 = geo._project_ops(d, m, px[sel], py[sel])
    nden = n + 1e-8 * (n == 0).to(dt)
    u, v, dd = q0 / nden, q1 / nden, q3 / nden
    fin = torch.isfinite(u) & torch.isfinite(v)
    uu, vv = torch.where(fin, u, torch.zeros_like(u)), torch.where(fin, v, torch.zeros_like(v))
    s = [geo._sample_ops(If[c], base[sel], uu, vv, h, w) for c in range(nc)]
    sd = None
    if occl_thresh > 0:
      sd = geo._sample_ops(Ef, base[sel], uu, vv, h, w)
    return d, n, u, v, dd, s, sd, fin

  with torch.no_grad():
    every = torch.arange(p * h * w, device=dev)
    d, n, u, v, dd, s, sd, fin = run(every)
    scored = (torch.isfinite(d) & fin & torch.isfinite(dd) & (n > 0) & (dd > 0) &
              (u >= 0.5) & (u <= w - 0.5) & (v >= 0.5) & (v <= h - 0.5))
    for c in range(nc):
      scored &= torch.isfinite(Tf[:, c]) & torch.isfinite(s[c])
    if occl_thresh > 0:
      thr = torch.tensor(np.float32(occl_thresh).item() if dt == torch.float32
                         else occl_thresh, dtype=dt, device=dev)
      scored &= (sd > 0) & ~(sd - dd > thr * (sd + dd))
    sel = torch.nonzero(scored)[:, 0]
  if sel.numel() == 0:
    out = (Df * 0.0).nan_to_num().sum() + (Tf * 0.0).nan_to_num().sum()
    return (out, scored.reshape(p, h, w)) if return_scored else out
  _, _, _, _, _, s, _, _ = run(sel)
  tex = Tf[sel]
  e = 0.0
  for c in range(nc):
    df = tex[:, c] - s[c]
    e = e + (torch.sqrt(df * df + eps * eps) if mode == 'charb' else df.abs())
  e = e / float(nc)
  sums = torch.zeros(p, dtype=dt, device=dev).index_add(0, plane[sel], e)
  n = torch.zeros(p, dtype=dt, device=dev).index_add(0, plane[sel], torch.ones_like(e))
  has = n > 0
  terms = torch.where(has, sums / torch.where(has, n, torch.ones_like(n)),
                      torch.zeros_like(n))
  out = terms.sum() / has.sum().to(dt)
  return (out, scored.reshape(p, h, w)) if return_scored else out


def loss_and_grad_ops(T, D, I, M, E=None, shift=0, mode='l1', occl_thresh=0.0, eps=1e-3,
                      upstream=1.0):
  """(loss, gradient of upstream * loss w.r.t. T, w.r.t. D) from `loss_ops` by
  autograd, as float / fp64 arrays."""
  T = T.detach().clone().requires_grad_(True)
  D = D.detach().clone().requires_grad_(True)
  l = loss_ops(T, D, I, M, E, shift, mode, occl_thresh, eps)
  (l * upstream).backward()
  return (float(l.detach()), T.grad.double().cpu().numpy(),
          D.grad.double().cpu().numpy())
