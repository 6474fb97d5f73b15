"""float32 / int64 NumPy restatement of the LDI mesh rasteriser (DESIGN.md
section 4.25, the comment of lsi_ldi_raster in include/lsi_hip.h).  Every fp32
operation is rounded on its own, in the stated order; the edge functions are
int64; the z-test is a maximum over 64-bit keys.  The existence rule is
ldi_mesh_ref.exists.  test_ldi_raster_gpu.py holds the kernels to it with
np.array_equal.

  r = raster(tex, mask, disp, M, ht, wt, ...)
  r['img'] B x V x Ht x Wt x 3, r['cov'], r['disp'] B x V x Ht x Wt,
  r['count']    B x V x Ht x Wt int32: triangles that cover the pixel's centre
                (the fill rule alone, before any z-test),
  r['winner']   B x V x Ht x Wt int64: the winning triangle's id, -1 at holes,
  r['max_coord']       the largest finite |u| or |v| of an existing vertex,
  r['dropped_extent']  triangles dropped by max_extent alone,
  r['triangles']       triangles that reached the coverage test.
"""
import numpy as np

import ldi_mesh_ref

F = np.float32
I = np.int64
GUARD = 16384
SUB = 256


def _sq(a):
  a = np.asarray(a, F)
  return a[..., 0] if a.ndim == 5 else a


def project(d, m):
  """d L x H x W float32, m 4 x 4: (X, Y int64, dd float32, usable, u, v)."""
  _, h, w = d.shape
  px = (np.arange(w, dtype=F) + F(0.5)).astype(F)[None, None, :]
  py = (np.arange(h, dtype=F) + F(0.5)).astype(F)[None, :, None]
  m = np.asarray(m, F)
  with np.errstate(all='ignore'):
    q = []
    for j in range(4):
      s = ((px * m[j, 0]).astype(F) + (py * m[j, 1]).astype(F)).astype(F)
      s = (s + m[j, 2]).astype(F)
      q.append((s + (d * m[j, 3]).astype(F)).astype(F))
    n = q[2]
    u, v, dd = (q[0] / n).astype(F), (q[1] / n).astype(F), (q[3] / n).astype(F)
    usable = (np.isfinite(u) & np.isfinite(v) & np.isfinite(dd) & (n > 0) & (dd > 0) &
              (np.abs(u) <= F(GUARD)) & (np.abs(v) <= F(GUARD)))
    x = np.where(usable, np.rint((u * F(SUB)).astype(F)), 0).astype(I)
    y = np.where(usable, np.rint((v * F(SUB)).astype(F)), 0).astype(I)
  return x, y, dd, usable, u, v


def _edges(t, px, py):
  """E_k (int64) and `inside` of pixel centres (px, py) for the set-up triangles
  t = dict of X, Y (3 x n)."""
  es, inside = [], np.ones(px.shape, bool)
  for k in range(3):
    ka, kb = (k + 1) % 3, (k + 2) % 3
    dx, dy = t['X'][kb] - t['X'][ka], t['Y'][kb] - t['Y'][ka]
    e = dx * (py - t['Y'][ka]) - dy * (px - t['X'][ka])
    top_left = (dy < 0) | ((dy == 0) & (dx > 0))
    inside &= (e > 0) | ((e == 0) & top_left)
    es.append(e)
  return es, inside


def _weights(es, area):
  fa = area.astype(F)
  b1 = (es[1].astype(F) / fa).astype(F)
  b2 = (es[2].astype(F) / fa).astype(F)
  b0 = ((F(1) - b1).astype(F) - b2).astype(F)
  return b0, b1, b2


def _blend(b, c0, c1, c2):
  with np.errstate(all='ignore'):
    return (((b[0] * c0).astype(F) + (b[1] * c1).astype(F)).astype(F) +
            (b[2] * c2).astype(F)).astype(F)


def _view(tex, e, d, m, ht, wt, edge_ratio, max_extent, bg_value, cull_back):
  nl, h, w = d.shape
  x, y, dd, usable, u, v = project(d, m)
  ok_v = e & usable
  with np.errstate(invalid='ignore'):
    coords = np.abs(np.stack([u, v]))[:, e]
    coords = coords[np.isfinite(coords)]
  max_coord = float(coords.max()) if coords.size else 0.0
  ls, ys, xs = np.meshgrid(np.arange(nl), np.arange(h - 1), np.arange(w - 1), indexing='ij')
  ls, ys, xs = ls.ravel(), ys.ravel(), xs.ravel()
  parts = []
  for t, corners in enumerate((((0, 0), (1, 0), (0, 1)), ((0, 1), (1, 0), (1, 1)))):
    vy = [ys + c[0] for c in corners]
    vx = [xs + c[1] for c in corners]
    ok = ok_v[ls, vy[0], vx[0]] & ok_v[ls, vy[1], vx[1]] & ok_v[ls, vy[2], vx[2]]
    ds = [d[ls, vy[k], vx[k]] for k in range(3)]
    with np.errstate(invalid='ignore', over='ignore'):
      lo = np.minimum(np.minimum(ds[0], ds[1]), ds[2])
      hi = np.maximum(np.maximum(ds[0], ds[1]), ds[2])
      ok &= lo >= (F(edge_ratio) * hi).astype(F)
    ids = ((ls * h + ys) * w + xs) * 2 + t
    parts.append((ok, ids, ls, vy, vx))
  ok = np.concatenate([p[0] for p in parts])
  ids = np.concatenate([p[1] for p in parts])[ok]
  ll = np.concatenate([p[2] for p in parts])[ok]
  vy = [np.concatenate([p[3][k] for p in parts])[ok] for k in range(3)]
  vx = [np.concatenate([p[4][k] for p in parts])[ok] for k in range(3)]
  X = [x[ll, vy[k], vx[k]] for k in range(3)]
  Y = [y[ll, vy[k], vx[k]] for k in range(3)]
  area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
  keep = area != 0
  if cull_back:
    keep &= area < 0               # area > 0: seen from behind
  swap = area < 0                  # the export's order under an orientation-keeping view
  sel = lambda a1, a2: (np.where(swap, a2, a1), np.where(swap, a1, a2))
  X[1], X[2] = sel(X[1], X[2])
  Y[1], Y[2] = sel(Y[1], Y[2])
  vy[1], vy[2] = sel(vy[1], vy[2])
  vx[1], vx[2] = sel(vx[1], vx[2])
  area = np.abs(area)
  xlo, xhi = np.minimum(np.minimum(X[0], X[1]), X[2]), np.maximum(np.maximum(X[0], X[1]), X[2])
  ylo, yhi = np.minimum(np.minimum(Y[0], Y[1]), Y[2]), np.maximum(np.maximum(Y[0], Y[1]), Y[2])
  i0 = np.maximum((xlo + 127) >> 8, 0)
  i1 = np.minimum((xhi - 128) >> 8, wt - 1)
  j0 = np.maximum((ylo + 127) >> 8, 0)
  j1 = np.minimum((yhi - 128) >> 8, ht - 1)
  keep &= (i0 <= i1) & (j0 <= j1)
  small = (i1 - i0 < max_extent) & (j1 - j0 < max_extent)
  dropped_extent = int((keep & ~small).sum())
  keep &= small
  take = lambda a: a[keep]
  tri = {'X': [take(a) for a in X], 'Y': [take(a) for a in Y], 'A': take(area), 'id': take(ids),
         'l': take(ll), 'vy': [take(a) for a in vy], 'vx': [take(a) for a in vx]}
  tri['dd'] = [dd[tri['l'], tri['vy'][k], tri['vx'][k]] for k in range(3)]
  i0, i1, j0, j1 = take(i0), take(i1), take(j0), take(j1)
  keys = np.zeros((ht, wt), np.uint64)
  count = np.zeros((ht, wt), np.int32)
  n = len(tri['id'])
  if n:
    for dj in range(int((j1 - j0).max()) + 1):
      for di in range(int((i1 - i0).max()) + 1):
        j, i = j0 + dj, i0 + di
        es, inside = _edges(tri, i * SUB + 128, j * SUB + 128)
        inside &= (j <= j1) & (i <= i1)
        jj, ii = np.where(inside, j, 0), np.where(inside, i, 0)
        np.add.at(count, (jj[inside], ii[inside]), 1)
        b = _weights(es, tri['A'])
        z = _blend(b, *tri['dd'])
        with np.errstate(invalid='ignore'):
          hit = inside & np.isfinite(z) & (z > 0)
        key = ((z.view(np.uint32).astype(np.uint64) << np.uint64(32)) |
               (np.uint64(0xFFFFFFFF) - tri['id'].astype(np.uint64)))
        np.maximum.at(keys, (jj[hit], ii[hit]), key[hit])
  # resolve
  img = np.full((ht, wt, 3), F(bg_value), F)
  cov = np.zeros((ht, wt), F)
  out_disp = np.zeros((ht, wt), F)
  winner = np.full((ht, wt), -1, I)
  pj, pi = np.nonzero(keys)
  if len(pj):
    k = keys[pj, pi]
    wid = (np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(I)
    lookup = np.full(2 * nl * h * w, -1, I)
    lookup[tri['id']] = np.arange(n)
    at = lookup[wid]
    assert (at >= 0).all()
    win = {'X': [a[at] for a in tri['X']], 'Y': [a[at] for a in tri['Y']]}
    es, inside = _edges(win, pi * SUB + 128, pj * SUB + 128)
    assert inside.all()
    b = _weights(es, tri['A'][at])
    cols = [tex[tri['l'][at], tri['vy'][c][at], tri['vx'][c][at]] for c in range(3)]
    for ch in range(3):
      img[pj, pi, ch] = _blend(b, cols[0][:, ch], cols[1][:, ch], cols[2][:, ch])
    cov[pj, pi] = 1
    out_disp[pj, pi] = (k >> np.uint64(32)).astype(np.uint32).view(F)
    winner[pj, pi] = wid
  return img, cov, out_disp, count, winner, max_coord, dropped_extent, n


def raster(tex, mask, disp, M, ht, wt, disp_min=1e-3, mask_min=0.5, edge_ratio=0.0,
           merge_ratio=0.0, max_extent=32, bg_value=1.0, cull_back=False):
  """tex L x B x H x W x 3, mask None or L x B x H x W [x 1], disp likewise, M
  B x V x 4 x 4: the module doc's dict."""
  tex, disp = np.asarray(tex, F), _sq(disp)
  mask = None if mask is None else _sq(mask)
  M = np.asarray(M, F)
  nb, nv = M.shape[:2]
  out = {'img': np.zeros((nb, nv, ht, wt, 3), F), 'cov': np.zeros((nb, nv, ht, wt), F),
         'disp': np.zeros((nb, nv, ht, wt), F), 'count': np.zeros((nb, nv, ht, wt), np.int32),
         'winner': np.zeros((nb, nv, ht, wt), I), 'max_coord': 0.0, 'dropped_extent': 0,
         'triangles': 0}
  for b in range(nb):
    d = disp[:, b]
    e = ldi_mesh_ref.exists(None if mask is None else mask[:, b], d, disp_min, mask_min,
                            merge_ratio)
    for v in range(nv):
      img, cov, od, count, winner, mc, dropped, n = _view(
          tex[:, b], e, d, M[b, v], ht, wt, edge_ratio, max_extent, bg_value, cull_back)
      out['img'][b, v], out['cov'][b, v], out['disp'][b, v] = img, cov, od
      out['count'][b, v], out['winner'][b, v] = count, winner
      out['max_coord'] = max(out['max_coord'], mc)
      out['dropped_extent'] += dropped
      out['triangles'] += n
  return out
