"""Shared by test_layers_grad_cpu.py / test_layers_grad_gpu.py: the fused
renderer's op graph on oracle/lsi_torch_ref.py (any float dtype, autograd), the
closed-form gradients of DESIGN section 4.9 as plain tensor arithmetic, the
pixels at a kink, and small random scenes."""
import numpy as np
import torch

import lsi_torch_ref as TR

EPS = 1e-8


def view_xy(h, w, dt):
  x = (torch.arange(w, dtype=dt) + 0.5).view(1, 1, w).expand(1, h, w)
  y = (torch.arange(h, dtype=dt) + 0.5).view(1, h, 1).expand(1, h, w)
  return x, y


def warp(hom, dmat, hw):
  """hom P x 9, dmat P x 3 -> coords P x H x W x 2 (texture pixels), dm P x H x
  W x 1: hom (x + .5, y + .5, 1), divide_safe, the dmat product."""
  x, y = view_xy(hw[0], hw[1], hom.dtype)
  hh = hom.reshape(-1, 9, 1, 1)
  q = [(x * hh[:, 3 * r] + y * hh[:, 3 * r + 1]) + hh[:, 3 * r + 2] for r in range(3)]
  coords = torch.stack([TR.divide_safe(q[0], q[2]), TR.divide_safe(q[1], q[2])], -1)
  dd = dmat.reshape(-1, 3, 1, 1)
  dm = ((dd[:, 0] * x + dd[:, 1] * y) + dd[:, 2]).unsqueeze(-1)
  return coords, dm


def fused_oracle(tex, hom, dmat, hw, soft, min_disp, temp):
  """tex B x P x Hs x Ws x 4, hom B x V x P x 9, dmat B x V x P x 3 ->
  img B x V x H x W x 3, disp B x V x H x W x 1."""
  imgs, disps = [], []
  for b in range(hom.shape[0]):
    for v in range(hom.shape[1]):
      coords, dm = warp(hom[b, v], dmat[b, v], hw)
      both = TR.bilinear(tex[b], coords)
      imgs.append(TR.compose(both[..., :3], both[..., 3:4], dm, soft, min_disp, temp))
      disps.append(TR.compose_depth(both[..., 3:4], dm, False, min_disp, temp))
  shape = tuple(hom.shape[:2]) + tuple(hw)
  return torch.stack(imgs).reshape(shape + (3,)), torch.stack(disps).reshape(shape + (1,))


def probs(masks, dmaps, min_disp, temp):
  """p = softmax(z) over the L + 1 layers and relu(d) of the L layers."""
  d = torch.relu(dmaps)
  m_all = torch.cat([masks, torch.ones_like(masks[:1])], 0)
  d_all = torch.cat([d, torch.full_like(d[:1], min_disp)], 0)
  den = d_all + EPS * (d_all == 0).to(d.dtype)
  z = torch.log(m_all + EPS) - 1.0 / (den * temp)
  return torch.softmax(z, 0), d


def compose_closed(imgs, masks, dmaps, g, soft, min_disp, temp):
  """Section 4.9: (g_imgs, g_masks, g_dmaps) of layers.compose."""
  nl = imgs.shape[0]
  p, d = probs(masks, dmaps, min_disp, temp)
  if not soft:
    win = torch.argmax(p, 0, keepdim=True)
    sel = (torch.arange(nl).view((nl,) + (1,) * (p.dim() - 1)) == win).to(g.dtype)
    return sel * g, torch.zeros_like(masks), torch.zeros_like(dmaps)
  col = torch.cat([imgs, torch.ones_like(imgs[:1])], 0)
  out = (p * col).sum(0)
  gz = p * ((g * col).sum(-1, keepdim=True) - (g * out).sum(-1, keepdim=True))
  gz = gz[:nl]
  pos = (d > 0).to(g.dtype)
  d2 = torch.where(d > 0, d * d, torch.ones_like(d))
  return p[:nl] * g, gz / (masks + EPS), gz * pos / (temp * d2)


def compose_depth_closed(masks, dmaps, g, bg_layer, min_disp, temp):
  """Section 4.9: g_dmaps of layers.compose_depth."""
  nl = masks.shape[0]
  d = torch.relu(dmaps)
  if bg_layer:
    dmax = max(float(d.max()), min_disp)
    # probs() appends min_disp itself; relu(dmax - d) = dmax - d
    p, _ = probs(masks, dmax - d, min_disp, temp)
  else:
    p, _ = probs(masks, dmaps, min_disp, temp)
  win = torch.argmax(p, 0, keepdim=True)
  sel = (torch.arange(nl).view((nl,) + (1,) * (p.dim() - 1)) == win).to(g.dtype)
  return sel * g * (d > 0).to(g.dtype)


def fused_closed(tex, hom, dmat, hw, soft, min_disp, temp, g_img, g_disp):
  """Section 4.9, the fused chain: (g_tex, g_hom, g_dmat)."""
  dt = tex.dtype
  nb, npl, hs, ws, _ = tex.shape
  h, w = hw
  x, y = view_xy(h, w, dt)
  one = torch.ones_like(x)
  g_tex, g_hom, g_dmat = torch.zeros_like(tex), torch.zeros_like(hom), torch.zeros_like(dmat)
  for b in range(nb):
    flat = tex[b].reshape(npl, hs * ws, 4)
    for v in range(hom.shape[1]):
      hh = hom[b, v].reshape(npl, 9, 1, 1)
      q = [(x * hh[:, 3 * r] + y * hh[:, 3 * r + 1]) + hh[:, 3 * r + 2] for r in range(3)]
      den = q[2] + EPS * (q[2] == 0).to(dt)
      u, vv = q[0] / den, q[1] / den
      xs, ys = u - 0.5, vv - 0.5
      x0, y0 = torch.floor(xs), torch.floor(ys)
      wx = [x0 + 1 - xs, xs - x0]
      wy = [y0 + 1 - ys, ys - y0]
      cx = [x0, x0 + 1]
      cy = [y0, y0 + 1]
      vx = [((c >= 0) & (c <= ws - 1)).to(dt) for c in cx]
      vy = [((c >= 0) & (c <= hs - 1)).to(dt) for c in cy]
      taps = []   # (i, j): x tap i, y tap j -> masked weight, index, texels
      both = torch.zeros((npl, h, w, 4), dtype=dt)
      for i in range(2):
        for j in range(2):
          idx = (cx[i].clamp(0, ws - 1) + cy[j].clamp(0, hs - 1) * ws).long()
          t = torch.stack([flat[p][idx[p]] for p in range(npl)])   # P x H x W x 4
          c = vx[i] * vy[j] * wx[i] * wy[j]
          both = both + c.unsqueeze(-1) * t
          taps.append((i, j, c, idx, t))
      dd = dmat[b, v].reshape(npl, 3, 1, 1)
      dm = ((dd[:, 0] * x + dd[:, 1] * y) + dd[:, 2]).unsqueeze(-1)
      col, m = both[..., :3], both[..., 3:4]
      gi = g_img[b, v] if g_img is not None else torch.zeros((h, w, 3), dtype=dt)
      g_col, g_m, g_d = compose_closed(col, m, dm, gi, soft, min_disp, temp)
      if g_disp is not None:
        g_d = g_d + compose_depth_closed(m, dm, g_disp[b, v], False, min_disp, temp)
      g_both = torch.cat([g_col, g_m], -1)                          # P x H x W x 4
      gx = torch.zeros((npl, h, w), dtype=dt)
      gy = torch.zeros((npl, h, w), dtype=dt)
      for i, j, c, idx, t in taps:
        for p in range(npl):
          g_tex[b, p].view(hs * ws, 4).index_add_(
              0, idx[p].reshape(-1), (c[p].unsqueeze(-1) * g_both[p]).reshape(-1, 4))
        s = (g_both * t).sum(-1)
        gx = gx + s * vx[i] * vy[j] * wy[j] * (1 if i else -1)
        gy = gy + s * vx[i] * vy[j] * wx[i] * (1 if j else -1)
      gq = [gx / den, gy / den, -(gx * u + gy * vv) / den]
      for r in range(3):
        for k, pk in enumerate((x, y, one)):
          g_hom[b, v, :, 3 * r + k] = (gq[r] * pk).sum((1, 2))
      gdd = g_d[..., 0]      # compose_closed / compose_depth_closed carry [d > 0]
      for k, pk in enumerate((x, y, one)):
        g_dmat[b, v, :, k] = (gdd * pk).sum((1, 2))
  return g_tex, g_hom, g_dmat


def kink_keep(tex, hom, dmat, hw, hard, min_disp, temp):
  """fp64: B x V x H x W bool, False where some plane's x or y lies within 1e-3
  of an integer or (hard) the two largest probabilities differ by < 1e-4."""
  keep = torch.ones(tuple(hom.shape[:2]) + tuple(hw), dtype=torch.bool)
  for b in range(hom.shape[0]):
    for v in range(hom.shape[1]):
      coords, dm = warp(hom[b, v], dmat[b, v], hw)
      xy = coords - 0.5
      near = ((xy - torch.round(xy)).abs() < 1e-3).any(-1).any(0)
      keep[b, v] &= ~near
      if hard:
        both = TR.bilinear(tex[b], coords)
        p, _ = probs(both[..., 3:4], dm, min_disp, temp)
        top = torch.sort(p, 0)[0]
        keep[b, v] &= ((top[-1] - top[-2]) >= 1e-4)[..., 0]
  return keep


def scene(seed, nb, nv, npl, hs, ws, h, w):
  """A generic small scene (fp64): planes mostly inside the views, in front of
  the camera, disparities around the background's."""
  rs = np.random.RandomState(seed)
  tex = rs.rand(nb, npl, hs, ws, 4)
  hom = np.tile(np.array([ws / w, 0, 0, 0, hs / h, 0, 0, 0, 1.0]), (nb, nv, npl, 1))
  hom[..., [0, 4]] *= 1 + 0.1 * rs.randn(nb, nv, npl, 2)
  hom[..., [1, 3]] = 0.05 * rs.randn(nb, nv, npl, 2)
  hom[..., [2, 5]] = 1.5 * rs.randn(nb, nv, npl, 2)
  hom[..., [6, 7]] = 0.003 * rs.randn(nb, nv, npl, 2)
  dmat = np.concatenate([0.004 * rs.randn(nb, nv, npl, 2),
                         0.15 + 0.5 * rs.rand(nb, nv, npl, 1)], -1)
  return torch.tensor(tex), torch.tensor(hom), torch.tensor(dmat)
