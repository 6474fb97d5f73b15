"""The edge-aware disparity smoothness loss restated in torch
ops, dtype-generic; autograd gives the gradient.  The yardstick of
tests/test_edge_smooth_*.py in fp64, and in fp32 the measure of what fp32
arithmetic itself costs."""
import torch

EPS = 1e-7


def _guide5(disp, guide):
  """The guide as L x B x H x W x 3 (a shared one broadcast over the layers)."""
  return guide.unsqueeze(0).expand(disp.shape[0], -1, -1, -1, -1) \
      if guide.dim() == 4 else guide


def stencils(disp, guide, order):
  """(sx, sy, ex, ey): sx L x B x H x (W - o), sy L x B x (H - o) x W on the raw
  disparities disp L x B x H x W x 1, ex / ey the guide's mean absolute
  differences at the same places."""
  d = disp[..., 0]
  g = _guide5(disp, guide)
  if order == 1:
    sx = d[:, :, :, :-1] - d[:, :, :, 1:]
    sy = d[:, :, :-1, :] - d[:, :, 1:, :]
    ex = (g[:, :, :, :-1] - g[:, :, :, 1:]).abs().mean(-1)
    ey = (g[:, :, :-1, :] - g[:, :, 1:, :]).abs().mean(-1)
  elif order == 2:
    sx = d[:, :, :, :-2] - 2 * d[:, :, :, 1:-1] + d[:, :, :, 2:]
    sy = d[:, :, :-2, :] - 2 * d[:, :, 1:-1, :] + d[:, :, 2:, :]
    ex = 0.5 * (g[:, :, :, 2:] - g[:, :, :, :-2]).abs().mean(-1)
    ey = 0.5 * (g[:, :, 2:, :] - g[:, :, :-2, :]).abs().mean(-1)
  else:
    raise ValueError(order)
  return sx, sy, ex, ey


def plane_sums(disp, guide, alpha, order):
  """(A, B, S), each L x B."""
  sx, sy, ex, ey = stencils(disp, guide, order)
  a = (sx.abs() * torch.exp(-alpha * ex)).sum((2, 3))
  b = (sy.abs() * torch.exp(-alpha * ey)).sum((2, 3))
  return a, b, disp[..., 0].sum((2, 3))


def loss(disp, guide, alpha, order, normalise):
  nl, nb, h, w, _ = disp.shape
  a, b, s = plane_sums(disp, guide, alpha, order)
  k = 1.0 / (s / (h * w) + EPS) if normalise else torch.ones_like(s)
  return (k * (a / (h * (w - order)) + b / ((h - order) * w))).sum() / (nl * nb)


def loss_and_grad(disp, guide, alpha, order, normalise, upstream=1.0):
  d = disp.clone().requires_grad_(True)
  l = loss(d, guide, alpha, order, normalise)
  (l * upstream).backward()
  return l.detach(), d.grad


def min_nonzero_stencil(disp, guide, order):
  """(smallest non-zero |stencil|, fraction of exact zeros)."""
  sx, sy, _, _ = stencils(disp, guide, order)
  v = torch.cat([sx.reshape(-1), sy.reshape(-1)]).abs()
  nz = v[v != 0]
  return (float(nz.min()) if nz.numel() else float('inf'),
          float((v == 0).double().mean()))
