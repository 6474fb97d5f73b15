"""The SSIM view-synthesis loss and metric restated twice (the
reference project has none, so the definition is the yardstick):

  * in torch ops (separable F.conv2d, dtype-generic): in fp64 the yardstick of
    tests/test_ssim_gpu.py, in fp32 the arithmetic baseline whose own error
    against fp64 sets the bar for the kernels;
  * directly in numpy fp64: explicit n x n windows in loops, no convolution.

tests/test_ssim_cpu.py holds the two against each other."""
import math

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 1e-4, 9e-4


def py2_round(x):
  return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def window64(win, sigma):
  """The weights in fp64: g[i] ~ exp(-(i - (n-1)/2)^2 / (2 sigma^2)), sum 1;
  sigma <= 0: the box.  sigma is an fp32 parameter of the C ABI: the formula is
  evaluated at that value."""
  sigma = float(np.float32(sigma))
  x = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
  w = np.exp(-(x * x) / (2.0 * sigma * sigma)) if sigma > 0 else np.ones(win)
  return w / w.sum()


def window(win, sigma, dtype):
  """What the kernels take: the fp64 weights rounded to fp32 (then widened again
  for the fp64 restatement, so that both dtypes weigh alike)."""
  return torch.from_numpy(window64(win, sigma).astype(np.float32)).to(dtype)


def area(target, ht, wt):
  """AREA resize for integer factors: the box's elements added rows then
  columns in order, one multiply by 1 / (fy fx).  target B x H x W x 3."""
  b, h, w, c = target.shape
  fy, fx = h // ht, w // wt
  assert fy * ht == h and fx * wt == w
  blocks = target.reshape(b, ht, fy, wt, fx, c)
  t = torch.zeros((b, ht, wt, c), dtype=target.dtype, device=target.device)
  for dy in range(fy):
    for dx in range(fx):
      t = t + blocks[:, :, dy, :, dx]
  return t * (1.0 / (fy * fx))


def ssim_maps(recons, target, x_min, y_min, win, sigma):
  """S [nl, B, Hv, Wv, 3] of recons nl x B x Ht x Wt x 3 against target
  B x H x W x 3, in the dtype of recons."""
  nl, b, ht, wt, _ = recons.shape
  dt = recons.dtype
  t = area(target.to(dt), ht, wt)
  x = recons[:, :, y_min:ht - y_min, x_min:wt - x_min]
  y = t[:, y_min:ht - y_min, x_min:wt - x_min].unsqueeze(0).expand_as(x)
  g = window(win, sigma, dt).to(recons.device)

  def blur(v):  # [nl, B, hc, wc, 3] -> [nl, B, Hv, Wv, 3]: rows, then columns
    hc, wc = v.shape[2:4]
    p = v.permute(0, 1, 4, 2, 3).reshape(-1, 1, hc, wc)
    p = F.conv2d(p, g.view(1, 1, 1, win))
    p = F.conv2d(p, g.view(1, 1, win, 1))
    return p.reshape(nl, b, 3, hc - win + 1, wc - win + 1).permute(0, 1, 3, 4, 2)

  mx, my = blur(x), blur(y)
  exx, eyy, exy = blur(x * x), blur(y * y), blur(x * y)
  vx, vy, cxy = exx - mx * mx, eyy - my * my, exy - mx * my
  return ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) *
                                                 (vx + vy + C2))


def dssim_maps(recons, target, x_min, y_min, win, sigma):
  """d [nl, B, Hv, Wv]."""
  s = ssim_maps(recons, target, x_min, y_min, win, sigma)
  return (1.0 - s.sum(dim=4) / 3.0) / 2.0


def loss(recons, target, x_min, y_min, win, sigma):
  """mean over b, v, u of min_l d; amin splits the gradient evenly among tied
  layers (TF's reduce_min rule)."""
  return torch.amin(dssim_maps(recons, target, x_min, y_min, win, sigma),
                    dim=0).mean()


def metric(recons, target, x_min, y_min, win, sigma):
  """(sum over b, v, u of layer 0's mean SSIM, number of windows)."""
  s = ssim_maps(recons[:1], target, x_min, y_min, win, sigma).sum(dim=4) / 3.0
  return float(s.sum()), float(s.numel())


def best_gap(recons, target, x_min, y_min, win, sigma):
  """Smallest gap between the best and the second-best layer over all windows
  (inf for one layer)."""
  d = dssim_maps(recons, target, x_min, y_min, win, sigma)
  if d.shape[0] < 2:
    return float('inf')
  two = torch.topk(d, 2, dim=0, largest=False).values
  return float((two[1] - two[0]).min())


def dssim_direct(recons, target, x_min, y_min, win, sigma):
  """d [nl, B, Hv, Wv] in numpy fp64, one explicit window at a time."""
  recons = np.asarray(recons, np.float64)
  target = np.asarray(target, np.float64)
  nl, b, ht, wt, _ = recons.shape
  _, h, w, _ = target.shape
  fy, fx = h // ht, w // wt
  t = target.reshape(b, ht, fy, wt, fx, 3).sum(axis=(2, 4)) / (fy * fx)
  g = window64(win, sigma).astype(np.float32).astype(np.float64)
  w2 = np.outer(g, g)[:, :, None]
  hv, wv = ht - 2 * y_min - win + 1, wt - 2 * x_min - win + 1
  d = np.zeros((nl, b, hv, wv))
  for l in range(nl):
    for i in range(b):
      for v in range(hv):
        for u in range(wv):
          y0, x0 = y_min + v, x_min + u
          x = recons[l, i, y0:y0 + win, x0:x0 + win]
          y = t[i, y0:y0 + win, x0:x0 + win]
          mx, my = (w2 * x).sum(axis=(0, 1)), (w2 * y).sum(axis=(0, 1))
          vx = (w2 * x * x).sum(axis=(0, 1)) - mx * mx
          vy = (w2 * y * y).sum(axis=(0, 1)) - my * my
          cxy = (w2 * x * y).sum(axis=(0, 1)) - mx * my
          s = ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) *
                                                      (vx + vy + C2))
          d[l, i, v, u] = (1.0 - s.sum() / 3.0) / 2.0
  return d
