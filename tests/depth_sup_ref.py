"""The sparse depth-supervision loss (include/lsi_hip.h) restated
twice: in NumPy fp64, loss and analytic gradient -- the yardstick of
tests/test_depth_sup_gpu.py --, and in fp32 torch ops with autograd, which is
used only to measure what fp32 costs on the same inputs.

Both decide WHICH pixels are scored as the definition does, in fp32 (gt >
valid_above, g = gt * gt_scale[p] as one fp32 product, g_min <= g <= g_max); the
fp64 restatement then widens the fp32 values q = max(pred, eps) and g and does
everything else in fp64."""
import numpy as np
import torch

MODES = ('silog', 'l1')


def scored(gt, gt_scale, valid_above, g_min, g_max):
  """(mask P x H x W, g P x H x W fp32) of gt P x H x W, gt_scale P floats or None."""
  gt = np.asarray(gt, np.float32)
  g = gt
  if gt_scale is not None:
    g = gt * np.asarray(gt_scale, np.float32)[:, None, None]
  with np.errstate(invalid='ignore'):
    ok = ((gt > np.float32(valid_above)) & (g >= np.float32(g_min)) &
          (g <= np.float32(g_max)))
  return ok, g


def clamp(pred, eps):
  """(q = fmaxf(pred, eps) fp32, pred > eps): a NaN prediction becomes eps."""
  pred, eps = np.asarray(pred, np.float32), np.float32(eps)
  with np.errstate(invalid='ignore'):
    above = pred > eps
  return np.where(above, pred, eps).astype(np.float32), above


def loss_and_grad(pred, gt, gt_scale, mode, lam, valid_above, g_min, g_max, eps,
                  upstream=1.0):
  """fp64: (loss, gradient of upstream * loss w.r.t. pred [P,H,W], plane sums
  [P,3] = n_p, A_p, Q_p)."""
  assert mode in MODES
  ok, g32 = scored(gt, gt_scale, valid_above, g_min, g_max)
  q32, above = clamp(pred, eps)
  p = ok.shape[0]
  q = np.where(ok, q32, 1.0).astype(np.float64)
  g = np.where(ok, g32, 1.0).astype(np.float64)
  n = ok.reshape(p, -1).sum(1).astype(np.float64)
  has = n > 0
  s = float(has.sum())
  nn = np.where(has, n, 1.0)[:, None, None]
  sums = np.zeros((p, 3))
  sums[:, 0] = n
  grad = np.zeros(ok.shape)
  if s == 0:
    return 0.0, grad, sums
  if mode == 'silog':
    d = np.where(ok, np.log(q) - np.log(g), 0.0)
    a, qq = d.reshape(p, -1).sum(1), (d * d).reshape(p, -1).sum(1)
    sums[:, 1], sums[:, 2] = a, qq
    terms = np.where(has, qq / nn[:, 0, 0] - lam * (a / nn[:, 0, 0]) ** 2, 0.0)
    grad = (2.0 * d / nn - 2.0 * lam * a[:, None, None] / (nn * nn)) / q / s
  else:
    e = np.where(ok, q - g, 0.0)
    a = np.abs(e).reshape(p, -1).sum(1)
    sums[:, 1] = a
    terms = np.where(has, a / nn[:, 0, 0], 0.0)
    grad = np.sign(e) / (nn * s)
  grad = np.where(ok & above, grad, 0.0) * float(upstream)
  return float(terms.sum() / s), grad, sums


def loss(pred, gt, gt_scale, mode, lam, valid_above, g_min, g_max, eps):
  return loss_and_grad(pred, gt, gt_scale, mode, lam, valid_above, g_min, g_max,
                       eps)[0]


def loss_ops(pred, gt, gt_scale, mode, lam, valid_above, g_min, g_max, eps):
  """The same graph in torch ops of pred's dtype (differentiable w.r.t. pred):
  masks, wheres, logs and per-plane reductions."""
  assert mode in MODES
  g = gt if gt_scale is None else gt * gt_scale[:, None, None]
  ok = (gt > valid_above) & (g >= g_min) & (g <= g_max)
  one = torch.ones_like(pred)
  q = torch.where(pred > eps, pred, eps * one)
  q, g = torch.where(ok, q, one), torch.where(ok, g, one)
  n = ok.sum(dim=(1, 2)).to(pred.dtype)
  has = n > 0
  nn = torch.where(has, n, torch.ones_like(n))
  if mode == 'silog':
    d = torch.log(q) - torch.log(g)            # 0 where not scored
    m1, m2 = d.sum(dim=(1, 2)) / nn, (d * d).sum(dim=(1, 2)) / nn
    terms = m2 - lam * m1 * m1
  else:
    terms = (q - g).abs().sum(dim=(1, 2)) / nn
  s = has.sum()
  if int(s) == 0:
    return (q * 0.0).sum()                     # q is all ones here
  return torch.where(has, terms, torch.zeros_like(terms)).sum() / s.to(pred.dtype)


def loss_and_grad_ops(pred, gt, gt_scale, mode, lam, valid_above, g_min, g_max, eps,
                      upstream=1.0):
  """(loss, gradient of upstream * loss) from `loss_ops` by autograd, as float /
  fp64 array."""
  pred = pred.detach().clone().requires_grad_(True)
  l = loss_ops(pred, gt, gt_scale, mode, lam, valid_above, g_min, g_max, eps)
  (l * upstream).backward()
  return float(l.detach()), pred.grad.double().numpy()
