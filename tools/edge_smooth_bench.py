"""Times the fused edge-aware smoothness loss (csrc/lsi_edge_smooth.hip), forward
+ backward, against the same graph in torch ops (tests/edge_smooth_ref.py in
fp32) on one device, in alternating rounds of one process.

    python tools/edge_smooth_bench.py [--out FILE] [--rounds 5] [--iters 200]

Times are device events around `iters` back-to-back calls.  Bytes are what the
algorithm needs: the forward reads disp and guide once, the backward reads them
once more and writes the gradient."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'layered-scene-inference_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def timed(fn, iters):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(iters):
    fn()
  stop.record()
  stop.synchronize()
  return start.elapsed_time(stop) * 1e3 / iters    # us per call


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default='')
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=200)
  ap.add_argument('--shape', type=int, nargs=4, default=[4, 8, 256, 768])
  ap.add_argument('--order', type=int, default=1)
  ap.add_argument('--alpha', type=float, default=10.0)
  args = ap.parse_args(argv)
  if not torch.cuda.is_available():
    raise SystemExit('edge_smooth_bench: no ROCm device')
  import edge_smooth_ref as ref
  from lsi.loss import _hip
  dev = torch.device('cuda:0')
  nl, b, h, w = args.shape
  gen = torch.Generator(device='cpu').manual_seed(0)
  disp = (0.05 + 0.95 * torch.rand((nl, b, h, w, 1), generator=gen)).to(dev)
  guide = torch.rand((b, h, w, 3), generator=gen).to(dev)
  disp.requires_grad_(True)

  def fused_fwd():
    return _hip.edge_smoothness_loss(disp, guide, args.alpha, args.order, True)

  def fused():
    disp.grad = None
    fused_fwd().backward()

  def ops():
    disp.grad = None
    ref.loss(disp, guide, args.alpha, args.order, True).backward()

  # the two agree before they are timed
  fused()
  g_fused, l_fused = disp.grad.clone(), float(fused_fwd())
  ops()
  g_ops, l_ops = disp.grad.clone(), float(ref.loss(disp, guide, args.alpha,
                                                   args.order, True))
  grad_diff = float((g_fused - g_ops).abs().max() / g_ops.abs().max())
  for fn in (fused, ops, fused_fwd):
    timed(fn, 20)                                   # warm-up
  rows = {'fused': [], 'fused_fwd': [], 'ops': []}
  for _ in range(args.rounds):
    rows['fused'].append(timed(fused, args.iters))
    rows['ops'].append(timed(ops, max(args.iters // 4, 1)))
    with torch.no_grad():
      rows['fused_fwd'].append(timed(fused_fwd, args.iters))
  med = {k: float(np.median(v)) for k, v in rows.items()}
  lo = {k: float(np.min(v)) for k, v in rows.items()}
  n = nl * b * h * w
  fwd_bytes = 4 * (n + b * h * w * 3)
  bwd_bytes = fwd_bytes + 4 * n
  bwd_us = med['fused'] - med['fused_fwd']
  lines = [
      'edge-aware smoothness loss, forward + backward, fp32; disp %d x %d x %d x %d x 1, '
      'shared guide %d x %d x %d x 3, order %d, normalised, alpha %g' %
      (nl, b, h, w, b, h, w, args.order, args.alpha),
      '%d rounds of %d calls (op graph: %d), alternating; us per call, median (min)' %
      (args.rounds, args.iters, max(args.iters // 4, 1)),
      'fused forward + backward  %9.1f (%.1f)' % (med['fused'], lo['fused']),
      'fused forward alone       %9.1f (%.1f)   %.1f MB -> %.2f TB/s' %
      (med['fused_fwd'], lo['fused_fwd'], fwd_bytes / 1e6,
       fwd_bytes / med['fused_fwd'] / 1e6),
      'fused backward (the rest) %9.1f          %.1f MB -> %.2f TB/s' %
      (bwd_us, bwd_bytes / 1e6, bwd_bytes / max(bwd_us, 1e-9) / 1e6),
      'op graph fwd + bwd        %9.1f (%.1f)' % (med['ops'], lo['ops']),
      'loss fused %.9g ops %.9g; gradient difference %.3g of the largest entry' %
      (l_fused, l_ops, grad_diff),
      '(the fused times include the autograd and allocator work of one call each way)',
  ]
  text = '\n'.join(lines) + '\n'
  sys.stdout.write(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text)
  return 0 if med['fused'] < med['ops'] else 1


if __name__ == '__main__':
  sys.exit(main())
