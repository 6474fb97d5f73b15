"""Times the fused depth accuracy metrics (csrc/lsi_depth_metrics.hip through
MetricAccumulator.add_depth_accuracy) with and without median scaling and, as
context, the torch-op route of the same arguments
(eval_metrics.depth_accuracy_metrics), and counts what a call puts on the
device.

    python tools/depth_metrics_bench.py [--out FILE] [--rounds 5] [--shape 4 256 768]

Inputs: depths log-uniform over [0.5, 120], 30 % of the ground truth empty,
predictions gt exp(N(0, 0.3)); the whole image is scored.  Times are device
events around back-to-back calls, at least 50 ms per round, rounds alternating
between the routes; the median over the rounds (and the minimum).  The op route
reads sizes back to the host (boolean indexing, one image at a time), so its
time includes those synchronisations.  Bytes are what the kernels read: gt and
pred at every pixel of the crop, once per pass over the maps (one pass, five
with median scaling).  Launches and copies are counted in a torch
profiler trace of one call, taken after the timing."""
import argparse
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'layered-scene-inference_amd'))


def timed(fn, iters):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(iters):
    fn()
  stop.record()
  stop.synchronize()
  return start.elapsed_time(stop) * 1e3 / iters    # us per call


def traced(fn):
  """(kernel names, copies) one call puts on the device."""
  from torch.profiler import profile, ProfilerActivity
  torch.cuda.synchronize()
  with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    fn()
    torch.cuda.synchronize()
  names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA')]
  copies = [n for n in names if 'memcpy' in n.lower()]
  return [n for n in names if n not in copies], copies


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default='')
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--shape', type=int, nargs=3, default=[4, 256, 768])
  args = ap.parse_args(argv)
  if not torch.cuda.is_available():
    raise SystemExit('depth_metrics_bench: no ROCm device')
  from lsi.nnutils import eval_metrics
  dev = torch.device('cuda:0')
  B, H, W = args.shape
  rs = np.random.RandomState(0)
  depth = np.exp(rs.uniform(np.log(0.5), np.log(120.), (B, H, W)))
  gt_np = (1.0 / depth).astype(np.float32)
  gt_np[rs.rand(B, H, W) < 0.3] = 0
  pred_np = (gt_np * np.exp(0.3 * rs.randn(B, H, W))).astype(np.float32)
  pred_np[gt_np == 0] = 0.1
  pred, gt = torch.tensor(pred_np, device=dev), torch.tensor(gt_np, device=dev)
  scored = int(((gt_np > 0) & (1 / np.maximum(gt_np, 1e-30) <= 80.)).sum())
  acc = eval_metrics.MetricAccumulator(dev)

  fns = {
      'fused': lambda: acc.add_depth_accuracy(pred, gt),
      'fused_median': lambda: acc.add_depth_accuracy(pred, gt, median=True),
      'ops': lambda: eval_metrics.depth_accuracy_metrics(pred, gt),
      'ops_median': lambda: eval_metrics.depth_accuracy_metrics(pred, gt, median=True),
  }
  n = {}
  for name, fn in fns.items():
    timed(fn, 10)                                          # warm-up
    us = timed(fn, 10)
    n[name] = max(int(60e3 / us) + 1, 10)                  # >= 50 ms per round
  rows = {k: [] for k in fns}
  for _ in range(args.rounds):
    for name, fn in fns.items():
      rows[name].append(timed(fn, n[name]))
  med = {k: float(np.median(v)) for k, v in rows.items()}
  lo = {k: float(np.min(v)) for k, v in rows.items()}
  one_pass = 8 * B * H * W
  trace = {k: traced(fns[k]) for k in ('fused', 'fused_median', 'ops_median')}
  lines = [
      'depth accuracy of %d x %d x %d maps, %d pixels scored (%.0f %%), whole image' %
      (B, H, W, scored, 100.0 * scored / (B * H * W)),
      'bytes read: %.2f MB per pass over the maps (gt and pred, fp32)' %
      (one_pass / 1e6),
      '%d rounds, alternating; calls per round: %s; us per call, median (min)' %
      (args.rounds, ', '.join('%s %d' % kv for kv in n.items())),
      'fused, no scaling:      2 launches          %9.1f (%.1f)   %.2f TB/s over 1 pass' %
      (med['fused'], lo['fused'], one_pass / med['fused'] / 1e6),
      'fused, median scaling: 10 launches          %9.1f (%.1f)   %.2f TB/s over 5 passes' %
      (med['fused_median'], lo['fused_median'], 5 * one_pass / med['fused_median'] / 1e6),
      'context, torch ops, no scaling              %9.1f (%.1f)' % (med['ops'], lo['ops']),
      'context, torch ops, median scaling (sorts)  %9.1f (%.1f)' %
      (med['ops_median'], lo['ops_median']),
      '(the fused calls are timed as the evaluation makes them: the Python binding and its',
      ' checks, not the kernels alone)',
      'profiler trace of one call, kernels / copies on the device:',
  ]
  for k in ('fused', 'fused_median', 'ops_median'):
    kernels, copies = trace[k]
    lines.append('  %-13s %3d kernels, %d copies' % (k, len(kernels), len(copies)))
    if k.startswith('fused'):
      short = [(re.findall(r'\w+_kernel', name) or [name[:60]])[-1] for name in kernels]
      for name in sorted(set(short)):
        lines.append('      %2d x %s' % (short.count(name), name))
  text = '\n'.join(lines) + '\n'
  sys.stdout.write(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text)
  return 0


if __name__ == '__main__':
  sys.exit(main())
