"""Times the fused sparse depth-supervision loss (csrc/lsi_depth_sup.hip), forward
+ backward, at dense and at LiDAR-like 5 % ground truth, against the same graph
in torch ops (tests/depth_sup_ref.py in fp32) on one device, in alternating
rounds of one process.

    python tools/depth_sup_bench.py [--out FILE] [--rounds 5] [--iters 1000]
    python tools/depth_sup_bench.py --kernels-only   # for a kernel trace

Times are device events around `iters` back-to-back calls (a round of the fused
calls is 60 ms or more), after a second of warm-up: the first tenths of a second
of a process run at another clock.  Bytes are what the
algorithm needs: the forward reads gt once and pred where a pixel is scored, the
backward reads the same once more and writes the gradient."""
import argparse
import os
import sys
import time

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
  ap.add_argument('--iters', type=int, default=1000)
  ap.add_argument('--shape', type=int, nargs=3, default=[8, 256, 768])
  ap.add_argument('--mode', default='silog', choices=['silog', 'l1'])
  ap.add_argument('--layout', default='contiguous', choices=['contiguous', 'rgbd'],
                  help="pred contiguous, or channel 3 of layer 0 of the network's "
                  'P x H x W x (L 4) buffer (x-stride 8 at L = 2)')
  ap.add_argument('--kernels-only', action='store_true',
                  help='50 fused calls per density and nothing else')
  args = ap.parse_args(argv)
  if not torch.cuda.is_available():
    raise SystemExit('depth_sup_bench: no ROCm device')
  import depth_sup_ref as ref
  from lsi.loss import _hip
  dev = torch.device('cuda:0')
  p, h, w = args.shape
  n = p * h * w
  g_min = float(np.float32(1.0) / np.float32(80.0))
  g_max = float(np.float32(1.0) / np.float32(1e-3))
  kw = (args.mode, 0.5, 0.0, g_min, g_max, 1e-6)
  gen = torch.Generator(device='cpu').manual_seed(0)
  values = 0.05 + 0.95 * torch.rand((p, h, w), generator=gen)
  if args.layout == 'rgbd':
    buf = torch.zeros((p, h, w, 8))
    buf[..., 3] = values
    pred = buf.to(dev)[..., 3]
  else:
    pred = values.to(dev)
  pred.requires_grad_(True)
  full = 0.05 + 0.95 * torch.rand((p, h, w), generator=gen)
  keep = torch.rand((p, h, w), generator=gen) < 0.05
  text = ''
  ok_all = True
  for name, gt in (('dense', full.to(dev)), ('5 %', (full * keep).to(dev))):
    scored = int((gt > 0).sum())

    def fused_fwd():
      return _hip.depth_supervision_loss(pred, gt, None, *kw)

    def fused():
      pred.grad = None
      fused_fwd().backward()

    def ops():
      pred.grad = None
      ref.loss_ops(pred, gt, None, *kw).backward()

    if args.kernels_only:
      timed(fused, 50)
      continue
    # the two agree before they are timed
    fused()
    g_fused, l_fused = pred.grad.clone(), float(fused_fwd())
    ops()
    g_ops, l_ops = pred.grad.clone(), float(ref.loss_ops(pred, gt, None, *kw))
    grad_diff = float((g_fused - g_ops).abs().max() / g_ops.abs().max())
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:             # warm-up, a second of it
      for fn in (fused, ops, fused_fwd):
        timed(fn, 20)
    rows = {'fused': [], 'fused_fwd': [], 'ops': []}
    for _ in range(args.rounds):
      rows['fused'].append(timed(fused, args.iters))
      rows['ops'].append(timed(ops, max(args.iters // 4, 1)))
      with torch.no_grad():
        rows['fused_fwd'].append(timed(fused_fwd, args.iters))
    med = {k: float(np.median(v)) for k, v in rows.items()}
    lo = {k: float(np.min(v)) for k, v in rows.items()}
    fwd_bytes = 4 * (n + scored)
    bwd_bytes = fwd_bytes + 4 * n
    bwd_us = med['fused'] - med['fused_fwd']
    lines = [
        'depth-supervision loss (%s), forward + backward, fp32; pred and gt %d x %d x '
        '%d, pred %s, ground truth %s: %d of %d pixels scored' %
        (args.mode, p, h, w, args.layout, name, scored, n),
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
        '',
    ]
    text += '\n'.join(lines) + '\n'
    ok_all = ok_all and med['fused'] < med['ops']
  torch.cuda.synchronize()
  sys.stdout.write(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text)
  return 0 if ok_all else 1


if __name__ == '__main__':
  sys.exit(main())
