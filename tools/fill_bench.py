"""Times the push-pull hole filler (csrc/lsi_fill.hip through
lsi.geometry.fill) and, as context, the torch-op route of the same arguments
(fill_holes_ops); lists what a call puts on the device with the time of each
kernel, compares the kernels with the bytes the algorithm needs, and times an
iteration of ldi_render.py.

    python tools/fill_bench.py [--out FILE] [--rounds 5] [--shape 8 256 768 3]
                               [--render_views 9] [--render_iters 10]

Inputs: a random image over a canvas of value 1 in the form forward_splat
leaves it (LSI_FILL_SPLAT): a quarter of the pixels unreached at the default
shape -- 15 % scattered, the rest in bands 24 pixels wide -- the others reached
with a weight of 0.5 .. 2.5 over a canvas weight of 1e-3.

Times are device events around back-to-back calls, at least 50 ms per round,
rounds alternating between the routes; the median over the rounds (and the
minimum).  A call is what a user makes: the Python binding and its checks with
a workspace and an output kept between calls, not the kernels alone.  Kernel
times are the device durations in a torch profiler trace of 20 calls taken
after the timing, averaged.  The bytes are what the algorithm needs: one read
of img and w, one write of out, and a third of that each way for the pyramid.
The render time is a host clock around `Renderer.render_batch` calls that end
in a device synchronise (synthetic planes, an untrained model, K cameras): the
prediction, one forward_splat, one fill, the hole fractions and the two PSNRs;
the sheet's PNG is encoded off the thread and not in it."""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'layered-scene-inference_amd'))

HBM_TBS = 8.0    # MI355X peak HBM3E bandwidth, TB/s


def timed(fn, iters):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(iters):
    fn()
  stop.record()
  stop.synchronize()
  return start.elapsed_time(stop) * 1e3 / iters    # us per call


def traced(fn, calls):
  """name -> (launches per call, mean device time in us)."""
  from torch.profiler import profile, ProfilerActivity
  torch.cuda.synchronize()
  with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    for _ in range(calls):
      fn()
    torch.cuda.synchronize()
  rows = {}
  for e in prof.events():
    if not str(e.device_type).endswith('CUDA') or 'memcpy' in e.name.lower():
      continue
    short = (re.findall(r'\w+_kernel', e.name) or [e.name[:48]])[-1]
    rows.setdefault(short, []).append(e.device_time if hasattr(e, 'device_time') else e.cuda_time)
  return {k: (len(v) / float(calls), float(np.mean(v))) for k, v in rows.items()}


def inputs(dev, n, h, w, c, bg_wt):
  g = torch.Generator(device='cpu').manual_seed(0)
  fg = torch.rand((n, h, w, c), generator=g)
  reach = torch.rand((n, h, w), generator=g) > 0.15
  for b in range(n):
    for k in range(max(1, int(0.15 * w / 24))):
      x0 = int(torch.randint(0, max(w - 24, 1), (1,), generator=g))
      reach[b, :, x0:x0 + 24] = False
  lw = (0.5 + 2.0 * torch.rand((n, h, w), generator=g)) * reach
  wts = lw + bg_wt
  img = (fg * lw.unsqueeze(-1) + bg_wt) / wts.unsqueeze(-1)
  return img.to(dev).contiguous(), wts.to(dev).contiguous(), float(1 - reach.float().mean())


def render_time(views, iters):
  """ms per `render_batch` (after two warm-up calls), and the frame size."""
  import ldi_enc_dec as script
  import ldi_render
  argv = ['--dataset', 'synthetic', '--synth_scene', 'planes', '--batch_size', '1',
          '--n_layers', '2', '--random_weights', 'true', '--render_views', str(views),
          '--checkpoint_dir', tempfile.mkdtemp(prefix='fill_bench_')]
  opts = script.apply_dataset_overrides(ldi_render.build_parser().parse_args(argv))
  r = ldi_render.Renderer(opts)
  r.restore()
  batches = [r.trainer.data_loader.forward(1) for _ in range(4)]
  for k in range(2):
    r.render_batch(batches[k])
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for k in range(iters):
    r.render_batch(batches[k % 4])
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e3 / iters, len(r.s), opts.img_height, opts.img_width


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default='')
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--shape', type=int, nargs=4, default=[8, 256, 768, 3])
  ap.add_argument('--render_views', type=int, default=9)
  ap.add_argument('--render_iters', type=int, default=10)
  args = ap.parse_args(argv)
  if not torch.cuda.is_available():
    raise SystemExit('fill_bench: no ROCm device')
  from lsi import _C
  from lsi.geometry import fill
  dev = torch.device('cuda:0')
  n, h, w, c = args.shape
  bg_wt = 1e-3
  img, wts, holes = inputs(dev, n, h, w, c, bg_wt)
  out = torch.empty_like(img)
  need = int(_C.lib().lsi_fill_holes_workspace_bytes(n, h, w, c))
  ws = torch.empty(need, dtype=torch.uint8, device=dev)
  splat = _C.LSI_FILL_SPLAT
  fns = {
      'hip': lambda: fill._fill(img, wts, splat, bg_wt, 1.0, 1e-3, out=out, workspace=ws),
      'ops': lambda: fill.fill_holes_ops(img, wts, 1e-3, 1.0, mode='splat', bg_wt=bg_wt),
  }
  got, ops = fns['hip']().clone(), fns['ops']()
  err = float((got - ops).abs().max())
  unreached = wts <= bg_wt
  left = float((got[unreached] == 1.0).all(dim=-1).float().mean())
  reps = {}
  for name, fn in fns.items():
    timed(fn, 10)                                          # warm-up
    us = timed(fn, 10)
    reps[name] = max(int(60e3 / us) + 1, 10)               # >= 50 ms per round
  rows = {k: [] for k in fns}
  for _ in range(args.rounds):
    for name, fn in fns.items():
      rows[name].append(timed(fn, reps[name]))
  med = {k: float(np.median(v)) for k, v in rows.items()}
  lo = {k: float(np.min(v)) for k, v in rows.items()}
  trace = {k: traced(fns[k], 20) for k in fns}
  level0 = 4 * n * h * w * (c + 1)             # img and w
  io = level0 + 4 * n * h * w * c              # ... read once, out written
  pyramid = io / 3.0                           # and a third of that each way (levels 1 ..)
  need_bytes = io + 2 * pyramid
  # what the kernels move: push and pull both read level 0; the pushed levels
  # (c + 1 floats per pixel) are written once and read once
  moved = 2 * level0 + 4 * n * h * w * c + 2 * level0 / 3.0
  lines = [
      'lsi_fill_holes, LSI_FILL_SPLAT, %d x %d x %d x %d fp32, %.1f %% of the pixels unreached; '
      'workspace %.2f MB' % (n, h, w, c, 100 * holes, need / 1e6),
      'max |kernel - torch ops| on these inputs: %.3g; unreached pixels still at the canvas '
      'value after the fill: %.4f %%' % (err, 100 * left),
      '%d rounds, alternating; calls per round: %s; us per call, median (min)' %
      (args.rounds, ', '.join('%s %d' % kv for kv in reps.items())),
      'HIP, 3 launches                             %9.1f (%.1f)' % (med['hip'], lo['hip']),
      'context, torch ops                          %9.1f (%.1f)' % (med['ops'], lo['ops']),
      'the fused call takes %.3f of the op route\'s time' % (med['hip'] / med['ops']),
      '(a HIP call is timed as a user makes it: the Python binding and its checks, output and',
      ' workspace kept between calls, not the kernels alone)',
      'profiler trace of 20 calls: launches per call x mean device time, us',
  ]
  for k in ('hip', 'ops'):
    kernels = trace[k]
    total = sum(cnt * t for cnt, t in kernels.values())
    lines.append('  %-4s %6.1f kernels per call, %.1f us on the device' %
                 (k, sum(cnt for cnt, _ in kernels.values()), total))
    if k == 'hip':
      for name in sorted(kernels):
        lines.append('      %4.1f x %-28s %8.2f' % (kernels[name][0], name, kernels[name][1]))
  dev_us = sum(cnt * t for cnt, t in trace['hip'].values())
  lines += [
      'bytes the algorithm needs: %.2f MB (img + w read, out written) + 2 x %.2f MB (the pyramid, '
      'a third each way) = %.2f MB' % (io / 1e6, pyramid / 1e6, need_bytes / 1e6),
      'over the %.1f us of the three kernels: %.3f TB/s, %.1f %% of the %.1f TB/s HBM peak '
      '(the bound is bandwidth)' %
      (dev_us, need_bytes / dev_us / 1e6, 100 * need_bytes / dev_us / 1e6 / HBM_TBS, HBM_TBS),
      'bytes the kernels move (img + w read by push and by pull, out written, the pushed levels '
      'written once and read once): %.2f MB, %.3f TB/s' % (moved / 1e6, moved / dev_us / 1e6),
  ]
  if args.render_iters > 0:
    ms, k, ih, iw = render_time(args.render_views, args.render_iters)
    lines.append('ldi_render.py, synthetic planes, 2 layers, %d x %d, K = %d cameras, untrained '
                 'model: %.2f ms per iteration (host clock, %d iterations after 2 warm-up)' %
                 (ih, iw, k, ms, args.render_iters))
  text = '\n'.join(lines) + '\n'
  sys.stdout.write(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text)
  return 0 if med['hip'] <= med['ops'] else 1


if __name__ == '__main__':
  sys.exit(main())
