"""Times the LiDAR rasteriser (csrc/lsi_lidar.hip through
lsi.geometry.lidar.rasterize_points) with the occlusion filter off and on and,
as context, the torch-op route of the same arguments (rasterize_points_ops),
and lists what a call puts on the device with the time of each kernel.

    python tools/lidar_bench.py [--out FILE] [--rounds 5] [--scans 4] [--points 120000]
                                [--shape 256 768] [--trace_calls 0]

Inputs: synthetic Velodyne HDL-64 scans in the file order of KITTI raw (64 rings
from +2 to -24.8 degrees, all around; a ground plane 1.73 m below the scanner,
returns at 5 - 80 m above it, 3 % range noise), padded form, projected into two
views by velodyne.velo_to_image of a calibration with KITTI's published
magnitudes (f = 721.5 px at 375 x 1242, 0.54 m baseline) resized to the shape.
About an eighth of a scan falls inside a view.

Times are device events around back-to-back calls, at least 50 ms per round,
rounds alternating between the routes; the median over the rounds (and the
minimum).  A call is what the evaluation makes: the Python binding, its checks
and the upload of the B descriptors (one 16 B x B host-to-device copy), not the
kernels alone.  Kernel times are the device durations in a torch profiler trace
of 20 calls taken after the timing, averaged.  The scatter's bytes are what the
algorithm needs: 16 B per point.  --trace_calls N makes N calls of each HIP
variant and exits: for an external kernel trace."""
import argparse
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'layered-scene-inference_amd'))

HBM_TBS = 8.0    # MI355X peak HBM3E bandwidth, TB/s


def synthetic_scan(rs, n):
  rings = 64
  per_ring = n // rings
  elev = np.deg2rad(np.linspace(2.0, -24.8, rings))[:, None]
  azim = np.linspace(np.pi, -np.pi, per_ring, endpoint=False)[None, :]
  ground = np.where(elev < -0.02, 1.73 / np.maximum(np.sin(-elev), 1e-3), np.inf)
  rng = np.minimum(rs.uniform(5.0, 80.0, (rings, per_ring)), ground)
  rng = rng * (1 + 0.03 * rs.randn(rings, per_ring))
  pts = np.stack([rng * np.cos(elev) * np.cos(azim), rng * np.cos(elev) * np.sin(azim),
                  rng * np.sin(elev), rs.rand(rings, per_ring)], -1).reshape(-1, 4)
  out = np.full((n, 4), np.nan, np.float32)
  out[:len(pts)] = pts
  return out, len(pts)


def calibration():
  cam = {'R_rect_00': np.eye(3).reshape(9)}
  for c, tx in ((2, 44.86), (3, -339.52)):
    cam['P_rect_0%d' % c] = np.array([721.54, 0, 609.56, tx, 0, 721.54, 172.85, 0.22,
                                      0, 0, 1, 0.0027])
  rot = np.array([[0.0076, -0.99997, -0.0006], [0.0148, 0.0007, -0.99989],
                  [0.99986, 0.0076, 0.0148]])
  return cam, (rot, np.array([-0.004, -0.076, -0.272]))


def timed(fn, iters):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(iters):
    fn()
  stop.record()
  stop.synchronize()
  return start.elapsed_time(stop) * 1e3 / iters    # us per call


def traced(fn, calls):
  """name -> (launches per call, mean device time in us), and copies per call."""
  from torch.profiler import profile, ProfilerActivity
  torch.cuda.synchronize()
  with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    for _ in range(calls):
      fn()
    torch.cuda.synchronize()
  rows, copies = {}, 0
  for e in prof.events():
    if not str(e.device_type).endswith('CUDA'):
      continue
    if 'memcpy' in e.name.lower():
      copies += 1
      continue
    short = (re.findall(r'\w+_kernel', e.name) or [e.name[:48]])[-1]
    rows.setdefault(short, []).append(e.device_time if hasattr(e, 'device_time') else e.cuda_time)
  return {k: (len(v) / float(calls), float(np.mean(v))) for k, v in rows.items()}, copies / float(calls)


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default='')
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--scans', type=int, default=4)
  ap.add_argument('--points', type=int, default=120000)
  ap.add_argument('--shape', type=int, nargs=2, default=[256, 768])
  ap.add_argument('--trace_calls', type=int, default=0)
  args = ap.parse_args(argv)
  if not torch.cuda.is_available():
    raise SystemExit('lidar_bench: no ROCm device')
  from lsi.data.kitti import velodyne
  from lsi.geometry import lidar
  dev = torch.device('cuda:0')
  B, N = args.scans, args.points
  H, W = args.shape
  rs = np.random.RandomState(0)
  scans = [synthetic_scan(rs, N) for _ in range(B)]
  pts = torch.from_numpy(np.stack([s[0] for s in scans])).to(dev)
  count = [s[1] for s in scans]
  cam, velo = calibration()
  mat = np.stack([velodyne.velo_to_image(cam, velo, c, (375, 1242, 3), H, W).reshape(12)
                  for c in (2, 3)])
  mats = torch.from_numpy(np.stack([mat] * B)).to(dev)
  kw_on = dict(occl_window=(2, 2), occl_ratio=1.25)

  fns = {
      'hip': lambda: lidar.rasterize_points(pts, None, count, mats, H, W),
      'hip_filter': lambda: lidar.rasterize_points(pts, None, count, mats, H, W, **kw_on),
      'ops': lambda: lidar.rasterize_points_ops(pts, None, count, mats, H, W),
      'ops_filter': lambda: lidar.rasterize_points_ops(pts, None, count, mats, H, W, **kw_on),
  }
  if args.trace_calls:
    for name in ('hip', 'hip_filter'):
      for _ in range(args.trace_calls):
        fns[name]()
    torch.cuda.synchronize()
    return 0
  agree = [bool(torch.equal(fns[a](), fns[b]()))
           for a, b in (('hip', 'ops'), ('hip_filter', 'ops_filter'))]
  filled = float((fns['hip']() != 0).float().mean())
  removed = 1.0 - float((fns['hip_filter']() != 0).float().mean()) / filled
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
  trace = {k: traced(fns[k], 20) for k in ('hip', 'hip_filter', 'ops_filter')}
  point_bytes = 16 * sum(count)
  lines = [
      '%d scans of %d points (padded to %d), 2 views, %d x %d; %.1f %% of the pixels filled, '
      'the (2, 2) x 1.25 filter empties %.1f %% of them' %
      (B, count[0], N, H, W, 100 * filled, 100 * removed),
      'maps of the two routes on these inputs, torch.equal: filter off %s, filter on %s' %
      tuple(agree),
      '%d rounds, alternating; calls per round: %s; us per call, median (min)' %
      (args.rounds, ', '.join('%s %d' % kv for kv in n.items())),
      'HIP, filter off:            3 launches      %9.1f (%.1f)' % (med['hip'], lo['hip']),
      'HIP, filter (2, 2) x 1.25:  3 launches      %9.1f (%.1f)' %
      (med['hip_filter'], lo['hip_filter']),
      'context, torch ops, filter off              %9.1f (%.1f)' % (med['ops'], lo['ops']),
      'context, torch ops, filter (2, 2) x 1.25    %9.1f (%.1f)' %
      (med['ops_filter'], lo['ops_filter']),
      '(a HIP call is timed as the evaluation makes it: the Python binding, its checks and the',
      ' upload of the scan descriptors, not the kernels alone)',
      'profiler trace of 20 calls: launches per call x mean device time, us',
  ]
  for k in ('hip', 'hip_filter', 'ops_filter'):
    kernels, copies = trace[k]
    total = sum(c * t for c, t in kernels.values())
    lines.append('  %-11s %5.1f kernels, %.1f copies per call, %.1f us on the device' %
                 (k, sum(c for c, _ in kernels.values()), copies, total))
    if k.startswith('hip'):
      for name in sorted(kernels):
        lines.append('      %4.1f x %-28s %8.2f' % (kernels[name][0], name, kernels[name][1]))
  scatter = trace['hip'][0]['scatter_kernel'][1]
  lines += [
      'scatter: %.2f MB of points (16 B each) in %.2f us = %.3f TB/s, %.1f %% of the %.1f TB/s '
      'HBM peak' % (point_bytes / 1e6, scatter, point_bytes / scatter / 1e6,
                    100 * point_bytes / scatter / 1e6 / HBM_TBS, HBM_TBS),
  ]
  text = '\n'.join(lines) + '\n'
  sys.stdout.write(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text)
  return 0


if __name__ == '__main__':
  sys.exit(main())
