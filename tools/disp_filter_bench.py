"""Times the disparity post-filters (csrc/lsi_disp_filter.hip through
lsi.geometry.stereo.filter_disparity) on the two maps of one KITTI-sized pair
in one call (B = 2), kernel by kernel, then the matcher with the filters on
against off, then the preprocessing tool with the filters on against off.

    python tools/disp_filter_bench.py [--out FILE] [--rounds 5] [--shape 375 1242]
                                      [--pairs 48] [--skip_host]

Inputs of the filter call: the matcher's own output for the generated pair of
tools/sgm_bench.py (D = 128, 8 paths); an all-valid constant map (one component
over every tile); and a one-pixel-wide serpentine (every even row whole, joined
at alternate ends: the longest chains the union can meet).  Method as in
tools/sgm_bench.py: device events around back-to-back calls, at least 50 ms per
round, the median over the rounds (and the minimum), the Python binding
included; per kernel the device durations out of a torch profiler trace of 5
calls, the median per launch position.  The tool: pairs per second over --pairs
generated pairs with 16 threads, filters off and on in alternating rounds (the
rate is bound by PNG encoding on the host and wanders from run to run: every
round is printed), and what the encoder alone makes of either kind of map on the
same threads with the device idle.  As context only, the SciPy statement of
tests/disp_filter_ref.py on the host for the matcher's maps."""
import argparse
import os
import shutil
import sys
import tempfile
import time
from concurrent import futures

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'layered-scene-inference_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from sgm_bench import kernel_times, street_pair, timed  # noqa: E402

FILTERS = dict(median=3, speckle_size=20, speckle_range=256)


def measure(fns, rounds):
  """{key: (median us, min us, calls per round)} -- the rounds interleaved."""
  iters = {}
  for k, fn in fns.items():
    timed(fn, 3)
    iters[k] = max(int(60e3 / timed(fn, 3)) + 1, 3)
  rows = {k: [] for k in fns}
  for _ in range(rounds):
    for k, fn in fns.items():
      rows[k].append(timed(fn, iters[k]))
  return {k: (float(np.median(v)), float(np.min(v)), iters[k]) for k, v in rows.items()}


def serpentine(h, w, value=512):
  img = np.zeros((h, w), np.uint16)
  img[0::2] = value
  for i, y in enumerate(range(1, h - 1, 2)):
    img[y, w - 1 if i % 2 == 0 else 0] = value
  return img


def tool_rates(h, w, pairs, threads, rounds, lines):
  from PIL import Image
  from lsi.data.kitti import data as kitti
  from lsi.data.kitti import preprocess
  root = tempfile.mkdtemp(prefix='disp_filter_bench_')
  try:
    seq = kitti.raw_city_sequences()[0]
    base = os.path.join(root, 'kitti_raw', seq[:10], seq + '_sync')
    variants = [street_pair(100 + i, h, w) for i in range(4)]
    for n in range(pairs):
      for cam, img in zip(('image_02', 'image_03'), variants[n % 4]):
        path = os.path.join(base, cam, 'data', '%010d.png' % n)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(np.roll(img, n, axis=0)).save(path)
    modes = (('off', {}), ('on', FILTERS))
    rates, mb = {'off': [], 'on': []}, {}
    for name, kw in modes:
      preprocess.run(root, workers=threads, sequences=[seq], overwrite=True, **kw)   # warm-up
    for _ in range(rounds):
      for name, kw in modes:
        torch.cuda.synchronize()
        t = time.perf_counter()
        preprocess.run(root, workers=threads, sequences=[seq], overwrite=True, **kw)
        rates[name].append(pairs / (time.perf_counter() - t))
        mb[name] = sum(os.path.getsize(q) for p in preprocess.left_images(root, [seq])
                       for q in preprocess.disparity_paths(root, p)) / 1e6 / pairs
    lines.append('the tool on %d generated pairs of %d x %d, %d threads, max_disp 128, 8 paths, '
                 'end to end, %d alternating rounds' % (pairs, h, w, threads, rounds))
    for name, _ in modes:
      med = float(np.median(rates[name]))
      lines.append('  filters %-4s %7.1f pairs / s, median (%.2f ms per pair; rounds: %s; %.2f MB '
                   'of map PNGs per pair)' % (
                       name, med, 1e3 / med, ' '.join('%.1f' % r for r in rates[name]), mb[name]))
    # what the encoder makes of either kind of map, the device idle
    lefts = preprocess.left_images(root, [seq])
    enc = {'off': [], 'on': []}
    with futures.ThreadPoolExecutor(threads) as pool:
      kinds = {}
      for name, kw in modes:
        preprocess.run(root, workers=threads, sequences=[seq], overwrite=True, **kw)
        kinds[name] = [[np.asarray(Image.open(q)).astype(np.uint16)
                        for q in preprocess.disparity_paths(root, p)] for p in lefts[:8]]
      out = os.path.join(root, 'encode_only')
      for _ in range(rounds):
        for name, _ in modes:
          def encode(n, maps=kinds[name]):
            for side, m in zip('lr', maps[n % len(maps)]):
              preprocess.write_disparity_png(os.path.join(out, '%d_%s.png' % (n, side)), m)
          t = time.perf_counter()
          list(pool.map(encode, range(pairs)))
          enc[name].append(pairs / (time.perf_counter() - t))
    for name, _ in modes:
      med = float(np.median(enc[name]))
      lines.append('  encoding alone, maps written with filters %-4s %7.1f pairs / s, median (%.2f ms '
                   'per pair; rounds: %s)' % (name, med, 1e3 / med,
                                              ' '.join('%.1f' % r for r in enc[name])))
  finally:
    shutil.rmtree(root, ignore_errors=True)


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default='')
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--shape', type=int, nargs=2, default=[375, 1242])
  ap.add_argument('--pairs', type=int, default=48)
  ap.add_argument('--skip_host', action='store_true')
  args = ap.parse_args(argv)
  if not torch.cuda.is_available():
    raise SystemExit('disp_filter_bench: no ROCm device')
  from lsi.geometry import stereo
  dev = torch.device('cuda:0')
  h, w = args.shape
  left_np, right_np = street_pair(0, h, w)
  left, right = torch.from_numpy(left_np).to(dev), torch.from_numpy(right_np).to(dev)
  # (through NumPy: torch has few uint16 operators)
  sgm_np = np.stack([m.cpu().numpy() for m in stereo.sgm_disparity(left, right, max_disp=128)])
  sgm = torch.from_numpy(sgm_np).to(dev)
  maps = {
      'matcher output': sgm,
      'constant': torch.from_numpy(np.full((2, h, w), 5000, np.uint16)).to(dev),
      'serpentine': torch.from_numpy(np.stack([serpentine(h, w)] * 2)).to(dev),
  }
  lines = ['post-filters of the two %d x %d maps of one pair in one call (B = 2): median 3, '
           'speckle_size 20, speckle_range 256' % (h, w),
           '%d rounds; us per call, median (min); per kernel: median us over 5 traced calls' %
           args.rounds]
  configs = [('median + speckle', FILTERS), ('speckle only', dict(FILTERS, median=0)),
             ('median only', dict(FILTERS, speckle_size=0))]
  for name, m in maps.items():
    fns = {c: (lambda kw=kw, m=m: stereo.filter_disparity(m, **kw)) for c, kw in configs}
    res = measure(fns, args.rounds)
    out = fns['median + speckle']()
    lines.append('%s: %.1f %% valid, %.1f %% after the filters; workspace %.1f MB' % (
        name, 100 * float((m.cpu().numpy() != 0).mean()),
        100 * float((out.cpu().numpy() != 0).mean()),
        stereo.filter_workspace_bytes(2, h, w, 3, 20) / 1e6))
    for c, _ in configs:
      lines.append('  %-18s %8.1f (%.1f) us per call, %d calls per round' % ((c,) + res[c]))
    for kname, us in kernel_times(fns['median + speckle']):
      lines.append('    %-16s %8.1f us' % (kname, us))
  fns = {'off': lambda: stereo.sgm_disparity(left, right, max_disp=128),
         'on': lambda: stereo.sgm_disparity(left, right, max_disp=128, **FILTERS)}
  res = measure(fns, args.rounds)
  lines.append('sgm_disparity, one pair, D = 128, 8 paths, measured in the same rounds:')
  lines.append('  filters off        %8.1f (%.1f) us per call, %d calls per round' % res['off'])
  lines.append('  filters on         %8.1f (%.1f) us per call, %d calls per round' % res['on'])
  lines.append('  the filters add %.1f us = %.1f %% of the unfiltered call' % (
      res['on'][0] - res['off'][0], 100 * (res['on'][0] - res['off'][0]) / res['off'][0]))
  if not args.skip_host:
    import disp_filter_ref as F
    host = sgm_np
    t = time.perf_counter()
    want = F.filter_batch(host, sizes=F.component_sizes_scipy, **FILTERS)
    t_host = time.perf_counter() - t
    same = np.array_equal(want, stereo.filter_disparity(sgm, **FILTERS).cpu().numpy())
    lines.append('context, the NumPy / SciPy statement on the host for the matcher\'s two maps: '
                 '%.0f ms (same bits as the kernels: %s)' % (1e3 * t_host, same))
  tool_rates(h, w, args.pairs, 16, args.rounds, lines)
  text = '\n'.join(lines) + '\n'
  sys.stdout.write(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text)
  return 0


if __name__ == '__main__':
  sys.exit(main())
