"""Writes the disparity maps the KITTI raw_city loader reads as ground truth
(data.DataLoader with kitti_dl_disparities / kitti_dl_disparities_px):

    python -m lsi.data.kitti.preprocess --kitti_data_root ROOT
        [--max_disp 128 --p1 10 --p2 120 --paths 8 --uniqueness 95 --lr_max 1]
        [--median 0 --speckle_size 0 --speckle_range 256]
        [--workers 8 --overwrite false --sequences a,b,...]

For every stereo pair of the raw_city sequences (the frame the loader excludes
is skipped) it decodes image_02 / image_03 on a pool of threads, runs the
semi-global matcher of lsi.geometry.stereo on the device at the files' own
resolution, optionally post-filters both maps there (--median 3: a 3 x 3 median
of the valid values; --speckle_size N: components of at most N pixels are
removed; both off by default), and writes both views'
maps as 16-bit PNGs (disparity * 256, 0 = no match) to

    ROOT/kitti_raw/spss_stereo_results/<sequence>_sync/
        <frame>_{left,right}_initial_disparity.png

-- the paths data.DataLoader builds.  The reference produces these files with an
external SPS-stereo executable; the maps written here are this project's own
matcher's output in the same format, not SPS-stereo's.
With --overwrite false a file that exists is kept whatever settings and filters
it was written with.

The device never waits for a PNG: decodes run ahead of the matcher, and a
result's download is only waited for by the worker thread that encodes it.
"""
import argparse
import collections
import fnmatch
import os
import sys
import time
from concurrent import futures

import numpy as np

from lsi.data.kitti import data as kitti_data
from lsi.data.kitti import pipeline

EXCLUDED = '2011_09_26_drive_0117_sync/image_02/data/0000000074.png'


def left_images(root, sequences=None):
  """The image_02 files of the raw_city sequences under root/kitti_raw, named as
  data.DataLoader names them, without the excluded frame."""
  top = os.path.join(root, 'kitti_raw')
  out = []
  for seq in (sequences if sequences is not None else kitti_data.raw_city_sequences()):
    seq_dir = os.path.join(top, seq[0:10], '{}_sync'.format(seq))
    for base, _, names in os.walk(os.path.join(seq_dir, 'image_02')):
      for name in sorted(fnmatch.filter(names, '*.png')):
        path = os.path.join(base, name)
        if EXCLUDED not in path:
          out.append(path)
  return out


def right_image(left_path):
  return left_path.replace('image_02', 'image_03')


def disparity_paths(root, left_path):
  """(left map, right map) of the pair whose left image is left_path: what
  data.DataLoader puts into img_list_disp_src / img_list_disp_trg."""
  parts = left_path.split('/')
  left = os.path.join(root, 'kitti_raw', 'spss_stereo_results', parts[-4],
                      parts[-1][:-4] + '_left_initial_disparity.png')
  return left, left.replace('left', 'right')


def write_disparity_png(path, u16):
  """A H x W uint16 array as a 16-bit greyscale PNG, complete or absent."""
  from PIL import Image  # pylint: disable=g-import-not-at-top
  arr = np.ascontiguousarray(u16)
  if arr.dtype != np.uint16 or arr.ndim != 2:
    raise ValueError('a disparity map is a 2-D uint16 array, got %s %s' %
                     (arr.dtype, arr.shape))
  os.makedirs(os.path.dirname(path), exist_ok=True)
  tmp = path + '.part'
  Image.fromarray(arr).save(tmp, format='PNG')
  os.replace(tmp, path)


def _decode_pair(left_path):
  left = pipeline.decode_u8(left_path, 3)
  right = pipeline.decode_u8(right_image(left_path), 3)
  if left.shape != right.shape:
    raise ValueError('%s is %s, its right image %s' % (left_path, left.shape, right.shape))
  return left.copy(), right.copy()   # (writable and contiguous: torch.from_numpy)


def _encode_pair(event, host_l, host_r, out_l, out_r):
  event.synchronize()            # the download of this pair, nothing later
  write_disparity_png(out_l, host_l.numpy())
  write_disparity_png(out_r, host_r.numpy())


def run(root, max_disp=128, p1=10, p2=120, paths=8, uniqueness=95, lr_max=1, workers=8,
        overwrite=False, sequences=None, device='cuda', log=None, median=0,
        speckle_size=0, speckle_range=256):
  """Matches every pair under `root`; returns (pairs written, pairs skipped).
  median, speckle_size, speckle_range: stereo.filter_disparity's, off by default."""
  import torch  # pylint: disable=g-import-not-at-top
  from lsi.geometry import stereo  # pylint: disable=g-import-not-at-top
  dev = torch.device(device)
  if dev.type != 'cuda' or not torch.cuda.is_available():
    raise RuntimeError('the matcher runs as HIP kernels and needs a ROCm GPU (got '
                       'device %s); there is no CPU fallback' % dev)
  todo, skipped = [], 0
  for left in left_images(root, sequences):
    outs = disparity_paths(root, left)
    if not overwrite and all(os.path.exists(p) for p in outs):
      skipped += 1
    else:
      todo.append((left, outs))
  n_threads = pipeline.pool_size(workers)
  ahead = 2 * n_threads          # pairs decoded ahead; results waiting for a thread
  decodes, encodes = collections.deque(), collections.deque()
  nxt = 0
  with futures.ThreadPoolExecutor(n_threads, thread_name_prefix='kitti-sgm') as pool:
    try:
      for i, (left, outs) in enumerate(todo):
        while nxt < len(todo) and len(decodes) < ahead:
          decodes.append(pool.submit(_decode_pair, todo[nxt][0]))
          nxt += 1
        try:
          img_l, img_r = decodes.popleft().result()
        except Exception as e:  # pylint: disable=broad-except
          raise pipeline._named(left, e)  # pylint: disable=protected-access
        with torch.cuda.device(dev):
          d_l, d_r = stereo.sgm_disparity(
              torch.from_numpy(img_l).to(dev), torch.from_numpy(img_r).to(dev),
              max_disp, p1, p2, paths, uniqueness, lr_max, median, speckle_size,
              speckle_range)
          host_l = torch.empty(d_l.shape, dtype=torch.uint16, pin_memory=True)
          host_r = torch.empty(d_r.shape, dtype=torch.uint16, pin_memory=True)
          host_l.copy_(d_l, non_blocking=True)
          host_r.copy_(d_r, non_blocking=True)
          event = torch.cuda.Event()
          event.record()
        encodes.append(pool.submit(_encode_pair, event, host_l, host_r, *outs))
        while encodes and (encodes[0].done() or len(encodes) > ahead):
          encodes.popleft().result()   # (an encode error surfaces here)
        if log is not None and (i + 1) % 100 == 0:
          log('%d / %d pairs' % (i + 1, len(todo)))
      while encodes:
        encodes.popleft().result()
    finally:
      for f in list(decodes) + list(encodes):
        f.cancel()
  return len(todo), skipped


def _bool(text):
  if text.lower() in ('true', '1', 'yes'):
    return True
  if text.lower() in ('false', '0', 'no'):
    return False
  raise argparse.ArgumentTypeError('true or false, got %r' % text)


def build_parser():
  p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
  p.add_argument('--kitti_data_root', required=True)
  p.add_argument('--max_disp', type=int, default=128,
                 help='number of disparities: a multiple of 16 in [16, 256]')
  p.add_argument('--p1', type=int, default=10)
  p.add_argument('--p2', type=int, default=120)
  p.add_argument('--paths', type=int, default=8, choices=(4, 8))
  p.add_argument('--uniqueness', type=int, default=95)
  p.add_argument('--lr_max', type=int, default=1)
  p.add_argument('--workers', type=int, default=8,
                 help='decode / encode threads, at most %d' % pipeline.MAX_THREADS)
  p.add_argument('--median', type=int, default=0, choices=(0, 3),
                 help='3: a 3 x 3 median over the valid values after the matcher; 0: off')
  p.add_argument('--speckle_size', type=int, default=0,
                 help='remove connected components of at most this many pixels; 0: off')
  p.add_argument('--speckle_range', type=int, default=256,
                 help='neighbours belong to one component when they differ by at most '
                      'this much, in 1/256 px')
  p.add_argument('--overwrite', type=_bool, default=False,
                 help='false skips a pair whose files exist, whatever settings and '
                      'filters they were written with')
  p.add_argument('--sequences', default='',
                 help='comma-separated sequence names; default: all of raw_city')
  p.add_argument('--device', default='cuda')
  return p


def main(argv=None):
  a = build_parser().parse_args(argv)
  seqs = [s for s in a.sequences.split(',') if s] or None
  t0 = time.time()
  done, skipped = run(a.kitti_data_root, a.max_disp, a.p1, a.p2, a.paths, a.uniqueness,
                      a.lr_max, a.workers, a.overwrite, seqs, a.device,
                      log=lambda m: print(m, flush=True), median=a.median,
                      speckle_size=a.speckle_size, speckle_range=a.speckle_range)
  print('%d pairs matched, %d already there, %.1f s' % (done, skipped, time.time() - t0))
  return 0


if __name__ == '__main__':
  sys.exit(main())
