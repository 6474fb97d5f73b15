"""Feed rate of the KITTI loaders against the training step they feed.

Writes a KITTI-shaped raw_city tree of procedural PNGs (ragged sizes around
375 x 1242, one per sequence; nothing is downloaded) and reports, for batch 4
at 256 x 768 on this host, in this run:
  * the synchronous loader (data.DataLoader inside KittiBatches): the baseline;
  * pipeline.PrefetchLoader, resize on the host, at 2, 4, 8 and 16 threads;
  * the same with the resize on the device (csrc/lsi_image.hip);
  * the HIP-event time of the resize launch alone and the bytes it moves;
  * where one image's host time goes (decode / resize);
  * the 2- and 4-layer training step on procedural pairs (tools/train_bench.py's
    measurement), and the 2-layer step fed from the tree by both loaders, eager
    and as a captured HIP graph.
  python tools/data_bench.py [--out FILE] [--batches N] [--skip_steps] [--kernel_only]

--augment [--parent_lib SO] measures the augmenting launch instead
(lsi_augment_resize_u8): the plain launch, the augmenting launch
at identity parameters and at a typical draw (zoom 1.1, flip, tone table,
gains), alternated in one process over --rounds rounds of HIP-event medians;
with --parent_lib also the lsi_area_resize_u8 of another build (a shared
library made from an earlier csrc/lsi_image.hip), whose range over the rounds is
the run-to-run spread the others are read against.  Then the device-route loader
at 16 threads with --kitti_augment off and on.

--gt [--parent_pkg DIR] measures --kitti_gt_everywhere on the
same tree with 16-bit disparity maps and 120 000-point scans added: the
lsi_augment_sample_u16 launch on 8 maps beside the lsi_area_resize_u8 launch,
the loaders with pixel disparities and with Velodyne scans (prefetching, device
route, 16 threads; synchronous with the flag), the prefetching loader without
ground truth, and the training step fed from the files with the term on.  Then
the device-route loader with the flag off, one child process per figure, over
--rounds rounds; with --parent_pkg (the package directory of a checkout of the
previous commit, its library built) the two builds alternate.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (--gt's child processes measure another checkout's package: LSI_BENCH_PKG)
sys.path.insert(0, os.environ.get('LSI_BENCH_PKG') or
                os.path.join(ROOT, 'layered-scene-inference_amd'))

from lsi.data.kitti import data as kitti_data  # noqa: E402
from lsi.data.kitti import pipeline  # noqa: E402

SIZES = [(375, 1242), (370, 1226), (374, 1238), (376, 1241)]  # KITTI raw dates
PAIRS_PER_SEQ = 6
H, W, BS = 256, 768, 4


def procedural_png(path, h, w, seed):
  """A smooth random texture plus sensor-like noise: compresses to about two
  thirds of its raw size, as a photograph does."""
  from PIL import Image
  rs = np.random.RandomState(seed)
  lo = rs.rand(h // 16 + 2, w // 16 + 2, 3)
  yy = np.linspace(0, lo.shape[0] - 1.001, h)
  xx = np.linspace(0, lo.shape[1] - 1.001, w)
  y0, x0 = yy.astype(int), xx.astype(int)
  fy, fx = (yy - y0)[:, None, None], (xx - x0)[None, :, None]
  img = ((lo[y0][:, x0] * (1 - fx) + lo[y0][:, x0 + 1] * fx) * (1 - fy) +
         (lo[y0 + 1][:, x0] * (1 - fx) + lo[y0 + 1][:, x0 + 1] * fx) * fy)
  img = img * 255 + rs.randint(-6, 7, (h, w, 3))
  os.makedirs(os.path.dirname(path), exist_ok=True)
  Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(path)


def procedural_disparity(path, h, w, seed):
  """A smooth 16-bit disparity map (value = disparity * 256), a left band and
  scattered pixels without a match."""
  from PIL import Image
  rs = np.random.RandomState(seed)
  lo = rs.uniform(2, 90, (h // 32 + 2, w // 32 + 2))
  d = np.kron(lo, np.ones((32, 32)))[:h, :w] + rs.uniform(-0.5, 0.5, (h, w))
  d[:, :w // 8] = 0
  d[rs.rand(h, w) < 0.1] = 0
  os.makedirs(os.path.dirname(path), exist_ok=True)
  Image.fromarray(np.rint(d * 256).astype(np.uint16)).save(path)


N_POINTS = 120000


def write_gt(root, seq, n, h, w, seed):
  """The two disparity maps and the scan of frame n of `seq`."""
  top = os.path.join(root, 'kitti_raw')
  for k, side in enumerate(('left', 'right')):
    procedural_disparity(os.path.join(top, 'spss_stereo_results', seq + '_sync',
                                      '%010d_%s_initial_disparity.png' % (n, side)),
                         h, w, seed + k)
  rs = np.random.RandomState(seed + 2)
  x = rs.uniform(3, 80, N_POINTS)
  scan = np.stack([x, rs.uniform(-0.9, 0.9, N_POINTS) * x, rs.uniform(-0.3, 0.1, N_POINTS) * x,
                   rs.rand(N_POINTS)], 1).astype(np.float32)
  path = os.path.join(top, seq[:10], seq + '_sync', 'velodyne_points', 'data', '%010d.bin' % n)
  os.makedirs(os.path.dirname(path), exist_ok=True)
  scan.tofile(path)


def write_tree(root, gt=False):
  opts = loader_opts(root)
  seqs = kitti_data.DataLoader(opts).split_sequences()[:len(SIZES)]
  top = os.path.join(root, 'kitti_raw')
  n_bytes = 0
  for s, (seq, (h, w)) in enumerate(zip(seqs, SIZES)):
    date = seq[:10]
    for n in range(PAIRS_PER_SEQ):
      for cam in ('image_02', 'image_03'):
        path = os.path.join(top, date, seq + '_sync', cam, 'data', '%010d.png' % n)
        procedural_png(path, h, w, 1000 * s + 2 * n + (cam == 'image_03'))
        n_bytes += os.path.getsize(path)
      if gt:
        write_gt(root, seq, n, h, w, 5000 * s + 3 * n)
    with open(os.path.join(top, date, 'calib_cam_to_cam.txt'), 'w') as f:
      p = '721.5 0 609.6 %f 0 721.5 172.9 0 0 0 1 0'
      f.write('P_rect_02: %s\nP_rect_03: %s\n' % (p % 44.86, p % -339.5))
      if gt:
        f.write('R_rect_00: 1 0 0 0 1 0 0 0 1\n')
    if gt:
      with open(os.path.join(top, date, 'calib_velo_to_cam.txt'), 'w') as f:
        f.write('R: 0 -1 0 0 0 -1 1 0 0\nT: 0 -0.08 -0.27\n')
  return n_bytes / (2.0 * PAIRS_PER_SEQ * len(SIZES))


def loader_opts(root, **more):
  return types.SimpleNamespace(
      batch_size=BS, kitti_data_root=root, kitti_dataset_variant='raw_city',
      data_split='train', img_height=H, img_width=W, kitti_dl_disparities=False,
      **more)


def time_loader(make, batches, warm=2):
  """ms per batch of forward(BS), the device idle at the end of the clock."""
  ld = make()
  try:
    for _ in range(warm):
      ld.forward(BS)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(batches):
      out = ld.forward(BS)
    torch.cuda.synchronize()
    del out
    return (time.perf_counter() - t0) * 1e3 / batches
  finally:
    close = getattr(ld, 'close', None)
    if close is not None:
      close()


def time_kernel(root, reps=20):
  """HIP-event time of one lsi_area_resize_u8 launch on 8 images of the tree."""
  ld = kitti_data.DataLoader(loader_opts(root))
  paths = [p for i in range(0, len(ld.img_list_src), PAIRS_PER_SEQ)
           for p in (ld.img_list_src[i], ld.img_list_trg[i])][:2 * BS]
  st = pipeline._Staging(len(paths), sum(
      pipeline._round16(h * w * 3) for h, w in SIZES) * 2)
  stop = __import__('threading').Event()
  for slot, p in enumerate(paths):
    pipeline._device_task(stop, p, 3, st, slot)
  used = st.used + 16
  packed = torch.empty(used, dtype=torch.uint8, device='cuda')
  packed.copy_(st.tensor[:used])
  out = torch.empty((len(paths), H, W, 3), device='cuda')
  run = lambda: pipeline.area_resize_u8(packed, st.desc, packed.data_ptr(),
                                        len(paths), H, W, 3, out=out)
  for _ in range(3):
    run()
  torch.cuda.synchronize()
  times = []
  for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1) * 1e3)
  moved = int(st.desc['H'].astype(np.int64) @ st.desc['W'] * 3) + out.numel() * 4
  return float(np.median(times)), float(min(times)), moved, used


def _event_median(run, reps):
  times = []
  for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1) * 1e3)
  return float(np.median(times))


def time_augment_launches(root, parent_lib='', rounds=7, reps=40):
  """us per launch on 8 images of the tree, HIP events: {variant: [median of
  `reps` launches, one per round]}; the variants alternate inside a round."""
  import ctypes
  from lsi import _C
  from lsi.data.kitti import augment
  ld = kitti_data.DataLoader(loader_opts(root))
  paths = [p for i in range(0, len(ld.img_list_src), PAIRS_PER_SEQ)
           for p in (ld.img_list_src[i], ld.img_list_trg[i])][:2 * BS]
  n = len(paths)
  cap = sum(pipeline._round16(h * w * 3) for h, w in SIZES) * 2
  stop = __import__('threading').Event()
  # one buffer per descriptor layout, the same pixels in both
  plain = pipeline._Staging(n, cap)
  aug = {k: pipeline._Staging(n, cap, n_tables=n // 2, dtype=pipeline.AUG_DESC_DTYPE)
         for k in ('identity', 'typical')}
  for st in [plain] + list(aug.values()):
    for slot, p in enumerate(paths):
      pipeline._device_task(stop, p, 3, st, slot)
  draw = augment.IDENTITY._replace(flip=True, zoom_y=1.1, zoom_x=1.1, off_y=0.5,
                                   off_x=0.5, gamma=0.9, brightness=1.2,
                                   color=(0.9, 1.0, 1.1))
  for key, st in aug.items():
    d = st.desc
    d['flags'], d['table'], d['gain'] = 0, -1, 1.0
    d['y0'], d['x0'], d['ch'], d['cw'] = 0, 0, d['H'], d['W']
    d['reserved'], d['reserved2'] = 0, 0
    if key == 'typical':
      table, gains = augment.image_params(draw, 3)
      st.tables[...] = table
      for m in range(n):
        rec = d[m:m + 1]
        rec['y0'], rec['x0'], rec['ch'], rec['cw'] = augment.window(
            draw, int(d['H'][m]), int(d['W'][m]))
        rec['flags'], rec['table'], rec['gain'] = pipeline.AUG_FLIP, m // 2, gains

  def upload(st):
    used = st.used + 16
    packed = torch.empty(used, dtype=torch.uint8, device='cuda')
    packed.copy_(st.tensor[:used])
    return packed
  out = torch.empty((n, H, W, 3), device='cuda')
  runs = {}
  pk = upload(plain)
  if parent_lib:
    parent = ctypes.CDLL(os.path.abspath(parent_lib))
    parent.lsi_area_resize_u8.restype = ctypes.c_int
    parent.lsi_area_resize_u8.argtypes = (
        [ctypes.c_int32] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t] +
        [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 2)
  # (every variant is one bare ctypes call on prepared arguments: the same
  # host work inside the timed window)
  stream = _C.stream_ptr(pk.device)
  hosts = []

  def call(fn, st, packed, *extra):
    host = np.ascontiguousarray(st.desc)
    hosts.append(host)
    args = (n, host.ctypes.data, packed.data_ptr(), packed.data_ptr(),
            packed.numel()) + extra + (H, W, 3, out.data_ptr(), stream)

    def run():
      rc = fn(*args)
      assert rc == 0, rc
    return run
  if parent_lib:
    runs['parent_plain'] = call(parent.lsi_area_resize_u8, plain, pk)
  runs['plain'] = call(_C.lib().lsi_area_resize_u8, plain, pk)
  packed = {k: upload(st) for k, st in aug.items()}
  for key, st in aug.items():
    runs['augment_' + key] = call(_C.lib().lsi_augment_resize_u8, st, packed[key],
                                  st.tables_offset, st.n_tables)
  # the same seeded inputs, the same bits: parent = plain = augment at identity
  ref = None
  for key in ('parent_plain', 'plain', 'augment_identity'):
    if key in runs:
      runs[key]()
      got = out.clone()
      assert ref is None or torch.equal(got, ref), key
      ref = got
  for run in runs.values():
    for _ in range(5):
      run()
  torch.cuda.synchronize()
  times = {k: [] for k in runs}
  for _ in range(rounds):
    for key, run in runs.items():
      times[key].append(_event_median(run, reps))
  px = {'plain': int(plain.desc['H'].astype(np.int64) @ plain.desc['W'])}
  for key, st in aug.items():
    px['augment_' + key] = int(st.desc['ch'].astype(np.int64) @ st.desc['cw'])
  px['parent_plain'] = px['plain']
  moved = {k: px[k] * 3 + out.numel() * 4 for k in runs}
  return times, moved


def time_sample_launch(root, rounds=9, reps=40):
  """us per launch, HIP events: lsi_augment_sample_u16 on 8 maps of the tree (a
  typical draw: zoom 1.1 centred, flipped) and lsi_area_resize_u8 on its 8
  images, alternated; [median of `reps` launches per round]."""
  from lsi.data.kitti import augment
  ld = kitti_data.DataLoader(loader_opts(root, kitti_dl_disparities_px=True,
                                         kitti_gt_everywhere=True))
  ids = list(range(0, len(ld.img_list_src), PAIRS_PER_SEQ))[:BS]
  imgs = [p for i in ids for p in (ld.img_list_src[i], ld.img_list_trg[i])]
  maps = [lst[i] for lst in (ld.img_list_disp_src, ld.img_list_disp_trg) for i in ids]
  cap = sum(pipeline._round16(h * w * 3) + pipeline._round16(h * w * 2) + 32
            for h, w in SIZES) * 2
  st = pipeline._Staging(len(imgs), cap, n_maps=len(maps))
  stop = __import__('threading').Event()
  for slot, p in enumerate(imgs):
    pipeline._device_task(stop, p, 3, st, slot)
  for slot, p in enumerate(maps):
    assert pipeline._device_px_task(stop, p, st, slot)[1] is None
  draw = augment.IDENTITY._replace(flip=True, zoom_y=1.1, zoom_x=1.1, off_y=0.5, off_x=0.5)
  d = st.map_desc
  d['table'], d['gain'], d['reserved'], d['reserved2'] = -1, 1.0, 0, 0
  for m in range(len(maps)):
    rec = d[m:m + 1]
    rec['y0'], rec['x0'], rec['ch'], rec['cw'] = augment.window(
        draw, int(d['H'][m]), int(d['W'][m]))
    rec['flags'] = pipeline.AUG_FLIP
  used = st.used + 16
  packed = torch.empty(used, dtype=torch.uint8, device='cuda')
  packed.copy_(st.tensor[:used])
  out3 = torch.empty((len(imgs), H, W, 3), device='cuda')
  out1 = torch.empty((len(maps), H, W, 1), device='cuda')
  runs = {
      'area_resize_u8': lambda: pipeline.area_resize_u8(
          packed, st.desc, packed.data_ptr(), len(imgs), H, W, 3, out=out3),
      'augment_sample_u16': lambda: pipeline.augment_sample_u16(
          packed, st.map_desc, packed.data_ptr() + st.maps_offset, len(maps), H, W,
          out=out1)}
  for run in runs.values():
    for _ in range(5):
      run()
  torch.cuda.synchronize()
  times = {k: [] for k in runs}
  for _ in range(rounds):
    for key, run in runs.items():
      times[key].append(_event_median(run, reps))
  moved = {'area_resize_u8': int(st.desc['H'].astype(np.int64) @ st.desc['W']) * 3 +
                             out3.numel() * 4,
           'augment_sample_u16': out1.numel() * (4 + 2)}   # one gather per output pixel
  return times, moved


def flag_off_child(root, batches):
  """One figure: ms per batch of the device-route loader, 16 threads, no ground
  truth, no flag (the package under LSI_BENCH_PKG)."""
  import ldi_enc_dec as script
  ms = time_loader(lambda: script.KittiBatches(pipeline.PrefetchLoader(
      kitti_data.DataLoader(loader_opts(root)), workers=16, resize='device',
      device=torch.device('cuda', 0))), batches)
  print('FLAG_OFF_MS %.4f' % ms, flush=True)


def flag_off_rounds(root, rounds, batches, parent_pkg=''):
  """{build: [ms per batch, one child process each]}, the builds alternating."""
  pkgs = {'this': os.path.join(ROOT, 'layered-scene-inference_amd')}
  if parent_pkg:
    pkgs = {'parent': os.path.abspath(parent_pkg), 'this': pkgs['this']}
  out = {k: [] for k in pkgs}
  for _ in range(rounds):
    for key, pkg in pkgs.items():
      env = dict(os.environ, LSI_BENCH_PKG=pkg)
      res = subprocess.run([sys.executable, os.path.abspath(__file__), '--flag_off_child',
                            root, '--batches', str(batches)], env=env, timeout=300,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
      if res.returncode != 0:
        raise RuntimeError('the %s child failed (%d):\n%s' % (key, res.returncode,
                                                              res.stdout[-2000:]))
      out[key].append(float(res.stdout.split('FLAG_OFF_MS')[1].split()[0]))
  return out


def run_gt(args, say, rec):
  import ldi_enc_dec as script
  with tempfile.TemporaryDirectory(prefix='lsi_kitti_gt_tree_') as root:
    png = write_tree(root, gt=True)
    say('tree: %d sequences x %d pairs, sizes %s, mean PNG %.0f kB, 16-bit maps, %d-point '
        'scans; batch %d -> %d x %d' % (len(SIZES), PAIRS_PER_SEQ, SIZES, png / 1e3,
                                        N_POINTS, BS, H, W))
    rounds = max(9, args.rounds)
    times, moved = time_sample_launch(root, rounds)
    say('launches, HIP events, us: median of the %d round medians [min .. max]' % rounds)
    for key, t in times.items():
      say('  %-20s %6.1f  [%5.1f .. %5.1f]  %.1f MB' % (
          key, float(np.median(t)), min(t), max(t), moved[key] / 1e6))
    rec['launch_us'] = times
    dev0 = torch.device('cuda', 0)
    pre = lambda **kw: script.KittiBatches(pipeline.PrefetchLoader(
        kitti_data.DataLoader(loader_opts(root, **kw)), workers=16, resize='device',
        device=dev0))
    sync = lambda **kw: script.KittiBatches(kitti_data.DataLoader(loader_opts(root, **kw)))
    px = dict(kitti_dl_disparities_px=True, kitti_gt_everywhere=True)
    velo = dict(kitti_dl_velodyne=True, kitti_gt_everywhere=True)
    rec['loader_ms_per_batch'] = {}
    for name, make in (
        ('prefetching, device route, 16 threads, no ground truth', lambda: pre(kitti_augment=True)),
        ('prefetching, device route, 16 threads, px', lambda: pre(kitti_augment=True, **px)),
        ('prefetching, device route, 16 threads, velodyne',
         lambda: pre(kitti_augment=True, **velo)),
        ('synchronous with the flag, px', lambda: sync(kitti_augment=True, **px)),
        ('synchronous with the flag, velodyne', lambda: sync(kitti_augment=True, **velo)),
        ('synchronous, no ground truth', lambda: sync(kitti_augment=True))):
      ms = [time_loader(make, args.batches) for _ in range(3)]
      say('%-58s %8.1f ms/batch  [%.1f .. %.1f] over 3 runs' % (
          name, float(np.median(ms)), min(ms), max(ms)))
      rec['loader_ms_per_batch'][name] = ms
    if not args.skip_steps:
      rec['step_ms'] = {}
      tree = ['--kitti_dataset_variant', 'raw_city', '--kitti_data_root', root, '--n_layers',
              '2', '--data_workers', '16', '--kitti_resize', 'device', '--kitti_augment',
              'true']
      on = ['--kitti_gt_everywhere', 'true', '--depth_sup_wt', '1']
      for name, extra in (('no ground truth', []),
                          ('px, --depth_sup_wt 1', on + ['--kitti_dl_disparities_px', 'true']),
                          ('velodyne, --depth_sup_wt 1', on + ['--kitti_dl_velodyne', 'true'])):
        ms = time_step(tree + extra, steps=12, warm=6)
        say('training step, 2 layers, fed from the tree, %s: %.1f ms' % (name, ms))
        rec['step_ms'][name] = ms
    off = flag_off_rounds(root, rounds, args.batches, args.parent_pkg)
    say('device-route loader, flag off, 16 threads, ms/batch, one process per figure, %d '
        'rounds%s:' % (rounds, ', the builds alternating' if args.parent_pkg else ''))
    for key, t in off.items():
      say('  %-8s median %.2f  [%.2f .. %.2f]  %s' % (
          key, float(np.median(t)), min(t), max(t), ' '.join('%.2f' % v for v in t)))
    rec['flag_off_ms_per_batch'] = off


def time_host_parts(root, reps=8):
  ld = kitti_data.DataLoader(loader_opts(root))
  paths = ld.img_list_src[:reps]
  t0 = time.perf_counter()
  arrs = [pipeline.decode_u8(p, 3) for p in paths]
  t1 = time.perf_counter()
  for a in arrs:
    kitti_data.area_resize(a.astype(np.float32) * np.float32(1.0 / 255), H, W)
  t2 = time.perf_counter()
  for p in paths:
    kitti_data._load_image(p, H, W)
  t3 = time.perf_counter()
  return ((t1 - t0) * 1e3 / reps, (t2 - t1) * 1e3 / reps, (t3 - t2) * 1e3 / reps)


def time_step(extra, steps=20, warm=6):
  import ldi_enc_dec as script
  base = ['--dataset', 'kitti', '--batch_size', str(BS), '--img_height', str(H),
          '--img_width', str(W), '--checkpoint_dir',
          os.path.join(tempfile.gettempdir(), 'lsi_data_bench_ckpt'),
          '--save_latest_freq', '1000000', '--checkpoint_freq', '1000000',
          '--log_freq', '1000000']
  opts = script.apply_dataset_overrides(script.build_parser().parse_args(base + extra))
  tr = script.Trainer(opts)
  tr.setup()
  try:
    for _ in range(warm):
      tr.train_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
      tr.train_step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps
  finally:
    close = getattr(tr.data_loader, 'close', None)
    if close is not None:
      close()


def main():
  ap = argparse.ArgumentParser(description=__doc__)
  ap.add_argument('--out', default='')
  ap.add_argument('--batches', type=int, default=12)
  ap.add_argument('--skip_steps', action='store_true')
  ap.add_argument('--kernel_only', action='store_true',
                  help='only the resize launch (for a rocprofv3 --kernel-trace run)')
  ap.add_argument('--augment', action='store_true',
                  help='the augmenting launch and loader instead (module doc)')
  ap.add_argument('--parent_lib', default='',
                  help='--augment: a library with another build\'s lsi_area_resize_u8')
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--gt', action='store_true',
                  help='--kitti_gt_everywhere: launch, loaders, step (module doc)')
  ap.add_argument('--parent_pkg', default='',
                  help="--gt: the previous commit's package directory, library built")
  ap.add_argument('--flag_off_child', default='', help=argparse.SUPPRESS)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'data_bench needs a ROCm device'
  lines, rec = [], {}

  def say(s):
    print(s, flush=True)
    lines.append(s)

  if args.flag_off_child:
    flag_off_child(args.flag_off_child, args.batches)
    return
  if args.gt:
    run_gt(args, say, rec)
    say(json.dumps(rec))
    if args.out:
      os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
      with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return

  with tempfile.TemporaryDirectory(prefix='lsi_kitti_tree_') as root:
    png = write_tree(root)
    say('tree: %d sequences x %d pairs, sizes %s, mean PNG %.0f kB; batch %d -> %d x %d'
        % (len(SIZES), PAIRS_PER_SEQ, SIZES, png / 1e3, BS, H, W))
    if args.kernel_only:
      med, best, moved, _ = time_kernel(root, reps=50)
      say('resize launch alone: median %.1f us, min %.1f us by HIP events, %.1f MB'
          % (med, best, moved / 1e6))
      return
    if args.augment:
      times, moved = time_augment_launches(root, args.parent_lib, max(5, args.rounds))
      say('launch on 8 RGB images -> 8 x %d x %d x 3 fp32, HIP events, us: median '
          'of the %d round medians [min .. max over the rounds]'
          % (H, W, max(5, args.rounds)))
      for key, t in times.items():
        say('  %-18s %6.1f  [%5.1f .. %5.1f]  %.1f MB' % (
            key, float(np.median(t)), min(t), max(t), moved[key] / 1e6))
      base = times.get('parent_plain', times['plain'])
      spread = max(base) - min(base)
      say('  spread of %s over the rounds: %.1f us; bar = its median + spread = %.1f us'
          % ('parent_plain' if 'parent_plain' in times else 'plain', spread,
             float(np.median(base)) + spread))
      rec['augment_launch_us'] = times
      import ldi_enc_dec as script
      rec['augment_loader_ms_per_batch'] = {}
      for _ in range(2):
        for on in (False, True):
          ms = time_loader(lambda: script.KittiBatches(pipeline.PrefetchLoader(
              kitti_data.DataLoader(loader_opts(root, kitti_augment=on)), workers=16,
              resize='device', device=torch.device('cuda', 0))), args.batches)
          say('16 threads, resize on the device, --kitti_augment %-5s %8.1f ms/batch'
              % (str(on).lower(), ms))
          rec['augment_loader_ms_per_batch'].setdefault(
              'on' if on else 'off', []).append(ms)
      say(json.dumps(rec))
      if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
          f.write('\n'.join(lines) + '\n')
      return
    dec, rsz, whole = time_host_parts(root)
    say('one image on one thread: decode %.1f ms, host AREA resize %.1f ms, '
        '_load_image %.1f ms' % (dec, rsz, whole))
    rec['image_ms'] = {'decode': dec, 'host_resize': rsz, 'load_image': whole}
    med, best, moved, up = time_kernel(root)
    say('resize launch alone (8 RGB images -> 8 x %d x %d x 3 fp32): median %.1f us, '
        'min %.1f us, %.1f MB moved (%.0f GB/s at the median); upload %.1f MB'
        % (H, W, med, best, moved / 1e6, moved / med / 1e3, up / 1e6))
    rec['resize_kernel'] = {'median_us': med, 'min_us': best, 'bytes': moved,
                            'upload_bytes': up}
    import ldi_enc_dec as script
    sync = time_loader(lambda: script.KittiBatches(
        kitti_data.DataLoader(loader_opts(root))), args.batches)
    say('%-34s %8.1f ms/batch %7.2f batches/s' % ('synchronous loader (baseline)',
                                                 sync, 1e3 / sync))
    rec['loaders_ms_per_batch'] = {'sync': sync}
    for resize in ('host', 'device'):
      for n in (2, 4, 8, 16):
        ms = time_loader(lambda: script.KittiBatches(pipeline.PrefetchLoader(
            kitti_data.DataLoader(loader_opts(root)), workers=n, resize=resize,
            device=torch.device('cuda', 0))), args.batches)
        say('%-34s %8.1f ms/batch %7.2f batches/s  x%.1f' % (
            '%2d threads, resize on the %s' % (n, resize), ms, 1e3 / ms, sync / ms))
        rec['loaders_ms_per_batch']['%s_%d' % (resize, n)] = ms
    if not args.skip_steps:
      rec['step_ms'] = {}
      for nl in (2, 4):
        ms = time_step(['--kitti_procedural', 'true', '--n_layers', str(nl)])
        say('training step, %d layers, procedural pairs: %.1f ms (%.2f steps/s)'
            % (nl, ms, 1e3 / ms))
        rec['step_ms']['L%d' % nl] = ms
      tree = ['--kitti_dataset_variant', 'raw_city', '--kitti_data_root', root,
              '--n_layers', '2']
      dev = lambda n: ['--data_workers', str(n), '--kitti_resize', 'device']
      graph = ['--hip_graph', 'true']
      for key, name, extra in (
          ('L2_tree_sync', 'tree, synchronous loader', tree),
          ('L2_tree_device_8', 'tree, 8 threads + device resize', tree + dev(8)),
          ('L2_tree_device_16', 'tree, 16 threads + device resize', tree + dev(16)),
          ('L2_graph', 'procedural pairs, --hip_graph', graph + [
              '--kitti_procedural', 'true', '--n_layers', '2']),
          ('L2_graph_tree_device_16', 'tree, 16 threads + device resize, --hip_graph',
           tree + dev(16) + graph)):
        ms = time_step(extra, steps=12, warm=6)
        say('training step, 2 layers, %s: %.1f ms' % (name, ms))
        rec['step_ms'][key] = ms
  say(json.dumps(rec))
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
