"""Times the LDI mesh rasteriser (csrc/lsi_ldi_raster.hip through
lsi.geometry.raster) at the shape ldi_render.py uses -- 2 layers, 256 x 768, the
cameras of --render_views 9 -- per call and per kernel, on an interpolating path
(--render_span 0) and on one that runs beyond both views with forward motion
(--render_span 0.5: the surfaces are magnified); as context the forward_splat +
lsi_fill_holes of the same frames (the K-fold copy of the LDI that route needs
included), the 64-bit atomic maxima of raster_kernel counted exactly on a
surface that is covered once, and an iteration of ldi_render.py with the flag
off and on (against another copy of the script, if one is given: the parent
commit's).

    python tools/raster_bench.py [--out FILE] [--rounds 5] [--render_iters 10]
                                 [--parent_script PATH] [--parts raster,atomics,render]

Input: mesh_bench.py's `typical` LDI (a smooth field with boxes in front, a
hidden layer on 60 % of the texels), edge_ratio 0.9, merge_ratio 0.98.  Times
are device events around back-to-back calls, at least 50 ms per round, rounds
alternating between the routes; the median over the rounds (and the minimum).
A call is what a user makes: the Python binding and its checks, with outputs
and workspace kept between calls.  Kernel times are the device durations in a
torch profiler trace of 20 calls taken after the timing, averaged.  The render
time is a host clock around `Renderer.render_batch` calls that end in a device
synchronise, rounds alternating between the scripts."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'layered-scene-inference_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_bench  # noqa: E402  (timed, traced, inputs, load_script)


def cameras(h, w, span, views=9):
  """(s, (k_s, k_t, rot, t)) of ldi_render.py's path for a pair whose target
  camera stands to the right of and in front of the source camera."""
  import ldi_render
  from lsi.geometry import trajectory
  s = ldi_render.camera_parameters(views, span)
  k = torch.tensor([[[0.58 * w, 0, 0.5 * w], [0, 0.58 * w, 0.5 * h], [0, 0, 1]]])
  c, sn = float(np.cos(0.03)), float(np.sin(0.03))
  rot = torch.tensor([[[c, 0, sn], [0, 1, 0], [-sn, 0, c]]])
  trans = torch.tensor([[[-0.4], [0.0], [-1.2]]])
  kt, r, t = trajectory.interpolate_cameras(k, k, rot, trans, s)
  n = len(s)
  return s, (k.expand(n, 3, 3).contiguous(), kt[:, 0].contiguous(), r[:, 0].contiguous(),
             t[:, 0].contiguous())


def raster_rows(dev, shape, span, rounds, lines):
  from lsi.geometry import fill, ldi as ldi_utils, raster
  nl, nb, h, w = shape
  buf_host, par = mesh_bench.inputs('typical', nl, nb, h, w)
  buf = torch.from_numpy(buf_host).to(dev)
  ldi = [buf[..., :3], None, buf[..., 3:]]
  s, cams = cameras(h, w, span)
  n = len(s)
  m = raster.view_matrices(1, *cams)
  par = dict(par, max_extent=32)
  out = raster.rasterize_ldi(ldi, m, (h, w), **par)
  ws = torch.empty(n * (h * w * 8 + nl * h * w * 16), dtype=torch.uint8, device=dev)
  m_dev = m.to(dev)
  kw = dict(bg_layer_disp=1e-6, max_disp=1.0, zbuf_scale=50.0)

  def hip():
    img, cov, _ = raster.rasterize_ldi(ldi, m_dev, (h, w), out=out, workspace=ws, **par)
    return img, cov

  def hip_filled():
    img, cov = hip()
    return fill.fill_holes(img[0], cov[0])

  def splat():
    rep = [None if x is None else x.expand(-1, n, -1, -1, -1).contiguous() for x in ldi]
    img, wts, _ = ldi_utils.forward_splat(rep, None, *cams, compose_layers=True,
                                          compute_trg_disp=True, **kw)
    return img, wts

  def splat_filled():
    img, wts = splat()
    return fill.fill_splat_holes(img, wts, n_layers=nl, **kw)

  fns = {'raster': hip, 'raster + fill_holes': hip_filled, 'splat': splat,
         'splat + fill_splat_holes': splat_filled}
  cov = hip()[1]
  torch.cuda.synchronize()
  covered = float(cov.sum())
  wts = splat()[1]
  conf = fill.splat_confidence(wts, n_layers=nl, **kw)
  reps = {}
  for name, fn in fns.items():
    mesh_bench.timed(fn, 3)
    us = mesh_bench.timed(fn, 3)
    reps[name] = max(int(60e3 / us) + 1, 3)
  rows = {key: [] for key in fns}
  for _ in range(rounds):
    for name, fn in fns.items():
      rows[name].append(mesh_bench.timed(fn, reps[name]))
  trace = mesh_bench.traced(hip, 20)
  trace_splat = mesh_bench.traced(splat, 5)
  lines += [
      '',
      'span %.1f: s = %s' % (span, ', '.join('%+.2f' % v for v in s)),
      '%d x %d x %d x %d packed RGBD fp32 into %d views of %d x %d; edge_ratio %.2f, merge_ratio '
      '%.2f, max_extent %d; workspace %.1f MB' % (nl, nb, h, w, n, h, w, par['edge_ratio'],
                                                   par['merge_ratio'], par['max_extent'],
                                                   ws.numel() / 1e6),
      'covered pixels: %.1f %% of the frames (mesh); mean splat confidence %.1f %%' %
      (100 * covered / (n * h * w), 100 * float(conf.mean())),
      '%d rounds, alternating; calls per round: %s; us per call, median (min)' %
      (rounds, ', '.join('%s %d' % kv for kv in reps.items())),
  ]
  for name in fns:
    lines.append('  %-28s %9.1f (%.1f)' % (name, float(np.median(rows[name])),
                                           float(np.min(rows[name]))))
  lines.append('profiler trace, lsi_ldi_raster (20 calls): launches per call x mean device time, us')
  for name in sorted(trace):
    lines.append('      %4.1f x %-28s %8.2f' % (trace[name][0], name, trace[name][1]))
  dev_us = sum(cnt * t for cnt, t in trace.values())
  ras = trace.get('raster_kernel', (0, 0.0))[1]
  lines += [
      '  %.1f us on the device per call; forward_splat alone: %.1f us on the device in %.1f '
      'launches' % (dev_us, sum(cnt * t for cnt, t in trace_splat.values()),
                    sum(cnt for cnt, _ in trace_splat.values())),
      '  raster_kernel: %.2f M (view, quad) threads, %.2f M pixels won; at least %.1f 64-bit '
      'maxima per ns arrive (every won pixel took one or more; the skipped and the lost ones '
      'are not counted, so this is a floor, not the rate of the atomic unit)' %
      (n * nl * (h - 1) * (w - 1) / 1e6, covered / 1e6, covered / max(ras, 1e-9) / 1e3),
  ]


def atomic_rows(dev, lines):
  """The 64-bit atomic maximum, counted exactly: one fully valid smooth layer is
  covered exactly once (a shared edge has one owner), so every covered pixel is
  one atomic that a zero key could not skip, and none is lost.  raster_kernel's
  time with the surface in the frame, less its time with the same surface
  projected beside the frame (every box empty: set-up only), is the time of the
  pixel walk and its atomics."""
  from lsi.geometry import raster
  h, w, n = 256, 768, 9
  yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
  buf = np.concatenate([np.random.RandomState(0).rand(1, 1, h, w, 3).astype(np.float32),
                        (0.2 + 0.1 * xx / w + 0.05 * yy / h)[None, None, :, :, None]], -1)
  buf = torch.from_numpy(buf).to(dev)
  ldi = [buf[..., :3], None, buf[..., 3:]]
  lines += ['', '64-bit atomic maxima, counted: 1 x 1 x %d x %d, fully valid, %d equal views; '
            'raster_kernel device time, us (profiler trace, 20 calls)' % (h, w, n)]
  for name, scale in (('identity, 1 pixel per quad', 1), ('2 x magnified, 4 pixels per quad', 2),
                      ('4 x magnified, 16 pixels per quad', 4)):
    ht, wt = h * scale, w * scale
    m = torch.diag(torch.tensor([float(scale), float(scale), 1.0, 1.0]))
    off = m.clone()
    off[0, 2] = 12000.0                                     # beside the frame, inside the guard
    times = {}
    for key, mat in (('in', m), ('off', off)):
      mats = mat.expand(1, n, 4, 4).contiguous().to(dev)
      out = raster.rasterize_ldi(ldi, mats, (ht, wt), edge_ratio=0.0)
      ws = torch.empty(n * (ht * wt * 8 + h * w * 16), dtype=torch.uint8, device=dev)
      fn = lambda: raster.rasterize_ldi(ldi, mats, (ht, wt), edge_ratio=0.0, out=out, workspace=ws)
      mesh_bench.timed(fn, 20)
      times[key] = mesh_bench.traced(fn, 20)['raster_kernel'][1]
      if key == 'in':
        atomics = float(out[1].sum())
      else:
        assert float(out[1].sum()) == 0
    dt = times['in'] - times['off']
    lines.append('  %-34s %8.2f in the frame, %6.2f beside it; %.3f M atomics in %.2f us: %.1f per '
                 'ns, %.3f TB/s of key bytes' % (name, times['in'], times['off'], atomics / 1e6, dt,
                                                 atomics / dt / 1e3, atomics * 8 / dt / 1e6))


def render_rows(rounds, iters, parent_script, lines):
  import ldi_enc_dec as script
  import ldi_render
  mods = {'this tree, flag off': (ldi_render, []),
          'this tree, --render_mesh': (ldi_render, ['--render_mesh', 'true'])}
  if parent_script:
    mods['other script'] = (mesh_bench.load_script(parent_script, 'ldi_render_other'), [])
  rs, batches = {}, None
  for name, (mod, extra) in mods.items():
    argv = ['--dataset', 'synthetic', '--synth_scene', 'planes', '--batch_size', '1',
            '--n_layers', '2', '--random_weights', 'true', '--render_views', '9',
            '--checkpoint_dir', tempfile.mkdtemp(prefix='raster_bench_')] + extra
    opts = script.apply_dataset_overrides(mod.build_parser().parse_args(argv))
    r = mod.Renderer(opts)
    r.restore()
    if batches is None:
      batches = [r.trainer.data_loader.forward(1) for _ in range(4)]
    for k in range(2):
      r.render_batch(batches[k])
    rs[name] = (r, opts)
  ms = {name: [] for name in rs}
  for rnd in range(rounds):
    for name, (r, _) in list(rs.items())[::1 if rnd % 2 == 0 else -1]:   # A B C, C B A, ...
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for k in range(iters):
        r.render_batch(batches[k % 4])
      torch.cuda.synchronize()
      ms[name].append((time.perf_counter() - t0) * 1e3 / iters)
  r0, o = rs['this tree, flag off']
  lines += ['', 'ldi_render.py, synthetic planes, 2 layers, %d x %d, K = %d cameras, untrained '
            'model; ms per iteration (host clock), %d rounds of %d iterations, alternating, after '
            '2 warm-up: median (min .. max)' %
            (o.img_height, o.img_width, len(r0.s), rounds, iters)]
  for name, v in ms.items():
    lines.append('  %-26s %.3f (%.3f .. %.3f)' % (name, float(np.median(v)), min(v), max(v)))
  frames = rs['this tree, --render_mesh'][0].render_batch(batches[0])['frames']
  lines.append('  hole fractions of the first pair, s: splat / mesh: ' + ', '.join(
      '%+.2f: %.4f / %.4f' % (f['s'], f['hole_fraction'], f['hole_fraction_mesh'])
      for f in frames))


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default='')
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--render_iters', type=int, default=10)
  ap.add_argument('--parent_script', default='',
                  help='another ldi_render.py to time beside this tree\'s')
  ap.add_argument('--small', action='store_true', help='tiny shapes: a rehearsal')
  ap.add_argument('--parts', default='raster,atomics,render',
                  help='which measurements to take, comma-separated')
  args = ap.parse_args(argv)
  if not torch.cuda.is_available():
    raise SystemExit('raster_bench: no ROCm device')
  dev = torch.device('cuda:0')
  lines = ['LDI mesh rasteriser: lsi.geometry.raster.rasterize_ldi (csrc/lsi_ldi_raster.hip), '
           'MI355X']
  shape = (2, 1, 32, 96) if args.small else (2, 1, 256, 768)
  parts = args.parts.split(',')
  for span in (0.0, 0.5) if 'raster' in parts else ():
    raster_rows(dev, shape, span, args.rounds, lines)
  if 'atomics' in parts:
    atomic_rows(dev, lines)
  if args.render_iters > 0 and 'render' in parts:
    render_rows(args.rounds, args.render_iters, args.parent_script, lines)
  text = '\n'.join(lines) + '\n'
  sys.stdout.write(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text)
  return 0


if __name__ == '__main__':
  sys.exit(main())
