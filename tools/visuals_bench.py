"""Times the contact-sheet launch of a saved evaluation iteration
(csrc/lsi_visual.hip through lsi.visualization.SheetBuilder) and, as context,
the obvious torch-op route: every visual clamped, scaled, rounded, cast and
copied to the host on its own.

    python tools/visuals_bench.py [--out FILE] [--rounds 5] [--shape 256 768] [--layers 3]

The cells are those of a synthetic iteration (ldi_pred_eval.py --save_visuals)
on random tensors of the real shapes; the renderings are half size.  Times are
device events around back-to-back calls, at least 50 ms per round.  Bytes are
what the algorithm needs: every source element the sheet shows once, and the
sheet."""
import argparse
import os
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


def cells(dev, L, H, W):
  """[(adder, name, tensors, range)] of one synthetic iteration, batch of 2."""
  r = lambda *s: torch.rand(s, device=dev)
  B, h, w = 2, H // 2, W // 2
  out = [('rgb', 'src_im', (r(B, H, W, 3)[0],), (0., 1.)),
         ('rgb', 'trg_im', (r(B, H, W, 3)[0],), (0., 1.))]
  tex, disp = [r(L, B, H, W, 3) for _ in range(2)], [r(L, B, H, W, 1) for _ in range(2)]
  for l in range(L):
    for v, key in enumerate(('src', 'trg')):
      out.append(('rgb', '%s_tex_pred_layer_%d' % (key, l), (tex[v][l, 0],), (0., 1.)))
      out.append(('map', '%s_disp_pred_layer_%d' % (key, l), (disp[v][l, 0, :, :, 0],),
                  (0., 1.)))
  for key in ('trg', 'src'):
    recons, rdisp, small, gt = r(1, B, h, w, 3), r(1, B, h, w, 1), r(B, h, w, 3), r(B, h, w, 1)
    out += [('rgb', key + '_splat_tex', (recons[0, 0],), (0., 1.)),
            ('absdiff', key + '_vs_loss', (recons[0, 0], small[0]), (0., 0.5)),
            ('map', key + '_splat_disp', (rdisp[0, 0, :, :, 0],), (0., 1.)),
            ('map', key + '_gt_disp', (gt[0, :, :, 0],), (0., 1.)),
            ('absdiff', key + '_depth_loss', (rdisp[0, 0], gt[0]), (0., 0.5)),
            ('gray', key + '_disocc_mask', ((r(B, H, W, 1) > 0.6).float()[0, :, :, 0],),
             (0., 1.))]
  for key in ('src', 'trg'):
    out += [('rgb', key + '_gt_tex_bg', (r(B, H, W, 3)[0],), (0., 1.)),
            ('map', key + '_gt_disp_bg', (r(B, H, W, 1)[0, :, :, 0],), (0., 1.))]
  return out


def op_route(items, lut):
  """One uint8 host array per visual, the way torch ops would make them."""
  out = []
  for kind, _, ts, (lo, hi) in items:
    v = ts[0]
    if kind == 'absdiff':
      v = (ts[0] - ts[1]).abs()
      v = v.mean(dim=2) if v.dim() == 3 else v
    q = ((v - lo) * (1.0 / (hi - lo))).clamp(0, 1).mul(255).add(0.5).floor().to(torch.uint8)
    if kind in ('map', 'absdiff'):
      q = lut[q.long()]
    out.append(q.cpu())
  return out


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default='')
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--shape', type=int, nargs=2, default=[256, 768])
  ap.add_argument('--layers', type=int, default=3)
  ap.add_argument('--cols', type=int, default=6)
  args = ap.parse_args(argv)
  if not torch.cuda.is_available():
    raise SystemExit('visuals_bench: no ROCm device')
  from lsi.visualization import SheetBuilder
  dev = torch.device('cuda:0')
  H, W = args.shape
  torch.manual_seed(0)
  items = cells(dev, args.layers, H, W)
  sb = SheetBuilder(dev, args.cols, H, W)
  for kind, name, ts, (lo, hi) in items:
    if kind == 'absdiff':
      sb.add_absdiff(name, ts[0], ts[1], hi)
    else:
      getattr(sb, 'add_' + kind)(name, ts[0], lo, hi)
  sheet = sb.pack()
  hs, ws = sb.size()
  pitch = sheet.stride(0)
  nbytes = (hs - 1) * pitch + 3 * ws
  flat = torch.as_strided(sheet, (nbytes,), (1,))
  pinned = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)
  lut = torch.from_numpy(sb.lut).to(dev)

  def pack():
    sb.pack(out=sheet)

  def step():   # what a saved iteration adds to the loop's thread: launch + one copy
    sb.pack(out=sheet)
    pinned.copy_(flat, non_blocking=True)

  def ops():
    op_route(items, lut)

  read = sum(4 * t.numel() for _, _, ts, _ in items for t in ts)
  n = {}
  for name, fn in (('pack', pack), ('step', step), ('ops', ops)):
    timed(fn, 10)                                          # warm-up
    us = timed(fn, 10)
    n[name] = max(int(60e3 / us) + 1, 10)                  # >= 50 ms per round
  rows = {k: [] for k in n}
  for _ in range(args.rounds):
    for name, fn in (('pack', pack), ('step', step), ('ops', ops)):
      rows[name].append(timed(fn, n[name]))
  med = {k: float(np.median(v)) for k, v in rows.items()}
  lo_ = {k: float(np.min(v)) for k, v in rows.items()}
  lines = [
      'contact sheet of one saved iteration: %d cells of %d x %d (%d layers, renderings '
      'half size, zoom 2), %d columns -> %d x %d x 3 uint8' %
      (len(items), H, W, args.layers, args.cols, hs, ws),
      'bytes: %.2f MB of fp32 sources read, %.2f MB of sheet written' %
      (read / 1e6, 3 * hs * ws / 1e6),
      '%d rounds, alternating; calls per round: %s; us per call, median (min)' %
      (args.rounds, ', '.join('%s %d' % kv for kv in n.items())),
      'pack: descriptor upload + the one launch      %9.1f (%.1f)   %.2f TB/s' %
      (med['pack'], lo_['pack'], (read + 3 * hs * ws) / med['pack'] / 1e6),
      'visuals step: pack + one copy to pinned host  %9.1f (%.1f)' %
      (med['step'], lo_['step']),
      'context, torch ops: %d visuals quantised and copied one by one %9.1f (%.1f)' %
      (len(items), med['ops'], lo_['ops']),
      '(pack and step are timed as the evaluation calls them: SheetBuilder.pack with its',
      ' host-side descriptor copy, not the kernel alone; PNG encoding is on another thread)',
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
