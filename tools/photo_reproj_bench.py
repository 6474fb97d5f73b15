"""Times the fused backward-warp photometric loss (csrc/lsi_photo_reproj.hip),
forward + backward, on two layers of the paired training buffer (2 x 8 planes of
256 x 768 x 3: 4 source views, then 4 target views, against their 8 input
images, shift 4) for a rectified and for a general pose, contiguous and in the
network's layout (L x 2 B x H x W x 4 views of one 2 B x H x W x L x 4 buffer),
against the same graph in torch ops (tests/photo_reproj_ref.py (b), fp32) and
beside the geometric-consistency call on the same planes, on one device, in
alternating rounds of one process.

    python tools/photo_reproj_bench.py [--out FILE] [--rounds 5] [--iters 500]
    python tools/photo_reproj_bench.py --kernels-only   # for a kernel trace

Times are device events around `iters` back-to-back calls, after a second of
warm-up.  The bytes a call is held against are the ones the algorithm needs (the
header of csrc/lsi_photo_reproj.hip): per pixel of a plane 4 C + 4 read each
way and 4 C + 4 written by the backward, the sampled images and the partner read
once each way, the taps as cache hits; the rate they are compared with is the
6.29 TB/s a copy kernel reaches on the MI355X.  The op restatement finds the
scored pixels with `nonzero`, which waits for the device once per call: it is
context, not a contender.  The geometric-consistency call (ratio, the same
occlusion threshold) projects the same 16 disparity planes by the same matrices
into the same partner planes, in its two-tensor form.

This tool writes the per-call blocks of profiles/photo_reproj/loss_fwd_bwd.txt.
The kernel-time block at the end of that file comes from a run of its own,

    rocprofv3 --kernel-trace --stats -d DIR -o trace -- \
        python tools/photo_reproj_bench.py --kernels-only

which issues 50 fused calls per case in the order of the blocks (rectified
contiguous, rectified network, general contiguous, general network): the
durations of photo_fwd_kernel, plane_finish_kernel and photo_bwd_kernel in the
trace, split into four equal runs, the first 5 calls of each left out, median
(min .. max); the register and LDS figures beside it are the compiler's
(-Rpass-analysis=kernel-resource-usage), and the last line is bench.py's."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'layered-scene-inference_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

COPY_RATE = 6.29e12     # B/s, float4 copy on the MI355X


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
  ap.add_argument('--iters', type=int, default=500)
  ap.add_argument('--shape', type=int, nargs=5, default=[2, 8, 256, 768, 3],
                  metavar=('L', 'Q', 'H', 'W', 'C'))
  ap.add_argument('--mode', default='l1', choices=['l1', 'charb'])
  ap.add_argument('--occl', type=float, default=0.2)
  ap.add_argument('--noise', type=float, default=0.01,
                  help='amplitude of the per-pixel noise on the smooth disparities '
                  '(0.01 moves a rectified tap by up to 3.7 px at W = 768)')
  ap.add_argument('--kernels-only', action='store_true',
                  help='50 fused calls per case and nothing else')
  args = ap.parse_args(argv)
  if not torch.cuda.is_available():
    raise SystemExit('photo_reproj_bench: no ROCm device')
  import photo_reproj_ref as ref
  from geo_cons_bench import pair_matrices
  from lsi.loss import _hip
  dev = torch.device('cuda:0')
  nl, q, h, w, c = args.shape
  p = nl * q
  n = p * h * w
  yy, xx = np.mgrid[0:h, 0:w]
  rng = np.random.RandomState(0)
  layer0 = np.stack([0.2 + 0.06 * np.sin(0.02 * xx + 0.5 * i) + 0.05 * np.cos(0.03 * yy) +
                     args.noise * rng.uniform(size=(h, w)) for i in range(q)])
  disps = np.stack([layer0 * (1.0 - l / 5.0) for l in range(nl)]).astype(np.float32)
  colour = lambda k, ph: np.stack(
      [np.stack([0.5 + 0.25 * np.sin(0.03 * xx + 0.4 * i + ch + ph) +
                 0.2 * np.cos(0.05 * yy - 0.3 * ch) + 0.03 * rng.uniform(size=(h, w))
                 for ch in range(c)], axis=-1) for i in range(k)]).astype(np.float32)
  texs = colour(p, 0.0).reshape(nl, q, h, w, c)
  imgs = torch.from_numpy(colour(q, 0.1)).to(dev)
  fwd_bytes = n * (4 * c + 4) + q * h * w * (4 * c + 4)
  bwd_bytes = fwd_bytes + n * (4 * c + 4)
  text = ''
  ok_all = True
  poses = (('rectified, t = (-0.54, 0, 0)', (0, 0, 0), (-0.54, 0, 0)),
           ('general, rotation (2, -4, 3) deg, t = (0.3, -0.1, 0.25)', (2, -4, 3),
            (0.3, -0.1, 0.25)))
  for pose_name, deg, t in poses:
    mats = pair_matrices(q, h, w, deg, t)
    flat = lambda a: a.reshape((p,) + a.shape[2:])
    scored = int(ref.forward(flat(texs), flat(disps), imgs.cpu().numpy(), mats.numpy(),
                             disps[0], q // 2, args.occl)['scored'].sum())
    mats = mats.to(dev)
    for layout in ('contiguous', 'network'):
      if layout == 'network':
        if c > 3:
          raise SystemExit('photo_reproj_bench: the network layout holds 3 channels')
        buf = torch.zeros((q, h, w, nl, 4), device=dev)
        pred = buf.permute(3, 0, 1, 2, 4)
        pred[..., :c] = torch.from_numpy(texs).to(dev)
        pred[..., 3] = torch.from_numpy(disps).to(dev)
        tex, disp = pred[..., :c], pred[..., 3]
      else:
        tex, disp = torch.from_numpy(texs).to(dev), torch.from_numpy(disps).to(dev)
      tex.requires_grad_(True)
      disp.requires_grad_(True)
      partner = disp[0].detach()
      # geo-cons on the same planes: every layer against the partner of its view
      geo_mats = mats.repeat(nl, 1, 1)
      roll = (torch.arange(q, device=dev) + q // 2) % q
      geo_partner = partner[roll].repeat(nl, 1, 1).contiguous()
      geo_disp = disp.detach().reshape(p, h, w).contiguous().requires_grad_(True)

      def fused_fwd():
        return _hip.photometric_reprojection_loss(tex, disp, imgs, mats, partner, q // 2,
                                                  args.mode, args.occl, 1e-3)

      def fused():
        tex.grad = disp.grad = None
        fused_fwd().backward()

      flat_t = lambda a: a.reshape((p,) + tuple(a.shape[2:]))

      def ops_loss():
        return ref.loss_ops(flat_t(tex), flat_t(disp), imgs, mats, partner, q // 2,
                            args.mode, args.occl, 1e-3)

      def ops():
        tex.grad = disp.grad = None
        ops_loss().backward()

      def geo():
        geo_disp.grad = None
        _hip.geometric_consistency_loss(geo_disp, geo_partner, geo_mats, 'ratio',
                                        args.occl).backward()

      if args.kernels_only:
        timed(fused, 50)
        continue
      # the two agree before they are timed
      fused()
      gt_fused, gd_fused = tex.grad.clone(), disp.grad.clone()
      l_fused = float(fused_fwd().detach())
      ops()
      gt_ops, gd_ops = tex.grad.clone(), disp.grad.clone()
      l_ops = float(ops_loss().detach())
      gt_diff = float((gt_fused - gt_ops).abs().max() / gt_ops.abs().max())
      gd_diff = float((gd_fused - gd_ops).abs().max() / gd_ops.abs().max())
      t0 = time.perf_counter()
      while time.perf_counter() - t0 < 1.0:             # warm-up, a second of it
        timed(fused, 20)
        timed(fused_fwd, 20)
        timed(geo, 20)
        timed(ops, 2)
      rows = {'fused': [], 'fused_fwd': [], 'ops': [], 'geo': []}
      for _ in range(args.rounds):
        rows['fused'].append(timed(fused, args.iters))
        rows['ops'].append(timed(ops, max(args.iters // 25, 1)))
        rows['geo'].append(timed(geo, args.iters))
        with torch.no_grad():
          rows['fused_fwd'].append(timed(fused_fwd, args.iters))
      med = {k: float(np.median(v)) for k, v in rows.items()}
      lo = {k: float(np.min(v)) for k, v in rows.items()}
      hi = {k: float(np.max(v)) for k, v in rows.items()}
      bwd_us = med['fused'] - med['fused_fwd']
      rate = lambda nbytes, us: nbytes / max(us, 1e-9) / 1e6       # TB/s
      lines = [
          'photometric reprojection loss (%s, occl %g), forward + backward, fp32; %d layers '
          'x %d views x %d x %d x %d, %s; pose %s: %d of %d pixels scored' %
          (args.mode, args.occl, nl, q, h, w, c, layout, pose_name, scored, n),
          '%d rounds of %d calls (op graph: %d), alternating; us per call, median (min .. '
          'max)' % (args.rounds, args.iters, max(args.iters // 25, 1)),
          'fused forward + backward  %9.1f (%.1f .. %.1f)   %.1f MB -> %.2f TB/s of the '
          'algorithm\'s bytes; at %.2f TB/s they take %.1f us' %
          (med['fused'], lo['fused'], hi['fused'], (fwd_bytes + bwd_bytes) / 1e6,
           rate(fwd_bytes + bwd_bytes, med['fused']), COPY_RATE / 1e12,
           (fwd_bytes + bwd_bytes) / COPY_RATE * 1e6),
          'fused forward alone       %9.1f (%.1f .. %.1f)   %.1f MB -> %.2f TB/s' %
          (med['fused_fwd'], lo['fused_fwd'], hi['fused_fwd'], fwd_bytes / 1e6,
           rate(fwd_bytes, med['fused_fwd'])),
          'fused backward (the rest) %9.1f                  %.1f MB -> %.2f TB/s' %
          (bwd_us, bwd_bytes / 1e6, rate(bwd_bytes, bwd_us)),
          'geo-cons fwd + bwd        %9.1f (%.1f .. %.1f)   the same %d planes, two-tensor '
          'form, ratio' % (med['geo'], lo['geo'], hi['geo'], p),
          'op graph fwd + bwd        %9.1f (%.1f .. %.1f)' % (med['ops'], lo['ops'], hi['ops']),
          'loss fused %.9g ops %.9g; gradient difference %.3g (texture), %.3g (disparity) of '
          'the largest entry' % (l_fused, l_ops, gt_diff, gd_diff),
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
