"""Times the synthetic-planes loaders and the fused scene renderer.

    python tools/scene_bench.py [--bs 16] [--hw 256] [--rounds 3] [--gt]

* DataLoader.forward(bs) (per-instance op route) against
  BatchedDataLoader.forward(bs) with device and with host textures: seconds per
  batch, host clock around work that ends in a device synchronise; the loaders
  alternate, `--rounds` rounds after one warm-up call each.
* lsi_render_planes alone on one batch (HIP-graph replay, device time from
  events): microseconds per launch, the bytes it must move (every texture once
  + the outputs) and that traffic as a fraction of 8 TB/s.
Prints one line per measurement and a final JSON line.
"""
import argparse
import ctypes
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'layered-scene-inference_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--bs', type=int, default=16)
  ap.add_argument('--hw', type=int, default=256)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--gt', action='store_true', help='synth_dl_eval_data (14 outputs)')
  ap.add_argument('--replays', type=int, default=50)
  args = ap.parse_args()
  from lsi import _C
  from lsi.data import synthetic_planes as sp
  from lsi.geometry import layers
  from lsi.nnutils import helpers
  dev = torch.device('cuda:0')
  opts = types.SimpleNamespace(img_height=args.hw, img_width=args.hw, n_obj_max=4,
                               n_obj_min=1, n_box_planes=5, synth_ds_factor=1,
                               synth_dl_eval_data=args.gt)
  loaders = {
      'DataLoader': sp.DataLoader(opts, device=dev, seed=0),
      'Batched/device': sp.BatchedDataLoader(opts, device=dev, seed=0),
      'Batched/host': sp.BatchedDataLoader(opts, device=dev, seed=0, textures='host'),
  }
  times = {k: [] for k in loaders}
  for rnd in range(args.rounds + 1):           # round 0 warms every shape
    for name, ld in loaders.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      ld.forward(args.bs)
      torch.cuda.synchronize()
      dt = time.perf_counter() - t0
      if rnd:
        times[name].append(dt)
        print('round %d  %-15s %9.3f ms per batch of %d' % (rnd, name, dt * 1e3, args.bs))
  med = {k: float(np.median(v)) for k, v in times.items()}
  spread = {k: float(max(v) - min(v)) for k, v in times.items()}
  for k in loaders:
    print('%-15s median %9.3f ms  spread %8.3f ms  x%.1f vs DataLoader' %
          (k, med[k] * 1e3, spread[k] * 1e3, med['DataLoader'] / med[k]))

  # the launch alone
  ld = loaders['Batched/device']
  worlds = [ld.generator.forward(raster=False) for _ in range(args.bs)]
  tex = ld._device_textures([w[5] for w in worlds], [w[6] for w in worlds])
  st = lambda i: ld._t(np.stack([w[i] for w in worlds]))
  rot_w2s, t_w2s, k_w, n_hat_w, a_w = [st(i) for i in range(5)]
  views = [sp.sample_views(1, ld.rs)[0] for _ in range(args.bs)]
  rv = ld._t(np.stack([np.stack([np.eye(3), v[0]]) for v in views]))[:, :, None]
  tv = ld._t(np.stack([np.stack([np.zeros((3, 1)), v[1]]) for v in views]))[:, :, None]
  rot = helpers.seq_matmul(rv, rot_w2s[:, None])
  t = tv + helpers.seq_matmul(rv, t_w2s[:, None])
  hom, dmat = layers.plane_homographies(k_w[:, None], ld._t(ld.k_s)[None, None, None],
                                        rot, t, n_hat_w[:, None], a_w[:, None])
  npl, h, w = tex.shape[1], args.hw, args.hw
  hom = hom.reshape(args.bs, 2, npl, 9).contiguous()
  dmat = dmat.reshape(args.bs, 2, npl, 3).contiguous()
  result = {'loaders_s': med, 'spread_s': spread, 'bs': args.bs, 'hw': args.hw,
            'gt': bool(args.gt), 'launch': {}}
  out_bits = (_C.LSI_SCENE_IMG, _C.LSI_SCENE_DISP, _C.LSI_SCENE_IMG_ROOM,
              _C.LSI_SCENE_DISP_ROOM)
  for label, bits in (('img', out_bits[0]), ('img+disp', sum(out_bits[:2])),
                      ('all four', sum(out_bits))):
    d = _C.LsiSceneDesc()
    d.B, d.V, d.P, d.Hs, d.Ws, d.H, d.W = args.bs, 2, npl, h, w, h, w
    d.n_box, d.soft, d.min_disp, d.temp, d.outputs = 5, 0, sp.MIN_DISP, sp.SOFTMAX_TEMP, bits
    outs = [torch.empty((args.bs, 2, h, w, c), device=dev) for c in (3, 1, 3, 1)]
    stream = torch.cuda.Stream()

    def launch():
      rc = _C.lib().lsi_render_planes(
          ctypes.byref(d), _C.ptr(tex), _C.ptr(hom), _C.ptr(dmat),
          *([_C.ptr(o) for o in outs] + [_C.stream_ptr(dev)]))
      _C.check(rc, 'lsi_render_planes')
    with torch.cuda.stream(stream):
      launch()
      stream.synchronize()
      graph = torch.cuda.CUDAGraph()
      with torch.cuda.graph(graph, stream=stream):
        launch()
    for _ in range(5):
      graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.replays):
      graph.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / args.replays
    nbytes = tex.numel() * 4 + sum(o.numel() * 4 for o, bit in zip(outs, out_bits)
                                   if bits & bit)
    frac = nbytes / (us * 1e-6) / 8e12
    print('lsi_render_planes %-9s %8.1f us per launch, %6.1f MB to move, %4.1f %% of 8 TB/s'
          % (label, us, nbytes / 1e6, 100 * frac))
    result['launch'][label] = {'us': us, 'bytes': nbytes, 'frac_of_8TBs': frac}
  print(json.dumps(result))


if __name__ == '__main__':
  main()
