"""Times the LDI mesh export (csrc/lsi_ldi_mesh.hip through lsi.geometry.mesh)
and, as context, the torch-op route of the same arguments (ldi_mesh_ops); lists
the kernels of a call with their times, compares them with the bytes the
algorithm needs, times `.to_host()` and the file write on their own, and times
an iteration of ldi_render.py without --save_mesh (against another copy of the
script, if one is given: the parent commit's).

    python tools/mesh_bench.py [--out FILE] [--rounds 5] [--render_iters 10]
                               [--parent_script PATH]

Shapes: the 2 x 1 x 256 x 768 item ldi_render.py exports and the paired
2 x 8 x 256 x 768 buffer, both as views of one packed RGBD buffer.  Inputs:
`typical` -- a smooth disparity field with a few dozen fronto-parallel boxes in
front of it (depth steps), the hidden layer behind it valid on 60 % of the
texels and equal to the front layer on a fifth of those, edge_ratio 0.9,
merge_ratio 0.98; `all valid` -- a smooth field in both layers and no cut: the
largest output.

Times are device events around back-to-back calls, at least 50 ms per round,
rounds alternating between the routes; the median over the rounds (and the
minimum).  A call is what a user makes: the Python binding and its checks with
buffers and workspace kept between calls.  Kernel times are the device
durations in a torch profiler trace of 20 calls taken after the timing,
averaged.  Bytes: disp read by each of the three passes, tex by the vertex
pass, the index map written once and read once, the records written once.
`.to_host()` and `write_ply` are host clocks (the first ends in its own
synchronise).  The render time is a host clock around `Renderer.render_batch`
calls that end in a device synchronise, rounds alternating between the
scripts (this tree first in even rounds, last in odd ones)."""
import argparse
import ctypes
import importlib.util
import os
import re
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'layered-scene-inference_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

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


def inputs(kind, nl, nb, h, w):
  """(packed RGBD buffer L x B x H x W x 4 on the host, parameters)."""
  rs = np.random.RandomState(0)
  yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
  base = 0.05 + 0.1 * (yy / h) + 0.02 * np.sin(xx / 37.0)         # a ground plane, smooth
  disp = np.broadcast_to(base, (nl, nb, h, w)).astype(np.float32).copy()
  par = dict(disp_min=1e-3, edge_ratio=0.0, merge_ratio=0.0)
  if kind == 'typical':
    par.update(edge_ratio=0.9, merge_ratio=0.98)
    for b in range(nb):
      for _ in range(30):
        y0, x0 = rs.randint(0, h - 16), rs.randint(0, w - 32)
        bh, bw = rs.randint(8, 64), rs.randint(16, 128)
        disp[0, b, y0:y0 + bh, x0:x0 + bw] = 0.2 + 0.3 * rs.rand()
    if nl > 1:
      back = np.broadcast_to(base * 0.9, (nb, h, w)).astype(np.float32).copy()
      pick = rs.rand(nb, h, w)
      back[pick < 0.4] = 0.0                                        # no hidden surface
      same = (pick >= 0.4) & (pick < 0.52)
      back[same] = disp[0][same]                                    # coincides: merged
      disp[1:] = back
  else:
    for l in range(1, nl):
      disp[l] *= np.float32(0.8 ** l)
  tex = rs.rand(nl, nb, h, w, 3).astype(np.float32)
  return np.concatenate([tex, disp[..., None]], -1), par


def mesh_rows(dev, kind, shape, rounds, lines):
  from lsi import _C
  from lsi.geometry import mesh
  import ldi_mesh_ref as R
  nl, nb, h, w = shape
  buf_host, par = inputs(kind, *shape)
  buf = torch.from_numpy(buf_host).to(dev)
  ldi = [buf[..., :3], None, buf[..., 3:]]
  k = torch.tensor([[0.58 * w, 0, 0.5 * w], [0, 0.58 * w, 0.5 * h], [0, 0, 1]]).repeat(nb, 1, 1)
  vcap, fcap = mesh.full_capacity(nl, h, w)
  out = (torch.empty(nb * vcap * 16, dtype=torch.uint8, device=dev),
         torch.empty(nb * fcap * 13, dtype=torch.uint8, device=dev),
         torch.empty((nb, 2), dtype=torch.int32, device=dev))
  d = _C.LsiMeshDesc()
  d.L, d.B, d.H, d.W = nl, nb, h, w
  d.disp_min, d.edge_ratio = 1e-3, 0.5
  need = int(_C.lib().lsi_ldi_mesh_workspace_bytes(ctypes.byref(d)))
  ws = torch.empty(need, dtype=torch.uint8, device=dev)
  fns = {'hip': lambda: mesh.ldi_mesh(ldi, k, out=out, workspace=ws, **par),
         'ops': lambda: mesh.ldi_mesh_ops(ldi, k, **par)}
  m = fns['hip']()
  counts = m.counts.cpu().numpy()
  # the same bytes as the restatement, at the size that is timed (item 0 and the last)
  t0 = time.perf_counter()
  host = m.to_host()
  torch.cuda.synchronize()
  to_host_ms = (time.perf_counter() - t0) * 1e3
  from lsi.geometry import projection
  kinv = projection._inv3(k).numpy().reshape(nb, 9)
  equal = True
  for b in sorted({0, nb - 1}):
    (wv, wf), = R.mesh(buf_host[:, b:b + 1, ..., :3], None, buf_host[:, b:b + 1, ..., 3],
                       kinv[b:b + 1], **par)
    equal = equal and host[b][0].tobytes() == wv.tobytes() and host[b][1].tobytes() == wf.tobytes()
  ops = fns['ops']()
  equal_ops = all(len(o[0]) == c[0] and len(o[2]) == c[1] for o, c in zip(ops, counts))
  with tempfile.TemporaryDirectory() as tmp:
    t0 = time.perf_counter()
    mesh.write_ply(os.path.join(tmp, 'a.ply'), *host[0])
    write_ms = (time.perf_counter() - t0) * 1e3
    file_mb = os.path.getsize(os.path.join(tmp, 'a.ply')) / 1e6
  host_ms = []
  for _ in range(rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.to_host()
    host_ms.append((time.perf_counter() - t0) * 1e3)
  reps = {}
  for name, fn in fns.items():
    timed(fn, 3)
    us = timed(fn, 3)
    reps[name] = max(int(60e3 / us) + 1, 3)
  rows = {key: [] for key in fns}
  for _ in range(rounds):
    for name, fn in fns.items():
      rows[name].append(timed(fn, reps[name]))
  med = {key: float(np.median(v)) for key, v in rows.items()}
  lo = {key: float(np.min(v)) for key, v in rows.items()}
  trace = {'hip': traced(fns['hip'], 20), 'ops': traced(fns['ops'], 2)}
  n = nl * h * w
  nv, nf = int(counts[:, 0].sum()), int(counts[:, 1].sum())
  reads = nb * n * 4 * 3 + nb * n * 12 + nb * n * 4       # disp x 3 passes, tex, the map
  writes = nb * n * 4 + 16 * nv + 13 * nf
  dev_us = sum(cnt * t for cnt, t in trace['hip'].values())
  lines += [
      '',
      'lsi_ldi_mesh, %s, %d x %d x %d x %d packed RGBD fp32: %d vertices (%.1f %% of the texels), '
      '%d faces (%.1f %% of the quads\' triangles); workspace %.2f MB' %
      (kind, nl, nb, h, w, nv, 100.0 * nv / (nb * n), nf,
       100.0 * nf / max(nb * 2 * nl * (h - 1) * (w - 1), 1), need / 1e6),
      'records of items 0 and %d equal the float32 restatement byte for byte: %s; the op route '
      'has the same counts: %s' % (nb - 1, equal, equal_ops),
      '%d rounds, alternating; calls per round: %s; us per call, median (min)' %
      (rounds, ', '.join('%s %d' % kv for kv in reps.items())),
      'HIP, 4 launches                             %9.1f (%.1f)' % (med['hip'], lo['hip']),
      'context, torch ops                          %9.1f (%.1f)' % (med['ops'], lo['ops']),
      'the fused call takes %.4f of the op route\'s time' % (med['hip'] / med['ops']),
      'profiler trace (20 calls HIP, 2 calls ops): launches per call x mean device time, us',
  ]
  for key in ('hip', 'ops'):
    kernels = trace[key]
    lines.append('  %-4s %6.1f kernels per call, %.1f us on the device' %
                 (key, sum(cnt for cnt, _ in kernels.values()),
                  sum(cnt * t for cnt, t in kernels.values())))
    if key == 'hip':
      for name in sorted(kernels):
        lines.append('      %4.1f x %-28s %8.2f' % (kernels[name][0], name, kernels[name][1]))
  total = reads + writes
  lines += [
      'bytes the algorithm needs: %.2f MB read (disp by three passes, tex, the index map) + '
      '%.2f MB written (index map %.2f, vertex records %.2f, face records %.2f) = %.2f MB' %
      (reads / 1e6, writes / 1e6, nb * n * 4 / 1e6, 16 * nv / 1e6, 13 * nf / 1e6, total / 1e6),
      'over the %.1f us of the four kernels: %.3f TB/s, %.1f %% of the %.1f TB/s HBM peak' %
      (dev_us, total / dev_us / 1e6, 100 * total / dev_us / 1e6 / HBM_TBS, HBM_TBS),
      '.to_host() (counts, then the used prefixes of all %d items, %.2f MB): %.2f ms first call, '
      'then median %.2f ms (min %.2f)' %
      (nb, (16 * nv + 13 * nf) / 1e6, to_host_ms, float(np.median(host_ms)), min(host_ms)),
      'write_ply of item 0 (%.2f MB, a temporary directory): %.2f ms' % (file_mb, write_ms),
  ]


def load_script(path, name):
  spec = importlib.util.spec_from_file_location(name, path)
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def render_rows(rounds, iters, parent_script, lines):
  import ldi_enc_dec as script
  import ldi_render
  mods = {'this tree': ldi_render}
  if parent_script:
    mods['other script'] = load_script(parent_script, 'ldi_render_other')
  rs, batches = {}, None
  for name, mod in mods.items():
    argv = ['--dataset', 'synthetic', '--synth_scene', 'planes', '--batch_size', '1',
            '--n_layers', '2', '--random_weights', 'true', '--render_views', '9',
            '--checkpoint_dir', tempfile.mkdtemp(prefix='mesh_bench_')]
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
    for name, (r, _) in list(rs.items())[::1 if rnd % 2 == 0 else -1]:   # A B, B A, ...
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for k in range(iters):
        r.render_batch(batches[k % 4])
      torch.cuda.synchronize()
      ms[name].append((time.perf_counter() - t0) * 1e3 / iters)
  o = rs['this tree'][1]
  lines += ['', 'ldi_render.py without --save_mesh, synthetic planes, 2 layers, %d x %d, K = %d '
            'cameras, untrained model; ms per iteration (host clock), %d rounds of %d iterations, '
            'alternating, after 2 warm-up: median (min .. max)' %
            (o.img_height, o.img_width, len(rs['this tree'][0].s), rounds, iters)]
  for name, v in ms.items():
    lines.append('  %-14s %.3f (%.3f .. %.3f)' % (name, float(np.median(v)), min(v), max(v)))


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default='')
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--render_iters', type=int, default=10)
  ap.add_argument('--parent_script', default='',
                  help='another ldi_render.py to time beside this tree\'s')
  ap.add_argument('--small', action='store_true', help='tiny shapes: a rehearsal')
  args = ap.parse_args(argv)
  if not torch.cuda.is_available():
    raise SystemExit('mesh_bench: no ROCm device')
  dev = torch.device('cuda:0')
  lines = ['LDI mesh export: lsi.geometry.mesh.ldi_mesh (csrc/lsi_ldi_mesh.hip), MI355X']
  shapes = [(2, 1, 16, 48), (2, 2, 16, 48)] if args.small else [(2, 1, 256, 768), (2, 8, 256, 768)]
  for shape in shapes:
    for kind in ('typical', 'all valid'):
      mesh_rows(dev, kind, shape, args.rounds, lines)
  if args.render_iters > 0:
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
