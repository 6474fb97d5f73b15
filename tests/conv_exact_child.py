"""One sweep of tests/conv_exact_ref.py's SWEEPS in a process of its own:

    python tests/conv_exact_child.py <sweep name>

The implicit-GEMM planner reads LSI_IGEMM_MAXRW / LSI_IGEMM_MINWG once per
process; the parent (tests/test_conv_exact_gpu.py) sets them, and LSI_IG_DEBUG,
in this process's environment.  Every case runs forward and data gradient on
narrow-regime operands against the fp64 reference on the device.  stdout's last
line is the JSON verdict; the library writes one `ig ...` plan line per launch
to stderr.  Exit status 0: every case equal; 3: mismatches, reported in the
verdict; anything else is a crash."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, 'layered-scene-inference_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

import torch

import conv_exact_ref as R

MISMATCH = 3


def _where(got, want):
  """The mismatches of one tensor: how many, and the box they lie in."""
  bad = (got != want).nonzero()
  if not len(bad):
    return None
  lo, hi = bad.min(dim=0).values.tolist(), bad.max(dim=0).values.tolist()
  first = tuple(bad[0].tolist())
  return {'count': len(bad), 'of': got.numel(), 'n': [lo[0], hi[0]], 'c': [lo[1], hi[1]],
          'y': [lo[2], hi[2]], 'x': [lo[3], hi[3]], 'first': list(first),
          'got': float(got[first]), 'want': float(want[first])}


def run(name):
  from lsi.nnutils import _hip_conv
  dev = torch.device('cuda:0')
  cl = lambda t: t.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
  out = []
  for case in R.SWEEPS[name][1]:
    x, w, gy = R.operands(case, 'narrow')
    xb, gyb = cl(x).requires_grad_(True), cl(gy)
    wd = w.to(dev)
    y64, gx64, _ = R.reference(case, xb, wd, gyb, 'narrow', want_gw=False)
    if case.kind == 'convt':
      y = _hip_conv.conv_transpose2d(xb, wd, 2, 1)
    else:
      pt, _, oh = R.same_pads(case.h, case.kh, case.stride)
      pl, _, ow = R.same_pads(case.w, case.kw, case.stride)
      y = _hip_conv.conv2d(xb, wd, case.stride, pt, pl, oh, ow)
    gx, = torch.autograd.grad(y, xb, gyb)
    torch.cuda.synchronize()
    out.append({'case': list(case), 'y': _where(y.detach(), R.as_bf16(y64)),
                'gx': _where(gx, R.as_bf16(gx64))})
  ok = all(r['y'] is None and r['gx'] is None for r in out)
  print(json.dumps({'sweep': name, 'all_equal': ok, 'cases': out}))
  return 0 if ok else MISMATCH


if __name__ == '__main__':
  sys.exit(run(sys.argv[1]))
