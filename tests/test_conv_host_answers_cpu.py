"""What the host side of the bf16 and fp32 implicit-GEMM convolutions answers,
against the library from before the two families were given one host side
(csrc/lsi_conv_host.h): for every descriptor below and both precisions
`*_supported`, `*_packed_bytes`, `*_workspace_bytes` (modes 0, 1, 2), the weight
gradient's `*_workspace_bytes`, every `*_pack_job` (modes 0 - 3: return code,
block count, the whole filled LsiPackJob) and the refusal codes of the pack and
weight-gradient entries with every pointer NULL or misaligned in turn.

No call here can reach a launch: the pack entries are called with
`packed_bytes = 0` and the weight-gradient entries with `workspace_bytes = 0`,
and that size check is the last one before the first device call (the fully
valid call returns LSI_EWORKSPACE).  lsi_conv2d_run / lsi_conv2d_f32_run have no
such last guard, so the few refused calls recorded for them run only where no
device is visible: a wrongly accepted one would launch on dummy addresses.

conv_host_answers.json holds one line per descriptor; run this module as a script
to record it from the library in the tree (LSI_HIP_LIB selects another build):
`python tests/test_conv_host_answers_cpu.py [out.json]`.
"""
import ctypes
import json
import os
import sys

import pytest

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_host_answers.json')

# name -> (supported, packed_bytes, pack, pack_job, workspace_bytes, run,
#          wgrad_workspace_bytes, {weight-gradient entry: its pointer arguments})
_WG5 = ['x1', 'x2', 'gy', 'g_weight', 'workspace']
PRECISIONS = {
    'bf16': ('lsi_conv2d_supported', 'lsi_conv2d_packed_bytes', 'lsi_conv2d_pack',
             'lsi_conv2d_pack_job', 'lsi_conv2d_workspace_bytes', 'lsi_conv2d_run',
             'lsi_conv2d_wgrad_workspace_bytes',
             {'lsi_conv2d_wgrad': ['x', 'gy', 'g_weight', 'workspace'],
              'lsi_conv2d_wgrad_cat': _WG5}),
    'f32': ('lsi_conv2d_f32_supported', 'lsi_conv2d_f32_packed_bytes', 'lsi_conv2d_f32_pack',
            'lsi_conv2d_f32_pack_job', 'lsi_conv2d_f32_workspace_bytes', 'lsi_conv2d_f32_run',
            'lsi_conv2d_wgrad_f32_workspace_bytes', {'lsi_conv2d_wgrad_f32': _WG5}),
}
GRID_LIMIT = (2048, 4, 4, 64, 4, 4, 2048, 3, 3, 1, 1, 1)   # grid.z = 2048 x 2048 / 64 > 65535


def _same(size, k, s):
  out = -(-size // s)
  return out, max((out - 1) * s + k - size, 0) // 2


def _conv(n, h, w, cin, cout, k, s):
  (oh, pt), (ow, pl) = _same(h, k, s), _same(w, k, s)
  return (n, h, w, cin, oh, ow, cout, k, k, s, pt, pl)


def _convt(n, h, w, cin, cout):
  """A transposed 4 x 4 stride-2 convolution h x w -> 2h x 2w: the data gradient
  of this descriptor."""
  return (n, 2 * h, 2 * w, cout, h, w, cin, 4, 4, 2, 1, 1)


def _network(n, h=256, w=768):
  """Every convolution of the U-Net and the two heads (reference nets.py:244-348)."""
  out, cin = [], 3
  for cout, k, s in [(32, 7, 2), (32, 7, 1), (64, 5, 2), (64, 5, 1), (128, 3, 2), (128, 3, 1),
                     (256, 3, 2), (256, 3, 1), (512, 3, 2), (512, 3, 1), (512, 3, 2),
                     (512, 3, 1), (512, 3, 2), (512, 3, 1)]:
    out.append(_conv(n, h, w, cin, cout, k, s))
    h, w, cin = -(-h // s), -(-w // s), cout
  for ci, co, skip in [(512, 512, 512), (512, 512, 512), (512, 256, 256), (256, 128, 128),
                       (128, 128, 64), (128, 64, 32), (64, 32, 0)]:
    out.append(_convt(n, h, w, ci, co))
    h, w = 2 * h, 2 * w
    out.append(_conv(n, h, w, co + skip, co, 3, 1))
  out.append(_conv(n, h, w, 32, 4, 3, 1))   # the heads' prediction layer
  return out


def descriptors():
  import test_conv_f32_gpu as f32_cases
  ds = _network(4) + _network(8)
  ds += [_conv(*c) for c in f32_cases.CONV] + [_convt(*c) for c in f32_cases.CONVT]
  ds += [
      _conv(2, 8, 8, 32, 16, 3, 1), _conv(2, 8, 8, 32, 24, 3, 1), _conv(2, 8, 8, 48, 32, 3, 1),
      _conv(2, 16, 16, 32, 32, 9, 1), _conv(2, 9, 9, 32, 32, 3, 3),
      (2, 8, 8, 32, 8, 8, 32, 3, 3, 1, 3, 1), (2, 8, 8, 32, 8, 8, 32, 3, 3, 1, 1, 4),   # pad >= K
      (2, 8, 8, 32, 9, 8, 32, 3, 3, 1, 1, 1), (2, 9, 9, 64, 5, 6, 32, 3, 3, 2, 0, 0),   # OH, OW + 1
      (2, 8, 8, 32, 11, 8, 32, 3, 3, 1, 1, 1),   # the last output rows read no input
      _conv(8, 1024, 2048, 128, 32, 3, 1),    # N H W Cin = 2^31
      _conv(8, 1024, 2048, 32, 128, 3, 1),    # N OH OW Cout = 2^31
      GRID_LIMIT,
  ]
  return ds


def _struct(_C, geo):
  d = _C.LsiConvDesc()
  (d.N, d.H, d.W, d.Cin, d.OH, d.OW, d.Cout, d.KH, d.KW, d.stride, d.pad_t, d.pad_l) = geo
  return d


def _in_turn(call, n):
  """The codes of call(pointers): all set, then each NULL, then each misaligned."""
  ptrs = [0x10000 + 0x1000 * i for i in range(n)]
  out = [call(ptrs)]
  for bad in (lambda p: None, lambda p: p + 4):
    for i in range(n):
      out.append(call(ptrs[:i] + [bad(ptrs[i])] + ptrs[i + 1:]))
  return out


def answers(_C, geo, precision):
  lib = _C.lib()
  sup, pbytes, pack, pack_job, ws, _, wg_ws, wgrads = PRECISIONS[precision]
  d = _struct(_C, geo)
  ref = ctypes.byref(d)
  a = {'sup': getattr(lib, sup)(ref), 'pb': getattr(lib, pbytes)(ref),
       'ws': [getattr(lib, ws)(ref, m) for m in (0, 1, 2)], 'wg': getattr(lib, wg_ws)(ref)}
  jobs = []
  for mode in range(4):
    job, nb = _C.LsiPackJob(), ctypes.c_int32(-1)
    rc = getattr(lib, pack_job)(ref, mode, 0x10000, 0x20000, 1 << 40, ctypes.byref(job),
                                ctypes.byref(nb))
    jobs.append([rc, nb.value] + ([job.w or 0, job.dst or 0, job.D0, job.D1, job.khw, job.tr,
                                   job.ntaps, job.block0, list(job.tap)] if rc == 0 else []))
  a['job'] = jobs
  # packed_bytes = 0: (weight, packed), for pack_job also (job, nblocks), in turn
  a['pack'] = [_in_turn(lambda p: getattr(lib, pack)(ref, m, p[0], p[1], 0, None), 2)
               for m in (0, 1)]
  job, nb = _C.LsiPackJob(), ctypes.c_int32(0)
  a['pack_job'] = _in_turn(lambda p: getattr(lib, pack_job)(
      ref, 1, p[0], p[1], 0, ctypes.byref(job) if p[2] else None,
      ctypes.byref(nb) if p[3] else None), 4)[:7]   # (no misaligned job / nblocks)
  a['pack_null'] = [getattr(lib, pack)(None, 0, 0x10000, 0x20000, 0, None),
                    getattr(lib, pack_job)(None, 0, 0x10000, 0x20000, 0, ctypes.byref(job),
                                           ctypes.byref(nb))]
  # workspace_bytes = 0; the two-tensor entries with c1 = 32 and layout 0 | 2 | 1
  for name, args in wgrads.items():
    fn = getattr(lib, name)
    if len(args) == 4:
      a[name] = (_in_turn(lambda p: fn(ref, p[0], p[1], p[2], p[3], 0, None), 4) +
                 [fn(None, 0x10000, 0x11000, 0x12000, 0x13000, 0, None)])
    else:
      a[name] = sum((_in_turn(lambda p: fn(ref, p[0], p[1], 32, p[2], p[3], lay, p[4], 0, None),
                              5) for lay in (0, 2, 1)), [])
      a[name].append(fn(None, 0x10000, 0x11000, 32, 0x12000, 0x13000, 0, 0x14000, 0, None))
  return a


def record(_C):
  return [{'d': list(geo), 'bf16': answers(_C, geo, 'bf16'), 'f32': answers(_C, geo, 'f32')}
          for geo in descriptors()]


def run_refusals(_C):
  """Calls of lsi_conv2d[_f32]_run that the library refuses before its launch:
  the grid-limit geometry, mode 2, and a second output tensor in mode 0."""
  lib = _C.lib()
  out = {}
  for precision, names in PRECISIONS.items():
    run = getattr(lib, names[5])
    io = _C.LsiConvIO()
    io.x, io.packed, io.out = 0x10000, 0x20000, 0x30000
    two = _C.LsiConvIO()
    two.x, two.packed, two.out, two.out2, two.c1 = 0x10000, 0x20000, 0x30000, 0x40000, 32
    small = _struct(_C, _conv(2, 8, 8, 64, 64, 3, 1))
    out[precision] = [
        run(ctypes.byref(_struct(_C, GRID_LIMIT)), 0, ctypes.byref(io), None),
        run(ctypes.byref(small), 2, ctypes.byref(io), None),
        run(ctypes.byref(small), 0, ctypes.byref(two), None)]
  return out


@pytest.fixture(scope='module')
def recorded():
  with open(DATA) as f:
    return json.load(f)


def test_host_answers_are_those_of_the_recorded_library(built_lib, recorded):
  from lsi import _C
  want = recorded['descriptors']
  geos = descriptors()
  assert [w['d'] for w in want] == [list(g) for g in geos]
  taken = 0
  for geo, w in zip(geos, want):
    for precision in PRECISIONS:
      got = json.loads(json.dumps(answers(_C, geo, precision)))
      diff = {k: (got[k], w[precision].get(k)) for k in got if got[k] != w[precision].get(k)}
      assert not diff and sorted(got) == sorted(w[precision]), (
          '%s %s: {answer: (library, recorded)} %s' % (geo, precision, diff))
      taken += got['sup']
      # no call went past its size check: every code is a refusal
      for k in ('pack', 'pack_job', 'pack_null') + tuple(PRECISIONS[precision][7]):
        codes = sum(got[k], []) if k == 'pack' else got[k]
        assert all(-5 <= c < 0 for c in codes), (geo, precision, k, codes)
  assert taken >= 100   # (the list is mostly layers the kernels take)


def test_run_refusals_are_those_of_the_recorded_library(built_lib, recorded):
  import torch
  if torch.cuda.is_available():
    pytest.skip('a wrongly accepted call would launch on dummy addresses')
  from lsi import _C
  got = run_refusals(_C)
  assert got == recorded['run_refusals']
  assert all(c < 0 for codes in got.values() for c in codes)
  # (the grid limit is LSI_EINVAL in bf16 and LSI_EUNSUPPORTED in fp32)
  assert (got['bf16'][0], got['f32'][0]) == (-1, -5)


if __name__ == '__main__':
  _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  sys.path.insert(0, os.path.join(_root, 'layered-scene-inference_amd'))
  import torch as _torch
  from lsi import _C as _c
  assert not _torch.cuda.is_available(), 'record the run refusals where no device is visible'
  with open(sys.argv[1] if len(sys.argv) > 1 else DATA, 'w') as _f:
    _f.write('{"run_refusals": %s,\n "descriptors": [\n%s\n]}\n' % (
        json.dumps(run_refusals(_c)),
        ',\n'.join(json.dumps(r, separators=(',', ':')) for r in record(_c))))
