"""The fp32 convolution entries of the C ABI (include/lsi_hip.h:
lsi_conv2d_f32_*, lsi_conv2d_wgrad_f32*) on the host, no GPU needed: what they
take, the workspace they plan, and that every refusal comes back before any
launch (LSI_EUNSUPPORTED / LSI_EINVAL / LSI_ENULL) -- plus the Python switch
(nets.F32_CONV, --fp32_convs) and its default."""
import ctypes
import sys

import pytest
import torch

from conftest import PKG

EUNSUPPORTED, EINVAL, ENULL = -5, -1, -2


@pytest.fixture(scope='module')
def lib(built_lib):
  from lsi import _C
  return _C.lib()


def _desc(n, h, w, cin, cout, k, s, pad=None):
  from lsi.nnutils import _hip_conv
  oh, ow = -(-h // s), -(-w // s)
  p = max((oh - 1) * s + k - h, 0) // 2 if pad is None else pad
  return _hip_conv._conv_desc(n, h, w, cin, oh, ow, cout, k, k, s, p, p)


def test_supported_shapes(lib):
  ok = lambda d: lib.lsi_conv2d_f32_supported(ctypes.byref(d))
  assert ok(_desc(8, 256, 768, 32, 32, 3, 1)) == 1        # upcnv1b
  assert ok(_desc(8, 256, 768, 32, 32, 7, 1)) == 1        # cnv1b
  assert ok(_desc(8, 128, 384, 32, 64, 5, 2)) == 1        # cnv2
  assert ok(_desc(8, 2, 6, 512, 512, 3, 1)) == 1          # cnv7b
  assert ok(_desc(2, 8, 8, 32, 16, 3, 1)) == 1            # Cout a multiple of 16
  assert ok(_desc(2, 8, 8, 48, 32, 3, 1)) == 0            # Cin not a multiple of 32
  assert ok(_desc(2, 8, 8, 3, 32, 7, 2)) == 0             # cnv1: the image
  assert ok(_desc(2, 8, 8, 32, 24, 3, 1)) == 0            # Cout not a multiple of 16
  assert ok(_desc(2, 8, 8, 32, 32, 9, 1)) == 0            # kernel over 7 x 7
  assert ok(_desc(2, 8, 8, 32, 32, 3, 3)) == 0            # stride 3
  assert lib.lsi_conv2d_f32_supported(None) == 0
  assert lib.lsi_conv2d_f32_packed_bytes(ctypes.byref(_desc(2, 8, 8, 64, 32, 3, 1))) == \
      9 * 64 * 32 * 4
  assert lib.lsi_conv2d_f32_packed_bytes(ctypes.byref(_desc(2, 8, 8, 48, 32, 3, 1))) == 0


def test_workspaces(lib):
  ws = lambda d, m: lib.lsi_conv2d_f32_workspace_bytes(ctypes.byref(d), m)
  wg = lambda d: lib.lsi_conv2d_wgrad_f32_workspace_bytes(ctypes.byref(d))
  # the bottleneck maps split over the input channels, the large maps do not
  d = _desc(8, 4, 12, 512, 512, 3, 1)
  assert ws(d, 0) > 0 and ws(d, 0) % (8 * 4 * 12 * 512 * 4) == 0
  assert ws(_desc(8, 256, 768, 32, 32, 3, 1), 0) == 0
  assert ws(d, 2) == 0 and ws(_desc(2, 8, 8, 48, 32, 3, 1), 0) == 0
  # data gradient of a Cout-16 layer: its input would be 16 channels
  assert ws(_desc(2, 8, 8, 32, 16, 3, 1), 1) == 0
  # the weight gradient: partial sums of whole [tap][Cout][Cin] blocks, <= 96 MB
  for d in (_desc(8, 256, 768, 32, 32, 3, 1), d, _desc(8, 128, 384, 32, 64, 5, 2)):
    n = wg(d)
    per = d.Cout * d.Cin * d.KH * d.KW * 4
    assert 0 < n <= 96 << 20 and n % per == 0
  assert wg(_desc(2, 8, 8, 48, 32, 3, 1)) == 0


def test_refusals_come_before_any_launch(lib):
  """Pointers here are never dereferenced: every call returns before a kernel
  could be launched (there is no device on this machine)."""
  from lsi import _C
  run = lambda d, m, io: lib.lsi_conv2d_f32_run(ctypes.byref(d), m, ctypes.byref(io), None)
  io = _C.LsiConvIO()
  io.x, io.packed, io.out = 0x10000, 0x20000, 0x30000
  assert run(_desc(2, 8, 8, 48, 32, 3, 1), 0, io) == EUNSUPPORTED   # Cin % 32
  assert run(_desc(2, 8, 8, 32, 16, 3, 1), 1, io) == EUNSUPPORTED   # dgrad input 16
  d = _desc(2, 8, 8, 32, 32, 3, 1)
  assert run(d, 2, io) == EINVAL
  for field in ('x', 'packed', 'out'):
    bad = _C.LsiConvIO()
    bad.x, bad.packed, bad.out = io.x, io.packed, io.out
    setattr(bad, field, getattr(io, field) + 4)                      # misaligned
    assert run(d, 0, bad) == EUNSUPPORTED, field
  bad = _C.LsiConvIO()
  bad.x, bad.packed, bad.out, bad.x2, bad.c1 = io.x, io.packed, io.out, 0x40004, 16
  assert run(_desc(2, 8, 8, 64, 32, 3, 1), 0, bad) == EUNSUPPORTED   # x2 misaligned
  bad.x2 = 0x40000
  assert run(_desc(2, 8, 8, 64, 32, 3, 1), 0, bad) == EINVAL         # c1 % 32
  bad = _C.LsiConvIO()
  bad.x, bad.packed, bad.out, bad.bn_workspace = io.x, io.packed, io.out, 0x50000
  assert run(d, 0, bad) == EUNSUPPORTED          # no batch-norm sums in the epilogue
  bad = _C.LsiConvIO()
  bad.x, bad.out = io.x, io.out
  assert run(d, 0, bad) == ENULL
  # weight gradient
  wgr = lambda d, x, x2, c1, gy, lay=0: lib.lsi_conv2d_wgrad_f32(
      ctypes.byref(d), x, x2, c1, gy, 0x60000, lay, 0x70000, 1 << 30, None)
  assert wgr(_desc(2, 8, 8, 48, 32, 3, 1), 0x10000, None, 0, 0x20000) == EUNSUPPORTED
  assert wgr(d, 0x10004, None, 0, 0x20000) == EUNSUPPORTED
  assert wgr(d, 0x10000, None, 0, 0x20008) == EUNSUPPORTED
  assert wgr(d, 0x10000, None, 0, 0x20000, lay=1) == EINVAL
  assert wgr(_desc(2, 8, 8, 64, 32, 3, 1), 0x10000, 0x30000, 16, 0x20000) == EINVAL
  assert lib.lsi_conv2d_wgrad_f32(ctypes.byref(d), 0x10000, None, 0, 0x20000, 0x60000, 0,
                                  0x70000, 16, None) == -3           # workspace too small
  # packing
  assert lib.lsi_conv2d_f32_pack(ctypes.byref(_desc(2, 8, 8, 48, 32, 3, 1)), 0, 0x10000,
                                 0x20000, 1 << 20, None) == EUNSUPPORTED
  assert lib.lsi_conv2d_f32_pack(ctypes.byref(d), 0, 0x10000, 0x20004, 1 << 20,
                                 None) == EINVAL
  assert lib.lsi_conv2d_f32_pack(ctypes.byref(d), 0, 0x10000, 0x20000, 16, None) == -3


def test_pack_jobs_list_the_taps_in_parity_class_order(lib):
  from lsi import _C
  job, nb = _C.LsiPackJob(), ctypes.c_int32(0)
  d = _desc(2, 16, 16, 64, 32, 4, 2, pad=1)
  assert lib.lsi_conv2d_f32_pack_job(ctypes.byref(d), 1, 0x10000, 0x20000, 1 << 20,
                                     ctypes.byref(job), ctypes.byref(nb)) == 0
  taps = list(job.tap[:16])
  # four classes of 2 x 2 taps: every tap once
  assert sorted(taps) == list(range(16)) and nb.value == 2 * 1
  assert job.tr == 1 and job.D0 == 32 and job.D1 == 64
  assert lib.lsi_conv2d_f32_pack_job(ctypes.byref(d), 0, 0x10000, 0x20000, 1 << 20,
                                     ctypes.byref(job), ctypes.byref(nb)) == 0
  assert list(job.tap[:16]) == list(range(16))


def test_switch_is_off_by_default_and_routes_nothing_on_the_cpu(monkeypatch):
  sys.path.insert(0, PKG)
  monkeypatch.delenv('LSI_F32_CONV', raising=False)
  import ldi_enc_dec as script
  from lsi.nnutils import nets
  opts = script.build_parser().parse_args([])
  assert opts.fp32_convs == 'library'
  assert script.build_parser().parse_args(['--fp32_convs', 'own']).fp32_convs == 'own'
  monkeypatch.setenv('LSI_F32_CONV', '1')
  assert script.build_parser().parse_args([]).fp32_convs == 'own'
  x = torch.zeros((1, 32, 8, 8)).contiguous(memory_format=torch.channels_last)
  monkeypatch.setattr(nets, 'F32_CONV', True)
  assert not nets._f32_route(x)                  # (CPU tensors: never)
  layer = nets.SlimConv2d(32, 32, 3, 1)
  assert layer(x).shape == (1, 32, 8, 8)
