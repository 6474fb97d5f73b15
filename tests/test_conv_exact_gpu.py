"""The convolution kernels on integer operands against the fp64 reference
(tests/conv_exact_ref.py): bit for bit.

The bf16 kernels (csrc/lsi_conv_igemm.hip, lsi_conv.hip, lsi_conv_wgrad.hip,
lsi_conv_wgrad_igemm.hip, lsi_conv_first.hip) multiply bf16 values and
accumulate in fp32; with small integers every partial sum is exact in any order,
so the output is determined to the last bit: `torch.equal`, no tolerance.  A
dropped or doubled term, a tap that reads a padding pixel as data, a partial
tile that loses a row, a wrong chunk boundary of a split -- each is a failed
equality, where the Gaussian tests of test_conv_gpu.py allow 2^-7 of the largest
entry.  Every case runs the narrow regime (results exactly bf16s: the sharp
one) and the wide one (results in the thousands, rounded once: the store must
round to nearest even).

The only tolerances of this file belong to the batch-norm constants formed from
the epilogue's sums: the mean 2^-22 relative (two roundings, see _check_stats)
and rstd the rtol = 2e-5 of test_conv_gpu.py.

The last section runs every conv_igemm_kernel<RW, NCT, G> build the planner can
choose at small shapes, in child processes (the planner's knobs are read once
per process)."""
import ctypes
import functools
import itertools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_exact_ref as R

pytestmark = pytest.mark.gpu

_ids = lambda c: '-'.join(str(v) for v in c) if isinstance(c, tuple) else str(c)


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


@pytest.fixture
def own_wgrad_everywhere(monkeypatch):
  """lsi_conv2d_wgrad also below the size from which the network uses it."""
  from lsi.nnutils import _hip_conv
  monkeypatch.setattr(_hip_conv, 'IGEMM_WGRAD_MIN_PIXELS', 0)
  monkeypatch.setattr(_hip_conv, 'WGRAD_MIN_PIXELS', 1 << 30)   # (not the row-ring kernel)
  monkeypatch.setattr(_hip_conv, '_WGRAD_BYTES', {})


def _cl(t, dev, dtype=torch.bfloat16):
  return t.to(dev).to(dtype).contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _ref(case, regime):
  """(x, w, gy) as fp32 on the device and the fp64 reference (y, gx, gw),
  computed there once per (case, regime), shared and never modified."""
  dev = torch.device('cuda:0')
  x, w, gy = (t.to(dev) for t in R.operands(case, regime))
  return (x, w, gy), R.reference(case, x, w, gy, regime, groups=R.stats_groups(case))


def _same(name, got, want):
  """torch.equal, and on failure where the mismatches are."""
  assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, got.dtype)
  if torch.equal(got, want):
    return
  bad = (got != want).nonzero()
  lo, hi = bad.min(dim=0).values.tolist(), bad.max(dim=0).values.tolist()
  first = tuple(bad[0].tolist())
  pytest.fail('%s: %d of %d values differ, inside [%s .. %s]; first at %s: got %r, want %r'
              % (name, len(bad), got.numel(), lo, hi, first, float(got[first]),
                 float(want[first])))


def _desc(case):
  from lsi.nnutils import _hip_conv
  if case.kind == 'convt':
    return _hip_conv._conv_desc(case.n, 2 * case.h, 2 * case.w, case.cout, case.h, case.w,
                                case.cin, case.kh, case.kw, 2, 1, 1)
  pt, _, oh = R.same_pads(case.h, case.kh, case.stride)
  pl, _, ow = R.same_pads(case.w, case.kw, case.stride)
  return _hip_conv._conv_desc(case.n, case.h, case.w, case.cin, oh, ow, case.cout, case.kh,
                              case.kw, case.stride, pt, pl)


def _layer(case, x, w, groups=0, precision=None):
  from lsi.nnutils import _hip_conv
  p = precision or _hip_conv.BF16
  if case.kind == 'convt':
    return _hip_conv.conv_transpose2d(x, w, 2, 1, groups, p)
  pt, _, oh = R.same_pads(case.h, case.kh, case.stride)
  pl, _, ow = R.same_pads(case.w, case.kw, case.stride)
  return _hip_conv.conv2d(x, w, case.stride, pt, pl, oh, ow, groups, p)


def _supported(case, x):
  from lsi.nnutils import _hip_conv
  if case.kind == 'convt':
    return _hip_conv.convt_supported(x, case.cin, case.cout, case.kh, 2)
  return _hip_conv.igemm_supported(x, case.cin, case.cout, case.kh, case.stride)


# ---- a. implicit GEMM: forward, data gradient, own weight gradient ----------------

@pytest.mark.parametrize('regime', R.REGIMES)
@pytest.mark.parametrize('case', R.IGEMM + R.IGEMM_T, ids=_ids)
def test_igemm_forward_and_gradients_bit_for_bit(case, regime, dev, own_wgrad_everywhere):
  from lsi.nnutils import _hip_conv
  (x, w, gy), (y64, gx64, gw64) = _ref(case, regime)
  xb = _cl(x, dev).requires_grad_(True)
  wp = w.clone().requires_grad_(True)
  assert _supported(case, xb)
  assert _hip_conv._igemm_wgrad_bytes(_desc(case)) > 0      # (lsi_conv2d_wgrad takes it)
  y = _layer(case, xb, wp)
  assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
  gx, gw = torch.autograd.grad(y, (xb, wp), _cl(gy, dev))
  _same('y', y.detach(), R.as_bf16(y64))
  _same('gx', gx, R.as_bf16(gx64))
  assert gw.dtype == torch.float32
  _same('gw', gw, gw64.float())


# ---- b. the split over the input channels -----------------------------------------

@pytest.mark.parametrize('regime', R.REGIMES)
@pytest.mark.parametrize('case', R.SPLIT, ids=_ids)
def test_split_and_unsplit_contraction_bit_for_bit(case, regime, dev, monkeypatch):
  """Both equal the reference, hence each other: the chunks [i nch / ks,
  (i + 1) nch / ks) of the splits cover every input channel once."""
  from lsi import _C
  from lsi.nnutils import _hip_conv
  (x, w, gy), (y64, gx64, _) = _ref(case, regime)
  d = _desc(case)
  nbytes = [int(_C.lib().lsi_conv2d_workspace_bytes(ctypes.byref(d), m)) for m in (0, 1)]
  assert all(b > 0 for b in nbytes), nbytes                 # (both directions do split)
  for split in (True, False):
    monkeypatch.setattr(_hip_conv, 'SPLITK', split)
    xb = _cl(x, dev).requires_grad_(True)
    y = _layer(case, xb, w)
    gx, = torch.autograd.grad(y, xb, _cl(gy, dev))
    _same('y (split %s)' % split, y.detach(), R.as_bf16(y64))
    _same('gx (split %s)' % split, gx, R.as_bf16(gx64))


# ---- c. the input as two tensors ---------------------------------------------------

@pytest.mark.parametrize('regime', R.REGIMES)
@pytest.mark.parametrize('c1,case', R.CAT, ids=_ids)
def test_two_tensor_variants_bit_for_bit(c1, case, regime, dev, own_wgrad_everywhere):
  """lsi_conv2d_fwd_cat / _bwd_data_cat / _wgrad_cat against the reference of
  the concatenated tensor (not against their sibling kernels)."""
  from lsi.nnutils import _hip_conv
  (x, w, gy), (y64, gx64, gw64) = _ref(case, regime)
  x1 = _cl(x[:, :c1], dev).requires_grad_(True)
  x2 = _cl(x[:, c1:], dev).requires_grad_(True)
  wp = w.clone().requires_grad_(True)
  gyb = _cl(gy, dev)
  pt, _, oh = R.same_pads(case.h, case.kh, 1)
  pl, _, ow = R.same_pads(case.w, case.kw, 1)
  d = _desc(case)
  assert _hip_conv._igemm_wgrad_bytes(d) > 0
  blk = 64 if case.cin % 64 == 0 else 32                    # the data gradient's channel block
  if c1 % blk == 0:
    assert _hip_conv.cat_supported(x1, x2, case.cout, case.kh, 1)
    y = _hip_conv.conv2d_cat(x1, x2, wp, 1, pt, pl, oh, ow)
    g1, g2, gw = torch.autograd.grad(y, (x1, x2, wp), gyb)
    _same('gx1', g1, R.as_bf16(gx64[:, :c1]))
    _same('gx2', g2, R.as_bf16(gx64[:, c1:]))
  else:
    # the data gradient refuses this c1 (so the layer is not routed here); the
    # forward and the weight gradient take it
    assert not _hip_conv.cat_supported(x1, x2, case.cout, case.kh, 1)
    y = _hip_conv._run(_hip_conv.BF16, d, 0, wp, x1.detach(),
                       _hip_conv._empty_cl(case.n, case.cout, oh, ow, dev, torch.bfloat16),
                       x2=x2.detach(), c1=c1)
    gw = _hip_conv._igemm_wgrad(d, x1.detach(), gyb, wp, x2.detach())
    g1 = _hip_conv._empty_cl(case.n, c1, case.h, case.w, dev, torch.bfloat16)
    g2 = _hip_conv._empty_cl(case.n, case.cin - c1, case.h, case.w, dev, torch.bfloat16)
    with pytest.raises(RuntimeError, match='lsi_conv2d_run'):
      _hip_conv._run(_hip_conv.BF16, d, 1, wp, gyb, g1, out2=g2, c1=c1)
  _same('y', y.detach(), R.as_bf16(y64))
  _same('gw', gw, gw64.float())


# ---- d. the statistics of the epilogue ------------------------------------------------

def _check_stats(y, y64, mr, groups):
  """mean / rstd that lsi_bn_relu_norm forms from the sums the convolution left.

  The mean.  The epilogue adds up the values it stores; they are integers and so
  is every partial sum, below 2^24 (guarded): the fp32 sum is exact in any order,
  through the atomics and the fold of the slots.  bn_norm_sums_kernel
  (lsi_bn.hip) then computes inv_n = (float)(1.0 / (double)npix) and mean = sum *
  inv_n: two roundings to fp32 (the double reciprocal's own error, 2^-53, is
  nothing), each at most 2^-24 relative -- (1 + 2^-24)^2 - 1 < 2^-22.  A sum of
  0 gives exactly 0."""
  n, c, oh, ow = y.shape
  yr = R.as_bf16(y64).double().view(groups, n // groups, c, oh, ow)
  assert mr.shape == (groups, 2, c) and mr.dtype == torch.float32
  mean = yr.mean(dim=(1, 3, 4))
  got = mr[:, 0].double()
  zero = yr.sum(dim=(1, 3, 4)) == 0
  assert bool((got[zero] == 0).all())
  over = int(((got - mean).abs() > 2.0 ** -22 * mean.abs()).sum())
  assert over == 0, (over, float(((got - mean).abs() / mean.abs().clamp_min(1e-300)).max()))
  var = yr.var(dim=(1, 3, 4), unbiased=False)
  np.testing.assert_allclose(mr[:, 1].double().cpu().numpy(),
                             torch.rsqrt(var + 1e-3).cpu().numpy(), rtol=2e-5)


@pytest.mark.parametrize('regime', R.REGIMES)
@pytest.mark.parametrize('case,groups', R.STATS, ids=_ids)
def test_epilogue_statistics_leave_the_output_alone_and_are_exact(case, groups, regime, dev):
  from lsi.nnutils import _hip_bn
  (x, w, gy), (y64, _, _) = _ref(case, regime)
  xb = _cl(x, dev)
  y0 = _layer(case, xb, w)
  _same('y', y0, R.as_bf16(y64))
  y1 = _layer(case, xb, w, groups)
  beta = torch.zeros((case.cout,), device=dev, requires_grad=True)
  z1 = _hip_bn.batch_norm_relu(y1, beta, 1e-3, True, groups, True)
  _same('y with statistics', y1, y0)
  _check_stats(y1, y64, z1.grad_fn.saved_tensors[2], groups)


# ---- e. the 32-channel 3 x 3 kernels (lsi_conv.hip, lsi_conv_wgrad.hip) --------------

@pytest.mark.parametrize('regime', R.REGIMES)
@pytest.mark.parametrize('cout', [32, 16])
@pytest.mark.parametrize('shape', R.C32_FWD, ids=_ids)
def test_conv3x3_c32_forward_and_data_gradient_bit_for_bit(shape, cout, regime, dev):
  from lsi.nnutils import _hip_conv
  case = R.c32_case(*shape, cout=cout)
  (x, w, gy), (y64, gx64, _) = _ref(case, regime)
  xb = _cl(x, dev).requires_grad_(True)
  assert _hip_conv.supported(xb, 32, cout, 3, 1, False)
  y = _hip_conv.conv3x3_c32(xb, w)
  _same('y', y.detach(), R.as_bf16(y64))
  if cout == 32:     # (the 16-channel layer's data gradient is the library's)
    gx, = torch.autograd.grad(y, xb, _cl(gy, dev))
    _same('gx', gx, R.as_bf16(gx64))


@pytest.mark.parametrize('shape', R.C32_REFUSED, ids=_ids)
def test_conv3x3_c32_refuses_widths_that_are_no_multiple_of_16(shape, dev):
  """(why the forward cases above stand at 80 and 144 columns instead)"""
  from lsi import _C
  from lsi.nnutils import _hip_conv
  n, h, w = shape
  x = _cl(torch.zeros((n, 32, h, w)), dev)
  assert not _hip_conv.supported(x, 32, 32, 3, 1, False)
  wt = torch.zeros((32, 32, 3, 3), device=dev)
  out = torch.empty_like(x)
  rc = _C.lib().lsi_conv3x3_c32_fwd(n, h, w, 32, 0, _C.ptr(x), _C.ptr(wt), None, 1.0,
                                    _C.ptr(out), _C.stream_ptr(dev))
  assert rc == -1   # LSI_EINVAL


@pytest.mark.parametrize('regime', R.REGIMES)
@pytest.mark.parametrize('shape', R.C32_WGRAD, ids=_ids)
def test_conv3x3_weight_gradient_kernel_bit_for_bit(shape, regime, dev):
  from lsi import _C
  n, h, w, cin, cout = shape
  case = R.c32_case(*shape)
  (x, _, gy), (_, _, gw64) = _ref(case, regime)
  xb, gyb = _cl(x, dev), _cl(gy, dev)
  lib = _C.lib()
  nbytes = lib.lsi_conv3x3_wgrad_workspace_bytes(n, h, w, cin, cout)
  ws = torch.empty((nbytes // 4,), device=dev)
  gw = torch.full((cout, cin, 3, 3), float('nan'), device=dev)
  rc = lib.lsi_conv3x3_wgrad(n, h, w, cin, cout, _C.ptr(xb), _C.ptr(gyb), _C.ptr(gw),
                             _C.ptr(ws), nbytes, _C.stream_ptr(dev))
  assert rc == 0
  _same('gw', gw, gw64.float())


# ---- f. the first convolution (lsi_conv_first.hip) -----------------------------------

@pytest.mark.parametrize('regime', R.REGIMES)
@pytest.mark.parametrize('xdt,layout', [('f32', 'contig'), ('bf16', 'clast')])
@pytest.mark.parametrize('shape', R.FIRST, ids=_ids)
def test_first_convolution_bit_for_bit(shape, xdt, layout, regime, dev):
  """The integer image in fp32 and in bf16 storage, the parameter contiguous and
  with channels-last strides (the weight gradient comes in the same layout)."""
  from lsi.nnutils import _hip_bn, _hip_conv
  case = R.first_case(*shape)
  (x, w, gy), (y64, _, gw64) = _ref(case, regime)
  img = _cl(x, dev, torch.float32 if xdt == 'f32' else torch.bfloat16)  # N x H x W x 3 in memory
  wp = w.clone()
  if layout == 'clast':
    wp = wp.contiguous(memory_format=torch.channels_last)
  wp.requires_grad_(True)
  pt, _, oh = R.same_pads(case.h, 7, 2)
  pl, _, ow = R.same_pads(case.w, 7, 2)
  assert _hip_conv.first_supported(img, 3, 32, 7, 2)
  y = _hip_conv.conv2d_first(img, wp, 2, pt, pl, oh, ow)
  _same('y', y.detach(), R.as_bf16(y64))
  gw, = torch.autograd.grad(y, wp, _cl(gy, dev))
  assert gw.dtype == torch.float32 and gw.stride() == wp.stride()
  _same('gw', gw, gw64.float())
  for groups in sorted(set((1, case.n))):
    y1 = _hip_conv.conv2d_first(img, wp, 2, pt, pl, oh, ow, groups)
    beta = torch.zeros((32,), device=dev, requires_grad=True)
    z1 = _hip_bn.batch_norm_relu(y1, beta, 1e-3, True, groups, True)
    _same('y with statistics', y1.detach(), y.detach())
    _check_stats(y1, y64, z1.grad_fn.saved_tensors[2], groups)


# ---- g. the fp32 family: the same operands, the same host side -----------------------

@pytest.mark.parametrize('regime', R.REGIMES)
@pytest.mark.parametrize('case', R.F32 + R.F32_T, ids=_ids)
def test_fp32_family_bit_for_bit(case, regime, dev):
  from lsi.nnutils import _hip_conv
  (x, w, gy), (y64, gx64, gw64) = _ref(case, regime)
  xf = _cl(x, dev, torch.float32).requires_grad_(True)
  wp = w.clone().requires_grad_(True)
  assert _hip_conv.f32_wgrad_bytes(_desc(case)) > 0         # (lsi_conv2d_wgrad_f32 takes it)
  used = _hip_conv.USED_F32[0]
  y = _layer(case, xf, wp, 0, _hip_conv.F32)
  gx, gw = torch.autograd.grad(y, (xf, wp), _cl(gy, dev, torch.float32))
  assert _hip_conv.USED_F32[0] - used == 3
  assert y.dtype == torch.float32
  _same('y', y.detach(), y64.float())
  _same('gx', gx, gx64.float())
  _same('gw', gw, gw64.float())


# ---- h. the fp32 pack's edge tiles (D0 or D1 no multiple of 32) -------------------------

@pytest.mark.parametrize('regime', R.REGIMES)
@pytest.mark.parametrize('layout', ['contig', 'clast'])
@pytest.mark.parametrize('case', R.F32_EDGE, ids=_ids)
def test_fp32_pack_edge_tiles_bit_for_bit(case, layout, regime, dev):
  """Output channels that end inside a 32 x 32 tile of the pack: only the C
  entries reach them (a layer wants both directions, and the data gradient
  refuses Cout % 32 != 0).  lsi_conv2d_f32_pack + lsi_conv2d_f32_run (mode 0)
  and, where it takes the shape, lsi_conv2d_wgrad_f32; the parameter contiguous
  and with channels-last strides (the pack's and the fold's tr & 2 paths)."""
  from lsi import _C
  from lsi.nnutils import _hip_conv
  assert case.cout % 32 != 0 and case.cout % 16 == 0
  (x, w, gy), (y64, _, gw64) = _ref(case, regime)
  d = _desc(case)
  assert _C.lib().lsi_conv2d_f32_supported(ctypes.byref(d))
  xf = _cl(x, dev, torch.float32)
  wp = w.clone()
  if layout == 'clast':
    wp = wp.contiguous(memory_format=torch.channels_last)
  assert _hip_conv._pack_layout(wp) == (2 if layout == 'clast' else 0)
  oh, ow = R.out_size(case)
  y = _hip_conv._run(_hip_conv.F32, d, 0, wp, xf,
                     _hip_conv._empty_cl(case.n, case.cout, oh, ow, dev, torch.float32))
  _same('y', y, y64.float())
  if _hip_conv.f32_wgrad_bytes(d) > 0:
    gw = _hip_conv._wgrad(_hip_conv.F32, d, xf, _cl(gy, dev, torch.float32), wp)
    assert gw.dtype == torch.float32 and gw.stride() == wp.stride()
    _same('gw', gw, gw64.float())


# ---- every build of conv_igemm_kernel the planner can choose --------------------------
#
# 30 of the 32 instantiations are reached; the two that are not, and why:
#   <8, 4, 9> and <8, 4, 7>: a tile of 32 rows has a patch of at least 32 x 16
#     pixels x 80 bytes = 40960 bytes, and 9 (7) taps of 64 output channels are
#     46080 (35840) bytes more: over the 81920-byte LDS share with the smallest
#     patch there is (7 taps in one row or column make it 32 x 22 or 38 x 16).
#     ig_shape() then takes G = 5 or 4 (3 x 3 at RW = 8 runs <8, 4, 5>).  No
#     descriptor reaches them; no knob changes that.

ALL_BUILDS = set(itertools.product((8, 4, 2, 1), (4, 2), (9, 7, 5, 4)))
UNREACHABLE = {(8, 4, 9), (8, 4, 7)}
# what each child's plan lines must report, exactly (RW, NCT, G)
DECLARED = {
    'rw8': {(8, 4, 5), (8, 4, 4), (8, 2, 9), (8, 2, 7), (8, 2, 5), (4, 2, 9), (4, 2, 7),
            (4, 2, 5)},
    'rw8_classes': {(8, 4, 4), (8, 2, 4), (2, 4, 5), (2, 2, 4)},
    'rw4': {(4, 4, 9), (4, 4, 7), (4, 4, 5), (4, 4, 4), (4, 2, 9), (4, 2, 7), (4, 2, 5),
            (4, 2, 4), (2, 4, 5), (2, 4, 4), (2, 2, 4)},
    'rw2': set(itertools.product((2,), (4, 2), (9, 7, 5, 4))),
    'rw1': set(itertools.product((1,), (4, 2), (9, 7, 5, 4))),
}
CHILD_SECONDS = {'rw8': 90, 'rw8_classes': 90, 'rw4': 60, 'rw2': 60, 'rw1': 60}
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_exact_child.py')
_PLAN = re.compile(r'^ig N(\d+) .* ncls (\d+) taps \d+: RW (\d+) NCT (\d+) G (\d+) '
                   r'grid (\d+) x (\d+) x (\d+) = \d+ WGs \(ks (\d+)\)')
# a child that crashed, hung or faulted: nothing further is started on the device
_SWEEP = {'broken': None, 'done': {}}


def _child(name):
  """The verdict and the plans of one sweep, run once per session."""
  if name in _SWEEP['done']:
    return _SWEEP['done'][name]
  if _SWEEP['broken']:
    pytest.fail('not started: an earlier sweep ended abnormally (%s)' % _SWEEP['broken'])
  env = dict(os.environ)
  env.update(R.sweep_env(name))
  try:
    p = subprocess.run([sys.executable, CHILD, name], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True,
                       timeout=CHILD_SECONDS[name])
  except subprocess.TimeoutExpired:
    _SWEEP['broken'] = '%s: no end after %d s' % (name, CHILD_SECONDS[name])
    pytest.fail(_SWEEP['broken'])
  if p.returncode not in (0, 3):
    _SWEEP['broken'] = '%s: exit status %d' % (name, p.returncode)
    pytest.fail('%s\n%s' % (_SWEEP['broken'], p.stderr[-2000:]))
  verdict = json.loads(p.stdout.strip().splitlines()[-1])
  plans = []
  for line in p.stderr.splitlines():
    m = _PLAN.match(line)
    if m:
      n, ncls, rw, nct, g, gx, gy, gz, ks = (int(v) for v in m.groups())
      plans.append({'build': (rw, nct, g), 'ncls': ncls, 'ks': ks, 'tiles': gx * gy * n})
  _SWEEP['done'][name] = (p.returncode, verdict, plans)
  return _SWEEP['done'][name]


@pytest.mark.parametrize('name', list(R.SWEEPS))
def test_sweep_of_kernel_builds_bit_for_bit(name, dev):
  rc, verdict, plans = _child(name)
  bad = [c for c in verdict['cases'] if c['y'] or c['gx']]
  assert rc == 0 and verdict['all_equal'] and not bad, bad
  cases = R.SWEEPS[name][1]
  assert [tuple(c['case']) for c in verdict['cases']] == [tuple(c) for c in cases]
  assert len(plans) == 2 * len(cases), len(plans)           # forward + data gradient each
  assert set(p['build'] for p in plans) == DECLARED[name]


def test_sweeps_reach_every_build_and_both_block_orders(dev):
  plans = [p for name in R.SWEEPS for p in _child(name)[2]]
  assert set(p['build'] for p in plans) == ALL_BUILDS - UNREACHABLE
  assert set().union(*DECLARED.values()) == ALL_BUILDS - UNREACHABLE
  assert len(UNREACHABLE) <= 4
  # stride-2 parity classes (ncls = 4); among them a launch that takes the XCD
  # swizzle (>= 512 tiles, a multiple of 8, unsplit: ig_launch) at RW = 8 and
  # below, and one of >= 512 tiles that cannot
  par = [p for p in plans if p['ncls'] == 4 and p['ks'] == 1]
  assert any(p['tiles'] >= 512 and p['tiles'] % 8 == 0 and p['build'][0] == 8 for p in par)
  assert any(p['tiles'] >= 512 and p['tiles'] % 8 == 0 and p['build'][0] < 8 for p in par)
  assert any(p['tiles'] >= 512 and p['tiles'] % 8 != 0 for p in par)
