"""The skinny fully-connected kernels (csrc/lsi_fc.hip: fc_stream_kernel<MT>,
fc_fold_fwd_kernel, fc_fold_kernel, fc_prep_bwd_kernel, fc_dw_kernel<FAST_K>) on
integer operands against the fp64 reference of tests/fc_exact_ref.py.

a. Without batch norm every output is determined bit for bit (integers below
   2^24, any summation order): `torch.equal`, no tolerance -- forward, dX and dW,
   every weight layout the kernels read in place, bf16 and fp32 activations and
   outputs, one or both gradients requested, at the shapes where a step, a tile,
   a lane block or a chunk is partial.
b. With batch norm the inputs of the epilogue are those exact integers, and
   everything after is held to absolute bounds against fp64 that follow from
   the fp32 arithmetic alone (test_batch_norm_against_fp64 derives them).
c. The C ABI with a workspace of exactly lsi_fc_workspace_bytes and a guard
   behind every buffer: nothing is written outside.
d. Every run of a and b happens twice and gives the same bits."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import fc_exact_ref as R

pytestmark = pytest.mark.gpu

U32 = R.U32
PAIRS = [(c, g) for c in R.all_cases() for g in R.regimes(c)]
_pid = lambda p: R.ident(p) if isinstance(p, R.Case) else str(p)
FLAGS = [(False, False), (False, True), (True, False), (True, True)]   # (x fp32, y fp32)


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _ref(case, regime):
  """(x, gy, the parameter, its geometry) on the device and the fp64 reference
  (Z, dX, dW) computed there, once per (case, regime), shared, never modified."""
  dev = torch.device('cuda:0')
  x, w, gy, junk = R.operands(case, regime)
  param = R.parameter(case, R.scatter(case, w, junk), dev)
  x, w, gy = x.to(dev), w.to(dev), gy.to(dev)
  return (x, gy, param, R.lib_geometry(case, param)), R.reference(case, x, w, gy, regime)


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


def _run(x, param, gy, geo, x_f32, out_f32, want_dx=True, want_dw=True, beta=None, groups=1):
  """One forward and backward through the binding: (y, dx, dw, dbeta), None for
  what was not requested.  beta: with batch norm."""
  from lsi.nnutils import _hip_fc
  xin = (x if x_f32 else x.bfloat16()).clone().requires_grad_(want_dx)
  wp = param.detach().requires_grad_(want_dw)
  assert wp.data_ptr() == param.data_ptr() and wp.stride() == param.stride()
  bp = None if beta is None else beta.clone().requires_grad_(True)
  assert _hip_fc.supported(xin, wp, geo, groups, beta is not None, out_f32)
  y = _hip_fc.fc(xin, wp, bp, geo, bn=beta is not None, eps=R.EPS, groups=groups,
                 out_f32=out_f32)
  assert y.dtype == (torch.float32 if out_f32 else torch.bfloat16)
  ins = [t for t, on in ((xin, want_dx), (wp, want_dw), (bp, bp is not None)) if on]
  grads = list(torch.autograd.grad(y, ins, gy if out_f32 else gy.bfloat16()))
  dx = grads.pop(0) if want_dx else None
  dw = grads.pop(0) if want_dw else None
  db = grads.pop(0) if bp is not None else None
  if dx is not None:
    assert dx.dtype == xin.dtype and dx.shape == xin.shape
  if dw is not None:
    assert dw.dtype == torch.float32 and dw.stride() == param.stride()
  return y.detach(), dx, dw, db


# ---- a. without batch norm: bit for bit (d: twice) ----------------------------------

@pytest.mark.parametrize('case,regime', PAIRS, ids=_pid)
def test_product_and_gradients_bit_for_bit(case, regime, dev):
  (x, gy, param, geo), (z64, dx64, dw64) = _ref(case, regime)
  tag = R.ident(case) + ' ' + regime
  dw_want = R.scatter(case, dw64.float())       # zero where the geometry addresses nothing
  for x_f32, out_f32 in FLAGS:
    t = '%s x %s y %s: ' % (tag, 'f32' if x_f32 else 'bf16', 'f32' if out_f32 else 'bf16')
    y, dx, dw, _ = _run(x, param, gy, geo, x_f32, out_f32)
    _same(t + 'y', y, z64.float() if out_f32 else R.as_bf16(z64))
    _same(t + 'dx', dx, dx64.float() if x_f32 else R.as_bf16(dx64))
    _same(t + 'dw', R.storage_of(case, dw), dw_want)
    # one gradient requested: the same bits
    _, dx1, none, _ = _run(x, param, gy, geo, x_f32, out_f32, want_dw=False)
    assert none is None
    _same(t + 'dx alone', dx1, dx)
    _, none, dw1, _ = _run(x, param, gy, geo, x_f32, out_f32, want_dx=False)
    assert none is None
    _same(t + 'dw alone', R.storage_of(case, dw1), dw_want)
    # run to run
    y2, dx2, dw2, _ = _run(x, param, gy, geo, x_f32, out_f32)
    assert torch.equal(y2, y) and torch.equal(dx2, dx) and torch.equal(dw2, dw)
  # the parameter was read, not written
  assert torch.equal(R.storage_of(case, param).cpu(),
                     R.scatter(case, *R.operands(case, regime)[1::2]))


@pytest.mark.parametrize('regime', R.REGIMES)
@pytest.mark.parametrize('case', [c for c in R.CASES if c.layout.startswith('convt')], ids=_pid)
def test_transposed_convolution_entry_bit_for_bit(case, regime, dev):
  """_hip_fc.conv_transpose_1x1 against fp64 F.conv_transpose2d of the whole 4 x 4
  weight, whose outer taps hold integers of their own: they meet no pixel of a
  1 x 1 map, and their gradient is exactly zero."""
  from lsi.nnutils import _hip_fc
  (x, gy, param, geo), _ = _ref(case, regime)
  m, cin, cout = case.m, case.k, case.n // 4
  x64 = x.double().view(m, cin, 1, 1).requires_grad_(True)
  w64 = param.double().requires_grad_(True)
  y64 = F.conv_transpose2d(x64, w64, stride=2, padding=1)
  g4 = gy.view(m, 2, 2, cout).permute(0, 3, 1, 2)             # columns are (oy, ox, cout)
  gx64, gw64 = torch.autograd.grad(y64, (x64, w64), g4.double())
  R.guards(case, regime, y64.detach(), gx64, gw64)
  outer = gw64.clone()
  outer[:, :, 1:3, 1:3] = 0
  assert float(outer.abs().max()) == 0.0 and float(param.abs().sum()) > float(
      param[:, :, 1:3, 1:3].abs().sum())
  got = []
  for _ in range(2):
    xb = x.bfloat16().view(m, cin, 1, 1).requires_grad_(True)
    wp = param.detach().requires_grad_(True)
    y = _hip_fc.conv_transpose_1x1(xb, wp)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (m, cout, 2, 2)
    gx, gw = torch.autograd.grad(y, (xb, wp), g4.bfloat16())
    assert gw.stride() == param.stride()
    _same('y', y.detach().contiguous(), R.as_bf16(y64.detach()))
    _same('gx', gx, R.as_bf16(gx64))
    _same('gw', gw.contiguous(), gw64.float())
    got.append((y.detach(), gx, gw))
  assert all(torch.equal(a, b) for a, b in zip(*got))


# ---- b. with batch norm: absolute bounds against fp64 -------------------------------

@functools.lru_cache(maxsize=None)
def _bn_ref(case):
  dev = torch.device('cuda:0')
  x, w, gy, beta = (t.to(dev) for t in R.bn_operands(case))
  return (x, w, gy, beta), R.bn_reference(case, x, w, gy, beta)


def _half_ulp_bf16(t):
  """Half the spacing of the bf16s at t (fp64 holding bf16 values), 0 at 0: a value
  rounds to t only from within that distance (half of it, below a power of two)."""
  _, e = torch.frexp(t.abs())
  return torch.where(t == 0, torch.zeros_like(t), torch.pow(2.0, e.double() - 9))


def _between(name, got, lo, hi, ref, bound, where=None, rounded=False):
  """Asserts lo <= got <= hi (on `where`).  Returns, for the report, the worst
  error / bound: |got - ref| / bound, and for a quantity the kernel rounded to bf16
  the least error of the value it rounded that the stored bf16 admits,
  max(0, |got - ref| - half a bf16 ulp) / bound."""
  ok = (got >= lo) & (got <= hi)
  err = (got - ref).abs()
  if rounded:
    err = (err - _half_ulp_bf16(got)).clamp_min(0)
  ratio = err / bound.clamp_min(1e-300)
  if where is not None:
    ok = ok | ~where
    ratio = ratio * where
  if not bool(ok.all()):
    first = tuple((~ok).nonzero()[0].tolist())
    pytest.fail('%s: %d of %d values outside their bound (worst error / bound %.3f); first '
                'at %s: got %r, allowed [%r, %r], fp64 %r'
                % (name, int((~ok).sum()), ok.numel(), float(ratio.max()), first,
                   float(got[first]), float(lo[first]), float(hi[first]), float(ref[first])))
  return float(ratio.max())


@pytest.mark.parametrize('case', R.BN_CASES, ids=_pid)
def test_batch_norm_against_fp64(case, dev):
  """relu(bn(Z) + beta) and its backward on exact integer Z, against fp64, within
  bounds that follow from the fp32 arithmetic.  u = 2^-24; r = rows per group;
  all sums below are over the r rows of one (group, column) pair; first-order
  terms throughout, the quadratic ones covered by a factor 1 + 2^-10 (asserted
  to suffice in fc_exact_ref.dz_bound).  FMA contraction or not: a contracted
  operation drops one of the roundings counted here.

  Z.  x, w are small integers with X[:, :M] = I: Z read back without batch norm
  is bit-equal to the fp64 Z.  Every bound below is about the epilogue alone.

  Forward.  E32 of test_fc_gpu.py::test_batch_norm_relu_epilogue,
      E32 = 2 u (r + 8) (A + |x^| + |v|),   A = rstd max|z|, x^ = (z - mean) rstd,
  v = x^ + beta, bounds the distance of two fp32 evaluations and so that of one
  from fp64.  fp32 y within E32 of relu(v); bf16 y = the nearest-even rounding of
  that fp32 y, bit for bit.  r = 1: mean = z, x^ = 0 exactly, y = relu(beta)
  exactly (E32 = 0).

  ReLU mask.  A (group, column) pair is DECIDED when |v| > 4 E32 in all its rows:
  the kernel's mask y > 0 is then the reference's.  Undecided pairs are left out
  of the dbeta and dZ checks, counted, printed, and may be at most 1 % of a case.

  dbeta = sum_m g_m, g = gy where y > 0: at most 32 small integers, exact; checked
  on the columns all of whose pairs are decided.

  dZ = rstd ((g - s1) - x^ s2), s1 = mean(g), s2 = mean(g x^).  What the kernel
  (fc_prep_bwd_kernel, with mean and rstd as fc_fold_fwd_kernel stored them)
  rounds to bf16 differs from that by at most E:
    mean   = fl(fl(sum z) fl(1 / r)), the sum exact (integers, r max|z| < 2^24):
             |d mean| <= 2 u |mean| <= 2 u max|z|.
    d      = fl(z - mean): |d d| <= 2 u max|z| + u |d|.
    var    = the sum of r squares of d (r u), scaled (2 u), + eps (u); the errors
             of d enter as 2 sum |d| |d d| / r <= 4 u max|z| sigma + 2 u sigma^2,
             and sigma rstd <= 1: relative error of var + eps
             <= u (4 A + r + 5).
    rstd   = 1 / sqrt(.): half of that + 4 u (sqrt and divide, each allowed a
             whole ulp): rho <= u (2 A + r / 2 + 6.5) -- used as u (2 A + r / 2 + 9)
             =: u P, which also covers the two roundings of x^ = fl(fl(z - mean) rstd).
    x^     : |d x^| <= rstd |d d| + |x^| (rho + u) <= u (2 A + |x^| P) =: u X.
    s1     = fl(fl(sum g) fl(1 / r)), the sum exact: |d s1| <= 2 u |s1|.
    s2     : products (u), r - 1 additions, scaling (2 u):
             |d s2| <= u mean(|g| (X + (r + 2) |x^|)) =: u S.
    g - s1 : |.| <= 2 u |s1| + u |g - s1|.
    x^ s2  : |.| <= u (X |s2| + |x^| S + |x^ s2|).
    the difference c = (g - s1) - x^ s2: + u |c|;  times rstd: + (rho + u) |dZ|.
      E = u { rstd [ 2 |s1| + |g - s1| + X |s2| + |x^| S + |x^ s2| + |c| ]
              + |dZ| (P + 1) } (1 + 2^-10).
  The kernel's dZ is recovered from dW[:, :M] (X[:, :M] = I: exact, see
  test_fc_exact_cpu.py) and must be a bf16 with
      as_bf16(ref - E) <= dZ <= as_bf16(ref + E):
  rounding is monotone, so this allows one rounding of a value within E and
  nothing more.  r = 1: dZ = 0 exactly.

  dX and dW are then checked against fp64 products of that dZ -- the kernel's own,
  now verified -- within the summation bound of test_fc_gpu.py::_check_product,
  R u sum |a| |b| with R = N for dX = dZ W (W: integers, bf16s as they are) and
  R = M for dW = dZ^T X; a bf16 dX is one monotone rounding of a value within it.

  Measured on an MI355X, worst error / bound over all cases and flags (for a bf16
  quantity: the least error of the rounded value that the stored bf16 admits):
  y 0.059, dZ 0.15, dX 0.0011, dW 0.35; one (group, column) pair of 520 left out
  at (17, 1), none elsewhere.  Each line is printed per case."""
  (x, w, gy, beta), ref = _bn_ref(case)
  m, n, k, grp, r = case.m, case.n, case.k, case.groups, case.m // case.groups
  geo = R.geometry(case)
  tag = R.ident(case)
  z = _run(x, w, gy, geo, False, True)[0]
  _same(tag + ' z', z, ref['z'].float())

  decided = ref['decided']                                    # (groups, N)
  left_out = 1.0 - float(decided.double().mean())
  print('%s: %d of %d (group, column) pairs left out (%.3f %%)'
        % (tag, int((~decided).sum()), decided.numel(), 100 * left_out))
  assert left_out <= 0.01
  rows_ok = decided[:, None, :].expand(grp, r, n).reshape(m, n)
  cols_ok = decided.all(dim=0)
  e_dz = R.dz_bound(ref)
  dz_lo = R.as_bf16(ref['dz'] - e_dz).double()
  dz_hi = R.as_bf16(ref['dz'] + e_dz).double()

  y32 = {}
  for x_f32, out_f32 in sorted(FLAGS, key=lambda f: not f[1]):       # fp32 outputs first
    t = '%s x %s y %s' % (tag, 'f32' if x_f32 else 'bf16', 'f32' if out_f32 else 'bf16')
    y, dx, dw, db = _run(x, w, gy, geo, x_f32, out_f32, beta=beta, groups=grp)
    if out_f32:
      y32[x_f32] = y
      r_y = _between(t + ' y', y.double(), ref['y'] - ref['e32'], ref['y'] + ref['e32'], ref['y'],
                     ref['e32'])
      if r == 1:
        _same(t + ' y, one row per group', y, torch.relu(beta).expand(m, n).contiguous())
    else:
      r_y = float('nan')
      _same(t + ' y', y, y32[x_f32].bfloat16())
      assert bool((y >= 0).all())
    # dbeta: exact where the mask is decided
    assert db.dtype == torch.float32 and tuple(db.shape) == (n,)
    _same(t + ' dbeta', db[cols_ok], ref['dbeta'].float()[cols_ok])
    # dZ from the identity block
    dz = dw[:, :m].t().contiguous()
    _same(t + ' dZ is a bf16', dz.bfloat16().float(), dz)
    r_dz = _between(t + ' dZ', dz.double(), dz_lo, dz_hi, ref['dz'], e_dz, rows_ok, rounded=True)
    if r == 1:
      assert float(dz.abs().max()) == 0.0
    # dX = dZ W and dW = dZ^T X in fp64 from the kernel's dZ
    dzd, wd, xd = dz.double(), w.double(), x.double()
    want = dzd @ wd
    bound = n * U32 * (dzd.abs() @ wd.abs())
    lo, hi = want - bound, want + bound
    if not x_f32:
      lo, hi = R.as_bf16(lo).double(), R.as_bf16(hi).double()
    r_dx = _between(t + ' dX', dx.double(), lo, hi, want, bound, rounded=not x_f32)
    want = dzd.t() @ xd
    bound = m * U32 * (dzd.abs().t() @ xd.abs())
    r_dw = _between(t + ' dW', dw.double(), want - bound, want + bound, want, bound)
    print('%s: error / bound  y %.3e  dZ %.3e  dX %.3e  dW %.3e' % (t, r_y, r_dz, r_dx, r_dw))
    # run to run
    again = _run(x, w, gy, geo, x_f32, out_f32, beta=beta, groups=grp)
    for a, b in zip((y, dx, dw, db), again):
      assert torch.equal(a, b), t


# ---- c. the C ABI: exact workspace, guards behind every buffer ----------------------

GUARD = 4096
LSI_EWORKSPACE = -3      # include/lsi_hip.h
PATTERN = 0xA5
ABI_CASES = [R.lin(3, 40, 24), R.lin(17, 264, 520), R.convt(8, 40, 24, 'convt_cl')]


class _Guarded(object):
  """`nbytes` bytes on the device between two guards of GUARD bytes each; guards
  and body start as PATTERN."""

  def __init__(self, nbytes, dev, dtype, init=None):
    self.raw = torch.full((2 * GUARD + nbytes,), PATTERN, dtype=torch.uint8, device=dev)
    self.body = self.raw[GUARD:GUARD + nbytes].view(dtype)
    if init is not None:
      self.body.copy_(init.reshape(-1))
    self.ptr = self.body.data_ptr()
    self.nbytes = nbytes
    assert self.ptr % 16 == 0

  def guards_intact(self):
    return bool((self.raw[:GUARD] == PATTERN).all()) and \
        bool((self.raw[GUARD + self.nbytes:] == PATTERN).all())

  def untouched(self):
    return bool((self.raw == PATTERN).all())


def _abi_buffers(case, x, gy, param, x_f32, out_f32, dev):
  m, k, n = case.m, case.k, case.n
  xt, yt = (torch.float32 if x_f32 else torch.bfloat16), (torch.float32 if out_f32 else
                                                           torch.bfloat16)
  sx, sy = (4 if x_f32 else 2), (4 if out_f32 else 2)
  flat = R.storage_of(case, param)
  taps = R.geometry(case)[2]
  b = {'x': _Guarded(m * k * sx, dev, xt, x.to(xt)),
       'w': _Guarded(flat.numel() * 4, dev, torch.float32, flat),
       'dy': _Guarded(m * n * sy, dev, yt, gy.to(yt)),
       'y': _Guarded(m * n * sy, dev, yt),
       'z': _Guarded(m * n * 4, dev, torch.float32),
       'mean_rstd': _Guarded(case.groups * 2 * n * 4, dev, torch.float32),
       'dx': _Guarded(m * k * sx, dev, xt),
       # (elements of a tapped weight that no (n, k) addresses are the caller's: zero)
       'dw': _Guarded(flat.numel() * 4, dev, torch.float32,
                      torch.zeros_like(flat) if taps > 1 else None),
       'dbeta': _Guarded(n * 4, dev, torch.float32),
       'ws': _Guarded(R.workspace_bytes(case), dev, torch.uint8)}
  return b


def _abi_call(lib, d, b, beta, stream, ws_bytes):
  dref = ctypes.byref(d)
  bp = None if beta is None else beta.data_ptr()
  rc_f = lib.lsi_fc_fwd(dref, b['x'].ptr, b['w'].ptr, bp, b['y'].ptr, b['z'].ptr,
                        b['mean_rstd'].ptr, b['ws'].ptr, ws_bytes, stream)
  rc_b = lib.lsi_fc_bwd(dref, b['x'].ptr, b['w'].ptr, b['dy'].ptr, b['y'].ptr, b['z'].ptr,
                        b['mean_rstd'].ptr, b['dx'].ptr, b['dw'].ptr, b['dbeta'].ptr,
                        b['ws'].ptr, ws_bytes, stream)
  torch.cuda.synchronize()
  return rc_f, rc_b


@pytest.mark.parametrize('bn', [False, True], ids=['plain', 'bn'])
@pytest.mark.parametrize('case', ABI_CASES, ids=_pid)
def test_c_abi_writes_inside_its_buffers(case, bn, dev):
  """lsi_fc_fwd / lsi_fc_bwd with a workspace of exactly lsi_fc_workspace_bytes
  and 4 KiB of a fixed pattern before and behind the workspace and every input
  and output.  Without batch norm (bf16 in and out) the results are the exact
  ones of section a; with it (fp32 in and out) those of the binding, bit for bit.
  A workspace 256 bytes short: LSI_EWORKSPACE from both entries, nothing runs."""
  from lsi import _C
  from lsi.nnutils import _hip_fc
  lib = _C.lib()
  (x, gy, param, geo), (z64, dx64, dw64) = _ref(case, 'narrow')
  assert geo == R.geometry(case)
  x_f32 = out_f32 = bn
  flags = (_C.LSI_FC_BN | _C.LSI_FC_X_F32 | _C.LSI_FC_OUT_F32) if bn else 0
  d = R.descriptor(case, flags, R.EPS)
  need = int(lib.lsi_fc_workspace_bytes(ctypes.byref(d)))
  assert need == R.workspace_bytes(case) and need % 256 == 0
  beta = None
  if bn:
    beta = (0.5 * torch.randn(case.n, generator=torch.Generator().manual_seed(5))).to(dev)
  stream = _C.stream_ptr(dev)

  # one unit short: refused by both entries before anything is launched
  b = _abi_buffers(case, x, gy, param, x_f32, out_f32, dev)
  assert _abi_call(lib, d, b, beta, stream, need - 256) == (LSI_EWORKSPACE,) * 2
  for name in ('y', 'z', 'mean_rstd', 'dx', 'dbeta', 'ws'):
    assert b[name].untouched(), name
  assert b['dw'].guards_intact() and (case.layout == 'convt_cl' or b['dw'].untouched())

  assert _abi_call(lib, d, b, beta, stream, need) == (_C.LSI_OK, _C.LSI_OK)
  for name, buf in b.items():
    assert buf.guards_intact(), name
  m, k, n = case.m, case.k, case.n
  y, z, dx = b['y'].body.view(m, n), b['z'].body.view(m, n), b['dx'].body.view(m, k)
  _same('z', z, z64.float())
  if not bn:
    _same('y', y, R.as_bf16(z64))
    _same('dx', dx, R.as_bf16(dx64))
    _same('dw', b['dw'].body, R.scatter(case, dw64.float()))
    assert b['mean_rstd'].untouched() and b['dbeta'].untouched()
  else:
    y_b, dx_b, dw_b, db_b = _run(x, param, gy, geo, True, True, beta=beta, groups=case.groups)
    _same('y', y, y_b)
    _same('dx', dx, dx_b)
    _same('dw', b['dw'].body, R.storage_of(case, dw_b))
    _same('dbeta', b['dbeta'].body, db_b)
    assert not b['mean_rstd'].untouched()
    assert bool(torch.isfinite(b['mean_rstd'].body).all())
  # the inputs were only read
  assert torch.equal(b['w'].body, R.storage_of(case, param))
  assert torch.equal(b['x'].body.view(m, k), x.to(b['x'].body.dtype))
