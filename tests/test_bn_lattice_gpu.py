"""The batch-norm kernels (csrc/lsi_bn.hip: statistics, normalise, the one-pass
normalise behind a producer's sums, backward statistics, dx) against the fp64
restatement tests/bn_lattice_ref.py on lattice activations, where every sum
the kernels form is exact in fp32 in any order -- per thread, through LDS and
through the atomics.

Every other batch-norm test compares floats against one scalar bar per tensor
and leaves the ReLU's kink out.  Here nothing is left out:

* two-pass forward (lsi_bn_relu_fwd): mean_rstd and y equal the restatement
  with torch.equal at every shape -- one lost, doubled or misplaced pixel, a
  group that reads its neighbour's slice or constants, a bf16 store that does
  not round to nearest even is a failed equality;
* one-pass forward (lsi_bn_relu_norm, sums from _leave_sums and from the real
  convolution epilogue) and backward (lsi_bn_relu_bwd, through autograd and by
  ctypes on the reference's own mean_rstd): equal where npix is a power of two
  (the exact set), elsewhere inside the bars below; dbeta, an integer sum, is
  equal everywhere;
* y == 0 exactly where z <= 0 and dz = 0 exactly there: the scenes hold z == 0
  at a quarter of a channel's pixels, so a forward that masks z < 0 next to a
  backward that passes z >= 0 fails;
* after every call the counter, tag and accumulator words of every group's
  workspace block are zero bit for bit.
No kink mask, no outlier share: the lattice leaves no decision open.

The bars of the bounded set (npix a multiple of 4, no power of two; the sums
are still exact, the reference is fp64; U = 2^-24).
  dx     |dx - dx64| <= K U A, A = |rstd| (|dz| + |c1| + |xhat| |c2|), K = 4.
         c1 = fl(fl(1 / n) S1): two roundings; c2 the same two, and one more on
         xhat * c2; each subtraction rounds its result, which is at most the
         sum of the absolute values it has seen; rstd is a power of two.  In
         units of U: 2 |c1| + (|dz| + |c1|) + 3 |xhat c2| + (|dz| + |c1| +
         |xhat c2|) = 2 |dz| + 4 |c1| + 4 |xhat c2| <= 4 A / |rstd|.
         The fp32 op graph in torch reaches 2.20 on the same scenes
         (test_bn_lattice_cpu.py, pin 2.4): K = 4 <= 4 x 2.4.
  mean   one pass: 2^-23 |mean| (fl(1 / n), the product).
  rstd   one pass: rstd U ((3 m^2 + 1.5 v) / (v + eps) + 3) -- bar_rstd derives it.
  y      one pass: (rstd |mean - m| + |xhat| (rho + U) + U |z|) (1 + 2^-10), rho
         the bar of rstd relative to it -- bar_y derives it.
  bf16   a result stored as bf16 is rounded once more: half an ulp of 8 bits,
         + 2^-8 (|want| + bar).
The one-pass forward's gradient is taken on the exact set only: where its mean
and rstd carry a rounding, the mask of an element at z == 0 is theirs to
decide, and lsi_bn_relu_bwd is held to the bar on exact statistics instead.

MEASURED below is the record of the run on the MI355X; the bars are the bars.
Every equality the exact rule claims held there -- 496 tensor comparisons with
torch.equal, the statistics behind the real convolutions included, which equal
the kernel's fp32 finish carried out in exact arithmetic with one rounding per
operation -- and the bounded set stayed at 2.10 of K = 4.  csrc/lsi_bn.hip is
unchanged but for the launch-shape query."""
import fractions
import functools
import random

import numpy as np
import pytest
import torch

import bn_lattice_ref as R
import conv_exact_ref as CR
from test_bn_stats_gpu import WS_ACC, WS_STRIDE, _leave_sums

pytestmark = pytest.mark.gpu

WS_CONST = WS_ACC + 4096      # csrc/lsi_bn_ws.h: LSI_BN_WS_CONST

# worst error seen on the MI355X, (fp32, bf16).  dx: |dx - dx64| / (U A) in fp32
# (K = 4 is the bar), error / bar in bf16 (the bf16 rounding leads: a value just
# above a power of two sits 2^-8 of itself from its neighbours' midpoint); the
# one-pass quantities: error / bar.  0: every value was equal to the fp64 one --
# on the lattice fl(1 / n) * (n m) rounds back to the integer m, and rstd with it.
# The convolution's outputs are bf16 only.
MEASURED = {
    'lsi_bn_relu_bwd (autograd)': dict(dx=(2.103, 0.996)),
    'lsi_bn_relu_bwd (ctypes)': dict(dx=(2.103, 0.996)),
    'lsi_bn_relu_norm': dict(mean=(0.0, 0.0), rstd=(0.0, 0.0), y=(0.0, 0.996)),
    'lsi_bn_relu_norm behind a convolution': dict(mean=(None, 0.926), rstd=(None, 0.376),
                                                  y=(None, 0.969)),
}
WORST = {}   # filled by the run: (entry point, dtype, quantity) -> ratio
COUNTS = {}  # (entry point, 'equal' | 'bounded') -> comparisons made

_ids = lambda c: '-'.join(str(v) for v in c) if isinstance(c, tuple) else str(c)
_dt = lambda bf16: 'bf16' if bf16 else 'fp32'


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def _count(tag, kind):
  COUNTS[(tag, kind)] = COUNTS.get((tag, kind), 0) + 1


def _where(bad):
  idx = bad.nonzero()
  return (len(idx), idx.min(dim=0).values.tolist(), idx.max(dim=0).values.tolist(),
          tuple(idx[0].tolist()))


def _same(name, got, want, tag):
  """Bit for bit; on failure the count, the bounding box and the first one."""
  assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, got.dtype)
  _count(tag, 'equal')
  if torch.equal(got, want):
    return
  n, lo, hi, first = _where(got != want)
  pytest.fail('%s: %d of %d values differ, inside [%s .. %s]; first at %s: got %r, want %r'
              % (name, n, got.numel(), lo, hi, first, float(got[first]), float(want[first])))


def _within(name, got, want, bar, tag, key, unit=None):
  """|got - want| <= bar per element (fp64); records the worst error / unit."""
  assert got.shape == want.shape, (name, got.shape, want.shape)
  _count(tag, 'bounded')
  err = (got.double() - want).abs()
  unit = bar if unit is None else unit
  pos = unit > 0
  ratio = float((err[pos] / unit[pos]).max()) if bool(pos.any()) else 0.0
  WORST[key] = max(WORST.get(key, 0.0), ratio)
  bad = ~(err <= bar)
  if bool(bad.any()):
    n, lo, hi, first = _where(bad)
    pytest.fail('%s: %d of %d values beyond the bound, inside [%s .. %s]; first at %s: got %r, '
                'want %r, bound %.3e' % (name, n, got.numel(), lo, hi, first, float(got[first]),
                                         float(want[first]), float(bar[first])))


def _big(case, bf16):
  return case.groups * case.npix * R.channels(case, bf16) >= R.BIG


def _make(case, bf16):
  """The scene on the device and the kernels' operands: x, dy as channels-last
  groups x C x 2 x npix / 2 tensors over [groups][npix][C] memory, beta."""
  dev = 'cuda:0'
  if _big(case, bf16):
    sc = R.scene.__wrapped__(case, bf16, dev)
  else:
    sc = R.scene(case, bf16)
    sc = sc._replace(x=sc.x.to(dev), dy=sc.dy.to(dev), beta=sc.beta.to(dev))
  G, n, C = sc.x.shape
  dt = torch.bfloat16 if bf16 else torch.float32
  cl = lambda t: t.to(dt).view(G, 2, n // 2, C).permute(0, 3, 1, 2)
  x4, dy4 = cl(sc.x), cl(sc.dy)
  assert x4.is_contiguous(memory_format=torch.channels_last) and x4.data_ptr() % 16 == 0
  return sc, (x4, dy4, sc.beta)


_make_kept = functools.lru_cache(maxsize=None)(_make)
_restate_kept = functools.lru_cache(maxsize=None)(
    lambda case, bf16, relu: R.restate(_make_kept(case, bf16)[0], relu))


def _ref(case, bf16, relu):
  """(scene, operands, restatement): computed on the device once per (case,
  dtype, relu), shared and never modified; the two scenes of 40 M and 80 M
  elements are not kept."""
  if _big(case, bf16):
    sc, ops = _make(case, bf16)
    return sc, ops, R.restate(sc, relu)
  sc, ops = _make_kept(case, bf16)
  return sc, ops, _restate_kept(case, bf16, relu)


def _flat(t):
  """groups x C x 2 x npix / 2 (channels-last) -> [groups, npix, C]."""
  G, C, h, w = t.shape
  return t.permute(0, 2, 3, 1).reshape(G, h * w, C)


def _clean(x4, groups, what):
  """The workspace contract: counter, tag and accumulators of every group's
  block are zero bit for bit after the call."""
  from lsi.nnutils import _hip_bn
  ws = _hip_bn.stats_workspace(tuple(x4.shape), x4.device, int(x4.dtype == torch.bfloat16),
                               groups)
  words = ws[:groups * WS_STRIDE].view(torch.int32).view(groups, WS_STRIDE)[:, :WS_CONST]
  left = words != 0
  if bool(left.any()):
    n, lo, hi, first = _where(left)
    pytest.fail('%s: %d workspace words left nonzero, inside [%s .. %s]; first (group, word) '
                '%s = 0x%08x' % (what, n, lo, hi, first, int(words[first]) & 0xffffffff))


def _forward(ops, groups, relu, one_pass):
  """-> (y, mean_rstd, the leaves) through _hip_bn.batch_norm_relu."""
  from lsi.nnutils import _hip_bn
  x4, _, beta = ops
  xq = x4.detach().requires_grad_(True)
  bq = beta.clone().requires_grad_(True)
  assert _hip_bn.supported(xq, groups)
  if one_pass:
    _leave_sums(x4, groups)
  y = _hip_bn.batch_norm_relu(xq, bq, R.EPS, bool(relu), groups, one_pass)
  _clean(x4, groups, 'forward')
  return y, y.grad_fn.saved_tensors[2], (xq, bq)


def _bwd_ctypes(ops, mean_rstd, groups, relu):
  """lsi_bn_relu_bwd on statistics the caller supplies -> (dx, dbeta)."""
  from lsi import _C
  from lsi.nnutils import _hip_bn
  x4, dy4, beta = ops
  G, C, h, w = x4.shape
  assert G == groups and mean_rstd.shape == (G, 2, C) and mean_rstd.dtype == torch.float32
  assert mean_rstd.is_contiguous() and beta.shape == (C,) and beta.dtype == torch.float32
  bf16 = int(x4.dtype == torch.bfloat16)
  ws = _hip_bn.stats_workspace(tuple(x4.shape), x4.device, bf16, groups)
  assert ws.numel() >= groups * WS_STRIDE
  dx = torch.empty_like(x4)
  assert dx.stride() == x4.stride() and dy4.stride() == x4.stride()
  dbeta = torch.full((C,), float('nan'), device=x4.device)
  rc = _C.lib().lsi_bn_relu_bwd(x4.data_ptr(), dy4.data_ptr(), mean_rstd.data_ptr(),
                                beta.data_ptr(), dx.data_ptr(), dbeta.data_ptr(), ws.data_ptr(),
                                h * w, C, bf16, int(relu), groups, _C.stream_ptr(x4.device))
  assert rc == 0, rc
  _clean(x4, groups, 'lsi_bn_relu_bwd')
  return dx, dbeta


def _want_mr(r):
  return torch.stack([r.mean, r.rstd], 1).float()


def _check_statistics_and_y(what, r, bf16, relu, y, mr, tag, exact):
  if exact:
    _same(what + ' mean_rstd', mr, _want_mr(r), tag)
    _same(what + ' y', _flat(y.detach()), R.stored(r.y, bf16), tag)
    return
  key = lambda q: (tag, _dt(bf16), q)
  _within(what + ' mean', mr[:, 0], r.mean, R.bar_mean(r), tag, key('mean'))
  _within(what + ' rstd', mr[:, 1], r.rstd, R.bar_rstd(r), tag, key('rstd'))
  _within(what + ' y', _flat(y.detach()), r.y, R.bar_y(r, relu, bf16), tag, key('y'))


def _check_mask(what, r, y):
  """y == 0 exactly where the reference has z <= 0 (relu = 1)."""
  got = _flat(y.detach()) == 0
  want = r.z <= 0
  if not torch.equal(got, want):
    n, lo, hi, first = _where(got != want)
    pytest.fail('%s: the mask differs at %d elements, inside [%s .. %s]; first at %s: z = %r'
                % (what, n, lo, hi, first, float(r.z[first])))


def _check_gradients(what, case, r, bf16, dx, dbeta, tag):
  _same(what + ' dbeta', dbeta, r.dbeta.float(), tag)
  if R.exact(case):
    R.assert_backward_is_fp32(r)
    _same(what + ' dx', _flat(dx), R.stored(r.dx, bf16), tag)
  elif bf16:
    _within(what + ' dx', _flat(dx), r.dx, R.bar_dx(r, True), tag, (tag, 'bf16', 'dx'))
  else:
    _within(what + ' dx', _flat(dx), r.dx, R.bar_dx(r, False), tag, (tag, 'fp32', 'dx'),
            unit=R.U * r.A)


_EVERY = dict(argnames='case,bf16,relu',
              argvalues=[(c, b, r) for c in R.CASES for b in (False, True) for r in (0, 1)],
              ids=['%s-%s-relu%d' % (_ids(c), _dt(b), r)
                   for c in R.CASES for b in (False, True) for r in (0, 1)])


# ---- 1. the routes -------------------------------------------------------------------

@pytest.mark.parametrize(**_EVERY)
def test_two_pass_forward_and_autograd_backward(case, bf16, relu, dev):
  """lsi_bn_relu_fwd, then lsi_bn_relu_bwd through autograd on the statistics
  the forward saved: the forward is exact at every shape."""
  sc, ops, r = _ref(case, bf16, relu)
  what = 'two-pass %s %s relu %d' % (_ids(case), _dt(bf16), relu)
  y, mr, leaves = _forward(ops, case.groups, relu, False)
  _check_statistics_and_y(what, r, bf16, relu, y, mr, 'lsi_bn_relu_fwd', True)
  if relu:
    _check_mask(what, r, y)
  dx, dbeta = torch.autograd.grad(y, leaves, ops[1])
  _clean(ops[0], case.groups, what + ' backward')
  _check_gradients(what, case, r, bf16, dx, dbeta, 'lsi_bn_relu_bwd (autograd)')


@pytest.mark.parametrize(**_EVERY)
def test_one_pass_forward_on_sums_left_in_the_slots(case, bf16, relu, dev):
  """lsi_bn_relu_norm behind _leave_sums (exact sums of x and x^2 spread over
  the slots, the hand-over tag): exact where npix is a power of two -- its
  gradient then, too --, inside the bars elsewhere."""
  sc, ops, r = _ref(case, bf16, relu)
  what = 'one-pass %s %s relu %d' % (_ids(case), _dt(bf16), relu)
  y, mr, leaves = _forward(ops, case.groups, relu, True)
  _check_statistics_and_y(what, r, bf16, relu, y, mr, 'lsi_bn_relu_norm', R.exact(case))
  if R.exact(case):
    if relu:
      _check_mask(what, r, y)
    dx, dbeta = torch.autograd.grad(y, leaves, ops[1])
    _clean(ops[0], case.groups, what + ' backward')
    _check_gradients(what, case, r, bf16, dx, dbeta, 'lsi_bn_relu_bwd (autograd)')


@pytest.mark.parametrize(**_EVERY)
def test_backward_on_the_reference_statistics(case, bf16, relu, dev):
  """lsi_bn_relu_bwd by ctypes, mean_rstd from the restatement: the backward
  on its own exact inputs."""
  sc, ops, r = _ref(case, bf16, relu)
  what = 'ctypes %s %s relu %d' % (_ids(case), _dt(bf16), relu)
  dx, dbeta = _bwd_ctypes(ops, _want_mr(r), case.groups, relu)
  _check_gradients(what, case, r, bf16, dx, dbeta, 'lsi_bn_relu_bwd (ctypes)')


# ---- 2. forward and backward take the same mask -----------------------------------------

@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', [R.Case(16, 64, 3), R.Case(16, 260, 3)], ids=_ids)
def test_forward_and_backward_take_the_same_mask_at_z_equal_0(case, bf16, dev):
  """y == 0 exactly where z <= 0, and dx is the gradient that masks exactly
  those elements: the restatement with z >= 0 as the backward's mask differs
  from what the kernels give at elements with z == 0 and nowhere else in dz."""
  sc, ops, r = _ref(case, bf16, 1)
  at_zero = (r.z == 0) & (sc.dy != 0)
  assert int(at_zero.sum()) >= case.npix // 4
  y, mr, leaves = _forward(ops, case.groups, 1, False)
  _check_mask('mask', r, y)
  assert bool((_flat(y.detach())[r.z > 0] > 0).all())
  for route in ('autograd', 'ctypes'):
    if route == 'autograd':
      dx, dbeta = torch.autograd.grad(y, leaves, ops[1])
    else:
      dx, dbeta = _bwd_ctypes(ops, _want_mr(r), case.groups, 1)
    _check_gradients('mask ' + route, case, r, bf16, dx, dbeta, 'lsi_bn_relu_bwd (%s)' % route)
    ge = R.restate(sc, 1, mask_ge=True)
    assert not torch.equal(dbeta, ge.dbeta.float())
    assert not torch.equal(_flat(dx), R.stored(ge.dx, bf16))


# ---- 3. the one-pass route behind the real convolution ----------------------------------

def _f32(fr):
  """A rational rounded once to fp32, to nearest even."""
  v = np.float32(float(fr))
  best = None
  for c in (np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))):
    d = abs(fractions.Fraction(float(c)) - fr)
    even = int(np.float32(c).view(np.uint32)) & 1 == 0
    if best is None or d < best[0] or (d == best[0] and even and not best[2]):
      best = (d, np.float32(c), even)
  return best[1]


def _fp32_finish(S, Q, npix, eps):
  """bn_norm_sums_kernel's finish on exact integer sums, every operation rounded
  once: inv = (float)(1 / n), mean = S inv, var = max(fma(-mean, mean, Q inv), 0),
  rstd = 1 / sqrt(var + eps)."""
  F = fractions.Fraction
  inv = F(float(np.float32(1.0 / npix)))
  mean, rstd = [], []
  for s, q in zip(S, Q):
    m = _f32(F(int(s)) * inv)
    e2 = _f32(F(int(q)) * inv)
    var = max(_f32(F(float(e2)) - F(float(m)) ** 2), np.float32(0))
    w = _f32(F(float(var)) + F(float(np.float32(eps))))
    rstd.append(np.float32(1) / np.sqrt(np.float32(w)))
    mean.append(m)
  return np.array(mean, np.float32), np.array(rstd, np.float32)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('case', [CR.IGEMM[0], CR.IGEMM_T[0]], ids=_ids)
def test_one_pass_forward_behind_the_real_convolution(case, relu, dev):
  """The hand-over chain end to end: a 3 x 3 and a transposed convolution on
  the integer operands of conv_exact_ref.py (narrow regime: the epilogue's sums
  of y and y^2 are exact integers, guarded there) leave the sums of two groups,
  lsi_bn_relu_norm consumes them.  mean and rstd equal the kernel's fp32 finish
  carried out on the exact sums with every operation rounded once; y is held
  to the one-pass bar against fp64."""
  from lsi.nnutils import _hip_bn, _hip_conv
  groups, tag = 2, 'lsi_bn_relu_norm behind a convolution'
  x, w, _ = (t.to(dev) for t in CR.operands(case, 'narrow'))
  y64, _, _ = CR.reference(case, x, w, None, 'narrow', want_gw=False, groups=(groups,))
  xb = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
  if case.kind == 'convt':
    y1 = _hip_conv.conv_transpose2d(xb, w, 2, 1, groups, _hip_conv.BF16)
  else:
    pt, _, oh = CR.same_pads(case.h, case.kh, case.stride)
    pl, _, ow = CR.same_pads(case.w, case.kw, case.stride)
    y1 = _hip_conv.conv2d(xb, w, case.stride, pt, pl, oh, ow, groups, _hip_conv.BF16)
  _same('convolution output', y1, CR.as_bf16(y64), tag)
  n, c, oh, ow = y1.shape
  npix = (n // groups) * oh * ow
  flat = y1.permute(0, 2, 3, 1).reshape(groups, npix, c).float()
  beta = (((torch.arange(c) * 5) % 17 - 8) / 8.0).to(dev)
  sc = R.Scene(R.Case(c // 8, npix, groups), True, flat, torch.zeros_like(flat), beta, None)
  r = R.restate(sc, relu)
  bq = beta.clone().requires_grad_(True)
  z = _hip_bn.batch_norm_relu(y1, bq, R.EPS, bool(relu), groups, True)
  mr = z.grad_fn.saved_tensors[2]
  _clean(y1, groups, 'behind the convolution')
  S, Q = flat.double().sum(1), (flat.double() ** 2).sum(1)
  assert float(Q.max()) < 2.0 ** 24
  key = lambda q: (tag, 'bf16', q)
  for g in range(groups):
    mean, rstd = _fp32_finish(S[g].tolist(), Q[g].tolist(), npix, R.EPS)
    _same('mean behind the convolution', mr[g, 0].cpu(), torch.from_numpy(mean), tag)
    _same('rstd behind the convolution', mr[g, 1].cpu(), torch.from_numpy(rstd), tag)
  _within('mean', mr[:, 0], r.mean, R.bar_mean(r), tag, key('mean'))
  _within('rstd', mr[:, 1], r.rstd, R.bar_rstd(r), tag, key('rstd'))
  got = z.detach().permute(0, 2, 3, 1).reshape(groups, npix, c)
  _within('y', got, r.y, R.bar_y(r, relu, True), tag, key('y'))


# ---- 4. the workspace across calls ------------------------------------------------------

def test_exact_cases_twice_in_a_shuffled_order_on_the_shared_workspace(dev):
  """Every exact case, both dtypes, the three routes, in one fixed shuffled
  order, twice, in one process: C, groups, dtype and route alternate on the
  one workspace of the stream.  Every result equals its
  first one and the reference."""
  jobs = [(case, bf16, (i + j + int(bf16)) % 2, route)
          for i, case in enumerate(R.exact_cases()) for bf16 in (False, True)
          for j, route in enumerate(('two-pass', 'one-pass', 'ctypes'))]
  random.Random(7).shuffle(jobs)
  assert any(a[0] != b[0] and a[1] != b[1] and a[3] != b[3] for a, b in zip(jobs, jobs[1:]))
  first = {}
  for rnd in range(2):
    for job in jobs:
      case, bf16, relu, route = job
      sc, ops, r = _ref(case, bf16, relu)
      what = 'round %d %s %s %s relu %d' % (rnd, route, _ids(case), _dt(bf16), relu)
      if route == 'ctypes':
        dx, dbeta = _bwd_ctypes(ops, _want_mr(r), case.groups, relu)
        out = (dx, dbeta)
      else:
        y, mr, leaves = _forward(ops, case.groups, relu, route == 'one-pass')
        dx, dbeta = torch.autograd.grad(y, leaves, ops[1])
        _clean(ops[0], case.groups, what)
        _check_statistics_and_y(what, r, bf16, relu, y, mr, 'repeat', True)
        out = (y.detach(), mr, dx, dbeta)
      _check_gradients(what, case, r, bf16, dx, dbeta, 'repeat')
      if rnd == 0:
        first[job] = out
      else:
        for a, b in zip(out, first[job]):
          assert torch.equal(a, b), what


# ---- 5. the shapes reach what they are for ----------------------------------------------

def _trips(npix, rows, wg):
  """Loop trips of every (workgroup, row): pixels p0, p0 + stride, ... < npix."""
  stride = wg * rows
  p0 = np.arange(stride)
  return set(np.maximum(0, -(-(npix - p0) // stride)).tolist())


def test_the_cases_cover_the_launch_shapes(built_lib):
  """From the library's own launch shapes (lsi_bn_launch_workgroups): lanes per
  pixel 1, 2, a middle value and 256; 1, 2 and 3 groups; fewer pixels than one
  step; a partial last step; fewer than 2, exactly 2, 4 and 8, 8 q + 1 and 8 q + 7
  trips -- the boundaries of the 8-, 4- and 2-way unrolled loops and their tails
  --; both branches of the small-tensor rule; the 2048-workgroup cap with a tail."""
  from lsi import _C
  lib = _C.lib()
  trips, seen = set(), set()
  for case in R.CASES:
    for bf16 in (False, True):
      C = R.channels(case, bf16)
      wg = lib.lsi_bn_launch_workgroups(case.npix, C, int(bf16), case.groups)
      assert 1 <= wg <= 2048, (case, bf16, wg)
      rows = 256 // case.lpp
      t = _trips(case.npix, rows, wg)
      trips |= t
      elements = case.npix * C * case.groups
      print('bn lattice %s %s: C %d, %d workgroups x %d rows, trips %s, %d elements'
            % (_ids(case), _dt(bf16), C, wg, rows, sorted(t), elements))
      seen.add('lpp %d' % case.lpp)
      seen.add('groups %d' % case.groups)
      if case.npix < rows:
        seen.add('fewer pixels than rows')
      if case.npix % rows:
        seen.add('partial last step')
      small = elements <= 1 << 21
      nstep = -(-case.npix // rows)
      if small and wg == -(-nstep // 2):
        seen.add('small tensor: two steps per workgroup')
      if small and wg * case.groups >= 512 and wg < -(-nstep // 2):
        seen.add('small tensor: stopped at 512 workgroups')
      if not small and wg == -(-nstep // 16) and elements <= (1 << 21) + 4 * C:
        seen.add('just over 2^21 elements: sixteen steps')
      if wg == 2048 and nstep > 16 * 2048 and case.npix % (2048 * rows):
        seen.add('the cap with a tail')
  assert {'lpp 1', 'lpp 2', 'lpp 16', 'lpp 256', 'groups 1', 'groups 2', 'groups 3',
          'fewer pixels than rows', 'partial last step', 'small tensor: two steps per workgroup',
          'small tensor: stopped at 512 workgroups', 'just over 2^21 elements: sixteen steps',
          'the cap with a tail'} <= seen, sorted(seen)
  assert lib.lsi_bn_launch_workgroups(2048, 1024, 0, 1) == 512      # 2^21 elements: small
  assert lib.lsi_bn_launch_workgroups(2052, 1024, 0, 1) == 129      # just over
  assert {0, 1, 2, 4, 8} <= trips, sorted(trips)
  assert any(t % 8 == 1 and t > 8 for t in trips) and any(t % 8 == 7 for t in trips), sorted(trips)
  assert any(t % 8 == 3 and t > 16 for t in trips)                  # the cap's 19 = 16 + 3


def test_report_worst_ratios(capsys):
  """Not a check: prints what the run measured (the bars are in the tests)."""
  _make_kept.cache_clear()
  _restate_kept.cache_clear()
  torch.cuda.empty_cache()
  with capsys.disabled():
    for key in sorted(WORST):
      print('\nbn lattice: worst ratio %s: %.3f' % (' | '.join(key), WORST[key]), end='')
    for key in sorted(COUNTS):
      print('\nbn lattice: %s comparisons %s: %d' % (key[0], key[1], COUNTS[key]), end='')
    print()
