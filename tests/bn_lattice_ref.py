"""Fused batch norm + beta + ReLU and its gradient restated in fp64 (torch, any
device; from the formulas, no autograd), and the lattice activations on which
everything csrc/lsi_bn.hip writes is determined to the last bit.

TEST INFRASTRUCTURE ONLY.  tests/test_bn_lattice_cpu.py holds this file to
fp64 autograd of torch.nn.functional.batch_norm + relu and proves what the
exact set claims; tests/test_bn_lattice_gpu.py holds the HIP kernels to this
file.

The lattice.  A case is (lpp, npix, groups): C = lpp * 4 channels in fp32,
lpp * 8 in bf16 (lpp = the kernels' lanes per pixel), npix pixels per group, a
multiple of 4.  Channel c of group g holds x = m + d with
  m = m[g, c]  an integer, |m| <= m_max(npix) <= 40, different in neighbouring
               channels and in the same channel of neighbouring groups (81
               integers cannot all differ over 2048 channels),
  d            one of +-0.5, +-a, each at exactly npix / 4 pixels, placed by a
               seeded shuffle,
  a = a[g, c]  one of 0.5, 2.5, 5.5, rotating over channels and groups.
The mean is m, the biased variance (0.25 + a^2) / 2 = 0.25, 3.25 or 15.25,
and with eps = 0.75 rstd is exactly 1, 0.5 or 0.25.  Every value is a bf16.
  dy           integers in [-8, 8].
  beta[c]      +-(0.5 a' rstd'), a' and rstd' those of the channel in its
               OWNER group c % groups: there z = xhat + beta is exactly 0 at a
               quarter of the pixels (half where a = 0.5), and the other
               values of z are +-0.25, +-0.5, ... away from it.  (A beta
               that is a multiple of 0.25 cannot do that where rstd = 0.25 --
               xhat is then +-0.125 or +-1.375 --, so beta is a multiple of
               0.125; in the other groups |z| >= 0.125 everywhere.)
  bf16 only    channels c % 4 == 1 take beta = +-(1.5 + (2 i + 1) 2^-8) instead:
               z of the pixels that land in +-[1, 2) is a bf16 tie, to the even
               neighbour below for even i, above for odd i.

Why the sums are exact.  The statistics pass adds x - k and (x - k)^2 with k
one of the channel's own values (stat_shift: a median of three of them):
multiples of 0.5 and 0.25, the sums of their absolute values below 2^22, so
every partial sum in any order is a float32; the double finish is then exact
as well.  The one-pass route adds x and x^2: m_max(npix) keeps npix (|m| +
5.5)^2 below 2^22.  The backward adds dz (integers) and dz * xhat (multiples of
0.125).  assert_sums_fit() checks all of it per case, with the worst shift.

The exact set.  The two-pass forward (mean, rstd, y) at every npix; the one-pass
forward and the backward where npix is a power of two, because both multiply
their sums by (float)(1 / npix).  There every intermediate of rstd * (dz - c1 -
xhat * c2) is a float32 under either association (assert_backward_is_fp32).
Elsewhere the sums are still exact and the bars below apply.
"""
import collections
import functools
import math

import torch

EPS = 0.75
A_VALUES = (0.5, 2.5, 5.5)
U = 2.0 ** -24          # half an ulp of fp32, relative
K_BWD = 4.0             # the backward's bar, in units of U * A (see bar_dx)

# Worst |dx32 - dx64| / (U A) of the same formula in fp32 torch on the CPU over
# the bounded cases: measured and pinned by tests/test_bn_lattice_cpu.py (it
# fails above the pin and below half of it).  K_BWD must not exceed 4 x this.
REF_RATIO = 2.4

Case = collections.namedtuple('Case', 'lpp npix groups')

# What each case is for (the launch shapes are asserted from the library's own
# answers by test_bn_lattice_gpu.py::test_the_cases_cover_the_launch_shapes).
# rows = 256 / lpp pixels per workgroup step.
CASES = (
    Case(1, 4, 1),         # one lane per pixel; fewer pixels than rows
    Case(2, 64, 2),        # two lanes per pixel; half a step, two groups
    Case(16, 64, 3),       # exactly two steps per workgroup, three groups
    Case(16, 260, 3),      # npix no multiple of rows = 16: a partial last step
    Case(256, 2048, 1),    # fp32: 2^21 elements, the small-tensor rule's last; 4 steps
    Case(256, 2052, 1),    # just over: 16 and 15 (8 + 7) steps
    Case(1, 2048, 260),    # many groups put a small map on the 16-step rule: 8 steps
    Case(1, 4100, 260),    # ... 9 (8 + 1) and 8 steps, the last one partial
    Case(256, 38916, 1),   # the 2048-workgroup cap: 20 and 19 steps
)
BIG = 1 << 23   # elements from which a scene is built on the device


def channels(case, bf16):
  return case.lpp * (8 if bf16 else 4)


def pow2(n):
  return n & (n - 1) == 0


def exact(case):
  """One-pass forward and backward are determined bit for bit."""
  return pow2(case.npix)


def exact_cases():
  return tuple(c for c in CASES if exact(c))


def bounded_cases():
  return tuple(c for c in CASES if not exact(c))


def m_max(npix):
  """The largest |m| at which the plain sum of x^2 over a group stays below
  2^22 quarters' worth: npix (|m| + 5.5)^2 < 2^22."""
  return max(2, min(40, int(math.floor(math.sqrt(2.0 ** 22 / npix) - 5.5))))


Constants = collections.namedtuple('Constants', 'm a var rstd beta tie')


def constants(case, bf16):
  """m, a, var, rstd [groups, C], beta [C] (fp64), tie [C] (bool)."""
  c = torch.arange(channels(case, bf16))
  g = torch.arange(case.groups)[:, None]
  mm = m_max(case.npix)
  m = ((7 * c + 13 * g + 3) % (2 * mm + 1) - mm).double()
  a = torch.tensor(A_VALUES, dtype=torch.float64)[(c + g) % 3]
  var = (0.25 + a * a) / 2
  rstd = 1.0 / torch.sqrt(var + EPS)
  own = c % case.groups
  sign = 1.0 - 2.0 * ((c // 3) % 2).double()
  beta = sign * 0.5 * rstd[own, c]
  tie = (c % 4 == 1) if bf16 else torch.zeros_like(c, dtype=torch.bool)
  i = (c // 4) % 4
  tsign = 1.0 - 2.0 * (i >= 2).double()
  beta = torch.where(tie, tsign * (1.5 + (2 * i + 1).double() * 2.0 ** -8), beta)
  # neighbouring channels and neighbouring groups differ
  assert len(c) < 2 or bool((m[:, 1:] != m[:, :-1]).all())
  assert case.groups < 2 or bool((m[1:] != m[:-1]).all() and (a[1:] != a[:-1]).all())
  assert bool(((rstd == 1) | (rstd == 0.5) | (rstd == 0.25)).all())
  return Constants(m, a, var, rstd, beta, tie)


def assert_sums_fit(case, bf16):
  """Every sum the kernels form stays inside fp32's exact range, whatever the
  order and -- for the shifted sums -- whichever of the channel's values
  stat_shift picks.  Analytic: each of the four values of d is there npix / 4
  times.  Returns the largest sum in units of its lattice step (< 2^24)."""
  k = constants(case, bf16)
  n = case.npix
  assert n % 4 == 0
  d = torch.stack([0 * k.a + 0.5, 0 * k.a - 0.5, k.a, -k.a])          # [4, G, C]
  worst = 0.0
  for shift in d:                                                     # x - k = d - shift
    s = (d - shift).abs().sum(0) * (n / 4)       # multiples of 0.5
    q = ((d - shift) ** 2).sum(0) * (n / 4)      # multiples of 0.25
    worst = max(worst, float(s.max()) / 0.5, float(q.max()) / 0.25)
  x = k.m + d
  worst = max(worst, float(x.abs().sum(0).max()) * (n / 4) / 0.5,      # one-pass: x, x^2
              float((x * x).sum(0).max()) * (n / 4) / 0.25)
  xhat = (d * k.rstd).abs().max()
  worst = max(worst, 8.0 * n * case.groups,                            # dz; dbeta over groups
              8.0 * n * float(xhat) / 0.125)                           # dz * xhat
  assert worst < 2.0 ** 24, (case, bf16, worst)
  return worst


Scene = collections.namedtuple('Scene', 'case bf16 x dy beta k')


@functools.lru_cache(maxsize=None)
def scene(case, bf16, device='cpu'):
  """x, dy [groups, npix, C] fp32 (every value a bf16), beta [C] fp32, on
  `device`; the same for the same arguments."""
  assert_sums_fit(case, bf16)
  k = constants(case, bf16)
  G, n, C = case.groups, case.npix, channels(case, bf16)
  gen = torch.Generator(device=device).manual_seed(
      1000003 * case.lpp + 101 * case.npix + 7 * case.groups + int(bf16))
  rank = torch.rand((G, C, n), generator=gen, device=device).argsort(dim=-1)
  vals = torch.stack([0 * k.a + 0.5, 0 * k.a - 0.5, k.a, -k.a], -1).to(device)   # [G, C, 4]
  d = torch.gather(vals, 2, rank % 4)
  del rank
  x = (d + k.m.to(device)[:, :, None]).permute(0, 2, 1).contiguous().float()
  del d
  dy = torch.randint(-8, 9, (G, n, C), generator=gen, device=device).float()
  assert bool((x.bfloat16().float() == x).all())
  return Scene(case, bf16, x, dy, k.beta.float().to(device), k)


Result = collections.namedtuple(
    'Result', 'mean rstd xhat z y dz c1 c2 dx A dbeta')


def restate(sc, relu, drop_pixel=False, swap_groups=False, mask_ge=False, eps=EPS):
  """The whole op in fp64: mean, rstd, c1, c2 [groups, C]; xhat, z, y, dz, dx, A
  [groups, npix, C]; dbeta [C].  relu'(0) = 0: dz = dy where z > 0.
  A = |rstd| (|dz| + |c1| + |xhat| |c2|), the yardstick of dx's rounding.
  The three switches break it the way a kernel could (the CPU tests show that
  the scenes notice): the group's last pixel missing from every sum, the
  constants of the groups rotated by one, z >= 0 as the backward's mask."""
  x, dy = sc.x.double(), sc.dy.double()
  n = sc.case.npix
  beta = sc.beta.double()
  part = (lambda t: t[:, :n - 1]) if drop_pixel else (lambda t: t)
  mean = part(x).sum(1) / n
  dev2 = part(x - mean[:, None]) ** 2
  var = dev2.sum(1) / n
  del dev2
  rstd = 1.0 / torch.sqrt(var + eps)
  if swap_groups:
    mean, rstd = mean.roll(1, 0), rstd.roll(1, 0)
  xhat = (x - mean[:, None]) * rstd[:, None]
  z = xhat + beta
  if relu:
    y = torch.where(z > 0, z, torch.zeros_like(z))
    dz = dy * ((z >= 0) if mask_ge else (z > 0))
  else:
    y, dz = z, dy
  c1 = part(dz).sum(1) / n
  c2 = part(dz * xhat).sum(1) / n
  dx = rstd[:, None] * (dz - c1[:, None] - xhat * c2[:, None])
  A = rstd[:, None] * (dz.abs() + c1.abs()[:, None] + xhat.abs() * c2.abs()[:, None])
  return Result(mean, rstd, xhat, z, y, dz, c1, c2, dx, A, dz.sum((0, 1)))


def is_fp32(t):
  return bool((t.float().double() == t).all())


def assert_backward_is_fp32(r):
  """On the exact set every intermediate of rstd * (dz - c1 - xhat * c2) is a
  float32, whichever way the source associates it: the expectation does not
  depend on how the kernel is written."""
  e = lambda t: t[:, None]
  p = r.xhat * e(r.c2)
  for name, t in (('c1', r.c1), ('c2', r.c2), ('xhat c2', p), ('dz - c1', r.dz - e(r.c1)),
                  ('c1 + xhat c2', e(r.c1) + p), ('dz - xhat c2', r.dz - p),
                  ('dz - c1 - xhat c2', r.dz - e(r.c1) - p), ('rstd dz', e(r.rstd) * r.dz),
                  ('rstd c1', r.rstd * r.c1), ('rstd xhat c2', e(r.rstd) * p), ('dx', r.dx)):
    assert is_fp32(t), name


def stored(t64, bf16):
  """What a kernel has to write for the exact value t64: fp32 (exact on the
  exact set), rounded once to nearest even for bf16."""
  t = t64.float()
  return t.bfloat16() if bf16 else t


def truncated(t64):
  """bf16 by dropping the low 16 bits: the broken store."""
  return (t64.float().view(torch.int32) & -65536).view(torch.float32).bfloat16()


def ties(z64):
  """(ties whose even neighbour is the one below, ... above) among fp32 z."""
  bits = z64.float().view(torch.int32)
  tie = (bits & 0xffff) == 0x8000
  up = (bits >> 16) & 1 == 1
  return int((tie & ~up).sum()), int((tie & up).sum())


# ---- the bars of the bounded set ------------------------------------------------------

def _bf16_store(bar, want, bf16):
  # the bf16 store rounds the fp32 result once more: half an ulp of an 8-bit
  # significand, at most 2^-8 of the value (reached just above a power of two)
  return bar + 2.0 ** -8 * (want.abs() + bar) if bf16 else bar


def bar_dx(r, bf16):
  """|dx - dx64| <= K U A.  c1 = fl(fl(1 / n) S1) carries two roundings, c2 the
  same two and xhat * c2 one more; each of the two subtractions rounds its own
  result, bounded by the sum of the absolute values it has seen; the last
  product by rstd, a power of two, is exact.  In units of U:
    dz - c1            2 |c1| + 1 (|dz| + |c1|)
    ... - xhat c2      3 |xhat c2| + 1 (|dz| + |c1| + |xhat c2|)
  together 2 |dz| + 4 |c1| + 4 |xhat c2| <= 4 (|dz| + |c1| + |xhat c2|)."""
  return _bf16_store(K_BWD * U * r.A, r.dx, bf16)


def bar_mean(r):
  """One pass: mean = fl(fl(1 / n) S), S exact: two roundings, each at most
  U / (1 + U) relative -- together less than 2 U = 2^-23."""
  return 2.0 ** -23 * r.mean.abs()


def bar_rstd(r, eps=EPS):
  """One pass.  With m, v the exact moments: E2 = fl(fl(1 / n) Q) is (m^2 + v)
  (1 + 2 U), mean^2 is m^2 (1 + 4 U), and var = fl(E2 - mean^2) -- one fma --
  adds v U: |var - v| <= U (6 m^2 + 3 v).  rstd = fl(1 / fl(sqrt(fl(var +
  eps)))): half of that relative to v + eps, plus U / 2 (the sum under the
  root), U (root) and U (quotient).  3 instead of 2.5 for the second order."""
  m, v = r.mean, 1.0 / (r.rstd * r.rstd) - eps
  return r.rstd * U * ((3 * m * m + 1.5 * v) / (v + eps) + 3.0)


def bar_y(r, relu, bf16, eps=EPS):
  """One pass.  t = fl(x - mean) is off d = x - m by |mean - m| + U |t|; z =
  fl(t rstd + beta), one fma, by rstd |mean - m| + |xhat| (rho + U) + U |z| with
  rho the relative error of rstd; 1 + 2^-10 for the products of two errors (rho
  is below 2^-11).  The ReLU does not stretch an error."""
  rho = bar_rstd(r, eps) / r.rstd
  assert float(rho.max()) < 2.0 ** -11
  e = lambda t: t[:, None]
  bar = (e(r.rstd * bar_mean(r)) + r.xhat.abs() * e(rho + U) + U * r.z.abs()) * (1 + 2.0 ** -10)
  return _bf16_store(bar, r.y if relu else r.z, bf16)
