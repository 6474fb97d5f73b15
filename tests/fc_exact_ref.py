"""Integer operands for the skinny fully-connected kernels (csrc/lsi_fc.hip),
their exact fp64 reference, and a restatement of the planner for coverage.

As in tests/conv_exact_ref.py: the kernels multiply bf16 values and accumulate
in fp32, so with small integer operands every partial sum is an integer below
2^24 and the result is fixed bit for bit in ANY summation order -- whichever
wave, chunk or fold order the kernels use.  One dropped, doubled or misplaced
term is a failed equality.

  narrow  values in +-{1, 2}, operand density min(1, sqrt(32 / R)) for a
          contraction of length R (K for x and the weight, N for gy): every Z
          and dX is an integer of magnitude <= 256, exactly a bf16.
  wide    values in +-{1, 2, 3}, dense: results below 2^24, rounded once to
          bf16 (nearest even, ties included) where the kernel stores bf16.

A case is (M, K, N, groups, layout).  The layout says where the (N, K) weight
lives in memory -- the kernels read the parameter in place through
    w[tap_off[n / (N / taps)] + (n % (N / taps)) * w_sn + k * w_sk]
-- and thereby which code path runs (LAYOUTS).  Storage elements that no (n, k)
addresses hold integers of their own: a kernel that reads one of them does not
go unseen, and in a weight gradient they must stay exactly 0.

No GPU is needed for anything here; given a device, everything runs there.
"""
import collections
import math

import torch

from conv_exact_ref import BF16_EXACT, EXACT, REGIMES, as_bf16, ints  # noqa: F401

Case = collections.namedtuple('Case', 'm k n groups layout')

# layout: what it reaches
LAYOUTS = {
    'linear': 'nn.Linear weight (N, K), contiguous: 16-byte accesses along K',
    'linear_t': '(N, K) view of a contiguous (K, N) buffer: unit stride along N -- '
                'fc_dw_kernel<false> with one tap, vector dX, scalar forward',
    'linear_off4': 'contiguous (N, K) starting 4 bytes past a 16-byte boundary: '
                   'vec = 0 on a unit stride',
    'convt_cl': '(cin, cout, 4, 4) weight, channels-last: four taps, unit stride along N',
    'convt_contig': '(cin, cout, 4, 4) weight, contiguous: four taps, no unit stride',
    'taps2_odd': '2-D buffer, two taps at odd offsets, unit stride along N',
    'taps3': '2-D buffer, three taps, two offsets not multiples of 4, unit stride along K',
}


def lin(m, k, n, layout='linear', groups=1):
  return Case(m, k, n, groups, layout)


def convt(m, cin, cout, layout):
  return Case(m, cin, 4 * cout, 1, layout)


# ---- the cases: one sentence each on the structure it reaches ----------------------
# (steps = 32-deep reduction steps; tile = 16 output columns; MT = row tiles of 16)
CASES = [
    # one partial step with the lanes q >= 1 masked; one half column tile; one row
    lin(1, 8, 8),
    # the same through the scalar paths, and a weight gradient of two live lanes
    lin(1, 8, 8, 'linear_t'),
    lin(1, 8, 8, 'linear_off4'),
    # second step with 8 valid elements; second tile half full; 10 live lanes in fc_dw_kernel
    lin(3, 40, 24),
    # ... unit stride along N: 6 live lanes, the forward reads 8 strided dwords
    lin(3, 40, 24, 'linear_t'),
    # ... a unit stride that is not on a 16-byte boundary: scalar forward and dX
    lin(3, 40, 24, 'linear_off4'),
    # 17 forward steps: wave 0 makes a second trip of its unrolled loop, two chunks of
    # 9 + 8; fc_dw_kernel's third lane block has 2 lanes; fifth fold block partial; MT = 1 full
    lin(16, 520, 264),
    # ... with N the fast dimension: fc_dw_kernel<false>, F = 264, second lane block partial
    lin(16, 520, 264, 'linear_t'),
    # MT = 2 with 15 padding rows; dX reduction of 17 steps, split in two; F = 264
    lin(17, 264, 520),
    lin(17, 264, 520, 'linear_off4'),
    # MT = 2 nearly full, N = 64 tiles + 8 columns, dX over 33 steps in four chunks
    lin(31, 72, 1032),
    # MT = 2 full; K = 32 * 32 + 8: 33 steps, four chunks of 9, 9, 9, 6
    lin(32, 1032, 1000),
    lin(32, 1032, 1000, 'linear_t'),
    # odd M at a network size
    lin(5, 1000, 1000),
    # the transposed convolution on a 1 x 1 map, both layouts: one tile per tap and one step
    convt(2, 8, 8, 'convt_cl'),
    convt(2, 8, 8, 'convt_contig'),
    # ... a tap boundary inside a column tile (N / taps = 24), a partial second step
    convt(8, 40, 24, 'convt_cl'),
    convt(8, 40, 24, 'convt_contig'),
    # ... the network's own upcnv8
    convt(8, 1000, 512, 'convt_cl'),
    convt(8, 1000, 512, 'convt_contig'),
    # two taps of 8 columns at odd offsets: one tile holds both taps, every access scalar
    lin(4, 40, 16, 'taps2_odd'),
    # three taps of 24 columns: tap boundaries inside the second and fifth tile
    lin(7, 72, 72, 'taps3'),
]
# wide regime only: the largest network layer, the one full-size anchor
ANCHOR = lin(8, 6144, 2000)


def regimes(case):
  return ('wide',) if case == ANCHOR else REGIMES


def all_cases():
  return CASES + [ANCHOR]


def ident(case):
  return '-'.join(str(v) for v in case)


# ---- geometry ----------------------------------------------------------------------

def storage_shape(case):
  """Shape of the contiguous fp32 buffer behind the weight."""
  lay = case.layout
  if lay in ('linear', 'linear_off4'):
    return (case.n, case.k)
  if lay == 'linear_t':
    return (case.k, case.n)
  if lay == 'convt_cl':
    return (case.k, 4, 4, case.n // 4)       # (cin, ky, kx, cout)
  if lay == 'convt_contig':
    return (case.k, case.n // 4, 4, 4)
  if lay == 'taps2_odd':
    return (case.k, 2 * (case.n // 2) + 8)   # row k: 3 junk, tap 0, 2 junk, tap 1, 3 junk
  if lay == 'taps3':
    return (3 * (case.n // 3) + 3, case.k + 8)   # taps at rows 0, nt + 1, 2 nt + 2
  raise ValueError(lay)


def geometry(case):
  """(K, N, taps, w_sn, w_sk, tap_off) in elements from the weight's first one,
  as _hip_fc.linear_geometry / convt_geometry give it for the tensors of
  `parameter` (test_fc_exact_cpu.py checks that they agree)."""
  k, n, lay = case.k, case.n, case.layout
  if lay in ('linear', 'linear_off4'):
    return (k, n, 1, k, 1, (0,))
  if lay == 'linear_t':
    return (k, n, 1, 1, n, (0,))
  if lay == 'convt_cl':
    c = n // 4
    taps = tuple((4 * (oy + 1) + ox + 1) * c for oy in (0, 1) for ox in (0, 1))
    return (k, n, 4, 1, 16 * c, taps)
  if lay == 'convt_contig':
    c = n // 4
    return (k, n, 4, 16, 16 * c, (5, 6, 9, 10))
  if lay == 'taps2_odd':
    nt = n // 2
    return (k, n, 2, 1, 2 * nt + 8, (3, nt + 5))
  if lay == 'taps3':
    nt, row = n // 3, k + 8
    return (k, n, 3, row, 1, (1, (nt + 1) * row + 2, (2 * nt + 2) * row + 5))
  raise ValueError(lay)


def addressed(case):
  """int64 (N, K): the storage index of weight element (n, k)."""
  k, n, taps, sn, sk, off = geometry(case)
  nt = n // taps
  nn = torch.arange(n)
  base = torch.tensor(off)[nn // nt] + (nn % nt) * sn
  return base[:, None] + torch.arange(k)[None, :] * sk


def scatter(case, w_nk, fill=None):
  """The storage buffer (flat, storage_shape's numel) holding w_nk (N, K) where
  the geometry addresses it and `fill` (default zeros) elsewhere."""
  numel = math.prod(storage_shape(case))
  idx = addressed(case).to(w_nk.device)
  assert int(idx.max()) < numel and idx.unique().numel() == idx.numel(), case
  flat = (torch.zeros(numel, dtype=w_nk.dtype, device=w_nk.device) if fill is None
          else fill.to(w_nk.dtype).to(w_nk.device).clone())
  flat[idx.reshape(-1)] = w_nk.reshape(-1)
  return flat


def parameter(case, flat, device=None):
  """The weight tensor the binding is given: fp32, laid out as the case says, on
  `device`, holding the flat storage `flat` (see scatter)."""
  shape = storage_shape(case)
  flat = flat.float().to(device or flat.device)
  if case.layout == 'linear_off4':
    room = torch.zeros(flat.numel() + 8, dtype=torch.float32, device=flat.device)
    at = 1 + (-(room.data_ptr() // 4) % 4)       # 4 bytes past a 16-byte boundary
    w = room[at:at + flat.numel()].view(shape)
    w.copy_(flat.view(shape))
    assert w.data_ptr() % 16 == 4 and w.is_contiguous()
    return w
  buf = flat.clone().view(shape)
  if case.layout == 'linear_t':
    return buf.t()
  if case.layout == 'convt_cl':
    return buf.permute(0, 3, 1, 2)               # (cin, cout, 4, 4), channels-last
  return buf


def storage_of(case, t):
  """Flat view of the storage behind a tensor laid out like `parameter` (a weight
  gradient in the parameter's strides)."""
  shape = storage_shape(case)
  if case.layout == 'linear_t':
    t = t.t()
  elif case.layout == 'convt_cl':
    t = t.permute(0, 2, 3, 1)
  assert tuple(t.shape) == shape and t.is_contiguous(), (case, t.shape, t.stride())
  return t.reshape(-1)


def lib_geometry(case, w):
  """The geometry tuple as the binding derives it from the tensor (hand-written
  for the layouts it has no function for)."""
  from lsi.nnutils import _hip_fc
  if case.layout.startswith('linear'):
    return _hip_fc.linear_geometry(w)
  if case.layout.startswith('convt'):
    return _hip_fc.convt_geometry(w)
  return geometry(case)


def descriptor(case, flags=0, eps=1e-3):
  """The case's LsiFcDesc (include/lsi_hip.h) for the C ABI."""
  from lsi import _C
  k, n, taps, sn, sk, off = geometry(case)
  d = _C.LsiFcDesc()
  d.M, d.K, d.N, d.groups, d.taps, d.flags = case.m, k, n, case.groups, taps, flags
  d.w_sn, d.w_sk, d.eps = sn, sk, eps
  for i, o in enumerate(off):
    d.tap_off[i] = o
  return d


# ---- operands and reference ----------------------------------------------------------

def densities(case, regime):
  """(density of x and of the weight, density of gy, vmax)."""
  if regime == 'wide':
    return 1.0, 1.0, 3
  assert regime == 'narrow', regime
  return min(1.0, math.sqrt(32.0 / case.k)), min(1.0, math.sqrt(32.0 / case.n)), 2


def operands(case, regime, seed=0):
  """x (M, K), the weight (N, K), gy (M, N), junk (the storage's size: what the
  elements outside the geometry hold): fp32 on the CPU, integer-valued, the same
  for the same (case, regime, seed)."""
  s = sorted(LAYOUTS).index(case.layout)
  for v in case[:4]:
    s = (s * 131 + v) % 1000003
  g = torch.Generator().manual_seed(4 * s + 2 * (regime == 'wide') + 4000037 * seed)
  d, dg, vmax = densities(case, regime)
  x = ints((case.m, case.k), d, vmax, g)
  w = ints((case.n, case.k), d, vmax, g)
  gy = ints((case.m, case.n), dg, vmax, g)
  junk = ints((math.prod(storage_shape(case)),), d, vmax, g)
  return x, w, gy, junk


def guards(case, regime, z, dx=None, dw=None):
  """Conditions on the inputs (asserted, never loosened)."""
  for name, t in (('z', z), ('dx', dx), ('dw', dw)):
    if t is None:
      continue
    assert torch.equal(t, t.round()), (case, regime, name)
    m = float(t.abs().max())
    assert m < EXACT, (case, regime, name, m)
    # (the weight gradient is stored as fp32: it needs no more than 2^24)
    if regime == 'narrow' and name != 'dw':
      assert m <= BF16_EXACT, (case, regime, name, m)


def reference(case, x, w, gy=None, regime=None):
  """(Z, dX, dW) in fp64 from the integer operands: Z = X W^T, dX = gy W,
  dW = gy^T X (N, K).  Any float dtype, any device; regime: whose guards to
  assert (None: only the 2^24 ones)."""
  x64, w64 = x.double(), w.double()
  z = x64 @ w64.t()
  dx = dw = None
  if gy is not None:
    dx = gy.double() @ w64
    dw = gy.double().t() @ x64
  guards(case, regime, z, dx, dw)
  return z, dx, dw


# ---- the planner, restated (coverage only; checked against the library's
# lsi_fc_workspace_bytes in test_fc_exact_cpu.py) ------------------------------------
Plan = collections.namedtuple('Plan', 'steps chunks per lengths')
TARGET_GROUPS, WAVES = 512, 4


def split(r, c):
  """A reduction of length r for c output columns: 32-deep steps, the chunks the
  workgroups of one column tile take, the steps of each."""
  steps = (r + 31) // 32
  tiles = (c + 15) // 16
  want = min(-(-TARGET_GROUPS // tiles), max(steps // (2 * WAVES), 1))
  per = -(-steps // want)
  chunks = -(-steps // per)
  return Plan(steps, chunks, per, tuple(min(per, steps - i * per) for i in range(chunks)))


def plan(case):
  """fwd / dx: Plan of Z's reduction over K and of dX's over N; mt: 16-row tiles;
  dw_fast: the length of fc_dw_kernel's fast dimension (four elements a lane)."""
  _, _, _, sn, sk, _ = geometry(case)
  fast_n = sn == 1 and sk != 1
  return {'fwd': split(case.k, case.n), 'dx': split(case.n, case.k),
          'mt': 2 if case.m > 16 else 1, 'dw_fast': case.n if fast_n else case.k}


def align256(b):
  return (b + 255) // 256 * 256


def workspace_parts(case):
  """(forward bytes, dZ bytes, dX partial bytes) from the restatement."""
  p = plan(case)
  return (align256(p['fwd'].chunks * case.m * case.n * 4), align256(case.m * case.n * 2),
          align256(p['dx'].chunks * case.m * case.k * 4))


def workspace_bytes(case):
  f, dz, dx = workspace_parts(case)
  return max(f, dz + dx)


# ---- deliberately broken references (the sensitivity of the operands) ---------------
# Each returns (Z, dX) in fp64 with ONE of the errors these kernels could make,
# or None where the case cannot make it.  The narrow regime has to see every one
# (test_fc_exact_cpu.py): the operands are sparse, and an error that only ever
# meets zeros would go unseen.

def _products(x, w, gy):
  return x.double() @ w.double().t(), gy.double() @ w.double()


def broken_tail(case, x, w, gy, junk):
  """The last 8 reduction elements dropped: of K in Z, of N in dX."""
  z, _ = _products(x[:, :-8], w[:, :-8], gy)
  _, dx = _products(x, w[:-8], gy[:, :-8])
  return z, dx


def broken_chunk(case, x, w, gy, junk):
  """One chunk of the split skipped (the last; where the plan does not split,
  the last step -- one wave's share)."""
  out = []
  for which, r in (('fwd', case.k), ('dx', case.n)):
    p = plan(case)[which]
    gone = p.lengths[-1] if p.chunks > 1 else 1
    out.append(min(r, 32 * (p.steps - gone)))
  kz, nx = out
  z, _ = _products(x[:, :kz], w[:, :kz], gy)
  _, dx = _products(x, w[:nx], gy[:, :nx])
  return z, dx


def broken_rows(case, x, w, gy, junk):
  """The rows >= 16 (the second row tile) zeroed."""
  if case.m <= 16:
    return None
  z, dx = _products(x, w, gy)
  z[16:] = 0
  dx[16:] = 0
  return z, dx


def broken_tap(case, x, w, gy, junk):
  """The last tap's offset shifted by one element."""
  k, n, taps, sn, sk, off = geometry(case)
  flat = torch.cat([scatter(case, w, junk), junk[:1]])
  idx = addressed(case)
  idx[n - n // taps:] += 1
  return _products(x, flat[idx], gy)


def broken_half_tile(case, x, w, gy, junk):
  """The upper half of the last column tile left unwritten (the last 8 columns:
  of a half-full last tile, all it has)."""
  z, dx = _products(x, w, gy)
  z[:, -8:] = 0
  dx[:, -8:] = 0
  return z, dx


BROKEN = {'tail of 8 dropped': broken_tail, 'chunk skipped': broken_chunk,
          'rows 16.. zeroed': broken_rows, 'tap shifted': broken_tap,
          'half tile unwritten': broken_half_tile}


# ---- batch norm (section b of test_fc_exact_gpu.py) ----------------------------------
# (M, groups): 3 rows per group, one row per group, MT = 2, 32 groups
BN_ROWS = [(2, 2), (4, 1), (6, 2), (8, 2), (16, 2), (17, 1), (32, 1), (32, 4), (32, 32)]
BN_CASES = [lin(m, 264, 520, groups=g) for m, g in BN_ROWS] + [lin(8, 2048, 2000, groups=2)]
EPS = 1e-3
U32 = 2.0 ** -24
MARGIN = 4.0      # a ReLU is taken as decided where |v| > MARGIN * E32


def bn_operands(case, seed=0):
  """x (M, K) integers in +-{1, 2, 3} with X[:, :M] = I (dW[:, :M] is then dZ
  transposed, exactly), the weight (N, K) and gy (M, N) integers in +-{1, 2, 3},
  beta (N,) random: fp32 on the CPU."""
  g = torch.Generator().manual_seed(7919 * case.m + 104729 * case.groups + case.k +
                                    4000037 * seed)
  x = ints((case.m, case.k), 1.0, 3, g)
  x[:, :case.m] = torch.eye(case.m)
  w = ints((case.n, case.k), 1.0, 3, g)
  gy = ints((case.m, case.n), 1.0, 3, g)
  beta = 0.5 * torch.randn(case.n, generator=g)
  return x, w, gy, beta


def bn_reference(case, x, w, gy, beta, eps=EPS):
  """fp64 batch norm + ReLU, forward and backward, on the exact integer Z.

  Returns a dict of fp64 tensors: z, v (pre-ReLU), y, e32 (the forward bound),
  rstd, xhat, a (rstd max|z| of the group), g (masked gy), s1, s2, dz, dbeta --
  (M, N) each (group values broadcast over the group's rows), dbeta (N,) -- and
  `decided` (groups, N) bool: every row of the pair has |v| > MARGIN e32, so the
  ReLU mask of an fp32 evaluation within e32 is the reference's."""
  m, n, grp = case.m, case.n, case.groups
  r = m // grp
  z = x.double() @ w.double().t()
  assert float(z.abs().max()) * r < EXACT      # (the sums behind the means are exact)
  eps = float(torch.tensor(eps, dtype=torch.float32))   # the kernel's eps is an fp32
  zc = z.view(grp, r, n)
  mean = zc.mean(dim=1, keepdim=True)
  var = (zc - mean).square().mean(dim=1, keepdim=True)
  rstd = torch.rsqrt(var + eps)
  xhat = (zc - mean) * rstd
  b = beta.double()
  v = xhat + b
  a = zc.abs().amax(dim=1, keepdim=True) * rstd
  e32 = 2 * U32 * (r + 8) * (a + xhat.abs() + v.abs())
  if r == 1:
    # mean = z * 1.0f = z, d = z - z = 0: v is beta itself in any precision
    e32 = torch.zeros_like(e32)
  decided = (v.abs() > MARGIN * e32).all(dim=1)                  # (groups, N)
  g = gy.double().view(grp, r, n) * (v > 0)
  s1 = g.mean(dim=1, keepdim=True)
  s2 = (g * xhat).mean(dim=1, keepdim=True)
  dz = rstd * ((g - s1) - xhat * s2)
  full = lambda t: t.expand(grp, r, n).reshape(m, n)
  return {'z': z, 'v': full(v), 'y': full(v).clamp_min(0), 'e32': full(e32),
          'rstd': full(rstd), 'xhat': full(xhat), 'a': full(a), 'g': full(g),
          's1': full(s1), 's2': full(s2), 'dz': full(dz), 'dbeta': g.sum(dim=(0, 1)),
          'decided': decided, 'rows': r}


def dz_bound(ref):
  """Per-element bound E on |fp32 value the kernel rounds to dZ - fp64 dZ|; derived
  in the docstring of test_fc_exact_gpu.py::test_batch_norm_against_fp64."""
  r = ref['rows']
  rstd, xh, a, g, s1, s2, dz = (ref[k] for k in ('rstd', 'xhat', 'a', 'g', 's1', 's2', 'dz'))
  if r == 1:
    # s1 = g * 1.0f = g, x-hat = 0, s2 = 0: rstd * ((g - g) - 0 * 0) = 0 in any precision
    return torch.zeros_like(dz)
  rho = 2 * a + r / 2.0 + 9                       # rstd's and x-hat's relative error / u
  assert float(rho.max()) * U32 < 2.0 ** -11      # the quadratic terms: below 2^-10 of E
  ex = 2 * a + xh.abs() * rho                     # |d x-hat| / u
  grp = ref['decided'].shape[0]
  m, n = dz.shape
  per_group = lambda t: t.view(grp, r, n).mean(dim=1, keepdim=True).expand(grp, r, n).reshape(m, n)
  es2 = per_group(g.abs() * (ex + (r + 2) * xh.abs()))           # |d s2| / u
  c = (g - s1) - xh * s2
  e = rstd * (2 * s1.abs() + (g - s1).abs() + ex * s2.abs() + xh.abs() * es2 +
              (xh * s2).abs() + c.abs()) + dz.abs() * (rho + 1)
  return U32 * e * (1 + 2.0 ** -10)
