"""Integer operands for the bf16 (and fp32) convolution kernels, and their exact
reference.

The kernels multiply bf16 values and accumulate in fp32.  With small integer
operands every product and every partial sum is an integer below 2^24, hence
exact in fp32 in ANY summation order: the result is determined bit for bit and a
test needs no tolerance.  One wrong, missing or doubled term is a failed
equality.

Two regimes per case:

  narrow  values in +-{1, 2}, sparse: operand density min(1, sqrt(32 / K)), K the
          contraction length, so that about 32 products per output are nonzero
          and every output and data gradient is an integer of magnitude <= 256
          -- exactly a bf16: the kernel's final rounding cannot matter.  The
          sharp regime: a single unit of error shows.
  wide    values in +-{1, 2, 3}, dense.  Results reach the hundreds to thousands;
          the fp32 sum is still exact and the bf16 store rounds it once.  Expected
          is the fp64 result rounded fp64 -> fp32 (exact) -> bf16 (nearest even):
          this regime pins the rounding mode, ties such as 257 included.

The guards below are conditions on the test's own inputs, not tolerances: a case
that violates one is a bug in the case.  No GPU is needed for anything here;
given tensors on a device, `reference` runs there in fp64.
"""
import collections
import math

import torch
import torch.nn.functional as F

# kind 'conv': slim.conv2d, TF SAME padding, weight cout x cin x kh x kw;
# kind 'convt': slim.conv2d_transpose k x k stride 2 = torch
# conv_transpose2d(stride 2, padding 1) cut to 2h x 2w (k = 4: nothing is cut),
# weight cin x cout x k x k
Case = collections.namedtuple('Case', 'kind n cin cout h w kh kw stride')

REGIMES = ('narrow', 'wide')
EXACT = 1 << 24      # integers below are exact in fp32
BF16_EXACT = 256     # integers up to here are exact in bf16


def conv(n, cin, cout, h, w, k, stride):
  return Case('conv', n, cin, cout, h, w, k, k, stride)


def conv_hw(n, cin, cout, h, w, kh, kw, stride):
  return Case('conv', n, cin, cout, h, w, kh, kw, stride)


def convt(n, cin, cout, h, w, k=4):
  return Case('convt', n, cin, cout, h, w, k, k, 2)


def same_pads(size, k, s):
  """TF `SAME`: (before, after, out) -- the odd pixel goes after."""
  out = -(-size // s)
  total = max((out - 1) * s + k - size, 0)
  return total // 2, total - total // 2, out


def out_size(case):
  if case.kind == 'convt':
    return 2 * case.h, 2 * case.w
  return same_pads(case.h, case.kh, case.stride)[2], same_pads(case.w, case.kw, case.stride)[2]


def contraction(case):
  """Products per output value (a transposed layer's output pixel meets the taps
  of one parity class: (k / 2)^2 of them, rounded up)."""
  if case.kind == 'convt':
    return case.cin * ((case.kh + 1) // 2) * ((case.kw + 1) // 2)
  return case.cin * case.kh * case.kw


def ints(shape, density, vmax, generator):
  """fp32 tensor, nonzero with probability `density`, the nonzero values uniform
  in +-{1 .. vmax}."""
  mag = torch.randint(1, vmax + 1, shape, generator=generator)
  sign = torch.randint(0, 2, shape, generator=generator) * 2 - 1
  keep = torch.rand(shape, generator=generator) < density
  return (mag * sign * keep).to(torch.float32)


def densities(case, regime):
  """(operand density, incoming-gradient density, vmax)."""
  if regime == 'wide':
    return 1.0, 1.0, 3
  assert regime == 'narrow', regime
  d = min(1.0, math.sqrt(32.0 / contraction(case)))
  dg = min(1.0, math.sqrt(32.0 / (case.cout * case.kh * case.kw)))
  return d, dg, 2


def operands(case, regime, seed=0):
  """x (n x cin x h x w), the weight, gy (n x cout x oh x ow): fp32 on the CPU,
  integer-valued, the same for the same (case, regime, seed)."""
  s = int(case.kind == 'convt')
  for v in case[1:]:
    s = (s * 131 + v) % 1000003
  g = torch.Generator().manual_seed(4 * s + 2 * (regime == 'wide') + 4000037 * seed)
  d, dg, vmax = densities(case, regime)
  oh, ow = out_size(case)
  x = ints((case.n, case.cin, case.h, case.w), d, vmax, g)
  wshape = (case.cin, case.cout) if case.kind == 'convt' else (case.cout, case.cin)
  w = ints(wshape + (case.kh, case.kw), d, vmax, g)
  gy = ints((case.n, case.cout, oh, ow), dg, vmax, g)
  return x, w, gy


def forward(case, x, w):
  """The layer in the dtype of its operands (fp64 for the reference)."""
  if case.kind == 'convt':
    y = F.conv_transpose2d(x, w, None, 2, 1)
    return y[:, :, :2 * case.h, :2 * case.w]
  pt, pb, _ = same_pads(case.h, case.kh, case.stride)
  pl, pr, _ = same_pads(case.w, case.kw, case.stride)
  return F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, None, case.stride)


def guards(case, regime, y, gx=None, gw=None, groups=()):
  """Conditions on the inputs (asserted, never loosened): see the module text.
  groups: the sub-batch group counts whose epilogue statistics the caller checks
  -- sum y^2 per channel and group must be exact in fp32, too."""
  for name, t in (('y', y), ('gx', gx), ('gw', gw)):
    if t is None:
      continue
    m = float(t.abs().max())
    assert m < EXACT, (case, regime, name, m)
    # (the weight gradient is stored as fp32: it needs no more than 2^24)
    if regime == 'narrow' and name != 'gw':
      assert m <= BF16_EXACT, (case, regime, name, m)
  for grp in groups:
    # (the epilogue sums the values it stores, i.e. after the bf16 rounding.  The
    # sum behind the mean is exact in both regimes; the sum of squares in the
    # narrow one -- the wide regime's y^2 reach 10^6 and their sum rounds, which
    # only rstd sees, inside its tolerance)
    assert case.n % grp == 0, (case, grp)
    yr = as_bf16(y).double().view(grp, case.n // grp, y.shape[1], -1)
    s = yr.abs().sum(dim=(1, 3))
    assert float(s.max()) < EXACT, (case, regime, 'sum |y|', grp, float(s.max()))
    if regime == 'narrow':
      q = yr.square().sum(dim=(1, 3))
      assert float(q.max()) < EXACT, (case, regime, 'sum y^2', grp, float(q.max()))


def reference(case, x, w, gy=None, regime=None, want_gw=True, groups=()):
  """(y, gx, gw) of the layer in fp64 from the integer operands (any float
  dtype, any device; gx / gw None without gy / want_gw).  regime: whose guards
  to assert (None: only the 2^24 ones)."""
  x64 = x.detach().double().contiguous().requires_grad_(True)
  w64 = w.detach().double().contiguous().requires_grad_(True)
  y = forward(case, x64, w64)
  gx = gw = None
  if gy is not None:
    ins = (x64, w64) if want_gw else (x64,)
    gs = torch.autograd.grad(y, ins, gy.detach().double())
    gx = gs[0]
    gw = gs[1] if want_gw else None
  y = y.detach()
  guards(case, regime, y, gx, gw, groups)
  return y, gx, gw


def as_bf16(t64):
  """What a kernel that stores bf16 has to write: the exact value rounded once,
  to nearest even (fp64 -> fp32 is exact below 2^24)."""
  return t64.float().to(torch.bfloat16)


# ---- deliberately broken references (the sensitivity of the operands) ---------------
# Each returns the fp64 forward with ONE of the errors these kernels make.  The
# narrow regime has to see every one of them in every case
# (test_conv_exact_cpu.py): the operands are sparse, and an error that only ever
# meets zeros would go unseen.

def _one_tap(w, ky, kx):
  z = torch.zeros_like(w)
  z[:, :, ky, kx] = w[:, :, ky, kx]
  return z


def broken_dropped_term(case, x, w, y):
  """One product missing from the output pixel in the image's top-left corner."""
  x, w = x.double(), w.double()
  if case.kind == 'convt':
    # out (0, 0) = sum_ci x[ci, 0, 0] w[ci, co, 1, 1]  (2 iy - 1 + ky = 0)
    prod = x[0, :, 0, 0][:, None] * w[:, :, 1, 1]            # cin x cout
    nz = prod.nonzero()
    assert len(nz), (case, 'no nonzero product at the corner')
    ci, co = nz[0].tolist()
    term = prod[ci, co]
  else:
    pt, pb, _ = same_pads(case.h, case.kh, case.stride)
    pl, pr, _ = same_pads(case.w, case.kw, case.stride)
    patch = F.pad(x[:1], (pl, pr, pt, pb))[0, :, :case.kh, :case.kw]
    prod = w * patch[None]                                   # cout x cin x kh x kw
    nz = prod.nonzero()
    assert len(nz), (case, 'no nonzero product at the corner')
    co = int(nz[0][0])
    term = prod[tuple(nz[0].tolist())]
  out = y.clone()
  out[0, co, 0, 0] -= term
  return out


def broken_shifted_tap(case, x, w, y):
  """One tap reads its neighbour on the left for the last output column."""
  x, w = x.double(), w.double()
  if case.kind == 'convt':
    ky, kx = 1, 2          # (the tap that meets the input's last column there)
  else:
    ky, kx = case.kh // 2, case.kw // 2
  wt = _one_tap(w, ky, kx)
  right = forward(case, x, wt)
  shifted = forward(case, F.pad(x, (1, 0))[..., :-1], wt)
  out = y.clone()
  out[..., -1] += shifted[..., -1] - right[..., -1]
  return out


def broken_skipped_chunk(case, x, w, y):
  """The last chunk of 32 input channels never added."""
  x, w = x.double(), w.double()
  c0 = case.cin - min(32, case.cin)
  wc = w[c0:] if case.kind == 'convt' else w[:, c0:]
  return y - forward(case, x[:, c0:], wc)


BROKEN = {'dropped term': broken_dropped_term, 'shifted tap': broken_shifted_tap,
          'skipped chunk': broken_skipped_chunk}


# ---- the cases (tests/test_conv_exact_gpu.py; the guards: test_conv_exact_cpu.py) ---
# a. implicit GEMM: n, cin, cout, h, w, k, stride
IGEMM = [
    conv(2, 32, 32, 5, 17, 3, 1),      # fewer rows than two tiles, one column past a tile, BN = 32
    conv(1, 64, 64, 3, 7, 3, 1),       # smaller than one tile both ways
    conv(2, 96, 64, 9, 33, 3, 1),      # three chunks
    conv(1, 32, 96, 6, 16, 3, 1),      # Cout = 96 (BN = 32), width exactly one tile
    conv(2, 32, 64, 12, 20, 5, 2),     # stride 2, even sizes: pads 1 / 2
    conv(2, 32, 64, 11, 19, 5, 2),     # ... odd sizes: 2 / 2
    conv(1, 64, 128, 8, 18, 3, 2),     # 3 x 3 stride 2: pads 0 / 1
    conv(1, 64, 128, 7, 17, 3, 2),     # ... 1 / 1
    conv(1, 32, 32, 9, 21, 7, 1),      # 49 taps
    conv(2, 64, 64, 10, 19, 5, 1),     # 25 taps
    conv(2, 160, 128, 5, 7, 5, 1),     # five chunks: splits unevenly
    conv(2, 1024, 512, 4, 12, 3, 1),   # the deepest contraction
]
IGEMM_T = [convt(2, 64, 32, 3, 5), convt(1, 128, 64, 9, 17), convt(2, 512, 512, 2, 6)]
# b. the split over the input channels
SPLIT = [IGEMM[10], IGEMM[11], conv(8, 512, 512, 4, 12, 3, 1)]
# c. two-tensor variants: (c1, the case over c1 + c2 channels).  The data
#    gradient into two tensors wants c1 a multiple of its channel block (64 when
#    c1 + c2 is): it refuses the second case, which therefore checks forward and
#    weight gradient only, and the third adds that shape with c1 = 64
CAT = [(64, conv(2, 96, 64, 7, 21, 3, 1)), (32, conv(1, 128, 32, 5, 9, 5, 1)),
       (64, conv(1, 128, 32, 5, 9, 5, 1))]
# d. epilogue statistics: (case, groups) -- one is split over the input channels
#    (the fold kernel leaves the sums), one is transposed
STATS = [(IGEMM[0], 1), (IGEMM[0], 2), (IGEMM[5], 1), (IGEMM[5], 2), (IGEMM[11], 1),
         (IGEMM[11], 2), (IGEMM_T[0], 1), (IGEMM_T[0], 2)]
# e. the 32-channel 3 x 3 kernels: (n, h, w).  The forward / data-gradient kernel
#    takes widths that are multiples of 16 only: at the widths it refuses, their
#    neighbours 80 and 144; the weight-gradient kernel takes them all
C32_FWD = [(1, 3, 16), (2, 33, 80), (1, 5, 144)]
C32_REFUSED = [(2, 33, 70), (1, 5, 129)]
C32_WGRAD = [(1, 3, 16, 32, 32), (2, 33, 70, 32, 32), (1, 5, 129, 32, 32), (1, 5, 7, 96, 64),
             (2, 33, 70, 96, 64), (1, 5, 7, 64, 128), (2, 33, 70, 64, 128)]   # n, h, w, cin, cout
# f. the first convolution: (n, h, w); 3 -> 32 channels, 7 x 7 stride 2
FIRST = [(1, 9, 11), (2, 12, 20), (3, 37, 91)]
# g. the fp32 family
F32 = [IGEMM[0], IGEMM[4], IGEMM[10], IGEMM[11]]
F32_T = [IGEMM_T[0]]
# h. the fp32 pack's edge tiles (the fp32 forward takes output channels in
#    multiples of 16, the pack moves 32 x 32 tiles): Cout = 16, less than one
#    tile, and 48, one whole tile plus a half -- the two smallest channel counts
#    at which a guard can be wrong on either side of a tile edge
F32_EDGE = [conv(1, 32, 16, 3, 7, 3, 1), conv(1, 32, 48, 5, 17, 3, 1)]


def c32_case(n, h, w, cin=32, cout=32):
  return conv(n, cin, cout, h, w, 3, 1)


def first_case(n, h, w):
  return conv(n, 3, 32, h, w, 7, 2)


def all_cases():
  """Every case of sections a - h, once."""
  cs = IGEMM + IGEMM_T + SPLIT[2:] + [c for _, c in CAT]
  cs += [c32_case(*s) for s in C32_FWD] + [c32_case(n, h, w, 32, 16) for n, h, w in C32_FWD]
  cs += [c32_case(*s) for s in C32_WGRAD]
  cs += [first_case(*s) for s in FIRST]
  cs += F32_EDGE
  seen, out = set(), []
  for c in cs:
    if c not in seen:
      seen.add(c)
      out.append(c)
  return out


def stats_groups(case):
  return tuple(g for c, g in STATS if c == case) + \
      ((1, case.n) if case.cin == 3 else ())


# ---- every kernel build the planner can choose (section 4) ------------------------
# conv_igemm_kernel<RW, NCT, G>: RW rows per wave (tile = 4 RW rows x 16 columns),
# NCT = 4 | 2 (64 | 32 output channels per workgroup), G taps per weight stage.
# The planner's knobs are read once per process, so each sweep is a child process
# (conv_exact_child.py) with LSI_IGEMM_MINWG = 1 and one LSI_IGEMM_MAXRW.  A case
# runs forward and data gradient: two launches, two plans.
#
# Where the builds come from (lsi_conv_igemm.hip, ig_shape): the patch of a tile
# is PH x PW pixels of 80 bytes, PH = (4 RW - 1) s + span_y, PW = 15 s + span_x,
# at most 768 pixels, and patch + G x BN x 80 bytes of weights <= 80 KiB.  At
# RW = 8 that leaves, for 64 output channels, G = 5 for 3 x 3 (what the 256 x
# 768 training layers run) and G = 4 for 5 x 5; 7 x 7 has no RW = 8 patch at all,
# so G = 7 there comes from a 1 x 7 kernel (the descriptor takes any kh, kw <= 7).
# RW = 8 also needs ceil(oh / 32) ceil(ow / 16) N ncls Cout / BN >= 1024.
SWEEPS = collections.OrderedDict([
    ('rw8', (8, [
        conv(8, 32, 256, 63, 250, 3, 1),        # <8,4,5>; data gradient <4,2,9>
        conv(8, 32, 96, 33, 350, 3, 1),         # <8,2,9>
        conv(8, 32, 96, 33, 350, 5, 1),         # <8,2,5>
        conv_hw(8, 32, 96, 33, 350, 1, 7, 1),   # <8,2,7>
        conv(8, 32, 256, 63, 250, 5, 1),        # <8,4,4>: G = 5 does not fit
    ])),
    ('rw8_classes', (8, [
        convt(8, 32, 64, 33, 250),              # <8,4,4>, four parity classes
        convt(8, 32, 32, 33, 512),              # <8,2,4>, 512 tiles: the XCD swizzle
        conv(8, 64, 64, 66, 500, 3, 2),         # stride 2: data gradient <8,4,4> in classes
    ])),
    ('rw4', (4, [
        conv(2, 32, 64, 17, 33, 3, 1),          # <4,4,9> / <4,2,9>
        conv(1, 32, 64, 19, 21, 7, 1),          # <4,4,7> / <4,2,7>
        conv(2, 64, 32, 18, 20, 5, 1),          # <4,2,5> / <4,4,5>
        convt(2, 64, 32, 9, 17),                # <4,2,4>
        convt(1, 32, 64, 10, 20),               # <4,4,4>
        conv(2, 32, 64, 33, 50, 5, 2),          # stride-2 data gradients: parity classes
        conv(2, 64, 128, 40, 36, 3, 2),
        convt(3, 32, 32, 300, 140),             # 513 tiles in classes: no swizzle
    ])),
    ('rw2', (2, [
        conv(2, 32, 64, 9, 33, 3, 1),
        conv(1, 32, 64, 11, 21, 7, 1),
        conv(2, 64, 32, 10, 20, 5, 1),
        convt(2, 64, 32, 5, 17),
        convt(1, 32, 64, 6, 20),
        conv(2, 32, 64, 17, 50, 5, 2),
        conv(2, 64, 128, 20, 36, 3, 2),
        convt(8, 32, 32, 64, 128),              # 512 tiles in classes: the XCD swizzle
        convt(3, 32, 32, 150, 140),             # 513 tiles: no swizzle
    ])),
    ('rw1', (1, [
        conv(2, 32, 64, 5, 33, 3, 1),
        conv(1, 32, 64, 7, 21, 7, 1),
        conv(2, 64, 32, 6, 20, 5, 1),
        convt(2, 64, 32, 3, 17),
        convt(1, 32, 64, 3, 20),
        conv(2, 32, 64, 9, 50, 5, 2),
        conv(2, 64, 128, 10, 36, 3, 2),
    ])),
])


def sweep_env(name):
  return {'LSI_IGEMM_MINWG': '1', 'LSI_IGEMM_MAXRW': str(SWEEPS[name][0]),
          'LSI_IG_DEBUG': '1'}
