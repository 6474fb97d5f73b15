"""Inputs and NumPy restatements for the exact tests of the evaluation kernels
(csrc/lsi_eval.hip: eval_view_kernel, eval_layer_kernel, their finishing
kernels, disocclusion_kernel).  No torch, no device.

The kernels keep one fp32 sum per thread and quantity, widen it to fp64 and add
the rest in fp64 (csrc/lsi_reduce.h).  On the lattice inputs built here every
per-cell value is a small integer multiple of a power of two (its *unit*), so
fp32 computes it without rounding, and a thread's fp32 sum is exact as long as

    cells per thread x largest term / unit < 2^24            (the condition)

-- `exactness` evaluates that per case and quantity; nothing is assumed.  The
fp64 additions that follow are exact for the same reason with 2^53, so every
slot of the accumulator equals the exact total, whatever the order.

View metrics, lattice regime (`view_inputs`):
  target        integers in [0, 64] x 2^-6; AREA factors from {1, 2, 4}^2, so
                1 / (fy fx) is a power of two and the box mean t is on 2^-10
  recons        t - e, e on 2^-10, |e| < 2^-2; per cell and layer the three
                |e_c| 2^10 share one residue mod 3, so |e0| + |e1| + |e2| and
                e0^2 + e1^2 + e2^2 are divisible by 3 units: the kernel's
                `/ 3.0f` is exact.  Every third cell of a further layer holds a
                rotation of layer 0's errors: an exact tie of the minimum
  gt_disp       integers in [0, 26] x 2^-6; recons_disp the box mean -+ 2^-10
                steps, with ties between the layers of the same kind
  disocc        fp32 in {0, 1/4, .., 1}, bool or uint8: the box mean is on 2^-6
  valid         a band of zeros through the blocks, blocks with one zero
                element ((n - 1) / n <= 0.9375: out), and at factor 1 values of
                float32(0.95) (out) and its successor (in); or, with
                valid_above, a map with values equal to the threshold (invalid)
View metrics, rounded regime (`lattice=False`): arbitrary fp32 and any factor;
`view_cells(.., np.float32)` then computes every cell with one rounding per
operation in the kernel's order.

Layer metrics: textures and images on 2^-8, disparities on 2^-10,
bg_layer_disp = 2^-4, with pixels at gt == bg_layer_disp and gt == gt_bg.

Dis-occlusion mask: per item the matrix
    [1 0 s u0 - 1/2   16 s]      u  = x / s + u0 + k / 4
    [0 1 s v0 - 1/2  -16 s]      v  = y / s + v0 - k / 4
    [0 0 s            0   ]      dd = c + d
    [0 0 s c          s   ]
on source disparities d = k 2^-6, k in [0, 12]: a translation with a
disparity-proportional shift whose third row makes every division exact; u, v
fall on the quarter-pixel lattice, the bilinear weights on sixteenths, and with
disps_trg on 2^-8 the sampled disparity and |dd - sampled| on 2^-12.
"""
import collections
import decimal
import math

import numpy as np

TPB, MAXBLK = 256, 2048            # csrc/lsi_reduce.h
GRID_CELLS = TPB * MAXBLK          # cells one pass of the largest grid holds
F32 = np.float32
VALID_MIN = F32(0.95)              # the kernel's `v > 0.95f`


def grid_for(n):
  """csrc/lsi_reduce.h: blocks of a grid-stride pass over n items."""
  return max(1, min(MAXBLK, -(-n // TPB)))


def cells_per_thread(n):
  return -(-n // (grid_for(n) * TPB))


def py2_round(x):
  return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def is_f32(a):
  a = np.asarray(a, np.float64)
  return bool((a.astype(F32).astype(np.float64) == a).all())


# ---------------------------------------------------------------------------
# view metrics
# ---------------------------------------------------------------------------
ViewCase = collections.namedtuple(
    'ViewCase', 'name b ht wt fy fx nl bdry valid disocc depth layout lattice')


def _v(name, b, ht, wt, fy=1, fx=1, nl=2, bdry=0.1, valid='mask', disocc='f32',
       depth=True, layout='plain', lattice=True):
  return ViewCase(name, b, ht, wt, fy, fx, nl, bdry, valid, disocc, depth, layout, lattice)


LATTICE_FACTORS = [(fy, fx) for fy in (1, 2, 4) for fx in (1, 2, 4)]
VIEW_SMALL = (
    [_v('one-cell', 1, 1, 1, nl=1, bdry=0.0, valid=None)] +
    # three blocks, the last partial, the image boundary inside block 1
    [_v('7x37-f%dx%d' % f, 2, 7, 37, *f) for f in LATTICE_FACTORS] +
    [_v('crop-0', 2, 7, 37, 2, 2, bdry=0.0),
     _v('crop-single-cell', 1, 7, 37, 2, 2, bdry=0.48, valid=None),
     _v('crop-nothing-left', 2, 7, 37, 2, 2, bdry=0.5),
     _v('nl-1', 2, 7, 37, 2, 2, nl=1),
     _v('nl-4', 2, 7, 37, 2, 2, nl=4),
     _v('valid-none', 2, 7, 37, 2, 2, valid=None),
     _v('valid-above-f1x1', 2, 7, 37, 1, 1, valid='above'),
     _v('valid-above-f2x2', 2, 7, 37, 2, 2, valid='above'),
     _v('valid-above-f4x4', 2, 7, 37, 4, 4, valid='above'),
     _v('disocc-none', 2, 7, 37, 2, 2, disocc=None),
     _v('disocc-bool', 2, 7, 37, 2, 2, disocc='bool'),
     _v('disocc-u8', 2, 7, 37, 2, 2, disocc='u8'),
     _v('disocc-zero', 2, 7, 37, 2, 2, disocc='zero'),
     _v('no-depth', 2, 7, 37, 2, 2, depth=False),
     _v('no-depth-no-disocc', 2, 7, 37, 2, 2, depth=False, disocc=None),
     _v('target-channels-first', 2, 7, 37, 2, 4, layout='cfirst'),
     _v('target-rgba', 2, 7, 37, 4, 2, layout='rgba')])
VIEW_WRAP = [
    _v('wrap-512x1024', 1, 512, 1024, nl=1, bdry=0.0, valid=None, disocc='bool'),
    _v('wrap-3x1x174763', 3, 1, 174763, nl=2, bdry=0.0, valid=None),
    _v('wrap-512x1152', 1, 512, 1152, nl=2)]
VIEW_LATTICE = VIEW_SMALL + VIEW_WRAP
VIEW_ROUNDED = [
    _v('rounded-f3x3', 2, 7, 37, 3, 3, lattice=False),
    _v('rounded-f5x5', 2, 7, 37, 5, 5, lattice=False, disocc='bool'),
    _v('rounded-f3x2', 2, 7, 37, 3, 2, nl=4, lattice=False),
    _v('rounded-f1x1-511x1024', 1, 511, 1024, 1, 1, lattice=False, valid=None),
    _v('rounded-f2x4', 2, 7, 37, 2, 4, lattice=False, layout='cfirst')]

VIEW_KEYS = ('compose_splat_loss', 'compose_splat_loss_disocc', 'depth_splat_loss',
             'depth_splat_loss_disocc')
# per-thread sums of eval_view_kernel and the unit of each on the lattice
VIEW_UNITS = collections.OrderedDict(
    [('pw', 2.0 ** -10), ('centre', 1.0), ('pw_dm', 2.0 ** -16), ('centre_dm', 2.0 ** -6),
     ('pd', 2.0 ** -10), ('pd_dm', 2.0 ** -16), ('se', 2.0 ** -20)])
VALID_ABOVE = 3.0 / 64


def _seed(name):
  return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


def _box(x, fy, fx):
  """Exact fp64 box mean of a lattice map b x h x w x c (builders only)."""
  b, h, w, c = x.shape
  return x.reshape(b, h // fy, fy, w // fx, fx, c).astype(np.float64).sum(axis=(2, 4)) / (fy * fx)


def _valid_mask(rs, case, planted):
  b, ht, wt, fy, fx = case.b, case.ht, case.wt, case.fy, case.fx
  h, w = fy * ht, fx * wt
  v = np.ones((b, h, w, 1), F32)
  if h >= 5 and w >= 8:
    v[:, h // 3:h // 3 + max(3, h // 5)] = 0      # rows: edges inside the blocks
    v[:, :, w // 2 + 1:w // 2 + 4] = 0            # columns: three wide, odd start
  blocks = v.reshape(b, ht, fy, wt, fx)
  kind = rs.randint(0, 8, (b, ht, wt))
  full = blocks.min(axis=(2, 4)) == 1
  if fy * fx > 1:     # one element of the block zero: (n - 1) / n, out
    sel = full & (kind == 1)
    blocks[:, :, fy - 1, :, fx - 1][sel] = 0
    planted['valid blocks with one zero element'] = int(sel.sum())
    planted['valid blocks all ones'] = int((full & (kind != 1)).sum())
  else:
    below, above = full & (kind == 1), full & (kind == 2)
    blocks[:, :, 0, :, 0][below] = VALID_MIN
    blocks[:, :, 0, :, 0][above] = np.nextafter(VALID_MIN, F32(1))
    planted['valid == float32(0.95)'] = int(below.sum())
    planted['valid == its successor'] = int(above.sum())
  return v


def view_inputs(case):
  """The arrays of one add_rendered call, x_min / y_min and the planted counts."""
  rs = np.random.RandomState(_seed(case.name))
  b, ht, wt, fy, fx, nl = case.b, case.ht, case.wt, case.fy, case.fx, case.nl
  h, w = fy * ht, fx * wt
  planted = {}
  d = {'case': case, 'planted': planted, 'valid_above': None, 'valid': None, 'disocc': None,
       'recons_disp': None, 'gt_disp': None,
       'x_min': py2_round(wt * case.bdry), 'y_min': py2_round(ht * case.bdry)}
  if not case.lattice:
    d['target'] = rs.rand(b, h, w, 3).astype(F32)
    d['recons'] = rs.rand(nl, b, ht, wt, 3).astype(F32)
    if case.depth:
      d['gt_disp'] = (0.4 * rs.rand(b, h, w, 1)).astype(F32)
      d['recons_disp'] = (0.4 * rs.rand(nl, b, ht, wt, 1)).astype(F32)
    if case.valid:
      d['valid'] = (rs.rand(b, h, w, 1) > 0.02).astype(F32)
    if case.disocc == 'f32':
      d['disocc'] = rs.rand(b, h, w, 1).astype(F32)
    elif case.disocc:
      d['disocc'] = rs.rand(b, h, w, 1) > 0.6
    return d
  assert (fy, fx) in LATTICE_FACTORS
  d['target'] = (rs.randint(0, 65, (b, h, w, 3)) / 64.0).astype(F32)
  t = _box(d['target'], fy, fx)
  # |e_c| 2^10 = 3 k_c + r, one r per cell and layer; < 256
  mag = 3 * rs.randint(0, 85, (nl, b, ht, wt, 3)) + rs.randint(0, 3, (nl, b, ht, wt, 1))
  sign = 2 * rs.randint(0, 2, (nl, b, ht, wt, 3)) - 1
  tie = (np.arange(b * ht * wt).reshape(b, ht, wt) % 3) == 1
  for l in range(1, nl):
    mag[l][tie] = np.roll(mag[0], l, axis=-1)[tie]
  planted['cells with tied colour layers'] = int(tie.sum()) if nl > 1 else 0
  recons = t[None] - sign * mag / 1024.0
  d['recons'] = recons.astype(F32)
  assert is_f32(recons) and int(mag.max()) < 256
  if case.depth:
    d['gt_disp'] = (rs.randint(0, 27, (b, h, w, 1)) / 64.0).astype(F32)
    g = _box(d['gt_disp'], fy, fx)
    ed = rs.randint(-100, 101, (nl, b, ht, wt, 1))
    tie_d = (np.arange(b * ht * wt).reshape(b, ht, wt) % 5) == 2
    for l in range(1, nl):
      ed[l][tie_d] = -ed[0][tie_d]
    d['recons_disp'] = (g[None] - ed / 1024.0).astype(F32)
    planted['cells with tied disparity layers'] = int(tie_d.sum()) if nl > 1 else 0
  if case.valid == 'mask':
    d['valid'] = _valid_mask(rs, case, planted)
  elif case.valid == 'above':
    m = rs.randint(4, 27, (b, h, w, 1))
    kind = rs.randint(0, 6, (b, ht, wt))
    blocks = m.reshape(b, ht, fy, wt, fx)
    blocks[:, :, fy - 1, :, fx - 1][kind == 1] = 3      # equal to the threshold: invalid
    blocks[:, :, 0, :, 0][kind == 2] = 1                # below it
    planted['blocks with a value == valid_above'] = int((kind == 1).sum())
    planted['blocks with a value below valid_above'] = int((kind == 2).sum())
    d['valid'] = (m / 64.0).astype(F32)
    d['valid_above'] = VALID_ABOVE
  if case.disocc == 'f32':
    d['disocc'] = (rs.randint(0, 5, (b, h, w, 1)) / 4.0).astype(F32)
  elif case.disocc == 'zero':
    d['disocc'] = np.zeros((b, h, w, 1), F32)
  elif case.disocc == 'bool':
    d['disocc'] = rs.rand(b, h, w, 1) > 0.6
  elif case.disocc == 'u8':
    d['disocc'] = (rs.rand(b, h, w, 1) > 0.6).astype(np.uint8)
  return d


def _area(x, fy, fx, dt):
  """area_mean (csrc/lsi_layers.h): the block's elements added in order, rows
  then columns, from 0, then one multiply by fl(1 / (fy fx))."""
  b, h, w, c = x.shape
  blk = x.reshape(b, h // fy, fy, w // fx, fx, c)
  t = np.zeros((b, h // fy, w // fx, c), dt)
  for dy in range(fy):
    for dx in range(fx):
      t = t + blk[:, :, dy, :, dx, :].astype(dt)
  return t * (dt(1) / dt(fy * fx))


Cells = collections.namedtuple('Cells', 'centre terms best_colour best_disp')


def view_cells(d, dt=np.float64, mutate=None):
  """Every cell's contribution to the seven sums of eval_view_kernel, computed
  in `dt` with one operation per operation of the kernel, in its order
  (np.float32: one rounding each; on the lattice nothing rounds in either
  type).  `centre`: the scored cells; the terms are 0 elsewhere.
  mutate: 'skip_cell' drops the first cell past the grid, 'layer0' takes layer
  0 where the minimum over the layers is wanted, 'dm_shift' reads the
  dis-occlusion block one column over (tests/test_eval_lattice_cpu.py)."""
  case = d['case']
  fy, fx = case.fy, case.fx
  recons = d['recons'].astype(dt)
  nl, b, ht, wt, _ = recons.shape
  centre = np.zeros((b, ht, wt), bool)
  centre[:, d['y_min']:ht - d['y_min'], d['x_min']:wt - d['x_min']] = True
  if d['valid'] is not None:
    if d['valid_above'] is not None:
      ind = (d['valid'] > F32(d['valid_above'])).astype(dt)
      v = _area(ind, fy, fx, dt)
    else:
      v = _area(d['valid'], fy, fx, dt)
    centre &= v[..., 0] > dt(VALID_MIN)
  if mutate == 'skip_cell':
    assert centre.reshape(-1)[GRID_CELLS]
    centre.reshape(-1)[GRID_CELLS] = False
  t = _area(d['target'], fy, fx, dt)
  e = t[None] - recons
  a = np.abs(e)
  three = dt(3)
  l1 = ((a[..., 0] + a[..., 1]) + a[..., 2]) / three
  se = ((e[0, ..., 0] * e[0, ..., 0] + e[0, ..., 1] * e[0, ..., 1]) +
        e[0, ..., 2] * e[0, ..., 2]) / three
  pw = l1[0]
  for l in range(1, nl):
    pw = np.minimum(pw, l1[l])
  if mutate == 'layer0':
    pw = l1[0]
  dm = np.zeros((b, ht, wt), dt)
  if d['disocc'] is not None:
    dm = _area(d['disocc'], fy, fx, dt)[..., 0]
    if mutate == 'dm_shift':
      dm = np.roll(dm, -1, axis=2)
  pd = np.zeros((b, ht, wt), dt)
  best_disp = None
  if d['recons_disp'] is not None and d['gt_disp'] is not None:
    g = _area(d['gt_disp'], fy, fx, dt)[..., 0]
    ad = np.abs(g[None] - d['recons_disp'].astype(dt)[..., 0])
    pd = ad[0]
    for l in range(1, nl):
      pd = np.minimum(pd, ad[l])
    best_disp = ad == pd[None]
  terms = collections.OrderedDict(
      [('pw', pw), ('centre', np.ones((b, ht, wt), dt)), ('pw_dm', pw * dm), ('centre_dm', dm),
       ('pd', pd), ('pd_dm', pd * dm), ('se', se)])
  zero = dt(0)
  for k in terms:
    assert terms[k].dtype == dt, (k, terms[k].dtype)
    terms[k] = np.where(centre, terms[k], zero)
  return Cells(centre, terms, l1 == pw[None], best_disp)


def view_sums(cells):
  """The seven totals: the cells' values added without error (math.fsum)."""
  return {k: math.fsum(v[cells.centre].astype(np.float64).tolist())
          for k, v in cells.terms.items()}


def view_slots(d, s):
  """name -> (sum, norm) as eval_view_finish_kernel adds them; (0, 0) for a
  metric whose input is absent."""
  has_dm = d['disocc'] is not None
  has_depth = d['recons_disp'] is not None and d['gt_disp'] is not None
  out = {k: (0.0, 0.0) for k in VIEW_KEYS}
  out['compose_splat_loss'] = (s['pw'], s['centre'])
  if has_dm:
    out['compose_splat_loss_disocc'] = (s['pw_dm'], s['centre_dm'])
  if has_depth:
    out['depth_splat_loss'] = (s['pd'], s['centre'])
    if has_dm:
      out['depth_splat_loss_disocc'] = (s['pd_dm'], s['centre_dm'])
  return out


def exactness(cells, n_cells):
  """The condition, per sum: the cells' values are integer multiples of the
  unit, and cells per thread x largest value / unit.  Returns name -> that
  figure (to be held below 2^24)."""
  cpt = cells_per_thread(n_cells)
  out = collections.OrderedDict()
  for k, unit in VIEW_UNITS.items():
    q = cells.terms[k].astype(np.float64) / unit
    assert (q == np.round(q)).all() and (q >= 0).all(), k
    out[k] = cpt * float(q.max())
  return out


def fp32_thread_sums(values, n_cells, rs):
  """The total the kernel's scheme gives for one random assignment of cells to
  threads: cells_per_thread cells per thread added in fp32 in sequence, the
  threads' sums added in fp64 (exactly: fsum)."""
  cpt = cells_per_thread(n_cells)
  v = np.zeros((-(-values.size // cpt) * cpt,), F32)
  v[:values.size] = values.reshape(-1).astype(F32)
  v = v[rs.permutation(v.size)].reshape(-1, cpt)
  acc = np.zeros((v.shape[0],), F32)
  for j in range(cpt):
    acc = acc + v[:, j]
  return math.fsum(acc.astype(np.float64).tolist())


def psnr_reference(se, centre):
  """10 log10(centre / se) at 50 digits from the exact totals; the kernel's
  floor of the mean squared error at 1e-20 applied; None without a scored cell."""
  if centre == 0:
    return None
  with decimal.localcontext() as ctx:
    ctx.prec = 50
    mse = max(decimal.Decimal(se) / decimal.Decimal(centre), decimal.Decimal(1e-20))
    return 10 * (1 / mse).log10()


def ulp_distance(got, want):
  """|got - want| in ulps of float(want); want a Decimal."""
  with decimal.localcontext() as ctx:
    ctx.prec = 50
    return float(abs(decimal.Decimal(got) - want) / decimal.Decimal(math.ulp(float(want))))


# ---------------------------------------------------------------------------
# layer metrics
# ---------------------------------------------------------------------------
LayerCase = collections.namedtuple('LayerCase', 'name b h w L bg layout')
BG_LAYER_DISP = 2.0 ** -4
LAYER_SMALL = [
    LayerCase('1x1x1-L1', 1, 1, 1, 1, True, 'plain'),
    LayerCase('1x5x77-L1', 1, 5, 77, 1, True, 'plain'),     # 2 P = 770: block 1 holds both views
    LayerCase('1x5x77-L2', 1, 5, 77, 2, True, 'plain'),
    LayerCase('2x5x77-L4', 2, 5, 77, 4, True, 'plain'),
    LayerCase('no-bg', 1, 5, 77, 2, False, 'plain'),
    LayerCase('permuted', 1, 5, 77, 2, True, 'permuted'),
    LayerCase('packed-rgbd', 1, 5, 77, 2, True, 'packed')]
LAYER_WRAP = [LayerCase('wrap-1x512x520', 1, 512, 520, 2, True, 'plain')]   # 2 P = 532 480
LAYER_CASES = LAYER_SMALL + LAYER_WRAP
LAYER_KEYS = ('fg_tex_error', 'fg_disp_error', 'bg_tex_error', 'bg_disp_error')


def layer_inputs(case):
  """{'src' | 'trg': {tex, disp, img, gt_disp, gt_disp_bg, gt_tex_bg}}, 'planted'."""
  rs = np.random.RandomState(_seed(case.name))
  b, h, w, L = case.b, case.h, case.w, case.L
  out = {'case': case, 'planted': {'gt == bg_layer_disp': 0, 'gt == gt_bg': 0}}
  for side, off in (('src', 0), ('trg', 1)):
    idx = np.arange(b * h * w).reshape(b, h, w, 1) + off
    gt = rs.randint(0, 411, (b, h, w, 1))
    gt[idx % 8 == 1] = int(BG_LAYER_DISP * 1024)
    gt_bg = rs.randint(0, 411, (b, h, w, 1))
    gt_bg[idx % 8 == 2] = gt[idx % 8 == 2]
    out['planted']['gt == bg_layer_disp'] += int((gt == 64).sum())
    out['planted']['gt == gt_bg'] += int((gt == gt_bg).sum())
    out[side] = {
        'tex': (rs.randint(0, 257, (L, b, h, w, 3)) / 256.0).astype(F32),
        'disp': (rs.randint(0, 411, (L, b, h, w, 1)) / 1024.0).astype(F32),
        'img': (rs.randint(0, 257, (b, h, w, 3)) / 256.0).astype(F32),
        'gt_disp': (gt / 1024.0).astype(F32),
        'gt_disp_bg': (gt_bg / 1024.0).astype(F32) if case.bg else None,
        'gt_tex_bg': (rs.randint(0, 257, (b, h, w, 3)) / 256.0).astype(F32) if case.bg else None}
  return out


def layer_restate(d, strict=True, dt=np.float64):
  """name -> (sum, norm) of eval_layer_kernel and its finishing kernel: both
  views' pixels in one total per quantity, the texture totals divided by 3.0
  once in fp64.  strict=False admits gt == bg_layer_disp and gt == gt_bg (the
  mutation the planted pixels are there to notice).  Also returns the largest
  per-pixel term of each sum over its unit."""
  gt_cmp = (lambda a, b: a > b) if strict else (lambda a, b: a >= b)
  L = d['case'].L
  tot = collections.OrderedDict((k, []) for k in ('fg_tex', 'fg_disp', 'fg_n', 'bg_tex', 'bg_disp',
                                                  'bg_n'))
  for side in ('src', 'trg'):
    v = d[side]
    gd = v['gt_disp'].astype(dt)[..., 0]
    tex_l1 = lambda tex, ref: ((np.abs(tex[..., 0] - ref[..., 0]) + np.abs(tex[..., 1] - ref[..., 1]))
                               + np.abs(tex[..., 2] - ref[..., 2]))
    fg = gt_cmp(gd, dt(F32(BG_LAYER_DISP)))
    tot['fg_tex'].append(tex_l1(v['tex'][0].astype(dt), v['img'].astype(dt))[fg])
    tot['fg_disp'].append(np.abs(v['disp'][0].astype(dt)[..., 0] - gd)[fg])
    tot['fg_n'].append(np.ones(gd.shape, dt)[fg])
    if v['gt_disp_bg'] is not None:
      gb = v['gt_disp_bg'].astype(dt)[..., 0]
      bg = gt_cmp(gd, gb)
      tot['bg_tex'].append(tex_l1(v['tex'][L - 1].astype(dt), v['gt_tex_bg'].astype(dt))[bg])
      tot['bg_disp'].append(np.abs(v['disp'][L - 1].astype(dt)[..., 0] - gb)[bg])
      tot['bg_n'].append(np.ones(gd.shape, dt)[bg])
  units = {'fg_tex': 2.0 ** -8, 'fg_disp': 2.0 ** -10, 'fg_n': 1.0, 'bg_tex': 2.0 ** -8,
           'bg_disp': 2.0 ** -10, 'bg_n': 1.0}
  s, worst = {}, collections.OrderedDict()
  for k, parts in tot.items():
    a = np.concatenate(parts).astype(np.float64) if parts else np.zeros((0,))
    q = a / units[k]
    assert (q == np.round(q)).all(), k
    worst[k] = float(q.max()) if a.size else 0.0
    s[k] = math.fsum(a.tolist())
  out = {'fg_tex_error': (s['fg_tex'] / 3.0, s['fg_n']), 'fg_disp_error': (s['fg_disp'], s['fg_n']),
         'bg_tex_error': (0.0, 0.0), 'bg_disp_error': (0.0, 0.0)}
  if d['case'].bg:
    out['bg_tex_error'] = (s['bg_tex'] / 3.0, s['bg_n'])
    out['bg_disp_error'] = (s['bg_disp'], s['bg_n'])
  return out, worst


# ---------------------------------------------------------------------------
# dis-occlusion mask
# ---------------------------------------------------------------------------
# items: per batch element (s, u0, v0) of the matrix in the module docstring
DisoccCase = collections.namedtuple('DisoccCase', 'name hs ws ht wt items')
DISOCC_CASES = [
    DisoccCase('1x1', 1, 1, 1, 1, ((1.0, 0.25, 1.0),)),
    DisoccCase('5x77-onto-7x33', 5, 77, 7, 33,
               ((2.0, -1.0, 6.5), (0.5, -1.0, 1.0), (-1.0, 40.0, 8.0))),
    DisoccCase('ns-256', 16, 16, 16, 16, ((1.0, -1.0, 2.0),)),
    DisoccCase('ns-257', 1, 257, 1, 257, ((1.0, -1.0, 1.0),))]
DISOCC_THRESH = 2.0 ** -5
DISOCC_C = 3.0 / 256
K_MAX = 12


def disocc_matrix(s, u0, v0):
  return np.array([[1, 0, s * u0 - 0.5, 16 * s], [0, 1, s * v0 - 0.5, -16 * s],
                   [0, 0, s, 0], [0, 0, s * DISOCC_C, s]], F32)


def disocc_restate(ds, dt_, mat, thresh):
  """projection.py:109-150 in fp64 on the pixel-centre grid: transform, the two
  divide_safe, the strict truncation tests, the four-tap gather with its
  validity masks (sampling.py:54-123, compose=True), the threshold.  Returns
  the mask B x Hs x Ws x 1 (fp32) and the intermediate values."""
  ds = np.asarray(ds, np.float64)[..., 0]
  trg = np.asarray(dt_, np.float64)[..., 0]
  mat = np.asarray(mat, np.float64)
  b, hs, ws = ds.shape
  _, ht, wt = trg.shape
  px = (np.arange(ws) + 0.5)[None, None, :] + np.zeros((b, hs, 1))
  py = (np.arange(hs) + 0.5)[None, :, None] + np.zeros((b, 1, ws))
  pts = np.stack([px, py, np.ones_like(px), ds], axis=-1)            # b hs ws 4
  q = np.einsum('bij,bhwj->bhwi', mat, pts)
  den = q[..., 2] + 1e-8 * (q[..., 2] == 0)
  u, v, dd = q[..., 0] / den, q[..., 1] / den, q[..., 3] / den
  trunc = (u > wt) | (v > ht) | (u < 0) | (v < 0)
  x, y = u - 0.5, v - 0.5
  x0, y0 = np.floor(x), np.floor(y)
  x1, y1 = x0 + 1, y0 + 1
  clipx = lambda a: np.clip(a, 0, wt - 1)
  clipy = lambda a: np.clip(a, 0, ht - 1)
  bi = np.arange(b)[:, None, None]
  sampled = np.zeros_like(u)
  partial = np.zeros(u.shape, bool)
  for xa, wxa in ((x0, x1 - x), (x1, x - x0)):
    for ya, wya in ((y0, y1 - y), (y1, y - y0)):
      ok = (xa == clipx(xa)) & (ya == clipy(ya))
      tap = trg[bi, clipy(ya).astype(int), clipx(xa).astype(int)]
      sampled = sampled + ok * wxa * wya * tap
      partial |= ~ok & (wxa * wya > 0)
  diff = np.abs(dd - sampled)
  dis = diff > thresh
  mask = ((~trunc) & dis).astype(F32)[..., None]
  return mask, dict(u=u, v=v, dd=dd, sampled=sampled, diff=diff, trunc=trunc, dis=dis,
                    partial=partial & ~trunc)


def disocc_inputs(case):
  """disps_src, disps_trg, M, thresh with the edges planted; `planted` counts
  them from the restatement's own intermediate values."""
  rs = np.random.RandomState(_seed(case.name))
  b = len(case.items)
  hs, ws, ht, wt = case.hs, case.ws, case.ht, case.wt
  k = rs.randint(0, K_MAX + 1, (b, hs, ws))
  mat = np.stack([disocc_matrix(*it) for it in case.items])
  # the coordinate edges: every source pixel that can reach one takes it, in turn
  turn = 0
  for i, (s, u0, v0) in enumerate(case.items):
    for y in range(hs):
      for x in range(ws):
        reach = []
        for want in (0.0, float(wt), -0.25, wt + 0.25):
          kk = 4 * (want - x / s - u0)
          if kk == int(kk) and 0 <= kk <= K_MAX:
            reach.append(int(kk))
        for want in (0.0, float(ht), -0.25, ht + 0.25):
          kk = 4 * (y / s + v0 - want)
          if kk == int(kk) and 0 <= kk <= K_MAX:
            reach.append(int(kk))
        if reach and (x + y) % 2 == 0:
          k[i, y, x] = reach[turn % len(reach)]
          turn += 1
  ds = (k / 64.0).astype(F32)[..., None]
  trg = (rs.randint(0, 65, (b, ht, wt, 1)) / 256.0).astype(F32)
  # the threshold's edges: a source pixel that falls on a target pixel's centre
  # samples that pixel alone; give it dd -+ thresh, and dd -+ (thresh + 2^-8)
  _, z = disocc_restate(ds, trg, mat, DISOCC_THRESH)
  used = set()
  n = 0
  for i, y, x in zip(*np.nonzero(~z['trunc'])):
    tx, ty = z['u'][i, y, x] - 0.5, z['v'][i, y, x] - 0.5
    if tx != int(tx) or ty != int(ty) or not (0 <= tx < wt and 0 <= ty < ht):
      continue
    if (i, int(ty), int(tx)) in used:
      continue
    step = DISOCC_THRESH + (2.0 ** -8 if n % 2 else 0.0)
    val = z['dd'][i, y, x] + (step if n % 4 < 2 else -step)
    if not 0 <= val <= 1:
      val = z['dd'][i, y, x] - (step if n % 4 < 2 else -step)
    trg[i, int(ty), int(tx), 0] = val
    used.add((i, int(ty), int(tx)))
    n += 1
  mask, z = disocc_restate(ds, trg, mat, DISOCC_THRESH)
  inside_u = (z['u'] >= 0) & (z['u'] <= wt)
  inside_v = (z['v'] >= 0) & (z['v'] <= ht)
  live = z['dis']          # where the truncation decides the mask
  planted = collections.OrderedDict([
      ('|dd - sampled| == thresh', int(((z['diff'] == DISOCC_THRESH) & ~z['trunc']).sum())),
      ('|dd - sampled| == thresh + 2^-8',
       int(((z['diff'] == DISOCC_THRESH + 2.0 ** -8) & ~z['trunc']).sum())),
      ('u == 0', int(((z['u'] == 0) & inside_v & live).sum())),
      ('u == Wt', int(((z['u'] == wt) & inside_v & live).sum())),
      ('v == 0', int(((z['v'] == 0) & inside_u & live).sum())),
      ('v == Ht', int(((z['v'] == ht) & inside_u & live).sum())),
      ('u == -1/4', int(((z['u'] == -0.25) & inside_v & live).sum())),
      ('u == Wt + 1/4', int(((z['u'] == wt + 0.25) & inside_v & live).sum())),
      ('v == -1/4', int(((z['v'] == -0.25) & inside_u & live).sum())),
      ('v == Ht + 1/4', int(((z['v'] == ht + 0.25) & inside_u & live).sum())),
      ('taps partly outside', int(z['partial'].sum())),
      ('negative-depth items', sum(1 for it in case.items if it[0] < 0)),
      ('mask == 1', int(mask.sum())), ('pixels', int(mask.size))])
  return {'case': case, 'disps_src': ds, 'disps_trg': trg, 'M': mat, 'thresh': DISOCC_THRESH,
          'mask': mask, 'z': z, 'planted': planted}
