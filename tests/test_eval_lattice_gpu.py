"""The evaluation kernels (csrc/lsi_eval.hip: eval_view_kernel, eval_layer_kernel,
the two finishing kernels, disocclusion_kernel) against the restatements of
tests/eval_lattice_ref.py, through lsi.nnutils._hip_eval and
eval_metrics.MetricAccumulator.

tests/test_eval_fused_gpu.py holds these kernels to 2e-4 of a sum, 0.05 dB and
a mask outside a `near` set.  Here nothing is left open:

* lattice inputs (every per-cell value a small multiple of a power of two, every
  per-thread fp32 sum below 2^24 units -- tests/test_eval_lattice_cpu.py asserts
  that per case): every (sum, norm) slot of the accumulator equals the
  restatement's doubles with `==`, in `sums()` and through the host's one
  division in `results()`; the slots of absent metrics are exactly 0; a second
  and third call keep the accumulator equal to the running fp64 total.  One
  cell lost, doubled, read from the neighbouring block or minimised over the
  wrong layers is a failed equality, at one cell, at three blocks with a
  partial one, and past the 524 288 cells one pass of the grid holds;
* arbitrary fp32 inputs and factors 3, 5, 3 x 2 at no more than one cell per
  thread: the restatement computes each cell in np.float32 with one rounding
  per operation in the kernel's order and adds them without error; the bar is
  |got - want| <= n 2^-53 want, n the scored cells (non-negative terms, every
  addition after the cell in fp64);
* PSNR: 10 log10(centre / se) at 50 digits from the exact totals, in ulps of the
  value (PSNR_BAR_ULP below); exactly 200 dB on the 1e-20 floor; nothing added
  when no cell is scored;
* the layer metrics: all six slots with `==`, at one pixel, with both views in
  one block, L = 1, 2, 4, permuted and packed storage, and past the grid;
* the dis-occlusion mask: torch.equal on every pixel, no `near` set.
"""
import functools
import types

import numpy as np
import pytest
import torch

import eval_lattice_ref as R

pytestmark = pytest.mark.gpu

# The device's fp64 log10 is the one free quantity of the PSNR slot (the two
# divisions before it and the multiply by 10 after it are IEEE operations).  No
# ulp bound for it is documented with the toolchain, so the bar is twice the
# worst distance measured on the MI355X over every lattice case of this file,
# in ulps of the value, and may never exceed 16.  Measured: 0.730 ulp at worst
# (31 values between 14.7 and 18.7 dB, median 0.3) -- the reference is taken from
# the exact rationals, so the roundings of the two divisions and of the multiply
# are inside that figure; the rounded regime's cells all equalled the np.float32
# restatement (worst |got - want| / (n 2^-53 want): 0).
PSNR_MEASURED_ULP = 0.730
PSNR_BAR_ULP = 2 * PSNR_MEASURED_ULP
assert PSNR_BAR_ULP <= 16

ALL_KEYS = R.VIEW_KEYS + R.LAYER_KEYS + ('psnr',)
WORST = {}     # what the run measured: printed by the last test
_id = lambda c: c.name


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def T(x, dev):
  return None if x is None else torch.tensor(x, device=dev)


def _worst(key, value):
  WORST[key] = max(WORST.get(key, 0.0), value)


# ---- view metrics ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _view_ref(case):
  """(inputs, cells, the seven totals, name -> (sum, norm)): computed once per
  case, shared and never modified."""
  d = R.view_inputs(case)
  cells = R.view_cells(d, np.float64 if case.lattice else np.float32)
  sums = R.view_sums(cells)
  return d, cells, sums, R.view_slots(d, sums)


def _on_device(d, dev):
  """The call's tensors; the target in the case's storage layout."""
  target = T(d['target'], dev)
  layout = d['case'].layout
  if layout == 'cfirst':      # channels-first storage viewed as B x H x W x 3
    target = target.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert not target.is_contiguous() or target.shape[1] * target.shape[2] == 1
  elif layout == 'rgba':      # channels 0:3 of a B x H x W x 4 tensor
    buf = torch.full(target.shape[:3] + (4,), float('nan'), device=dev)
    buf[..., :3] = target
    target = buf[..., :3]
    assert target.stride() == (buf.stride(0), buf.stride(1), 4, 1)
  return dict(recons=T(d['recons'], dev), recons_disp=T(d['recons_disp'], dev), target=target,
              valid=T(d['valid'], dev), disocc=T(d['disocc'], dev), gt_disp=T(d['gt_disp'], dev))


def _add(acc, d, dv):
  acc.add_rendered(dv['recons'], dv['recons_disp'], dv['target'], d['case'].bdry,
                   valid_mask=dv['valid'], disocc_mask=dv['disocc'], gt_disp_trg=dv['gt_disp'],
                   valid_above=d['valid_above'])


def _direct(d, dv, dev):
  """The same call through _hip_eval.view_metrics into 16 doubles of its own."""
  from lsi.nnutils import _hip_eval
  acc = torch.zeros((_hip_eval.SLOT_COUNT,), dtype=torch.float64, device=dev)
  ws, n = _hip_eval.workspace(dev)
  _hip_eval.view_metrics(acc, ws, n, dv['recons'], dv['recons_disp'], dv['target'], d['x_min'],
                         d['y_min'], valid=dv['valid'], disocc=dv['disocc'],
                         gt_disp=dv['gt_disp'], valid_above=d['valid_above'])
  return acc


def _check_psnr(name, got, sums):
  """One call's PSNR slot against the 50-digit value of the exact totals."""
  ref = R.psnr_reference(sums['se'], sums['centre'])
  if ref is None:
    assert got == (0.0, 0.0), (name, got)
    return
  dist = R.ulp_distance(got[0], ref)
  print('%s: psnr %r, reference %s, %.3f ulp' % (name, got[0], str(ref)[:24], dist))
  _worst('psnr ulp', dist)
  assert got[1] == 1.0
  assert dist <= PSNR_BAR_ULP, (name, got[0], ref, dist)


def _check_results(acc, want):
  res = acc.results()
  for k in R.VIEW_KEYS + R.LAYER_KEYS:
    s, n = want.get(k, (0.0, 0.0))
    if n > 0:
      assert res[k] == s / n, k
    else:
      assert k not in res, k


@pytest.mark.parametrize('case', R.VIEW_LATTICE, ids=_id)
def test_view_metrics_lattice(case, dev):
  from lsi.nnutils import eval_metrics
  d, cells, sums, want = _view_ref(case)
  dv = _on_device(d, dev)
  acc = eval_metrics.MetricAccumulator(dev)
  _add(acc, d, dv)
  got = acc.sums()
  for k in R.VIEW_KEYS:
    print('%s %s: got %r, want %r' % (case.name, k, got[k], want[k]))
  for k in R.VIEW_KEYS:
    assert got[k] == want[k], k
  for k in R.LAYER_KEYS:
    assert got[k] == (0.0, 0.0), k
  _check_psnr(case.name, got['psnr'], sums)
  _check_results(acc, want)
  assert ('psnr' in acc.results()) == (sums['centre'] > 0)
  assert torch.equal(_direct(d, dv, dev), acc.acc)


@pytest.mark.parametrize('case', R.VIEW_ROUNDED, ids=_id)
def test_view_metrics_rounded(case, dev):
  from lsi.nnutils import eval_metrics
  d, cells, sums, want = _view_ref(case)
  n = int(cells.centre.sum())
  assert 0 < n and case.b * case.ht * case.wt <= R.GRID_CELLS
  dv = _on_device(d, dev)
  acc = eval_metrics.MetricAccumulator(dev)
  _add(acc, d, dv)
  got = acc.sums()
  for k in R.VIEW_KEYS:
    for g, w in zip(got[k], want[k]):
      print('%s %s: got %r, want %r, n %d' % (case.name, k, g, w, n))
      if w > 0:
        _worst('rounded |got - want| / (n 2^-53 want)', abs(g - w) / (n * 2.0 ** -53 * w))
  for k in R.VIEW_KEYS:
    for g, w in zip(got[k], want[k]):
      assert abs(g - w) <= n * 2.0 ** -53 * w, (k, g, w)
  assert got['compose_splat_loss'][1] == n and got['psnr'][1] == 1.0
  assert torch.equal(_direct(d, dv, dev), acc.acc)


def test_view_metrics_accumulate_to_the_running_total(dev):
  """Five calls with different optional inputs into one accumulator: after
  each, every slot equals the running fp64 total, the PSNR slot the running
  sum of the calls' own values; a second accumulator gets the same bits."""
  from lsi.nnutils import eval_metrics
  by = {c.name: c for c in R.VIEW_LATTICE}
  cases = [by[n] for n in ('7x37-f2x2', 'no-depth-no-disocc', 'crop-nothing-left', 'nl-4',
                           '7x37-f4x1')]
  accs = [eval_metrics.MetricAccumulator(dev) for _ in range(2)]
  run = {k: (0.0, 0.0) for k in R.VIEW_KEYS + ('psnr',)}
  for case in cases:
    d, _, sums, want = _view_ref(case)
    dv = _on_device(d, dev)
    one = eval_metrics.MetricAccumulator(dev)
    _add(one, d, dv)
    psnr = one.sums()['psnr']
    for acc in accs:
      _add(acc, d, dv)
    for k in R.VIEW_KEYS:
      run[k] = (run[k][0] + want[k][0], run[k][1] + want[k][1])
    run['psnr'] = (run['psnr'][0] + psnr[0], run['psnr'][1] + psnr[1])
    got = accs[0].sums()
    for k in run:
      assert got[k] == run[k], (case.name, k)
    _check_results(accs[0], run)
  assert run['psnr'][1] == 4.0 and run['depth_splat_loss'][1] < run['compose_splat_loss'][1]
  assert torch.equal(accs[0].acc, accs[1].acc)


def test_psnr_floor_is_exactly_200_db(dev):
  """recons == the box mean of the target: se == 0, the mean squared error is
  floored at 1e-20."""
  from lsi.nnutils import eval_metrics
  case = next(c for c in R.VIEW_LATTICE if c.name == '7x37-f2x2')
  d = dict(_view_ref(case)[0])
  d['recons'] = np.repeat(R._box(d['target'], case.fy, case.fx)[None], case.nl, 0).astype(np.float32)
  sums = R.view_sums(R.view_cells(d))
  assert sums['se'] == 0.0 and sums['pw'] == 0.0 and sums['centre'] > 0
  acc = eval_metrics.MetricAccumulator(dev)
  _add(acc, d, _on_device(d, dev))
  got = acc.sums()
  assert got['psnr'] == (200.0, 1.0), got['psnr']
  assert got['compose_splat_loss'] == (0.0, sums['centre'])
  assert acc.results()['psnr'] == 200.0


def test_int32_maps_are_refused_and_nothing_is_added(dev):
  """valid, gt_disp and the layer ground truth as int32 pass _C.require_device;
  the eval wrappers refuse them before any launch."""
  from lsi.nnutils import _hip_eval, eval_metrics
  case = next(c for c in R.VIEW_LATTICE if c.name == '7x37-f2x2')
  d = _view_ref(case)[0]
  dv = _on_device(d, dev)
  acc = eval_metrics.MetricAccumulator(dev)
  as_int = lambda t: (t * 64).to(torch.int32)
  for bad in (dict(valid=as_int(dv['valid'])), dict(gt_disp=as_int(dv['gt_disp'])),
              dict(recons_disp=as_int(dv['recons_disp'])), dict(target=as_int(dv['target']))):
    with pytest.raises(RuntimeError, match='must be fp32'):
      _add(acc, d, dict(dv, **bad))
    with pytest.raises(RuntimeError, match='must be fp32'):
      _direct(d, dict(dv, **bad), dev)
  with pytest.raises(RuntimeError, match='must be fp32'):     # the thresholded map, too
    acc.add_rendered(dv['recons'], dv['recons_disp'], dv['target'], 0.1,
                     valid_mask=as_int(dv['gt_disp']), valid_above=3)
  with pytest.raises(RuntimeError, match='fp32 or bool'):
    _add(acc, d, dict(dv, disocc=dv['disocc'].to(torch.int32)))
  lcase = R.LAYER_SMALL[2]
  ld = R.layer_inputs(lcase)
  for key in ('gt_disp', 'gt_disp_bg', 'gt_tex_bg', 'img', 'disp'):
    ldis, imgs, gt = _layer_on_device(ld, dev)
    if key == 'img':
      imgs[1] = as_int(imgs[1])
    elif key == 'disp':
      ldis[0][2] = as_int(ldis[0][2])
    else:
      gt['trg_' + key] = as_int(gt['trg_' + key])
    with pytest.raises(RuntimeError, match='must be fp32'):
      acc.add_layer_prediction(ldis[0], ldis[1], imgs[0], imgs[1], gt,
                               types.SimpleNamespace(bg_layer_disp=R.BG_LAYER_DISP))
  z = torch.zeros((1, 2, 2, 1), dtype=torch.int32, device=dev)
  with pytest.raises(RuntimeError, match='must be fp32'):
    _hip_eval.disocclusion_mask(z, z.float(), torch.eye(4, device=dev)[None], 0.01)
  assert not acc.acc.cpu().numpy().any()
  assert acc.results() == {}


# ---- layer metrics ---------------------------------------------------------------------

def _layer_on_device(d, dev):
  """([ldi_src, ldi_trg], [img_src, img_trg], gt) in the case's storage layout."""
  layout = d['case'].layout
  ldis, imgs, gt = [], [], {}
  for side in ('src', 'trg'):
    v = d[side]
    tex, disp = T(v['tex'], dev), T(v['disp'], dev)
    if layout == 'permuted':    # channels-first storage viewed as L x B x H x W x 3
      tex = tex.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)
      assert tex.stride(4) == tex.shape[2] * tex.shape[3]
    elif layout == 'packed':    # stride-4 textures, the disparity channel 3 of the same buffer
      buf = torch.cat([tex, disp], dim=-1)
      tex, disp = buf[..., :3], buf[..., 3:4]
      assert tex.stride(3) == 4 and disp.data_ptr() == buf.data_ptr() + 12
    ldis.append([tex, None, disp])
    imgs.append(T(v['img'], dev))
    for k in ('gt_disp', 'gt_disp_bg', 'gt_tex_bg'):
      if v[k] is not None:
        gt[side + '_' + k] = T(v[k], dev)
  return ldis, imgs, gt


@pytest.mark.parametrize('case', R.LAYER_CASES, ids=_id)
def test_layer_metrics_lattice(case, dev):
  from lsi.nnutils import _hip_eval, eval_metrics
  d = R.layer_inputs(case)
  want, _ = R.layer_restate(d)
  ldis, imgs, gt = _layer_on_device(d, dev)
  assert ('src_gt_disp_bg' in gt) == case.bg
  opts = types.SimpleNamespace(bg_layer_disp=R.BG_LAYER_DISP)
  acc = eval_metrics.MetricAccumulator(dev)
  run = {k: (0.0, 0.0) for k in R.LAYER_KEYS}
  for call in range(3):
    acc.add_layer_prediction(ldis[0], ldis[1], imgs[0], imgs[1], gt, opts)
    run = {k: (run[k][0] + want[k][0], run[k][1] + want[k][1]) for k in run}
    got = acc.sums()
    for k in R.LAYER_KEYS:
      print('%s call %d %s: got %r, want %r' % (case.name, call, k, got[k], run[k]))
    for k in R.LAYER_KEYS:
      assert got[k] == run[k], (call, k)
    for k in R.VIEW_KEYS + ('psnr',):
      assert got[k] == (0.0, 0.0), k
    _check_results(acc, run)
  direct = torch.zeros((_hip_eval.SLOT_COUNT,), dtype=torch.float64, device=dev)
  ws, n = _hip_eval.workspace(dev)
  for call in range(3):
    _hip_eval.layer_metrics(direct, ws, n, ldis[0], ldis[1], imgs[0], imgs[1], gt,
                            R.BG_LAYER_DISP)
  assert torch.equal(direct, acc.acc)


def test_view_and_layer_metrics_share_one_accumulator(dev):
  from lsi.nnutils import eval_metrics
  vcase = next(c for c in R.VIEW_LATTICE if c.name == '7x37-f2x4')
  d, _, sums, want = _view_ref(vcase)
  ld = R.layer_inputs(R.LAYER_SMALL[3])
  lwant, _ = R.layer_restate(ld)
  ldis, imgs, gt = _layer_on_device(ld, dev)
  acc = eval_metrics.MetricAccumulator(dev)
  acc.add_layer_prediction(ldis[0], ldis[1], imgs[0], imgs[1], gt,
                           types.SimpleNamespace(bg_layer_disp=R.BG_LAYER_DISP))
  _add(acc, d, _on_device(d, dev))
  got = acc.sums()
  for k in R.VIEW_KEYS:
    assert got[k] == want[k], k
  for k in R.LAYER_KEYS:
    assert got[k] == lwant[k], k
  _check_psnr('shared accumulator', got['psnr'], sums)
  assert set(acc.results()) == set(ALL_KEYS)


# ---- dis-occlusion mask ------------------------------------------------------------------

@pytest.mark.parametrize('case', R.DISOCC_CASES, ids=_id)
def test_disocclusion_mask_lattice(case, dev):
  from lsi.geometry import projection
  from lsi.nnutils import _hip_eval
  d = R.disocc_inputs(case)
  args = (T(d['disps_src'], dev), T(d['disps_trg'], dev))
  mat = T(d['M'], dev)
  want = torch.from_numpy(d['mask'])
  got = _hip_eval.disocclusion_mask(*args, mat, d['thresh']).cpu()
  assert got.dtype == torch.float32 and got.shape == want.shape
  bad = (got != want).nonzero()
  assert torch.equal(got, want), '%d of %d pixels differ; first at %s: %s' % (
      len(bad), want.numel(), bad[0].tolist(),
      {k: float(v[tuple(bad[0][:3].tolist())]) for k, v in d['z'].items()})
  assert torch.equal(projection.disocclusion_mask(*args, None, mat, thresh=d['thresh'],
                                                  fused=True).cpu(), want)


def test_report(capsys):
  """Not a check: prints what the run measured (the bars are above)."""
  _view_ref.cache_clear()
  with capsys.disabled():
    for key in sorted(WORST):
      print('\neval lattice: worst %s: %.3f' % (key, WORST[key]), end='')
    print()
