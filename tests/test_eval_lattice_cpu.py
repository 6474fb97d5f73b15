"""tests/eval_lattice_ref.py held to its own claims, without a device:

* view metrics, per lattice case: every cell's fp32 value equals its fp64
  value, the exactness condition (cells per thread x largest term / unit <
  2^24) holds and is printed, and fp32 sums per thread under random assignments
  of cells to threads give the fp64 total -- while 4096 cells per thread do not;
* the restatement agrees with the oracle's op-by-op restatement of the
  reference (oracle/lsi_oracle.py) on the lattice, where both are exact;
* the planted edges exist (counted and printed) and decide: a valid mask at
  `>=` 0.95, a minimum taken from layer 0, layer metrics with `>=`, each
  changes the answer;
* the three mutations of the view restatement -- a skipped cell past the grid,
  layer 0 for the minimum, the dis-occlusion block one column over -- each
  break an equality the GPU file demands;
* the dis-occlusion restatement equals the oracle's fp32 one on every pixel,
  its coordinates sit on the quarter-pixel lattice, and every planted edge is
  there with the mask depending on it."""
import math

import numpy as np
import pytest

import eval_lattice_ref as R
import lsi_oracle as O

_id = lambda c: c.name


def _show(capsys, text):
  with capsys.disabled():
    print('\n' + text, end='')


# ---- view metrics --------------------------------------------------------------------

@pytest.mark.parametrize('case', R.VIEW_LATTICE, ids=_id)
def test_view_lattice_is_exact_in_fp32(case, capsys):
  d = R.view_inputs(case)
  c64, c32 = R.view_cells(d, np.float64), R.view_cells(d, np.float32)
  assert np.array_equal(c64.centre, c32.centre)
  for k in R.VIEW_UNITS:
    assert c32.terms[k].dtype == np.float32
    assert np.array_equal(c32.terms[k].astype(np.float64), c64.terms[k]), k
  n = case.b * case.ht * case.wt
  cond = R.exactness(c64, n)
  assert all(v < 2.0 ** 24 for v in cond.values()), cond
  want = R.view_sums(c64)
  rs = np.random.RandomState(1)
  for k in R.VIEW_UNITS:
    for _ in range(3):
      assert R.fp32_thread_sums(c64.terms[k], n, rs) == want[k], k
  _show(capsys, 'eval lattice %s: %d cells, %d scored, %d per thread; condition (< %.3g): %s; '
        'planted %s' % (case.name, n, int(c64.centre.sum()), R.cells_per_thread(n), 2.0 ** 24,
                        ', '.join('%s %.3g' % kv for kv in cond.items()), d['planted']))


def test_the_condition_is_not_idle():
  """4096 squared-error terms in one fp32 sum lose bits: the condition is what
  keeps the lattice cases exact, not the lattice alone."""
  d = R.view_inputs(R.VIEW_WRAP[2])
  se = R.view_cells(d).terms['se']
  se = se[se > 0][:4096 * 32].reshape(-1, 4096)
  acc = np.zeros((se.shape[0],), np.float32)
  for j in range(4096):
    acc = acc + se[:, j].astype(np.float32)
  assert float(se.max()) / R.VIEW_UNITS['se'] * 4096 >= 2.0 ** 24
  assert math.fsum(acc.astype(np.float64).tolist()) != math.fsum(se.reshape(-1).tolist())


def test_view_cases_reach_what_they_are_for():
  by = {c.name: c for c in R.VIEW_LATTICE}
  cells = lambda c: c.b * c.ht * c.wt
  assert cells(by['wrap-512x1024']) == R.GRID_CELLS
  assert cells(by['wrap-3x1x174763']) == R.GRID_CELLS + 1
  assert cells(by['wrap-512x1152']) > R.GRID_CELLS
  assert all(cells(c) <= R.GRID_CELLS for c in R.VIEW_ROUNDED)
  assert R.grid_for(2 * 7 * 37) == 3 and (2 * 7 * 37) % R.TPB and 7 * 37 > R.TPB
  assert {(c.fy, c.fx) for c in R.VIEW_SMALL} >= set(R.LATTICE_FACTORS)
  assert {(c.fy, c.fx) for c in R.VIEW_ROUNDED} >= {(3, 3), (5, 5), (3, 2)}
  assert {c.nl for c in R.VIEW_SMALL} == {1, 2, 4}
  assert {c.disocc for c in R.VIEW_SMALL} == {None, 'f32', 'bool', 'u8', 'zero'}
  assert {c.layout for c in R.VIEW_SMALL} == {'plain', 'cfirst', 'rgba'}
  # the crops
  one = R.view_cells(R.view_inputs(by['crop-single-cell']))
  assert int(one.centre.sum()) == 1
  none = R.view_inputs(by['crop-nothing-left'])
  assert 2 * none['x_min'] >= 37 and not R.view_cells(none).centre.any()
  assert R.view_inputs(by['crop-0'])['x_min'] == 0
  assert R.view_inputs(by['7x37-f2x2'])['x_min'] == 4
  # exact ties between the layers, and cells whose best colour layer is not
  # their best disparity layer
  for name in ('7x37-f2x2', 'nl-4'):
    c = R.view_cells(R.view_inputs(by[name]))
    tied = (c.best_colour.sum(0) > 1) & c.centre
    tied_d = (c.best_disp.sum(0) > 1) & c.centre
    differ = c.centre & ~(c.best_colour & c.best_disp).any(0)
    assert tied.sum() > 10 and tied_d.sum() > 10 and differ.sum() > 10, name


@pytest.mark.parametrize('case', [c for c in R.VIEW_SMALL if c.valid != 'above'], ids=_id)
def test_view_restatement_equals_the_oracle_on_the_lattice(case):
  d = R.view_inputs(case)
  got = R.view_slots(d, R.view_sums(R.view_cells(d)))
  want = O.eval_view_synthesis_metrics(d['recons'], d['recons_disp'], d['target'], case.bdry,
                                       d['valid'], d['disocc'], d['gt_disp'])
  for k in R.VIEW_KEYS:
    assert got[k] == want.get(k, (0.0, 0.0)), k


def test_valid_edges_decide():
  by = {c.name: c for c in R.VIEW_LATTICE}
  for name, keys in (('7x37-f4x4', ('valid blocks with one zero element', 'valid blocks all ones')),
                     ('7x37-f1x1', ('valid == float32(0.95)', 'valid == its successor')),
                     ('valid-above-f4x4', ('blocks with a value == valid_above',)),
                     ('valid-above-f1x1', ('blocks with a value == valid_above',))):
    d = R.view_inputs(by[name])
    assert all(d['planted'][k] > 5 for k in keys), (name, d['planted'])
    centre = R.view_cells(d).centre
    crop = np.zeros_like(centre)
    crop[:, d['y_min']:by[name].ht - d['y_min'], d['x_min']:by[name].wt - d['x_min']] = True
    if d['valid_above'] is None:
      v = R._area(d['valid'], by[name].fy, by[name].fx, np.float32)[..., 0]
      # 15 of 16 and float32(0.95) are out, 16 of 16 and the successor are in
      edge = np.float32(0.9375) if by[name].fy == 4 else R.VALID_MIN
      assert ((v == edge) & crop).sum() > 3 and not (centre & (v == edge)).any()
      above = np.float32(1) if by[name].fy == 4 else np.nextafter(R.VALID_MIN, np.float32(1))
      assert (centre & (v == above)).sum() > 3
      assert (crop & (v >= R.VALID_MIN)).sum() > centre.sum() or by[name].fy == 4
    else:
      at = dict(d, valid_above=np.nextafter(np.float32(R.VALID_ABOVE), np.float32(0)))
      assert R.view_cells(at).centre.sum() > centre.sum()     # `>=` would let them in


@pytest.mark.parametrize('mutate,case', [('skip_cell', R.VIEW_WRAP[1]), ('skip_cell', R.VIEW_WRAP[2]),
                                         ('layer0', R.VIEW_SMALL[5]), ('dm_shift', R.VIEW_SMALL[5])],
                         ids=lambda v: v if isinstance(v, str) else v.name)
def test_mutating_the_restatement_breaks_an_equality(mutate, case):
  d = R.view_inputs(case)
  want = R.view_slots(d, R.view_sums(R.view_cells(d)))
  got = R.view_slots(d, R.view_sums(R.view_cells(d, mutate=mutate)))
  changed = [k for k in R.VIEW_KEYS if got[k] != want[k]]
  assert changed, mutate
  if mutate == 'skip_cell':       # one cell of 589 824: far inside the old 2e-4 bar
    assert got['compose_splat_loss'][1] == want['compose_splat_loss'][1] - 1
    assert abs(got['compose_splat_loss'][0] / want['compose_splat_loss'][0] - 1) < 1e-5
  if mutate == 'dm_shift':
    assert set(changed) == {'compose_splat_loss_disocc', 'depth_splat_loss_disocc'}


def test_psnr_reference():
  assert R.psnr_reference(0.0, 0.0) is None
  assert float(R.psnr_reference(0.0, 4.0)) == 200.0
  assert R.ulp_distance(10 * math.log10(1024.0), R.psnr_reference(2.0 ** -10, 1.0)) < 1
  want = R.psnr_reference(3.0, 7.0)
  assert R.ulp_distance(10 * math.log10(7.0 / 3.0), want) < 2
  assert 0.9 < R.ulp_distance(float(want) + math.ulp(float(want)), want) < 1.6


# ---- layer metrics ---------------------------------------------------------------------

@pytest.mark.parametrize('case', R.LAYER_CASES, ids=_id)
def test_layer_lattice(case, capsys):
  d = R.layer_inputs(case)
  want, worst = R.layer_restate(d)
  n = 2 * case.b * case.h * case.w
  cpt = R.cells_per_thread(n)
  assert all(cpt * v < 2.0 ** 24 for v in worst.values())
  got32, _ = R.layer_restate(d, dt=np.float32)
  assert got32 == want
  loose, _ = R.layer_restate(d, strict=False)
  planted = d['planted']
  assert planted['gt == bg_layer_disp'] >= 1 and (planted['gt == gt_bg'] >= 1 or n < 8)
  assert loose['fg_tex_error'] != want['fg_tex_error']
  if case.bg and n >= 8:
    assert loose['bg_tex_error'] != want['bg_tex_error']
    assert loose['bg_disp_error'][1] > want['bg_disp_error'][1]
  _show(capsys, 'eval lattice layer %s: 2 P = %d, %d per thread; largest term / unit %s; planted %s'
        % (case.name, n, cpt, dict(worst), planted))
  if case.bg:
    # the oracle divides each view's texture total by 3 and adds; the kernel adds, then
    # divides: the disparity sums and the normalisers are the same numbers
    f = lambda v: [[v['tex'], None, v['disp']], v['img']]
    (ls, im_s), (lt, im_t) = f(d['src']), f(d['trg'])
    gt = {s + '_' + k: d[s][k] for s in ('src', 'trg') for k in ('gt_disp', 'gt_disp_bg', 'gt_tex_bg')}
    o = O.eval_layer_prediction_metrics(ls, lt, im_s, im_t, gt, R.BG_LAYER_DISP)
    for k in ('fg_disp_error', 'bg_disp_error'):
      assert o[k] == want[k], k
    for k in ('fg_tex_error', 'bg_tex_error'):
      assert o[k][1] == want[k][1] and abs(o[k][0] - want[k][0]) <= 2 * math.ulp(want[k][0])


def test_layer_cases_reach_what_they_are_for():
  by = {c.name: c for c in R.LAYER_CASES}
  assert 2 * 5 * 77 > R.TPB * 3 and 5 * 77 % R.TPB and 5 * 77 // R.TPB == 2 * 5 * 77 // R.TPB // 2
  w = by['wrap-1x512x520']
  assert 2 * w.b * w.h * w.w > R.GRID_CELLS
  assert {c.L for c in R.LAYER_CASES} == {1, 2, 4}
  assert {c.layout for c in R.LAYER_CASES} == {'plain', 'permuted', 'packed'}
  assert not by['no-bg'].bg
  # 1 x 1 x 1: the source pixel is scored, the target one sits on bg_layer_disp
  d = R.layer_inputs(by['1x1x1-L1'])
  assert float(d['trg']['gt_disp'].reshape(())) == R.BG_LAYER_DISP
  assert R.layer_restate(d)[0]['fg_tex_error'][1] <= 1


# ---- dis-occlusion mask ------------------------------------------------------------------

@pytest.mark.parametrize('case', R.DISOCC_CASES, ids=_id)
def test_disocclusion_lattice(case, capsys):
  d = R.disocc_inputs(case)
  z = d['z']
  for k in ('u', 'v'):
    assert (z[k] * 4 == np.round(z[k] * 4)).all() and np.abs(z[k]).max() < 2 ** 12
  for k in ('dd', 'sampled', 'diff'):
    assert (z[k] * 4096 == np.round(z[k] * 4096)).all() and np.abs(z[k]).max() <= 1
  assert R.is_f32(d['M']) and R.is_f32(d['disps_trg'] * 256) and d['disps_trg'].max() <= 1
  assert (d['disps_trg'] * 256 == np.round(d['disps_trg'] * 256)).all()
  # the oracle's fp32 restatement of the op route, on every pixel
  assert np.array_equal(O.disocclusion_mask(d['disps_src'], d['disps_trg'], d['M'], d['thresh']),
                        d['mask'])
  _show(capsys, 'eval lattice disocclusion %s: %s' % (case.name, dict(d['planted'])))
  p = d['planted']
  if case.name == '5x77-onto-7x33':
    assert len(case.items) == 3 and p['negative-depth items'] == 1
    assert all(v >= 1 for v in p.values()), p
    assert 0.1 < p['mask == 1'] / p['pixels'] < 0.9
    # the edges decide: `>=` at the threshold, and `>=` in the truncation tests
    assert p['|dd - sampled| == thresh'] >= 5 and p['|dd - sampled| == thresh + 2^-8'] >= 5
    at = (z['diff'] == d['thresh']) & ~z['trunc']
    assert not d['mask'][..., 0][at].any()
    assert d['mask'][..., 0][(z['diff'] == d['thresh'] + 2.0 ** -8) & ~z['trunc']].all()
    on = ((z['u'] == 0) | (z['u'] == case.wt) | (z['v'] == 0) | (z['v'] == case.ht)) & ~z['trunc']
    assert d['mask'][..., 0][on & z['dis']].all()
  if case.name.startswith('ns-'):
    assert case.hs * case.ws == int(case.name[3:]) and p['|dd - sampled| == thresh'] >= 1


def test_disocclusion_cases_reach_what_they_are_for():
  assert {c.hs * c.ws for c in R.DISOCC_CASES} >= {1, 256, 257, 385}
  assert {it[0] for c in R.DISOCC_CASES for it in c.items} == {1.0, 2.0, 0.5, -1.0}
