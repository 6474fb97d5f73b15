"""tests/splat_lattice_ref.py held to its own claims, without a GPU:

* the NumPy restatement equals fp64 autograd of the reference op graph
  (lsi_torch_ref through test_disp_grad_gpu.oracle_splat: composed target
  disparity with amax) on every scene the GPU tests use, to 1e-12 of A;
* `wts` -- on every scene -- and every (scene, mode, quantity) in EXACT come out
  bit for bit the same in fp32 and fp64, from two fp32 evaluations that sum in
  different orders (NumPy scatter, torch index_add / autograd), and no sum of
  absolute terms reaches 2^24 units of its lattice step;
* the fp32 op graph's worst |g32 - g64| / A elsewhere is measured, printed and
  pinned (REF_RATIO: the GPU bound K is derived from it);
* each scene says something: overlaps between layers, every odd disparity,
  clamped border corners, crowded cells, empty cells."""
import functools

import numpy as np
import pytest
import torch

import splat_lattice_ref as R
import test_disp_grad_gpu as DG

MODES = ('layer', 'compose', 'both')


def _autograd(sc, G, dtype):
  """Outputs and gradients of the op graph; non-finite disparities (which the
  build defines as dropped) replaced by -1: weight 0, gradient 0."""
  disp = np.where(np.isfinite(sc.disp), sc.disp, -1.0)
  lv = {k: torch.tensor(v, dtype=dtype, requires_grad=True)
        for k, v in (('tex', sc.tex), ('disp', disp), ('M', sc.mat))}
  if sc.mask is not None:
    lv['mask'] = torch.tensor(sc.mask, dtype=dtype, requires_grad=True)
  loss, outs = 0, {}
  for compose, suffix in ((False, ''), (True, '_c')):
    o = DG.oracle_splat(lv['tex'], lv.get('mask'), lv['disp'], lv['M'], sc.s,
                        sc.bg_layer_disp, compose, sc.max_disp, sc.zbuf_scale)
    for n, t in zip(R.FWD_Q, o):
      outs[n + suffix] = t.detach().numpy()
      if n + suffix in G:
        loss = loss + (t * torch.tensor(G[n + suffix], dtype=dtype)).sum()
  if not G:
    return outs, {}
  loss.backward()
  return outs, {'g_' + k: v.grad.numpy() for k, v in lv.items()}


@functools.lru_cache(maxsize=None)
def _all(key, mode):
  sc = R.scene(*key)
  G = R.upstream(key, mode)
  f, g, A = R.evaluate(sc, G)
  return sc, G, f, g, A


def _ratio(err, A):
  """max err / (2^-24 A); where A = 0 the error must be 0."""
  assert (err[A == 0] == 0).all()
  return float((err[A > 0] / A[A > 0]).max()) * 2.0 ** 24 if (A > 0).any() else 0.0


ALL_CASES = sorted(set(R.small_cases() + R.stream_cases() + R.backward_cases()))


def test_every_kind_and_shape_of_the_issue_is_a_case():
  assert {c[0] for c in ALL_CASES} == set(R.KINDS)
  assert {c[1] for c in ALL_CASES} == set(R.SMALL_SHAPES + R.STREAM_SHAPES +
                                          R.BWD_STREAM_SHAPES)
  assert {c[2] for c in ALL_CASES if c[0] == 'quarter'} == {0.5, 1.0}
  for c in ALL_CASES:
    sc = R.scene(*c)
    for a in (sc.tex, sc.disp, sc.mat) + ((sc.mask,) if sc.mask is not None else ()):
      assert a.dtype == np.float32 and not a.flags.writeable
    assert sc.zbuf_scale == 0 and sc.max_disp == 0.5
    assert R.lattice_step(sc.tex) >= 1 / 8 and sc.tex.min() >= 0 and sc.tex.max() <= 1
    assert R.lattice_step(sc.disp[np.isfinite(sc.disp)]) >= 1 / 64
    assert R.lattice_step(sc.mat) >= 1 / 4
    if sc.mask is not None:
      assert set(np.unique(sc.mask)) <= {0.0, 0.125, 0.25, 0.5, 1.0, 2.0}


@pytest.mark.parametrize('case', ALL_CASES, ids=str)
def test_forward_equals_the_op_graph_and_wts_is_exact_in_fp32(case):
  sc = R.scene(*case)
  f = R.render(sc)
  outs, _ = _autograd(sc, {}, torch.float64)
  for n in ('img', 'wts', 'dsp', 'img_c', 'wts_c', 'dsp_c'):
    np.testing.assert_allclose(f[n], outs[n], rtol=1e-14, atol=0, err_msg=n)
  # fp32, two summation orders
  f32 = R.render(sc, np.float32)
  t32, _ = _autograd(sc, {}, torch.float32)
  for n in ('wts', 'wts_c'):
    assert f32[n].dtype == np.float32
    assert np.array_equal(f32[n].astype(np.float64), f[n]), n
    assert np.array_equal(t32[n].astype(np.float64), f[n]), n
  # every term a multiple of `step`, the sum of all of a cell's below 2^24 steps
  g = f['geom']
  upd = f['pw'][..., None] * g['w']
  step = R.lattice_step(np.concatenate([upd.ravel(), [f['bg']]]))
  assert step >= 2.0 ** -9                       # mask 1/8 x weight 1/64
  assert f['wts_c'].max() / step < 2.0 ** 24
  # every weight is 0 or far above the 1e-3 gate; every coordinate on the lattice
  w4 = g['w']
  assert (w4[w4 > 0] >= 1.0 / 64).all() and R.lattice_step(w4) >= 1.0 / 64
  assert R.lattice_step(g['u']) >= 1.0 / 8 and R.lattice_step(g['v']) >= 1.0 / 8
  # img, dsp: one rounding from the exact quotient
  for n in ('img', 'dsp', 'img_c', 'dsp_c'):
    err = np.abs(t32[n].astype(np.float64) - f[n])
    assert (err <= 2.0 ** -24 * np.abs(f[n])).all(), n


@pytest.mark.parametrize('case', R.backward_cases(), ids=str)
def test_gradients_equal_fp64_autograd_to_1e_12_of_A(case):
  for mode in MODES:
    sc, G, f, g, A = _all(case, mode)
    _, want = _autograd(sc, G, torch.float64)
    for n, w in want.items():
      assert g[n].shape == w.shape
      err = np.abs(g[n] - w)
      assert (err <= 1e-12 * A[n]).all(), (mode, n, _ratio(err, A[n]) * 2.0 ** -24)
      assert (np.abs(g[n]) <= A[n] * (1 + 1e-12)).all(), (mode, n)
    # a dropped pixel, and one whose four corners all left the target: exactly 0
    gone = ~f['geom']['ok'] | (f['geom']['w'].sum(-1) == 0)
    for n in ('g_tex', 'g_disp'):
      assert (g[n][gone] == 0).all(), (mode, n)


def test_the_exact_set_is_exact_in_fp32():
  """EXACT, claim by claim: fp32 (NumPy restatement and torch autograd, which
  sum in different orders) equals fp64 bit for bit, and the sum of the absolute
  terms of every element stays below 2^24 steps of the results' lattice."""
  seen = set()
  for case in ALL_CASES:
    for mode in MODES:
      sc = R.scene(*case)
      names = R.exact(sc, mode)
      if not names:
        continue
      seen.add((sc.kind, mode))
      G = R.upstream(case, mode)
      f, g, A = R.evaluate(sc, G)
      f32, g32, _ = R.evaluate(sc, G, np.float32)
      o32, t32 = _autograd(sc, G, torch.float32)
      suffix = {'layer': ('',), 'compose': ('_c',), 'both': ('', '_c')}[mode]
      for n in names:
        if n in ('img', 'dsp'):
          for sfx in suffix:
            assert np.array_equal(f32[n + sfx].astype(np.float64), f[n + sfx]), (case, mode, n)
            assert np.array_equal(o32[n + sfx].astype(np.float64), f[n + sfx]), (case, mode, n)
          can = f['CI'] if n == 'img' else f['CD']
          assert can.sum(0).max() / R.lattice_step(can) < 2.0 ** 24
        elif n in g and n in t32:
          assert g32[n].dtype == np.float32
          assert np.array_equal(g32[n].astype(np.float64), g[n]), (case, mode, n)
          assert np.array_equal(t32[n].astype(np.float64), g[n]), (case, mode, n)
          step = R.lattice_step(np.concatenate([g[n].ravel(), A[n].ravel()]))
          assert A[n].max() / step < 2.0 ** 24, (case, mode, n)
      # the weights the kernels take reciprocals of are powers of two
      for sfx in suffix:
        w = f['wts' + sfx]
        assert set(np.unique(w)) <= {1.0, 2.0, 4.0, 8.0}, (case, mode)
  assert seen == set(R.EXACT)


def test_fp32_op_graph_error_is_measured_and_pinned(capsys):
  """Worst |g32 - g64| / (2^-24 A) of the torch fp32 op graph over the
  backward cases and modes, per gradient: at most REF_RATIO, at least half
  of it (so that the pin cannot drift wide)."""
  worst = dict.fromkeys(R.GRAD_Q, 0.0)
  for case in R.backward_cases():
    for mode in MODES:
      sc, G, f, g, A = _all(case, mode)
      if R.GRAD_Q[0] in R.exact(sc, mode):
        continue
      _, g32 = _autograd(sc, G, torch.float32)
      for n, v in g32.items():
        worst[n] = max(worst[n], _ratio(np.abs(v.astype(np.float64) - g[n]), A[n]))
  with capsys.disabled():
    print('\nfp32 op graph, worst |g32 - g64| / (2^-24 A): ' +
          ', '.join('%s %.2f' % kv for kv in sorted(worst.items())))
  for n, v in worst.items():
    assert 0.5 * R.REF_RATIO[n] <= v <= R.REF_RATIO[n], (n, v, R.REF_RATIO[n])
    assert R.bound_k(n) <= 4 * R.REF_RATIO[n]


def test_each_scene_says_something():
  big = R.SMALL_SHAPES[0]

  def overlap(kind, s, mask=True):
    f = R.render(R.scene(kind, big, s, mask, 0))
    return float(((f['count'] > 0).sum(0) >= 2).mean()), f

  # cells that receive contributions from two different layers
  for kind, s, least in (('quarter', 1.0, 0.5), ('quarter', 0.5, 0.5), ('rowmix', 1.0, 0.5),
                         ('anypose', 1.0, 0.15), ('dropped', 1.0, 0.4),
                         ('crowded', 1.0, 0.02), ('shift_compose', 1.0, 0.5),
                         ('shift', 1.0, 0.3), ('no_background', 1.0, 0.2),
                         ('leaving', 1.0, 0.02)):
    share, f = overlap(kind, s, not kind.startswith('shift'))
    assert share >= least, (kind, s, share)
  # dropped: every odd value is there, and some cells are touched only by them
  sc = R.scene('dropped', big, 1.0, True, 0)
  d = sc.disp
  assert (d == 0).any() and (d < 0).any() and np.isnan(d).any()
  assert (d == np.inf).any() and (d == -np.inf).any() and (d > sc.max_disp).any()
  f = R.render(sc)
  assert (~f['geom']['ok']).sum() >= 3
  # (above max_disp is clamped, not dropped: weight exp(0) = 1)
  above = np.isfinite(d[..., 0]) & (d[..., 0] > sc.max_disp)
  assert (f['pw'][above] == sc.mask[..., 0][above]).all()
  # leaving: most pixels outside, some on column 0 with their left corner clamped
  sc = R.scene('leaving', big, 1.0, True, 0)
  f = R.render(sc)
  g = f['geom']
  assert (g['w'].sum(-1) == 0).mean() > 0.5
  x = g['u'] - 0.5
  clamped = (x > -1) & (x < 0) & (g['w'].sum(-1) > 0)
  assert clamped.sum() >= 1 and (g['w'][clamped][:, [0, 2]] == 0).all()
  assert (f['count'][..., 0] > 0).any()
  # crowded: 30 or more contributions in one cell
  assert R.render(R.scene('crowded', big, 1.0, True, 0))['count'].max() >= 30
  # no_background: empty cells weigh 0 and render exactly 0
  f = R.render(R.scene('no_background', big, 1.0, True, 0))
  empty = f['wts_c'] == 0
  assert f['bg'] == 0 and empty.mean() > 0.05 and (f['img_c'][empty[..., 0]] == 0).all()
  # the composed disparity has no near-ties (the kernels call a tie what is
  # within 2^-19 of the maximum): layers are tied exactly or clearly apart
  for case in R.backward_cases():
    f = R.render(R.scene(*case))
    gap = (f['dsp_c'] - f['dsp']) / np.maximum(np.abs(f['dsp_c']), 1e-30)
    assert ((gap == 0) | (gap > 2.0 ** -17)).all(), case
