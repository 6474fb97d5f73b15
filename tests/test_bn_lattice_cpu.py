"""tests/bn_lattice_ref.py held to its own claims, without a GPU:

* the scenes are what the module says (counted and printed): every value of d
  at exactly a quarter of the pixels, rstd a power of two, the sums inside
  fp32's exact range with the worst shift, z == 0 at a quarter of a channel's
  pixels in its owner group, bf16 ties towards both neighbours;
* the fp64 restatement equals fp64 autograd of torch.nn.functional.batch_norm
  + relu (relu'(0) = 0) to 1e-12 of A;
* on the exact set the formula run in fp32 under two associations equals fp64
  bit for bit;
* the fp32 op graph's worst |dx32 - dx64| / (2^-24 A) on the bounded set is
  measured, printed and pinned (REF_RATIO; K_BWD <= 4 x the pin);
* the scenes notice a dropped pixel, rotated group constants, z >= 0 as the
  backward's mask and a truncating bf16 store: the reference's own output,
  perturbed, breaks an equality in every case and dtype (no kernel is built)."""
import pytest
import torch
import torch.nn.functional as F

import bn_lattice_ref as R

CAP = R.CASES[-1]
SMALL = tuple(c for c in R.CASES if c != CAP)    # the scenes that are built here
_ids = lambda c: '-'.join(str(v) for v in c) if isinstance(c, tuple) else str(c)


def test_the_cases_are_what_the_exact_set_says(capsys):
  assert CAP == R.Case(256, 38916, 1) and CAP.npix == 16 * 2048 + 3 * 2048 + 4
  assert all(c.npix % 4 == 0 for c in R.CASES)
  assert {c.npix for c in R.exact_cases()} == {4, 64, 2048}
  assert {c.npix for c in R.bounded_cases()} == {260, 2052, 4100, 38916}
  assert {c.groups for c in R.CASES} >= {1, 2, 3}
  assert {c.lpp for c in R.CASES} == {1, 2, 16, 256}
  for case in R.CASES:
    for bf16 in (False, True):
      worst = R.assert_sums_fit(case, bf16)
      k = R.constants(case, bf16)
      assert float(k.m.abs().max()) <= 40 and set(k.var.unique().tolist()) <= {0.25, 3.25, 15.25}
      with capsys.disabled():
        print('\nbn lattice %s %s: |m| <= %d, largest sum %.3g lattice steps (2^24 = %.3g)'
              % (_ids(case), 'bf16' if bf16 else 'fp32', int(k.m.abs().max()), worst, 2.0 ** 24),
              end='')


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', SMALL, ids=_ids)
def test_scene_properties(case, bf16, capsys):
  sc = R.scene(case, bf16)
  k, n, G = sc.k, case.npix, case.groups
  x = sc.x.double()
  d = x - k.m[:, None]
  for v in (0.5, -0.5):
    want = torch.where(k.a == 0.5, n // 2, n // 4)       # (a = 0.5: +-a are +-0.5 again)
    assert torch.equal((d == v).sum(1), want)
  for s in (1.0, -1.0):
    assert bool(((d == s * k.a[:, None]).sum(1) >= n // 4).all())
  assert bool((sc.dy.abs() <= 8).all()) and R.is_fp32(sc.dy.double())
  assert bool((sc.dy == sc.dy.round()).all()) and float(sc.dy.abs().max()) == 8
  # the shifted sums with every value of the channel as the shift, from the tensor
  worst = 0.0
  for shift in (0.5, -0.5, k.a, -k.a):
    t = d - (shift[:, None] if torch.is_tensor(shift) else shift)
    assert bool((t * 2 == (t * 2).round()).all())
    worst = max(worst, float(t.abs().sum(1).max()) / 0.5, float((t * t).sum(1).max()) / 0.25)
  worst = max(worst, float((x * x).sum(1).max()) / 0.25)
  assert worst < 2.0 ** 24 and worst <= R.assert_sums_fit(case, bf16)
  for relu in (False, True):
    r = R.restate(sc, relu)
    assert torch.equal(r.mean, k.m) and torch.equal(r.rstd, k.rstd)       # dyadic, exact
    assert R.is_fp32(r.z) and R.is_fp32(r.xhat)
  # z == 0: a quarter (half at a = 0.5) of each channel's pixels in its owner
  # group, none elsewhere; the values next to the kink on both sides
  # (and in the groups that share the owner's a; nowhere else)
  own = torch.arange(len(sc.beta)) % G
  zero = (r.z == 0).sum(1)                                  # [G, C]
  plain = ~k.tie
  a_own = k.a[own, torch.arange(len(own))]
  want = torch.where(k.a == 0.5, n // 2, n // 4) * ((k.a == a_own) & plain)
  assert torch.equal(zero, want) and bool((want[own, torch.arange(len(own))][plain] > 0).all())
  near = r.z[:, :, plain]
  low, high = float(near[near > 0].min()), float(near[near < 0].max())
  assert low in (0.125, 0.25, 0.5) and -high in (0.125, 0.25, 0.5, 1.0)
  assert float(r.z[r.z != 0].abs().min()) >= 0.125 - 2.0 ** -6
  down, up = R.ties(r.z)
  with capsys.disabled():
    print('\nbn lattice %s %s: %d of %d elements at z == 0, nearest others %g and %g, bf16 ties '
          '%d down / %d up' % (_ids(case), 'bf16' if bf16 else 'fp32', int(zero.sum()),
                               r.z.numel(), high, low, down, up), end='')
  if bf16:
    assert down >= n // 4 and up >= n // 4
    assert bool(k.tie.any()) and bool((zero[:, k.tie] == 0).all())
  else:
    assert down == 0 and up == 0


@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', SMALL, ids=_ids)
def test_restatement_equals_fp64_autograd_of_batch_norm(case, bf16, relu):
  """The groups as further channels of one batch_norm call: the same beta in
  each, so its gradient comes out summed over the groups."""
  sc = R.scene(case, bf16)
  r = R.restate(sc, relu)
  G, n, C = sc.x.shape
  x = sc.x.double().permute(1, 0, 2).reshape(n, G * C).requires_grad_(True)
  beta = sc.beta.double().requires_grad_(True)
  ones = torch.ones(G * C, dtype=torch.float64)
  z = F.batch_norm(x, None, None, ones, beta.repeat(G), True, 0.0, R.EPS)
  y = torch.relu(z) if relu else z
  gx, gb = torch.autograd.grad(y, (x, beta), sc.dy.double().permute(1, 0, 2).reshape(n, G * C))
  back = lambda t: t.reshape(n, G, C).permute(1, 0, 2)
  assert float((back(y.detach()) - r.y).abs().max()) <= 1e-14
  assert torch.equal(back(y.detach()) == 0, r.y == 0)
  err = (back(gx) - r.dx).abs()
  assert bool((err <= 1e-12 * r.A).all()), float((err / r.A.clamp_min(1e-300)).max())
  assert bool((r.dx.abs() <= r.A * (1 + 1e-12)).all())
  assert torch.equal(gb, r.dbeta)


def _fp32_formula(sc, relu, assoc):
  """The op graph in fp32 torch, sums multiplied by (float)(1 / n) as the
  kernels do; assoc 0: (dz - c1) - xhat c2, 1: dz - (c1 + xhat c2)."""
  x, dy, beta = sc.x, sc.dy, sc.beta
  n = sc.case.npix
  inv = torch.tensor(1.0 / n, dtype=torch.float64).float()
  mean = x.sum(1) * inv
  var = ((x * x).sum(1) * inv - mean * mean).clamp_min(0)
  rstd = 1.0 / torch.sqrt(var + torch.tensor(R.EPS))
  xc = x - mean[:, None]
  xhat = xc * rstd[:, None]
  z = xhat + beta
  dz = dy * (z > 0) if relu else dy
  c1 = (dz.sum(1) * inv)[:, None]
  c2 = ((dz * xhat).sum(1) * inv)[:, None]
  t = (dz - c1) - xhat * c2 if assoc == 0 else dz - (c1 + xhat * c2)
  assert t.dtype == torch.float32
  return mean, rstd, (torch.relu(z) if relu else z), rstd[:, None] * t


@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', [c for c in R.exact_cases()], ids=_ids)
def test_the_exact_set_is_exact_in_fp32(case, bf16, relu):
  sc = R.scene(case, bf16)
  r = R.restate(sc, relu)
  R.assert_backward_is_fp32(r)
  for assoc in (0, 1):
    mean, rstd, y, dx = _fp32_formula(sc, relu, assoc)
    assert torch.equal(mean.double(), r.mean) and torch.equal(rstd.double(), r.rstd)
    assert torch.equal(y.double(), r.y) and torch.equal(dx.double(), r.dx)


def test_fp32_op_graph_error_is_measured_and_pinned(capsys):
  """Worst |dx32 - dx64| / (2^-24 A) of the fp32 formula over the bounded
  scenes built here, both associations: at most REF_RATIO, at least half of it
  (the pin cannot drift wide); K_BWD at most 4 x the pin.  The fp32 formula
  forms mean and rstd from one-pass sums here; where those are off, the ReLU
  mask of a z == 0 element is open: the backward is measured on its own, from
  the exact mean and rstd, as lsi_bn_relu_bwd gets them."""
  worst, differ, runs = 0.0, 0, 0
  for case in R.bounded_cases():
    if case == CAP:
      continue
    inv = torch.tensor(1.0 / case.npix, dtype=torch.float64).float()
    for bf16 in (False, True):
      sc = R.scene(case, bf16)
      for relu in (False, True):
        r = R.restate(sc, relu)
        xhat, dz = r.xhat.float(), r.dz.float()
        c1 = (dz.sum(1) * inv)[:, None]
        c2 = ((dz * xhat).sum(1) * inv)[:, None]
        for assoc in (0, 1):
          t = (dz - c1) - xhat * c2 if assoc == 0 else dz - (c1 + xhat * c2)
          dx = r.rstd.float()[:, None] * t
          err = (dx.double() - r.dx).abs()
          assert bool((err[r.A == 0] == 0).all())
          worst = max(worst, float((err / r.A.clamp_min(1e-300))[r.A > 0].max()) / R.U)
          differ += int(not torch.equal(dx.double(), r.dx))
          runs += 1
  with capsys.disabled():
    print('\nbn lattice: fp32 op graph, worst |dx32 - dx64| / (2^-24 A) on the bounded scenes: '
          '%.2f (pin %.2f, K %.1f); %d of %d runs differ from fp64' %
          (worst, R.REF_RATIO, R.K_BWD, differ, runs))
  assert 0.5 * R.REF_RATIO <= worst <= R.REF_RATIO
  assert R.K_BWD <= 4 * R.REF_RATIO
  assert differ > 0           # (the split between the exact and the bounded set is real)


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', SMALL, ids=_ids)
def test_the_scenes_notice_what_a_kernel_could_get_wrong(case, bf16):
  """Each perturbation of the reference's own output changes at least one
  stored value of every quantity it reaches, in this case and dtype.  (A
  truncating store exists in bf16 only: fp32 results are stored as they are.)"""
  sc = R.scene(case, bf16)
  st = lambda t: R.stored(t, bf16)
  for relu in (False, True):
    r = R.restate(sc, relu)
    drop = R.restate(sc, relu, drop_pixel=True)
    for name in ('mean', 'rstd', 'y', 'dx'):
      a, b = getattr(r, name), getattr(drop, name)
      assert not torch.equal(a.float(), b.float()), ('dropped pixel', name)
      if name in ('y', 'dx'):
        assert not torch.equal(st(a), st(b)), ('dropped pixel', name)
    if case.groups > 1:
      swap = R.restate(sc, relu, swap_groups=True)
      # (every group's constants are its neighbour's: every group is wrong)
      for g in range(case.groups):
        assert not torch.equal(st(r.y[g]), st(swap.y[g])), ('swapped', g)
        assert not torch.equal(st(r.dx[g]), st(swap.dx[g])), ('swapped', g)
  ge = R.restate(sc, True, mask_ge=True)
  assert torch.equal(ge.y, r.y)
  assert not torch.equal(st(ge.dx), st(r.dx)) and not torch.equal(ge.dbeta, r.dbeta)
  if bf16:
    for relu in (False, True):
      r = R.restate(sc, relu)
      assert not torch.equal(R.truncated(r.y), st(r.y))
      assert not torch.equal(R.truncated(r.dx), st(r.dx))
