"""What tests/fc_exact_ref.py promises, checked without a device: for every case
of tests/test_fc_exact_gpu.py,

  * the guards hold in both regimes and the fp32 products on the CPU equal the
    fp64 ones bit for bit (Z, dX, dW): the result does not depend on the
    summation order;
  * the case table reaches the structures it is there for, by the restated
    planner -- which equals the library's own for every case, through
    lsi_fc_workspace_bytes;
  * the geometry tuples are those the binding derives from the tensors;
  * the narrow regime sees a reference broken in each way these kernels could
    break;
  * the wide regime contains nearest-even ties;
  * the identity block in x gives dZ back from dW exactly, and the batch-norm
    operands leave at most 1 % of the (group, column) pairs undecided."""
import ctypes
import functools

import pytest
import torch

import fc_exact_ref as R

CASES = R.all_cases()
PAIRS = [(c, g) for c in CASES for g in R.regimes(c)]
_pid = lambda p: R.ident(p) if isinstance(p, R.Case) else str(p)


@functools.lru_cache(maxsize=None)
def _ref(case, regime):
  """(operands, fp64 reference): computed once, shared, never modified."""
  x, w, gy, junk = R.operands(case, regime)
  return (x, w, gy, junk), R.reference(case, x, w, gy, regime)


@pytest.mark.parametrize('case,regime', PAIRS, ids=_pid)
def test_guards_and_order_independence(case, regime):
  (x, w, gy, junk), (z64, dx64, dw64) = _ref(case, regime)    # (the guards: inside)
  assert set(x.unique().tolist()) <= {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
  z32, dx32, dw32 = x @ w.t(), gy @ w, gy.t() @ x
  assert z32.dtype == torch.float32
  assert torch.equal(z32.double(), z64)
  assert torch.equal(dx32.double(), dx64)
  assert torch.equal(dw32.double(), dw64)
  # the operands are bf16s, so the kernels' rounding on load changes nothing
  for t in (x, w, gy):
    assert torch.equal(t.bfloat16().float(), t)
  assert R.operands(case, regime)[1].equal(w) and not R.operands(case, regime, 1)[1].equal(w)


@pytest.mark.parametrize('case', CASES, ids=_pid)
def test_storage_and_geometry_agree_with_the_binding(case):
  """scatter / parameter / storage_of are inverse to each other, the elements the
  geometry addresses are distinct, and the tuple is the binding's own."""
  regime = R.regimes(case)[0]
  (x, w, gy, junk), _ = _ref(case, regime)
  flat = R.scatter(case, w, junk)
  p = R.parameter(case, flat)
  assert p.dtype == torch.float32
  assert R.lib_geometry(case, p) == R.geometry(case)
  assert torch.equal(R.storage_of(case, p), flat)
  k, n, taps, sn, sk, off = R.geometry(case)
  assert (k, n) == (case.k, case.n) and n % taps == 0 and (n // taps) % 8 == 0
  idx = R.addressed(case)
  assert torch.equal(flat[idx], w)
  # the (N, K) matrix as torch sees the parameter
  if case.layout.startswith('linear'):
    assert tuple(p.shape) == (n, k) and torch.equal(p, w)
  elif case.layout.startswith('convt'):
    centre = p[:, :, 1:3, 1:3].permute(2, 3, 1, 0).reshape(n, k)   # (oy, ox, cout), cin
    assert torch.equal(centre, w)
  else:
    assert any(o % 2 for o in off) and sum(o % 4 != 0 for o in off) >= 2
  # a gradient laid out like the parameter, as the binding allocates it
  assert torch.zeros_like(p).stride() == p.stride()
  assert torch.equal(R.storage_of(case, torch.zeros_like(p)), torch.zeros_like(flat))


def test_case_table_reaches_what_it_is_there_for():
  plans = {c: R.plan(c) for c in CASES}
  fwd = [p['fwd'] for p in plans.values()]
  dx = [p['dx'] for p in plans.values()]
  # a single partial step; exactly 17 steps in two chunks of unequal length
  assert any(c.k < 32 and plans[c]['fwd'].steps == 1 for c in CASES)
  assert any(p.steps == 17 and p.lengths == (9, 8) for p in fwd)
  assert any(p.steps == 17 and p.lengths == (9, 8) for p in dx)
  # a reduction with one step per wave at most, and one with a shorter last chunk of four
  assert any(1 < p.steps <= R.WAVES for p in fwd)
  assert any(p.chunks == 4 and p.lengths[-1] < p.per for p in fwd)
  assert any(p.chunks > 1 for p in dx)
  assert {p['mt'] for p in plans.values()} == {1, 2}
  assert {1, 16, 17, 32} <= {c.m for c in CASES} and any(c.m % 2 and c.m > 1 for c in CASES)
  # fc_dw_kernel: a lane block that is partial beyond the first, in both orientations
  for fast_n in (False, True):
    fs = [p['dw_fast'] for c, p in plans.items()
          if (R.geometry(c)[3] == 1 and R.geometry(c)[4] != 1) == fast_n]
    assert any(f > 256 and f % 256 for f in fs), fast_n
    assert any(f < 256 for f in fs), fast_n
  # one column tile wide; a half-full last tile; every layout; 2, 3 and 4 taps
  assert any(c.n <= 16 for c in CASES) and any(c.n % 16 == 8 and c.n > 16 for c in CASES)
  assert {c.layout for c in CASES} == set(R.LAYOUTS)
  assert {R.geometry(c)[2] for c in CASES} == {1, 2, 3, 4}
  assert {c.n // R.geometry(c)[2] for c in CASES if c.layout.startswith('taps')} == {8, 24}
  # the anchor is the largest network layer and runs the wide regime only
  assert R.ANCHOR[:3] == (8, 6144, 2000) and R.regimes(R.ANCHOR) == ('wide',)
  # batch norm: 3 rows per group, one row per group, MT = 2, a full-size run
  rows = {c.m // c.groups for c in R.BN_CASES}
  assert {1, 3} <= rows and any(c.m > 16 for c in R.BN_CASES)
  assert [(c.m, c.groups) for c in R.BN_CASES[:-1]] == R.BN_ROWS
  assert all((c.k, c.n) == (264, 520) for c in R.BN_CASES[:-1])
  assert R.BN_CASES[-1][:3] == (8, 2048, 2000)


@pytest.mark.parametrize('case', CASES + R.BN_CASES, ids=_pid)
def test_planner_restatement_equals_the_library(case, built_lib):
  from lsi import _C
  lib = _C.lib()
  p = R.plan(case)
  want = max(R.align256(p['fwd'].chunks * case.m * case.n * 4),
             R.align256(case.m * case.n * 2) + R.align256(p['dx'].chunks * case.m * case.k * 4))
  assert want == R.workspace_bytes(case)
  for flags in (0, _C.LSI_FC_X_F32 | _C.LSI_FC_OUT_F32):
    d = R.descriptor(case, flags)
    assert lib.lsi_fc_supported(ctypes.byref(d)) == 1
    assert lib.lsi_fc_workspace_bytes(ctypes.byref(d)) == want
  for pl in (p['fwd'], p['dx']):
    assert sum(pl.lengths) == pl.steps and len(pl.lengths) == pl.chunks
    assert all(0 < v <= pl.per for v in pl.lengths)


@pytest.mark.parametrize('how', sorted(R.BROKEN))
@pytest.mark.parametrize('case', R.CASES, ids=_pid)
def test_narrow_regime_sees_a_broken_reference(case, how):
  (x, w, gy, junk), (z64, dx64, _) = _ref(case, 'narrow')
  bad = R.BROKEN[how](case, x, w, gy, junk)
  if bad is None:
    assert how == 'rows 16.. zeroed' and case.m <= 16
    return
  for name, b, good in (('z', bad[0], z64), ('dx', bad[1], dx64)):
    assert b.shape == good.shape, name
    assert not torch.equal(b, good), name
    # ... also after the kernel's bf16 store
    assert not torch.equal(R.as_bf16(b), R.as_bf16(good)), name


def test_every_breakage_is_possible_somewhere():
  assert sum(c.m > 16 for c in R.CASES) >= 3
  assert sum(R.plan(c)['fwd'].chunks > 1 for c in R.CASES) >= 3


def test_wide_regime_fixes_the_rounding_of_ties():
  """257 lies midway between the bf16s 256 and 258: nearest-even gives 256, 259
  gives 260 -- and the wide regime does contain such ties, in Z and in dX."""
  t = torch.tensor([257.0, 259.0, -257.0, 1028.0, 1036.0], dtype=torch.float64)
  assert R.as_bf16(t).tolist() == [256.0, 260.0, -256.0, 1024.0, 1040.0]
  _, (z64, dx64, _) = _ref(R.lin(32, 1032, 1000), 'wide')
  for v in (z64, dx64):
    a = v.abs()
    ulp = torch.pow(2.0, torch.floor(torch.log2(a.clamp_min(1.0))) - 7)
    ties = (a >= 256) & (torch.remainder(a, ulp) == ulp / 2)
    assert int(ties.sum()) > 0
    assert not torch.equal(R.as_bf16(v).double(), v)      # (it does round)


def _dw_as_the_kernel_sums_it(dz, x):
  """fc_dw_kernel's arithmetic: for every (n, k) an fp32 fma chain over the rows
  in order, acc = fma(dz[m, n], x[m, k], acc).  (fp64 holds the product of two
  fp32 values and its sum with a third exactly enough: one rounding to fp32 per
  step, as the fma does -- the values here are bf16s, the products fp32s.)"""
  acc = torch.zeros(dz.shape[1], x.shape[1], dtype=torch.float32)
  for m in range(dz.shape[0]):
    acc = (dz[m].double()[:, None] * x[m].double()[None, :] + acc.double()).float()
  return acc


@pytest.mark.parametrize('case', [R.BN_CASES[2], R.BN_CASES[6]], ids=_pid)
def test_identity_block_gives_dz_back_from_dw(case):
  """With X[:, :M] = I, dW[n, k] = dZ[k, n] for k < M exactly, for ANY bf16 dZ:
  every other term of the sum is a product with zero."""
  x, w, gy, beta = R.bn_operands(case)
  assert torch.equal(x[:, :case.m], torch.eye(case.m))
  g = torch.Generator().manual_seed(11)
  dz = (torch.randn(case.m, case.n, generator=g) *
        torch.pow(2.0, torch.randint(-20, 20, (case.m, case.n), generator=g).float()))
  dz = dz.bfloat16().float()
  dw = _dw_as_the_kernel_sums_it(dz, x)
  assert torch.equal(dw[:, :case.m], dz.t())
  # ... and the other columns are not trivially that
  assert not torch.equal(dw[:, case.m:2 * case.m], dz.t())


@pytest.mark.parametrize('case', R.BN_CASES, ids=_pid)
def test_batch_norm_operands_leave_few_pairs_undecided(case):
  """The seeds of bn_operands: at most 1 % of the (group, column) pairs have a row
  with |v| within MARGIN E32 of the ReLU's kink (the GPU test leaves those pairs
  out and fails above 1 %)."""
  x, w, gy, beta = R.bn_operands(case)
  ref = R.bn_reference(case, x, w, gy, beta)
  assert torch.equal(ref['z'], ref['z'].round()) and float(ref['z'].abs().max()) < R.EXACT
  out = 1.0 - float(ref['decided'].double().mean())
  print('%s: %.4f %% of the pairs left out' % (R.ident(case), 100 * out))
  assert out <= 0.01
  e = R.dz_bound(ref)
  assert bool(torch.isfinite(e).all()) and bool((e > 0).any()) == (ref['rows'] > 1)
  if ref['rows'] == 1:
    assert float(ref['dz'].abs().max()) == 0.0 and torch.equal(ref['y'], ref['v'].clamp_min(0))
