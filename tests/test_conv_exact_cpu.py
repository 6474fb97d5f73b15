"""What tests/conv_exact_ref.py promises, checked without a device: for every
case of tests/test_conv_exact_gpu.py, in both regimes,

  * the guards hold (narrow: every output and data gradient at most 256, exactly
    a bf16; everything, the weight gradient included, below 2^24; sum y^2 below
    2^24 where the statistics are checked);
  * the fp32 convolution of the operands on the CPU equals the fp64 one bit for
    bit, forward and both gradients: the result does not depend on the summation
    order, which is the whole point of integer operands;
  * the narrow regime sees a reference broken in each of the ways these kernels
    break: one dropped term at an image corner, one tap shifted by a pixel on the
    last column, one chunk of 32 input channels skipped."""
import functools

import pytest
import torch

import conv_exact_ref as R

CASES = R.all_cases()
_ids = lambda c: '-'.join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def _ref(case, regime):
  """(operands, fp64 reference): computed once, shared, never modified."""
  x, w, gy = R.operands(case, regime)
  return (x, w, gy), R.reference(case, x, w, gy, regime, groups=R.stats_groups(case))


def test_generator_density_and_values():
  g = torch.Generator().manual_seed(1)
  t = R.ints((64, 64, 16), 0.25, 2, g)
  assert t.dtype == torch.float32
  assert set(t.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
  assert abs(float((t != 0).float().mean()) - 0.25) < 0.01
  t = R.ints((64, 64, 16), 1.0, 3, g)
  assert set(t.unique().tolist()) == {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
  # ... each value as often as the others, and the same tensor from the same seed
  assert abs(float((t == 3).float().mean()) - 1.0 / 6) < 0.01
  a = R.operands(CASES[0], 'narrow')
  b = R.operands(CASES[0], 'narrow')
  assert all(torch.equal(p, q) for p, q in zip(a, b))
  assert not torch.equal(a[0], R.operands(CASES[0], 'narrow', seed=1)[0])


def test_same_padding_is_tensorflows():
  assert R.same_pads(12, 5, 2) == (1, 2, 6) and R.same_pads(11, 5, 2) == (2, 2, 6)
  assert R.same_pads(8, 3, 2) == (0, 1, 4) and R.same_pads(7, 3, 2) == (1, 1, 4)
  assert R.same_pads(9, 7, 1) == (3, 3, 9) and R.same_pads(9, 7, 2) == (3, 3, 5)


@pytest.mark.parametrize('regime', R.REGIMES)
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_guards_and_order_independence(case, regime):
  (x, w, gy), (y64, gx64, gw64) = _ref(case, regime)   # (the guards: inside)
  # integers throughout
  for t in (y64, gx64, gw64):
    assert torch.equal(t, t.round())
  xf, wf = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
  y32 = R.forward(case, xf, wf)
  gx32, gw32 = torch.autograd.grad(y32, (xf, wf), gy)
  assert y32.dtype == torch.float32
  assert torch.equal(y32.detach().double(), y64)
  assert torch.equal(gx32.double(), gx64)
  assert torch.equal(gw32.double(), gw64)


@pytest.mark.parametrize('how', sorted(R.BROKEN))
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_narrow_regime_sees_a_broken_reference(case, how):
  (x, w, gy), (y64, _, _) = _ref(case, 'narrow')
  bad = R.BROKEN[how](case, x, w, y64)
  assert bad.shape == y64.shape
  assert not torch.equal(bad, y64)
  # ... also after the kernel's store: every value is still exactly a bf16, or
  # rounds to something else than the right one
  assert not torch.equal(R.as_bf16(bad), R.as_bf16(y64))
  if how == 'dropped term':
    assert int((bad != y64).sum()) == 1       # one product, one output value


def test_wide_regime_fixes_the_rounding_of_ties():
  """257 lies midway between the bf16s 256 and 258: nearest-even gives 256, 259
  gives 260 -- and the wide regime does contain such ties."""
  t = torch.tensor([257.0, 259.0, -257.0, 1028.0, 1036.0], dtype=torch.float64)
  assert R.as_bf16(t).tolist() == [256.0, 260.0, -256.0, 1024.0, 1040.0]
  (_, _, _), (y64, _, _) = _ref(R.IGEMM[11], 'wide')
  a = y64.abs()
  ulp = torch.pow(2.0, torch.floor(torch.log2(a.clamp_min(1.0))) - 7)
  ties = (a >= 256) & (torch.remainder(a, ulp) == ulp / 2)
  assert int(ties.sum()) > 0
