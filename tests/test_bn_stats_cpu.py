"""The one-pass batch-norm statistics (convolution epilogue -> slots ->
lsi_bn_relu_norm, csrc/lsi_bn.hip: bn_norm_sums_kernel) emulated in NumPy fp32,
and the bound tests/test_bn_stats_gpu.py holds the device to:

    |rstd / rstd_ref - 1|  <=  2^-20 * (v + m^2) / (v + eps)  +  2^-22

Where the bound comes from.  The route forms var = E[y^2] - mean^2 from plain
fp32 sums.  E[y^2] = v + m^2 and mean^2 = m^2 each carry a relative error of a
few 2^-24 (tile sums, atomics into the slots, the fold, the multiplication by
1 / n), so var is off by a few 2^-24 * (v + m^2) in absolute terms, and
rstd = (var + eps)^-1/2 by half of that over (v + eps) in relative terms.
With k * 2^-24 on each of the two terms that is k * 2^-24 * (v + m^2) / (v + eps)
on rstd; the coefficient 2^-20 takes k = 16.  2^-22 covers the roundings of
the finish itself (var + eps, the square root, the division).
Nothing here is fitted to the device: this file keeps the derivation
executable, and shows that the arithmetic alone stays inside the bound with
about 2 x to spare on the channel distributions the GPU test builds (mean /
sigma from 0 to 100, sigma from 2^-6 to 2^3, outputs rounded to bf16)."""
import numpy as np
import pytest

EPS = 1e-3
RATIOS = (0.0, 1.0, 3.0, 10.0, 30.0, 100.0)


def rstd_bound(m, v, eps=EPS):
  """The numerical contract of the one-pass route (per channel; fp64 moments
  m, v of the stored tensor)."""
  return 2.0 ** -20 * (v + m * m) / (v + eps) + 2.0 ** -22


def bf16_round(a):
  """fp32 -> bf16 (round to nearest even) -> fp32."""
  u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
  u = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
  return u.view(np.float32)


def stat_slots(c):
  """lsi_bn_stat_slots (csrc/lsi_bn_ws.h)."""
  ns = 1
  while ns < 32 and 2 * ns * 2 * c <= 4096:
    ns *= 2
  return ns


def _fma(a, b, c):
  # (the product of two fp32 is exact in fp64; one more rounding to fp32)
  return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def slot_sums(y, ns, rng, tile=256):
  """What a producer leaves: y [npix, C] fp32 -> (S, Q) [ns, C] fp32.  A tile of
  `tile` pixels is summed as the epilogue does (16 sequential rows per lane, a
  tree over 16 lanes); tile f goes to slot f % ns, the tiles of a slot arrive
  in random order (device atomics)."""
  npix, c = y.shape
  ntile = -(-npix // tile)
  pad = np.zeros((ntile * tile, c), np.float32)     # (pixels outside the map add 0)
  pad[:npix] = y
  t = pad.reshape(ntile, tile // 16, 16, c)
  s = np.zeros((ntile, 16, c), np.float32)
  q = np.zeros((ntile, 16, c), np.float32)
  for r in range(tile // 16):
    s = s + t[:, r]
    q = _fma(t[:, r], t[:, r], q)
  w = 16
  while w > 1:
    w //= 2
    s = s[:, :w] + s[:, w:2 * w]
    q = q[:, :w] + q[:, w:2 * w]
  s, q = s[:, 0], q[:, 0]                           # [ntile, C]
  big_s = np.zeros((ns, c), np.float32)
  big_q = np.zeros((ns, c), np.float32)
  for sl in range(ns):
    members = np.arange(sl, ntile, ns)
    rng.shuffle(members)
    for f in members:
      big_s[sl] = big_s[sl] + s[f]
      big_q[sl] = big_q[sl] + q[f]
  return big_s, big_q


def fold_and_finish(big_s, big_q, npix, eps=EPS, threads=256, half=False):
  """bn_norm_sums_kernel: the fold of the slots and the fp32 finish.  `half`
  folds only half of the slots (a deliberately broken variant, for the test
  that the bound notices)."""
  ns, c = big_s.shape
  n2 = 2 * c
  acc = np.concatenate([big_s, big_q], axis=1)      # [ns, 2C]: slot sl at sl * 2C
  nfold = ns // 2 if half else ns
  if n2 <= threads:
    sstep = threads // n2
    part = np.zeros((sstep, n2), np.float32)
    for s0 in range(sstep):
      for sl in range(s0, nfold, sstep):
        part[s0] = part[s0] + acc[sl]
    tot = np.zeros((n2,), np.float32)
    for k in range(sstep):
      tot = tot + part[k]
  else:
    tot = np.zeros((n2,), np.float32)
    for sl in range(nfold):
      tot = tot + acc[sl]
  inv_n = np.float32(1.0 / float(npix))
  mean = tot[:c] * inv_n
  var = np.maximum(_fma(-mean, mean, tot[c:] * inv_n), np.float32(0.0))
  rstd = np.float32(1.0) / np.sqrt(var + np.float32(eps), dtype=np.float32)
  return mean, rstd


def emulate_one_pass(y, rng, eps=EPS, half=False):
  """y [npix, C] (values as stored) -> fp32 (mean, rstd) of the one-pass route."""
  y = np.ascontiguousarray(y, dtype=np.float32)
  big_s, big_q = slot_sums(y, stat_slots(y.shape[1]), rng)
  return fold_and_finish(big_s, big_q, y.shape[0], eps, half=half)


def reference(y, eps=EPS):
  yd = y.astype(np.float64)
  m = yd.mean(axis=0)
  v = yd.var(axis=0)
  return m, v, 1.0 / np.sqrt(v + eps)


def channels(c, npix, rng):
  """Conv-output-like channels: Gaussian (sums of many products), channel ch at
  mean / sigma = RATIOS[ch % 6], sigma = 2^(-6 ... 3), rounded to bf16."""
  ch = np.arange(c)
  ratio = np.asarray(RATIOS)[ch % len(RATIOS)]
  sigma = 2.0 ** (-6.0 + 9.0 * ((ch * 7) % c) / max(c - 1, 1))
  y = rng.standard_normal((npix, c), dtype=np.float32) * sigma.astype(np.float32) \
      + (ratio * sigma).astype(np.float32)
  return bf16_round(y), ratio


@pytest.mark.parametrize('npix,c', [(196608, 32), (786432, 32), (6144, 512), (193, 1024)])
def test_emulated_one_pass_rstd_stays_inside_the_bound_with_2x_to_spare(npix, c):
  rng = np.random.default_rng(npix + c)
  y, ratio = channels(c, npix, rng)
  m, v, rstd_ref = reference(y)
  mean, rstd = emulate_one_pass(y, rng)
  err = np.abs(rstd.astype(np.float64) / rstd_ref - 1.0)
  bound = rstd_bound(m, v)
  for r in RATIOS:
    sel = ratio == r
    print('npix %7d C %4d mean/sigma %5.0f: rstd error %.2e  bound %.2e' %
          (npix, c, r, err[sel].max(), bound[sel].min()))
  assert np.all(err <= 0.5 * bound), float((err / bound).max())
  assert np.all(np.abs(mean - m) <= 1e-5 * np.abs(y).max())
  # at mean ~ 0 the bound is the suite's older 2e-5, and the arithmetic meets it
  centred = ratio == 0.0
  assert float(bound[centred].max()) <= 2e-5 and float(err[centred].max()) <= 2e-5


def test_constant_and_dead_channels():
  """All-zero and constant channels: the sums are exact or nearly so, var comes
  out within rounding of 0 (clamped at 0), rstd within the bound of eps^-1/2."""
  rng = np.random.default_rng(5)
  y = np.zeros((20000, 32), np.float32)
  y[:, 1] = 7.0
  y[:, 2] = 300.0
  y[:, 3] = -0.0439453125
  m, v, rstd_ref = reference(y)
  _, rstd = emulate_one_pass(y, rng)
  assert np.all(np.isfinite(rstd))
  assert np.all(np.abs(rstd / rstd_ref - 1.0) <= rstd_bound(m, v))
  assert rstd[0] == np.float32(1.0) / np.sqrt(np.float32(EPS), dtype=np.float32)


def test_the_bound_notices_a_fold_over_half_the_slots():
  rng = np.random.default_rng(6)
  y, _ = channels(32, 50000, rng)
  m, v, rstd_ref = reference(y)
  _, rstd = emulate_one_pass(y, rng, half=True)
  assert np.any(np.abs(rstd / rstd_ref - 1.0) > rstd_bound(m, v))
