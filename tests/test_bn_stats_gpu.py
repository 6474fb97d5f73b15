"""Batch-norm statistics on off-centre, mixed-scale activations (csrc/lsi_bn.hip
and the convolution epilogues that leave the sums for lsi_bn_relu_norm).

Every comparison is against fp64 on the SAME stored tensor (the bf16 / fp32
values the kernel reads, up-cast): torch.nn.functional.batch_norm in fp64 with
autograd, fp64 mean / var(unbiased=False).

The one-pass route (sums of y and y^2 in fp32, var = E[y^2] - mean^2) is held
to the contract derived in tests/test_bn_stats_cpu.py,

    |rstd / rstd_ref - 1|  <=  2^-20 * (v + m^2) / (v + eps) + 2^-22,

the two-pass route (sums around a per-channel shift, fp64 finish) to the
suite's older rtol 2e-5 at every mean / sigma."""
import pytest
import torch
import torch.nn.functional as F

from test_bn_stats_cpu import EPS, RATIOS, rstd_bound, stat_slots

pytestmark = pytest.mark.gpu

# csrc/lsi_bn_ws.h: the workspace per group, in floats
WS_ACC, WS_TAG, WS_STRIDE = 16, 1, 16 + 4096 + 3 * 2048
LSI_EINVAL = -1


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def _clast(t):
  return t.contiguous(memory_format=torch.channels_last)


def _same_pads(size, k, s):
  """TF `SAME`: (before, after, out)."""
  out = -(-size // s)
  total = max((out - 1) * s + k - size, 0)
  return total // 2, total - total // 2, out


def _beta(c, g, dev):
  """0.3 * randn, kept 0.05 away from 0: a dead or constant channel's
  pre-activation IS beta at every pixel, and within rounding of 0 its whole ReLU
  mask would be undecided."""
  b = torch.randn((c,), generator=g) * 0.3
  return (torch.sign(b) * (b.abs() + 0.05)).to(dev)


def _bn_ref(x, beta, groups, relu=True, eps=EPS):
  """fp64 reference on the stored tensor: (z, leaf x, leaf beta)."""
  n, c, h, w = x.shape
  xr = x.detach().double().requires_grad_(True)
  br = beta.detach().double().requires_grad_(True)
  ones = torch.ones(c, dtype=torch.float64, device=x.device)
  if (n // groups) * h * w > 1:
    bn = lambda xc: F.batch_norm(xc, None, None, ones, br, True, 0.0, eps)
  else:     # (F.batch_norm refuses one value per channel: the same formula by hand)
    bn = lambda xc: (xc - xc.mean(dim=(0, 2, 3), keepdim=True)) / torch.sqrt(
        xc.var(dim=(0, 2, 3), unbiased=False, keepdim=True) + eps) + br.view(1, c, 1, 1)
  zs = [bn(xc) for xc in xr.chunk(groups, 0)]
  z = torch.cat(zs, 0)
  return (torch.relu(z) if relu else z), xr, br


def _moments(x, groups):
  n, c, h, w = x.shape
  xf = x.detach().double().view(groups, n // groups, c, h, w)
  return xf, xf.mean(dim=(1, 3, 4)), xf.var(dim=(1, 3, 4), unbiased=False)


def _figures(tag, m, v, err, bound):
  """One line per decade of mean / sigma: the worst error and the bound there
  (printed before anything is asserted: pytest -s shows the measurement)."""
  ratio = (m.abs() / torch.sqrt(v + 1e-30)).flatten()
  err, bound = err.flatten(), bound.flatten()
  for lo, hi in ((0, 0.3), (0.3, 3), (3, 30), (30, 300), (300, 3000), (3000, float('inf'))):
    sel = (ratio >= lo) & (ratio < hi)
    if bool(sel.any()):
      i = int(torch.argmax(torch.where(sel, err / bound, torch.full_like(err, -1.0))))
      print('BNSTAT %-38s mean/sigma [%g, %g): channels %4d  rstd error %.2e  bound %.2e' %
            (tag, lo, hi, int(sel.sum()), float(err[i]), float(bound[i])))


def _check_forward(tag, y, z, mr, beta, groups, relu=True, one_pass=True):
  """mean / rstd (the tensor saved for the backward) and the activations."""
  n, c, h, w = y.shape
  yf, m, v = _moments(y, groups)
  rstd_ref = torch.rsqrt(v + EPS)
  err = (mr[:, 1].double() / rstd_ref - 1.0).abs()
  bound = rstd_bound(m, v) if one_pass else torch.full_like(v, 2e-5)
  _figures(tag, m, v, err, bound)
  ymax = float(yf.abs().max())
  mean_err = float((mr[:, 0].double() - m).abs().max())
  print('BNSTAT %-38s mean error %.2e (allowed %.2e)' % (tag, mean_err, 1e-5 * ymax))
  assert mean_err <= 1e-5 * ymax
  assert bool((err <= bound).all()), float((err / bound).max())
  e = lambda t: t.view(groups, 1, c, 1, 1)
  xhat = (yf - e(m)) * e(rstd_ref)
  pre = xhat + beta.detach().double().view(1, 1, c, 1, 1)
  z_ref = torch.relu(pre) if relu else pre
  zd = z.detach().double().view_as(z_ref)
  rounding = 2.0 ** -8 if y.dtype == torch.bfloat16 else 2.0 ** -22
  tol = rounding * z_ref.abs() + xhat.abs() * e(bound) + 1e-5
  over = (zd - z_ref).abs() - tol
  print('BNSTAT %-38s activations: worst error - allowed %.2e' % (tag, float(over.max())))
  assert float(over.max()) <= 0.0
  if relu:
    assert float(((zd > 0) != (z_ref > 0)).float().mean()) < 1e-3
  return m, v


def _check_backward(y, beta, groups, gz, gy, gb, relu=True):
  """dx and dbeta of the fused op against fp64 autograd, away from the ReLU's
  kink (tests/test_train_gpu.py: the mask of an element within rounding of 0 is
  decided by the last bit of the statistics).  Returns the reference dy."""
  bf16 = y.dtype == torch.bfloat16
  grad_tol = 3e-2 if bf16 else 2e-4
  z_ref, yr, br = _bn_ref(y, beta, groups, relu)
  z_ref.backward(gz.double())
  assert bool(torch.isfinite(gy.float()).all()) and bool(torch.isfinite(gb).all())
  err = (gy.double() - yr.grad).abs()
  gs = float(yr.grad.abs().max()) + 1e-12
  bs = float(br.grad.abs().max()) + 1e-12
  if relu:
    with torch.no_grad():
      pre, _, _ = _bn_ref(y, beta, groups, False)
      kink = pre.abs() < (2e-2 if bf16 else 1e-5)
    assert float(kink.float().mean()) < 2e-2
    slack = (gz.double().abs() * kink).sum(dim=(0, 2, 3))
    err = err[~kink]
  else:
    slack = 0.0
  assert float(err.max()) <= grad_tol * gs, (float(err.max()), grad_tol * gs)
  assert bool(((gb.double() - br.grad).abs() <= grad_tol * bs + slack).all())
  return yr.grad


# ---- 1. one-pass statistics per producer --------------------------------------------

def _activations(n, c, h, w, a, g, dev):
  """Post-ReLU-like: relu(randn + a), bf16; channel 0 a constant plane of ones."""
  x = torch.relu(torch.randn((n, c, h, w), generator=g) + a)
  x[:, 0] = 1.0
  return _clast(x.to(dev).to(torch.bfloat16))


def _weights(cout, cin, kh, kw, taps, ex, sx, g, per_pixel=None):
  """[cout, cin, kh, kw]: zero-mean noise (zero-sum over the input channels, so
  that the inputs' common offset cancels at every pixel, padded borders
  included) times a per-channel scale 2^-6 ... 2^3, plus a per-channel offset on
  `taps` -- the taps that read a real pixel at every output position, so that
  the offset adds the same amount everywhere.  Output channel ch comes out near
  mean / sigma = RATIOS[ch % 6].  ex, sx: mean and spread of the inputs.
  per_pixel: the taps one output pixel reads (kh * kw; 4 of the 16 for the
  transposed convolution).  Output channel 0 is dead (all-zero weights); output
  channel 1 reads only the constant input plane: the constant 7."""
  ch = torch.arange(cout)
  ratio = torch.tensor(RATIOS)[ch % len(RATIOS)]
  sigma = 2.0 ** (-6.0 + 9.0 * ((ch * 7) % cout).double() / (cout - 1))
  big_r = cin ** 0.5 * ex / sx            # mean / sigma of a pure-offset channel
  m = ratio * sigma / torch.sqrt(torch.clamp(1.0 - (ratio / big_r) ** 2, min=0.1))
  wn = torch.randn((cout, cin, kh, kw), generator=g).double()
  wn[:, 0] = 0.0                                   # (the constant plane)
  wn[:, 1:] -= wn[:, 1:].mean(dim=1, keepdim=True)
  wt = wn * (sigma / ((cin * (per_pixel or kh * kw)) ** 0.5 * sx)).view(-1, 1, 1, 1)
  for ky, kx in taps:
    wt[:, :, ky, kx] += (m / (cin * ex)).view(-1, 1)
  wt[0] = 0.0
  wt[1] = 0.0
  for ky, kx in taps:
    wt[1, 0, ky, kx] = 7.0
  return wt.float()


def _coverage(tag, m, v):
  """The case does cover what it is for: centred and far-off-centre channels,
  variances far below and far above eps, a dead and a constant channel."""
  live = v > 0
  ratio = m.abs() / torch.sqrt(v + 1e-30)
  print('BNSTAT %-38s mean/sigma %.2g ... %.3g, var %.2g ... %.3g' % (
      tag, float(ratio[live].min()), float(ratio[live].max()), float(v[live].min()),
      float(v.max())))
  assert float(ratio[live].min()) < 0.5 and float(ratio[live].max()) > 50.0
  assert float(v[live].min()) < 0.5 * EPS and float(v.max()) > 10.0
  assert bool((v[:, 0] == 0).all()) and bool((m[:, 0] == 0).all())          # dead
  assert bool((v[:, 1] == 0).all()) and bool(((m[:, 1] - 7.0).abs() < 1e-12).all())   # constant


# (producer, n, cin, h, w, cout, k, stride, groups)
_PRODUCERS = [
    ('conv', 4, 32, 37, 53, 32, 3, 1, 2),         # 32 slots; odd sizes
    ('conv', 2, 64, 40, 66, 512, 5, 2, 1),        # 2 slots; TF's asymmetric padding
    ('conv', 8, 32, 128, 384, 32, 7, 1, 2),       # 196 608 pixels per group
    ('conv', 4, 256, 6, 10, 1024, 3, 1, 2),       # 2 slots, 1024 channels
    ('cat', 2, 96, 21, 37, 64, 3, 1, 2),          # 64 + 32 input channels
    ('convt', 4, 64, 9, 13, 32, 4, 2, 2),
    ('convt', 2, 128, 16, 24, 512, 4, 2, 1),
    ('first', 8, 3, 256, 768, 32, 7, 2, 2),       # 196 608 pixels per group
    ('first', 3, 3, 37, 91, 32, 7, 2, 3),
    ('splitk', 8, 512, 8, 24, 512, 3, 1, 2),      # _SPLITK_CASES of test_conv_gpu.py
    ('splitk', 2, 256, 16, 48, 512, 3, 2, 2),
    ('splitk', 4, 256, 6, 10, 1024, 3, 1, 2),     # the fold over 1024 channels, 2 slots
]


def _produce(case, dev, g):
  """-> (run(bn_groups) -> y, the input that gets a gradient or None, the fp32
  convolution of that input)."""
  import ctypes
  from lsi import _C
  from lsi.nnutils import _hip_conv
  kind, n, cin, h, w, cout, k, s, groups = case
  a = max(150.0 / cin ** 0.5, 3.0)
  if kind == 'first':
    # a bright low-contrast image: mean 1, spread 0.04 / sqrt(12)
    img = 1.0 + 0.04 * (torch.rand((n, h, w, 3), generator=g) - 0.5)
    img[..., 0] = 1.0
    x = img.to(dev).permute(0, 3, 1, 2)
    pt, pb, oh = _same_pads(h, 7, 2)
    pl, pr, ow = _same_pads(w, 7, 2)
    wt = _weights(cout, 3, 7, 7, [(pt, pl)], 1.0, 0.04 / 12 ** 0.5, g).to(dev).requires_grad_(True)
    assert _hip_conv.first_supported(x, 3, cout, 7, 2)
    run = lambda bn: _hip_conv.conv2d_first(x, wt, 2, pt, pl, oh, ow, bn)
    return run, None, None
  if kind == 'convt':
    x = _activations(n, cin, h, w, a, g, dev).requires_grad_(True)
    wt = _weights(cout, cin, 4, 4, [(1, 1), (1, 2), (2, 1), (2, 2)], a, 1.0, g, 4)
    wt = wt.permute(1, 0, 2, 3).contiguous().to(dev)          # cin x cout x 4 x 4
    assert _hip_conv.convt_supported(x, cin, cout, 4, 2)
    run = lambda bn: _hip_conv.conv_transpose2d(x, wt, 2, 1, bn)
    ref = lambda xf: F.conv_transpose2d(xf, wt.to(torch.bfloat16).float(), None, 2, 1)
    return run, x, ref
  pt, pb, oh = _same_pads(h, k, s)
  pl, pr, ow = _same_pads(w, k, s)
  x = _activations(n, cin, h, w, a, g, dev).requires_grad_(True)
  wt = _weights(cout, cin, k, k, [(pt, pl)], a, 1.0, g).to(dev)
  ref = lambda xf: F.conv2d(F.pad(xf, (pl, pr, pt, pb)), wt.to(torch.bfloat16).float(), None, s)
  if kind == 'cat':
    c1 = 2 * cin // 3
    x1 = _clast(x.detach()[:, :c1]).requires_grad_(True)
    x2 = _clast(x.detach()[:, c1:])
    assert _hip_conv.cat_supported(x1, x2, cout, k, s)
    run = lambda bn: _hip_conv.conv2d_cat(x1, x2, wt, s, pt, pl, oh, ow, bn)
    ref1 = lambda xf: ref(torch.cat([xf, x2.float()], 1))
    return run, x1, ref1
  assert _hip_conv.igemm_supported(x, cin, cout, k, s)
  d = _hip_conv._conv_desc(n, h, w, cin, oh, ow, cout, k, k, s, pt, pl)
  if kind == 'splitk':       # (the launch does split; the others run with SPLITK off)
    assert _hip_conv.SPLITK and int(_C.lib().lsi_conv2d_workspace_bytes(ctypes.byref(d), 0)) > 0
  run = lambda bn: _hip_conv.conv2d(x, wt, s, pt, pl, oh, ow, bn)
  return run, x, ref


@pytest.mark.parametrize('case', _PRODUCERS, ids=lambda c: '-'.join(str(v) for v in c))
def test_one_pass_statistics_per_producer(case, dev, monkeypatch):
  """Every producer of the sums (tile epilogue, split-K fold, transposed
  convolution, first layer, two-tensor input) on post-ReLU-like inputs whose
  output channels cover mean / sigma 0 ... 100 and sigma^2 far below ... far
  above eps, with a dead and a constant channel: mean, rstd (the contract),
  activations, gradients; and the two-pass route on the same tensor at rtol
  2e-5."""
  from lsi.nnutils import _hip_bn, _hip_conv
  monkeypatch.setattr(_hip_conv, 'SPLITK', case[0] == 'splitk')
  g = torch.Generator().manual_seed(41)
  groups, cout = case[8], case[5]
  tag = '%s-k%ds%d-c%d-%dx%dx%d' % (case[0], case[6], case[7], cout, case[1], case[3], case[4])
  run, x, ref = _produce(case, dev, g)
  beta = _beta(cout, g, dev).requires_grad_(True)
  y0 = run(0)
  y1 = run(groups)
  assert torch.equal(y1, y0)
  z1 = _hip_bn.batch_norm_relu(y1, beta, EPS, True, groups, True)
  mr = z1.grad_fn.saved_tensors[2].clone()
  m, v = _check_forward(tag, y1, z1, mr, beta, groups)
  _coverage(tag, m, v)
  gz = _clast(torch.randn(z1.shape, generator=g).to(dev).to(torch.bfloat16))
  gy, gb = torch.autograd.grad(z1, (y1, beta), gz, retain_graph=True)
  gy_ref = _check_backward(y1, beta, groups, gz, gy, gb)
  if x is not None:     # ... and on through the convolution
    gx, = torch.autograd.grad(z1, x, gz)
    xf = x.detach().float().requires_grad_(True)
    gx_ref, = torch.autograd.grad(ref(xf), xf, gy_ref.float())
    assert float((gx.float() - gx_ref).abs().max()) <= 3e-2 * float(gx_ref.abs().max())
  # the two-pass route on the same tensor: the shift keeps rstd at 2e-5 everywhere
  yq = y0.detach().clone().requires_grad_(True)
  z0 = _hip_bn.batch_norm_relu(yq, beta, EPS, True, groups)
  _check_forward(tag + ' two-pass', yq, z0, z0.grad_fn.saved_tensors[2], beta, groups,
                 one_pass=False)
  gy0, gb0 = torch.autograd.grad(z0, (yq, beta), gz)
  _check_backward(yq, beta, groups, gz, gy0, gb0)


# ---- a producer written in torch: the sums of any tensor in the slots ---------------

def _leave_sums(x, groups, scale_q=None):
  """What lsi_conv2d_*_bnstats leaves for lsi_bn_relu_norm, for any tensor the
  batch norm takes (the convolutions produce bf16 with 32 | C only): the fp32
  sums of x and x^2 of each group spread over lsi_bn_stat_slots(C) slots -- pixel
  p in slot p % slots --, and the hand-over tag.  scale_q [C]: the sums of
  squares times that (a producer whose fp32 rounding went the other way)."""
  from lsi.nnutils import _hip_bn
  n, c, h, w = x.shape
  ns = stat_slots(c)
  ws = _hip_bn.stats_workspace(tuple(x.shape), x.device, int(x.dtype == torch.bfloat16), groups)
  xf = x.detach().double().view(groups, n // groups, c, h * w).permute(0, 1, 3, 2)
  xf = xf.reshape(groups, -1, c)
  npix = xf.shape[1]
  slot = torch.arange(npix, device=x.device) % ns
  for grp in range(groups):
    s = torch.zeros((ns, c), dtype=torch.float64, device=x.device).index_add_(0, slot, xf[grp])
    q = torch.zeros((ns, c), dtype=torch.float64, device=x.device).index_add_(
        0, slot, xf[grp] * xf[grp])
    if scale_q is not None:
      q = q * scale_q.double().view(1, c)
    base = grp * WS_STRIDE
    ws[base + WS_ACC:base + WS_ACC + ns * 2 * c] = torch.cat([s, q], 1).float().flatten()
    ws.view(torch.int32)[base + WS_TAG] = 0x5A000000 | ((groups & 0xfff) << 12) | (c & 0xfff)


def _run(x, beta, groups, relu, one_pass):
  from lsi.nnutils import _hip_bn
  if one_pass:
    _leave_sums(x, groups)
  return _hip_bn.batch_norm_relu(x, beta, EPS, relu, groups, one_pass)


def _off_centre(shape, dt, ratios, g, dev):
  """Channel ch at mean / sigma = ratios[ch % len], sigma = 2^(-6 ... 3)."""
  n, c, h, w = shape
  ch = torch.arange(c)
  ratio = torch.tensor(ratios)[ch % len(ratios)]
  sigma = 2.0 ** (-6.0 + 9.0 * ((ch * 7) % c).double() / max(c - 1, 1))
  x = torch.randn(shape, generator=g).double() * sigma.view(1, c, 1, 1) \
      + (ratio * sigma).view(1, c, 1, 1)
  return _clast(x.to(dev).to(dt)), sigma.to(dev)


# ---- 2. the two-pass route far off centre -------------------------------------------

def _shift_pixels(npix):
  """csrc/lsi_bn.hip, stat_shift: the shift is the median of these three pixels."""
  return (npix // 3, npix // 2 + npix // 7, npix - 1 - npix // 5)


@pytest.mark.parametrize('outlier', [None, 'first', 0, 1, 2],
                         ids=['plain', 'pixel-0-50-sigma-off', 'shift-pixel-a-50-sigma-off',
                              'shift-pixel-b-50-sigma-off', 'shift-pixel-c-50-sigma-off'])
@pytest.mark.parametrize('shape,groups', [((4, 32, 64, 96), 2), ((6, 64, 17, 23), 3),
                                          ((2, 8, 128, 384), 1)])
def test_two_pass_statistics_up_to_mean_1000_sigma(shape, groups, outlier, dev):
  """fp32 activations with mean / sigma up to 1000: the sums around the shift
  cannot cancel -- rstd at rtol 2e-5, mean at 1e-5 max|x| at every ratio; also
  with pixel 0 of one group (an image corner; the shift itself before it became a
  median of three pixels), or one of the three shift pixels, 50 sigma away from
  the channel's mean.
  Measured on the MI355X with the single-pixel shift: rstd off by 1.3e-3, 1.3e-4
  and 8.5e-4 on the three shapes with that pixel 50 sigma off; and with
  z = x * rstd + (beta - mean * rstd) the forward of 6 x 64 x 17 x 23 off by 1.29e-4
  (allowed 8.5e-5) at mean = 1000 sigma.  Both are fixed in csrc/lsi_bn.hip."""
  from lsi.nnutils import _hip_bn
  g = torch.Generator().manual_seed(sum(shape) + groups)
  n, c, h, w = shape
  x, sigma = _off_centre(shape, torch.float32, (0.0, 1.0, 10.0, 100.0, 300.0, 1000.0), g, dev)
  if outlier is not None:
    with torch.no_grad():
      first = (groups - 1) * (n // groups)     # the last group's first image
      p = 0 if outlier == 'first' else _shift_pixels((n // groups) * h * w)[outlier]
      x[first + p // (h * w), :, (p // w) % h, p % w] += 50.0 * sigma.float()
  beta = _beta(c, g, dev).requires_grad_(True)
  assert _hip_bn.supported(x, groups)
  xq = x.detach().clone().requires_grad_(True)
  z = _hip_bn.batch_norm_relu(xq, beta, EPS, True, groups)
  mr = z.grad_fn.saved_tensors[2]
  tag = 'two-pass f32 %s%s' % ('x'.join(map(str, shape)), '' if outlier is None else ' outlier')
  xf, m, v = _moments(x, groups)
  err = (mr[:, 1].double() * torch.sqrt(v + EPS) - 1.0).abs()
  _figures(tag, m, v, err, torch.full_like(v, 2e-5))
  mean_err = float((mr[:, 0].double() - m).abs().max())
  print('BNSTAT %-38s mean error %.2e (allowed %.2e)' % (tag, mean_err, 1e-5 * float(xf.abs().max())))
  assert float((m.abs() / v.sqrt()).max()) > 500.0
  assert mean_err <= 1e-5 * float(xf.abs().max())
  assert float(err.max()) <= 2e-5
  z_ref, _, _ = _bn_ref(x, beta, groups)
  scale = float(z_ref.abs().max()) + 1e-6
  ferr = float((z.detach().double() - z_ref).abs().max())
  print('BNSTAT %-38s forward error %.2e (allowed %.2e)' % (tag, ferr, 2e-5 * scale))
  assert ferr <= 2e-5 * scale
  assert float(((z > 0) != (z_ref > 0)).float().mean()) < 1e-3
  gz = _clast(torch.randn(shape, generator=g).to(dev))
  gx, gb = torch.autograd.grad(z, (xq, beta), gz)
  _check_backward(x, beta, groups, gz, gx, gb)


# ---- 3. relu = 0 ------------------------------------------------------------------

@pytest.mark.parametrize('one_pass', [False, True], ids=['two-pass', 'one-pass'])
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
@pytest.mark.parametrize('shape,groups', [((4, 32, 24, 40), 2), ((3, 128, 17, 23), 1)])
def test_batch_norm_without_the_relu(shape, groups, dtype, one_pass, dev):
  """relu = 0 through lsi_bn_relu_fwd / lsi_bn_relu_norm and lsi_bn_relu_bwd:
  fp64 batch_norm without the ReLU; nothing to exclude (no kink)."""
  g = torch.Generator().manual_seed(sum(shape))
  dt = getattr(torch, dtype)
  x = _clast((torch.randn(shape, generator=g) * 1.7 + 0.4).to(dev).to(dt))
  beta = _beta(shape[1], g, dev).requires_grad_(True)
  xq = x.detach().clone().requires_grad_(True)
  z = _run(xq, beta, groups, False, one_pass)
  z_ref, _, _ = _bn_ref(x, beta, groups, relu=False)
  assert float(z_ref.min()) < -1.0              # (a ReLU would show)
  fwd_tol = 2e-5 if dtype == 'float32' else 2e-2
  scale = float(z_ref.abs().max()) + 1e-6
  assert float((z.detach().double() - z_ref).abs().max()) <= fwd_tol * scale
  gz = _clast(torch.randn(shape, generator=g).to(dev).to(dt))
  gx, gb = torch.autograd.grad(z, (xq, beta), gz)
  _check_backward(x, beta, groups, gz, gx, gb, relu=False)


def test_convolution_statistics_without_the_relu(dev):
  """The one-pass route behind a real producer, relu = 0."""
  from lsi.nnutils import _hip_bn, _hip_conv
  g = torch.Generator().manual_seed(43)
  n, cin, h, w, cout, groups = 4, 64, 12, 20, 64, 2
  x = _clast(torch.relu(torch.randn((n, cin, h, w), generator=g) + 1.0).to(dev).to(torch.bfloat16))
  wt = (torch.randn((cout, cin, 3, 3), generator=g) * 0.1).to(dev)
  beta = _beta(cout, g, dev).requires_grad_(True)
  y = _hip_conv.conv2d(x, wt, 1, 1, 1, h, w, groups).detach().requires_grad_(True)
  z = _hip_bn.batch_norm_relu(y, beta, EPS, False, groups, True)
  _check_forward('conv relu=0', y, z, z.grad_fn.saved_tensors[2], beta, groups, relu=False)
  assert float(z.min()) < -1.0
  gz = _clast(torch.randn(z.shape, generator=g).to(dev).to(torch.bfloat16))
  gy, gb = torch.autograd.grad(z, (y, beta), gz)
  _check_backward(y, beta, groups, gz, gy, gb, relu=False)


# ---- 4. shape edges ---------------------------------------------------------------

def _ordinary(dev):
  g = torch.Generator().manual_seed(44)
  x = _clast((torch.randn((4, 64, 9, 14), generator=g) * 1.7 + 0.4).to(dev).to(torch.bfloat16))
  beta = _beta(64, g, dev)
  z_ref, _, _ = _bn_ref(x, beta, 2)
  return x, beta, z_ref


def _still_right(ordinary, one_pass):
  """An ordinary call on the same stream after an edge case: the arrival counter
  and the accumulators were left clean."""
  x, beta, z_ref = ordinary
  z = _run(x, beta, 2, True, one_pass)
  assert float((z.double() - z_ref).abs().max()) <= 2e-2 * float(z_ref.abs().max())


_EDGE_CHANNELS = [('bfloat16', 8), ('bfloat16', 16), ('bfloat16', 1024), ('bfloat16', 2048),
                  ('float32', 4), ('float32', 8), ('float32', 1024)]


@pytest.mark.parametrize('one_pass', [False, True], ids=['two-pass', 'one-pass'])
@pytest.mark.parametrize('dtype,c', _EDGE_CHANNELS)
def test_shape_edges(dtype, c, one_pass, dev):
  """The channel counts at both ends of the contract (one lane per pixel ...
  one pixel per workgroup step; C = 2048 fills the accumulator block), pixel
  counts below, around and off a workgroup step, 1, 3 and N groups."""
  from lsi.nnutils import _hip_bn
  dt = getattr(torch, dtype)
  rows = 256 // (c // (8 if dt == torch.bfloat16 else 4))
  ordinary = _ordinary(dev)
  fwd_tol, grad_tol = (2e-5, 2e-4) if dtype == 'float32' else (2e-2, 3e-2)
  for npix in sorted({1, 2, rows - 1, rows + 1, 10007} - {0}):
    for groups in (1, 3, 6):
      g = torch.Generator().manual_seed(1000 * c + npix + groups)
      per = 2 if (npix % 2 == 0 and groups == 3) else 1       # images per group
      shape = (groups * per, c, 1, npix // per)
      x = _clast((torch.randn(shape, generator=g) * 1.7 + 0.4).to(dev).to(dt))
      beta = _beta(c, g, dev).requires_grad_(True)
      assert _hip_bn.supported(x, groups), (shape, groups)
      xq = x.detach().clone().requires_grad_(True)
      z = _run(xq, beta, groups, True, one_pass)
      gz = _clast(torch.randn(shape, generator=g).to(dev).to(dt))
      gx, gb = torch.autograd.grad(z, (xq, beta), gz)
      z_ref, xr, br = _bn_ref(x, beta, groups)
      z_ref.backward(gz.double())
      what = (dtype, c, npix, groups)
      scale = float(z_ref.abs().max()) + 1e-6
      ferr = (z.detach().double() - z_ref).abs()
      if one_pass:
        # (two pixels whose values nearly agree are a channel far off centre: the
        # one-pass route owes its contract there, not the two-pass tolerance)
        xf, m, v = _moments(x, groups)
        e = lambda t: t.view(groups, 1, c, 1, 1)
        xhat = (xf - e(m)) * e(torch.rsqrt(v + EPS))
        ferr = ferr - (xhat.abs() * e(rstd_bound(m, v))).view_as(ferr)
      assert float(ferr.max()) <= fwd_tol * scale, what
      assert bool(torch.isfinite(gx.float()).all()), what
      if npix == 1:
        # one pixel per group: the variance is exactly 0, z = relu(beta), dx = 0
        want = torch.relu(beta.detach().double()).view(1, c, 1, 1).expand(shape)
        assert float((z.detach().double() - want).abs().max()) <= fwd_tol * scale, what
        assert bool((gx == 0).all()), what
      else:
        with torch.no_grad():
          pre, _, _ = _bn_ref(x, beta, groups, False)
          kink = pre.abs() < (2e-2 if dt == torch.bfloat16 else 1e-5)
        gs = float(xr.grad.abs().max()) + 1e-12
        err = (gx.double() - xr.grad).abs()
        if bool((~kink).any()):
          assert float(err[~kink].max()) <= grad_tol * gs, what
        slack = (gz.double().abs() * kink).sum(dim=(0, 2, 3))
        bs = float(br.grad.abs().max()) + 1e-12
        assert bool(((gb.double() - br.grad).abs() <= grad_tol * bs + slack).all()), what
      _still_right(ordinary, one_pass)


@pytest.mark.parametrize('one_pass', [False, True], ids=['two-pass', 'one-pass'])
def test_more_pixels_than_the_grid_cap_covers_in_sixteen_steps(one_pass, dev):
  """fp32, C = 32: 32 pixels per workgroup step, 16 steps per workgroup -- more
  than 1 048 576 pixels in one group cap the grid at 2048 workgroups, which then
  loop further."""
  from lsi.nnutils import _hip_bn
  g = torch.Generator().manual_seed(45)
  shape = (1, 32, 1030, 1031)
  assert shape[2] * shape[3] > 2048 * 16 * 32
  x = _clast((torch.randn(shape, generator=g) * 1.7 + 0.4).to(dev))
  beta = _beta(32, g, dev).requires_grad_(True)
  assert _hip_bn.supported(x, 1)
  xq = x.detach().clone().requires_grad_(True)
  z = _run(xq, beta, 1, True, one_pass)
  _check_forward('grid cap', x, z, z.grad_fn.saved_tensors[2], beta, 1, one_pass=one_pass)
  gz = _clast(torch.randn(shape, generator=g).to(dev))
  gx, gb = torch.autograd.grad(z, (xq, beta), gz)
  _check_backward(x, beta, 1, gz, gx, gb)
  _still_right(_ordinary(dev), one_pass)


def test_channel_counts_outside_the_contract_are_refused(dev):
  """fp32 C = 2048 and channel counts that are not a power-of-two multiple of the
  16-byte vector: supported() is false and every entry point returns LSI_EINVAL
  before any launch."""
  from lsi import _C
  from lsi.nnutils import _hip_bn
  lib = _C.lib()
  st = _C.stream_ptr(dev)
  for dt, c in ((torch.float32, 2048), (torch.float32, 12), (torch.float32, 6),
                (torch.bfloat16, 24), (torch.bfloat16, 4), (torch.bfloat16, 4096),
                (torch.bfloat16, 1536)):
    x = _clast(torch.zeros((2, c, 3, 5), dtype=dt, device=dev))
    assert not _hip_bn.supported(x), (dt, c)
    bf16 = int(dt == torch.bfloat16)
    assert lib.lsi_bn_workspace_floats(15, c, bf16, 2) == 0
    y = torch.empty_like(x)
    beta = torch.zeros((c,), device=dev)
    ws = torch.zeros((2 * WS_STRIDE,), device=dev)
    mr = torch.zeros((2, 2, c), device=dev)
    dbeta = torch.zeros((c,), device=dev)
    p = lambda t: t.data_ptr()
    assert lib.lsi_bn_relu_fwd(p(x), p(y), p(beta), p(ws), p(mr), 15, c, bf16, 1, EPS, 2,
                               st) == LSI_EINVAL
    assert lib.lsi_bn_relu_norm(p(x), p(y), p(beta), p(ws), p(mr), 15, c, bf16, 1, EPS, 2,
                                st) == LSI_EINVAL
    assert lib.lsi_bn_relu_bwd(p(x), p(y), p(mr), p(beta), p(y), p(dbeta), p(ws), 15, c, bf16,
                               1, 2, st) == LSI_EINVAL
    with pytest.raises(RuntimeError):
      _hip_bn.batch_norm_relu(x, beta, EPS, True, 2)
  torch.cuda.synchronize()


# ---- 5. constant channels, NaN ------------------------------------------------------

@pytest.mark.parametrize('one_pass', [False, True], ids=['two-pass', 'one-pass'])
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_dead_and_constant_channels(dtype, one_pass, dev):
  """An all-zero channel and constant 7.0 / -7.0 channels inside a random
  tensor: var = E[x^2] - mean^2 is within rounding of 0 on either side (clamped
  at 0).  z = relu(beta) within the contract, dx finite, dbeta the masked sum
  of dy."""
  g = torch.Generator().manual_seed(46)
  dt = getattr(torch, dtype)
  shape, groups = (4, 32, 33, 47), 2
  x = (torch.randn(shape, generator=g) * 1.7 + 0.4)
  consts = {3: 0.0, 8: 7.0, 30: -7.0}
  for ch, val in consts.items():
    x[:, ch] = val
  x = _clast(x.to(dev).to(dt))
  beta = _beta(32, g, dev).requires_grad_(True)
  xq = x.detach().clone().requires_grad_(True)
  z = _run(xq, beta, groups, True, one_pass)
  mr = z.grad_fn.saved_tensors[2]
  assert bool(torch.isfinite(mr).all())
  _check_forward('constant channels', x, z, mr, beta, groups, one_pass=one_pass)
  gz = _clast(torch.randn(shape, generator=g).to(dev).to(dt))
  gx, gb = torch.autograd.grad(z, (xq, beta), gz)
  assert bool(torch.isfinite(gx.float()).all()) and bool(torch.isfinite(gb).all())
  _check_backward(x, beta, groups, gz, gx, gb)
  for ch in consts:
    want = float(gz[:, ch].double().sum()) if float(beta[ch]) > 0 else 0.0
    tol = 1e-4 * float(gz[:, ch].double().abs().sum())     # (fp32 sums of the group, atomics)
    assert abs(float(gb[ch]) - want) <= tol, (ch, float(gb[ch]), want)


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_sums_of_a_constant_channel_that_rounded_below_zero_variance(dtype, dev):
  """What fp32 rounding in a producer may leave for a constant channel: sums of
  squares a few 2^-24 SHORT of n * mean^2.  lsi_bn_relu_norm clamps the variance
  at 0: rstd = eps^-1/2, finite, where var + eps < 0 would give NaN."""
  from lsi.nnutils import _hip_bn
  g = torch.Generator().manual_seed(47)
  dt = getattr(torch, dtype)
  shape, groups = (2, 32, 9, 14), 1
  x = torch.randn(shape, generator=g)
  x[:, 5] = 300.0
  x[:, 6] = 7.0
  x = _clast(x.to(dev).to(dt))
  beta = _beta(32, g, dev)
  short = torch.ones((32,), device=dev)
  short[5] = 1.0 - 2.0 ** -22       # 300^2 * 2^-22 = 0.02 below: var + eps < 0 unclamped
  short[6] = 1.0 - 2.0 ** -22
  _leave_sums(x, groups, short)
  xq = x.detach().clone().requires_grad_(True)
  z = _hip_bn.batch_norm_relu(xq, beta, EPS, True, groups, True)
  mr = z.grad_fn.saved_tensors[2]
  assert bool(torch.isfinite(mr).all()) and bool(torch.isfinite(z.float()).all())
  assert abs(float(mr[0, 1, 5]) * EPS ** 0.5 - 1.0) <= 2.0 ** -22
  want = torch.relu(beta[5:7]).view(1, 2, 1, 1)
  assert float((z[:, 5:7].float() - want).abs().max()) <= 2.0 ** -8 * float(want.max()) + 3e-3
  gx, = torch.autograd.grad(z, xq, torch.ones_like(z))
  assert bool(torch.isfinite(gx.float()).all())


@pytest.mark.parametrize('one_pass', [False, True], ids=['two-pass', 'one-pass'])
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_a_nan_stays_in_its_channel_and_group(dtype, one_pass, dev):
  g = torch.Generator().manual_seed(48)
  dt = getattr(torch, dtype)
  shape, groups = (4, 64, 13, 21), 2
  x = torch.randn(shape, generator=g) + 0.5
  x[3, 37, 5, 11] = float('nan')        # group 1, channel 37
  x = _clast(x.to(dev).to(dt))
  beta = _beta(64, g, dev)
  z = _run(x, beta, groups, True, one_pass)
  bad = torch.isnan(z.float())
  want = torch.zeros(shape, dtype=torch.bool, device=dev)
  want[2:, 37] = True
  assert torch.equal(bad, want)
  clean = x.clone()
  clean[3, 37, 5, 11] = 0.5
  z_ref, _, _ = _bn_ref(clean, beta, groups)
  ok = ~want
  assert float((z.double() - z_ref)[ok].abs().max()) <= \
      (2e-5 if dtype == 'float32' else 2e-2) * float(z_ref.abs().max())
  # ... and the next call is clean
  z2 = _run(clean, beta, groups, True, one_pass)
  assert bool(torch.isfinite(z2.float()).all())
