"""The seven kernels of csrc/lsi_sampling.hip (bilinear gather, its
compose=False taps, generic splat, scatter-add, and the three backward kernels)
against the fp64 restatement tests/sampling_ref.py: bit for bit.

Coordinates are multiples of 1/4 and every value an integer in [-8, 8], so each
weight is a multiple of 1/4, each product one of 1/16 and each sum -- the
atomic ones in any order -- exact in fp32 (tests/test_sampling_ref_cpu.py
proves that of every case, and the restatement against the oracle and fp64
autograd).  The assertion is `torch.equal` throughout: a block's tail thread
that runs or does not, a batch stride, a swapped weight, a gradient written for
a point that has none, one lost or doubled atomic update among 2000 -- each is
a failed equality, which the float comparisons of test_sampling_gpu.py
cannot be.

Every gradient path is asked for both gradients and for each alone (the other
output pointer NULL), which must not change what is written."""
import functools

import numpy as np
import pytest
import torch

import sampling_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def _t(a, grad=False):
  t = torch.tensor(np.asarray(a, np.float32), device='cuda:0')
  return t.requires_grad_(True) if grad else t


@functools.lru_cache(maxsize=None)
def _want(name, only=None):
  """The restatement's answers from fp32 coordinates, rounded (exactly) to fp32
  and on the device; computed once, shared and never modified."""
  return {k: _t(v) for k, v in R.expected(name, 'float32', only).items()}


def _case(name, only=None):
  cs = R.case(name)
  return cs if only is None else R.item(cs, only)


def _same(name, got, want, where=None):
  """torch.equal, and on failure where the mismatches are.  `where`: compare
  there only (broadcast against the tensors)."""
  assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, got.dtype)
  if where is not None:
    where = where.expand_as(got)
    got, want = torch.where(where, got, 0), torch.where(where, want, 0)
  if torch.equal(got, want):
    return
  bad = (got != want).nonzero()
  lo, hi = bad.min(dim=0).values.tolist(), bad.max(dim=0).values.tolist()
  first = tuple(bad[0].tolist())
  pytest.fail('%s: %d of %d values differ, inside [%s .. %s]; first at %s: got %r, want %r'
              % (name, len(bad), got.numel(), lo, hi, first, float(got[first]),
                 float(want[first])))


def _grads(out, g_out, inputs):
  return torch.autograd.grad(out, inputs, g_out)


# ---------------------------------------------------------------------------
# one function per operation: everything it computes, against `want`
# ---------------------------------------------------------------------------
def check_bilinear(cs, want):
  from lsi.geometry import sampling
  g = _t(cs.g_vals)
  for wi, wc in ((True, True), (True, False), (False, True)):
    imgs, coords = _t(cs.img, wi), _t(cs.coords, wc)
    out = sampling.bilinear(imgs, coords)
    _same('bilinear', out.detach(), want['bilinear'])
    got = _grads(out, g, [t for t, w in ((imgs, wi), (coords, wc)) if w])
    if wi:
      _same('bilinear g_imgs (coords %s)' % wc, got[0], want['bilinear_g_imgs'])
    if wc:
      _same('bilinear g_coords (imgs %s)' % wi, got[-1], want['bilinear_g_coords'])


def check_taps(cs, want):
  from lsi.geometry import sampling
  fin = torch.tensor(R.finite_points(cs), device='cuda:0')[None, ..., None]
  g_taps, g_wts = _t(cs.g_taps), _t(cs.g_wts)
  for wi in (True, False):
    for tag in ('t', 'w', 'tw'):
      imgs, coords = _t(cs.img, wi), _t(cs.coords, True)
      ims, wts = sampling.bilinear(imgs, coords, compose=False)
      assert len(ims) == 4 and len(wts) == 4
      ims, wts = torch.stack(ims), torch.stack(wts)
      _same('taps', ims.detach(), want['taps'])
      _same('weights (finite points)', wts.detach(), want['wts'], fin)
      outs, gs = [], []
      if 't' in tag:
        outs, gs = outs + [ims], gs + [g_taps]
      if 'w' in tag:
        outs, gs = outs + [wts], gs + [g_wts]
      got = torch.autograd.grad(outs, [imgs, coords] if wi else [coords], gs)
      what = 'taps, gradient from %s, imgs %s: ' % (tag, wi)
      if wi:
        _same(what + 'g_imgs', got[0], want['taps_g_imgs_' + tag])
      _same(what + 'g_coords', got[-1], want['taps_g_coords_' + tag])


def check_taps_abi(cs, want):
  """lsi_bilinear_taps_bwd itself, with every combination of absent incoming
  and outgoing gradients that autograd (which hands zeros) never forms."""
  from lsi import _C
  b, h, w, c = cs.img.shape
  hp, wp = cs.coords.shape[1:3]
  coords, g_taps, g_wts = _t(cs.coords), _t(cs.g_taps), _t(cs.g_wts)
  dev = coords.device
  for tag in ('t', 'w', 'tw'):
    for wi, wc in ((True, True), (True, False), (False, True)):
      if wi and 't' not in tag:
        continue        # refused: an image gradient needs the taps' (test_abi.py)
      g_imgs = torch.zeros((b, h, w, c), device=dev) if wi else None
      g_coords = torch.full((b, hp, wp, 2), 77.0, device=dev) if wc else None
      rc = _C.lib().lsi_bilinear_taps_bwd(
          b, h, w, c, hp, wp, _C.ptr(coords), _C.ptr(g_taps if 't' in tag else None),
          _C.ptr(g_wts if 'w' in tag else None), _C.ptr(g_imgs), _C.ptr(g_coords),
          _C.stream_ptr(dev))
      assert rc == 0, (tag, wi, wc, rc)
      what = 'lsi_bilinear_taps_bwd, incoming %s, outgoing imgs %s coords %s: ' % (tag, wi, wc)
      if wi:
        _same(what + 'g_imgs', g_imgs, want['taps_g_imgs_' + tag])
      if wc:
        _same(what + 'g_coords', g_coords, want['taps_g_coords_' + tag])


def check_splat(cs, want):
  from lsi.geometry import sampling
  g = _t(cs.g_img)
  for ws, wc, wn in ((True, True, True), (True, False, False), (False, True, False),
                     (False, False, True), (True, True, False)):
    src, coords, init = _t(cs.vals, ws), _t(cs.coords, wc), _t(cs.img, wn)
    out = sampling.splat(src, coords, init)
    _same('splat', out.detach(), want['splat'])
    _same('splat left init alone', init.detach(), _t(cs.img))
    asked = [(t, k) for t, w, k in ((src, ws, 'splat_g_src'), (coords, wc, 'splat_g_coords'),
                                    (init, wn, 'splat_g_init')) if w]
    got = _grads(out, g, [t for t, _ in asked])
    for gt, (_, key) in zip(got, asked):
      _same('%s (asked for src %s coords %s init %s)' % (key, ws, wc, wn), gt, want[key])


def check_all(name, only=None):
  cs, want = _case(name, only), _want(name, only)
  check_bilinear(cs, want)
  check_taps(cs, want)
  check_taps_abi(cs, want)
  check_splat(cs, want)


# ---------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', R.LATTICE)
def test_lattice_shapes(name, dev):
  """1, 255, 256, 257 and 513 points on 1x1, one-row, one-column and 9x13
  images, C in {1, 3, 5}, B in {1, 3}: forward values and every gradient."""
  check_all(name)


def test_batch_strides(dev):
  """Item 1 of a three-item batch on its own: the same bits as inside it."""
  name = R.STRIDES
  check_all(name, only=1)
  full, alone = _want(name), _want(name, 1)
  for key in alone:
    axis = 1 if key in ('taps', 'wts') else 0
    _same(key, alone[key], full[key].narrow(axis, 1, 1))


def test_bilinear_wrapper_two_leading_dimensions(dev):
  from lsi.geometry import sampling
  name = next(k for k in R.LATTICE if R.SHAPES[k].b == 6)
  cs, want = R.case(name), _want(name)
  lead = lambda a, ax=0: a.reshape(a.shape[:ax] + (2, 3) + a.shape[ax + 1:])
  imgs, coords = _t(lead(cs.img), True), _t(lead(cs.coords), True)
  out = sampling.bilinear_wrapper(imgs, coords)
  _same('wrapper', out.detach(), lead(want['bilinear']))
  gi, gc = _grads(out, _t(lead(cs.g_vals)), [imgs, coords])
  _same('wrapper g_imgs', gi, lead(want['bilinear_g_imgs']))
  _same('wrapper g_coords', gc, lead(want['bilinear_g_coords']))
  ims, wts = sampling.bilinear_wrapper(imgs, coords, compose=False)
  _same('wrapper taps', torch.stack(ims).detach(), lead(want['taps'], 1))
  _same('wrapper weights', torch.stack(wts).detach(), lead(want['wts'], 1))
  gi, gc = torch.autograd.grad(
      ims + wts, [imgs, coords],
      list(_t(lead(cs.g_taps, 1))) + list(_t(lead(cs.g_wts, 1))))
  _same('wrapper taps g_imgs', gi, lead(want['taps_g_imgs_tw']))
  _same('wrapper taps g_coords', gc, lead(want['taps_g_coords_tw']))


@pytest.mark.parametrize('name', R.HOSTILE)
def test_hostile_points(name, dev):
  """A tenth of the points NaN, +-Inf, +-1e9 or +-3e38 in x, y or both: zeros at
  the non-finite ones -- in the outputs and in every gradient, the compose=False
  coordinate gradient included -- and the same bits as ever elsewhere."""
  check_all(name)
  bad = torch.tensor(~R.finite_points(R.case(name)), device=dev)
  want = _want(name)
  assert bool(bad.any())
  for key in ('bilinear', 'bilinear_g_coords', 'taps_g_coords_tw', 'splat_g_coords',
              'splat_g_src'):
    assert not bool(want[key][bad].any()), key


@pytest.mark.parametrize('name', R.COLLIDE)
def test_two_thousand_points_in_one_place(name, dev):
  """Splat: 2000 sources onto one pixel centre (one corner, weight 1) or one
  pixel corner (four, weight 1/4).  Gather: 2000 targets sample that place, so
  its image gradient is as many atomic adds to the same taps."""
  check_all(name)
  cs, want = R.case(name), _want(name)
  moved = (want['splat'] != _t(cs.img)).any(-1).sum().item()
  hit = (want['bilinear_g_imgs'] != 0).any(-1).sum().item()
  assert moved == hit == (1 if R.SHAPES[name].kind == 'centre' else 4)


@pytest.mark.parametrize('name', R.CLAMPED)
def test_weight_clamp(name, dev):
  """Corner weights of 2^-10 (below 1e-3: dropped, with its gradients) and 2^-9
  (kept in full), from either side on either axis."""
  cs, want = R.case(name), _want(name)
  check_splat(cs, want)
  check_bilinear(cs, want)       # (the gather has no clamp: 2^-10 counts)


@pytest.mark.parametrize('name', list(R.SCATTER))
def test_scatter_add(name, dev):
  """N in {1, 257, 700} updates into P in {1, 5} places, B = 3; once with all
  700 updates of a row on one index."""
  from lsi.geometry import sampling
  (init, idx, upd, g), (out, g_init, g_upd) = R.scatter_case(name)
  tidx = torch.tensor(idx, device=dev)
  for wn, wu in ((True, True), (True, False), (False, True)):
    ti, tu = _t(init, wn), _t(upd, wu)
    got = sampling.batch_scatter_add_tensor(ti, tidx, tu)
    _same('batch_scatter_add_tensor', got.detach(), _t(out))
    grads = _grads(got, _t(g), [t for t, w in ((ti, wn), (tu, wu)) if w])
    if wn:
      _same('g_init', grads[0], _t(g_init))
    if wu:
      _same('g_upd', grads[-1], _t(g_upd))
  for row in range(init.shape[0]):
    ti, tu = _t(init[row], True), _t(upd[row], True)
    for ix in (tidx[row], tidx[row][:, None]):
      got = sampling.scatter_add_tensor(ti, ix, tu)
      _same('scatter_add_tensor', got.detach(), _t(out[row]))
    gi, gu = _grads(got, _t(g[row]), [ti, tu])
    _same('scatter_add_tensor g_init', gi, _t(g_init[row]))
    _same('scatter_add_tensor g_upd', gu, _t(g_upd[row]))


def test_repeatable_and_stream_ordered(dev):
  """One case twice on the current stream and once on a side stream: identical
  bits (the calls are ordered on the stream they are made on)."""
  from lsi.geometry import sampling
  cs = R.case(R.STRIDES)

  def run():
    imgs, coords, src = _t(cs.img, True), _t(cs.coords, True), _t(cs.vals, True)
    out = sampling.bilinear(imgs, coords)
    res = [out] + list(_grads(out, _t(cs.g_vals), [imgs, coords]))
    ims, wts = sampling.bilinear(imgs, coords, compose=False)
    res += list(torch.autograd.grad(ims + wts, [imgs, coords],
                                    list(_t(cs.g_taps)) + list(_t(cs.g_wts))))
    init = _t(cs.img, True)
    out = sampling.splat(src, coords, init)
    res += [out] + list(_grads(out, _t(cs.g_img), [src, coords, init]))
    return [r.detach() for r in res]

  first, second = run(), run()
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  with torch.cuda.stream(side):
    third = run()
  side.synchronize()
  want = _want(R.STRIDES)
  _same('bilinear', first[0], want['bilinear'])
  _same('splat', first[5], want['splat'])
  for k, (a, b, c) in enumerate(zip(first, second, third)):
    _same('result %d, second run' % k, b, a)
    _same('result %d, side stream' % k, c, a)
