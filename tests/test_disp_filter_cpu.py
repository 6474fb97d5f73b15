"""The disparity post-filters without a GPU: the NumPy restatement
(tests/disp_filter_ref.py) agrees with a second statement through
scipy.sparse.csgraph and with hand-made answers, the C entry points refuse bad
arguments before any launch and size their workspace as DESIGN.md section 4.18
says, and on the known scene of tests/sgm_ref.py the filter removes wrong
disparities for a negligible loss of density."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import disp_filter_ref as F
import sgm_ref as R

EINVAL, ENULL, EWORKSPACE = -1, -2, -3


# -- the restatement ------------------------------------------------------------------
@pytest.mark.parametrize('shape, rng', [((3, 37, 53), 256), ((1, 69, 73), 256),
                                        ((2, 20, 31), 0), ((2, 20, 31), 3)])
def test_second_restatement(shape, rng):
  img = F.random_map(sum(shape) + rng, shape, rng)
  some = False
  for b in range(shape[0]):
    a = F.component_sizes(img[b].astype(np.int64), rng)
    c = F.component_sizes_scipy(img[b].astype(np.int64), rng)
    assert np.array_equal(a, c)
    assert ((a > 0) == (img[b] > 0)).all()
    some |= a.max() > 5 and (a == 1).any() and (a == 2).any()
  assert some                                        # sizes on both sides of the thresholds below
  for size in (1, 2, 5):
    for median in (0, 3):
      want = F.filter_batch(img, median, size, rng)
      assert np.array_equal(want, F.filter_batch(img, median, size, rng,
                                                 sizes=F.component_sizes_scipy))
      assert not np.array_equal(want, F.filter_batch(img, median, 0, rng)), (size, median)


def test_known_answers_speckle():
  a = 1000
  img = np.array([[a, a, 0, a + 300, 0],
                  [0, a, 0, 0, a],
                  [0, a + 256, a + 512, 0, a],
                  [a, 0, 0, 0, a + 257],
                  [a, a, 0, 0, a + 257]], np.uint16)
  # components: 5 pixels (a chain of steps of exactly 256), one singleton at
  # (0, 3), a pair at the right edge cut from the pair under it by a step of
  # 257, and 3 pixels at the lower left; (2, 2) and (1, 4) touch only diagonally
  size = F.component_sizes(img.astype(np.int64), 256)
  assert size.tolist() == [[5, 5, 0, 1, 0],
                           [0, 5, 0, 0, 2],
                           [0, 5, 5, 0, 2],
                           [3, 0, 0, 0, 2],
                           [3, 3, 0, 0, 2]]
  assert np.array_equal(F.filter_batch(img, 0, 0), img)
  one = F.filter_batch(img, 0, 1)
  assert one[0, 3] == 0 and (one != img).sum() == 1
  two = F.filter_batch(img, 0, 2)
  assert (two != 0).sum() == 8 and two[3, 0] == a and two[1, 4] == 0
  four = F.filter_batch(img, 0, 4)
  assert np.array_equal(four != 0, size == 5)       # <= : a component of 5 survives 4
  assert not F.filter_batch(img, 0, 5).any()        # ... and not 5
  # the difference is taken in a wider integer
  wide = np.array([[65535, 1, 2]], np.uint16)
  assert F.component_sizes(wide.astype(np.int64), 65533).tolist() == [[1, 2, 2]]
  assert F.component_sizes(wide.astype(np.int64), 65534).tolist() == [[3, 3, 3]]


def test_known_answers_median():
  img = np.array([[10, 0, 30, 0, 7],
                  [0, 20, 0, 0, 9],
                  [50, 0, 40, 0, 0],
                  [0, 0, 0, 0, 0],
                  [3, 0, 0, 5, 4]], np.uint16)
  got = F.filter_batch(img, 3)
  want = np.zeros_like(img)
  want[0, 0] = 10       # {10, 20}: element 0 of 2 -- the lower median
  want[0, 2] = 20       # {20, 30}
  want[1, 1] = 30       # {10, 20, 30, 40, 50}
  want[2, 0] = 20       # {20, 50}
  want[2, 2] = 20       # {20, 40}
  want[0, 4] = 7        # {7, 9}
  want[1, 4] = 7
  want[4, 0] = 3        # alone
  want[4, 3] = 4        # {4, 5}
  want[4, 4] = 4
  assert np.array_equal(got, want)                  # and every hole stayed one
  # the stage reads its input only: a chain 1 2 3 4 5 does not cascade
  row = np.array([[256, 512, 768, 1024, 1280]], np.uint16)
  assert F.filter_batch(row, 3).tolist() == [[256, 512, 768, 1024, 1024]]
  # median first, speckle on its output: the median joins 100 | 900 | 100 ...
  img = np.array([[100, 900, 100, 0, 100]], np.uint16)
  assert F.filter_batch(img, 0, 2, 256).tolist() == [[0, 0, 0, 0, 0]]
  assert F.filter_batch(img, 3, 2, 256).tolist() == [[100, 100, 100, 0, 0]]


def test_patterns():
  img, n = F.serpentine(9, 7)
  assert n == 5 * 7 + 4
  size = F.component_sizes(img.astype(np.int64), 0)
  assert set(size[img != 0].tolist()) == {n}
  img, n = F.serpentine(8, 7)                        # an even height: the last row is empty
  assert n == 4 * 7 + 3 and not img[7].any()
  assert set(F.component_sizes(img.astype(np.int64), 0)[img != 0].tolist()) == {n}


# -- the C entry points -------------------------------------------------------------
def _call(lib, B=2, H=8, W=12, src=1, dst=1, median=3, size=20, rng=256, ws=1, ws_bytes=None,
          same=False):
  """lsi_disparity_filter_u16 with host buffers standing in for device memory:
  a call that is refused launches nothing and never touches them."""
  bufs = [(ctypes.c_char * 64)() for _ in range(3)]
  p = lambda on, k: ctypes.addressof(bufs[k]) if on else None
  if ws_bytes is None:
    ws_bytes = 1 << 40
  return lib.lsi_disparity_filter_u16(B, H, W, p(src, 0), p(dst, 0 if same else 1), median,
                                      size, rng, p(ws, 2), ws_bytes, None)


def test_abi_refusals(built_lib):
  from lsi import _C
  lib = _C.lib()
  for dims in (dict(B=0), dict(H=0), dict(W=-3), dict(B=1 << 14, H=1 << 7, W=(1 << 7) + 1)):
    assert _call(lib, **dims) == EINVAL, dims
  for bad in (dict(median=1), dict(median=5), dict(median=-3), dict(size=-1),
              dict(size=(1 << 27) + 1), dict(rng=-1), dict(rng=65536), dict(same=True)):
    assert _call(lib, **bad) == EINVAL, bad
  for name in ('src', 'dst', 'ws'):
    assert _call(lib, **{name: 0}) == ENULL, name
  # (every call here must be one the library refuses: where a device is present
  # an accepted call would launch on these host buffers)
  need = lib.lsi_disparity_filter_workspace_bytes(2, 8, 12, 3, 20)
  assert need > 0
  assert _call(lib, ws_bytes=need - 1) == EWORKSPACE
  # refusals come in the documented order: arguments, pointers, workspace
  assert _call(lib, median=5, src=0, ws_bytes=0) == EINVAL
  assert _call(lib, same=True, ws=0, ws_bytes=0) == EINVAL
  assert _call(lib, src=0, ws_bytes=0) == ENULL
  assert _call(lib, ws_bytes=0) == EWORKSPACE


def test_workspace_size(built_lib):
  from lsi import _C
  f = _C.lib().lsi_disparity_filter_workspace_bytes
  for b, h, w in ((2, 375, 1242), (1, 1, 1), (3, 37, 53), (1, 1 << 13, 1 << 14)):
    n = b * h * w
    assert f(b, h, w, 0, 20) == 8 * n               # a 4-byte parent and size per pixel
    assert f(b, h, w, 3, 20) == 8 * n + (2 * n + 15) // 16 * 16   # ... and the median plane
    assert f(b, h, w, 3, 0) == 0 and f(b, h, w, 0, 0) == 0        # no labelling, no scratch
  assert f(1, 8, 8, 0, 1 << 27) == 8 * 64
  for bad in ((0, 8, 8, 3, 20), (1, 0, 8, 3, 20), (1, 8, -1, 3, 20), (1, 8, 8, 5, 20),
              (1, 8, 8, 1, 20), (1, 8, 8, 3, -1), (1, 8, 8, 3, (1 << 27) + 1),
              (1 << 14, 1 << 7, (1 << 7) + 1, 3, 20)):
    assert f(*bad) == 0, bad


def test_no_cpu_fallback_and_argument_checks(built_lib):
  from lsi.geometry import stereo
  u16 = torch.zeros(1, 8, 12, dtype=torch.uint16)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    stereo.filter_disparity(u16, median=3)
  with pytest.raises(TypeError):
    stereo.filter_disparity(u16.numpy())
  img = torch.zeros(1, 8, 12, 3, dtype=torch.uint8)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    stereo.sgm_disparity(img, img, max_disp=16, median=3, speckle_size=20, speckle_range=256)


def test_parser_defaults_are_off():
  from lsi.data.kitti import preprocess
  a = preprocess.build_parser().parse_args(['--kitti_data_root', '/x'])
  assert (a.median, a.speckle_size, a.speckle_range) == (0, 0, 256)
  b = preprocess.build_parser().parse_args(
      ['--kitti_data_root', '/x', '--median', '3', '--speckle_size', '20', '--speckle_range',
       '128'])
  assert (b.median, b.speckle_size, b.speckle_range) == (3, 20, 128)
  with pytest.raises(SystemExit):
    preprocess.build_parser().parse_args(['--kitti_data_root', '/x', '--median', '5'])
  assert 'whatever' in preprocess.build_parser().format_help()
  import inspect
  sig = inspect.signature(preprocess.run)
  assert list(sig.parameters)[-3:] == ['median', 'speckle_size', 'speckle_range']
  assert [sig.parameters[k].default for k in list(sig.parameters)[-3:]] == [0, 0, 256]


# -- the filter earns its place -------------------------------------------------------
DENSITY_CAP = 0.003      # twice the worst measured drop (0.00144 -> 0.0015)


@functools.lru_cache(maxsize=None)
def scene(seed, lr_max):
  left, right, disp, visible = R.step_scene(seed)
  out_l, _ = R.sgm_pair(left, right, D=32, lr_max=lr_max)
  return out_l, disp, visible


def _figures(out, disp, visible):
  got = out > 0
  wrong = int((np.abs(out[got] / 256.0 - disp[got]) > 1.0).sum())
  density = (got & visible).sum() / float(visible.sum())
  return wrong, density


@pytest.mark.parametrize('lr_max', [1, -1])
@pytest.mark.parametrize('seed', [1, 2, 3, 4, 5])
def test_filter_removes_wrong_disparities(seed, lr_max):
  out, disp, visible = scene(seed, lr_max)
  wrong0, dens0 = _figures(out, disp, visible)
  filt = F.filter_batch(out, 0, 20, 256)
  wrong1, dens1 = _figures(filt, disp, visible)
  print('seed %d lr_max %d: wrong %d -> %d, density %.4f -> %.4f (drop %.4f)' % (
      seed, lr_max, wrong0, wrong1, dens0, dens1, dens0 - dens1))
  assert wrong1 < wrong0
  assert dens0 - dens1 <= DENSITY_CAP
