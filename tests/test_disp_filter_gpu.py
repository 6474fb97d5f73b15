"""The disparity post-filters on the device (csrc/lsi_disp_filter.hip through
lsi.geometry.stereo.filter_disparity) against the NumPy restatement in
tests/disp_filter_ref.py: equal bit for bit, no tolerance -- everything is
integer and components are unique.

The kernel labels T x T tiles in LDS and merges them across their edges; T is
stated here.  "Multi-tile" is (2 T + 5) x (2 T + 9): three tiles in each
direction, the last one ragged -- the smallest shape at which the merge across
edges and corners can go wrong.  The other shapes are one pixel, one row, one
column and an odd size inside a tile or two."""
import os

import numpy as np
import pytest
import torch

import disp_filter_ref as F
import sgm_ref as R

pytestmark = pytest.mark.gpu

T = 32                                   # TILE of csrc/lsi_disp_filter.hip
MH, MW = 2 * T + 5, 2 * T + 9            # multi-tile


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def run(dev, img, median=0, size=0, rng=256):
  from lsi.geometry import stereo
  return stereo.filter_disparity(torch.from_numpy(np.array(img)).to(dev), median=median,
                                 speckle_size=size, speckle_range=rng)


def assert_same(got, want, what):
  got = got.cpu().numpy()
  assert got.dtype == np.uint16 and got.shape == want.shape, what
  if not np.array_equal(got, want):
    bad = np.argwhere(got != want)
    pytest.fail('%s: %d of %d pixels differ, first at %s: got %d, want %d' % (
        what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def check(dev, img, median=0, size=0, rng=256, what=''):
  """The device's answer is the restatement's; returns the restatement's."""
  img = np.ascontiguousarray(img, dtype=np.uint16)
  want = F.filter_batch(img, median, size, rng)
  assert_same(run(dev, img, median, size, rng), want,
              '%s median %d size %d range %d' % (what, median, size, rng))
  return want


# -- single pixel, row, column ---------------------------------------------------------
def test_one_pixel_row_column(dev):
  for v in (0, 700):
    one = np.full((1, 1, 1), v, np.uint16)
    for median in (0, 3):
      assert check(dev, one, median, 0, what='1x1')[0, 0, 0] == v
      assert check(dev, one, median, 1, what='1x1')[0, 0, 0] == 0
  row = F.random_map(3, (1, 1, 2 * T + 9), 256, valid=0.8)
  col = F.random_map(4, (1, 2 * T + 5, 1), 256, valid=0.8)
  for img, what in ((row, 'row'), (col, 'column'), (row[0], 'row, unbatched')):
    kept = [int((check(dev, img, median, size, what=what) != 0).sum())
            for median in (0, 3) for size in (0, 1, 2, 4)]
    assert kept[0] > kept[1] > kept[3] > 0, (what, kept)     # the sizes say something


# -- uniform maps ------------------------------------------------------------------------
def test_all_invalid(dev):
  img = np.zeros((2, MH, MW), np.uint16)
  for median in (0, 3):
    assert not check(dev, img, median, 20).any()


def test_one_component_over_every_tile(dev):
  img = np.full((1, MH, MW), 5000, np.uint16)
  assert check(dev, img, 0, MH * MW - 1, what='constant').all()      # kept
  assert not check(dev, img, 0, MH * MW, what='constant').any()      # removed
  assert check(dev, np.repeat(img, 2, 0), 3, MH * MW - 1, what='constant x2').all()


# -- serpentine --------------------------------------------------------------------------
@pytest.mark.parametrize('transposed', [False, True])
def test_serpentine(dev, transposed):
  img, n = F.serpentine(MH, MW)
  assert n == (MH + 1) // 2 * MW + (MH - 1) // 2
  if transposed:
    img = np.ascontiguousarray(img.T)
  assert not check(dev, img, 0, n, 0, 'serpentine').any()            # length = speckle_size
  assert np.array_equal(check(dev, img, 0, n - 1, 0, 'serpentine'), img)   # = speckle_size + 1
  # two of them in a batch, the second one upside down (its path runs the other way)
  both = np.stack([img, img[::-1]])
  assert np.array_equal(check(dev, both, 0, n - 1, 256, 'serpentines'), both)
  assert not check(dev, both, 0, n, 256, 'serpentines').any()


# -- the link threshold ------------------------------------------------------------------
def test_link_threshold(dev):
  y, x = np.indices((MH, MW))
  rng = 256
  ramp = (300 + (x + y) * rng).astype(np.uint16)                     # neighbours differ by rng
  assert int(ramp.max()) - int(ramp.min()) > 100 * rng
  assert np.array_equal(check(dev, ramp, 0, MH * MW - 1, rng, 'ramp'), ramp)
  assert not check(dev, ramp, 0, MH * MW, rng, 'ramp').any()
  steep = (300 + (x + y) * (rng + 1)).astype(np.uint16)              # ... by rng + 1
  assert not check(dev, steep, 0, 1, rng, 'steep ramp').any()        # all singletons
  assert np.array_equal(check(dev, steep, 0, 1, rng + 1, 'steep ramp'), steep)
  # range 0: equal neighbours are linked, unequal ones are not
  blocks = (500 + ((x // 5 + y // 3) % 2)).astype(np.uint16)         # 5 x 3 blocks of 500 / 501
  want = check(dev, blocks, 0, 14, 0, 'blocks')
  assert want.any() and not want.all()                               # ragged blocks went
  assert not check(dev, blocks, 0, 15, 0, 'blocks').any()
  assert np.array_equal(check(dev, blocks, 0, 15, 1, 'blocks'), blocks)
  # the difference needs more than 16 bits' care
  wide = np.zeros((MH, MW), np.uint16)
  wide[T - 1:T + 1, :] = np.where((x[:2] + y[:2]) % 2 == 0, 65535, 1)   # two rows, checkered
  assert not check(dev, wide, 0, 1, 65533, '65535 beside 1').any()
  assert np.array_equal(check(dev, wide, 0, 1, 65534, '65535 beside 1'), wide)
  assert np.array_equal(check(dev, wide, 0, 2 * MW - 1, 65535, '65535 beside 1'), wide)


# -- the size threshold ------------------------------------------------------------------
def test_size_threshold_across_a_tile_corner(dev):
  img = np.zeros((MH, MW), np.uint16)
  img[T - 1:T + 1, T - 3:T + 3] = 900          # 12 pixels around the corner (T, T)
  img[T - 2, T] = 900                          # 13
  img[2 * T - 1:2 * T + 1, 2 * T - 3:2 * T + 3] = 2000    # 12 around (2 T, 2 T)
  img[T - 4:T + 3, 2 * T] = 3000               # 7 down an edge
  img[T - 1, 2 * T - 3:2 * T + 1] = 3000       # ... and 3 more along a row: 10
  sizes = sorted(set(F.component_sizes(img.astype(np.int64), 256).ravel().tolist()))
  assert sizes == [0, 10, 12, 13]
  for size, left in ((9, 3), (10, 2), (11, 2), (12, 1), (13, 0)):
    want = check(dev, img, 0, size, 256, 'corner')
    assert len(set(want.ravel().tolist()) - {0}) == left, size


# -- 4-connectivity ----------------------------------------------------------------------
def test_checkerboard(dev):
  y, x = np.indices((MH, MW))
  img = np.where((x + y) % 2 == 0, 4000, 0).astype(np.uint16)
  assert not check(dev, img, 0, 1, 65535, 'checkerboard').any()
  assert np.array_equal(check(dev, img, 0, 0, 65535, 'checkerboard'), img)


# -- batch isolation ---------------------------------------------------------------------
def test_nothing_joins_across_images_or_row_ends(dev):
  b, h, w = 3, 37, 53
  img = np.zeros((b, h, w), np.uint16)
  img[:, 0, :] = 800                      # the first and the last row: consecutive in memory
  img[:, h - 1, :] = 800                  # from one image to the next
  for y in range(4, h - 5, 4):
    img[:, y, w - 2:] = 800               # the end of a row and the start of the next
    img[:, y + 1, :2] = 800
  for size in (1, 2, 3, w - 1, w, 2 * w - 1):
    want = check(dev, img, 0, size, 256, 'isolation')
    assert want[:, 0].all() == (size < w) and want[:, 4, w - 2:].all() == (size < 2)
  # the same on one tall multi-tile image pair
  tall = np.zeros((2, MH, MW), np.uint16)
  tall[:, 0, :] = tall[:, MH - 1, :] = 800
  tall[:, T - 1, MW - 2:] = tall[:, T, :2] = 800
  for size in (2, 3, MW, 2 * MW - 1):
    check(dev, tall, 0, size, 256, 'isolation, multi-tile')


# -- random maps -------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(3, 37, 53), (2, MH, MW)])
def test_random_maps(dev, shape):
  rng = 256
  img = F.random_map(11 + shape[0], shape, rng)
  sizes = F.component_sizes(img[0].astype(np.int64), rng)
  assert sizes.max() > 5 and (sizes == 1).any() and (sizes == 2).any()
  kept = [int((check(dev, img, 0, size, rng, 'random') != 0).sum()) for size in (1, 2, 3, 5, 9)]
  assert kept == sorted(kept, reverse=True) and len(set(kept)) == len(kept)
  # a denser map: components that wind through several tiles
  dense = F.random_map(12 + shape[0], shape, rng, valid=0.95)
  dense = np.where(dense > 300 + rng, dense - rng - 1, dense).astype(np.uint16)   # 2 linked levels
  assert F.component_sizes(dense[0].astype(np.int64), rng).max() > shape[1] * shape[2] // 2
  for size in (3, 40, shape[1] * shape[2] // 2):
    check(dev, dense, 0, size, rng, 'dense')
    check(dev, dense, 3, size, rng, 'dense')


# -- the median --------------------------------------------------------------------------
def test_median(dev):
  known = np.array([[10, 0, 30, 0, 7],
                    [0, 20, 0, 0, 9],
                    [50, 0, 40, 0, 0],
                    [0, 0, 0, 0, 0],
                    [3, 0, 0, 5, 4]], np.uint16)
  want = check(dev, known, 3, what='known')
  assert want[1, 1] == 30 and want[0, 0] == 10 and want[4, 4] == 4 and want[1, 0] == 0
  for shape, valid in (((3, 37, 53), 0.6), ((1, MH, MW), 0.9), ((2, 5, 7), 1.0), ((1, 2, 2), 1.0)):
    rs = np.random.RandomState(shape[1])
    img = rs.randint(1, 65536, shape).astype(np.uint16)    # the whole range of values
    img[rs.rand(*shape) >= valid] = 0
    img[:, 0, 0] = 65535                                   # a valid corner
    want = check(dev, img, 3, what='median')
    assert ((want == 0) == (img == 0)).all()               # no hole filled, none made
    assert not np.array_equal(want, img)
    smooth = F.random_map(shape[2], shape, 256, valid)
    for size in (2, 6):                                    # the median, then the speckles
      both = check(dev, smooth, 3, size, 256, 'median + speckle')
      if valid < 1.0:                                      # each stage has its say
        assert not np.array_equal(both, F.filter_batch(smooth, 0, size, 256))
        assert not np.array_equal(both, F.filter_batch(smooth, 3, 0, 256))


def test_both_stages_off_is_a_copy(dev):
  img = F.random_map(5, (2, 37, 53), 256)
  src = torch.from_numpy(img).to(dev)
  from lsi.geometry import stereo
  out = stereo.filter_disparity(src)
  assert out.data_ptr() != src.data_ptr()
  assert_same(out, img, 'copy')
  assert_same(src, img, 'the input')


# -- composition with the matcher --------------------------------------------------------
def test_sgm_disparity_with_filters(dev):
  from lsi.geometry import stereo
  left, right = R.noise_pair(21, 2, 24, 40, 3)
  l, r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
  raw = stereo.sgm_disparity(l, r, max_disp=16)
  want_raw = R.sgm_batch(left, right, D=16)
  for got, want in zip(raw, want_raw):
    assert_same(got, want, 'the unfiltered call')             # unchanged by the filters' arrival
  fused = stereo.sgm_disparity(l, r, max_disp=16, median=3, speckle_size=20)
  for got, unfiltered, want in zip(fused, raw, want_raw):
    assert got.shape == (2, 24, 40)
    assert torch.equal(got, stereo.filter_disparity(unfiltered, median=3, speckle_size=20))
    ref = F.filter_batch(want, 3, 20, 256)
    assert_same(got, ref, 'matcher + filters')
    assert not np.array_equal(ref, want)
  one = stereo.sgm_disparity(l[1], r[1], max_disp=16, speckle_size=20, speckle_range=128)
  for got, want in zip(one, want_raw):
    assert_same(got, F.filter_batch(want[1], 0, 20, 128), 'unbatched matcher + speckle')
  with pytest.raises(RuntimeError, match='lsi_disparity_filter_u16'):
    stereo.sgm_disparity(l, r, max_disp=16, median=5)
  with pytest.raises(RuntimeError, match='lsi_disparity_filter_u16'):
    stereo.filter_disparity(raw[0], speckle_size=20, speckle_range=65536)
  with pytest.raises(RuntimeError, match='uint16'):
    stereo.filter_disparity(l)
  with pytest.raises(RuntimeError, match=r'\[B, H, W\]'):
    stereo.filter_disparity(raw[0][None])


# -- plumbing ----------------------------------------------------------------------------
def test_repeatable_side_stream_and_strides(dev):
  from lsi.geometry import stereo
  img = F.random_map(31, (2, MH, MW), 256, valid=0.9)
  want = F.filter_batch(img, 3, 30, 256)
  src = torch.from_numpy(img).to(dev)
  a = stereo.filter_disparity(src, 3, 30, 256)
  b = stereo.filter_disparity(src, 3, 30, 256)
  assert torch.equal(a, b)
  assert_same(a, want, 'default stream')
  side = torch.cuda.Stream(device=dev)
  torch.cuda.synchronize(dev)
  with torch.cuda.stream(side):
    c = stereo.filter_disparity(src, 3, 30, 256)
  side.synchronize()
  assert torch.equal(a, c)
  # a non-contiguous view: every other column of a wider tensor, and a transpose
  spread = np.zeros((2, MH, 2 * MW), np.uint16)
  spread[:, :, ::2] = img
  view = torch.from_numpy(spread).to(dev)[:, :, ::2]
  assert not view.is_contiguous()
  assert torch.equal(stereo.filter_disparity(view, 3, 30, 256), a)
  turned = src.transpose(1, 2)
  assert not turned.is_contiguous()
  assert_same(stereo.filter_disparity(turned, 0, 30, 256),
              F.filter_batch(np.ascontiguousarray(img.transpose(0, 2, 1)), 0, 30, 256), 'transposed')


def _read_png(path):
  from PIL import Image
  with Image.open(path) as im:
    assert im.mode in ('I;16', 'I;16B', 'I;16L')
    return np.asarray(im).astype(np.uint16)


def test_tool_with_and_without_filters(dev, tmp_path):
  from lsi.data.kitti import data as kitti
  from lsi.data.kitti import pipeline, preprocess
  from lsi.geometry import stereo
  from test_kitti_pipeline_cpu import make_opts, make_tree
  differ = 0
  for name, flags, kw in (
      ('plain', [], {}),
      ('filtered', ['--median', '3', '--speckle_size', '6', '--speckle_range', '200'],
       dict(median=3, speckle_size=6, speckle_range=200))):
    root = tmp_path / name
    root.mkdir()
    make_tree(root, 'val')                            # five pairs, each of its own size
    assert preprocess.main(['--kitti_data_root', str(root), '--max_disp', '16', '--workers', '4',
                            '--sequences', ','.join(kitti.raw_city_sequences())] + flags) == 0
    opts = make_opts(root, 'val')
    opts.kitti_dl_disparities_px = True
    loader = kitti.DataLoader(opts)
    assert len(loader.img_list_src) == 5
    for i, src in enumerate(loader.img_list_src):
      left = torch.from_numpy(pipeline.decode_u8(src, 3).copy()).to(dev)
      right = torch.from_numpy(pipeline.decode_u8(loader.img_list_trg[i], 3).copy()).to(dev)
      plain = stereo.sgm_disparity(left, right, max_disp=16)
      want = stereo.sgm_disparity(left, right, max_disp=16, **kw)
      for path, w, p in zip((loader.img_list_disp_src[i], loader.img_list_disp_trg[i]), want,
                            plain):
        assert os.path.exists(path), path
        assert np.array_equal(_read_png(path), w.cpu().numpy()), path
        differ += int(not torch.equal(w, p))
  assert differ > 0                                   # the flags reached the filter
