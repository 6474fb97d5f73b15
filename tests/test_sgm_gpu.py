"""The semi-global matcher on the device (csrc/lsi_sgm.hip through
lsi.geometry.stereo) against the NumPy restatement in tests/sgm_ref.py: both
outputs equal bit for bit, no tolerance -- everything is integer.

Shapes are the smallest at which each thing can go wrong: one pixel, one row,
one column (every path is a first pixel); a batch of 3 at D = 16 (idle lanes,
batch strides, both path counts); W < D; P2 = 193, where a path cost reaches
255; D = 48 and 80 (no multiple of 64) on grey input; D = 128 (the default: two
disparities per lane), 144, 176 and 192 (three per lane; at 176 the last lane
holds two, at 192 every lane is full) and 256 (four per lane, d0 up to 255), each wider than a group of prefetched
steps and than D; each switch; and a scene of constant blocks with ties of the
argmin.  The preprocessing tool runs end to end on the miniature KITTI
tree of tests/test_kitti_pipeline_cpu.py."""
import functools
import os

import numpy as np
import pytest
import torch

import sgm_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


# name -> (scene, (B, H, W, C), matcher arguments of sgm_ref.sgm_pair)
CASES = {
    'one_pixel': ('noise', (1, 1, 1, 1), dict(D=16)),
    'one_row': ('noise', (1, 1, 37, 3), dict(D=16)),
    'one_column': ('noise', (1, 29, 1, 3), dict(D=16)),
    'batch3_paths8': ('noise', (3, 24, 40, 3), dict(D=16)),
    'batch3_paths4': ('noise', (3, 24, 40, 3), dict(D=16, paths=4)),
    'narrower_than_d': ('noise', (1, 33, 20, 3), dict(D=32)),
    'saturation': ('noise', (1, 33, 70, 3), dict(D=64, p2=193)),
    'grey_d48': ('noise', (2, 19, 75, 1), dict(D=48)),
    'grey_d80': ('noise', (2, 19, 75, 1), dict(D=80)),
    'd128': ('noise', (1, 13, 150, 3), dict(D=128)),
    'd144': ('noise', (1, 11, 170, 1), dict(D=144)),
    'd192': ('noise', (1, 10, 210, 1), dict(D=192)),
    'd176_paths4': ('noise', (1, 11, 200, 1), dict(D=176, paths=4)),
    'd176': ('noise', (2, 9, 200, 3), dict(D=176)),
    'd256': ('noise', (1, 20, 300, 3), dict(D=256)),
    'd256_last_disparity': ('shift255', (1, 12, 300, 1), dict(D=256)),
    'no_lr_check': ('noise', (1, 24, 40, 3), dict(D=16, lr_max=-1)),
    'uniq100': ('noise', (1, 24, 40, 3), dict(D=16, uniq=100)),
    'uniq0': ('noise', (1, 24, 40, 3), dict(D=16, uniq=0)),
    'no_penalties': ('noise', (1, 24, 40, 3), dict(D=16, p1=0, p2=0)),
    'blocks': ('blocks', (1, 24, 40, 3), dict(D=16)),
    'blocks_grey_d32': ('blocks', (2, 19, 75, 1), dict(D=32)),
}


@functools.lru_cache(maxsize=None)
def case(name):
  """(left, right, kwargs, want_left, want_right, stats): computed once, left
  unchanged."""
  scene, shape, kw = CASES[name]
  seed = sorted(CASES).index(name) + 1
  if name == 'saturation':
    l, r, _, _ = R.step_scene(1, *shape[1:])       # the scene of tests/test_sgm_cpu.py
    left, right = l[None], r[None]
  elif scene == 'noise':
    left, right = R.noise_pair(seed, *shape)
  elif scene == 'shift255':
    left, right = R.shift_pair(seed, *shape, shift=255)
  else:
    left, right = R.block_pair(seed, *shape)
  stats = {}
  want_l, want_r = R.sgm_batch(left, right, stats=stats, **kw)
  for a in (left, right, want_l, want_r):
    a.setflags(write=False)
  return left, right, kw, want_l, want_r, stats


def run(dev, left, right, kw):
  from lsi.geometry import stereo
  kw = dict(kw)
  out = stereo.sgm_disparity(
      torch.from_numpy(np.array(left)).to(dev), torch.from_numpy(np.array(right)).to(dev),
      max_disp=kw.pop('D'), p1=kw.pop('p1', 10), p2=kw.pop('p2', 120),
      paths=kw.pop('paths', 8), uniqueness=kw.pop('uniq', 95), lr_max=kw.pop('lr_max', 1))
  assert not kw
  return out


def assert_same(got, want, what):
  got = got.cpu().numpy()
  assert got.dtype == np.uint16 and got.shape == want.shape
  if not np.array_equal(got, want):
    bad = np.argwhere(got != want)
    pytest.fail('%s: %d of %d pixels differ, first at %s: got %d, want %d' % (
        what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize('name', sorted(CASES))
def test_bit_exact(dev, name):
  left, right, kw, want_l, want_r, stats = case(name)
  if name == 'saturation':
    assert stats['max_path_cost'] == 255
  if name.startswith('blocks'):
    assert stats['argmin_ties'] > 50 and stats['tie_next'] > 0
  if name == 'd256_last_disparity':                  # d0 = D - 1 = 255: the largest value
    assert (want_l[:, 4:-4, 260:-5] == 255 * 256).all() and want_l.max() == 255 * 256
  if name in ('one_pixel', 'one_column'):            # x - d < 0 for every d > 0
    assert not want_l.any() and not want_r.any()
  else:
    assert want_l.any() and want_r.any()           # the case says something
  got_l, got_r = run(dev, left, right, kw)
  assert_same(got_l, want_l, name + ' left')
  assert_same(got_r, want_r, name + ' right')


def test_switches_change_the_answer():
  """Each switch of the cases above is one: the restatement's answers differ."""
  base = case('batch3_paths8')
  assert not np.array_equal(base[3], case('batch3_paths4')[3])
  plain = R.sgm_batch(*case('no_lr_check')[:2], D=16)
  for name in ('no_lr_check', 'uniq100', 'uniq0', 'no_penalties'):
    left, right, kw, want_l, _, _ = case(name)
    ref = R.sgm_batch(left, right, D=16)
    assert not np.array_equal(ref[0], want_l), name
  assert plain[0].any()


def test_unbatched_and_split_batches(dev, monkeypatch):
  from lsi.geometry import stereo
  left, right, kw, want_l, want_r, _ = case('batch3_paths8')
  one_l, one_r = run(dev, left[1], right[1], kw)
  assert one_l.shape == want_l.shape[1:]
  assert_same(one_l, want_l[1], 'single left')
  assert_same(one_r, want_r[1], 'single right')
  # a cap that holds two pairs: the batch of 3 is matched as 2 + 1
  per_pair = stereo.workspace_bytes(1, 24, 40, 3, 16, 8)
  monkeypatch.setattr(stereo, 'WORKSPACE_CAP', 2 * per_pair + 1)
  got_l, got_r = run(dev, left, right, kw)
  assert_same(got_l, want_l, 'split left')
  assert_same(got_r, want_r, 'split right')


def test_repeatable_and_on_a_side_stream(dev):
  left, right, kw, want_l, want_r, _ = case('grey_d80')
  a = run(dev, left, right, kw)
  b = run(dev, left, right, kw)
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
  side = torch.cuda.Stream(device=dev)
  torch.cuda.synchronize(dev)
  with torch.cuda.stream(side):
    c = run(dev, left, right, kw)
  side.synchronize()
  assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
  assert_same(c[0], want_l, 'side stream left')


def test_tool_end_to_end(dev, tmp_path):
  from PIL import Image
  from lsi.data.kitti import data as kitti
  from lsi.data.kitti import pipeline, preprocess
  from lsi.geometry import stereo
  from test_kitti_pipeline_cpu import OUT_H, OUT_W, make_opts, make_tree
  make_tree(tmp_path, 'val')                        # five pairs, each of its own size
  root = str(tmp_path)
  assert preprocess.main(['--kitti_data_root', root, '--max_disp', '16', '--workers', '4',
                          '--sequences', ','.join(kitti.raw_city_sequences())]) == 0
  opts = make_opts(tmp_path, 'val')
  opts.kitti_dl_disparities_px = True
  loader = kitti.DataLoader(opts)
  assert len(loader.img_list_src) == 5
  for i, name in enumerate(loader.img_list_src):
    left = torch.from_numpy(pipeline.decode_u8(name, 3).copy()).to(dev)
    right = torch.from_numpy(pipeline.decode_u8(loader.img_list_trg[i], 3).copy()).to(dev)
    want = stereo.sgm_disparity(left, right, max_disp=16)
    for path, w in zip((loader.img_list_disp_src[i], loader.img_list_disp_trg[i]), want):
      assert os.path.exists(path), path
      with Image.open(path) as im:
        assert im.mode in ('I;16', 'I;16B', 'I;16L')
        got = np.asarray(im).astype(np.uint16)
      assert np.array_equal(got, w.cpu().numpy()), path
  batch = loader.forward(2)
  assert len(batch) == 8 and batch[6].shape == (2, OUT_H, OUT_W, 1)
  assert batch[6].dtype == np.float32 and np.isfinite(batch[6]).all()
  # a second run finds everything in place and writes nothing
  stamp = {p: os.path.getmtime(p) for p in loader.img_list_disp_src}
  assert preprocess.run(root, max_disp=16, workers=2) == (0, 5)
  assert stamp == {p: os.path.getmtime(p) for p in loader.img_list_disp_src}
