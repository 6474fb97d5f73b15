"""The prefetching KITTI loader (lsi/data/kitti/pipeline.py) and the argument
checks of lsi_area_resize_u8, without a GPU: order and values against the
synchronous loader, decode errors, the C ABI's refusals before any launch, and
the integer AREA formula the GPU tests use as their oracle."""
import ctypes
import os
import time
import types

import numpy as np
import pytest

# five pairs of different sizes: ratios 1.4 - 1.6 to 16 x 40, rows of 183, 177,
# 192, 186, 180 bytes (most not dword-aligned)
SIZES = [(23, 61), (24, 59), (22, 64), (25, 62), (23, 60)]
OUT_H, OUT_W = 16, 40


def _calib_text(fx, fy, cx, cy, baseline2, baseline3):
  def p(b):
    return '%f 0 %f %f 0 %f %f 0 0 0 1 0' % (fx, cx, -fx * b, fy, cy)
  return ('calib_time: 09-Jan-2012 13:57:47\n'
          'P_rect_02: %s\nP_rect_03: %s\n' % (p(baseline2), p(baseline3)))


def make_opts(root, split='train', disparities=False, bs=2, h=OUT_H, w=OUT_W):
  return types.SimpleNamespace(
      batch_size=bs, kitti_data_root=str(root), kitti_dataset_variant='raw_city',
      data_split=split, img_height=h, img_width=w,
      kitti_dl_disparities=disparities)


def make_tree(root, split='train', disparities=False, sizes=SIZES):
  """A miniature raw_city tree: len(sizes) stereo pairs of one sequence of
  `split`, each pair of its own size; with `disparities` the 16-bit SPS-stereo
  maps of both views (left third empty, as a stereo matcher leaves it)."""
  from PIL import Image
  from lsi.data.kitti import data
  opts = make_opts(root, split, disparities)
  seq = data.DataLoader(opts).split_sequences()[0]
  date = seq[:10]
  top = os.path.join(str(root), 'kitti_raw')
  for n, (h, w) in enumerate(sizes):
    for cam in ('image_02', 'image_03'):
      path = os.path.join(top, date, seq + '_sync', cam, 'data', '%010d.png' % n)
      os.makedirs(os.path.dirname(path), exist_ok=True)
      rs = np.random.RandomState(10 * n + (cam == 'image_03'))
      Image.fromarray(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(path)
    if disparities:
      for side in ('left', 'right'):
        path = os.path.join(top, 'spss_stereo_results', seq + '_sync',
                            '%010d_%s_initial_disparity.png' % (n, side))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        rs = np.random.RandomState(100 + 10 * n + (side == 'right'))
        d = rs.randint(0, 65536, (h, w)).astype(np.uint16)
        d[:, :w // 3] = 0
        Image.fromarray(d).save(path)
  with open(os.path.join(top, date, 'calib_cam_to_cam.txt'), 'w') as f:
    f.write(_calib_text(700.0, 710.0, 30.0, 12.0, 0.06, 0.59))
  return opts


def exact_area(img_u8, ho, wo):
  """The exact rational AREA resize of a uint8 H x W x C image divided by 255:
  integer overlaps oy[i, y] = min((i+1) H, (y+1) Ho) - max(i H, y Ho) (columns
  alike), int64 sums, one float64 division by 255 H W."""
  img = np.asarray(img_u8)
  assert img.dtype == np.uint8 and img.ndim == 3
  h, w = img.shape[:2]

  def overlaps(n_in, n_out):
    i = np.arange(n_out, dtype=np.int64)[:, None]
    j = np.arange(n_in, dtype=np.int64)[None, :]
    return np.maximum(np.minimum((i + 1) * n_in, (j + 1) * n_out) -
                      np.maximum(i * n_in, j * n_out), 0)

  oy, ox = overlaps(h, ho), overlaps(w, wo)
  assert (oy.sum(1) == h).all() and (ox.sum(1) == w).all()
  s = np.einsum('iy,kx,yxc->ikc', oy, ox, img.astype(np.int64))
  return s.astype(np.float64) / (255.0 * h * w)


def _same_batches(a, b):
  assert len(a) == len(b)
  for u, v in zip(a, b):
    assert u.dtype == v.dtype and np.array_equal(u, v)


@pytest.mark.parametrize('rank', [0, 3])
@pytest.mark.parametrize('split,disparities', [('train', False), ('val', True)])
def test_threaded_host_loader_is_the_synchronous_one(tmp_path, rank, split,
                                                     disparities):
  from lsi.data.kitti import data, pipeline
  opts = make_tree(tmp_path, split, disparities)
  sync = data.DataLoader(opts)
  sync._rng = np.random.RandomState(rank)
  inner = data.DataLoader(opts)
  assert len(inner.img_list_src) == 5
  with pipeline.PrefetchLoader(inner, workers=4, resize='host') as pre:
    pre._rng = np.random.RandomState(rank)
    assert pre.n_threads == 4
    names = []
    for _ in range(5):              # two epochs of 5 samples in batches of 2
      want = sync.forward(2)
      got = pre.forward(2)
      assert len(got) == (8 if disparities else 6)
      _same_batches(got, want)
      assert pre.src_image_names == sync.src_image_names
      names += pre.src_image_names
    assert sorted(names[:5]) == sorted(sync.img_list_src)   # one whole epoch
    if disparities:
      assert got[6].shape == (2, OUT_H, OUT_W, 1) and float(got[6].max()) > 0
  assert pre.workers_alive() == 0


def test_pool_size_is_clamped_and_shared_by_the_ranks():
  from lsi.data.kitti import pipeline
  assert pipeline.pool_size(0) == 1 and pipeline.pool_size(4) == 4
  assert pipeline.pool_size(1000) == 16
  assert pipeline.pool_size(16, world_size=8) == 2
  assert pipeline.pool_size(4, world_size=8) == 1


def test_decode_errors_come_from_the_forward_that_owns_the_sample(tmp_path):
  from lsi.data.kitti import data, pipeline
  opts = make_tree(tmp_path)
  sync = data.DataLoader(opts)
  order = [int(i) for i in np.random.RandomState(0).permutation(5)]
  # batch 0 = order[0:2] is intact; batch 1 holds a missing target image,
  # batch 2 a truncated one
  missing = sync.img_list_trg[order[2]]
  truncated = sync.img_list_trg[order[4]]
  want = sync.forward(2)
  os.remove(missing)
  raw = open(truncated, 'rb').read()
  with open(truncated, 'wb') as f:
    f.write(raw[:len(raw) // 2])
  pre = pipeline.PrefetchLoader(data.DataLoader(opts), workers=4, resize='host')
  _same_batches(pre.forward(2), want)
  with pytest.raises(Exception) as e1:
    pre.forward(2)
  assert missing in str(e1.value)
  with pytest.raises(Exception) as e2:
    pre.forward(2)
  assert truncated in str(e2.value)
  t0 = time.monotonic()
  pre.close()
  assert time.monotonic() - t0 < 1.0
  assert pre.workers_alive() == 0
  with pytest.raises(RuntimeError, match='closed'):
    pre.forward(2)


def test_grey_image_where_rgb_is_needed_names_the_file(tmp_path):
  from PIL import Image
  from lsi.data.kitti import data, pipeline
  opts = make_tree(tmp_path, sizes=SIZES[:1])
  inner = data.DataLoader(opts)
  Image.fromarray(np.zeros((23, 61), np.uint8)).save(inner.img_list_src[0])
  with pipeline.PrefetchLoader(inner, workers=2) as pre:
    with pytest.raises(ValueError, match='channels') as e:
      pre.forward(1)
    assert inner.img_list_src[0] in str(e.value)


def test_decode_u8_follows_decode_png(tmp_path):
  """uint8 pixels of the staging route = the float pixels of the host route:
  RGB, 16-bit (high byte) and the first channel of an RGB file."""
  from PIL import Image
  from lsi.data.kitti import data, pipeline
  rs = np.random.RandomState(3)
  rgb, d16 = str(tmp_path / 'rgb.png'), str(tmp_path / 'd16.png')
  Image.fromarray(rs.randint(0, 256, (7, 9, 3), dtype=np.uint8)).save(rgb)
  Image.fromarray(rs.randint(0, 65536, (7, 9)).astype(np.uint16)).save(d16)
  for path, nc in ((rgb, 3), (rgb, 1), (d16, 1)):
    got = pipeline.decode_u8(path, nc)
    assert got.dtype == np.uint8
    assert np.array_equal(got.astype(np.float32), data.decode_png(path)[:, :, :nc])


def test_device_resize_on_a_cpu_run_is_refused(tmp_path, built_lib):
  import torch
  import ldi_enc_dec as script
  from lsi.data.kitti import data, pipeline
  opts = make_tree(tmp_path)
  if not torch.cuda.is_available():
    with pytest.raises(RuntimeError, match='ROCm GPU'):
      pipeline.PrefetchLoader(data.DataLoader(opts), workers=2, resize='device')
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    pipeline.area_resize_u8(torch.zeros(64, dtype=torch.uint8),
                            np.zeros(1, pipeline.DESC_DTYPE), 0, 1, 4, 4, 3)
  argv = ['--dataset', 'kitti', '--kitti_dataset_variant', 'raw_city',
          '--kitti_data_root', str(tmp_path), '--kitti_resize', 'device',
          '--cpu', 'true', '--checkpoint_dir', str(tmp_path / 'ckpt'),
          '--img_height', '16', '--img_width', '40']
  o = script.apply_dataset_overrides(script.build_parser().parse_args(argv))
  with pytest.raises(ValueError, match='--kitti_resize device'):
    script.Trainer(o).define_data_loader()


def test_default_switches_build_the_synchronous_loader(tmp_path):
  import ldi_enc_dec as script
  from lsi.data.kitti import data, pipeline
  make_tree(tmp_path)
  base = ['--dataset', 'kitti', '--kitti_dataset_variant', 'raw_city',
          '--kitti_data_root', str(tmp_path), '--cpu', 'true',
          '--checkpoint_dir', str(tmp_path / 'ckpt'), '--img_height', '16',
          '--img_width', '40']
  parse = lambda extra: script.apply_dataset_overrides(
      script.build_parser().parse_args(base + extra))
  o = parse([])
  assert o.data_workers == 0 and o.kitti_resize == 'host'
  tr = script.Trainer(o)
  tr.define_data_loader()
  assert type(tr.data_loader.loader) is data.DataLoader
  want = tr.feed()
  tr2 = script.Trainer(parse(['--data_workers', '3']))
  tr2.define_data_loader()
  assert isinstance(tr2.data_loader.loader, pipeline.PrefetchLoader)
  assert tr2.data_loader.loader.n_threads == 3
  got = tr2.feed()
  for u, v in zip(got, want):
    assert u.dtype == v.dtype and bool((u == v).all())
  assert tr2.data_loader.src_image_names == tr.data_loader.src_image_names
  tr2.data_loader.close()
  assert tr2.data_loader.loader.workers_alive() == 0
  import ldi_pred_eval
  e = ldi_pred_eval.build_parser().parse_args(['--data_workers', '2',
                                               '--kitti_resize', 'device'])
  assert e.data_workers == 2 and e.kitti_resize == 'device'


def test_resize_arguments_are_refused_before_any_launch(built_lib):
  from lsi import _C
  lib = _C.lib()
  EINVAL, ENULL = -1, -2

  def descs(*rows):
    arr = (_C.LsiImageDesc * len(rows))()
    for d, (off, h, w, c) in zip(arr, rows):
      d.offset, d.H, d.W, d.C = off, h, w, c
    return arr

  # (addresses that are never dereferenced: every call below is refused)
  dev, packed, out = 0x10000, 0x20000, 0x30000

  def call(d, n, packed_bytes, co, desc_dev=dev, pk=packed, o=out, ho=16, wo=40):
    host = ctypes.addressof(d) if d is not None else None
    return lib.lsi_area_resize_u8(n, host, desc_dev, pk, packed_bytes, ho, wo, co,
                                  o, None)

  ok = descs((0, 23, 61, 3))
  big = 1 << 30
  assert call(None, 1, big, 3) == ENULL
  assert call(ok, 1, big, 3, desc_dev=None) == ENULL
  assert call(ok, 1, big, 3, pk=None) == ENULL
  assert call(ok, 1, big, 3, o=None) == ENULL
  assert call(ok, 0, big, 3) == EINVAL                          # n = 0
  assert call(descs((0, 23, 61, 2)), 1, big, 2) == EINVAL       # C not in {1, 3}
  assert call(descs((0, 23, 61, 4)), 1, big, 4) == EINVAL
  assert call(descs((0, 23, 61, 1)), 1, big, 3) == EINVAL       # C != Co
  assert call(descs((0, 23, 61, 3), (4224, 23, 61, 1)), 2, big, 3) == EINVAL
  assert call(descs((0, 0, 61, 3)), 1, big, 3) == EINVAL        # sizes positive
  assert call(descs((0, 23, -1, 3)), 1, big, 3) == EINVAL
  assert call(ok, 1, big, 3, ho=0) == EINVAL
  # the extent passes packed_bytes: 23 * 61 * 3 = 4209 bytes from offset 16
  assert call(descs((16, 23, 61, 3)), 1, 4224, 3) == EINVAL
  assert call(descs((4240, 23, 61, 3)), 1, 4224, 3) == EINVAL   # offset itself
  assert call(descs((8, 23, 61, 3)), 1, big, 3) == EINVAL       # offset alignment
  assert call(descs((-16, 23, 61, 3)), 1, big, 3) == EINVAL
  # 5000 x 4000 = 20 000 000 > 16 843 009 pixels: 255 H W >= 2^32
  assert call(descs((0, 5000, 4000, 1)), 1, big, 1) == EINVAL
  assert call(descs((0, 4104, 4105, 1)), 1, big, 1) == EINVAL   # 16 846 920
  assert _C.LSI_IMAGE_MAX_PIXELS == 16843009
  assert 255 * 16843009 < 2 ** 32 <= 255 * 16843010
  assert ctypes.sizeof(_C.LsiImageDesc) == 24
  from lsi.data.kitti import pipeline
  assert pipeline.DESC_DTYPE.itemsize == 24
  assert [pipeline.DESC_DTYPE.fields[n][1] for n in ('offset', 'H', 'W', 'C')] == [
      getattr(_C.LsiImageDesc, n).offset for n in ('offset', 'H', 'W', 'C')]


def test_integer_formula_is_the_projects_area_resize():
  """The oracle of the GPU tests against the existing definition
  (data._area_matrix / area_resize), not against the kernel: the same weights
  in float64 agree to 1e-12, and the project's float32 route to its own bar."""
  from lsi.data.kitti import data
  rs = np.random.RandomState(5)
  img = rs.randint(0, 256, (23, 61, 3), dtype=np.uint8)
  got = exact_area(img, 16, 40)

  def area_matrix64(n_in, n_out):       # data._area_matrix without its float32 cast
    scale = n_in / float(n_out)
    m = np.zeros((n_out, n_in), np.float64)
    for i in range(n_out):
      lo, hi = i * scale, (i + 1) * scale
      j0, j1 = int(np.floor(lo)), min(int(np.ceil(hi)), n_in)
      for j in range(j0, j1):
        m[i, j] = min(hi, j + 1) - max(lo, j)
      m[i] /= scale
    return m

  for n_in, n_out in ((23, 16), (61, 40)):
    assert np.array_equal(area_matrix64(n_in, n_out).astype(np.float32),
                          data._area_matrix(n_in, n_out))
  x = img.astype(np.float64) * (1.0 / 255)
  want = np.tensordot(area_matrix64(23, 16), x, axes=(1, 0))
  want = np.tensordot(area_matrix64(61, 40), want, axes=(1, 1)).transpose(1, 0, 2)
  assert np.abs(got - want).max() <= 1e-12
  host = data.area_resize(img.astype(np.float32) * np.float32(1.0 / 255), 16, 40)
  assert np.abs(host - got).max() <= 1e-6
  # up-scaling and a mixed case through the same formula
  for (h, w) in ((9, 13), (40, 13)):
    small = rs.randint(0, 256, (h, w, 1), dtype=np.uint8)
    host = data.area_resize(small.astype(np.float32) * np.float32(1.0 / 255), 16, 40)
    assert np.abs(host - exact_area(small, 16, 40)).max() <= 1e-6


def test_collected_loader_and_exiting_interpreter_do_not_hang(tmp_path):
  import gc
  import subprocess
  import sys
  from conftest import PKG
  from lsi.data.kitti import data, pipeline
  opts = make_tree(tmp_path)
  pre = pipeline.PrefetchLoader(data.DataLoader(opts), workers=4)
  pre.forward(2)                       # two more batches are in flight
  threads = list(pre._pool._threads)
  assert threads
  del pre
  gc.collect()
  deadline = time.monotonic() + 5.0
  for t in threads:
    t.join(max(0.0, deadline - time.monotonic()))
  assert not any(t.is_alive() for t in threads)
  # an interpreter that leaves without close()
  code = ('import sys, types; sys.path.insert(0, %r)\n'
          'from lsi.data.kitti import data, pipeline\n'
          'o = types.SimpleNamespace(batch_size=2, kitti_data_root=%r, '
          "kitti_dataset_variant='raw_city', data_split='train', img_height=16, "
          'img_width=40, kitti_dl_disparities=False)\n'
          'p = pipeline.PrefetchLoader(data.DataLoader(o), workers=4)\n'
          "print(len(p.forward(2)), 'outputs')\n" % (PKG, str(tmp_path)))
  done = subprocess.run([sys.executable, '-c', code], capture_output=True,
                        text=True, timeout=60)
  assert done.returncode == 0, done.stderr
  assert '6 outputs' in done.stdout
