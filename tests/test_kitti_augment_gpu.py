"""lsi_augment_resize_u8 (csrc/lsi_image.hip) on a ROCm device: bit for bit
lsi_area_resize_u8 at identity parameters, bit for bit the NumPy restatement
(augment.augment_area_resize, held to the exact rational AREA resize in
test_kitti_augment_cpu.py) with windows, flips, tone tables and gains, and the
device route of the augmenting loader and of the trainer."""
import json

import numpy as np
import pytest
import torch

from test_kitti_pipeline_cpu import make_opts, make_tree
from test_kitti_pipeline_gpu import CANARY, CASES as PLAIN_CASES
from test_kitti_pipeline_gpu import _images, _pack as _pack_plain

pytestmark = pytest.mark.gpu


def _pack(images, tables=(), tight=False):
  """[descriptors | tables | images at 16-byte aligned offsets | pad]: the
  buffer, the image offsets and the tables' offset."""
  from lsi.data.kitti import pipeline
  n, nc = len(images), images[0].shape[2]
  t_off = (n * pipeline.AUG_DESC_DTYPE.itemsize + 15) // 16 * 16
  off = t_off + (len(tables) * nc * 256 + 15) // 16 * 16
  offsets = []
  for img in images:
    offsets.append(off)
    off = (off + img.size + 15) // 16 * 16
  buf = np.full(off + (0 if tight else 16), 0xA5, np.uint8)
  for m, t in enumerate(tables):
    buf[t_off + m * nc * 256:t_off + (m + 1) * nc * 256] = np.asarray(t, np.uint8).ravel()
  for o, img in zip(offsets, images):
    buf[o:o + img.size] = img.ravel()
  return buf, offsets, t_off


def _augment(images, ho, wo, windows=None, flips=None, table_ids=None, tables=(),
             gains=None, canaries=False, tight=False):
  from lsi.data.kitti import pipeline
  buf, offsets, t_off = _pack(images, tables, tight)
  desc = pipeline.augment_desc([im.shape for im in images], offsets, windows, flips,
                               table_ids, gains)
  if tight:
    assert offsets[-1] + images[-1].size == buf.size
  buf[:desc.nbytes] = desc.view(np.uint8)
  packed = torch.from_numpy(buf).cuda()
  n, nc = len(images), images[0].shape[2]
  args = (packed, desc, packed.data_ptr(), n, ho, wo, nc, t_off, len(tables))
  if not canaries:
    return pipeline.augment_resize_u8(*args)
  full = torch.full((n + 2, ho, wo, nc), CANARY, device='cuda')
  out = pipeline.augment_resize_u8(*args, out=full[1:n + 1])
  torch.cuda.synchronize()
  assert bool((full[0] == CANARY).all()) and bool((full[n + 1] == CANARY).all())
  return out


def _restate(images, ho, wo, windows=None, flips=None, table_ids=None, tables=(),
             gains=None):
  from lsi.data.kitti import augment
  out = []
  for m, img in enumerate(images):
    h, w, nc = img.shape
    t = None
    if table_ids is not None and table_ids[m] >= 0:
      t = tables[table_ids[m]]
    out.append(augment.augment_area_resize(
        img, windows[m] if windows is not None else (0, 0, h, w),
        bool(flips[m]) if flips is not None else False, t,
        gains[m] if gains is not None else np.ones(nc, np.float32), ho, wo))
  return np.stack(out)


# ---------------------------------------------------------------------------
# identity parameters: the plain kernel's bits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('nc', [3, 1])
@pytest.mark.parametrize('case', ['ragged_batch', 'tile_edge', 'tile_edge_wide_vec',
                                  'large_ratio'])
def test_identity_parameters_give_the_plain_resize(built_lib, case, nc):
  from lsi.data.kitti import pipeline
  sizes, ho, wo = PLAIN_CASES[case]
  images = _images(sizes, nc, seed=len(case))
  buf, desc = _pack_plain(images)
  packed = torch.from_numpy(buf).cuda()
  plain = pipeline.area_resize_u8(packed, desc, packed.data_ptr(), len(images), ho,
                                  wo, nc)
  assert torch.equal(_augment(images, ho, wo), plain)
  # ... and with an identity table that is looked up
  ident = [np.broadcast_to(np.arange(256, dtype=np.uint8), (nc, 256))]
  assert torch.equal(_augment(images, ho, wo, table_ids=[0] * len(images),
                              tables=ident), plain)


# ---------------------------------------------------------------------------
# bit equality with the restatement
# ---------------------------------------------------------------------------
def _perm_tables(rs, n, nc):
  return [np.stack([rs.permutation(256) for _ in range(nc)]).astype(np.uint8)
          for _ in range(n)]


def _case(name, nc):
  """(images, ho, wo, keyword arguments, tight) of a named case."""
  rs = np.random.RandomState(len(name) + nc)
  tight = False
  if name == 'lds_phase':
    # x0 C = 9 or 3 and the row pitch 183 or 61 are no multiples of 16
    sizes, ho, wo = [(23, 61)], 16, 40
    kw = dict(windows=[(0, 3, 23, 50)])
  elif name == 'window_ends_on_the_last_byte':
    # a tight buffer; the last image's window holds its last pixel
    sizes, ho, wo = ([(23, 61), (16, 40)] if nc == 3 else [(23, 61), (32, 16)]), 16, 40
    kw = dict(windows=[(1, 2, 20, 57),
                       (4, 10, 12, 30) if nc == 3 else (8, 4, 24, 12)])
    tight = True
  elif name == 'flip_tile_edge':          # Wo = 70 is no multiple of the tile
    sizes, ho, wo = PLAIN_CASES['tile_edge']
    kw = dict(flips=[1, 1], windows=[(0, 0, 29, 113), (2, 5, 22, 90)])
  elif name == 'flip_wide_scalar_stores':  # one channel: 150 % 4 != 0
    sizes, ho, wo = PLAIN_CASES['tile_edge_wide']
    kw = dict(flips=[1, 1], windows=[(0, 0, 20, 200), (1, 7, 19, 221)])
  elif name == 'flip_wide_vector_stores':  # one channel: float4, reversed
    sizes, ho, wo = PLAIN_CASES['tile_edge_wide_vec']
    kw = dict(flips=[1], windows=[(1, 3, 18, 180)])
  elif name == 'nine_images':
    sizes, ho, wo = PLAIN_CASES['nine_images']
    wins = []
    for h, w in sizes:
      ch, cw = rs.randint(h // 2, h + 1), rs.randint(w // 2, w + 1)
      wins.append((rs.randint(0, h - ch + 1), rs.randint(0, w - cw + 1), ch, cw))
    kw = dict(windows=wins, flips=[1, 0, 0, 1, 1, 0, 1, 0, 1])
  elif name == 'chunk_loop':              # 64 x 126 input pixels under one tile
    sizes, ho, wo = PLAIN_CASES['large_ratio']
    kw = dict(windows=[(2, 3, 64, 126)], flips=[1])
  elif name == 'upscaling_window':        # ch < Ho, cw < Wo
    sizes, ho, wo = [(23, 61), (24, 59)], 16, 40
    kw = dict(windows=[(5, 10, 9, 20), (0, 30, 24, 29)], flips=[0, 1])
  elif name == 'permutation_tables':
    # different per channel and per image: a swapped index shows
    sizes, ho, wo = PLAIN_CASES['ragged_batch']
    kw = dict(tables=_perm_tables(rs, 3, nc), table_ids=[2, 0, 1],
              windows=[(0, 3, 23, 50), (1, 0, 22, 59), (0, 0, 22, 64)],
              flips=[0, 1, 0])
  elif name == 'tables_on_some_images':
    sizes, ho, wo = PLAIN_CASES['ragged_batch']
    kw = dict(tables=_perm_tables(rs, 2, nc), table_ids=[-1, 1, 0])
  elif name == 'clamping_gains':
    sizes, ho, wo = PLAIN_CASES['ragged_batch']
    kw = dict(gains=[(1.6, 2.2, 0.9)[:nc], (2.0, 0.0, 1.7)[:nc], (1.9, 1.5, 0.3)[:nc]],
              flips=[0, 1, 0])
  elif name == 'everything':
    sizes, ho, wo = PLAIN_CASES['tile_edge']
    kw = dict(windows=[(3, 7, 24, 100), (0, 1, 25, 99)], flips=[1, 0],
              tables=_perm_tables(rs, 2, nc), table_ids=[1, 0],
              gains=[(1.7, 0.6, 2.4)[:nc], (1.8, 1.0, 0.5)[:nc]])
  else:
    raise KeyError(name)
  return _images(sizes, nc, seed=len(name)), ho, wo, kw, tight


NAMES = ['lds_phase', 'window_ends_on_the_last_byte', 'flip_tile_edge',
         'flip_wide_scalar_stores', 'flip_wide_vector_stores', 'nine_images',
         'chunk_loop', 'upscaling_window', 'permutation_tables',
         'tables_on_some_images', 'clamping_gains', 'everything']


@pytest.mark.parametrize('nc', [3, 1])
@pytest.mark.parametrize('name', NAMES)
def test_kernel_is_the_restatement_bit_for_bit(built_lib, name, nc):
  images, ho, wo, kw, tight = _case(name, nc)
  want = _restate(images, ho, wo, **kw)
  if 'gains' in kw:
    # the case is only worth its name if the restatement itself clamps some
    # values of every image and leaves others
    base = _restate(images, ho, wo, **{k: v for k, v in kw.items() if k != 'gains'})
    for m, w in enumerate(want):
      unclamped = base[m] * np.asarray(kw['gains'][m], np.float32)
      assert (unclamped > 1).any() and (unclamped < 1).any() and w.max() == 1
  out = _augment(images, ho, wo, tight=tight, **kw)
  got = out.cpu().numpy()
  assert got.shape == want.shape and got.dtype == np.float32
  bad = np.argwhere(got != want)
  assert bad.size == 0, 'first of %d differing values at %s: %r != %r' % (
      len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
  # between canary planes (where the slice is not 16-byte aligned: through the
  # scalar stores): the same bits, nothing outside; and again: the same bits
  assert torch.equal(_augment(images, ho, wo, canaries=True, tight=tight, **kw), out)
  assert torch.equal(_augment(images, ho, wo, tight=tight, **kw), out)


def test_flip_is_the_mirror_of_the_unflipped_output(built_lib):
  for case, nc in (('tile_edge', 3), ('tile_edge_wide', 1), ('tile_edge_wide_vec', 1)):
    sizes, ho, wo = PLAIN_CASES[case]
    images = _images(sizes, nc, seed=3)
    plain = _augment(images, ho, wo)
    flipped = _augment(images, ho, wo, flips=[1] * len(images))
    assert torch.equal(flipped, torch.flip(plain, dims=[2]))


# ---------------------------------------------------------------------------
# loader and trainer
# ---------------------------------------------------------------------------
def _ragged_pair_tree(root):
  """make_tree's tree with the right images of other sizes than the left."""
  from PIL import Image
  from lsi.data.kitti import data
  opts = make_tree(root)
  for n, path in enumerate(sorted(data.DataLoader(opts).img_list_trg)):
    rs = np.random.RandomState(50 + n)
    Image.fromarray(rs.randint(0, 256, (22 + n % 3, 58 + n, 3), dtype=np.uint8)).save(path)
  return opts


def _aug_opts(root, **kw):
  o = make_opts(root)
  o.kitti_augment = True
  for k, v in kw.items():
    setattr(o, k, v)
  return o


def _run(opts, resize, batches=4):
  from lsi.data.kitti import data, pipeline
  got = []
  with pipeline.PrefetchLoader(data.DataLoader(opts), workers=2, resize=resize,
                               prefetch_depth=1) as pre:
    for _ in range(batches):
      out = pre.forward(2)
      if resize == 'device':
        assert all(t.is_cuda and t.dtype == torch.float32 for t in out[:2])
      got.append(([t.cpu().numpy() if torch.is_tensor(t) else t for t in out],
                  list(pre.src_image_names)))
  assert pre.workers_alive() == 0
  return got


def test_device_loader_augments_like_the_host_route(built_lib, tmp_path):
  _ragged_pair_tree(tmp_path)
  opts = _aug_opts(tmp_path, aug_seed=2, aug_zoom_max=1.4, aug_color_prob=0.7)
  host, dev = _run(opts, 'host'), _run(opts, 'device')
  flips = 0
  for (h, h_names), (d, d_names) in zip(host, dev):
    assert h_names == d_names and len(h) == len(d) == 6
    for k in range(6):
      assert h[k].dtype == d[k].dtype and np.array_equal(h[k], d[k]), k
    flips += int((h[5][:, 0, 0] > 0).sum())     # the baseline's sign
  assert 0 < flips < 8


def test_device_loader_flip_is_the_mirror(built_lib, tmp_path):
  _ragged_pair_tree(tmp_path)
  # the whole image is a symmetric window: flip 1 and flip 0 mirror each other,
  # colour included (the draws do not shift)
  kw = dict(aug_seed=4, aug_zoom_max=1.0, aug_color_prob=0.6)
  on = _run(_aug_opts(tmp_path, aug_flip_prob=1.0, **kw), 'device', 3)
  off = _run(_aug_opts(tmp_path, aug_flip_prob=0.0, **kw), 'device', 3)
  for (a, a_names), (b, b_names) in zip(on, off):
    assert a_names == b_names
    for k in (0, 1):
      assert np.array_equal(a[k], np.flip(b[k], axis=2))
      assert np.array_equal(b[k], np.flip(a[k], axis=2))
    assert np.array_equal(a[5][:, 0], -b[5][:, 0])
    assert np.array_equal(a[2][:, 0, 2], 40 - b[2][:, 0, 2])


def test_trainer_trains_from_the_augmenting_device_loader(built_lib, tmp_path, capsys):
  import ldi_enc_dec as script
  from lsi import _C
  make_tree(tmp_path)
  argv = ['--dataset', 'kitti', '--kitti_dataset_variant', 'raw_city',
          '--kitti_data_root', str(tmp_path), '--data_workers', '2',
          '--kitti_resize', 'device', '--n_layers', '2', '--batch_size', '2',
          '--img_height', '128', '--img_width', '384', '--num_iter', '2',
          '--log_freq', '1', '--checkpoint_dir', str(tmp_path / 'ckpt'),
          '--kitti_augment', 'true']
  parse = lambda a: script.apply_dataset_overrides(script.build_parser().parse_args(a))
  # the renderer's kernel family for a flipped and an unflipped batch
  plans, mats = [], []
  for prob in ('1', '0'):
    tr = script.Trainer(parse(argv + ['--aug_flip_prob', prob]))
    tr.device = torch.device('cuda', 0)
    tr.define_data_loader()
    _, plan = tr.stage(tr.feed())
    tr.data_loader.close()
    plans.append([p[0] for p in plan])
    mats.append(tr.host_mats['trg'])
  assert plans[0] == plans[1] == [_C.LSI_PATH_STREAM] * 2
  assert not torch.equal(mats[0], mats[1])
  capsys.readouterr()
  trainer = script.main(argv)
  lines = [json.loads(l) for l in capsys.readouterr().out.splitlines()
           if l.startswith('{')]
  assert [l['iter'] for l in lines] == [1, 2]
  assert all(np.isfinite(l['total_loss']) for l in lines)
  assert trainer.data_loader.loader.workers_alive() == 0
