"""lsi_area_resize_u8 (csrc/lsi_image.hip) against the exact rational AREA
resize, and the device route of the prefetching KITTI loader and of the trainer
against the host route, on a ROCm device.

Kernel bound: |out - exact| <= 2^-22 max(exact, 2^-24) -- 4 ulp: the derived
1.5 ulp (one rounding in the int-to-float conversion, one in the multiply) plus
room for the rounded reciprocal.  `exact` is test_kitti_pipeline_cpu.exact_area
(int64 sums, one float64 division), pinned there to data.area_resize."""
import json

import numpy as np
import pytest
import torch

from test_kitti_pipeline_cpu import exact_area, make_tree

pytestmark = pytest.mark.gpu

CANARY = -7.0


def _pack(images, tight=False):
  """[descriptors | images at 16-byte aligned offsets | pad].  tight: the buffer
  ends at the last image's last byte rounded up to 16 and no further."""
  from lsi.data.kitti import pipeline
  n = len(images)
  header = (n * pipeline.DESC_DTYPE.itemsize + 15) // 16 * 16
  desc = np.zeros(n, pipeline.DESC_DTYPE)
  off = header
  for m, img in enumerate(images):
    desc[m] = (off, img.shape[0], img.shape[1], img.shape[2], 0)
    off = (off + img.size + 15) // 16 * 16
  buf = np.full(off + (0 if tight else 16), 0xA5, np.uint8)
  buf[:header].view(np.uint8)[:n * desc.itemsize] = desc.view(np.uint8)
  for d, img in zip(desc, images):
    buf[d['offset']:d['offset'] + img.size] = img.ravel()
  return buf, desc


def _resize(images, ho, wo, canaries=False, tight=False):
  from lsi.data.kitti import pipeline
  buf, desc = _pack(images, tight)
  packed = torch.from_numpy(buf).cuda()
  n, nc = len(images), images[0].shape[2]
  if not canaries:
    return pipeline.area_resize_u8(packed, desc, packed.data_ptr(), n, ho, wo, nc)
  # the output between two canary rows of one image each
  full = torch.full((n + 2, ho, wo, nc), CANARY, device='cuda')
  out = pipeline.area_resize_u8(packed, desc, packed.data_ptr(), n, ho, wo, nc,
                                out=full[1:n + 1])
  torch.cuda.synchronize()
  assert bool((full[0] == CANARY).all()) and bool((full[n + 1] == CANARY).all())
  return out


def _check(out, images, ho, wo):
  got = out.cpu().numpy().astype(np.float64)
  assert got.shape == (len(images), ho, wo, images[0].shape[2])
  worst = 0.0
  for g, img in zip(got, images):
    exact = exact_area(img, ho, wo)
    ratio = np.abs(g - exact) / np.maximum(exact, 2.0 ** -24)
    worst = max(worst, float(ratio.max()))
  print('worst |out - exact| / max(exact, 2^-24) = %.3g (bound %.3g)' %
        (worst, 2.0 ** -22))
  assert worst <= 2.0 ** -22


def _images(sizes, nc, seed=0):
  rs = np.random.RandomState(seed)
  return [rs.randint(0, 256, (h, w, nc), dtype=np.uint8) for h, w in sizes]


CASES = {
    'box_2x2': ([(32, 96)], 16, 48),
    'ragged_batch': ([(23, 61), (24, 59), (22, 64)], 16, 40),
    'identity': ([(16, 40)], 16, 40),
    'upscale': ([(9, 13)], 16, 40),
    'mixed': ([(40, 13)], 16, 40),
    'large_ratio': ([(67, 131)], 16, 24),
    'tile_edge': ([(29, 113), (26, 101)], 17, 70),
    # one-channel tiles are 128 pixels wide: an edge inside, scalar / float4 stores
    'tile_edge_wide': ([(20, 200), (21, 233)], 17, 150),
    'tile_edge_wide_vec': ([(20, 190)], 9, 132),
    'nine_images': ([(23, 61), (24, 59), (22, 64), (25, 62), (23, 60), (21, 57),
                     (26, 66), (22, 58), (24, 63)], 16, 40),
}


@pytest.mark.parametrize('nc', [3, 1])
@pytest.mark.parametrize('case', sorted(CASES))
def test_resize_is_the_exact_area_mean(built_lib, case, nc):
  sizes, ho, wo = CASES[case]
  images = _images(sizes, nc, seed=len(case))
  out = _resize(images, ho, wo)
  _check(out, images, ho, wo)
  # between canaries (and, where the slice is not 16-byte aligned, through the
  # scalar stores): the same bits; and again: the same bits
  assert torch.equal(_resize(images, ho, wo, canaries=True), out)
  assert torch.equal(_resize(images, ho, wo), out)
  if case == 'box_2x2':
    box = images[0].astype(np.float64).reshape(16, 2, 48, 2, nc).mean(axis=(1, 3))
    assert np.abs(out[0].cpu().numpy() - box / 255).max() <= 2.0 ** -22


@pytest.mark.parametrize('nc', [3, 1])
def test_last_image_ends_at_the_buffers_last_byte(built_lib, nc):
  # 16 x 40 x 3 and 32 x 16 x 1 bytes are multiples of 16: the buffer ends with
  # the image, without a pad; the first image's rows are not dword-aligned
  sizes = [(23, 61), (16, 40)] if nc == 3 else [(23, 61), (32, 16)]
  images = _images(sizes, nc, seed=9)
  buf, desc = _pack(images, tight=True)
  assert int(desc[-1]['offset']) + images[-1].size == buf.size
  _check(_resize(images, 16, 40, tight=True), images, 16, 40)


@pytest.mark.parametrize('value', [0, 1, 254, 255])
def test_constant_images_keep_their_value(built_lib, value):
  images = [np.full((h, w, 3), value, np.uint8) for h, w in CASES['ragged_batch'][0]]
  out = _resize(images, 16, 40)
  _check(out, images, 16, 40)        # exact = value / 255: the weights sum to 1
  want = np.float32(value / 255.0)
  assert float((out - float(want)).abs().max()) <= 2.0 ** -22 * max(want, 2.0 ** -24)
  if value == 0:
    assert bool((out == 0).all())


def test_empty_regions_stay_exactly_zero(built_lib):
  from lsi.data.kitti import data
  rs = np.random.RandomState(4)
  img = rs.randint(1, 256, (22, 64, 1), dtype=np.uint8)
  img[:, :64 // 3] = 0
  out = _resize([img], 16, 40)[0].cpu().numpy()
  host = data.area_resize(img.astype(np.float32) * np.float32(1.0 / 255), 16, 40)
  assert (host == 0).any() and (host != 0).any()
  assert np.array_equal(out == 0, host == 0)
  assert np.array_equal(out == 0, exact_area(img, 16, 40) == 0)


# ---------------------------------------------------------------------------
# loader and trainer
# ---------------------------------------------------------------------------
TOL = 1e-6 + 2.0 ** -22   # the host path's bar (test_data_cpu.py) + the kernel's


def _run_device_loader(opts, batches, depth):
  from lsi.data.kitti import data, pipeline
  got = []
  with pipeline.PrefetchLoader(data.DataLoader(opts), workers=2, resize='device',
                               prefetch_depth=depth) as pre:
    for _ in range(batches):
      out = pre.forward(2)
      assert all(t.is_cuda and t.dtype == torch.float32
                 for t in out[:2] + out[6:])
      assert all(isinstance(a, np.ndarray) for a in out[2:6])
      # (read back at once: the next batches' decodes then overlap the copies)
      got.append(([t.cpu().numpy() if torch.is_tensor(t) else t for t in out],
                  list(pre.src_image_names)))
  assert pre.workers_alive() == 0
  return got


@pytest.fixture(scope='module')
def val_tree(tmp_path_factory):
  return make_tree(tmp_path_factory.mktemp('kitti_val'), 'val', True)


@pytest.fixture(scope='module')
def host_batches(val_tree):
  from lsi.data.kitti import data
  sync = data.DataLoader(val_tree)
  out = []
  for _ in range(6):
    out.append((sync.forward(2), list(sync.src_image_names)))
  return out


def _compare(got, want):
  for (g, g_names), (w, w_names) in zip(got, want):
    assert g_names == w_names
    assert len(g) == len(w) == 8
    for k in (2, 3, 4, 5):
      assert np.array_equal(g[k], w[k])
    for k in (0, 1, 6, 7):
      assert g[k].shape == w[k].shape
      assert np.abs(g[k] - w[k]).max() <= TOL
    for k in (6, 7):                 # ldi_pred_eval's `disp == 0` mask
      assert np.array_equal(g[k] == 0, w[k] == 0)


def test_device_loader_is_the_synchronous_one(built_lib, val_tree, host_batches):
  got = _run_device_loader(val_tree, 5, depth=2)    # two epochs of 5 in twos
  _compare(got, host_batches[:5])
  # one batch ahead, six batches: every staging buffer is used again
  again = _run_device_loader(val_tree, 6, depth=1)
  _compare(again, host_batches)
  for (g, _), (a, _) in zip(got, again):
    for u, v in zip(g, a):
      assert np.array_equal(u, v)


def test_trainer_trains_from_the_device_loader(built_lib, tmp_path, capsys):
  import ldi_enc_dec as script
  make_tree(tmp_path)
  argv = ['--dataset', 'kitti', '--kitti_dataset_variant', 'raw_city',
          '--kitti_data_root', str(tmp_path), '--data_workers', '2',
          '--kitti_resize', 'device', '--n_layers', '2', '--batch_size', '2',
          '--img_height', '128', '--img_width', '384', '--num_iter', '2',
          '--log_freq', '1', '--checkpoint_dir', str(tmp_path / 'ckpt')]
  parse = lambda a: script.apply_dataset_overrides(script.build_parser().parse_args(a))
  # what is staged for the first batch, by both routes (no model needed)
  staged = []
  for extra in ([], ['--data_workers', '0', '--kitti_resize', 'host']):
    tr = script.Trainer(parse(argv + extra))
    tr.device = torch.device('cuda', 0)
    tr.define_data_loader()
    s, _ = tr.stage(tr.feed())
    staged.append([t.cpu() for t in s])
    names = tr.data_loader.src_image_names
    tr.data_loader.close()
    staged.append(names)
  assert staged[1] == staged[3]
  for u, v in zip(staged[0], staged[2]):
    assert u.shape == v.shape and float((u - v).abs().max()) <= TOL
  assert torch.equal(staged[0][2], staged[2][2])      # the projection matrices
  capsys.readouterr()
  trainer = script.main(argv)
  lines = [json.loads(l) for l in capsys.readouterr().out.splitlines()
           if l.startswith('{')]
  assert [l['iter'] for l in lines] == [1, 2]
  assert all(np.isfinite(l['total_loss']) for l in lines)
  assert trainer.data_loader.loader.workers_alive() == 0
