"""--kitti_gt_everywhere on a ROCm device: lsi_augment_sample_u16
bit for bit its NumPy restatement (augment.sample_disparity_px, held to
data.load_disparity_px in test_kitti_gt_cpu.py), the prefetching loader's device
route against its host route, rasterising through augment_projection's matrix,
and one training step on the train split.  Every tree here is synthetic."""
import numpy as np
import pytest
import torch

import test_lidar_cpu as L
from test_kitti_gt_cpu import _map, gt_opts, make_gt_tree

pytestmark = pytest.mark.gpu

CANARY = 12345.0


def _sample(maps, windows, flips, ho, wo, gap=48, canaries=True):
  """One lsi_augment_sample_u16 launch on [descriptors | maps at 16-byte aligned
  offsets, `gap` bytes of 0xA5 between them]; `out` is pre-filled with NaN and,
  with `canaries`, lies between two planes that must stay untouched."""
  from lsi.data.kitti import pipeline
  n = len(maps)
  off = (n * pipeline.AUG_DESC_DTYPE.itemsize + 15) // 16 * 16
  offsets = []
  for m in maps:
    offsets.append(off)
    off = (off + m.nbytes + gap + 15) // 16 * 16
  buf = np.full(off + 16, 0xA5, np.uint8)
  for o, m in zip(offsets, maps):
    buf[o:o + m.nbytes] = np.ascontiguousarray(m, np.uint16).view(np.uint8).ravel()
  desc = pipeline.augment_desc([m.shape + (1,) for m in maps], offsets, windows, flips)
  buf[:desc.nbytes] = desc.view(np.uint8)
  packed = torch.from_numpy(buf).cuda()
  full = torch.full((n + 2, ho, wo, 1), float('nan'), device='cuda')
  full[0], full[n + 1] = CANARY, CANARY
  out = full[1:n + 1] if canaries else torch.full((n, ho, wo, 1), float('nan'), device='cuda')
  got = pipeline.augment_sample_u16(packed, desc, packed.data_ptr(), n, ho, wo, out=out)
  torch.cuda.synchronize()
  assert got.data_ptr() == out.data_ptr()
  if canaries:
    assert bool((full[0] == CANARY).all()) and bool((full[n + 1] == CANARY).all())
  return got


SIZES = [(23, 61), (24, 59), (22, 64), (25, 62), (9, 11), (40, 200)]
# each edge touched, one row, one column, narrower than the output, the whole map
WINDOWS = [(0, 3, 20, 50), (4, 0, 20, 59), (2, 24, 20, 40), (24, 5, 1, 50), (0, 10, 9, 1),
           (0, 0, 40, 200)]
FLIPS = [1, 0, 1, 0, 1, 0]


@pytest.mark.parametrize('wo', [40, 37])
def test_kernel_is_the_restatement_bit_for_bit(built_lib, wo):
  from lsi.data.kitti import augment
  ho = 16
  maps = [_map(h, w, seed=k) for k, (h, w) in enumerate(SIZES)]
  for m, (y0, x0, ch, cw) in zip(maps, WINDOWS):
    m[y0, x0], m[y0 + ch - 1, x0 + cw - 1] = 65535, 0
    assert y0 + ch <= m.shape[0] and x0 + cw <= m.shape[1]
  want = np.stack([augment.sample_disparity_px(m, win, bool(f), ho, wo)
                   for m, win, f in zip(maps, WINDOWS, FLIPS)])
  assert (want == 0).any() and (want == np.float32(65535 / 256.0 * (wo / 50.0))).any()
  got = _sample(maps, WINDOWS, FLIPS, ho, wo)
  assert got.shape == want.shape and not bool(torch.isnan(got).any())   # written fully
  assert torch.equal(got.cpu(), torch.from_numpy(want))
  # again, into a tensor of its own: the same bits
  assert torch.equal(_sample(maps, WINDOWS, FLIPS, ho, wo, canaries=False), got)
  # the full windows, unflipped: load_disparity_px's definition
  full = _sample(maps, None, None, ho, wo)
  for k, m in enumerate(maps):
    assert torch.equal(full[k].cpu(), torch.from_numpy(augment.sample_disparity_px(
        m, (0, 0) + m.shape, False, ho, wo)))
  # n = 1, mirrored
  one = _sample(maps[2:3], WINDOWS[2:3], [1], ho, wo)
  assert torch.equal(one[0].cpu(), torch.from_numpy(want[2]))
  assert torch.equal(_sample(maps[2:3], WINDOWS[2:3], [0], ho, wo),
                     torch.flip(one, dims=[2]))


def test_more_than_one_block_per_row_and_column(built_lib):
  """260 columns (65 quads: two blocks along a row) and 9 rows (three blocks of
  four rows), up- and down-sampled, both store paths."""
  from lsi.data.kitti import augment
  maps = [_map(30, 300, 1), _map(5, 90, 2)]
  wins, flips = [(1, 7, 28, 290), (0, 2, 5, 88)], [1, 1]
  for wo in (260, 258):
    got = _sample(maps, wins, flips, 9, wo)
    want = np.stack([augment.sample_disparity_px(m, w, True, 9, wo)
                     for m, w in zip(maps, wins)])
    assert torch.equal(got.cpu(), torch.from_numpy(want))


# ---------------------------------------------------------------------------
# the loaders
# ---------------------------------------------------------------------------
def _run(opts, resize, batches=3, workers=2):
  from lsi.data.kitti import data, pipeline
  got = []
  with pipeline.PrefetchLoader(data.DataLoader(opts), workers=workers, resize=resize,
                               prefetch_depth=1) as pre:
    for _ in range(batches):
      out = pre.forward(2)
      got.append(([t.cpu().numpy() if torch.is_tensor(t) else t for t in out],
                  [torch.is_tensor(t) and t.is_cuda for t in out], list(pre.src_image_names)))
  assert pre.workers_alive() == 0
  return got


@pytest.mark.parametrize('gt', ['px', 'velodyne', 'both'])
@pytest.mark.parametrize('aug', [True, False])
def test_device_route_is_the_host_route(built_lib, tmp_path, gt, aug):
  make_gt_tree(tmp_path)
  opts = gt_opts(tmp_path, px=gt != 'velodyne', velodyne=gt != 'px', augment=aug,
                 aug_seed=2, aug_zoom_max=1.5, aug_color_prob=0.5)
  host, dev = _run(opts, 'host'), _run(opts, 'device')
  n_out = {'px': 8, 'velodyne': 9, 'both': 11}[gt]
  on_device = [True, True] + [False] * 4 + {'px': [True, True], 'velodyne': [True, False, False],
                                            'both': [True, True, True, False, False]}[gt]
  flips = 0
  for (h, _, h_names), (d, d_cuda, d_names) in zip(host, dev):
    assert h_names == d_names and len(h) == len(d) == n_out
    assert d_cuda == on_device
    # (without augmentation the host route resizes the images in float32, a few
    # ulp from the device's exact sums: tests/test_kitti_pipeline_gpu.py; the
    # cameras and the ground truth are the same bits either way)
    for k in range(0 if aug else 2, n_out):
      assert h[k].dtype == d[k].dtype and h[k].shape == d[k].shape, k
      assert np.array_equal(h[k], d[k], equal_nan=h[k].dtype.kind == 'f'), k
    flips += int((h[5][:, 0, 0] > 0).sum())
  assert (0 < flips < 6) if aug else flips == 0
  # the synchronous loader gives the same batches
  from lsi.data.kitti import data
  sync = data.DataLoader(opts)
  for h, _, names in host:
    want = sync.forward(2)
    assert names == sync.src_image_names
    assert all(np.array_equal(a, b, equal_nan=a.dtype.kind == 'f') for a, b in zip(h, want))


# ---------------------------------------------------------------------------
# rasterising through an augmented matrix
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('cam', [2, 3])
def test_rasterising_through_the_augmented_matrix_is_the_crop(built_lib, tmp_path, cam, flip):
  """32 x 96 frames, the 16 x 48 window at (9, 29) -- scale 1 -- into a 16 x 48
  output: exactly the [9:25, 29:77] crop of the native 32 x 96 rasterisation
  (mirrored under a flip), because row 2 of the matrix, and so every depth, is
  untouched and every point projects a quarter pixel inside its cell."""
  from lsi.data.kitti import augment, data, velodyne
  from lsi.geometry import lidar
  top, _, _ = L._make_tree(tmp_path)
  calib = data.read_calib_file(str(top / 'calib_cam_to_cam.txt'))
  velo = velodyne.read_velo_calib(str(top / 'calib_velo_to_cam.txt'))
  H, W, h, w, y0, x0 = 32, 96, 16, 48, 9, 29
  p = calib['P_rect_0%d' % cam].reshape(3, 4)
  rs = np.random.RandomState(cam)
  n = 1200
  # area coordinates (column + 0.25, row + 0.25) of the native frame, inside
  # and around the window; depths 4 .. 60 m
  u = rs.randint(0, W, n) + 0.25
  v = rs.randint(0, H, n) + 0.25
  z = rs.uniform(4, 60, n)
  zc = z - p[2, 3]
  xc = ((u - 0.5) * z - p[0, 2] * zc - p[0, 3]) / p[0, 0]
  yc = ((v - 0.5) * z - p[1, 2] * zc - p[1, 3]) / p[1, 1]
  pts = (np.stack([xc, yc, zc], 1) - velo[1]) @ velo[0]          # R^T (X - T)
  pts = np.concatenate([pts, np.zeros((n, 1))], 1).astype(np.float32)
  native = velodyne.velo_to_image(calib, velo, cam, (H, W, 3), H, W)
  small = augment.augment_projection(
      velodyne.velo_to_image(calib, velo, cam, (H, W, 3), h, w), (H, W, 3),
      (y0, x0, h, w), flip, h, w)
  assert np.array_equal(small[2], native[2])
  dev = torch.device('cuda')
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
  whole = lidar.rasterize_points(t(pts[None]), None, [n], t(native.reshape(1, 1, 12)), H, W)
  part = lidar.rasterize_points(t(pts[None]), None, [n], t(small.reshape(1, 1, 12)), h, w)
  want = whole[:, :, y0:y0 + h, x0:x0 + w]
  if flip:
    want = torch.flip(want, dims=[3])
  assert 0.2 < float((want > 0).float().mean()) < 1.0
  assert torch.equal(part, want)


# ---------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------
def _trainer(root, ckpt, *extra):
  import ldi_enc_dec as script
  # 128 x 128: the smallest size of the training tests (tests/test_depth_sup_gpu.py)
  argv = ['--dataset', 'kitti', '--kitti_dataset_variant', 'raw_city', '--kitti_data_root',
          str(root), '--batch_size', '2', '--n_layers', '2', '--img_height', '128',
          '--img_width', '128', '--bf16', 'false', '--checkpoint_dir', str(ckpt),
          '--log_freq', '1000000', '--save_latest_freq', '1000000', '--checkpoint_freq',
          '1000000', '--aug_seed', '4', '--aug_zoom_max', '1.4'] + list(extra)
  opts = script.apply_dataset_overrides(script.build_parser().parse_args(argv))
  torch.manual_seed(0)
  np.random.seed(0)
  tr = script.Trainer(opts)
  tr.setup()
  return tr


@pytest.mark.parametrize('source', ['px', 'velodyne'])
def test_a_training_step_on_the_train_split(built_lib, tmp_path, source, monkeypatch):
  import ldi_enc_dec as script
  from lsi.data.kitti import data
  from lsi.geometry import lidar
  from lsi.loss import loss
  make_gt_tree(tmp_path / 'kitti', points=(400, 300, 500, None, 350))
  flag = '--kitti_dl_disparities_px' if source == 'px' else '--kitti_dl_velodyne'
  tr = _trainer(tmp_path / 'kitti', tmp_path / 'ckpt', '--depth_sup_wt', '1',
                '--kitti_gt_everywhere', 'true', '--kitti_augment', 'true',
                '--data_workers', '2', '--kitti_resize', 'device', flag, 'true')
  try:
    o, dev = tr.opts, tr.device
    assert o.data_split == 'train' and tr.depth_sup_source == source
    seen = []
    real = loss.depth_supervision_loss

    def spy(pred, gt, gt_scale=None, **kw):
      seen.append((pred.detach(), gt, gt_scale, kw))
      return real(pred, gt, gt_scale, **kw)

    monkeypatch.setattr(loss, 'depth_supervision_loss', spy)
    fed = tr.feed()
    assert fed[6][0] == source and fed[6][1].is_cuda
    staged, _ = tr.stage(fed)
    if source == 'px':
      # the sampling launch's [2 B, H, W, 1] tensor itself: no concatenation
      assert staged[4].shape == (4, 128, 128, 1)
      assert staged[4].data_ptr() == fed[6][1].data_ptr()
    _, scalars = tr.compute_losses(staged)
    got = float(scalars['depth_sup_loss'].detach())
    assert np.isfinite(got) and got > 0
    # the ground truth of the host-route batch drawn with the same seeds
    host = script.KittiBatches(data.DataLoader(o), tr.rank).forward(2)
    k_s, k_t, trans = (t.float() for t in (host[2], host[3], host[5]))
    scale = None
    if source == 'px':
      gt = torch.cat([host[6], host[7]], dim=0).to(dev)
      t_x = trans[:, 0, 0].abs()
      scale = torch.cat([1.0 / (k_s[:, 0, 0] * t_x), 1.0 / (k_t[:, 0, 0] * t_x)]).to(dev)
      assert torch.equal(staged[5], scale)
    else:
      inv = lidar.rasterize_points(host[6].to(dev), None, host[7], host[8].float().to(dev),
                                   128, 128, z_min=o.depth_sup_min, z_max=o.depth_sup_max,
                                   inverse=True)
      gt = torch.cat([inv[:, 0], inv[:, 1]], dim=0)
    assert torch.equal(staged[4], gt)
    assert 0.001 < float((gt > 0).float().mean()) < 0.9
    assert len(seen) in (1, 2)       # one call on the 2 B views (twice its mean), or two
    want = 0.0
    n = gt.shape[0] // len(seen)
    for k, (pred, _, _, kw) in enumerate(seen):
      part = slice(k * n, (k + 1) * n)
      want += (2.0 if len(seen) == 1 else 1.0) * float(real(
          pred, gt[part], None if scale is None else scale[part], **kw))
    print('depth_sup_loss (%s): %.9g, on the host-route ground truth %.9g' % (source, got, want))
    assert abs(got - want) <= 1e-6 * abs(want)
  finally:
    tr.data_loader.close()


def test_flag_off_and_weight_zero_is_the_step_without_either(built_lib, tmp_path):
  """The launches, the batch and the loss of an augmenting device-route step
  with `--kitti_gt_everywhere false --depth_sup_wt 0` against one that never
  sets either (the network pass pinned: test_depth_sup_gpu.py says why)."""
  from lsi.loss import _hip
  from test_depth_sup_gpu import SIX, _pin_network
  make_gt_tree(tmp_path / 'kitti')
  runs, pair = [], None
  common = ('--kitti_augment', 'true', '--data_workers', '2', '--kitti_resize', 'device')
  for i, extra in enumerate(((), ('--kitti_gt_everywhere', 'false', '--depth_sup_wt', '0'),
                             ('--kitti_gt_everywhere', 'true'))):
    tr = _trainer(tmp_path / 'kitti', tmp_path / str(i), *(common + extra))
    try:
      assert tr.depth_sup_source is None
      before = dict(_hip.CALLS)
      batch = tr.feed()
      assert len(batch) == 6
      staged, _ = tr.stage(batch)
      assert len(staged) == 4
      if pair is None:
        with torch.no_grad():
          tr.train_model(staged[0], staged[1])
        pair = [None if t is None else t.detach().clone() for t in tr.model.pair_ldi]
      _pin_network(tr, pair)
      total, scalars = tr.compute_losses(staged)
      assert set(scalars) == SIX
      calls = {k: v - before.get(k, 0) for k, v in _hip.CALLS.items() if v != before.get(k, 0)}
      runs.append((total.detach().clone(), [t.clone() for t in staged], calls,
                   {k: float(torch.as_tensor(v).detach()) for k, v in scalars.items()}))
      print('flag off, run %d (%s): %s' % (i, ' '.join(extra) or 'neither', runs[-1][3]))
    finally:
      tr.data_loader.close()
  for other in runs[1:]:
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], other[1]))
    assert other[2] == runs[0][2]
    assert torch.equal(runs[0][0], other[0]) and other[3] == runs[0][3]
  assert float(runs[0][0]) > 0 and 'depth_sup_fwd' not in runs[0][2]
