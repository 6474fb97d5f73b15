"""--kitti_gt_everywhere without a GPU: the restatement of
lsi_augment_sample_u16 against data.load_disparity_px and by hand, the scale
convention of augmented pixel disparities, augment_projection against the
augmented intrinsics, the synchronous and the prefetching loader (host route)
on a synthetic raw_city tree, and the C entry point's refusals before any
launch.  No KITTI data is used anywhere: every tree here is synthetic."""
import ctypes
import os
import types

import numpy as np
import pytest

import test_kitti_pipeline_cpu as P
import test_lidar_cpu as L

OUT_H, OUT_W = P.OUT_H, P.OUT_W
# points per frame of make_gt_tree; None = the frame has no scan file
POINTS = (5, 0, 9, None, 3)


def gt_opts(root, split='train', px=False, velodyne=False, everywhere=True, augment=False,
            bs=2, h=OUT_H, w=OUT_W, **kw):
  o = dict(batch_size=bs, kitti_data_root=str(root), kitti_dataset_variant='raw_city',
           data_split=split, img_height=h, img_width=w, kitti_dl_disparities_px=px,
           kitti_dl_velodyne=velodyne, kitti_augment=augment)
  if everywhere is not None:
    o['kitti_gt_everywhere'] = everywhere
  o.update(kw)
  return types.SimpleNamespace(**o)


def make_gt_tree(root, split='train', sizes=P.SIZES, points=POINTS, spread=1.0):
  """test_kitti_pipeline_cpu.make_tree with 16-bit maps, plus a rectifying
  rotation, calib_velo_to_cam.txt and one scan per frame (points[n] points in
  front of the cameras; None: no file)."""
  from lsi.data.kitti import data
  P.make_tree(root, split, True, sizes)
  seq = data.DataLoader(P.make_opts(root, split)).split_sequences()[0]
  top = os.path.join(str(root), 'kitti_raw', seq[:10])
  with open(os.path.join(top, 'calib_cam_to_cam.txt'), 'a') as f:
    f.write('R_rect_00: 1 0 0 0 1 0 0 0 1\n')
  with open(os.path.join(top, 'calib_velo_to_cam.txt'), 'w') as f:
    f.write('calib_time: 15-Mar-2012 11:37:16\nR: 0 -1 0 0 0 -1 1 0 0\n'
            'T: 0.01 -0.07 -0.27\n')
  vdir = os.path.join(top, seq + '_sync', 'velodyne_points', 'data')
  os.makedirs(vdir, exist_ok=True)
  scans = {}
  for n, count in enumerate(points[:len(sizes)]):
    if count is None:
      continue
    rs = np.random.RandomState(50 + n)
    # scanner frame: x forward 5 .. 40 m, a narrow cone around the axis
    x = rs.uniform(5, 40, count)
    scans[n] = np.stack([x, rs.uniform(-0.04, 0.04, count) * x * spread,
                         rs.uniform(-0.015, 0.015, count) * x * spread,
                         rs.uniform(0, 1, count)], 1).astype(np.float32)
    scans[n].tofile(os.path.join(vdir, '%010d.bin' % n))
  return top, seq, scans


def _map(h, w, seed=0):
  rs = np.random.RandomState(seed)
  raw = rs.randint(0, 65536, (h, w)).astype(np.uint16)
  raw[:, :w // 3] = 0
  raw[-1, -1] = 65535
  return raw


# --- the restatement ------------------------------------------------------------
@pytest.mark.parametrize('size,out', [(s, (OUT_H, OUT_W)) for s in P.SIZES] +
                         [((9, 11), (16, 40)), ((9, 11), (27, 33)), ((5, 7), (16, 41)),
                          ((1, 1), (3, 5)), ((23, 61), (23, 61))])
def test_full_window_is_load_disparity_px(tmp_path, size, out):
  from PIL import Image
  from lsi.data.kitti import augment, data
  raw = _map(size[0], size[1], seed=size[0] * size[1])
  path = str(tmp_path / 'd.png')
  Image.fromarray(raw).save(path)
  want = data.load_disparity_px(path, out[0], out[1])
  assert np.array_equal(data.decode_u16(path), raw)
  got = augment.sample_disparity_px(data.decode_u16(path), (0, 0) + size, False, *out)
  assert got.dtype == np.float32 and got.shape == out + (1,)
  assert np.array_equal(got, want)
  assert (got[raw[np.minimum((np.arange(out[0]) * 2 + 1) * size[0] // (2 * out[0]),
                             size[0] - 1)][:, np.minimum(
                                 (np.arange(out[1]) * 2 + 1) * size[1] // (2 * out[1]),
                                 size[1] - 1)] == 0] == 0).all()


def test_window_and_flip_by_hand():
  from lsi.data.kitti import augment
  raw = np.array([[1, 2, 3, 4, 5, 6],
                  [7, 8, 0, 65535, 256, 12],
                  [13, 14, 512, 0, 384, 18],
                  [19, 20, 21, 22, 23, 24]], np.uint16)
  # rows 1, 2 and columns 2, 3, 4 of the map, at scale 3 / 3, mirrored
  got = augment.sample_disparity_px(raw, (1, 2, 2, 3), True, 2, 3)
  want = np.array([[1.0, 65535 / 256.0, 0.0], [1.5, 0.0, 2.0]], np.float32)
  assert np.array_equal(got[:, :, 0], want)
  assert np.array_equal(augment.sample_disparity_px(raw, (1, 2, 2, 3), False, 2, 3)[:, :, 0],
                        want[:, ::-1])
  # twice as wide: every pixel twice, values times 6 / 3
  wide = augment.sample_disparity_px(raw, (1, 2, 2, 3), False, 2, 6)[:, :, 0]
  assert np.array_equal(wide, np.repeat(want[:, ::-1], 2, axis=1) * np.float32(2))
  for bad in ((0, 0, 5, 6), (0, 0, 4, 7), (-1, 0, 2, 2), (0, 0, 0, 3), (3, 0, 2, 3)):
    with pytest.raises(ValueError, match='window'):
      augment.sample_disparity_px(raw, bad, False, 2, 3)


def _calib(fx=700.0, fy=710.0, cx=30.0, cy=12.0, b2=0.06, b3=0.59):
  p = lambda b: np.array([fx, 0, cx, -fx * b, 0, fy, cy, 0, 0, 0, 1, 0], np.float64)
  return {'P_rect_02': p(b2), 'P_rect_03': p(b3)}


def test_inverse_depth_does_not_depend_on_the_crop_or_the_flip():
  """out / (k_s'[0, 0] |t'_x|) of the augmented pair is raw / 256 / (K[0, 0]
  |t_x|) of the native one at the documented source pixel: 1e-6 relative (the
  fp32 rounding of `out` is 6e-8, the rest is float64)."""
  from lsi.data.kitti import augment, data
  H, W, h, w = 23, 61, OUT_H, OUT_W
  raw = _map(H, W, 3)
  calib = _calib()
  k_s, k_t, rot, t = data.pair_cameras(calib, (H, W, 3), (H, W, 3), h, w)
  native = raw.astype(np.float64) / 256.0 / (700.0 * abs(t[0, 0]))
  rs = np.random.RandomState(7)
  opts = augment.AugmentOptions(0.5, 3.0, 0.0, (1, 1), (1, 1), (1, 1))
  seen = set()
  for _ in range(40):
    aug = augment.sample(rs, opts)
    win = augment.window(aug, H, W)
    y0, x0, ch, cw = win
    ks2, _, _, t2 = augment.augment_cameras(k_s, k_t, rot, t, (H, W, 3), (H, W, 3), win, win,
                                            aug.flip, h, w)
    out = augment.sample_disparity_px(raw, win, aug.flip, h, w)[:, :, 0].astype(np.float64)
    inv = out / (ks2[0, 0] * abs(t2[0, 0]))
    ys = y0 + np.minimum(((2 * np.arange(h) + 1) * ch) // (2 * h), ch - 1)
    xs = x0 + np.minimum(((2 * np.arange(w) + 1) * cw) // (2 * w), cw - 1)
    want = native[ys][:, xs]
    if aug.flip:
      want = want[:, ::-1]
    assert (np.abs(inv - want) <= 1e-6 * np.abs(want)).all()
    assert ((want == 0) == (out == 0)).all() and (out >= 0).all()
    seen.add(aug.flip)
  assert seen == {False, True}


# --- the projection -------------------------------------------------------------
def test_projection_full_window_returns_the_input_bits():
  from lsi.data.kitti import augment, velodyne
  cam, velo = L._calibs()
  for c in (2, 3):
    m = velodyne.velo_to_image(cam, velo, c, (375, 1242, 3), 128, 416)
    got = augment.augment_projection(m, (375, 1242, 3), (0, 0, 375, 1242), False, 128, 416)
    assert got.dtype == np.float32 and got.shape == (3, 4)
    assert np.array_equal(got.view(np.uint32), m.view(np.uint32))
  z = np.array([[-0.0, 1, 2, 3], [4, -0.0, 5, 6], [-1, -2, -3, -4]], np.float32)
  assert np.array_equal(augment.augment_projection(z, (8, 8), (0, 0, 8, 8), False, 4, 4)
                        .view(np.uint32), z.view(np.uint32))


@pytest.mark.parametrize('origin', [0.0, 0.5])
def test_projection_follows_the_augmented_intrinsics(origin):
  """The pixel of augment_projection(velo_to_image(...)) against the pixel of
  augment_cameras' k_s applied to the point in the (flipped) camera-2 frame, in
  float64 to 1e-9.  velo_to_image adds (0.5 - lidar_origin) to KITTI's
  coordinate before it scales -- pixel i covers [i - 0.5, i + 0.5) -- and the
  intrinsics do not: with lidar_origin = 0 the two differ by exactly that half
  source pixel, (0.5 w / cw, 0.5 h / ch), mirrored with the image; with 0.5 by
  nothing.  Both are asserted."""
  from lsi.data.kitti import augment, data, velodyne
  cam, velo = L._calibs(1)
  H, W, h, w = 375, 1242, 128, 416
  shape = (H, W, 3)
  k_s, k_t, rot, t = data.pair_cameras(cam, shape, shape, h, w)
  # the point in the frame of camera 2: P_rect_02 = K [I | c]
  p2 = cam['P_rect_02'].reshape(3, 4)
  c2 = np.linalg.solve(p2[:, :3], p2[:, 3])
  rect = cam['R_rect_00'].reshape(3, 3)
  rs = np.random.RandomState(2)
  pts = np.stack([rs.uniform(5, 60, 6), rs.uniform(-8, 8, 6), rs.uniform(-2, 1, 6)], 1)
  opts = augment.AugmentOptions(0.5, 2.0, 0.0, (1, 1), (1, 1), (1, 1))
  m = velodyne.velo_to_image(cam, velo, 2, shape, h, w, origin=origin, dtype=np.float64)
  seen = set()
  for _ in range(24):
    aug = augment.sample(rs, opts)
    win = augment.window(aug, H, W)
    y0, x0, ch, cw = win
    ks2 = augment.augment_cameras(k_s, k_t, rot, t, shape, shape, win, win, aug.flip, h, w)[0]
    m2 = augment.augment_projection(m, shape, win, aug.flip, h, w, dtype=np.float64)
    assert np.array_equal(m2[2], m[2])
    for p in pts:
      x_cam = rect @ (velo[0] @ p + velo[1]) + c2
      if aug.flip:
        x_cam = x_cam * np.array([-1.0, 1.0, 1.0])
      want = ks2 @ x_cam
      got = m2 @ np.append(p, 1.0)
      assert abs(got[2] - want[2]) <= 1e-9
      half = (0.5 - origin) * np.array([(-1.0 if aug.flip else 1.0) * w / cw, h / ch])
      assert np.abs(got[:2] / got[2] - (want[:2] / want[2] + half)).max() <= 1e-9
      # the flip maps column x to w - x
      m1 = augment.augment_projection(m, shape, win, False, h, w, dtype=np.float64)
      plain = m1 @ np.append(p, 1.0)
      if aug.flip:
        assert abs(got[0] / got[2] - (w - plain[0] / plain[2])) <= 1e-9
        assert got[1] == plain[1]
    seen.add(aug.flip)
  assert seen == {False, True}


# --- the synchronous loader -----------------------------------------------------
def _same(a, b):
  assert len(a) == len(b)
  for u, v in zip(a, b):
    assert u.dtype == v.dtype and u.shape == v.shape
    assert np.array_equal(u, v, equal_nan=u.dtype.kind == 'f')


def test_train_split_emits_ground_truth_and_val_is_unchanged(tmp_path):
  from lsi.data.kitti import data
  make_gt_tree(tmp_path / 'train', 'train')
  make_gt_tree(tmp_path / 'val', 'val')
  off = data.DataLoader(gt_opts(tmp_path / 'train', px=True, velodyne=True, everywhere=False))
  assert off.gt_everywhere is False
  assert not off.output_disparities_px and not off.output_velodyne
  assert not data.DataLoader(gt_opts(tmp_path / 'train', px=True, everywhere=None)).gt_everywhere
  on = data.DataLoader(gt_opts(tmp_path / 'train', px=True, velodyne=True))
  assert on.gt_everywhere is True and on.output_disparities_px and on.output_velodyne
  # the 8-bit maps stay val / test only
  assert not data.DataLoader(gt_opts(tmp_path / 'train', kitti_dl_disparities=True)
                             ).output_disparities
  batch = on.forward(2)
  assert len(batch) == 11
  _same(batch[:6], off.forward(2))
  for view, lst in ((6, on.img_list_disp_src), (7, on.img_list_disp_trg)):
    for k, name in enumerate(on.src_image_names):
      i = on.img_list_src.index(name)
      assert np.array_equal(batch[view][k], data.load_disparity_px(lst[i], OUT_H, OUT_W))
  assert batch[8].shape[0] == 2 and batch[9].dtype == np.int32 and batch[10].shape == (2, 2, 12)
  # val: the batch the loader gives without the flag
  a = data.DataLoader(gt_opts(tmp_path / 'val', 'val', px=True, velodyne=True))
  b = data.DataLoader(gt_opts(tmp_path / 'val', 'val', px=True, velodyne=True,
                              everywhere=None))
  for _ in range(3):
    _same(a.forward(2), b.forward(2))


def test_the_old_refusals_stay_with_the_flag_off(tmp_path):
  from lsi.data.kitti import data, pipeline
  make_gt_tree(tmp_path, 'val')
  for kw in (dict(px=True), dict(velodyne=True)):
    with pytest.raises(ValueError, match='cannot augment'):
      data.DataLoader(gt_opts(tmp_path, 'val', everywhere=False, augment=True, **kw))
    with pytest.raises(ValueError, match='synchronous loader only'):
      pipeline.PrefetchLoader(data.DataLoader(gt_opts(tmp_path, 'val', everywhere=False, **kw)))
  # the 8-bit maps cannot be augmented, flag or no flag
  with pytest.raises(ValueError, match='cannot augment'):
    data.DataLoader(gt_opts(tmp_path, 'val', augment=True, kitti_dl_disparities=True))
  # an object that lacks the attribute is refused as before
  for name in ('output_disparities_px', 'output_velodyne'):
    with pytest.raises(ValueError, match='synchronous loader only'):
      pipeline.PrefetchLoader(types.SimpleNamespace(**{name: True}))


AUG_MIRROR = dict(aug_flip_prob=1.0, aug_zoom_max=1.0, aug_color_prob=0.0)


def test_mirrored_pairs_carry_mirrored_ground_truth(tmp_path):
  from lsi.data.kitti import data
  make_gt_tree(tmp_path)
  plain = data.DataLoader(gt_opts(tmp_path, px=True, velodyne=True))
  flipped = data.DataLoader(gt_opts(tmp_path, px=True, velodyne=True, augment=True,
                                    **AUG_MIRROR))
  for _ in range(3):
    a, b = plain.forward(2), flipped.forward(2)
    assert len(b) == 11 and plain.src_image_names == flipped.src_image_names
    for view in (6, 7):
      assert np.array_equal(b[view], a[view][:, :, ::-1]) and float(b[view].max()) > 0
    _same(a[8:10], b[8:10])        # the scans are not touched
    m, f = a[10].reshape(2, 2, 3, 4).astype(np.float64), b[10].reshape(2, 2, 3, 4)
    assert np.array_equal(f[:, :, 0], (OUT_W * m[:, :, 2] - m[:, :, 0]).astype(np.float32))
    assert np.array_equal(f[:, :, 1:], a[10].reshape(2, 2, 3, 4)[:, :, 1:])


def test_ground_truth_does_not_shift_the_draws(tmp_path):
  from lsi.data.kitti import augment, data
  make_gt_tree(tmp_path)
  kw = dict(augment=True, aug_seed=5, aug_zoom_max=1.5)
  bare = data.DataLoader(gt_opts(tmp_path, everywhere=None, **kw))
  full = data.DataLoader(gt_opts(tmp_path, px=True, velodyne=True, **kw))
  rs = np.random.RandomState(5)
  augs = []
  for _ in range(3):
    a, b = bare.forward(2), full.forward(2)
    assert len(a) == 6 and len(b) == 11
    _same(a, b[:6])
    augs += [augment.sample(rs, full.augment) for _ in range(2)]
  # ... and they are N_DRAWS per pair: the third batch's maps follow from them
  assert augment.N_DRAWS == 11
  for k, name in enumerate(full.src_image_names):
    i = full.img_list_src.index(name)
    raw = data.decode_u16(full.img_list_disp_trg[i])
    aug = augs[4 + k]
    assert np.array_equal(b[7][k], augment.sample_disparity_px(
        raw, augment.window(aug, *raw.shape), aug.flip, OUT_H, OUT_W))


# --- the prefetching loader, host route -----------------------------------------
@pytest.mark.parametrize('workers', [1, 3, 16])
@pytest.mark.parametrize('rank', [0, 3])
@pytest.mark.parametrize('gt', ['px', 'velodyne'])
@pytest.mark.parametrize('aug', [False, True])
def test_threaded_host_loader_is_the_synchronous_one(tmp_path, workers, rank, gt, aug):
  from lsi.data.kitti import data, pipeline
  make_gt_tree(tmp_path)
  opts = gt_opts(tmp_path, px=gt == 'px', velodyne=gt == 'velodyne', augment=aug,
                 aug_seed=3, aug_zoom_max=1.6)
  sync, inner = data.DataLoader(opts), data.DataLoader(opts)
  with pipeline.PrefetchLoader(inner, workers=workers, resize='host',
                               prefetch_depth=1 + workers % 3) as pre:
    assert pre.n_threads == workers
    for ld in (sync, pre):
      ld._rng = np.random.RandomState(rank)
      if aug:
        ld._aug_rng = np.random.RandomState([3, rank])
    zero = False
    for _ in range(3):                # 6 samples of a tree of 5: the order wraps
      want, got = sync.forward(2), pre.forward(2)
      assert len(got) == (8 if gt == 'px' else 9)
      _same(got, want)
      assert pre.src_image_names == sync.src_image_names
      zero = zero or (gt == 'velodyne' and (got[7] == 0).any())
    assert zero == (gt == 'velodyne')   # the missing and the empty scan came by
  assert pre.workers_alive() == 0


def test_corrupt_map_and_truncated_scan_are_named_by_the_owning_forward(tmp_path):
  from lsi.data.kitti import data, pipeline
  make_gt_tree(tmp_path)
  opts = gt_opts(tmp_path, px=True, velodyne=True, augment=True)
  sync = data.DataLoader(opts)
  order = [int(i) for i in np.random.RandomState(0).permutation(5)]
  bad_map = sync.img_list_disp_trg[order[2]]     # batch 1
  bad_scan = sync.scan_list[order[4]]            # batch 2
  want = sync.forward(2)
  from PIL import Image
  Image.fromarray(np.zeros((23, 61), np.uint8)).save(bad_map)   # 8 bits: no disparity map
  with open(bad_scan, 'wb') as f:
    f.write(b'\0' * 40)
  pre = pipeline.PrefetchLoader(data.DataLoader(opts), workers=3, resize='host')
  _same(pre.forward(2), want)
  with pytest.raises(Exception) as e1:
    pre.forward(2)
  assert bad_map in str(e1.value)
  with pytest.raises(Exception) as e2:
    pre.forward(2)
  assert bad_scan in str(e2.value)
  pre.close()
  with pytest.raises(ValueError, match=os.path.basename(bad_map)):
    sync.forward(2)


def test_flag_defaults_and_messages():
  import ldi_enc_dec as script
  import ldi_pred_eval as ev
  assert script.build_parser().parse_args([]).kitti_gt_everywhere is False
  assert ev.build_parser().parse_args([]).kitti_gt_everywhere is False
  assert script.build_parser().parse_args(['--kitti_gt_everywhere', 'true']).kitti_gt_everywhere
  assert ev.build_parser().parse_args(['--kitti_gt_everywhere', 'true']).kitti_gt_everywhere
  assert '--kitti_gt_everywhere' in script.DEPTH_SUP_SOURCES


# --- the C entry point's refusals ----------------------------------------------
EINVAL, ENULL = -1, -2


def test_entry_point_refuses_before_any_launch(built_lib):
  """No device here: every answer is given before any launch, from pointers
  that are never dereferenced."""
  from lsi import _C
  lib = _C.lib()

  def call(rows=(dict(),), n=None, Ho=16, Wo=40, packed=1 << 20, packed_bytes=1 << 16,
           desc_dev=1 << 12, out=1 << 16, host=True):
    arr = (_C.LsiAugmentDesc * max(len(rows), 1))()
    for d, kw in zip(arr, rows):
      f = dict(offset=0, H=23, W=61, C=1, flags=0, y0=0, x0=0, ch=23, cw=61, table=-1)
      f.update(kw)
      for name, v in f.items():
        setattr(d, name, v)
      d.gain[0] = float('nan')     # not read
    return lib.lsi_augment_sample_u16(
        len(rows) if n is None else n, ctypes.addressof(arr) if host else None, desc_dev,
        packed, packed_bytes, Ho, Wo, out, None)

  ok = dict(out=None)   # acceptable but for the missing output: the last answer
  assert call(**ok) == ENULL
  for name in ('packed', 'desc_dev', 'out'):
    assert call(**{name: None}) == ENULL, name
  assert call(host=False) == ENULL
  for kw in (dict(n=0), dict(n=-1), dict(n=65536),
             dict(rows=(dict(C=3),)), dict(rows=(dict(C=0),)),
             dict(rows=(dict(H=0, ch=0),)), dict(rows=(dict(W=0, cw=0),)),
             dict(rows=(dict(H=-3),)), dict(rows=(dict(W=-3),)),
             dict(rows=(dict(ch=0),)), dict(rows=(dict(cw=0),)),
             dict(rows=(dict(y0=-1),)), dict(rows=(dict(x0=-1),)),
             dict(rows=(dict(y0=1),)), dict(rows=(dict(x0=1),)),
             dict(rows=(dict(y0=22, ch=2),)), dict(rows=(dict(x0=60, cw=2),)),
             dict(rows=(dict(flags=2),)), dict(rows=(dict(flags=3),)),
             dict(rows=(dict(flags=0x80000000),)),
             dict(rows=(dict(table=0),)), dict(rows=(dict(table=-2),)),
             dict(rows=(dict(offset=-16),)), dict(rows=(dict(offset=8),)),
             dict(rows=(dict(offset=(1 << 16) - 2800),)),           # 2 H W = 2806 > 2800
             dict(rows=(dict(offset=1 << 16),)), dict(rows=(dict(offset=1 << 40),)),
             dict(packed_bytes=2 * 23 * 61 - 6),                    # a multiple of 16, too few
             # (2 Ho + 1)(ch + 1) = 65535 * 32769, (2 Wo + 1)(cw + 1) = 2049 * 1048065
             dict(rows=(dict(H=1 << 15, W=1, ch=1 << 15, cw=1),), Ho=32767),
             dict(rows=(dict(H=1, W=1 << 20, ch=1, cw=1048064),), Wo=1 << 10,
                  packed_bytes=1 << 22),
             dict(Ho=0), dict(Wo=0), dict(Ho=-1),
             dict(packed=(1 << 20) + 8), dict(packed_bytes=(1 << 16) + 8),
             dict(out=(1 << 16) + 2), dict(desc_dev=(1 << 12) + 4),
             dict(rows=(dict(), dict(C=3)))):
    assert call(**kw) == EINVAL, kw
  # the edges that are accepted (then refused for the missing output)
  for kw in (dict(rows=(dict(flags=1),)), dict(rows=(dict(y0=22, x0=60, ch=1, cw=1),)),
             dict(rows=(dict(offset=(1 << 16) - 2816),)),           # 2 H W = 2806 <= 2816
             dict(rows=(dict(),) * 3), dict(Wo=37),
             dict(rows=(dict(H=1 << 15, W=1, ch=1 << 15, cw=1),), Ho=32766),
             dict(rows=(dict(H=1, W=1 << 20, ch=1, cw=1048063),), Wo=1 << 10,
                  packed_bytes=1 << 22)):
    assert call(out=None, **kw) == ENULL, kw
