"""The LiDAR rasteriser without a GPU: the NumPy restatement
(tests/lidar_ref.py) against answers worked out by hand, the scanner-to-image
matrix, the loader's three velodyne outputs on a miniature raw_city tree, and
every refusal of the C entry point, which are all made before any launch."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import lidar_ref as R

# u = (64 x + 32 z) / z, v = (64 y + 16 z) / z: with z = 4 (or 8) and x, y
# multiples of 1/16 every intermediate is an integer or a dyadic fraction
M = np.array([[64, 0, 32, 0], [0, 64, 16, 0], [0, 0, 1, 0]], np.float32)
H, W = 32, 64


def _one(points, **kw):
  pts = np.asarray(points, np.float32).reshape(-1, 3)
  pts = np.concatenate([pts, np.zeros((len(pts), 1), np.float32)], 1)
  return _both(pts, [0], [len(pts)], M[None, None], **kw)[0, 0, :, :, 0]


def _both(pts, first, count, mats, **kw):
  """The restatement's maps, which the op route (the same definition in torch ops,
  here on the CPU) must give as well, bit for bit."""
  from lsi.geometry import lidar
  want = R.rasterize(pts, first, count, mats, H, W, **kw)
  mats = np.asarray(mats, np.float32).reshape(len(count), -1, 12)
  got = lidar.rasterize_points_ops(torch.from_numpy(np.array(pts)), first, count,
                                   torch.from_numpy(mats), H, W, **kw)
  assert got.shape == want.shape
  assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
  return want


def _only(img, entries):
  want = np.zeros((H, W), np.float32)
  for (r, c), z in entries.items():
    want[r, c] = z
  return np.array_equal(img, want)


# --- the restatement against hand-worked answers ------------------------------
def test_projection_and_image_bounds_by_hand():
  assert _only(_one([(-2, -1, 4)]), {(0, 0): 4})            # X = Y = 0
  assert _only(_one([(0, 0, 4)]), {(16, 32): 4})
  assert _only(_one([(2 - 1 / 16., 1 - 1 / 16., 4)]), {(31, 63): 4})
  assert _only(_one([(2, 1, 4)]), {})                        # u = 64 = W
  assert _only(_one([(0, 1, 4)]), {})                        # v = 32 = H
  assert _only(_one([(-2 - 1 / 16., -1, 4)]), {})            # u = -1
  assert _only(_one([(-2 - 2.0 ** -20, -1, 4)]), {})         # u = -2^-16
  assert _only(_one([(-2, -1 - 2.0 ** -20, 4)]), {})         # v = -2^-16
  assert _only(_one([(-2 + 2.0 ** -20, -1, 4)]), {(0, 0): 4})
  # (u, v) = (32.75, 16.5) -> floor
  assert _only(_one([(3 / 64., 1 / 32., 4)]), {(16, 32): 4})
  assert _only(_one([(-2, -1, 4)], inverse=True), {(0, 0): 0.25})


def test_nearest_return_wins_in_either_order():
  near, far = (0, 0, 4), (0, 0, 8)                           # both on (16, 32)
  for pts in ([near, far], [far, near], [far, near, far]):
    assert _only(_one(pts), {(16, 32): 4})
  assert _only(_one([far, near], inverse=True), {(16, 32): 0.25})


def test_depth_bounds_and_nan():
  kw = dict(z_min=2., z_max=8.)
  assert _only(_one([(0, 0, 2)], **kw), {(16, 32): 2})      # equal to z_min
  assert _only(_one([(0, 0, 8)], **kw), {(16, 32): 8})      # equal to z_max
  assert _only(_one([(0, 0, 1.5)], **kw), {})
  assert _only(_one([(0, 0, 8.5)], **kw), {})
  assert _only(_one([(0, 0, np.nan)], **kw), {})
  assert _only(_one([(np.nan, 0, 4)], **kw), {})
  assert _only(_one([(0, np.nan, 4)], **kw), {})
  assert _only(_one([(0, 0, -4)], **kw), {})
  # a dropped point does not shadow a kept one
  assert _only(_one([(0, 0, 1.5), (0, 0, 4), (0, 0, np.nan)], **kw), {(16, 32): 4})


def test_occlusion_filter_by_hand():
  near, far = (0, 0, 4), (1 / 8., 0, 8)                     # (16, 32) and (16, 33)
  both = {(16, 32): 4, (16, 33): 8}
  assert _only(_one([near, far]), both)
  assert _only(_one([near, far], occl_window=(0, 1), occl_ratio=1.5), {(16, 32): 4})
  assert _only(_one([far, near], occl_window=(2, 2), occl_ratio=1.5), {(16, 32): 4})
  assert _only(_one([near, far], occl_window=(0, 1), occl_ratio=2.5), both)
  assert _only(_one([near, far], occl_window=(0, 1), occl_ratio=2.0), both)   # 8 < 8 is false
  assert _only(_one([near, far], occl_window=(1, 0), occl_ratio=1.5), both)   # not in the column
  assert _only(_one([near, far], occl_window=(0, 1), occl_ratio=1.0), {(16, 32): 4})
  # the filter reads the unfiltered buffer: the middle return is removed by the
  # near one and still removes the far one
  chain = [near, (1 / 8., 0, 6), (3 / 8., 0, 8.5)]           # columns 32, 33, 34: 4, 6, 8.5
  assert _only(_one(chain), {(16, 32): 4, (16, 33): 6, (16, 34): 8.5})
  assert _only(_one(chain, occl_window=(0, 1), occl_ratio=1.4), {(16, 32): 4})
  # a window clipped by the image corner: near on (0, 0), far on (1, 1)
  corner = [(-2, -1, 4), (-3.875, -1.875, 8)]
  assert _only(_one(corner), {(0, 0): 4, (1, 1): 8})
  assert _only(_one(corner, occl_window=(1, 1), occl_ratio=1.5), {(0, 0): 4})
  assert _only(_one(corner, occl_window=(8, 8), occl_ratio=1.5), {(0, 0): 4})
  assert _only(_one(corner, occl_window=(1, 0), occl_ratio=1.5), {(0, 0): 4, (1, 1): 8})
  assert _only(_one(corner, occl_window=(1, 1), occl_ratio=1.5, inverse=True), {(0, 0): 0.25})


def test_batches_views_and_ragged_forms_of_the_restatement():
  pts = np.zeros((2, 4, 4), np.float32)
  pts[:] = np.nan
  pts[0, 0, :3] = (0, 0, 4)
  shifted = M.copy()
  shifted[0, 2] += 1                                        # one column to the right
  mats = np.stack([np.stack([M, shifted])] * 2).reshape(2, 2, 12)
  out = _both(pts, None, [1, 0], mats)
  assert out.shape == (2, 2, H, W, 1) and out.dtype == np.float32
  assert _only(out[0, 0, :, :, 0], {(16, 32): 4}) and _only(out[0, 1, :, :, 0], {(16, 33): 4})
  assert not out[1].any()
  packed = _both(pts.reshape(-1, 4), [4, 0], [0, 1], mats)
  assert np.array_equal(packed[1], out[0]) and not packed[0].any()


# --- the scanner-to-image matrix ---------------------------------------------
def _calibs(seed=0):
  rs = np.random.RandomState(seed)
  q, _ = np.linalg.qr(rs.randn(3, 3))
  q2, _ = np.linalg.qr(np.eye(3) + 0.01 * rs.randn(3, 3))
  cam = {'R_rect_00': q2.reshape(9)}
  for c, tx in ((2, 40.0), (3, -340.0)):
    cam['P_rect_0%d' % c] = np.array([721.5, 0, 609.5, tx, 0, 721.5, 172.8, 0.2 * c,
                                      0, 0, 1, 0.003])
  return cam, (q, rs.randn(3))


@pytest.mark.parametrize('origin', [0.0, 1.0])
@pytest.mark.parametrize('size', [(375, 1242), (128, 416)])
def test_velo_to_image_is_the_float64_product(origin, size):
  from lsi.data.kitti import velodyne
  cam, (rot, trans) = _calibs()
  h0, w0 = 375, 1242
  h, w = size
  for c in (2, 3):
    got = velodyne.velo_to_image(cam, (rot, trans), c, (h0, w0, 3), h, w, origin=origin)
    assert got.shape == (3, 4) and got.dtype == np.float32
    rt = np.vstack([np.hstack([rot, trans.reshape(3, 1)]), [0, 0, 0, 1]])
    rect = np.eye(4)
    rect[:3, :3] = cam['R_rect_00'].reshape(3, 3)
    s = np.array([[w / w0, 0, (0.5 - origin) * w / w0],
                  [0, h / h0, (0.5 - origin) * h / h0], [0, 0, 1.0]])
    want = s @ cam['P_rect_0%d' % c].reshape(3, 4) @ rect @ rt
    # float64 products associated differently agree to ~1e-13 here (entries up to
    # 1e3, three-term sums); the result is rounded to float32 once: half an ulp
    assert (np.abs(got - want) <= 2.0 ** -24 * np.abs(want) + 1e-12).all()
    assert want[2, 2] != 0 and np.array_equal(got[2], want[2].astype(np.float32))


def test_a_hand_placed_point_lands_where_its_geometry_says():
  from lsi.data.kitti import velodyne
  # scanner x forward, y left, z up -> camera x right, y down, z forward
  rot = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], np.float64)
  cam = {'R_rect_00': np.eye(3).reshape(9),
         'P_rect_02': np.array([700, 0, 600.25, 0, 0, 700, 180, 0, 0, 0, 1, 0.])}
  # 10 m ahead, 1 m to the right, 0.5 m below: KITTI coordinate (670.25, 215)
  pt = np.array([[10, -1, -0.5, 0.3]], np.float32)
  for origin, size, pixel in ((0., (376, 1240), (215, 670)), (1., (376, 1240), (214, 669)),
                              (0., (188, 620), (107, 335)), (1., (188, 620), (107, 334))):
    m = velodyne.velo_to_image(cam, (rot, np.zeros(3)), 2, (376, 1240, 3), size[0], size[1],
                               origin=origin)
    out = R.rasterize(pt, [0], [1], m.reshape(1, 1, 12), size[0], size[1])[0, 0, :, :, 0]
    assert sorted(zip(*np.nonzero(out))) == [pixel], (origin, size)
    assert out[pixel] == 10


# --- the loader ---------------------------------------------------------------
def _write_png(path, h, w, seed):
  from PIL import Image
  os.makedirs(os.path.dirname(path), exist_ok=True)
  rs = np.random.RandomState(seed)
  Image.fromarray(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(path)


def _opts(root, **kw):
  base = dict(batch_size=3, kitti_data_root=str(root), kitti_dataset_variant='raw_city',
              data_split='val', img_height=16, img_width=48, kitti_dl_velodyne=True)
  base.update(kw)
  return types.SimpleNamespace(**base)


def _make_tree(root):
  """Three frames of one val sequence, 32 x 96 images; frames 0 and 2 have scans
  of 5 and 2 points, frame 1 has none."""
  from lsi.data.kitti import data
  seq = data.DataLoader(_opts(root)).split_sequences()[0]
  date = seq[:10]
  top = root / 'kitti_raw' / date
  for cam in ('image_02', 'image_03'):
    for i in range(3):
      _write_png(str(top / (seq + '_sync') / cam / 'data' / ('%010d.png' % i)), 32, 96,
                 10 * i + (cam == 'image_03'))
  p = lambda fx, tx: '%f 0 48 %f 0 %f 16 0 0 0 1 0' % (fx, tx, fx)
  (top / 'calib_cam_to_cam.txt').write_text(
      'calib_time: 09-Jan-2012 13:57:47\nR_rect_00: 1 0 0 0 1 0 0 0 1\n'
      'P_rect_02: %s\nP_rect_03: %s\n' % (p(70.0, 4.2), p(70.0, -37.1)))
  (top / 'calib_velo_to_cam.txt').write_text(
      'calib_time: 15-Mar-2012 11:37:16\nR: 0 -1 0 0 0 -1 1 0 0\nT: 0.01 -0.07 -0.27\n'
      'delta_f: 0 0\ndelta_c: 0 0\n')
  scans = {}
  rs = np.random.RandomState(5)
  vdir = top / (seq + '_sync') / 'velodyne_points' / 'data'
  os.makedirs(str(vdir))
  for i, n in ((0, 5), (2, 2)):
    scans[i] = rs.uniform(-20, 20, (n, 4)).astype(np.float32)
    scans[i].tofile(str(vdir / ('%010d.bin' % i)))
  return top, seq, scans


def test_loader_appends_scans_counts_and_matrices(tmp_path):
  from lsi.data.kitti import data, pipeline, velodyne
  top, seq, scans = _make_tree(tmp_path)
  dl = data.DataLoader(_opts(tmp_path, lidar_origin=1.0))
  assert dl.output_velodyne and len(dl.img_list_src) == 3
  out = dl.forward(3)
  assert len(out) == 9
  pts, counts, mats = out[6:]
  frames = [int(os.path.basename(n)[:-4]) for n in dl.src_image_names]
  assert sorted(frames) == [0, 1, 2]
  assert pts.shape == (3, 8, 4) and pts.dtype == np.float32      # 5 -> 8
  assert counts.dtype == np.int32 and counts.shape == (3,)
  assert mats.shape == (3, 2, 12) and mats.dtype == np.float32
  cam = data.read_calib_file(str(top / 'calib_cam_to_cam.txt'))
  velo = velodyne.read_velo_calib(str(top / 'calib_velo_to_cam.txt'))
  assert velo[0].shape == (3, 3) and np.array_equal(velo[1], [0.01, -0.07, -0.27])
  for k, frame in enumerate(frames):
    n = len(scans[frame]) if frame in scans else 0
    assert counts[k] == n
    if n:
      assert np.array_equal(pts[k, :n], scans[frame])
    assert np.isnan(pts[k, n:]).all()
    for view, c in enumerate((2, 3)):
      want = velodyne.velo_to_image(cam, velo, c, (32, 96, 3), 16, 48, origin=1.0)
      assert np.array_equal(mats[k, view], want.reshape(12))
  # the first six outputs are what the loader gives without the option
  plain = data.DataLoader(_opts(tmp_path, kitti_dl_velodyne=False))
  assert not plain.output_velodyne
  six = plain.forward(3)
  assert len(six) == 6 and all(np.array_equal(a, b) for a, b in zip(six, out[:6]))
  # a batch without any scan: Nmax is 4, all NaN
  only = data.DataLoader(_opts(tmp_path, batch_size=1))
  for _ in range(3):
    o = only.forward(1)
    if o[7][0] == 0:
      assert o[6].shape == (1, 4, 4) and np.isnan(o[6]).all()
      break
  else:
    raise AssertionError('the frame without a scan never came')
  # training batches never carry scans; the prefetching loader refuses them
  assert not data.DataLoader(_opts(tmp_path, data_split='train')).output_velodyne
  with pytest.raises(ValueError, match='kitti_dl_velodyne'):
    pipeline.PrefetchLoader(dl, workers=1)
  # as the evaluation sees them: the counts stay integers
  import ldi_enc_dec as script
  batch = script.KittiBatches(data.DataLoader(_opts(tmp_path))).forward(3)
  assert batch[7].dtype == torch.int32 and batch[6].dtype == torch.float32
  assert batch[0].dtype == torch.float32 and batch[2].dtype == torch.float32


def test_a_truncated_scan_is_named(tmp_path):
  from lsi.data.kitti import data, velodyne
  top, seq, scans = _make_tree(tmp_path)
  bad = top / (seq + '_sync') / 'velodyne_points' / 'data' / ('%010d.bin' % 1)
  bad.write_bytes(b'\0' * 40)
  with pytest.raises(ValueError, match=os.path.basename(str(bad))):
    velodyne.load_scan(str(bad))
  with pytest.raises(ValueError, match=os.path.basename(str(bad))):
    data.DataLoader(_opts(tmp_path)).forward(3)
  assert velodyne.load_scan(str(bad.parent / ('%010d.bin' % 0))).shape == (5, 4)


def test_flags():
  import ldi_enc_dec as script
  import ldi_pred_eval as ev
  assert script.build_parser().parse_args([]).kitti_dl_velodyne is False
  e = ev.build_parser().parse_args([])
  assert e.kitti_dl_velodyne is False and e.lidar_origin == 0.0
  assert list(e.lidar_occl_window) == [0, 0] and e.lidar_occl_ratio >= 1.0
  on = ev.build_parser().parse_args(['--kitti_dl_velodyne', 'true', '--lidar_origin', '1',
                                     '--lidar_occl_window', '2', '3',
                                     '--lidar_occl_ratio', '1.5'])
  assert on.kitti_dl_velodyne and on.lidar_origin == 1.0
  assert list(on.lidar_occl_window) == [2, 3] and on.lidar_occl_ratio == 1.5
  # two ground truths for one score are refused, with a message that says to pick
  both = ev.build_parser().parse_args(['--dataset', 'kitti', '--kitti_dl_velodyne', 'true',
                                       '--kitti_dl_disparities_px', 'true'])
  with pytest.raises(ValueError, match='pick the Velodyne scans'):
    ev.Tester(both)


# --- the C entry point's refusals --------------------------------------------
EINVAL, ENULL, EWORKSPACE = -1, -2, -3


class _Call(object):
  """lsi_lidar_rasterize with acceptable arguments and pointers that are never
  dereferenced (every answer here is given before any launch); keyword
  arguments replace single ones."""

  def __init__(self, _C):
    self._C, self.lib = _C, _C.lib()

  def __call__(self, scans=((0, 8), (8, 8)), **kw):
    a = dict(B=len(scans), V=2, H=32, W=64, n_total=16, z_min=1e-3, z_max=80., win_y=0,
             win_x=0, ratio=1.0, flags=0, desc_host=True, desc_dev=64, pts=64, mats=64, out=64,
             ws=64, ws_bytes=1 << 40, reserved=0)
    a.update(kw)
    desc = (self._C.LsiScanDesc * max(len(scans), 1))()
    for k, (first, n) in enumerate(scans):
      desc[k].first, desc[k].n, desc[k].reserved = first, n, a['reserved']
    return self.lib.lsi_lidar_rasterize(
        a['B'], a['V'], a['H'], a['W'], ctypes.addressof(desc) if a['desc_host'] else None,
        a['desc_dev'], a['pts'], a['n_total'], a['mats'], a['z_min'], a['z_max'], a['win_y'],
        a['win_x'], a['ratio'], a['flags'], a['out'], a['ws'], a['ws_bytes'], None)


def test_entry_point_refuses_before_any_launch(built_lib):
  from lsi import _C
  call = _Call(_C)
  one = ((0, 8),)
  # acceptable arguments with a workspace that is too small: the last refusal
  assert call(ws_bytes=2 * 2 * 32 * 64 * 4 - 1) == EWORKSPACE
  for kw in (dict(B=0, scans=()), dict(B=-1, scans=()), dict(B=65536, H=1, W=1),
             dict(V=0), dict(V=3), dict(V=-1), dict(H=0), dict(W=0), dict(H=-4), dict(W=-4),
             dict(scans=one, V=1, H=1 << 14, W=(1 << 13) + 1),         # B V H W = 2^27 + 2^14
             dict(scans=one, V=2, H=1 << 13, W=(1 << 13) + 1),
             dict(scans=one, V=2, H=1 << 30, W=1 << 30),
             dict(scans=((0, -1),)), dict(scans=((-1, 4),)), dict(scans=((9, 8),)),
             dict(scans=((0, 8), (8, 9))), dict(scans=((1 << 62, 1 << 30),)),
             dict(n_total=-1), dict(scans=one, n_total=(1 << 27) + 1),
             dict(z_min=0.), dict(z_min=-1.), dict(z_min=2., z_max=1.),
             dict(z_min=float('nan')), dict(z_max=float('nan')), dict(z_max=float('inf')),
             dict(z_min=float('inf'), z_max=float('inf')),
             dict(win_y=-1), dict(win_x=-1), dict(win_y=9), dict(win_x=9),
             dict(win_y=1, ratio=0.999), dict(win_x=1, ratio=float('nan')),
             dict(win_x=8, win_y=8, ratio=-2.),
             dict(flags=2), dict(flags=0x80000001), dict(reserved=1),
             dict(pts=68), dict(pts=72), dict(pts=65)):
    # a refused call is refused whatever else is wrong with it: EINVAL comes first
    assert call(**kw) == EINVAL, kw
    assert call(ws_bytes=0, out=None, **kw) == EINVAL, kw
  # the edges that are accepted (then refused for the missing output)
  for kw in (dict(scans=one, V=1, H=1 << 14, W=1 << 13), dict(scans=((8, 8),)),
             dict(scans=((16, 0),)), dict(scans=one, n_total=1 << 27),
             dict(z_min=1., z_max=1.), dict(win_y=8, win_x=8, ratio=1.0),
             dict(win_y=0, win_x=0, ratio=0.), dict(flags=1), dict(V=1)):
    assert call(out=None, **kw) == ENULL, kw
  # 65535 scans, none with points
  assert call(scans=((0, 0),) * 65535, H=1, W=1, out=None) == ENULL
  # every required pointer on its own; then the workspace's size
  for name in ('desc_host', 'desc_dev', 'mats', 'out', 'ws', 'pts'):
    assert call(**{name: None}) == ENULL, name
    assert call(ws_bytes=0, **{name: None}) == ENULL, name
  # without points anywhere pts may be NULL
  assert call(scans=((0, 0), (16, 0)), pts=None, ws_bytes=0) == EWORKSPACE
  assert call(scans=((0, 0), (3, 1)), pts=None, ws_bytes=0) == ENULL


def test_workspace_query(built_lib):
  from lsi import _C
  q = _C.lib().lsi_lidar_workspace_bytes
  assert q(2, 2, 32, 64, 0, 0) == 2 * 2 * 32 * 64 * 4
  assert q(1, 1, 1 << 14, 1 << 13, 8, 8) == 4 << 27
  for args in ((0, 2, 32, 64, 0, 0), (65536, 1, 1, 1, 0, 0), (1, 3, 32, 64, 0, 0),
               (1, 0, 32, 64, 0, 0), (1, 1, 0, 64, 0, 0), (1, 1, 32, 0, 0, 0),
               (1, 1, 1 << 14, (1 << 13) + 1, 0, 0), (1, 2, 1 << 30, 1 << 30, 0, 0),
               (1, 1, 32, 64, 9, 0), (1, 1, 32, 64, 0, 9), (1, 1, 32, 64, -1, 0),
               (1, 1, 32, 64, 0, -1)):
    assert q(*args) == 0, args
  assert ctypes.sizeof(_C.LsiScanDesc) == 16 and _C.LsiScanDesc.n.offset == 8


def test_no_cpu_fallback(built_lib):
  from lsi.geometry import lidar
  pts = torch.zeros(1, 4, 4)
  mats = torch.zeros(1, 1, 12)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    lidar.rasterize_points(pts, None, [4], mats, 8, 8)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    lidar.rasterize_points(pts.reshape(4, 4), [0], [4], mats, 8, 8)
  assert lidar.TILE == (16, 64)


def test_op_route_is_the_restatement_on_the_cpu():
  """rasterize_points_ops runs anywhere: on the CPU, whose division is the
  correctly rounded one, it equals the restatement bit for bit."""
  from lsi.geometry import lidar
  rs = np.random.RandomState(3)
  pts = np.empty((2, 400, 4), np.float32)
  pts[..., 0] = rs.uniform(-1.9, 1.9, (2, 400))
  pts[..., 1] = rs.uniform(-0.9, 0.9, (2, 400))
  pts[..., 2] = np.where(rs.rand(2, 400) < 0.5, 4, 7) + rs.uniform(0, 0.5, (2, 400))
  pts[..., 3] = 0
  pts[1, 300:] = np.nan
  mats = np.stack([M, M * np.float32(1.03)]).reshape(1, 2, 12).repeat(2, 0)
  for kw in (dict(), dict(inverse=True), dict(occl_window=(1, 2), occl_ratio=1.25),
             dict(occl_window=(8, 8), occl_ratio=1.0, inverse=True, z_min=4.2, z_max=7.3)):
    want = R.rasterize(pts, None, [400, 300], mats, H, W, **kw)
    got = lidar.rasterize_points_ops(torch.from_numpy(pts), None, [400, 300],
                                     torch.from_numpy(mats), H, W, **kw)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32)), kw
    assert (want != 0).any()
