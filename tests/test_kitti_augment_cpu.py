"""KITTI augmentation (lsi/data/kitti/augment.py) without a GPU: the NumPy
restatement of lsi_augment_resize_u8 against the exact rational AREA resize of
the transformed array, the camera algebra against the pixel map it stands for,
the sampling order, the loaders, the flags, and the C ABI's refusals before any
launch."""
import ctypes
import types

import numpy as np
import pytest

from test_kitti_pipeline_cpu import exact_area, make_opts, make_tree

IDENT_G = np.ones(3, np.float32)


def _aug_opts(root, **kw):
  o = make_opts(root)
  o.kitti_augment = True
  for k, v in kw.items():
    setattr(o, k, v)
  return o


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
CASES = [  # (H, W), window (y0, x0, ch, cw), (ho, wo)
    ((23, 61), (0, 3, 23, 50), (16, 40)),
    ((23, 61), (2, 0, 20, 61), (16, 40)),
    ((67, 131), (5, 9, 60, 120), (16, 24)),
    ((9, 13), (1, 2, 7, 10), (16, 40)),       # upscaling on both axes
    ((40, 13), (3, 1, 35, 11), (16, 40)),     # mixed
    ((5, 7), (4, 6, 1, 1), (3, 4)),           # a one-pixel window
]


@pytest.mark.parametrize('nc', [3, 1])
@pytest.mark.parametrize('shape,win,out', CASES)
def test_restatement_is_the_exact_area_mean_of_the_transformed_array(shape, win,
                                                                     out, nc):
  from lsi.data.kitti import augment
  rs = np.random.RandomState(sum(shape) + nc)
  img = rs.randint(0, 256, shape + (nc,), dtype=np.uint8)
  table = np.stack([rs.permutation(256) for _ in range(nc)]).astype(np.uint8)
  y0, x0, ch, cw = win
  ho, wo = out
  # the transformed array, in NumPy: slice, table, resize, mirror
  sub = img[y0:y0 + ch, x0:x0 + cw]
  sub = np.stack([table[c][sub[:, :, c]] for c in range(nc)], axis=2)
  exact = exact_area(sub, ho, wo)[:, ::-1]
  ones = np.ones(nc, np.float32)
  got = augment.augment_area_resize(img, win, True, table, ones, ho, wo)
  assert got.dtype == np.float32 and got.shape == (ho, wo, nc)
  ratio = np.abs(got.astype(np.float64) - exact) / np.maximum(exact, 2.0 ** -24)
  assert ratio.max() <= 2.0 ** -22
  # the flip is a mirrored store of the same values
  plain = augment.augment_area_resize(img, win, False, table, ones, ho, wo)
  assert np.array_equal(got, np.flip(plain, axis=1))
  # gains: the restatement's own two fp32 operations on that value, bit for bit
  g = rs.uniform(0.3, 2.5, nc).astype(np.float32)
  with_g = augment.augment_area_resize(img, win, False, table, g, ho, wo)
  assert np.array_equal(with_g, np.minimum(plain * g, np.float32(1)))
  assert (with_g == 1).any() or float((plain * g).max()) < 1


def test_identity_parameters_are_the_plain_integer_formula():
  from lsi.data.kitti import augment
  rs = np.random.RandomState(2)
  for shape, (ho, wo) in (((23, 61, 3), (16, 40)), ((9, 13, 1), (16, 40))):
    img = rs.randint(0, 256, shape, dtype=np.uint8)
    h, w, nc = shape
    acc = np.rint(exact_area(img, ho, wo) * (255.0 * h * w)).astype(np.int64)
    want = acc.astype(np.float32) * np.float32(1.0 / (255.0 * h * w))
    got = augment.augment_area_resize(img, (0, 0, h, w), False, None,
                                      np.ones(nc, np.float32), ho, wo)
    assert np.array_equal(got, want)
    ident = np.broadcast_to(np.arange(256, dtype=np.uint8), (nc, 256))
    assert np.array_equal(got, augment.augment_area_resize(
        img, (0, 0, h, w), False, ident, np.ones(nc, np.float32), ho, wo))
  for bad in ((0, 0, 24, 61), (0, -1, 23, 61), (0, 0, 0, 61), (1, 0, 23, 61)):
    with pytest.raises(ValueError, match='window'):
      augment.augment_area_resize(np.zeros((23, 61, 3), np.uint8), bad, False, None,
                                  IDENT_G, 16, 40)
  for g in ((1, -0.5, 1), (1, np.nan, 1), (np.inf, 1, 1)):
    with pytest.raises(ValueError, match='gains'):
      augment.augment_area_resize(np.zeros((23, 61, 3), np.uint8), (0, 0, 23, 61),
                                  False, None, g, 16, 40)


def test_tone_table_and_gains():
  from lsi.data.kitti import augment
  aug = augment.IDENTITY._replace(gamma=0.8, brightness=1.5, color=(0.9, 1.0, 1.1))
  t = augment.tone_table(aug)
  assert t.dtype == np.uint8 and t.shape == (3, 256)
  v = np.arange(256, dtype=np.float64)
  assert np.array_equal(t[1], np.rint(255.0 * (v / 255.0) ** 0.8).astype(np.uint8))
  assert np.array_equal(t[0], t[1]) and np.array_equal(t[0], t[2])
  assert t[0, 0] == 0 and t[0, 255] == 255 and (np.diff(t[0].astype(int)) >= 0).all()
  assert np.array_equal(augment.tone_table(augment.IDENTITY)[0], np.arange(256))
  g = augment.gains(aug)
  assert g.dtype == np.float32
  assert np.array_equal(g, np.float32(1.5 * np.array([0.9, 1.0, 1.1])))
  table, g1 = augment.image_params(aug, 1)       # one channel: identity
  assert table is None and np.array_equal(g1, np.ones(1, np.float32))
  table, g3 = augment.image_params(augment.IDENTITY, 3)
  assert table is None and np.array_equal(g3, np.ones(3, np.float32))


# ---------------------------------------------------------------------------
# cameras
# ---------------------------------------------------------------------------
def _calib(skew=0.0):
  def p(fx, fy, cx, cy, b):
    k = np.array([[fx, skew, cx], [0, fy, cy], [0, 0, 1.0]])
    return np.hstack([k, k @ np.array([[b], [0.01], [0.002]])]).reshape(-1)
  return {'P_rect_02': p(700.0, 710.0, 30.0, 12.0, 0.06),
          'P_rect_03': p(705.0, 708.0, 31.0, 11.0, -0.48)}


def _rot(axis, angle):
  axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
  kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]],
                 [-axis[1], axis[0], 0]])
  return np.eye(3) + np.sin(angle) * kx + (1 - np.cos(angle)) * kx @ kx


@pytest.mark.parametrize('rot_angle', [0.0, 0.07])
@pytest.mark.parametrize('flip,zoom', [(True, 1.0), (False, 1.3), (True, 1.3)])
@pytest.mark.parametrize('shapes', [((23, 61), (23, 61)), ((23, 61), (25, 64))])
def test_cameras_follow_the_pixel_map(shapes, flip, zoom, rot_angle):
  from lsi.data.kitti import augment, data
  h, w = 16, 40
  src_shape, trg_shape = shapes
  k_s, k_t, rot, t = data.pair_cameras(_calib(skew=0.3), src_shape, trg_shape, h, w)
  if rot_angle:
    rot = _rot([0.2, 1.0, -0.3], rot_angle)
  aug = augment.IDENTITY._replace(flip=flip, zoom_y=zoom, zoom_x=zoom * 1.1 if
                                  zoom > 1 else 1.0, off_y=0.3, off_x=0.8)
  win_s, win_t = augment.window(aug, *src_shape), augment.window(aug, *trg_shape)
  if zoom > 1:
    assert win_s[2] < src_shape[0] and win_s[3] < src_shape[1] and win_s[1] > 0
  k_s2, k_t2, rot2, t2 = augment.augment_cameras(
      k_s, k_t, rot, t, src_shape, trg_shape, win_s, win_t, flip, h, w)
  assert all(a.dtype == np.float64 for a in (k_s2, k_t2, rot2, t2))
  assert t2.shape == (3, 1) and rot2.shape == (3, 3)
  rs = np.random.RandomState(1)
  x_s = np.stack([rs.uniform(-3, 3, 64), rs.uniform(-1, 1, 64), rs.uniform(4, 30, 64)])
  x_t = rot @ x_s + t
  assert (x_t[2] > 1).all()
  s = np.diag([-1.0, 1.0, 1.0]) if flip else np.eye(3)

  def project(k, x):
    p = k @ x
    return p[0] / p[2], p[1] / p[2]

  def pixel_map(u, v, shape, win):
    # whole image resized to w x h -> the window resized to w x h (-> mirrored)
    y0, x0, ch, cw = win
    u_src, v_src = u * shape[1] / w, v * shape[0] / h     # source pixels
    u2, v2 = (u_src - x0) * (w / cw), (v_src - y0) * (h / ch)
    return (w - u2 if flip else u2), v2

  # the augmented target-frame point is the augmented motion of the augmented
  # source-frame point
  x_s2 = s @ x_s
  x_t2 = rot2 @ x_s2 + t2
  assert np.abs(x_t2 - s @ x_t).max() <= 1e-12
  for k, k2, x, x2, shape, win in ((k_s, k_s2, x_s, x_s2, src_shape, win_s),
                                   (k_t, k_t2, x_t, x_t2, trg_shape, win_t)):
    want = pixel_map(*project(k, x), shape, win)
    got = project(k2, x2)
    assert np.abs(got[0] - want[0]).max() <= 1e-9
    assert np.abs(got[1] - want[1]).max() <= 1e-9


def test_full_window_without_flip_is_pair_cameras_exactly():
  from lsi.data.kitti import augment, data
  for shapes in (((23, 61), (23, 61)), ((375, 1242), (370, 1226))):
    cams = data.pair_cameras(_calib(), shapes[0], shapes[1], 256, 768)
    wins = [augment.window(augment.IDENTITY, *s) for s in shapes]
    assert wins == [(0, 0) + s for s in shapes]
    got = augment.augment_cameras(*cams, shapes[0], shapes[1], wins[0], wins[1],
                                  False, 256, 768)
    for a, b in zip(got, cams):
      assert a.dtype == np.float64 and np.array_equal(a, b)


# ---------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------
def test_sampling_is_seeded_and_options_do_not_shift_each_other():
  from lsi.data.kitti import augment
  full = augment.DEFAULTS._replace(flip_prob=0.5, zoom_max=1.5, color_prob=0.7)
  draw = lambda o, n=40: [augment.sample(rs, o) for rs in [np.random.RandomState(11)]
                          for _ in range(n)]
  a, b = draw(full), draw(full)
  assert a == b
  assert len({x.flip for x in a}) == 2 and len({x.gamma == 1.0 for x in a}) == 2
  rs = np.random.RandomState(11)
  for _ in range(40):
    augment.sample(rs, full)
  assert rs.random_sample() == np.random.RandomState(11).random_sample(
      40 * augment.N_DRAWS + 1)[-1]
  geometry = lambda x: (x.zoom_y, x.zoom_x, x.off_y, x.off_x)
  colour = lambda x: (x.gamma, x.brightness, x.color)
  no_flip = draw(full._replace(flip_prob=0.0))
  assert not any(x.flip for x in no_flip)
  assert [x._replace(flip=False) for x in a] == no_flip
  no_zoom = draw(full._replace(zoom_max=1.0))
  assert all(x.zoom_y == 1.0 and x.zoom_x == 1.0 for x in no_zoom)
  assert [(x.flip, x.off_y, x.off_x) + colour(x) for x in a] == [
      (x.flip, x.off_y, x.off_x) + colour(x) for x in no_zoom]
  no_colour = draw(full._replace(color_prob=0.0))
  assert all(colour(x) == (1.0, 1.0, (1.0, 1.0, 1.0)) for x in no_colour)
  assert [(x.flip,) + geometry(x) for x in a] == [(x.flip,) + geometry(x)
                                                  for x in no_colour]
  for x in a:
    assert 1.0 <= x.zoom_y <= 1.5 and 0.0 <= x.off_x < 1.0
    if x.gamma != 1.0:
      assert 0.8 <= x.gamma <= 1.2 and 0.5 <= x.brightness <= 2.0
      assert all(0.8 <= c <= 1.2 for c in x.color)


def test_windows_lie_inside_the_image():
  from lsi.data.kitti import augment
  rs = np.random.RandomState(3)
  opts = augment.DEFAULTS._replace(zoom_max=3.0)
  edge = [augment.IDENTITY._replace(zoom_y=z, zoom_x=z, off_y=o, off_x=o)
          for z in (1.0, 3.0) for o in (0.0, 0.5, 1.0)]
  for hh in range(1, 51):
    for ww in range(1, 51):
      for aug in edge + [augment.sample(rs, opts)]:
        y0, x0, ch, cw = augment.window(aug, hh, ww)
        assert 0 <= y0 and ch >= 1 and y0 + ch <= hh
        assert 0 <= x0 and cw >= 1 and x0 + cw <= ww
  assert augment.window(augment.IDENTITY._replace(zoom_y=2.0, off_y=0.5), 40, 30) == (
      10, 0, 20, 30)


# ---------------------------------------------------------------------------
# loaders
# ---------------------------------------------------------------------------
def _same(a, b):
  assert len(a) == len(b)
  for u, v in zip(a, b):
    assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v)


def test_augmentation_off_is_todays_loader(tmp_path):
  from lsi.data.kitti import data
  plain = make_tree(tmp_path)
  off = _aug_opts(tmp_path, kitti_augment=False, aug_flip_prob=1.0, aug_seed=5)
  a, b = data.DataLoader(plain), data.DataLoader(off)
  assert b.augment is None and not hasattr(b, '_aug_rng')
  for _ in range(3):
    _same(a.forward(2), b.forward(2))
    assert a.src_image_names == b.src_image_names


def test_augmented_loader_keeps_the_order_and_transforms_pairs(tmp_path):
  from lsi.data.kitti import augment, data, pipeline
  plain = make_tree(tmp_path)
  a = data.DataLoader(plain)
  b = data.DataLoader(_aug_opts(tmp_path, aug_seed=3, aug_zoom_max=1.4))
  rs = np.random.RandomState(3)
  changed = False
  for _ in range(3):
    want, got = a.forward(2), b.forward(2)
    assert a.src_image_names == b.src_image_names
    assert [g.shape for g in got] == [w.shape for w in want]
    assert [g.dtype for g in got] == [w.dtype for w in want]
    for j, name in enumerate(b.src_image_names):
      aug = augment.sample(rs, b.augment)       # one draw per sample, in order
      for view, path in ((0, name), (1, name.replace('image_02', 'image_03'))):
        arr = pipeline.decode_u8(path, 3)
        table, gains = augment.image_params(aug, 3)
        ref = augment.augment_area_resize(
            arr, augment.window(aug, *arr.shape[:2]), aug.flip, table, gains, 16, 40)
        assert np.array_equal(got[view][j], ref)
      if aug.flip:
        assert got[5][j][0, 0] == -want[5][j][0, 0]     # the baseline's sign
      changed = changed or not np.array_equal(got[0][j], want[0][j])
  assert changed


@pytest.mark.parametrize('workers,depth', [(1, 2), (4, 2), (4, 1), (4, 3)])
def test_threaded_augmenting_loader_is_the_synchronous_one(tmp_path, workers, depth):
  from lsi.data.kitti import data, pipeline
  make_tree(tmp_path)
  opts = _aug_opts(tmp_path, aug_seed=7, aug_zoom_max=1.3, aug_color_prob=0.8)
  sync = data.DataLoader(opts)
  with pipeline.PrefetchLoader(data.DataLoader(opts), workers=workers,
                               resize='host', prefetch_depth=depth) as pre:
    for _ in range(4):
      want, got = sync.forward(2), pre.forward(2)
      assert len(got) == 6
      _same(got, want)
      assert pre.src_image_names == sync.src_image_names
  assert pre.workers_alive() == 0


def test_ranks_draw_their_own_augmentations(tmp_path):
  import ldi_enc_dec as script
  from lsi.data.kitti import data, pipeline
  make_tree(tmp_path)
  opts = _aug_opts(tmp_path, aug_seed=7)
  first = []
  for rank in (0, 1):
    sync = script.KittiBatches(data.DataLoader(opts), rank)
    pre = script.KittiBatches(pipeline.PrefetchLoader(data.DataLoader(opts), workers=2),
                              rank)
    a, b = sync.forward(2), pre.forward(2)
    pre.close()
    assert all(bool((u == v).all()) for u, v in zip(a, b))
    first.append(sync.loader._aug_rng.random_sample())
  assert first[0] != first[1]
  with pipeline.PrefetchLoader(data.DataLoader(opts), workers=2) as pre:
    pre.forward(2)
    with pytest.raises(RuntimeError, match='before the first forward'):
      pre._aug_rng = np.random.RandomState(0)


@pytest.mark.parametrize('field', ['kitti_dl_disparities', 'kitti_dl_disparities_px',
                                   'kitti_dl_velodyne'])
def test_ground_truth_loader_refuses_augmentation(tmp_path, field):
  from lsi.data.kitti import data
  make_tree(tmp_path, 'val', True)
  opts = _aug_opts(tmp_path, data_split='val', **{field: True})
  with pytest.raises(ValueError, match='kitti_augment'):
    data.DataLoader(opts)
  opts.kitti_augment = False
  data.DataLoader(opts)


def test_flags_and_refusals_of_the_scripts(tmp_path):
  import ldi_enc_dec as script
  import ldi_pred_eval
  o = script.build_parser().parse_args([])
  assert o.kitti_augment is False and o.aug_seed == 0
  assert (o.aug_flip_prob, o.aug_zoom_max, o.aug_color_prob) == (0.5, 1.15, 0.5)
  assert (list(o.aug_gamma), list(o.aug_brightness), list(o.aug_color)) == (
      [0.8, 1.2], [0.5, 2.0], [0.8, 1.2])
  from lsi.data.kitti import augment
  assert augment.options_from(o) == augment.DEFAULTS
  assert augment.options_from(types.SimpleNamespace()) == augment.DEFAULTS
  with pytest.raises(ValueError, match='zoom_max'):
    augment.options_from(types.SimpleNamespace(aug_zoom_max=0.9))
  with pytest.raises(ValueError, match='aug_gamma'):
    augment.options_from(types.SimpleNamespace(aug_gamma=(1.2, 0.8)))
  make_tree(tmp_path)
  base = ['--cpu', 'true', '--checkpoint_dir', str(tmp_path / 'ckpt'),
          '--img_height', '16', '--img_width', '40', '--kitti_augment', 'true']
  parse = lambda extra: script.apply_dataset_overrides(
      script.build_parser().parse_args(base + extra))
  for extra in (['--dataset', 'synthetic'],
                ['--dataset', 'synthetic', '--synth_scene', 'planes'],
                ['--dataset', 'kitti', '--kitti_procedural', 'true']):
    with pytest.raises(ValueError, match='--kitti_augment'):
      script.Trainer(parse(extra)).define_data_loader()
    if '--synth_scene' not in extra:     # (the planes renderer needs a device)
      off = parse(extra + ['--kitti_augment', 'false', '--aug_flip_prob', '1'])
      script.Trainer(off).define_data_loader()    # the --aug_* values are ignored
  files = ['--dataset', 'kitti', '--kitti_dataset_variant', 'raw_city',
           '--kitti_data_root', str(tmp_path), '--aug_seed', '4', '--aug_gamma',
           '0.9', '1.1']
  tr = script.Trainer(parse(files))
  tr.define_data_loader()
  assert tr.data_loader.loader.augment.gamma == (0.9, 1.1)
  assert tr.data_loader.loader.aug_seed == 4
  assert len(tr.feed()) == 6
  e = ldi_pred_eval.build_parser().parse_args(base + files)
  with pytest.raises(ValueError, match='--kitti_augment'):
    ldi_pred_eval.Tester(script.apply_dataset_overrides(e))


# ---------------------------------------------------------------------------
# the C ABI's refusals
# ---------------------------------------------------------------------------
def test_augment_arguments_are_refused_before_any_launch(built_lib):
  from lsi import _C
  from lsi.data.kitti import pipeline
  lib = _C.lib()
  EINVAL, ENULL = -1, -2
  assert ctypes.sizeof(_C.LsiAugmentDesc) == 64
  assert pipeline.AUG_DESC_DTYPE.itemsize == 64
  names = ('offset', 'H', 'W', 'C', 'flags', 'y0', 'x0', 'ch', 'cw', 'table', 'gain')
  assert [pipeline.AUG_DESC_DTYPE.fields[n][1] for n in names] == [
      getattr(_C.LsiAugmentDesc, n).offset for n in names]
  assert pipeline.AUG_FLIP == _C.LSI_AUG_FLIP == 1

  def descs(*rows, **kw):
    arr = (_C.LsiAugmentDesc * len(rows))()
    for d, (off, h, w, c) in zip(arr, rows):
      d.offset, d.H, d.W, d.C = off, h, w, c
      d.y0, d.x0, d.ch, d.cw = kw.get('win', (0, 0, h, w))
      d.table, d.flags = kw.get('table', -1), kw.get('flags', 0)
      d.gain[0], d.gain[1], d.gain[2] = kw.get('gain', (1.0, 1.0, 1.0))
    return arr

  # (addresses that are never dereferenced: every call below is refused)
  dev, packed, out = 0x10000, 0x20000, 0x30000

  def call(d, n, packed_bytes, co, desc_dev=dev, pk=packed, o=out, ho=16, wo=40,
           tables_offset=0, n_tables=0):
    host = ctypes.addressof(d) if d is not None else None
    return lib.lsi_augment_resize_u8(n, host, desc_dev, pk, packed_bytes,
                                     tables_offset, n_tables, ho, wo, co, o, None)

  ok = descs((0, 23, 61, 3))
  big = 1 << 30
  assert call(None, 1, big, 3) == ENULL
  assert call(ok, 1, big, 3, desc_dev=None) == ENULL
  assert call(ok, 1, big, 3, pk=None) == ENULL
  assert call(ok, 1, big, 3, o=None) == ENULL
  # what the plain call refuses
  assert call(ok, 0, big, 3) == EINVAL
  assert call(descs((0, 23, 61, 2)), 1, big, 2) == EINVAL
  assert call(descs((0, 23, 61, 1)), 1, big, 3) == EINVAL
  assert call(descs((0, 0, 61, 3), win=(0, 0, 1, 1)), 1, big, 3) == EINVAL
  assert call(ok, 1, big, 3, ho=0) == EINVAL
  assert call(descs((16, 23, 61, 3)), 1, 4224, 3) == EINVAL
  assert call(descs((8, 23, 61, 3)), 1, big, 3) == EINVAL
  assert call(descs((-16, 23, 61, 3)), 1, big, 3) == EINVAL
  assert call(ok, 1, big, 3, pk=packed + 8) == EINVAL           # misalignments
  assert call(ok, 1, big + 8, 3) == EINVAL
  assert call(ok, 1, big, 3, o=out + 2) == EINVAL
  assert call(ok, 1, big, 3, desc_dev=dev + 4) == EINVAL
  assert call(descs((0, 5000, 4000, 1), win=(0, 0, 10, 10)), 1, big, 1) == EINVAL
  # the window: inside the image, not empty
  for win in ((0, 0, 24, 61), (1, 0, 23, 61), (0, 0, 23, 62), (0, 12, 23, 50),
              (-1, 0, 23, 61), (0, -1, 23, 61), (0, 0, 0, 61), (0, 0, 23, 0),
              (0, 0, -3, 61), (2 ** 31 - 1, 0, 1, 1), (0, 2 ** 31 - 1, 1, 1)):
    assert call(descs((0, 23, 61, 3), win=win), 1, big, 3) == EINVAL, win
  # the table index and the tables' place in the buffer
  assert call(descs((0, 23, 61, 3), table=0), 1, big, 3) == EINVAL
  assert call(descs((0, 23, 61, 3), table=2), 1, big, 3, n_tables=2) == EINVAL
  assert call(descs((0, 23, 61, 3), table=-2), 1, big, 3, n_tables=2) == EINVAL
  assert call(descs((0, 23, 61, 3), table=0), 1, big, 3, n_tables=1,
              tables_offset=8) == EINVAL
  assert call(descs((0, 23, 61, 3), table=0), 1, big, 3, n_tables=1,
              tables_offset=-16) == EINVAL
  assert call(descs((0, 23, 61, 3), table=0), 1, 4224, 3, n_tables=1,
              tables_offset=4224 - 752) == EINVAL               # 768 bytes needed
  assert call(ok, 1, big, 3, n_tables=-1) == EINVAL
  assert call(descs((0, 23, 61, 3), flags=2), 1, big, 3) == EINVAL
  # gains: finite and >= 0, in the channels that exist
  for gain in ((-0.5, 1, 1), (1, float('nan'), 1), (1, 1, float('inf')),
               (float('-inf'), 1, 1)):
    assert call(descs((0, 23, 61, 3), gain=gain), 1, big, 3) == EINVAL, gain
  # the int32 products, for ch and cw: (Ho + 1)(ch + 1), (Wo + 1)(cw + 1) < 2^31
  tall = descs((0, 4000, 4000, 1))
  assert call(tall, 1, big, 1, ho=600000, wo=40) == EINVAL
  assert call(tall, 1, big, 1, ho=16, wo=600000) == EINVAL
