"""The depth accuracy metrics without a GPU: the op route of
lsi.nnutils.eval_metrics against the fp64 restatement (tests/depth_metrics_ref.py),
the crop, the C entry points' refusals and workspace size, the pixel-disparity
loader and the new switches' defaults."""
import ctypes
import os

import numpy as np
import pytest
import torch

import depth_metrics_ref as R

# (shape, arguments): what tests/test_depth_metrics_gpu.py runs on the device
CASES = [
    ((1, 1, 1), dict(empty=0., depth_max=150.)),
    ((3, 20, 28), dict()),
    ((3, 20, 28), dict(median=True)),
    ((2, 64, 96), dict(crop=(5, 51, 7, 90), mask='bool', median=True)),
    ((2, 64, 96), dict(crop=(5, 51, 7, 90), mask='f32', depth_max=40.)),
]


def check_against_table(got, table, near=0):
  """got: name -> (sum, scored images) against the restatement's table: the
  sums within 1e-5 relative (tests/test_depth_metrics_gpu.py has the bound's
  derivation), the delta shares equal up to the `near` pixels that may flip."""
  want = R.totals(table)
  n_min = max(1.0, table[table[:, 9] > 0, 8].min()) if table[:, 9].any() else 1.0
  for k in R.KEYS:
    s, c = float(got[k][0]), float(got[k][1])
    assert c == want[k][1], k
    if k in ('depth_a1', 'depth_a2', 'depth_a3'):
      assert abs(s - want[k][0]) <= near / n_min + 1e-12 * table.shape[0], (k, s, want[k][0])
    else:
      assert abs(s - want[k][0]) <= 1e-5 * abs(want[k][0]), (k, s, want[k][0])


@pytest.mark.parametrize('case', range(len(CASES)))
def test_op_route_matches_the_restatement(case):
  from lsi.nnutils import eval_metrics
  shape, kw = CASES[case]
  pred, gt, kw = R.case_inputs(100 + case, shape, kw)
  scale = np.ones((shape[0],), np.float32)
  table, near = R.per_image_table(pred, gt, scale, margin=1e-4, **kw)
  assert near == 0
  tkw = {k: (torch.tensor(v) if k == 'mask' else v) for k, v in kw.items()}
  got = eval_metrics.depth_accuracy_metrics(
      torch.tensor(pred)[..., None], torch.tensor(gt)[..., None], torch.tensor(scale), **tkw)
  assert ('depth_scale' in got) == bool(kw.get('median'))
  for k, (s, c) in got.items():
    assert np.isfinite(float(s)), k
  check_against_table(got, table)
  if kw.get('median'):
    assert float(got['depth_scale'][0]) == table[:, 7].sum()


def test_op_route_uses_the_averaged_median_and_a_scale():
  from lsi.nnutils import eval_metrics
  # four scored pixels: the median of the predicted depths 0.5, 2, 4, 16 is 3 (the
  # lower one, 2, is what torch.median gives), of the true depths 1, 2, 4, 8 too
  gt = torch.tensor([1., 1 / 2., 1 / 4., 1 / 8.]).view(1, 2, 2)
  pred = torch.tensor([2., 1 / 2., 1 / 4., 1 / 16.]).view(1, 2, 2)
  got = eval_metrics.depth_accuracy_metrics(pred, gt, median=True)
  assert float(got['depth_scale'][0]) == 1.0 and float(got['depth_scale'][1]) == 1.0
  # pixel disparities: gt_scale turns them into inverse depth
  px = gt * 50.
  got2 = eval_metrics.depth_accuracy_metrics(pred, px, torch.tensor([1 / 50.]), median=True)
  for k in R.KEYS:
    assert abs(float(got2[k][0]) - float(got[k][0])) <= 1e-6 * abs(float(got[k][0])) + 1e-12
  # an image without ground truth adds nothing
  got3 = eval_metrics.depth_accuracy_metrics(pred, torch.zeros(1, 2, 2))
  assert all(float(s) == 0 and float(c) == 0 for s, c in got3.values())


def test_garg_crop_known_answers():
  from lsi.nnutils import eval_metrics
  assert eval_metrics.garg_crop(375, 1242) == (153, 371, 44, 1197)
  y0, y1, x0, x1 = eval_metrics.garg_crop(128, 384)
  assert (y0, y1, x0, x1) == (int(0.40810811 * 128), int(0.99189189 * 128),
                              int(0.03594771 * 384), int(0.96405229 * 384))
  assert all(isinstance(v, int) for v in (y0, y1, x0, x1))


def _call(lib, B=2, H=8, W=12, pred=1, gt=1, mask=0, scale=1, crop=None, valid_above=0.,
          dmin=1e-3, dmax=80., flags=0, acc=1, ws=1, ws_bytes=None):
  """lsi_eval_depth_metrics with host buffers standing in for device memory: a
  call that is refused launches nothing and never touches them."""
  buf = (ctypes.c_char * 64)()
  p = lambda on: ctypes.addressof(buf) if on else None
  y0, y1, x0, x1 = crop or (0, H, 0, W)
  if ws_bytes is None:
    ws_bytes = 1 << 30
  return lib.lsi_eval_depth_metrics(B, H, W, p(pred), p(gt), p(mask), p(scale), y0, y1,
                                    x0, x1, valid_above, dmin, dmax, flags, p(acc), None,
                                    p(ws), ws_bytes, None)


def test_abi_refusals(built_lib):
  from lsi import _C
  lib = _C.lib()
  EINVAL, ENULL, EWORKSPACE = -1, -2, -3
  for name in ('pred', 'gt', 'scale', 'acc'):
    assert _call(lib, **{name: 0}) == ENULL, name
  for dims in (dict(B=0), dict(H=0), dict(W=-3)):
    assert _call(lib, **dims) == EINVAL, dims
  for crop in ((4, 4, 0, 12), (0, 8, 6, 5), (-1, 8, 0, 12), (0, 9, 0, 12), (0, 8, 0, 13),
               (0, 8, -2, 12)):
    assert _call(lib, crop=crop) == EINVAL, crop
  assert _call(lib, dmin=0.) == EINVAL
  assert _call(lib, dmin=-1.) == EINVAL
  assert _call(lib, dmin=2., dmax=1.) == EINVAL
  assert _call(lib, valid_above=-1e-6) == EINVAL
  assert _call(lib, flags=4) == EINVAL
  for median in (0, 1):
    need = lib.lsi_eval_depth_workspace_bytes(2, 8, 12, median)
    assert need > 0
    assert _call(lib, flags=2 * median, ws_bytes=need - 1) == EWORKSPACE
  assert b'workspace' in lib.lsi_strerror(EWORKSPACE)


def test_workspace_size(built_lib):
  from lsi import _C
  f = _C.lib().lsi_eval_depth_workspace_bytes
  for median in (0, 1):
    sizes = [f(b, 256, 768, median) for b in (1, 2, 3, 8)]
    assert sizes[0] > 0 and sizes == sorted(set(sizes))       # strictly monotone in B
  for shape in ((1, 1, 1), (3, 20, 28), (4, 256, 768)):
    assert f(*shape, 1) > f(*shape, 0)
  assert f(0, 8, 8, 0) == 0 and f(1, 0, 8, 1) == 0


def _write_disparity_png(path, values):
  from PIL import Image
  Image.fromarray(values.astype(np.uint16)).save(path)


def test_load_disparity_px(tmp_path):
  from lsi.data.kitti import data as kitti
  rs = np.random.RandomState(5)
  raw = rs.randint(1, 60000, size=(6, 10))
  raw[raw % 256 == 0] += 37                  # low bytes that matter
  raw[1, 3] = raw[4, 7] = raw[0, 0] = raw[3, 3] = 0
  raw[2, 5] = 0x1234
  path = os.path.join(str(tmp_path), 'd_left_initial_disparity.png')
  _write_disparity_png(path, raw)
  full = kitti.load_disparity_px(path, 6, 10)
  assert full.shape == (6, 10, 1) and full.dtype == np.float32
  assert np.array_equal(full[:, :, 0], (raw / 256.0).astype(np.float32))
  assert full[2, 5, 0] == 0x12 + 0x34 / 256.0 and full[1, 3, 0] == 0
  # 3 x 5: the centres of the output pixels fall on rows 1, 3, 5 and columns 1,
  # 3, 5, 7, 9; disparities halve with the width
  half = kitti.load_disparity_px(path, 3, 5)
  assert np.array_equal(half[:, :, 0], (raw[1::2, 1::2] / 256.0 * 0.5).astype(np.float32))
  assert half[0, 1, 0] == 0 == half[1, 1, 0]   # the matcher's empty pixels stay empty
  # the high-byte output of --kitti_dl_disparities is what it was
  old = kitti._load_image(path, 6, 10, 1)[0]
  assert np.array_equal(old[:, :, 0], (raw >> 8).astype(np.float32) * np.float32(1.0 / 255))
  with pytest.raises(ValueError, match='16-bit'):
    from PIL import Image
    p8 = os.path.join(str(tmp_path), 'eight.png')
    Image.fromarray((raw % 256).astype(np.uint8)).save(p8)
    kitti.load_disparity_px(p8, 6, 10)


def test_parser_defaults_are_off():
  import ldi_enc_dec
  import ldi_pred_eval
  e = ldi_pred_eval.build_parser().parse_args([])
  assert e.eval_depth is False and e.depth_median_scale is False
  assert e.depth_min == 1e-3 and e.depth_max == 80. and e.depth_crop == 'none'
  assert e.kitti_dl_disparities_px is False
  assert ldi_enc_dec.build_parser().parse_args([]).kitti_dl_disparities_px is False
  on = ldi_pred_eval.build_parser().parse_args(
      ['--eval_depth', 'true', '--depth_crop', 'garg', '--depth_median_scale', 'true',
       '--kitti_dl_disparities_px', 'true'])
  assert on.eval_depth and on.depth_median_scale and on.depth_crop == 'garg'
  assert on.kitti_dl_disparities_px


def test_prefetching_loader_refuses_pixel_disparities():
  import types
  from lsi.data.kitti import pipeline
  loader = types.SimpleNamespace(output_disparities=False, output_disparities_px=True)
  with pytest.raises(ValueError, match='synchronous loader'):
    pipeline.PrefetchLoader(loader, workers=1)


def test_kitti_loader_appends_pixel_disparities(tmp_path):
  from lsi.data.kitti import data as kitti
  from test_kitti_pipeline_cpu import OUT_H, OUT_W, make_opts, make_tree
  make_tree(tmp_path, 'val', disparities=True)

  def batch(**kw):
    opts = make_opts(tmp_path, 'val', **{k: v for k, v in kw.items() if k == 'disparities'})
    opts.kitti_dl_disparities_px = kw.get('px', False)
    if 'split' in kw:
      opts.data_split = kw['split']
    loader = kitti.DataLoader(opts)
    return loader, loader.forward(2)

  _, old = batch(disparities=True)
  assert len(old) == 8
  loader, both = batch(disparities=True, px=True)
  assert len(both) == 10 and all(np.array_equal(a, b) for a, b in zip(old, both[:8]))
  names = loader.src_image_names
  for k, lst in ((8, loader.img_list_disp_src), (9, loader.img_list_disp_trg)):
    assert both[k].shape == (2, OUT_H, OUT_W, 1) and both[k].dtype == np.float32
    for i, name in enumerate(names):
      path = lst[loader.img_list_src.index(name)]
      assert np.array_equal(both[k][i], kitti.load_disparity_px(path, OUT_H, OUT_W))
    assert (both[k] == 0).any() and both[k].max() > 0
  _, px = batch(px=True)
  assert len(px) == 8 and all(np.array_equal(a, b) for a, b in zip(px, both[:6] + both[8:]))
  assert len(batch()[1]) == 6


def test_evaluator_turns_pixel_disparities_into_depth():
  """Tester.eval_depth on KITTI ground truth: gt_scale = 1 / (f_x |t_x|) with
  each view's own intrinsics, the Garg crop, both views scored."""
  import types
  import ldi_pred_eval as ev
  from lsi.nnutils import eval_metrics
  b, h, w = 2, 32, 96
  rs = np.random.RandomState(3)
  inv = {k: torch.tensor(1 / np.exp(rs.uniform(0, 4, (b, h, w, 1))), dtype=torch.float32)
         for k in ('src', 'trg')}
  pred = {k: v * torch.tensor(np.exp(0.3 * rs.randn(b, h, w, 1)), dtype=torch.float32)
          for k, v in inv.items()}
  k_s = torch.tensor([[[64., 0, 48], [0, 64, 16], [0, 0, 1]]]).repeat(b, 1, 1)
  k_t = k_s.clone()
  k_t[:, 0, 0] = 128.
  trans = torch.tensor([[[-0.5], [0.], [0.]]]).repeat(b, 1, 1)
  px = {'src': inv['src'] * 32., 'trg': inv['trg'] * 64.}      # d = f_x |t_x| / depth
  opts = types.SimpleNamespace(img_height=h, img_width=w, depth_min=1e-3, depth_max=80.,
                               depth_crop='garg', depth_median_scale=False, bg_layer_disp=1e-6)
  me = types.SimpleNamespace(opts=opts, trainer=types.SimpleNamespace(device=torch.device('cpu')))
  ldi = lambda k: [None, None, torch.stack([pred[k], pred[k] * 0.5])]
  got = ev.Tester.eval_depth(me, None, ldi('src'), ldi('trg'), k_s, k_t, trans, None, px)
  assert len(got) == 2
  for d, key in zip(got, ('src', 'trg')):
    want = eval_metrics.depth_accuracy_metrics(pred[key], inv[key],
                                               crop=eval_metrics.garg_crop(h, w))
    for name in R.KEYS:
      assert float(d[name][1]) == b
      assert float(d[name][0]) == float(want[name][0]), name   # powers of two: exact
  with pytest.raises(ValueError, match='kitti_dl_disparities_px'):
    ev.Tester.eval_depth(me, None, ldi('src'), ldi('trg'), k_s, k_t, trans, None, None)
