"""Semi-global matching without a GPU: the NumPy restatement (tests/sgm_ref.py)
is a working stereo matcher -- it recovers a known scene, answers the trivial
inputs as it must and reaches the byte bound of a path cost exactly -- the C
entry points refuse bad arguments before any launch, and the preprocessing tool
names and writes its files as the KITTI loader reads them."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import sgm_ref as R


@functools.lru_cache(maxsize=None)
def scene_result(seed, paths):
  left, right, disp, visible = R.step_scene(seed)
  out_l, _ = R.sgm_pair(left, right, D=32, paths=paths)
  return out_l, disp, visible


@pytest.mark.parametrize('paths', [8, 4])
@pytest.mark.parametrize('seed', [1, 2, 3, 4, 5])
def test_restatement_recovers_a_known_scene(seed, paths):
  out_l, disp, visible = scene_result(seed, paths)
  got = out_l > 0
  density = (got & visible).sum() / float(visible.sum())
  within = (np.abs(out_l[got] / 256.0 - disp[got]) <= 1.0).mean()
  print('seed %d paths %d: density %.4f, within 1 px %.4f' % (seed, paths, density, within))
  assert density >= 0.97
  assert within >= 0.97


def test_identical_and_constant_images_give_no_match():
  rs = np.random.RandomState(7)
  img = rs.randint(0, 256, (20, 48, 3)).astype(np.uint8)
  for pair in ((img, img), (np.full_like(img, 90), np.full_like(img, 90))):
    out_l, out_r = R.sgm_pair(*pair, D=16)
    assert not out_l.any() and not out_r.any()     # d0 = 0 everywhere: "no match"


def test_a_pure_shift_reads_back():
  rs = np.random.RandomState(8)
  wide = rs.randint(0, 256, (24, 64 + 5, 1)).astype(np.uint8)
  left, right = wide[:, :64], wide[:, 5:]          # right[x] = left[x + 5]
  out_l, out_r = R.sgm_pair(left, right, D=16)
  # interior (the census window and the match stay inside both images): the
  # winner is 5 at every pixel and its summed cost is 0; the sub-pixel term
  # moves the 16-bit value by (S[4] - S[6]) 128 / (S[4] + S[6]) around 5 * 256
  # -- never by half a pixel or more, and not to one side
  for inner in (out_l[4:-4, 5 + 5:-5].astype(np.int64), out_r[4:-4, 5:-5 - 5].astype(np.int64)):
    assert (inner > 0).all()
    assert ((inner + 128) >> 8 == 5).all()
    assert np.abs(inner - 5 * 256).max() < 128
    assert abs(inner.mean() - 5 * 256) < 8


def test_path_cost_reaches_the_byte_bound_exactly():
  left, right, _, _ = R.step_scene(1, 33, 70, 3)
  hi, lo = {}, {}
  R.sgm_pair(left, right, D=64, p2=193, stats=hi)
  R.sgm_pair(left, right, D=64, p2=120, stats=lo)
  assert hi['max_path_cost'] == 255                # 62 + 193: the saturation case is one
  assert lo['max_path_cost'] == 182                # 62 + 120


def test_block_scene_has_ties():
  left, right = R.block_pair(3, 1, 24, 40, 3)
  st = {}
  R.sgm_pair(left[0], right[0], D=16, stats=st)
  assert st['argmin_ties'] > 50 and st['tie_next'] > 0
  # S[d0 - 1] > S[d0] for a first argmin, so den = 0 cannot occur (sgm_ref.winner)
  assert st['den_zero'] == 0


# -- the C entry points -------------------------------------------------------------
def _call(lib, B=2, H=8, W=12, C=3, left=1, right=1, D=16, P1=10, P2=120, paths=8, uniq=95,
          lr_max=1, out_l=1, out_r=1, ws=1, ws_bytes=None):
  """lsi_sgm_disparity_u8 with host buffers standing in for device memory: a
  call that is refused launches nothing and never touches them."""
  buf = (ctypes.c_char * 64)()
  p = lambda on: ctypes.addressof(buf) if on else None
  if ws_bytes is None:
    ws_bytes = 1 << 40
  return lib.lsi_sgm_disparity_u8(B, H, W, C, p(left), p(right), D, P1, P2, paths, uniq,
                                  lr_max, p(out_l), p(out_r), p(ws), ws_bytes, None)


def test_abi_refusals(built_lib):
  from lsi import _C
  lib = _C.lib()
  EINVAL, ENULL, EWORKSPACE = -1, -2, -3
  for name in ('left', 'right', 'out_l', 'out_r', 'ws'):
    assert _call(lib, **{name: 0}) == ENULL, name
  for d in (0, 8, 24, 272):
    assert _call(lib, D=d) == EINVAL, d
  assert _call(lib, P1=121) == EINVAL              # P1 > P2
  assert _call(lib, P1=-1) == EINVAL
  assert _call(lib, P2=194) == EINVAL
  assert _call(lib, paths=6) == EINVAL
  assert _call(lib, uniq=101) == EINVAL
  assert _call(lib, uniq=-1) == EINVAL
  for dims in (dict(B=0), dict(H=0), dict(W=-3), dict(C=2), dict(C=4)):
    assert _call(lib, **dims) == EINVAL, dims
  need = lib.lsi_sgm_workspace_bytes(2, 8, 12, 3, 16, 8)
  assert need > 0
  assert _call(lib, ws_bytes=need - 1) == EWORKSPACE
  # refusals come in the documented order: arguments, pointers, workspace
  assert _call(lib, D=8, left=0, ws_bytes=0) == EINVAL
  assert _call(lib, left=0, ws_bytes=0) == ENULL


def test_workspace_size(built_lib):
  from lsi import _C
  f = _C.lib().lsi_sgm_workspace_bytes
  for D in (16, 128, 256):
    sizes = [f(b, 375, 1242, 3, D, 8) for b in (1, 2, 3, 8)]
    assert sizes[0] > 0 and sizes == sorted(set(sizes))      # strictly monotone in B
    # the 16-bit volume of both views and no eight of them
    assert 2 * 2 * 375 * 1242 * D <= sizes[0] < 2 * 2 * 375 * 1242 * D + 64 * 375 * 1242
  assert f(1, 8, 8, 3, 128, 8) > f(1, 8, 8, 3, 64, 8)
  for bad in ((0, 8, 8, 3, 16, 8), (1, 0, 8, 3, 16, 8), (1, 8, -1, 3, 16, 8),
              (1, 8, 8, 2, 16, 8), (1, 8, 8, 3, 24, 8), (1, 8, 8, 3, 0, 8),
              (1, 8, 8, 3, 272, 8), (1, 8, 8, 3, 16, 6), (1 << 14, 1 << 7, 1 << 7, 3, 16, 8)):
    assert f(*bad) == 0, bad


def test_no_cpu_fallback(built_lib):
  from lsi.geometry import stereo
  img = torch.zeros(1, 8, 12, 3, dtype=torch.uint8)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    stereo.sgm_disparity(img, img, max_disp=16)
  u16 = torch.tensor([[0, 256, 640, 65535]], dtype=torch.uint16)
  px = stereo.disparity_px(u16)
  assert px.dtype == torch.float32
  assert px.tolist() == [[0.0, 1.0, 2.5, 65535 / 256.0]]


# -- the tool -------------------------------------------------------------------------
def test_parser_defaults():
  from lsi.data.kitti import preprocess
  a = preprocess.build_parser().parse_args(['--kitti_data_root', '/x'])
  assert (a.max_disp, a.p1, a.p2, a.paths, a.uniqueness, a.lr_max) == (128, 10, 120, 8, 95, 1)
  assert a.overwrite is False and a.workers >= 1
  b = preprocess.build_parser().parse_args(
      ['--kitti_data_root', '/x', '--max_disp', '16', '--overwrite', 'true', '--paths', '4'])
  assert b.max_disp == 16 and b.overwrite is True and b.paths == 4
  with pytest.raises(SystemExit):
    preprocess.build_parser().parse_args([])


@pytest.mark.parametrize('split', ['val', 'test'])   # (train loads no disparities)
def test_tool_paths_are_the_loaders(tmp_path, split):
  from lsi.data.kitti import data as kitti
  from lsi.data.kitti import preprocess
  from test_kitti_pipeline_cpu import make_opts, make_tree
  make_tree(tmp_path, split)
  opts = make_opts(tmp_path, split, disparities=True)
  opts.kitti_dl_disparities_px = True
  loader = kitti.DataLoader(opts)
  assert len(loader.img_list_src) == 5
  lefts = preprocess.left_images(str(tmp_path))
  assert sorted(lefts) == sorted(loader.img_list_src)
  for left in lefts:
    i = loader.img_list_src.index(left)
    assert preprocess.right_image(left) == loader.img_list_trg[i]
    assert preprocess.disparity_paths(str(tmp_path), left) == (
        loader.img_list_disp_src[i], loader.img_list_disp_trg[i])


def test_excluded_frame_is_skipped(tmp_path):
  from PIL import Image
  from lsi.data.kitti import preprocess
  seq = '2011_09_26_drive_0117'
  base = os.path.join(str(tmp_path), 'kitti_raw', seq[:10], seq + '_sync', 'image_02', 'data')
  os.makedirs(base)
  for n in (73, 74, 75):
    Image.fromarray(np.zeros((4, 6, 3), np.uint8)).save(os.path.join(base, '%010d.png' % n))
  names = [os.path.basename(p) for p in preprocess.left_images(str(tmp_path))]
  assert names == ['0000000073.png', '0000000075.png']
  assert preprocess.left_images(str(tmp_path), ['2011_09_28_drive_0001']) == []


def test_written_map_reads_back_through_the_loader(tmp_path):
  from lsi.data.kitti import data as kitti
  from lsi.data.kitti import preprocess
  rs = np.random.RandomState(11)
  raw = rs.randint(0, 65536, (9, 14)).astype(np.uint16)
  raw[0, 0], raw[3, 5], raw[8, 13] = 0, 0x1234, 65535
  path = os.path.join(str(tmp_path), 'deep', 'dir', '0000000003_left_initial_disparity.png')
  preprocess.write_disparity_png(path, raw)
  assert os.listdir(os.path.dirname(path)) == [os.path.basename(path)]   # no partial file
  from PIL import Image
  with Image.open(path) as im:
    assert im.mode in ('I;16', 'I;16B', 'I;16L') and im.size == (14, 9)
  back = kitti.load_disparity_px(path, 9, 14)
  assert np.array_equal(back[:, :, 0], (raw / 256.0).astype(np.float32))
  with pytest.raises(ValueError):
    preprocess.write_disparity_png(path, raw.astype(np.int32))
