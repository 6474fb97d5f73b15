"""The host side of the evaluation visuals (lsi/visualization),
without a GPU: the colour maps, the sheet arithmetic, every refusal of
lsi_visual_pack_u8 -- which all come before any launch, so fake device addresses
are never touched --, the NumPy restatement against hand-computed bytes, and
the VisualWriter on host arrays."""
import ctypes
import json
import math
import os
import struct

import numpy as np
import pytest

import visual_ref as R

EINVAL, ENULL = -1, -2


# --- colour maps --------------------------------------------------------------------
def test_colormaps_are_tables_and_repeatable(built_lib):
  from lsi.visualization import colormap
  for name in ('gray', 'ember'):
    a, b = colormap(name), colormap(name)
    assert a.shape == (256, 3) and a.dtype == np.uint8
    assert np.array_equal(a, b) and a is not b
  k = np.arange(256)
  assert np.array_equal(colormap('gray'), np.stack([k, k, k], 1))
  # ordered: the luma grows with every step, so no two entries are equal
  e = colormap('ember').astype(np.int64)
  luma = 77 * e[:, 0] + 150 * e[:, 1] + 29 * e[:, 2]
  assert (np.diff(luma) > 0).all()
  assert tuple(e[0]) == (0, 0, 0) and e[255].min() >= 250
  with pytest.raises(ValueError, match='unknown colour map'):
    colormap('jet')


# --- sheet size ---------------------------------------------------------------------
@pytest.mark.parametrize('rows,cols,ch,cw,g', [(3, 3, 12, 20, 3), (1, 1, 3, 7, 0),
                                               (1, 1, 3, 7, 1), (4, 6, 128, 384, 2)])
def test_sheet_size(built_lib, rows, cols, ch, cw, g):
  from lsi.visualization import sheet_size
  want = (rows * ch + (rows + 1) * g, cols * cw + (cols + 1) * g)
  assert sheet_size(rows, cols, ch, cw, g) == want == R.sheet_size(rows, cols, ch, cw, g)


def test_sheet_size_literals_and_refusals(built_lib):
  from lsi.visualization import sheet_size
  assert sheet_size(3, 3, 12, 20, 3) == (48, 72)
  assert sheet_size(1, 1, 3, 7, 0) == (3, 7)
  assert sheet_size(4, 6, 128, 384, 2) == (522, 2318)
  for bad in ((0, 1, 4, 4, 0), (1, 0, 4, 4, 0), (1, 1, 0, 4, 0), (1, 1, 4, 0, 0),
              (1, 1, 4, 4, -1)):
    with pytest.raises(RuntimeError, match='lsi_visual_sheet_size failed'):
      sheet_size(*bad)


def test_struct_layout(built_lib):
  from lsi import _C
  assert ctypes.sizeof(_C.LsiVisSheet) == 32 and _C.LsiVisSheet.bg.offset == 24
  assert ctypes.sizeof(_C.LsiVisItem) == 96
  assert _C.LsiVisItem.s_y.offset == 16 and _C.LsiVisItem.kind.offset == 64
  assert _C.LsiVisItem.lo.offset == 88


# --- refusals, all before any launch ---------------------------------------------------
FAKE = 0x10000  # stands for device memory: a refused call never reads it


def _call(_C, sheet_kw=None, item_kw=None, n=1, lut=FAKE, out=FAKE, row_bytes=None,
          items_host=True, items_dev=FAKE, sheet=True):
  s = dict(rows=1, cols=2, cell_h=8, cell_w=12, gutter=1, n_items=n)
  s.update(sheet_kw or {})
  sh = _C.LsiVisSheet(**s)
  items = (_C.LsiVisItem * max(n, 1))()
  for k in range(n):
    kw = dict(src=FAKE, kind=_C.LSI_VIS_GRAY, H=8, W=12, C=1, zoom=1, lo=0.0, inv=1.0,
              s_y=12, s_x=1, s_c=1)
    kw.update(item_kw or {})
    for f, v in kw.items():
      setattr(items[k], f, v)
  if row_bytes is None:
    row_bytes = (3 * (sh.cols * sh.cell_w + (sh.cols + 1) * sh.gutter) + 3) // 4 * 4
  return _C.lib().lsi_visual_pack_u8(
      ctypes.byref(sh) if sheet else None, ctypes.addressof(items) if items_host else None,
      items_dev, lut, out, row_bytes, None)


def test_null_pointers_are_refused(built_lib):
  from lsi import _C
  assert _call(_C, sheet=False) == ENULL
  assert _call(_C, out=None) == ENULL
  assert _call(_C, items_host=False) == ENULL
  assert _call(_C, items_dev=None) == ENULL
  assert _call(_C, item_kw=dict(src=None)) == ENULL
  lut_kinds = dict(kind=_C.LSI_VIS_LUT)
  absdiff = dict(kind=_C.LSI_VIS_ABSDIFF, ref=FAKE, r_y=12, r_x=1, r_c=1)
  assert _call(_C, item_kw=lut_kinds, lut=None) == ENULL
  assert _call(_C, item_kw=absdiff, lut=None) == ENULL
  assert _call(_C, item_kw=dict(absdiff, ref=None)) == ENULL


@pytest.mark.parametrize('item_kw', [
    dict(kind=1, C=1), dict(kind=1, C=4),                    # RGB wants 3
    dict(kind=2, C=3), dict(kind=3, C=3), dict(kind=3, C=0),  # GRAY, LUT want 1
    dict(kind=4, ref=FAKE, C=2), dict(kind=5), dict(kind=-1),
    dict(zoom=0), dict(zoom=-2), dict(zoom=2),               # 16 x 24 in 8 x 12
    dict(H=9), dict(W=13), dict(H=0), dict(W=-1),
    dict(H=4, W=6, zoom=3),                                  # 12 x 18 in 8 x 12
    dict(H=1 << 30, zoom=1 << 30),                           # the product in 64 bits
    dict(s_y=-1), dict(s_x=-1), dict(s_c=-1),
    dict(kind=4, ref=FAKE, r_y=-1), dict(kind=4, ref=FAKE, r_x=-5),
    dict(kind=4, ref=FAKE, r_c=-1),
    dict(inv=0.0), dict(inv=-1.0), dict(inv=float('inf')), dict(inv=float('nan')),
    dict(lo=float('nan')), dict(lo=float('inf')),
])
def test_bad_items_are_refused(built_lib, item_kw):
  from lsi import _C
  assert _call(_C, item_kw=item_kw) == EINVAL
  # ... in whichever cell the bad item sits
  sh = _C.LsiVisSheet(rows=1, cols=2, cell_h=8, cell_w=12, gutter=1, n_items=2)
  items = (_C.LsiVisItem * 2)()
  for k in range(2):
    kw = dict(src=FAKE, kind=_C.LSI_VIS_GRAY, H=8, W=12, C=1, zoom=1, lo=0.0, inv=1.0,
              s_y=12, s_x=1, s_c=1)
    if k == 1:
      kw.update(item_kw)
    for f, v in kw.items():
      setattr(items[k], f, v)
  assert _C.lib().lsi_visual_pack_u8(ctypes.byref(sh), ctypes.addressof(items), FAKE,
                                     FAKE, FAKE, 84, None) == EINVAL


def test_bad_sheets_are_refused(built_lib):
  from lsi import _C
  for kw in (dict(rows=0), dict(cols=0), dict(cell_h=0), dict(cell_w=-3),
             dict(gutter=-1)):
    assert _call(_C, sheet_kw=kw, n=0) == EINVAL, kw
  assert _call(_C, n=3) == EINVAL                       # 1 x 2 cells
  assert _call(_C, sheet_kw=dict(n_items=-1), n=0) == EINVAL
  # 257 items, though the grid has the cells
  big = dict(rows=20, cols=20, cell_h=8, cell_w=12, gutter=0)
  assert _call(_C, sheet_kw=big, n=257) == EINVAL
  # the sheet is 27 pixels = 81 bytes wide
  assert _call(_C, row_bytes=80) == EINVAL              # too short
  assert _call(_C, row_bytes=81) == EINVAL              # not a multiple of 4
  assert _call(_C, row_bytes=86) == EINVAL
  assert _call(_C, row_bytes=0) == EINVAL
  assert _call(_C, row_bytes=-84) == EINVAL
  for off in (1, 2, 3):
    assert _call(_C, out=FAKE + off) == EINVAL
  assert _call(_C, items_dev=FAKE + 4) == EINVAL
  assert _call(_C, lut=FAKE + 2) == EINVAL
  # more than 2^31 - 1 bytes: by the rows, and by the pitch alone
  tall = dict(rows=30000, cols=1, cell_h=30000, cell_w=1, gutter=0)   # 9e8 rows x 4
  assert _call(_C, sheet_kw=tall, n=0) == EINVAL
  assert _call(_C, n=0, row_bytes=1 << 28) == EINVAL                  # 10 rows
  assert _call(_C, n=0, row_bytes=1 << 40) == EINVAL
  wide = dict(rows=1, cols=1, cell_h=1, cell_w=800000000, gutter=0)   # 2.4e9 bytes
  assert _call(_C, sheet_kw=wide, n=0) == EINVAL


def test_builder_has_no_cpu_path(built_lib):
  from lsi.visualization import SheetBuilder
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    SheetBuilder('cpu', 3, 8, 8)


# --- the restatement against hand-computed bytes -------------------------------------
def _fl(x):
  return struct.unpack('f', struct.pack('f', x))[0]


def _scalar(v, lo, hi):
  """The contract on Python floats, each step rounded to fp32 (a sum or product
  of two fp32 values is exact in a double before that rounding)."""
  v, lo = _fl(v), _fl(lo)
  inv = _fl(1.0 / _fl(_fl(hi) - lo))
  if v != v:
    return None
  t = min(max(_fl(_fl(v - lo) * inv), 0.0), 1.0)
  return int(math.floor(_fl(_fl(t * 255.0) + 0.5)))


HAND = [  # v, lo, hi, byte (None: the NaN marker)
    (0.0, 0, 1, 0), (1.0, 0, 1, 255),             # lo and hi
    (0.2, 0.2, 0.7, 0), (0.7, 0.2, 0.7, 255),
    (-0.2, 0, 1, 0), (1.2, 0, 1, 255),            # outside
    (0.5, 0, 1, 128),                             # 127.5 + 0.5
    (0.25, 0, 0.5, 128),                          # inv = 2 exactly
    (1 / 3., 0, 1, 85),                           # fl(1/3) 255 = 85.00000253 -> 85
    (float('inf'), 0, 1, 255), (float('-inf'), 0, 1, 0), (float('nan'), 0, 1, None),
    # (k + 0.5) / 255: fl(fl((k + 0.5) / 255) 255) is k + 0.5 exactly for these k
    # (the product's error is below half an ulp of k + 0.5), and floor(k + 1) = k + 1
    (0.5 / 255, 0, 1, 1), (1.5 / 255, 0, 1, 2), (100.5 / 255, 0, 1, 101),
    (127.5 / 255, 0, 1, 128), (254.5 / 255, 0, 1, 255),
]


def test_restatement_against_hand_computed_bytes():
  for (val, lo, hi, want) in HAND:
    q, nan = R.quantise(np.array([val], np.float32), lo, hi)
    assert (None if nan[0] else int(q[0])) == want == _scalar(val, lo, hi), (val, lo, hi)
  # ... and 4000 random values against the scalar form
  rs = np.random.RandomState(5)
  v = (rs.rand(4000) * 1.4 - 0.2).astype(np.float32)
  q, nan = R.quantise(v, 0.1, 0.9)
  assert not nan.any()
  assert [int(x) for x in q] == [_scalar(float(x), 0.1, 0.9) for x in v]


def test_restatement_sheet_by_hand():
  """A 2 x 3 GRAY item at zoom 2 and an ABSDIFF item in a 1 x 2 grid of 4 x 7
  cells, gutter 1: every pixel is placed by hand."""
  lut = np.stack([np.arange(256), 255 - np.arange(256), np.full(256, 7)], 1).astype(np.uint8)
  ref = R.RefSheet(2, 4, 7, gutter=1, bg=(9, 8, 7), nan=(1, 2, 3), lut=lut)
  a = np.array([[0.0, 1.0, 0.5], [np.nan, 2.0, -1.0]], np.float32)
  ref.add(R.GRAY, a, 0., 1., zoom=2)
  x = np.array([[[0.9, 0.5, 0.1]]], np.float32)
  y = np.array([[[0.6, 0.5, 0.7]]], np.float32)   # |d| = .3, 0, .6 -> mean .3 -> 0.3 / 0.5
  ref.add(R.ABSDIFF, x, 0., 0.5, zoom=1, ref=y)
  assert ref.size() == (6, 17)
  got = ref.render()
  want = np.empty((6, 17, 3), np.uint8)
  want[:] = (9, 8, 7)
  gray = {0: 0, 1: 255, 2: 128}
  for yy in range(4):
    for xx in range(6):
      sy, sx = yy // 2, xx // 2
      want[1 + yy, 1 + xx] = (1, 2, 3) if (sy, sx) == (1, 0) else (
          gray[sx] if sy == 0 else (255 if sx == 1 else 0))
  d0, d1, d2 = _fl(_fl(0.9) - _fl(0.6)), 0.0, _fl(_fl(0.7) - _fl(0.1))
  q = _scalar(_fl(_fl(_fl(d0 + d1) + d2) * _fl(1 / 3.)), 0, 0.5)
  assert q == 153                                  # 0.6 x 255 = 153
  want[1, 9] = lut[q]
  assert np.array_equal(got, want)
  # the bytes of a row beyond 3 x 17 stay as they were
  buf = np.full((6, 56), 0xAB, np.uint8)
  ref.render_into(buf)
  assert np.array_equal(buf[:, :51].reshape(6, 17, 3), want) and (buf[:, 51:] == 0xAB).all()


# --- the writer -----------------------------------------------------------------------
def _sheets():
  rs = np.random.RandomState(11)
  return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((9, 14), (9, 14),
                                                                      (5, 3))]


def test_writer_round_trip(tmp_path):
  from PIL import Image
  from lsi.visualization import VisualWriter
  sheets = _sheets()
  w = VisualWriter(str(tmp_path / 'visuals'), max_pending=1)
  for i, s in enumerate(sheets):
    w.submit('iter_%06d' % i, s, ['a<b', 'c'], {'rows': 1, 'cols': 2, 'cell': [4, 6],
                                               'gutter': 1, 'ranges': [[0, 1], None]})
    s[:] = 0    # the writer took its own copy
  w.close()
  w.close()
  sheets = _sheets()
  for i, s in enumerate(sheets):
    got = np.asarray(Image.open(str(tmp_path / 'visuals' / ('iter_%06d.png' % i))))
    assert got.dtype == np.uint8 and np.array_equal(got, s)
  meta = json.load(open(str(tmp_path / 'visuals' / 'visuals.json')))
  assert [m['file'] for m in meta] == ['iter_%06d.png' % i for i in range(3)]
  for m, s in zip(meta, sheets):
    assert (m['rows'], m['cols'], m['cell'], m['gutter']) == (1, 2, [4, 6], 1)
    assert m['names'] == ['a<b', 'c'] and m['ranges'] == [[0, 1], None]
    assert (m['height'], m['width']) == s.shape[:2]
  page = open(str(tmp_path / 'visuals' / 'index.html')).read()
  for i in range(3):
    assert 'src="iter_%06d.png"' % i in page
  assert 'a&lt;b' in page and 'a<b' not in page
  with pytest.raises(RuntimeError, match='closed'):
    w.submit('late', sheets[0], [], {})


def test_writer_surfaces_a_failed_write_in_close(tmp_path):
  from lsi.visualization import VisualWriter
  sheets = _sheets()
  w = VisualWriter(str(tmp_path), max_pending=2)
  w.submit('ok', sheets[0], ['x'], {})
  w.submit(os.path.join('no_such_dir', 'bad'), sheets[1], ['x'], {})
  w.submit('after', sheets[2], ['x'], {})   # does not block on the failed one
  with pytest.raises(OSError):
    w.close()
  assert os.path.exists(str(tmp_path / 'ok.png'))
  assert len(json.load(open(str(tmp_path / 'visuals.json')))) == 3
  w = VisualWriter(str(tmp_path))
  with pytest.raises(ValueError, match='uint8'):
    w.submit('f', sheets[0].astype(np.float32), [], {})
  w.close()


def test_writer_holds_max_pending_sheets_in_flight(tmp_path, monkeypatch):
  """A sheet's slot is taken by `submit` and given back only after its file is
  written, so the next `submit` beyond max_pending has to wait for the worker."""
  import threading
  from PIL import Image
  from lsi.visualization import VisualWriter
  gate, save = threading.Event(), Image.Image.save

  def gated_save(self, *a, **k):
    assert gate.wait(60)
    return save(self, *a, **k)

  monkeypatch.setattr(Image.Image, 'save', gated_save)
  sheets = _sheets()
  w = VisualWriter(str(tmp_path), max_pending=2)
  w.submit('a', sheets[0], [], {})
  w.submit('b', sheets[1], [], {})
  assert not w._slots.acquire(blocking=False)    # a third submit would block here
  gate.set()
  w.close()
  assert w._slots.acquire(blocking=False) and w._slots.acquire(blocking=False)
  assert sorted(os.listdir(str(tmp_path))) == ['a.png', 'b.png', 'index.html', 'visuals.json']
