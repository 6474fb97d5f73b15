"""The contact-sheet kernel (csrc/lsi_visual.hip) through lsi.visualization,
against the float32 NumPy restatement tests/visual_ref.py: every comparison is
`torch.equal`, no tolerance.  Then the evaluation script with
--save_visuals / --save_preds on fixed batches: results.txt must be the bytes
of a run without the flags (see `Replay` for what that takes)."""
import json
import os

import numpy as np
import pytest
import torch

import visual_ref as R

pytestmark = pytest.mark.gpu

KINDS = {R.RGB: 'add_rgb', R.GRAY: 'add_gray', R.LUT: 'add_map'}


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def values(rs, shape, lo=0.0, hi=1.0, special=True):
  """Random values on [lo - 0.2 (hi - lo), hi + 0.2 (hi - lo)] with NaN, +inf,
  -inf, exact lo, exact hi and, on [0, 1], (k + 0.5) / 255 planted."""
  a = (lo + (hi - lo) * (rs.rand(*shape) * 1.4 - 0.2)).astype(np.float32)
  if special:
    flat = a.reshape(-1)
    plant = [np.nan, np.inf, -np.inf, lo, hi] + [
        lo + (hi - lo) * (k + 0.5) / 255 for k in (0, 1, 2, 100, 127, 128, 253, 254)]
    where = rs.choice(flat.size, len(plant), replace=False)
    flat[where] = np.array(plant, np.float32)
  return a


class Pair(object):
  """One sheet built twice: on the device and by the restatement."""

  def __init__(self, dev, cols, cell_h, cell_w, gutter, **kw):
    from lsi.visualization import SheetBuilder, colormap
    self.sb = SheetBuilder(dev, cols, cell_h, cell_w, gutter=gutter, **kw)
    self.ref = R.RefSheet(cols, cell_h, cell_w, gutter=gutter,
                          bg=kw.get('bg', (255, 255, 255)), nan=kw.get('nan', (255, 0, 255)),
                          lut=colormap(kw.get('cmap', 'ember')))

  def add(self, kind, a=None, lo=0., hi=1., zoom=None, ref=None):
    """a, ref: device views; the restatement gets their values."""
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    name = 'cell%d' % len(self.ref.items)
    if kind == R.SKIP:
      self.sb.skip()
    elif kind == R.ABSDIFF:
      assert lo == 0.
      self.sb.add_absdiff(name, a, ref, hi, zoom=zoom)
    else:
      getattr(self.sb, KINDS[kind])(name, a, lo, hi, zoom=zoom)
    self.ref.add(kind, host(a), lo, hi, zoom, host(ref))

  def check(self, got=None):
    got = self.sb.pack() if got is None else got
    want = torch.from_numpy(self.ref.render())
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape)
    got = got.cpu()
    if not torch.equal(got, want):
      bad = (got != want).any(dim=2).nonzero()
      y, x = [int(v) for v in bad[0]]
      pytest.fail('%d pixels differ; first at (%d, %d): got %s, want %s' %
                  (len(bad), y, x, got[y, x].tolist(), want[y, x].tolist()))
    return got


# --- 1. mixed sheet -------------------------------------------------------------------
def mixed(dev, seed=0):
  rs = np.random.RandomState(seed)
  T = lambda a: torch.tensor(a, device=dev)
  p = Pair(dev, 3, 12, 20, 3, bg=(250, 240, 230), nan=(255, 0, 255))
  p.add(R.RGB, T(values(rs, (12, 20, 3))))
  p.add(R.RGB, T(values(rs, (3, 5, 7))).permute(1, 2, 0))         # channels first
  p.add(R.GRAY, T(values(rs, (6, 10))), 0., 1., zoom=2)
  lbhw = T(values(rs, (3, 2, 12, 20, 1), 0.1, 0.9))
  p.add(R.LUT, lbhw[1, 1, :, :, 0], 0.1, 0.9)
  p.add(R.LUT, T(values(rs, (4, 5, 1))), 0., 1., zoom=3)          # 12 x 15 of 12 x 20
  a = T(values(rs, (5, 9, 3)))
  b = T(values(rs, (3, 5, 12)))[:, :, 1:10].permute(1, 2, 0)      # other strides
  b[0, 0] = a[0, 0]                                               # a zero difference
  a[1, 1, 0], b[1, 1, 0] = float('inf'), float('inf')             # inf - inf: NaN
  a[2, 2], b[2, 2] = T(np.float32([100.5 / 255, 0.25, 1.0])), T(np.float32([0, 0.25, 1.0]))
  p.add(R.ABSDIFF, a, lo=0., hi=1. / 3, zoom=2, ref=b)
  c, d = T(values(rs, (12, 20, 1))), T(values(rs, (12, 40)))[:, ::2]
  c[3, 3, 0], d[3, 3] = 127.5 / 255, 0.0
  p.add(R.ABSDIFF, c, lo=0., hi=1., ref=d)
  return p


def test_mixed_sheet(dev):
  p = mixed(dev)
  assert p.sb.rows == 3 and p.sb.size() == (48, 72)
  got = p.check()
  # the planted values did land in the picture
  assert (got == torch.tensor([255, 0, 255], dtype=torch.uint8)).all(dim=2).sum() >= 5
  assert (got[36:, 26:] == torch.tensor([250, 240, 230], dtype=torch.uint8)).all()
  assert p.sb.names[:2] == ['cell0', 'cell1'] and len(p.sb.meta()['ranges']) == 7


# --- 2. row tail and pitch --------------------------------------------------------------
@pytest.mark.parametrize('gutter', [0, 1])
def test_row_tail_and_pitch(dev, gutter):
  rs = np.random.RandomState(3)
  p = Pair(dev, 1, 3, 7, gutter)
  p.add(R.RGB, torch.tensor(values(rs, (3, 7, 3), special=False), device=dev))
  hs, ws = p.sb.size()
  assert (hs, ws) == (3 + 2 * gutter, 7 + 2 * gutter)
  pitch = (3 * ws + 3) // 4 * 4 + (4 if 3 * ws % 4 == 0 else 0)   # 21 -> 24, 27 -> 28
  assert pitch - 3 * ws == 3 - 2 * gutter
  buf = torch.full((64 + hs * pitch + 64,), 0xAB, dtype=torch.uint8, device=dev)
  out = buf[64:64 + hs * pitch].view(hs, pitch)[:, :3 * ws].unflatten(1, (ws, 3))
  assert p.sb.pack(out=out) is out
  p.check(out)
  host = buf.cpu().numpy()
  want = np.full(host.shape, 0xAB, np.uint8)
  p.ref.render_into(want[64:64 + hs * pitch].reshape(hs, pitch))
  assert (host[:64] == 0xAB).all() and (host[-64:] == 0xAB).all()
  assert (host[64:-64].reshape(hs, pitch)[:, 3 * ws:] == 0xAB).all()
  assert np.array_equal(host, want)


# --- 3. repeat, SKIP, full grid ---------------------------------------------------------
def test_repeat_allocates_nothing(dev):
  p = mixed(dev, seed=1)
  first = p.sb.pack()
  second = torch.empty_like(first)
  torch.cuda.synchronize()
  before = torch.cuda.memory_allocated(dev)
  p.sb.pack(out=second)
  assert torch.cuda.memory_allocated(dev) == before
  assert torch.equal(first, second)
  p.check(second)


def test_skip_and_full_grid(dev):
  rs = np.random.RandomState(4)
  p = Pair(dev, 2, 5, 6, 1)
  for k in range(4):                                   # n_items = rows cols = 4
    if k == 1:
      p.add(R.SKIP)
    else:
      p.add(R.LUT, torch.tensor(values(rs, (5, 6), special=False), device=dev))
  assert p.sb.rows == 2 and p.sb.names[1] == '' and p.sb.meta()['ranges'][1] is None
  got = p.check()
  assert (got[1:6, 8:14] == 255).all()                 # the skipped cell is background
  # ... and a sheet of SKIPs alone, or of nothing, is background
  q = Pair(dev, 2, 5, 6, 1, bg=(1, 2, 3))
  q.check()
  q.add(R.SKIP)
  q.check()


# --- 4. one evaluation-sized sheet ----------------------------------------------------
def test_evaluation_sized_sheet(dev):
  """The cells of a 3-layer synthetic iteration at 128 x 384: textures and
  disparities are [l, b] slices of L x B x H x W x C buffers, the renderings
  half size and zoomed."""
  rs = np.random.RandomState(6)
  L, B, H, W = 3, 2, 128, 384
  T = lambda a: torch.tensor(a, device=dev)
  p = Pair(dev, 6, H, W, 2)
  imgs = T(values(rs, (2, B, H, W, 3)))
  tex = [T(values(rs, (L, B, H, W, 3))) for _ in range(2)]
  disp = [T(values(rs, (L, B, H, W, 1), 0., 0.4)) for _ in range(2)]
  p.add(R.RGB, imgs[0, 0])
  p.add(R.RGB, imgs[1, 0])
  for l in range(L):
    for v in range(2):
      p.add(R.RGB, tex[v][l, 0])
      p.add(R.LUT, disp[v][l, 0, :, :, 0], 0., 0.4)
  for v in range(2):
    recons = T(values(rs, (1, B, H // 2, W // 2, 3)))
    rdisp = T(values(rs, (1, B, H // 2, W // 2, 1), 0., 0.4))
    small = T(values(rs, (B, H // 2, W // 2, 3), special=False))
    gt = T(values(rs, (B, H // 2, W // 2, 1), 0., 0.4))
    p.add(R.RGB, recons[0, 0])
    p.add(R.ABSDIFF, recons[0, 0], 0., 0.5, ref=small[0])
    p.add(R.LUT, rdisp[0, 0, :, :, 0], 0., 0.4)
    p.add(R.LUT, gt[0, :, :, 0], 0., 0.4)
    p.add(R.ABSDIFF, rdisp[0, 0], 0., 0.5, ref=gt[0])
    p.add(R.GRAY, T((rs.rand(B, H, W, 1) > 0.6).astype(np.float32))[0, :, :, 0], 0., 1.)
  for v in range(2):
    p.add(R.RGB, T(values(rs, (B, H, W, 3)))[0])
    p.add(R.LUT, T(values(rs, (B, H, W, 1), 0., 0.4))[0, :, :, 0], 0., 0.4)
  assert len(p.sb.names) == 30 and p.sb.size() == (5 * 128 + 12, 6 * 384 + 14)
  assert p.ref.items[14][4] == 2 and p.sb.pack().stride(0) % 4 == 0
  p.check()


# --- errors -----------------------------------------------------------------------------
def test_builder_refusals(dev):
  from lsi.visualization import SheetBuilder
  sb = SheetBuilder(dev, 2, 8, 8)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    sb.add_rgb('x', torch.zeros(8, 8, 3))
  with pytest.raises(RuntimeError, match='fp32'):
    sb.add_rgb('x', torch.zeros(8, 8, 3, device=dev, dtype=torch.float16))
  with pytest.raises(RuntimeError, match='fp32'):
    sb.add_gray('x', torch.zeros(8, 8, device=dev, dtype=torch.int32), 0., 1.)
  with pytest.raises(ValueError, match='H x W x 3'):
    sb.add_rgb('x', torch.zeros(8, 8, 1, device=dev))
  with pytest.raises(ValueError, match='does not fit'):
    sb.add_gray('x', torch.zeros(9, 8, device=dev), 0., 1.)
  with pytest.raises(ValueError, match='does not fit'):
    sb.add_gray('x', torch.zeros(4, 4, device=dev), 0., 1., zoom=3)
  with pytest.raises(ValueError, match='range'):
    sb.add_gray('x', torch.zeros(4, 4, device=dev), 1., 1.)
  with pytest.raises(ValueError, match='one shape'):
    sb.add_absdiff('x', torch.zeros(4, 4, 3, device=dev), torch.zeros(4, 4, 1, device=dev), 1.)
  assert sb.names == []
  with pytest.raises(ValueError, match='out must be'):
    sb.pack(out=torch.empty(3, 3, 3, dtype=torch.uint8, device=dev))


# --- 5. through the script ----------------------------------------------------------------
def _eval_argv(ckpt, extra=()):
  return ['--dataset', 'synthetic', '--synth_scene', 'planes', '--batch_size', '1',
          '--n_layers', '2', '--img_height', '128', '--img_width', '128',
          '--n_obj_max', '2', '--num_eval_iter', '2', '--random_weights', 'true',
          '--checkpoint_dir', str(ckpt)] + list(extra)


class Replay(object):
  """Pins what the evaluation does not reproduce from run to run.  The network's
  forward and forward_splat add in an order that varies (float atomics; the
  splat is reproducible only with LSI_DETERMINISTIC, which the evaluation does
  not set), so two runs WITHOUT any visuals flag write different files: three
  such runs of this configuration gave psnr 11.171727 / 11.171722 / 11.171740 and
  compose_splat_loss_disocc 0.222654 / 0.222652 / 0.222649, and renderings of
  one input differed by 2.4e-7.  The first run records the value of every call
  of the two; in the second the calls are made as well, and return the
  recorded values.  Everything downstream -- masks, metrics, aggregation, the
  file -- is compared byte for byte."""

  def __init__(self):
    self.tape, self.pos, self.recording = {}, {}, True

  def start(self, recording):
    self.recording, self.pos = recording, {}

  @staticmethod
  def copy(v):
    if isinstance(v, (list, tuple)):
      return type(v)(Replay.copy(x) for x in v)
    return v.clone() if isinstance(v, torch.Tensor) else v

  def __call__(self, name, value):
    i = self.pos[name] = self.pos.get(name, -1) + 1
    if self.recording:
      self.tape.setdefault(name, []).append(Replay.copy(value))
      return value
    return Replay.copy(self.tape[name][i])


def _run(tmp_path, name, batches, extra, replay=None, monkeypatch=None):
  import ldi_enc_dec as script
  import ldi_pred_eval as ev
  from lsi.nnutils import eval_metrics
  opts = script.apply_dataset_overrides(ev.build_parser().parse_args(
      _eval_argv(tmp_path / name, extra)))
  opts.debug_synth_texture = False
  opts.synth_dl_eval_data = True
  tester = ev.Tester(opts)
  if batches is None:
    tester.restore()
    return [tester.trainer.data_loader.forward(opts.batch_size) for _ in range(2)]
  if replay is not None:
    restore, splat = ev.Tester.restore, eval_metrics.ldi_utils.forward_splat

    def pinned_restore(self):
      restore(self)
      model = self.trainer.model
      self.trainer.model = lambda *a: replay('model', model(*a))

    monkeypatch.setattr(ev.Tester, 'restore', pinned_restore)
    monkeypatch.setattr(eval_metrics.ldi_utils, 'forward_splat',
                        lambda *a, **k: replay('splat', splat(*a, **k)))
  try:
    tester.test(batches=batches)
  finally:
    if replay is not None:
      monkeypatch.undo()
  res = os.path.join(opts.checkpoint_dir, 'results')
  return res, open(os.path.join(res, 'results.txt'), 'rb').read()


@pytest.fixture(scope='module')
def batches(tmp_path_factory, dev):
  return _run(tmp_path_factory.mktemp('batches'), 'b', None, ())


@pytest.mark.parametrize('device_metrics', ['false', 'true'])
def test_eval_script_saves_visuals_and_keeps_the_results(tmp_path, dev, batches,
                                                         device_metrics, monkeypatch):
  from PIL import Image
  route = ['--device_metrics', device_metrics]
  replay = Replay()
  _, plain = _run(tmp_path, 'plain', batches, route, replay, monkeypatch)
  replay.start(recording=False)
  res, saved = _run(tmp_path, 'saved', batches,
                    route + ['--save_visuals', '1', '--save_preds', 'true'], replay,
                    monkeypatch)
  assert replay.pos == {'model': 1, 'splat': 3}      # 2 iterations: 2 + 4 calls, as before
  print(plain.decode())
  assert saved == plain and len(plain.splitlines()) == 9
  vis = os.path.join(res, 'visuals')
  assert sorted(os.listdir(vis)) == ['index.html', 'iter_000000.png', 'visuals.json']
  assert os.listdir(os.path.join(res, 'preds')) == ['iter_000000.npz']
  # 2 images + 2 layers x 4 + 2 directions x 6 + 4 background cells = 26: 5 rows of 6
  png = np.asarray(Image.open(os.path.join(vis, 'iter_000000.png')))
  assert png.shape == (5 * 128 + 6 * 2, 6 * 128 + 7 * 2, 3) and png.dtype == np.uint8
  meta = json.load(open(os.path.join(vis, 'visuals.json')))
  assert len(meta) == 1 and meta[0]['file'] == 'iter_000000.png'
  assert (meta[0]['rows'], meta[0]['cols'], meta[0]['cell']) == (5, 6, [128, 128])
  names = meta[0]['names']
  assert names[:6] == ['src_im', 'trg_im', 'src_tex_pred_layer_0', 'src_disp_pred_layer_0',
                       'trg_tex_pred_layer_0', 'trg_disp_pred_layer_0']
  assert sorted(names[10:22]) == sorted(
      '%s_%s' % (k, n) for k in ('src', 'trg') for n in (
          'splat_tex', 'vs_loss', 'splat_disp', 'gt_disp', 'depth_loss', 'disocc_mask'))
  assert names[22:] == ['src_gt_tex_bg', 'src_gt_disp_bg', 'trg_gt_tex_bg', 'trg_gt_disp_bg']
  assert len(meta[0]['ranges']) == 26
  page = open(os.path.join(vis, 'index.html')).read()
  assert 'iter_000000.png' in page and 'trg_disocc_mask' in page
  for k, img in enumerate(batches[0][:2]):             # the src_im and trg_im cells
    want = R.item_pixels(R.RGB, img[0].cpu().numpy(), 0., 1., None, (255, 0, 255))
    x0 = 2 + 130 * k
    assert np.array_equal(png[2:130, x0:x0 + 128], want), names[k]
  assert (png[:2] == 255).all() and (png[:, :2] == 255).all()
  z = np.load(os.path.join(res, 'preds', 'iter_000000.npz'))
  want = R.item_pixels(R.RGB, z['src_tex'][0, 0], 0., 1., None, (255, 0, 255))
  assert np.array_equal(png[2:130, 262:390], want), names[2]
  # the predictions of the whole batch
  assert set(z.files) >= {'src_disp', 'src_tex', 'trg_disp', 'trg_tex'}
  for key in ('src', 'trg'):
    assert z[key + '_tex'].shape == (2, 1, 128, 128, 3) and z[key + '_tex'].dtype == np.float32
    assert z[key + '_disp'].shape == (2, 1, 128, 128, 1)
    assert np.isfinite(z[key + '_tex']).all() and np.isfinite(z[key + '_disp']).all()
