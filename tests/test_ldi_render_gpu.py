"""ldi_render.py on synthetic planes with an untrained model: the frames are
forward_splat's, the target-view frame is the evaluation's rendering bit for
bit, the source view has the fewest holes, the filler leaves no canvas inside
the crop, and the sheet, its page and render.json are written.

Sizes: 128 x 256, the smallest non-square size the network takes (the U-Net
refuses heights and widths that are not multiples of 128, so 64 x 96 cannot be
predicted).  The target-view comparison is `torch.equal` with forward_splat
pinned (`Pinned`): the any-pose kernels are not run-to-run deterministic."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W, K = 128, 256, 5


@pytest.fixture(scope='module')
def dev(built_lib):
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


def _renderer(ckpt, extra=()):
  import ldi_enc_dec as script
  import ldi_render
  argv = ['--dataset', 'synthetic', '--synth_scene', 'planes', '--batch_size', '1',
          '--n_layers', '2', '--img_height', str(H), '--img_width', str(W),
          '--n_obj_max', '2', '--random_weights', 'true', '--render_views', str(K),
          '--num_render_iter', '2', '--trg_splat_downsampling', '1',
          '--checkpoint_dir', str(ckpt), '--results_dir', str(ckpt) + '_results'] + list(extra)
  opts = script.apply_dataset_overrides(ldi_render.build_parser().parse_args(argv))
  return ldi_render.Renderer(opts)


@pytest.fixture(scope='module')
def run(tmp_path_factory, dev):
  """One run of the script's `render` on two pairs, and those pairs rendered
  again by `render_batch` with and without the filler: shared, read only."""
  root = tmp_path_factory.mktemp('render')
  r = _renderer(root / 'a')
  r.restore()
  batches = [r.trainer.data_loader.forward(1) for _ in range(2)]
  iters = r.render(batches=batches)
  filled = r.render_batch(batches[0])
  plain = _renderer(root / 'b', ['--fill_holes', 'false'])
  plain.restore()
  return {'renderer': r, 'iters': iters, 'filled': filled, 'plain': plain, 'batch': batches[0],
          'dir': os.path.join(str(root / 'a') + '_results', 'render')}


def test_camera_parameters():
  import ldi_render
  assert ldi_render.camera_parameters(5, 0.5) == [-0.5, 0.0, 0.5, 1.0, 1.5]
  assert ldi_render.camera_parameters(4, 0.5) == pytest.approx(
      [-0.5, 0.0, 1 / 6, 5 / 6, 1.0, 1.5])
  assert ldi_render.camera_parameters(1, 0.0) == [0.0, 1.0]
  with pytest.raises(ValueError):
    ldi_render.camera_parameters(0, 0.5)


class Pinned(object):
  """forward_splat with its values pinned, as test_visuals_gpu.py's `Replay` pins
  them: the any-pose kernels add a cell's splats in the order of a linked list
  that threads build with exchanges (csrc/lsi_splat_tile.hip: "not run-to-run
  deterministic"), so two renderings of one input differ in the last bits.  Every
  call is made; a call whose arguments equal an earlier call's -- the same LDI
  tensors, equal cameras, equal settings -- must agree with it to that noise and
  returns the earlier values."""

  def __init__(self, real):
    self.real, self.calls, self.replayed = real, [], 0

  @staticmethod
  def same(a, b):
    if isinstance(a, (list, tuple)):
      return (isinstance(b, (list, tuple)) and len(a) == len(b) and
              all(Pinned.same(x, y) for x, y in zip(a, b)))
    if isinstance(a, torch.Tensor):
      return isinstance(b, torch.Tensor) and (a is b or (a.shape == b.shape and torch.equal(a, b)))
    return a == b

  def __call__(self, *args, **kw):
    out = self.real(*args, **kw)
    for args0, kw0, out0 in self.calls:
      if Pinned.same(args0, args) and sorted(kw0) == sorted(kw) and all(
          Pinned.same(kw0[k], kw[k]) for k in kw):
        for a, b in zip(out0, out):
          # summation-order noise of a few terms of O(1) colours
          assert float((a - b).abs().max() / b.abs().max().clamp_min(1.0)) <= 1e-5
        self.replayed += 1
        return out0
    self.calls.append((args, kw, out))
    return out


def test_target_view_frame_is_the_evaluations_rendering(run, monkeypatch):
  from lsi.nnutils import eval_metrics
  pinned = Pinned(eval_metrics.ldi_utils.forward_splat)
  monkeypatch.setattr(eval_metrics.ldi_utils, 'forward_splat', pinned)
  p = run['plain'].render_batch(run['batch'])
  assert p['filled'] is None and p['s'] == [-0.5, 0.0, 0.5, 1.0, 1.5]
  assert tuple(p['raw'].shape) == (1, K, H, W, 3) and tuple(p['wts'].shape) == (1, K, H, W, 1)
  assert len(pinned.calls) == 1 and pinned.replayed == 0          # ONE forward_splat
  recons, _ = eval_metrics.render_view(p['ldi'], None, *p['cams'], run['plain'].opts)
  assert len(pinned.calls) == 1 and pinned.replayed == 1          # ... and the evaluation's
  i = p['s'].index(1.0)
  assert torch.equal(p['raw'][0, i], recons[0, i])
  # the cameras at s = 1 are the pair's, at s = 0 the source's
  k_s, k_t, rot, t = p['cams']
  assert torch.equal(k_t[p['s'].index(0.0)], k_s[0])
  assert torch.equal(rot[p['s'].index(0.0)], torch.eye(3))


def test_source_view_has_the_fewest_holes(run):
  frames = run['filled']['frames']
  assert [f['s'] for f in frames] == run['filled']['s']
  at = {f['s']: f['hole_fraction'] for f in frames}
  print(at)
  assert all(0.0 <= v <= 1.0 for v in at.values())
  for s, v in at.items():
    if abs(s) >= 1:
      assert at[0.0] < v, (s, at)
  for f in frames:
    assert ('psnr_raw' in f) == (f['s'] in (0.0, 1.0)) == ('psnr_filled' in f)
  assert all(np.isfinite(f['psnr_raw']) and np.isfinite(f['psnr_filled'])
             for f in frames if 'psnr_raw' in f)


def test_files(run):
  from PIL import Image
  d = run['dir']
  assert sorted(os.listdir(d)) == ['index.html', 'iter_000000.png', 'iter_000001.png',
                                   'render.json', 'visuals.json']
  meta = json.load(open(os.path.join(d, 'render.json')))
  assert meta == run['iters'] and len(meta) == 2
  for it, entry in enumerate(meta):
    assert entry['file'] == 'iter_%06d.png' % it and len(entry['frames']) == K
    assert [f['s'] for f in entry['frames']] == [-0.5, 0.0, 0.5, 1.0, 1.5]
  # K columns; raw row, filled row, the two real images
  png = np.asarray(Image.open(os.path.join(d, 'iter_000000.png')))
  assert png.shape == (3 * H + 4 * 2, K * W + (K + 1) * 2, 3)
  names = json.load(open(os.path.join(d, 'visuals.json')))[0]['names']
  assert len(names) == 2 * K + 2 and names[0] == 'raw_s_-0.500' and names[K] == 'filled_s_-0.500'
  assert names[-2:] == ['src_im', 'trg_im']
  page = open(os.path.join(d, 'index.html')).read()
  assert 'iter_000001.png' in page and 'filled_s_+1.000' in page


def test_no_canvas_is_left_inside_the_crop(run):
  import hole_fill_ref as R
  from lsi.geometry import fill
  r, o = run['filled'], run['renderer'].opts
  raw, filled, conf = r['raw'][0], r['filled'][0], r['conf']
  y0, x0 = int(round(H * o.splat_bdry_ignore)), int(round(W * o.splat_bdry_ignore))
  crop = (slice(None), slice(y0, H - y0), slice(x0, W - x0))
  hole = (conf == 0)
  seen = 0
  for i in range(K):
    if bool(hole[i].all()):
      continue
    h = hole[i][crop[1:]]
    seen += int(h.sum())
    assert not bool((filled[i][crop[1:]][h] == 1.0).all(dim=-1).any()), r['s'][i]
  assert seen > 0                                   # there were holes to fill
  # and the frames are the filler's, bit for bit
  bg_wt = fill.canvas_weight(o.bg_layer_disp, o.max_disp, o.zbuf_scale, n_layers=2)
  want = R.fill(raw.cpu().numpy(), r['wts'][0, ..., 0].cpu().numpy(), R.SPLAT,
                conf_min=o.fill_conf_min, bg_wt=bg_wt)
  assert np.array_equal(filled.cpu().numpy().view(np.uint32), want.view(np.uint32))
