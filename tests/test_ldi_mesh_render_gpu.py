"""ldi_render.py --save_mesh on synthetic planes with an untrained model, at
test_ldi_render_gpu.py's shapes: the .ply files are written next to the sheets,
parse, carry the counts render.json lists and equal `ldi_mesh` called on the
same LDI; without the flag the directory holds what it held before."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W, K = 128, 256, 5
MESH = ['--save_mesh', 'true', '--mesh_edge_ratio', '0.8', '--mesh_merge_ratio', '0.95',
        '--mesh_disp_min', '0.002', '--mesh_flip_yz', 'true']


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
  """One run of `render` with the flag and one without on the same two pairs:
  shared, read only."""
  root = tmp_path_factory.mktemp('mesh_render')
  r = _renderer(root / 'a', MESH)
  r.restore()
  batches = [r.trainer.data_loader.forward(1) for _ in range(2)]
  outs, render_batch = [], r.render_batch

  def recording(batch=None):       # what `render` rendered, kept for the comparisons
    outs.append(render_batch(batch))
    return outs[-1]

  r.render_batch = recording
  iters = r.render(batches=batches)
  r.render_batch = render_batch
  plain = _renderer(root / 'b')
  plain_iters = plain.render(batches=batches)
  results = lambda name: os.path.join(str(root / name) + '_results', 'render')
  return {'renderer': r, 'iters': iters, 'batches': batches, 'dir': results('a'), 'outs': outs,
          'plain': plain, 'plain_iters': plain_iters, 'plain_dir': results('b')}


def test_defaults():
  import ldi_render
  from lsi.geometry import mesh
  o = ldi_render.build_parser().parse_args([])
  assert o.save_mesh is False and o.mesh_merge_ratio == 0.0 and o.mesh_disp_min == 1e-3
  assert o.mesh_edge_ratio == mesh.EDGE_RATIO


def test_files_with_the_flag(run):
  from lsi.geometry import mesh
  d = run['dir']
  assert sorted(os.listdir(d)) == ['index.html', 'iter_000000.ply', 'iter_000000.png',
                                   'iter_000001.ply', 'iter_000001.png', 'render.json',
                                   'visuals.json']
  meta = json.load(open(os.path.join(d, 'render.json')))
  assert meta == run['iters'] and len(meta) == 2
  page = open(os.path.join(d, 'index.html')).read()
  for it, entry in enumerate(meta):
    m = entry['mesh']
    assert entry['file'] == 'iter_%06d.png' % it and m['file'] == 'iter_%06d.ply' % it
    v, f = mesh.read_ply(os.path.join(d, m['file']))
    assert (len(v), len(f)) == (m['vertices'], m['faces'])
    assert 0 < len(v) <= 2 * H * W and 0 < len(f) <= 4 * (H - 1) * (W - 1)
    assert f['i'].min() >= 0 and f['i'].max() < len(v) and (f['n'] == 3).all()
    assert '%s</a>: %d vertices, %d faces' % (m['file'], len(v), len(f)) in page


def test_files_equal_ldi_mesh_on_the_same_ldi(run):
  """The file against ldi_mesh and against the restatement on the LDI the frames
  were splatted from (render_batch's K-fold LDI is a repeat of it)."""
  import ldi_mesh_ref as R
  from lsi.geometry import mesh, projection
  assert len(run['outs']) == 2
  for it, (batch, out) in enumerate(zip(run['batches'], run['outs'])):
    ldi = [None if x is None else x[:, :1].contiguous() for x in out['ldi']]
    k_s = batch[2][:1].float()
    par = dict(disp_min=0.002, edge_ratio=0.8, merge_ratio=0.95, flip_yz=True)
    (v, f), = mesh.ldi_mesh(ldi, k_s, **par).to_host()
    fv, ff = mesh.read_ply(os.path.join(run['dir'], 'iter_%06d.ply' % it))
    assert fv.tobytes() == v.tobytes() and ff.tobytes() == f.tobytes()
    # and what render_batch hands out is that mesh
    (v2, f2), = out['mesh'].to_host()
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()
    kinv = projection._inv3(k_s).numpy().reshape(1, 9)
    (wv, wf), = R.mesh(ldi[0].cpu().numpy(), None if ldi[1] is None else ldi[1].cpu().numpy(),
                       ldi[2].cpu().numpy(), kinv, **par)
    assert wv.tobytes() == v.tobytes() and wf.tobytes() == f.tobytes()


def test_flag_off_leaves_the_directory_as_it_was(run):
  d = run['plain_dir']
  assert sorted(os.listdir(d)) == ['index.html', 'iter_000000.png', 'iter_000001.png',
                                   'render.json', 'visuals.json']
  meta = json.load(open(os.path.join(d, 'render.json')))
  assert meta == run['plain_iters']
  assert all(sorted(e) == ['file', 'frames'] for e in meta)
  page = open(os.path.join(d, 'index.html')).read()
  assert '.ply' not in page and 'vertices' not in page
  assert 'mesh' not in run['plain'].render_batch(run['batches'][0])
  # the sheets do not depend on the flag: the same legends
  names = lambda p: [s['names'] for s in json.load(open(os.path.join(p, 'visuals.json')))]
  assert names(d) == names(run['dir'])
