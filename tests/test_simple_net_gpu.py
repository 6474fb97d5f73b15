"""The FC-bottleneck network (--use_unet false) in bf16 on the GPU with its `fc`
stack and first up-convolution on the skinny fully-connected kernels
(csrc/lsi_fc.hip): pinned stage by stage to the reference's recorded
activations relative to the library route, traced for library kernels, and
trained next to the library route."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, golden

pytestmark = pytest.mark.gpu

LIBRARY_KERNELS = re.compile(r'miopen|MIOpen|ck::|Cijk_|rocblas|hipblaslt', re.I)
# batch norm over the 4 - 8 values of the bottleneck can turn bf16 noise into
# O(1): only these stages may be exempted, and only where the library route's
# own error exceeds 0.5 stage standard deviations
MAY_BE_EXEMPT = ('encoder/fc/fc_1', 'encoder/fc/fc_2', 'encoder/fc/fc_3',
                 'decoder/upcnv5', 'decoder/upcnv5b')


def _dev():
  if not torch.cuda.is_available():
    pytest.fail('gpu test selected but no ROCm device is visible')
  return torch.device('cuda:0')


class _route(object):
  """LSI_FC_OWN for the block (the route reads it at every call)."""

  def __init__(self, own):
    self.value = '1' if own else '0'

  def __enter__(self):
    self.saved = os.environ.get('LSI_FC_OWN')
    os.environ['LSI_FC_OWN'] = self.value

  def __exit__(self, *exc):
    if self.saved is None:
      del os.environ['LSI_FC_OWN']
    else:
      os.environ['LSI_FC_OWN'] = self.saved
    return False


def _stage_errors(own):
  """RMS error / stage std of every recorded stage of nets.npz['simple'] and of
  the heads' outputs, bf16 autocast, golden weights."""
  import test_nets_golden as G
  from lsi.nnutils import _hip_fc, tf_checkpoint
  dev = _dev()
  g = golden('nets.npz')
  names, _, tf_vars = G._tf_variables(g, 'simple')
  model = G._model('simple')
  loaded, skipped = tf_checkpoint.load_tf_variables(model, tf_vars, strict=True)
  assert not skipped and sorted(loaded) == sorted(names)
  model = model.to(dev).train()
  prefix = {}
  for tf_name, key, _ in tf_checkpoint.variable_map(model):
    if tf_name.endswith('/weights'):
      prefix[tf_name[:-len('/weights')]] = key.rsplit('.', 2)[0]
  mods = dict(model.named_modules())
  got, hooks = {}, []
  for alias, pfx in prefix.items():
    def hook(_m, _i, out, alias=alias):
      got[alias] = out.detach().float().cpu()
    hooks.append(mods[pfx].register_forward_hook(hook))
  imgs = torch.tensor(G._images(g, 'simple'), device=dev)
  before = dict(_hip_fc.CALLS)
  with _route(own), torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
    tex, _, disps = model.predict(imgs)
  for h in hooks:
    h.remove()
  calls = {k: _hip_fc.CALLS[k] - before[k] for k in before}
  errors = []
  stages = [str(s) for s in g['simple_stages']]
  shapes = [tuple(int(d) for d in str(s).split(',')) for s in g['simple_stage_shapes']]
  for alias, shape in zip(stages, shapes):
    out = got[alias]
    if out.dim() == 4:
      out = out.permute(0, 2, 3, 1)
    assert tuple(out.shape) == shape, (alias, tuple(out.shape), shape)
    flat = out.reshape(-1).numpy().astype(np.float64)
    idx = g['simple_act_idx/' + alias]
    want = g['simple_act_val/' + alias].astype(np.float64)
    _, std = g['simple_act_stat/' + alias]
    errors.append((alias, float(np.sqrt(np.mean((flat[idx] - want) ** 2))) /
                   max(float(std), 1e-3)))
  for name, t in (('tex', tex), ('disp', disps)):
    flat = t.detach().float().cpu().reshape(-1).numpy().astype(np.float64)
    idx, want = g['simple_ldi_%s_idx' % name], g['simple_ldi_%s_val' % name].astype(np.float64)
    std = float(np.std(want))
    errors.append(('ldi_' + name, float(np.sqrt(np.mean((flat[idx] - want) ** 2))) /
                   max(std, 1e-3)))
  return errors, calls


def test_every_stage_stays_as_close_to_the_reference_as_the_library_route(built_lib):
  """Per recorded stage: RMS error / stage std of the own route <= 2 x that of
  the library route (LSI_FC_OWN=0, same test) + 2^-8."""
  lib, lib_calls = _stage_errors(False)
  own, own_calls = _stage_errors(True)
  assert lib_calls == {'fc': 0, 'convt': 0, 'declined': 0}
  assert own_calls == {'fc': 3, 'convt': 1, 'declined': 0}
  print('stage, own rms/std, library rms/std')
  failed, exempt = [], []
  for (alias, eo), (alias2, el) in zip(own, lib):
    assert alias == alias2
    print('%-70s %.4f %.4f' % (alias, eo, el))
    if eo <= 2 * el + 2.0 ** -8:
      continue
    if alias in MAY_BE_EXEMPT and el > 0.5:
      exempt.append(alias)
      continue
    failed.append((alias, eo, el))
  print('exempt (library route itself above 0.5 std):', exempt)
  assert not failed, failed


def _trainer(tmp_path, **kw):
  sys.path.insert(0, PKG)
  import ldi_enc_dec as script
  args = ['--dataset', 'kitti', '--kitti_procedural', 'true', '--batch_size', '4',
          '--n_layers', '1', '--use_unet', 'false', '--img_height', '256', '--img_width',
          '256', '--num_iter', '3', '--log_freq', '1000000', '--checkpoint_dir', str(tmp_path),
          '--bf16', 'true']
  for k, v in kw.items():
    args += ['--' + k, str(v)]
  opts = script.apply_dataset_overrides(script.build_parser().parse_args(args))
  torch.manual_seed(0)
  np.random.seed(0)
  tr = script.Trainer(opts)
  tr.setup()
  return tr


def _traced_step(tr):
  from torch.profiler import profile, ProfilerActivity
  from lsi.nnutils import _hip_fc
  for _ in range(2):
    tr.train_step()
  torch.cuda.synchronize()
  before = dict(_hip_fc.CALLS)
  with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    tr.train_step()
    torch.cuda.synchronize()
  calls = {k: _hip_fc.CALLS[k] - before[k] for k in before}
  names = set()
  for e in prof.events():
    if str(e.device_type).endswith('CUDA'):
      names.add(e.name)
  return names, calls


@pytest.mark.parametrize('paired', ['true', 'false'])
def test_traced_training_step_runs_no_library_kernel(tmp_path, built_lib, paired):
  """A bf16 training step of --use_unet false --n_layers 1 at 256 x 256, batch 4,
  lists no MIOpen / CK / rocBLAS / hipBLASLt kernel, and no flagged layer fell
  back; the same filter does fire on the LSI_FC_OWN=0 step."""
  _dev()
  with _route(False):
    names, calls = _traced_step(_trainer(tmp_path / 'lib', batched_pairs=paired))
  assert len(names) > 20, names
  assert calls == {'fc': 0, 'convt': 0, 'declined': 0}
  hits = sorted(n for n in names if LIBRARY_KERNELS.search(n))
  print('library route: %d kernels, library ones: %s' % (len(names), hits))
  assert hits, 'the filter matches nothing on the library route'
  with _route(True):
    names, calls = _traced_step(_trainer(tmp_path / 'own', batched_pairs=paired))
  hits = sorted(n for n in names if LIBRARY_KERNELS.search(n))
  print('own route: %d kernels, library ones: %s, calls %s' % (len(names), hits, calls))
  assert any('fc_stream_kernel' in n for n in names), sorted(names)
  assert not hits, hits
  passes = 1 if paired == 'true' else 2
  assert calls == {'fc': 3 * passes, 'convt': passes, 'declined': 0}


def _fc_grads(tr):
  enc_dec = tr.model.enc_dec
  out = [m.fc.weight.grad.detach().clone() for m in enc_dec.encoder.fc]
  out.append(getattr(enc_dec.decoder, 'upcnv%d' % enc_dec.decoder.nconv)
             .conv.weight.grad.detach().clone())
  return out


def test_ten_adam_steps_next_to_the_library_route(tmp_path, built_lib):
  """Ten Adam steps with the own route and with LSI_FC_OWN=0 from the same seed:
  all six scalars finite.  The first step's gradients of the `fc` weights and of
  the first up-convolution agree between the routes within the bar of
  tests/test_fc_gpu.py's backward test: against an oracle -- here the fp32 step
  from the same seed and batch, the reference's own arithmetic, whose error is
  2^-16 of bf16's -- the own route's error, as a fraction of the largest
  gradient entry, is at most twice the library route's plus 2^-9.

  (A first version of this test bounded the difference between the two routes
  by 0.25 of the largest entry, from an estimate of what the library's bf16
  batch norm over 4 rows can do.  The estimate was wrong about the library:
  its single-layer error against fp64 is 0.03 - 0.46 in the backward test, and
  the two routes differ by 1.48 of the largest entry of the first layer's
  gradient.  The rule the backward test uses needs an oracle; this is it.)

  Measured on MI355X (error against the fp32 step, own | library, fc x 3 and the
  up-convolution): 1.39 | 1.02, 1.32 | 1.01, 0.95 | 1.20, 1.63 | 1.78 of the
  largest entry -- behind three batch norms over 4 rows the first step's bf16
  gradient of EITHER route is dominated by rounding noise, so this comparison
  shows that the routes are equally far from fp32, not that a gradient is
  right; that is what tests/test_fc_gpu.py's backward tests show (0.2 - 0.4 %
  against fp64 autograd).  Loss after ten steps: own 1.4845, library 1.4910.

  The figures do not repeat from the same seed: the batch-norm sums of the
  convolutions' epilogues and the splats are float atomics, and behind the
  4-row batch norms their last bits decide the gradient.  Twelve runs of this
  test in one job (two builds of the library whose convolutions and `fc`
  kernels compute the same bits, six runs each): own 0.96 - 2.41, library
  0.82 - 2.87 of the largest entry, and one of the twelve missed the bar
  (gradient 1: own 2.35 against library 1.08)."""
  _dev()
  runs = {}
  for tag, own, bf16 in (('oracle', False, 'false'), ('library', False, 'true'),
                         ('own', True, 'true')):
    with _route(own):
      tr = _trainer(tmp_path / tag, batched_pairs='true', bf16=bf16)
      batch = tr.feed()
      tr.feed = lambda batch=batch: batch
      w0 = tr.model.enc_dec.encoder.fc[0].fc.weight.detach().clone()
      grads = None
      for step in range(1 if tag == 'oracle' else 10):
        total, scalars = tr.train_step()
        assert len(scalars) >= 6
        assert all(np.isfinite(float(v)) for v in scalars.values()), scalars
        if step == 0:
          grads = _fc_grads(tr)
      runs[tag] = (grads, float(total), w0)
  assert torch.equal(runs['own'][2], runs['oracle'][2])      # same seed: same weights
  assert torch.equal(runs['library'][2], runs['oracle'][2])
  failed = []
  for i, want in enumerate(runs['oracle'][0]):
    scale = float(want.abs().max())
    e_own = float((runs['own'][0][i] - want).abs().max()) / scale
    e_lib = float((runs['library'][0][i] - want).abs().max()) / scale
    assert runs['own'][0][i].stride() == runs['library'][0][i].stride()
    print('first-step gradient %d: error vs fp32, own %.4f library %.4f of the largest entry'
          % (i, e_own, e_lib))
    if not e_own <= 2 * e_lib + 2.0 ** -9:
      failed.append((i, e_own, e_lib))
  print('loss after ten steps: own %.5f library %.5f' % (runs['own'][1], runs['library'][1]))
  assert not failed, failed


def test_captured_graph_step_gives_the_eager_loss(tmp_path, built_lib):
  _dev()
  runs = {}
  for mode in ('false', 'true'):
    tr = _trainer(tmp_path / mode, hip_graph=mode, batched_pairs='true')
    batch = tr.feed()
    tr.feed = lambda batch=batch: batch
    runs[mode] = [float(tr.train_step()[0]) for _ in range(6)]
    if mode == 'true':
      assert tr._graph is not None
  print('eager', runs['false'], 'graph', runs['true'])
  # the own kernels are bitwise reproducible; the remaining library-free step
  # has atomically accumulated splats: a fraction of a step, as the U-Net's test
  for a, b in zip(runs['false'], runs['true']):
    assert abs(a - b) <= 2e-2 * abs(a), runs
