"""The training objective's assembly (Trainer.compute_losses), pinned on the CPU.

The loss kernels and the renderer are replaced by stubs that record what they
are called with, so what is left of a step is which call gets which tensor and
argument, in which order, and the fp32 scalar arithmetic that combines the
returned values.  tests/objective_calls.json holds, per configuration, paired
and per direction: the call list, the total and the scalars bit for bit, and
how many aten operators (and how many of them aten.cat) ran.  It was recorded
with this harness, `python tests/test_objective_cpu.py`, on the commit before
lsi/loss/objective.py existed; a later recording must come from a commit whose
objective is known to be right."""
import contextlib
import json
import math
import os
import sys
import types
from unittest import mock

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from conftest import PKG

sys.path.insert(0, PKG)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'objective_calls.json')
B, H, W = 2, 8, 16
ALL_ON = ['--ssim_wt', '.3', '--edge_smooth_wt', '.2', '--depth_sup_wt', '.7',
          '--geo_cons_wt', '.4', '--photo_reproj_wt', '.6']
# name -> (flags, the depth-supervision source, ground-truth disparities staged)
CONFIGS = {
    'defaults': ([], None, False),
    'all_on_px': (ALL_ON, 'px', False),
    'all_on_variants': (ALL_ON + ['--edge_smooth_norm', 'false', '--geo_cons_mode', 'l1',
                                  '--edge_smooth_guide', 'texture',
                                  '--photo_reproj_what', 'image'], 'px', False),
    'all_on_planes': (ALL_ON, 'planes', False),
    'no_indep_splat': (['--indep_splat_wt', '0'], None, False),
    'no_compose_splat_ssim': (['--compose_splat_wt', '0', '--ssim_wt', '.3'], None, False),
    'no_splat_geo_photo': (['--indep_splat_wt', '0', '--compose_splat_wt', '0',
                            '--geo_cons_wt', '.4', '--photo_reproj_wt', '.6'], None, False),
    'l0_self_cons': (['--l0_self_cons', 'true'], None, False),
    'one_layer': (['--n_layers', '1'], None, False),
    'debug_synth_texture': (['--debug_synth_texture', 'true'], None, True),
}
LOSS_STUBS = ('zbuffer_composition_loss', 'view_synthesis_loss', 'ssim_view_synthesis_loss',
              'edge_aware_smoothness_loss', 'depth_supervision_loss',
              'geometric_consistency_loss', 'photometric_reprojection_loss')
# operators that launch nothing: views of their input
VIEWS = {'aten::' + n for n in (
    'alias', 'as_strided', 'detach', 'expand', 'permute', 'select', 'slice', 'split',
    'squeeze', 't', 'transpose', 'unbind', 'unsqueeze', 'view', '_unsafe_view',
    '_reshape_alias', 'lift_fresh')}


class _Counter(TorchDispatchMode):
  """Counts the aten operators that are no views; the stubs pause it."""

  def __init__(self):
    super().__init__()
    self.ops, self.cats, self.paused = 0, 0, False

  def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
    name = func._schema.name
    if not self.paused and name not in VIEWS:
      self.ops += 1
      self.cats += name == 'aten::cat'
    return func(*args, **(kwargs or {}))


def _describe(v):
  if isinstance(v, torch.Tensor):
    flat = v.detach().reshape(-1)
    return '%s%s/%s%s %r..%r' % (
        str(v.dtype).replace('torch.', ''), list(v.shape), list(v.stride()),
        ' grad' if v.requires_grad else '', float(flat[0]), float(flat[-1]))
  if isinstance(v, (list, tuple)):
    return [_describe(x) for x in v]
  return v


@contextlib.contextmanager
def _stubbed(calls, counter):
  """The seven loss functions, disp_regularisers and forward_splat_both replaced
  by recorders.  The n-th loss call returns sqrt(n) (the regularisers: sqrt(n)
  and sqrt(n + 1/2)); the renderer returns constant images."""
  from lsi.geometry import ldi as ldi_utils
  from lsi.loss import _hip, loss
  n = [0]

  def record(name, args, kw):
    counter.paused = True
    calls.append([name, [_describe(a) for a in args],
                  {k: _describe(kw[k]) for k in sorted(kw)}])

  def scalar(x):
    out = torch.tensor(math.sqrt(x), dtype=torch.float32)
    counter.paused = False
    return out

  def loss_stub(name):
    def stub(*args, **kw):
      record(name, args, kw)
      n[0] += 1
      return scalar(n[0])
    return stub

  def regularisers(*args, **kw):
    record('disp_regularisers', args, kw)
    n[0] += 1
    return scalar(n[0]), scalar(n[0] + 0.5)

  def render(l, *args, **kw):
    record('forward_splat_both', (l,) + args, kw)
    nl, views = l[0].shape[:2]
    out = (torch.full((nl, views, H // 2, W // 2, 3), 0.75), None,
           torch.full((1, views, H // 2, W // 2, 3), 0.875), None)
    counter.paused = False
    return out

  with contextlib.ExitStack() as stack:
    for name in LOSS_STUBS:
      stack.enter_context(mock.patch.object(loss, name, loss_stub(name)))
    stack.enter_context(mock.patch.object(_hip, 'disp_regularisers', regularisers))
    stack.enter_context(mock.patch.object(ldi_utils, 'forward_splat_both', render))
    yield


def _ramp(shape, start):
  """start, start + 1/64, ...: the halves of a tensor stay told apart."""
  n = math.prod(shape)
  return (start + torch.arange(n, dtype=torch.float32) / 64).reshape(shape)


def _options(flags):
  import ldi_enc_dec as script
  argv = ['--n_layers', '2', '--batch_size', str(B), '--img_height', str(H),
          '--img_width', str(W), '--cpu', 'true', '--bf16', 'false'] + list(flags)
  return script, script.apply_dataset_overrides(script.build_parser().parse_args(argv))


def _run(config, paired):
  """One compute_losses under the stubs: the record the fixture keeps."""
  flags, source, gt_disps = CONFIGS[config]
  script, opts = _options(flags)
  nl = opts.n_layers
  tr = script.Trainer(opts)
  tr.device = types.SimpleNamespace(type='cuda')
  tr.host_mats = {'trg': torch.full((B, 4, 4), 5.0), 'src': torch.full((B, 4, 4), 6.0)}
  tr.depth_sup_source = source
  tr.model = types.SimpleNamespace(pair_ldi=None)
  pred = torch.arange(nl * 2 * B * H * W * 4, dtype=torch.float32).reshape(
      nl, 2 * B, H, W, 4).requires_grad_(True)
  tex, disp = pred[..., 0:3], pred[..., 3:4]
  half = lambda t, k: t[:, k * B:(k + 1) * B]
  src, trg = [half(tex, 0), None, half(disp, 0)], [half(tex, 1), None, half(disp, 1)]

  def network(_a, _b):
    tr.model.pair_ldi = [tex, None, disp] if paired else None
    return list(src), list(trg)
  tr.train_model = network
  staged = [torch.full((B, H, W, 3), 0.25), torch.full((B, H, W, 3), 0.5),
            torch.full((B, 4, 4), 2.0), torch.full((B, 4, 4), 3.0)]
  if gt_disps:
    staged += [torch.full((nl, B, H, W, 1), 0.125), torch.full((nl, B, H, W, 1), 0.375)]
  if source is not None:
    staged += [_ramp((2 * B, H, W, 1), 7.0)]
  if source == 'px':
    staged += [_ramp((2 * B,), 9.0)]
  calls, counter = [], _Counter()
  with _stubbed(calls, counter), counter:
    total, scalars = tr.compute_losses(staged)
  return {'calls': calls, 'total': float(total.detach()).hex(),
          'scalars': [[k, float(v.detach()).hex()] for k, v in scalars.items()],
          'ops': counter.ops, 'cats': counter.cats}


def _generate():
  """Writes the fixture: one call per line."""
  rows = []
  for config in CONFIGS:
    for form in ('paired', 'per_direction'):
      r = _run(config, form == 'paired')
      calls = ',\n'.join('   ' + json.dumps(c) for c in r.pop('calls'))
      rows.append(' "%s/%s": {\n  "calls": [\n%s],\n%s}' % (
          config, form, calls,
          ',\n'.join('  %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in r.items())))
  with open(FIXTURE, 'w') as f:
    f.write('{\n' + ',\n'.join(rows) + '\n}\n')


@pytest.fixture(scope='module')
def expected():
  with open(FIXTURE) as f:
    return json.load(f)


@pytest.mark.parametrize('form', ['paired', 'per_direction'])
@pytest.mark.parametrize('config', list(CONFIGS))
def test_calls_scalars_and_operator_counts(config, form, expected):
  want = expected['%s/%s' % (config, form)]
  got = json.loads(json.dumps(_run(config, form == 'paired')))
  for i, (g, w) in enumerate(zip(got['calls'], want['calls'])):
    assert g == w, (i, g, w)
  assert len(got['calls']) == len(want['calls'])
  assert got['scalars'] == want['scalars']
  assert got['total'] == want['total']
  # the step may lose launches (a concatenation made once), it gains none
  assert got['ops'] <= want['ops'] and got['cats'] <= want['cats'], (
      got['ops'], want['ops'], got['cats'], want['cats'])


def test_the_recorded_calls_are_the_expected_kind(expected):
  n = lambda key: len(expected[key]['calls'])
  assert n('all_on_px/paired') == 11 and n('all_on_px/per_direction') == 22
  assert n('defaults/paired') == 5
  # staged ground-truth disparities switch the pairing off
  assert (expected['debug_synth_texture/paired']['calls'] ==
          expected['debug_synth_texture/per_direction']['calls'])
  # no render without a splat weight; the l0 term is plain torch
  names = lambda key: [c[0] for c in expected[key]['calls']]
  assert 'forward_splat_both' not in names('no_splat_geo_photo/paired')
  assert 'zbuffer_composition_loss' not in names('l0_self_cons/paired')


def _coefficients(flags):
  from lsi.loss import objective
  return list(objective.loss_coefficients(_options(flags)[1]).items())


def test_coefficient_table():
  """loss_coefficients: the enabled terms in the order they are added, each with
  the factor its scalar is multiplied by (the 'ssim' row multiplies
  compose_splat_wt * compose_ssim_loss + indep_splat_wt * indep_ssim_loss)."""
  six = [('self_cons', 1.0), ('compose_splat', 1.0), ('indep_splat', 1.0)]
  assert _coefficients([]) == six + [('incr_depth', 10.0), ('disp_smoothness', 0.1)]
  tail = [('incr_depth', 10.0), ('disp_smoothness', 0.1)]
  assert _coefficients(ALL_ON) == six + [('ssim', 0.3)] + tail + [
      ('edge_smooth', 0.2), ('depth_sup', 0.7), ('geo_cons', 0.4), ('photo_reproj', 0.6)]
  # an unnormalised edge term and the l1 geometric term are linear in d: divided
  # by max_disp (1 for the synthetic scenes; then 2, where the division shows)
  linear = ALL_ON + ['--edge_smooth_norm', 'false', '--geo_cons_mode', 'l1']
  assert _coefficients(linear) == six + [('ssim', 0.3)] + tail + [
      ('edge_smooth', 0.2 / 1.0), ('depth_sup', 0.7), ('geo_cons', 0.4 / 1.0),
      ('photo_reproj', 0.6)]
  assert _coefficients(linear + ['--max_disp', '2']) == six + [
      ('ssim', 0.3), ('incr_depth', 10.0 / 2), ('disp_smoothness', 0.1 / (2 * 2)),
      ('edge_smooth', 0.2 / 2), ('depth_sup', 0.7), ('geo_cons', 0.4 / 2),
      ('photo_reproj', 0.6)]
  # the KITTI value
  assert _coefficients(['--max_disp', '0.4']) == six + [
      ('incr_depth', 10.0 / 0.4), ('disp_smoothness', 0.1 / (0.4 * 0.4))]
  # a weight of 0 takes its row out
  assert _coefficients(['--self_cons_wt', '0', '--incr_depth_wt', '0']) == six[1:] + [
      ('disp_smoothness', 0.1)]


if __name__ == '__main__':
  _generate()
