"""The host side of the fused evaluation metrics, without a GPU: the slot names
of lsi.nnutils._hip_eval against include/lsi_hip.h, MetricAccumulator.sums() /
results() on a host array standing in for the device accumulator, and the
--device_metrics flag of ldi_pred_eval.py."""
import os
import re

import pytest
import torch

from conftest import ROOT


def test_slot_names_match_the_header():
  from lsi.nnutils import _hip_eval
  text = open(os.path.join(ROOT, 'include', 'lsi_hip.h')).read()
  defs = {m.group(1): int(m.group(2))
          for m in re.finditer(r'^#define LSI_EVAL_([A-Z_0-9]+) (\d+)u?\b', text, re.M)}
  assert defs.pop('SLOTS') == _hip_eval.SLOT_COUNT == 16
  assert defs.pop('DISOCC_U8') == _hip_eval.LSI_EVAL_DISOCC_U8
  assert defs.pop('VALID_GT') == _hip_eval.LSI_EVAL_VALID_GT
  assert defs == _hip_eval.SLOTS
  assert sorted(defs.values()) == list(range(16))
  for name, (s, n) in _hip_eval.METRICS.items():
    assert s in defs and n in defs, name


def test_sums_and_results_from_a_host_array():
  from lsi.nnutils import eval_metrics
  acc = eval_metrics.MetricAccumulator('cpu')
  assert acc.results() == {}
  vals = [6.0, 3.0,      # compose_splat_loss
          1.0, 0.5,      # compose_splat_loss_disocc
          0.0, 0.0,      # depth_splat_loss: never scored
          0.0, 0.0,
          45.0, 2.0,     # psnr: two views
          9.0, 4.0, 8.0,  # fg tex, fg disp, fg norm
          5.0, 2.5, 0.0]  # bg sums with an empty normaliser
  acc.acc.copy_(torch.tensor(vals, dtype=torch.float64))
  sums = acc.sums()
  assert sums['compose_splat_loss'] == (6.0, 3.0)
  assert sums['psnr'] == (45.0, 2.0)
  assert sums['fg_tex_error'] == (9.0, 8.0) and sums['fg_disp_error'] == (4.0, 8.0)
  assert sums['bg_tex_error'] == (5.0, 0.0) and sums['bg_disp_error'] == (2.5, 0.0)
  assert all(isinstance(x, float) for pair in sums.values() for x in pair)
  assert len(sums) == 9
  # sum / norm for norm > 0, as eval_metrics.aggregate
  assert acc.results() == {'compose_splat_loss': 2.0, 'compose_splat_loss_disocc': 2.0,
                           'psnr': 22.5, 'fg_tex_error': 1.125, 'fg_disp_error': 0.5}
  acc.reset()
  assert acc.sums()['psnr'] == (0.0, 0.0) and acc.results() == {}


def test_host_tensors_are_refused():
  from lsi.nnutils import eval_metrics
  acc = eval_metrics.MetricAccumulator('cpu')
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    acc.add_rendered(torch.rand(1, 1, 4, 4, 3), None, torch.rand(1, 4, 4, 3), 0.1)


def test_device_metrics_flag_parses_and_defaults_to_false():
  import ldi_pred_eval as ev
  assert ev.build_parser().parse_args([]).device_metrics is False
  assert ev.build_parser().parse_args(['--device_metrics', 'true']).device_metrics is True
  assert ev.build_parser().parse_args(['--device_metrics=false']).device_metrics is False
