"""The order of the argument checks of the five splat backward entries.

Every entry is called with each descriptor below and either all pointers set
(distinct dummy addresses) or exactly one of them NULL, always with a non-NULL
workspace of `workspace_bytes = 0`: the workspace-size check is the last one
before the first device call, so no call reaches a launch or dereferences a
dummy -- the fully valid call returns LSI_EWORKSPACE -- and the code a call
returns tells which check refused it first.  splat_bwd_refusals.json holds the
codes of the library before the backward entries were given one host core;
run this module as a script to record them from the library in the tree
(`python tests/test_splat_bwd_refusals_cpu.py [out.json]`).
"""
import ctypes
import json
import os
import sys

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'splat_bwd_refusals.json')

_HEAD = ['tex', 'disp', 'mask', 'M', 'out_img', 'out_wts']
_TAIL = ['g_tex', 'g_disp_in', 'g_mask']
# the pointer arguments between the descriptor and the workspace
ENTRIES = {
    'lsi_splat_bwd': _HEAD + ['g_img', 'g_wts'] + _TAIL,
    'lsi_splat_bwd_m': _HEAD + ['g_img', 'g_wts'] + _TAIL + ['g_M'],
    'lsi_splat_bwd_disp': (_HEAD + ['out_disp', 'g_img', 'g_wts', 'g_disp_out'] + _TAIL +
                           ['g_M']),
    'lsi_splat_bwd_both': (_HEAD + ['out_img_c', 'out_wts_c', 'g_img', 'g_wts', 'g_img_c',
                                    'g_wts_c'] + _TAIL),
    'lsi_splat_bwd_both_m': (_HEAD + ['out_img_c', 'out_wts_c', 'g_img', 'g_wts', 'g_img_c',
                                      'g_wts_c'] + _TAIL + ['g_M']),
}


def _flag_sets(_C):
  """{0, COMPOSE} x {0, HAS_MASK} x {0, GRAD_M}, each without and with
  LSI_WANT_DISP (which lsi_splat_bwd_disp requires), for every entry."""
  return [c | m | g | w for w in (0, _C.LSI_WANT_DISP) for c in (0, _C.LSI_COMPOSE)
          for m in (0, _C.LSI_HAS_MASK) for g in (0, _C.LSI_GRAD_M)]


def _desc(_C, flags):
  """tests/test_camera_grad_cpu.py::_desc's geometry."""
  d = _C.LsiSplatDesc()
  d.L, d.B, d.H, d.W, d.Ht, d.Wt = 2, 2, 16, 64, 8, 32
  d.tex_sl, d.tex_sb, d.tex_sy, d.tex_sx, d.tex_sc = 2 * 16 * 64 * 3, 16 * 64 * 3, 64 * 3, 3, 1
  d.disp_sl, d.disp_sb, d.disp_sy, d.disp_sx = 2 * 16 * 64, 16 * 64, 64, 1
  d.trg_downsampling, d.max_disp, d.zbuf_scale, d.bg_wt = 0.5, 0.4, 50.0, 1e-11
  d.flags = flags
  return d


def codes(_C, name, flags):
  """The return codes of entry `name` for a descriptor with `flags`:
  [all pointers set, descriptor NULL, then each pointer of ENTRIES[name] NULL
  in turn]."""
  fn = getattr(_C.lib(), name)
  n = len(ENTRIES[name])
  ptrs = [ctypes.c_void_p(0x1000 + 0x100 * i) for i in range(n + 1)]
  d = _desc(_C, flags)
  out = [fn(ctypes.byref(d), *ptrs, 0, None), fn(None, *ptrs, 0, None)]
  for k in range(n):
    args = list(ptrs)
    args[k] = None
    out.append(fn(ctypes.byref(d), *args, 0, None))
  return out


def record(_C):
  return {name: {str(f): codes(_C, name, f) for f in _flag_sets(_C)} for name in ENTRIES}


def test_refusals_are_those_of_the_recorded_library(built_lib):
  from lsi import _C
  with open(DATA) as f:
    want = json.load(f)
  assert sorted(want) == sorted(ENTRIES)
  for name, args in ENTRIES.items():
    assert sorted(want[name]) == sorted(str(f) for f in _flag_sets(_C)), name
    for f in _flag_sets(_C):
      got = codes(_C, name, f)
      assert len(got) == len(args) + 2
      cases = ['-', 'desc'] + args
      diff = [(c, g, w) for c, g, w in zip(cases, got, want[name][str(f)]) if g != w]
      assert not diff, '%s flags=%d: (NULL argument, code, recorded code) %s' % (name, f, diff)
      # every call is refused; the all-set one at the latest by LSI_EWORKSPACE
      assert all(-3 <= c < 0 for c in got), (name, f, got)


if __name__ == '__main__':
  _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  sys.path.insert(0, os.path.join(_root, 'layered-scene-inference_amd'))
  from lsi import _C as _c
  _rows = ['  "%s": {\n%s\n  }' % (name, ',\n'.join(
      '    "%s": %s' % (f, json.dumps(v)) for f, v in by_flags.items()))
           for name, by_flags in record(_c).items()]
  with open(sys.argv[1] if len(sys.argv) > 1 else DATA, 'w') as _f:
    _f.write('{\n%s\n}\n' % ',\n'.join(_rows))
