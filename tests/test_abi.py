"""C-ABI boundary checks that need no GPU: the library builds, loads, exports
every symbol include/lsi_hip.h declares, host-only entry points behave, and the
Python mirror refuses to run without a ROCm device (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden


def declared_symbols():
  text = open(os.path.join(ROOT, 'include', 'lsi_hip.h')).read()
  text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  return sorted(set(re.findall(r'\b(lsi_[a-z_0-9]+)\s*\(', text)))


def test_header_symbols_are_exported(built_lib):
  handle = ctypes.CDLL(built_lib)
  names = declared_symbols()
  assert len(names) >= 14
  for n in names:
    assert hasattr(handle, n), 'symbol %s declared but not exported' % n


def test_binding_covers_the_header(built_lib):
  from lsi import _C
  assert sorted(_C.SIGNATURES) == declared_symbols()
  lib = _C.lib()
  assert lib.lsi_version() == 100
  assert lib.lsi_strerror(0) == b'ok'
  assert b'workspace' in lib.lsi_strerror(-3)
  assert b'unknown' in lib.lsi_strerror(-99)


def test_desc_struct_matches_header_layout(built_lib):
  from lsi import _C
  # 6 int32 + 13 int64 + 4 float + uint32 + 5 int32 = 24 + 104 + 16 + 24
  assert ctypes.sizeof(_C.LsiSplatDesc) == 176
  assert _C.LsiSplatDesc.adapt.offset == 168
  assert ctypes.sizeof(_C.LsiStreamAdapt) == 32
  assert _C.LsiSplatDesc.tex_sl.offset == 24
  assert _C.LsiSplatDesc.trg_downsampling.offset == 128
  assert _C.LsiSplatDesc.flags.offset == 144


def test_layouts_and_constants_match_the_compiler(tmp_path):
  """Everything lsi._C derives from include/lsi_hip.h, held to what the C
  compiler of the ROCm toolchain makes of the same header: the size of every
  struct, the offset and size of every field and the value of every constant,
  as _Static_asserts in one C11 file.  Syntax check only: no GPU, no link, no
  run."""
  import subprocess
  import build as lsi_build  # layered-scene-inference_amd/build.py
  from lsi import _C
  bin_dir = os.path.dirname(os.path.realpath(lsi_build.hipcc()))
  found = [p for p in (os.path.join(bin_dir, 'amdclang'),
                       os.path.join(bin_dir, '..', 'lib', 'llvm', 'bin', 'clang'),
                       os.path.join(bin_dir, '..', 'llvm', 'bin', 'clang'))
           if os.path.exists(p)]
  assert found, 'no clang beside %s' % lsi_build.hipcc()
  lines = ['#include <stddef.h>', '#include "lsi_hip.h"']
  check = lambda cond: lines.append('_Static_assert(%s, "%s");' % (cond, cond))
  n_fields = 0
  for name, cls in _C.STRUCTS.items():
    assert getattr(_C, name) is cls
    check('sizeof(%s) == %d' % (name, ctypes.sizeof(cls)))
    for field, _ in cls._fields_:
      at = getattr(cls, field)
      check('offsetof(%s, %s) == %d' % (name, field, at.offset))
      check('sizeof(((%s*)0)->%s) == %d' % (name, field, at.size))
      n_fields += 1
  for name, value in _C.CONSTANTS.items():
    assert getattr(_C, name) == value
    check('%s == %d' % (name, value))
  assert len(_C.STRUCTS) >= 17 and n_fields >= 222 and len(_C.CONSTANTS) >= 78
  src = tmp_path / 'layouts.c'
  src.write_text('\n'.join(lines) + '\n')
  done = subprocess.run(
      [found[0], '-x', 'c', '-std=c11', '-fsyntax-only', '-Wall', '-Werror',
       '-I', os.path.join(ROOT, 'include'), str(src)],
      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
  assert done.returncode == 0, done.stdout


SNIPPET = '''
/* a comment may hold anything:
#define LSI_NOT 1
int lsi_not(void); */
#ifndef LSI_SNIPPET_H_
#define LSI_SNIPPET_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define LSI_FLAG 4u   /* a flag */
#define LSI_ECODE -3
typedef void* lsi_stream_t; /* hipStream_t */
typedef struct LsiRec {
  int64_t first;           /* bytes */
  int32_t n, tap[3];
  const float* src;        /* device */
  uint8_t bg[2];
} LsiRec;
int lsi_run(const LsiRec* one, const LsiRec many[], const float* data,
            size_t nbytes, lsi_stream_t stream);
const char* lsi_name(int code);
size_t lsi_bytes(void);
#ifdef __cplusplus
}
#endif
#endif /* LSI_SNIPPET_H_ */
'''


def test_header_parser_maps_the_style_and_refuses_the_rest():
  """lsi._C.parse on literal snippets in the header's style: exactly the
  expected ctypes; a declaration it cannot map raises, none is skipped."""
  from lsi import _C
  constants, structs, signatures = _C.parse(SNIPPET)
  assert constants == {'LSI_FLAG': 4, 'LSI_ECODE': -3}
  assert list(structs) == ['LsiRec']
  rec = structs['LsiRec']
  assert issubclass(rec, ctypes.Structure) and rec.__name__ == 'LsiRec'
  assert rec._fields_ == [
      ('first', ctypes.c_int64), ('n', ctypes.c_int32), ('tap', ctypes.c_int32 * 3),
      ('src', ctypes.c_void_p), ('bg', ctypes.c_uint8 * 2)]
  assert ctypes.sizeof(rec) == 40 and rec.src.offset == 24 and rec.bg.offset == 32
  assert signatures == {
      'lsi_run': (ctypes.c_int, [ctypes.POINTER(rec), ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_size_t, ctypes.c_void_p]),
      'lsi_name': (ctypes.c_char_p, [ctypes.c_int]),
      'lsi_bytes': (ctypes.c_size_t, []),
  }
  record = 'typedef struct LsiRec { int32_t n; } LsiRec;\n'
  for bad in ('int lsi_f(long n);',                      # unknown type
              'typedef struct LsiBad { wchar_t c; } LsiBad;',
              'unsigned lsi_f(void);',
              '#define LSI_HALF 0.5',                    # non-integer defines
              '#define LSI_SHIFT (1 << 4)',
              '#define LSI_TEXT "text"',
              'int lsi_f(int (*callback)(int));',        # prototypes it cannot split
              'int lsi_f(int32_t a, b);',
              'int lsi_f(int32_t a)',
              'int lsi_f(int32_t a) { return a; }',
              record + 'int lsi_f(LsiRec by_value);',
              record + 'LsiRec* lsi_f(void);',
              'int lsi_f(const float* rows[]);',
              'typedef struct LsiBad { int32_t* a, b; } LsiBad;',
              'typedef struct LsiBad { int32_t n; } LsiOther;',
              'typedef int lsi_int;',
              '#if LSI_FLAG\n#endif',
              'static const int lsi_k = 1;'):
    with pytest.raises(ValueError):
      _C.parse(bad)


def test_bg_weight_matches_reference_known_answers(built_lib):
  from lsi import _C
  g = golden('known_answers.npz')
  assert abs(_C.bg_weight(1e-3, 0.4, 50) / float(g['bg_wt_kitti']) - 1) < 2e-6
  assert abs(_C.bg_weight(2e-1, 1.0, 50) / float(g['bg_wt_synth']) - 1) < 2e-6
  assert _C.bg_weight(0.0, 1.0, 10) == 0.0


def _desc(_C, L=2, B=2, H=32, W=96, s=0.5, flags=1):
  d = _C.LsiSplatDesc()
  d.L, d.B, d.H, d.W, d.Ht, d.Wt = L, B, H, W, int(H * s), int(W * s)
  d.trg_downsampling, d.max_disp, d.zbuf_scale, d.bg_wt = s, 0.4, 50.0, 1e-11
  d.flags = flags
  return d


def test_rowband_precondition_and_workspace(built_lib):
  from lsi import _C
  lib = _C.lib()
  d = _desc(_C)
  g = golden('fs_kitti_L2_s05.npz')       # rectified stereo: row-band exact
  m = np.ascontiguousarray(g['M'], np.float32)
  assert lib.lsi_rowband_ok(ctypes.byref(d), m.ctypes.data) == 1
  g2 = golden('fs_general_L3_s05.npz')    # 3-D translation: not row-band
  d2 = _desc(_C, L=3, B=2, H=32, W=32)
  m2 = np.ascontiguousarray(g2['M'], np.float32)
  assert lib.lsi_rowband_ok(ctypes.byref(d2), m2.ctypes.data) == 0
  mb = m.copy()
  mb[0, 2, 2] = -1.0                      # normaliser negative: rejected
  assert lib.lsi_rowband_ok(ctypes.byref(d), mb.ctypes.data) == 0
  # one allocation serves every path: max(ATOMIC canvases, STREAM exchange area)
  def stream_need(npass):  # 1-row bands: counters (256-B granules) + 2 rows/band
    return (npass * 2 * 16 * 4 + 255) // 256 * 256 + npass * 2 * 16 * 2 * 48 * 16
  # compose without disparity: one 4-channel canvas per batch element
  assert lib.lsi_splat_workspace_bytes(ctypes.byref(d)) == max(
      2 * 16 * 48 * 4 * 4, stream_need(1))
  d.flags = 1 | 2                         # + disparity: L canvases x 5 channels
  assert lib.lsi_splat_workspace_bytes(ctypes.byref(d)) == max(
      2 * 2 * 16 * 48 * 5 * 4, stream_need(1))
  d.flags = 0                             # independent layers
  assert lib.lsi_splat_workspace_bytes(ctypes.byref(d)) == max(
      2 * 2 * 16 * 48 * 4 * 4, stream_need(2))
  assert lib.lsi_splat_bwd_workspace_bytes(ctypes.byref(d)) == 2 * 2 * 16 * 48 * 16
  bad = _desc(_C, L=0)
  assert lib.lsi_splat_workspace_bytes(ctypes.byref(bad)) == 0
  # a descriptor that names its path asks for that path's need only: the
  # any-pose path keeps 8 disparity ranges per (layer, view), STREAM counters
  # and boundary rows -- not the ATOMIC canvases
  d.flags = 1
  d.path = _C.LSI_PATH_TILE
  assert lib.lsi_splat_workspace_bytes(ctypes.byref(d)) == 2 * 2 * 8 * 8
  d.path = _C.LSI_PATH_STREAM
  assert lib.lsi_splat_workspace_bytes(ctypes.byref(d)) == stream_need(1)


def test_argument_errors_are_reported_before_any_launch(built_lib):
  from lsi import _C
  lib = _C.lib()
  d = _desc(_C)
  null = ctypes.c_void_p(None)
  rc = lib.lsi_splat_fwd(ctypes.byref(d), null, null, null, null, null, null,
                         null, null, 0, null)
  assert rc == -2                          # LSI_ENULL
  bad = _desc(_C, L=-1)
  rc = lib.lsi_splat_fwd(ctypes.byref(bad), null, null, null, null, null, null,
                         null, null, 0, null)
  assert rc == -1                          # LSI_EINVAL
  assert lib.lsi_bilinear_fwd(0, 4, 4, 3, 4, 4, null, null, null, null) == -1
  assert lib.lsi_scatter_add(1, 8, 0, null, null, null, null) == 0


def test_sampling_entry_points_refuse_before_any_launch(built_lib):
  """The seven entry points of csrc/lsi_sampling.hip with NULL pointers: sizes
  are judged first (-1, LSI_EINVAL), then the required pointers (-2,
  LSI_ENULL); neither answer touches the device."""
  from lsi import _C
  lib = _C.lib()
  one = ctypes.c_void_p(64)     # non-NULL, never dereferenced: a NULL follows it
  # name -> (number of pointers before the stream, the required ones, which of
  #          Hs x Ws / Ht x Wt is the image or canvas limited to 2^24)
  entries = {
      'lsi_splat_generic': (3, (0, 1, 2), 'trg'),
      'lsi_splat_generic_bwd': (5, (0, 1, 2), 'trg'),
      'lsi_bilinear_fwd': (3, (0, 1, 2), 'src'),
      'lsi_bilinear_bwd': (5, (0, 1, 2), 'src'),
      'lsi_bilinear_taps': (4, (0, 1, 2, 3), 'src'),
      'lsi_bilinear_taps_bwd': (5, (0,), 'src'),
  }
  for name, (nptr, required, limited) in entries.items():
    fn = getattr(lib, name)
    call = lambda b, hs, ws, c, ht, wt, ptrs=None: fn(
        b, hs, ws, c, ht, wt, *((ptrs or [None] * nptr) + [None]))
    assert call(1, 4, 4, 3, 4, 4) == -2, name
    assert call(0, 4, 4, 3, 4, 4) == -1, name
    assert call(65536, 4, 4, 3, 4, 4) == -1, name
    assert call(65535, 4, 4, 3, 4, 4) == -2, name
    for dims in ((1, 0, 4, 3, 4, 4), (1, 4, -1, 3, 4, 4), (1, 4, 4, 0, 4, 4),
                 (1, 4, 4, 3, 0, 4), (1, 4, 4, 3, 4, 0)):
      assert call(*dims) == -1, (name, dims)
    # the sampled image / the canvas: an area of 2^24 is refused, 2^24 - 1 is not
    area = lambda h, w: (1, h, w, 3, 4, 4) if limited == 'src' else (1, 4, 4, 3, h, w)
    assert call(*area(4096, 4096)) == -1, name
    assert call(*area(1, (1 << 24) - 1)) == -2, name
    # the point count on the other side has to fit the kernels' int32 index
    pts = lambda h, w: (1, 4, 4, 3, h, w) if limited == 'src' else (1, h, w, 3, 4, 4)
    assert call(*pts(65536, 65536)) == -1, name
    assert call(*pts(32768, 65536)) == -1, name            # 2^31
    assert call(*pts(1, 0x7fffffff)) == -1, name           # whole blocks do not fit
    assert call(*pts(1, 0x7fffffff - 255)) == -2, name
    assert call(*pts(32768, 65535)) == -2, name
    # each required pointer on its own
    for miss in required:
      ptrs = [None if k == miss else one for k in range(nptr)]
      assert call(1, 4, 4, 3, 4, 4, ptrs) == -2, (name, miss)
  # lsi_bilinear_taps_bwd(coords, g_taps, g_wts, g_imgs, g_coords): an image
  # gradient cannot be formed without the taps' incoming gradient
  assert lib.lsi_bilinear_taps_bwd(1, 4, 4, 3, 4, 4, one, None, one, one, None,
                                   None) == -2
  # lsi_scatter_add(B, P, N, idx, upd, out)
  sa = lambda b, p, n, ptrs=(None, None, None): lib.lsi_scatter_add(b, p, n, *ptrs, None)
  assert sa(1, 8, 0) == 0 and sa(65535, 8, 0) == 0
  assert sa(0, 8, 4) == -1 and sa(65536, 8, 4) == -1
  assert sa(1, 0, 4) == -1 and sa(1, 8, -1) == -1
  assert sa(1, 8, 4) == -2
  for miss in range(3):
    assert sa(1, 8, 4, [None if k == miss else one for k in range(3)]) == -2, miss


def test_bn_entry_points_answer_on_the_host(built_lib):
  """lsi_bn_workspace_floats and lsi_bn_launch_workgroups: host only.  A shape
  the batch-norm entry points refuse gets 0 from both; one they take, the
  workspace of 16 + 4096 + 3 * 2048 floats per group and 1 ... 2048 workgroups
  per group that cover the group's pixels in whole steps."""
  from lsi import _C
  lib = _C.lib()
  for npix, c, bf16, groups in ((15, 12, 0, 1), (15, 4, 1, 1), (15, 2048, 0, 1),
                                (15, 4096, 1, 1), (0, 32, 0, 1), (15, 32, 0, 0),
                                (15, 32, 1, 65536)):
    assert lib.lsi_bn_launch_workgroups(npix, c, bf16, groups) == 0, (npix, c, bf16, groups)
  assert lib.lsi_bn_workspace_floats(15, 12, 0, 1) == 0
  for npix, c, bf16, groups in ((1, 4, 0, 1), (4, 8, 1, 3), (10007, 64, 0, 2),
                                (2048, 1024, 0, 1), (2052, 1024, 0, 1), (38916, 2048, 1, 1),
                                (1 << 22, 32, 1, 2)):
    wg = lib.lsi_bn_launch_workgroups(npix, c, bf16, groups)
    rows = 256 // (c // (8 if bf16 else 4))
    assert 1 <= wg <= 2048 and (wg - 1) * rows < npix, (npix, c, bf16, groups, wg)
    assert lib.lsi_bn_workspace_floats(npix, c, bf16, groups) == groups * (16 + 4096 + 3 * 2048)
  # (which shapes land where in the launch rule: test_bn_lattice_gpu.py)
  assert lib.lsi_bn_launch_workgroups(1 << 22, 32, 0, 1) == 2048     # the cap


def test_no_cpu_fallback(built_lib):
  from lsi.geometry import ldi, sampling
  tex = torch.rand(1, 1, 8, 8, 3)
  disp = torch.rand(1, 1, 8, 8, 1)
  eye = torch.eye(4).unsqueeze(0)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    ldi.forward_splat_matrix([tex, None, disp], eye)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    sampling.bilinear(torch.rand(1, 4, 4, 1), torch.rand(1, 4, 4, 2))
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    sampling.splat(torch.rand(1, 4, 4, 1), torch.rand(1, 4, 4, 2),
                   torch.zeros(1, 4, 4, 1))


def test_missing_library_fails_loudly(built_lib, monkeypatch):
  from lsi import _C
  monkeypatch.setattr(_C, '_lib', None)
  monkeypatch.setattr(_C, 'SO_PATH', '/nonexistent/liblsi_hip.so')
  with pytest.raises(RuntimeError, match='liblsi_hip.so is missing'):
    _C.lib()
