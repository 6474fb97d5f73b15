"""The target-disparity gradient of forward_splat, the parts that need no GPU:
the C ABI of lsi_splat_bwd_disp is declared in the header, bound in
lsi/_C.py's SIGNATURES and exported by the library, and it checks its
arguments before any device call."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('lsi_splat_bwd_disp_workspace_bytes', 'lsi_splat_bwd_disp')
EINVAL, ENULL, EWORKSPACE = -1, -2, -3     # include/lsi_hip.h


def _header():
  with open(os.path.join(ROOT, 'include', 'lsi_hip.h')) as f:
    return f.read()


def test_header_declares_the_new_entries():
  h = _header()
  assert re.search(r'size_t\s+lsi_splat_bwd_disp_workspace_bytes\s*\(\s*const LsiSplatDesc\*', h)
  m = re.search(r'int\s+lsi_splat_bwd_disp\s*\(([^)]*)\)\s*;', h)
  assert m
  params = [p.strip() for p in m.group(1).split(',')]
  assert len(params) == 18, params
  assert params[0].startswith('const LsiSplatDesc*')
  assert params[-3].startswith('void* workspace') and params[-1].startswith('lsi_stream_t')


def test_signatures_bind_the_new_entries():
  from lsi import _C
  for n in NEW:
    assert n in _C.SIGNATURES, n
  res, args = _C.SIGNATURES['lsi_splat_bwd_disp']
  assert res is ctypes.c_int and len(args) == 18
  assert args[16] is ctypes.c_size_t
  assert _C.SIGNATURES['lsi_splat_bwd_disp_workspace_bytes'][1] == [_C._DP]


def test_entries_exported_and_check_their_arguments(built_lib):
  from lsi import _C
  lib = _C.lib()
  for n in NEW:
    assert hasattr(ctypes.CDLL(built_lib), n)
  d = _C.LsiSplatDesc()
  d.L, d.B, d.H, d.W, d.Ht, d.Wt = 2, 1, 8, 16, 4, 8
  d.tex_sl, d.tex_sb, d.tex_sy, d.tex_sx, d.tex_sc = 384, 384, 48, 3, 1
  d.disp_sl, d.disp_sb, d.disp_sy, d.disp_sx = 128, 128, 16, 1
  d.trg_downsampling, d.max_disp, d.zbuf_scale = 0.5, 1.0, 10.0
  d.flags = _C.LSI_COMPOSE | _C.LSI_WANT_DISP
  assert int(lib.lsi_splat_bwd_disp_workspace_bytes(ctypes.byref(d))) > \
      int(lib.lsi_splat_bwd_workspace_bytes(ctypes.byref(d)))
  p = ctypes.c_void_p(16)     # never dereferenced: every call below is refused
  def call(desc, g_disp_out=p, g_m=None, nbytes=1 << 30):
    return lib.lsi_splat_bwd_disp(ctypes.byref(desc), p, p, None, p, p, p, p, p, None,
                                  g_disp_out, p, p, None, g_m, p, nbytes, None)
  assert call(d, g_disp_out=None) == ENULL
  assert call(d, g_m=p) == EINVAL            # g_M without LSI_GRAD_M
  assert call(d, nbytes=16) == EWORKSPACE
  plain = _C.LsiSplatDesc.from_buffer_copy(d)
  plain.flags = _C.LSI_COMPOSE                      # no target disparity
  assert call(plain) == EINVAL
  gm = _C.LsiSplatDesc.from_buffer_copy(d)
  gm.flags |= _C.LSI_GRAD_M
  assert call(gm) == ENULL                    # LSI_GRAD_M without g_M
