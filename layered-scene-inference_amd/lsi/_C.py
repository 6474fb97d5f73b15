"""ctypes binding of liblsi_hip.so, derived at import from its C ABI,
include/lsi_hip.h: every LSI_* constant, one ctypes.Structure per struct and
SIGNATURES, the argument types of every prototype (the header's opening comment
has the mapping).  Nothing is declared here a second time.

There is NO fallback: if the header or the shared library is missing, or an op
is handed a tensor that does not live on a ROCm device, this module raises.
PyTorch is used only for device memory, streams and autograd bookkeeping.
"""
import ctypes
import os
import re

import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# LSI_HIP_LIB=hooks selects the instrumented build (build.py --hooks) whose
# stream kernel honours the timing-experiment bits of LsiSplatDesc.reserved
# (any other value picks liblsi_hip_<value>.so: experiment builds)
SO_PATH = os.path.join(_PKG, 'liblsi_hip_%s.so' % os.environ['LSI_HIP_LIB'] if
                       os.environ.get('LSI_HIP_LIB') else 'liblsi_hip.so')
HEADER_PATH = os.path.join(os.path.dirname(_PKG), 'include', 'lsi_hip.h')

_SCALARS = {
    'void': None, 'char': ctypes.c_char, 'int': ctypes.c_int, 'float': ctypes.c_float,
    'double': ctypes.c_double, 'size_t': ctypes.c_size_t, 'int8_t': ctypes.c_int8,
    'uint8_t': ctypes.c_uint8, 'uint16_t': ctypes.c_uint16, 'int32_t': ctypes.c_int32,
    'uint32_t': ctypes.c_uint32, 'int64_t': ctypes.c_int64,
}
# [const|volatile] type [*] name [[N] | []]
_DECL = re.compile(r'((?:(?:const|volatile) )*\w+) ?(\*?) ?(\w+) ?(?:\[(\d*)\])?$')


def _declarator(text, structs, where):
  """(name, ctype) of a struct field, a parameter or `restype function`."""
  m = _DECL.match(text.strip())
  if not m:
    raise ValueError('lsi_hip.h: cannot read the declaration `%s`' % text)
  base, star, name, dim = m.group(1).split()[-1], m.group(2), m.group(3), m.group(4)
  if base == 'lsi_stream_t' and not star and dim is None and where == 'param':
    return name, ctypes.c_void_p
  if base not in _SCALARS and base not in structs:
    raise ValueError('lsi_hip.h: unknown type `%s` in `%s`' % (base, text))
  if dim is not None:
    if not star and where == 'field' and dim and _SCALARS.get(base):
      return name, _SCALARS[base] * int(dim)    # T x[N]: an array member
    if not star and where == 'param' and not dim:
      return name, ctypes.c_void_p              # T x[]: the address of an array
    raise ValueError('lsi_hip.h: cannot map the array `%s`' % text)
  if star:
    if where == 'return':
      if base != 'char':
        raise ValueError('lsi_hip.h: cannot map the return type of `%s`' % text)
      return name, ctypes.c_char_p
    typed = where == 'param' and base in structs
    return name, ctypes.POINTER(structs[base]) if typed else ctypes.c_void_p
  if base in structs or base == 'char' or (base == 'void' and where != 'return'):
    raise ValueError('lsi_hip.h: cannot map `%s`' % text)
  return name, _SCALARS[base]


def parse(text):
  """(constants, structs, signatures) of a header written in lsi_hip.h's style;
  raises ValueError on anything it cannot map.  A pure function of the text."""
  constants, structs, signatures = {}, {}, {}
  code, cplusplus = [], False
  for line in re.sub(r'/\*.*?\*/', ' ', text, flags=re.S).splitlines():
    line = line.strip()
    if cplusplus:           # what only a C++ compiler sees is no part of the C ABI
      cplusplus = line != '#endif'
    elif line == '#ifdef __cplusplus':
      cplusplus = True
    elif line.startswith('#define'):
      words = line.split(None, 2)
      if len(words) == 3:   # (a define without a value is the include guard)
        if not re.match(r'-?\d+u?$', words[2]):
          raise ValueError('lsi_hip.h: `%s` is no integer constant' % line)
        constants[words[1]] = int(words[2].rstrip('u'))
    elif line.startswith('#'):
      if not re.match(r'#(include|ifndef|endif)\b', line):
        raise ValueError('lsi_hip.h: cannot read `%s`' % line)
    else:
      code.append(line)
  code = ' '.join(' '.join(code).split())

  def struct(m):
    fields = []
    for stmt in filter(None, (s.strip() for s in m.group(2).split(';'))):
      # `type a, b[N], c`: one type, then the names that share it
      d = re.match(r'(.*?[ *])(\w+(?:\[\d*\])?(?: ?, ?\w+(?:\[\d*\])?)*)$', stmt)
      if not d or ('*' in d.group(1) and ',' in d.group(2)):
        raise ValueError('lsi_hip.h: cannot read the member `%s`' % stmt)
      fields += [_declarator(d.group(1) + n.strip(), structs, 'field')
                 for n in d.group(2).split(',')]
    structs[m.group(1)] = type(m.group(1), (ctypes.Structure,), {'_fields_': fields})
    return ''

  code = re.sub(r'typedef struct (\w+) \{(.*?)\} ?\1 ?;', struct, code)
  *stmts, rest = code.split(';')
  if rest.strip():
    raise ValueError('lsi_hip.h: `%s` does not end in `;`' % rest)
  for stmt in stmts:
    stmt = stmt.strip()
    if stmt in ('', 'typedef void* lsi_stream_t'):  # (mapped by name in _declarator)
      continue
    m = re.match(r'([^(){}]+)\(([^(){}]*)\)$', stmt)
    if not m:
      raise ValueError('lsi_hip.h: cannot read the declaration `%s`' % stmt)
    name, res = _declarator(m.group(1), structs, 'return')
    params = [] if m.group(2).strip() == 'void' else m.group(2).split(',')
    signatures[name] = (res, [_declarator(p, structs, 'param')[1] for p in params])
  return constants, structs, signatures


if not os.path.exists(HEADER_PATH):
  raise RuntimeError('include/lsi_hip.h is missing (%s): the binding of '
                     'liblsi_hip.so is derived from it' % HEADER_PATH)
with open(HEADER_PATH) as _f:
  # LSI_* -> int; Lsi* -> Structure; name -> (restype, argtypes) of every symbol
  CONSTANTS, STRUCTS, SIGNATURES = parse(_f.read())
globals().update(CONSTANTS)
globals().update(STRUCTS)
_DP = ctypes.POINTER(STRUCTS['LsiSplatDesc'])
PATH_NAMES = {v: k[len('LSI_PATH_'):].lower() for k, v in CONSTANTS.items()
              if k.startswith('LSI_PATH_') and v != CONSTANTS['LSI_PATH_AUTO']}

_lib = None


def lib():
  """The loaded shared library; raises if it has not been built."""
  global _lib
  if _lib is None:
    if not os.path.exists(SO_PATH):
      raise RuntimeError(
          'liblsi_hip.so is missing (%s). Build it with '
          '`python layered-scene-inference_amd/build.py`; there is no CPU or '
          'PyTorch fallback for the lsi HIP ops.' % SO_PATH)
    handle = ctypes.CDLL(SO_PATH)
    for name, (res, args) in SIGNATURES.items():
      fn = getattr(handle, name)  # AttributeError => ABI mismatch, loudly
      fn.restype = res
      fn.argtypes = args
    _lib = handle
  return _lib


def check(rc, what):
  if rc != LSI_OK:  # pylint: disable=undefined-variable  (from the header)
    msg = lib().lsi_strerror(rc).decode()
    raise RuntimeError('%s failed: %s (code %d)' % (what, msg, rc))


def require_device(*tensors):
  """Every tensor must be fp32 on one ROCm device; returns that device."""
  dev = None
  for t in tensors:
    if t is None:
      continue
    if not t.is_cuda:
      raise RuntimeError(
          'lsi HIP ops need tensors on a ROCm GPU (got device %s); there is no '
          'CPU fallback' % t.device)
    if t.dtype != torch.float32 and t.dtype != torch.int32:
      raise RuntimeError('lsi HIP ops are fp32 (got %s)' % t.dtype)
    if dev is None:
      dev = t.device
    elif t.device != dev:
      raise RuntimeError('tensors on different devices: %s vs %s' %
                         (dev, t.device))
  return dev


def ptr(t):
  """Device address for a c_void_p parameter: a plain int (every entry point has
  its argtypes declared in SIGNATURES, so ctypes converts it itself -- a
  c_void_p object per argument costs half a microsecond of an eager step that
  makes hundreds of these calls)."""
  return None if t is None else t.data_ptr()


_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream_ptr(device):
  """The current HIP stream of `device` as an integer.  torch's raw accessor
  where it exists: `torch.cuda.current_stream(device).cuda_stream` builds a
  Stream object per call -- 5 us, 160 times per eager training step
  (profiles/r06/host_profile_L4.txt: 0.8 ms of a 10.6 ms launch side)."""
  if _RAW_STREAM is not None:
    idx = device.index
    if idx is None:
      idx = torch.cuda.current_device()
    return _RAW_STREAM(idx)
  return torch.cuda.current_stream(device).cuda_stream


def bg_weight(bg_layer_disp, max_disp, zbuf_scale):
  return float(lib().lsi_bg_weight(float(bg_layer_disp), float(max_disp),
                                   float(zbuf_scale)))
