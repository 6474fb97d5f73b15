"""tools/device_asm_sha256.py [-j N] [--keep DIR]: sha256 of every source's gfx950 assembly.

One line per (source, extra flags): build.py's SOURCES under its HIPCC_FLAGS,
plus the hooks build of the three sources that react to LSI_STREAM_HOOKS and the
stamps build of the compact kernel.  The `__hip_cuid_` lines (a hash per
compilation) are dropped before hashing.  Two trees whose tables agree compile
the same device code: what a refactor of the kernels has to show; --keep DIR
leaves the hashed assembly there, to diff where they do not.  No GPU needed.
"""
import concurrent.futures
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'layered-scene-inference_amd'))
import build  # noqa: E402

HOOKS = ['lsi_splat_stream.hip', 'lsi_splat_tile.hip', 'lsi_splat_sweep.hip']
CASES = ([(s, '') for s in build.SOURCES] +
         [(s, '-DLSI_STREAM_HOOKS=1') for s in HOOKS] +
         [('lsi_splat_stream2.hip', '-DS2X_STAMPS')])


def digest(case):
  src, extra = case
  # (the source is named relative to csrc/, so that no path of the tree can
  # reach the assembly)
  cmd = ([build.hipcc()] + build.HIPCC_FLAGS + extra.split() +
         ['--cuda-device-only', '-S', src, '-o', '-'])
  asm = subprocess.run(cmd, cwd=build.CSRC, check=True, stdout=subprocess.PIPE,
                       stderr=subprocess.DEVNULL).stdout
  kept = b''.join(l for l in asm.splitlines(True) if b'__hip_cuid_' not in l)
  if '--keep' in sys.argv:
    name = src[:-4] + extra.replace('=', '') + '.s'
    with open(os.path.join(sys.argv[sys.argv.index('--keep') + 1], name), 'wb') as f:
      f.write(kept)
  return hashlib.sha256(kept).hexdigest()


if __name__ == '__main__':
  jobs = int(sys.argv[sys.argv.index('-j') + 1]) if '-j' in sys.argv else 8
  with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
    for (src, extra), h in zip(CASES, pool.map(digest, CASES)):
      print('%-28s %-22s %s' % (src, extra or '-', h))
