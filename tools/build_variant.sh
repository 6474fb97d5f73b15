#!/bin/bash
# tools/build_variant.sh <name> <source.hip> [-D...]: liblsi_hip_<name>.so = the
# current objects with <source.hip> rebuilt under extra flags (select it with
# LSI_HIP_LIB=<name>).  Experiment builds for A/B runs on the GPU box.  Sources
# and compiler flags are build.py's.
set -e
name=$1; src=$2; shift 2
cd "$(dirname "$0")/../layered-scene-inference_amd"
flags=$(python -c "import build; print(' '.join(build.HIPCC_FLAGS))")
sources=$(python -c "import build; print(' '.join(build.SOURCES))")
obj=csrc/${src%.hip}.$name.o
/opt/rocm/bin/hipcc $flags "$@" -c csrc/$src -o $obj
objs=""
for s in $sources; do
  if [ "$s" == "$src" ]; then objs="$objs $obj"; else objs="$objs csrc/${s%.hip}.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o liblsi_hip_$name.so $objs
echo liblsi_hip_$name.so
