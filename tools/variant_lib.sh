#!/bin/bash
# Development aid: builds a VARIANT of libapgpu.so for same-box A/B measurements.
#   tools/variant_lib.sh <name> "<extra hipcc flags>" <translation unit> [<translation unit> ...]
# recompiles the named units (as `python -m astrophotography_amd._build --commands` lists them, e.g. stack_mad or
# stack_inst_f32_calib_d) with the extra flags (e.g. -DAPGPU_VARIANT_X) into build_variants/<name>/ and links them with the
# production objects of every other unit, in the production order -> build_variants/<name>/libapgpu.so.  Select it at run time
# with APGPU_LIBRARY=build_variants/<name>/libapgpu.so (astrophotography_amd/_lib.py).  Never used by tests or the bench.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; FLAGS=$2; shift 2
OUT=$ROOT/build_variants/$NAME
mkdir -p $OUT
cd $ROOT
OBJS=""
while IFS=$'\t' read -r unit src cmd; do
  obj=$ROOT/astrophotography_amd/csrc/_obj/$unit.o
  for tu in "$@"; do
    if [ "$unit" = "$(basename $tu .hip)" ]; then obj=$OUT/$unit.o; eval "$cmd $FLAGS" & fi
  done
  OBJS="$OBJS $obj"
done < <(python3 -m astrophotography_amd._build --commands --obj-dir $OUT)
wait
for tu in "$@"; do [ -f $OUT/$(basename $tu .hip).o ] || { echo "no object for unit $tu" >&2; exit 1; }; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT/libapgpu.so $OBJS
echo built $OUT/libapgpu.so
