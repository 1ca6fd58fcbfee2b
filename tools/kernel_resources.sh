#!/bin/bash
# Register / scratch / LDS use of every kernel in libapgpu.so (compiles each translation unit of the build, with the build's
# flags, to assembly):
#   bash tools/kernel_resources.sh > profiles/<round>/kernel_resources.csv
REPO=$(cd "$(dirname "$0")/.." && pwd)
TMP=$(mktemp -d)
cd $REPO
python3 -m astrophotography_amd._build --commands --obj-dir $TMP > $TMP/units
echo "translation_unit,kernel,vgpr,sgpr_spill,vgpr_spill,scratch_bytes,lds_bytes"
while IFS=$'\t' read -r b src cmd; do
  echo "$cmd -S --cuda-device-only -o $TMP/$b.s 2>/dev/null"
done < $TMP/units | xargs -P ${MAX_JOBS:-$(nproc)} -d '\n' -n 1 bash -c
sort $TMP/units | while IFS=$'\t' read -r b src cmd; do
  python3 - $TMP/$b.s $b <<'PY'
import re,sys
txt=open(sys.argv[1]).read()
for blk in txt.split('  - .agpr_count:')[1:]:
    g=lambda k: (re.search(r'\.%s:\s+(\S+)'%k, blk) or [None,'?'])[1]
    name=g('name')
    try:
        import subprocess
        dem=subprocess.run(['c++filt', name],capture_output=True,text=True).stdout.strip()
    except Exception:
        dem=name
    dem=dem.replace(',',';')
    print('%s,"%s",%s,%s,%s,%s,%s'%(sys.argv[2],dem[:150],g('vgpr_count'),g('sgpr_spill_count'),g('vgpr_spill_count'),g('private_segment_fixed_size'),g('group_segment_fixed_size')))
PY
done
rm -rf $TMP
