#!/bin/bash
# tools/build_kt.sh FAM — instrumented library lvi-exc_amd/liblvx_kt_FAM.so: lvx_eval.hip with the per-phase cycle counters of k_family_mfma<FAM>
# (LVX_KTIME), the other objects from the regular build.  Use: LVX_LIB=lvi-exc_amd/liblvx_kt_FAM.so python bench.py --steps 1 --warmup 1 --no-secondary --no-cpu-baseline
# tools/build_kt.sh FOLD — the counters of the two one-lane / one-workgroup chains instead (LVX_KTIME_FOLD): the hub block of k_clear and the phases of k_fold_all
# (with SERIAL=1: of the one-workgroup dense fold k_fold_border_dense).
set -e
FAM=${1:-SurfAcc}
cd "$(dirname "$0")/../lvi-exc_amd"
python build.py > /dev/null
TAG=$(echo "$FAM" | tr -cd 'A-Za-z0-9')
DEFS="-DLVX_KTIME -DLVX_KTIME_FAM=$FAM"
[ "$FAM" = "FOLD" ] && DEFS="-DLVX_KTIME_FOLD"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -fno-gpu-rdc -Wno-unused-result -ffp-contract=fast $DEFS -c csrc/lvx_eval.hip -o /tmp/lvx_eval_kt_$TAG.o
OBJS=""
for s in csrc/*.hip; do f=$(basename "$s" .hip); [ "$f" = "lvx_eval" ] || OBJS="$OBJS csrc/$f.o"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o liblvx_kt_$TAG.so /tmp/lvx_eval_kt_$TAG.o $OBJS -ldl -Wl,-rpath,/opt/rocm/lib
echo liblvx_kt_$TAG.so
