#!/bin/bash
# tools/build_variant.sh NAME FILE.hip[,FILE2.hip...] "-DFLAG=..." -- an A/B build of libspmv_hip.so with the named kernel files
# compiled differently: spmv-test_amd/lib/libspmv_hip_NAME.so (tools/explore.py takes it as {"lib": "spmv-test_amd/lib/libspmv_hip_NAME.so"})
# A knob that two files read has to be compiled into both: SPMV_T_BLKBITS and SPMV_T_NPT (tiled_chunks.hpp, spmv_internal.hpp)
# take kernels_adaptive.hip,plan_adaptive.hip; SPMV_T_GROUP, SPMV_T_HUGE and SPMV_T_SHORT are read by kernels_adaptive.hip alone,
# SPMV_T_SORTED_FROM by plan_adaptive.hip alone.  SPMV_T_IDENTITY_ORDER takes both files, SPMV_T_IDENTITY_SHARE plan_adaptive.hip,
# SPMV_T_WINDOW_FIRST kernels_adaptive.hip (tiled_chunks.hpp; several libraries side by side: tools/ab_libs.py).
set -e
NAME=$1; FILES=${2//,/ }; DEFS=$3
PKG=$(cd "$(dirname "$0")/../spmv-test_amd" && pwd)
make -s -C "$PKG" lib/libspmv_hip.so
OBJS=""
for f in "$PKG"/build/*.o; do
  case " $(basename -a -s .hip $FILES | tr '\n' ' ')" in
    *" $(basename $f .o) "*) ;;
    *) OBJS="$OBJS $f" ;;
  esac
done
TMPS=""
for FILE in $FILES; do
  TMP="$PKG/build/variant_${NAME}_$(basename $FILE .hip).o.tmp"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -fvisibility-inlines-hidden \
    -I"$PKG/../include" -I"$PKG/csrc" $DEFS -c "$PKG/csrc/$FILE" -o "$TMP"
  TMPS="$TMPS $TMP"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS $TMPS \
  -Wl,--version-script="$PKG/csrc/exports.map" -o "$PKG/lib/libspmv_hip_$NAME.so"
rm -f $TMPS
echo "built $PKG/lib/libspmv_hip_$NAME.so"
