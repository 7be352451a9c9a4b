#!/bin/bash
# Builds the diagnostic variant of the library whose k_cg_persist stamps the export stores (kernels_persist.h FDAPDE_STAMP_EXPORT): persist_engine.hip
# is recompiled with the switch, everything else is linked from the regular build.  -> tools/bin/variants/libfdapde_hip_st.so (cross-compiled here,
# shipped to the GPU box; run there with tools/c3_export_ab.sh)
set -eu
cd "$(dirname "$0")/../fdapde-core_amd/csrc"
make -s -j8
OUT=../../tools/bin/variants
mkdir -p $OUT
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Wall -Wno-unused-result -Wno-unused-function"
/opt/rocm/bin/hipcc $FLAGS -DFDAPDE_STAMP_EXPORT -c -o $OUT/persist_engine_st.o persist_engine.hip
objs=$(ls ../build/*.o | grep -v persist_engine.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -o $OUT/libfdapde_hip_st.so $objs $OUT/persist_engine_st.o -lpthread
rm -f $OUT/persist_engine_st.o
ls -la $OUT
