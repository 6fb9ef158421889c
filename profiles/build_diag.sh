#!/bin/bash
# builds profiles/_ab/libxeng_diag.so: the library with -DXENG_DIAGNOSTICS (the host-side XENG_GRID / XENG_MM_STREAMS / XENG_ITEM_ORDER /
# XENG_DBG_STAMPS / XENG_SPECTRA_NSLOT ... switches that the shipped build compiles out).  usage: bash profiles/build_diag.sh
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
B=${TMPDIR:-/tmp}/diagbuild
mkdir -p $B $R/profiles/_ab
cd $R/caltech-bifrost-dsp_amd/csrc
for f in xeng_util xcorr corracc beamform ingest slab ring xeng_bfarray; do
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -DXENG_DIAGNOSTICS -c $f.hip -o $B/$f.o &
done
# the fine-channel family (complex fp32 FFTs: -fno-slp-vectorize as in csrc/Makefile); XENG_SPECTRA_NSLOT lives in upchan_spectra
for f in upchan upchan_corr upchan_beams upchan_spectra dedisp pulse; do
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -fno-slp-vectorize -DXENG_DIAGNOSTICS -c $f.hip -o $B/$f.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/profiles/_ab/libxeng_diag.so $B/*.o
ls -la $R/profiles/_ab/libxeng_diag.so
