#!/bin/bash
# Builds the CPU functional emulation of the kernel library (every csrc/*.hip): imagen-pytorch_amd/libimagen_emul.so;
# `NAME -Dflags...` builds libimagen_emul_NAME.so with those flags (an A/B variant of a kernel edit).  Host clang (the ROCm toolchain's),
# no GPU code; skipped when the library is newer than its sources.  See tools/emul/README.md.
set -e
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
P=$ROOT/imagen-pytorch_amd
CL=/opt/rocm/lib/llvm/bin/clang++
OUT=$P/build/emul
mkdir -p $OUT
TAG=""; DEFS=""
if [ -n "${1:-}" ]; then TAG="_$1"; shift; DEFS="$*"; fi       # any other name: the remaining arguments are the -D flags of that variant
LIB=$P/libimagen_emul$TAG.so
TUS="igemm conv_dma conv_stream conv_pw conv_big conv_pro conv_gemm conv_small rowchain elementwise sampler tiles temporal attention linear_xattn capi codesize probe"
SRCS="$(for t in $TUS; do echo $P/csrc/$t.hip; done) $P/csrc/conv_epilogue.h $P/csrc/gca_device.h $P/csrc/conv_families.h $P/csrc/conv_launch.h $P/csrc/lds_dma.h $P/csrc/common.h $ROOT/include/imagen_hip.h $ROOT/tools/emul/emul_runtime.cpp $ROOT/tools/emul/hip/hip_runtime.h $ROOT/tools/emul/build_emul_lib.sh"
if [ -f "$LIB" ]; then
  fresh=1
  for s in $SRCS; do [ "$s" -nt "$LIB" ] && fresh=0; done
  if [ $fresh = 1 ]; then echo "up to date: $LIB"; exit 0; fi
fi
FLAGS="-x c++ -std=c++17 -O1 -fPIC -w -DIMAGEN_EMUL $DEFS -I$ROOT/tools/emul -I$ROOT/include -I$P/csrc"
OBJS=""
for t in $TUS; do
  $CL $FLAGS -c $P/csrc/$t.hip -o $OUT/$t$TAG.o &
  OBJS="$OBJS $OUT/$t$TAG.o"
done
$CL $FLAGS -c $ROOT/tools/emul/emul_runtime.cpp -o $OUT/runtime$TAG.o &
wait
$CL -shared -fPIC -o $LIB $OBJS $OUT/runtime$TAG.o -ldl
echo built $LIB
