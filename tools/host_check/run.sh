#!/bin/bash
# Host code of the device gauge log under AddressSanitizer + UBSan, without a GPU: pclaw.hip built with the sanitizers on
# its host side, linked with the kernels' objects, gauge_log_host_check.cpp and hip_shim.cpp (which stands in for the HIP
# runtime: the program's own definitions come before libamdhip64's).  A stand-alone program: nothing is loaded into python.
#   tools/host_check/run.sh [build directory]
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
CSRC=$HERE/../../pyclaw_amd/csrc
OUT=${1:-$(mktemp -d)}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
ARCH=${ARCH:-gfx950}
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer -g"
make -C "$CSRC" kernels_exact.o kernels_fast.o kernels_strict.o
$HIPCC --offload-arch=$ARCH -O1 -std=c++17 -I/opt/rocm/include -ffp-contract=off -DPCL_ARCH="\"$ARCH\"" -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -g \
    -Wno-unused-value -c -o "$OUT/pclaw_san.o" "$CSRC/pclaw.hip"
/opt/rocm/llvm/bin/clang++ -O1 -std=c++17 $SAN -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -c -o "$OUT/hip_shim.o" "$HERE/hip_shim.cpp"
/opt/rocm/llvm/bin/clang++ -O1 -std=c++17 $SAN -c -o "$OUT/check.o" "$HERE/gauge_log_host_check.cpp"
$HIPCC --offload-arch=$ARCH $SAN -o "$OUT/gauge_log_host_check" "$OUT/check.o" "$OUT/hip_shim.o" "$OUT/pclaw_san.o" \
    "$CSRC/kernels_exact.o" "$CSRC/kernels_fast.o" "$CSRC/kernels_strict.o" -ldl
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/gauge_log_host_check"
