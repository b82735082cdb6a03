#!/bin/bash
# Host code of the device gauge log and of the user-written Riemann solvers under AddressSanitizer + UBSan, without a GPU:
# pclaw.hip built with the sanitizers on its host side, linked with the kernels' objects, one of the two check programs
# (gauge_log_host_check.cpp, cellrp_host_check.cpp) and hip_shim.cpp (which stands in for the HIP runtime: the program's
# own definitions come before libamdhip64's).  Stand-alone programs: nothing is loaded into python.
#   tools/host_check/run.sh [build directory]
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
CSRC=$HERE/../../pyclaw_amd/csrc
OUT=${1:-$(mktemp -d)}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
ARCH=${ARCH:-gfx950}
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer -g"
make -C "$CSRC" kernels_exact.o kernels_fast.o kernels_strict.o cellrp_headers.inc
$HIPCC --offload-arch=$ARCH -O1 -std=c++17 -I/opt/rocm/include -ffp-contract=off -DPCL_ARCH="\"$ARCH\"" -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -g \
    -Wno-unused-value -c -o "$OUT/pclaw_san.o" "$CSRC/pclaw.hip"
/opt/rocm/llvm/bin/clang++ -O1 -std=c++17 $SAN -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -c -o "$OUT/hip_shim.o" "$HERE/hip_shim.cpp"
for prog in gauge_log_host_check cellrp_host_check; do
    /opt/rocm/llvm/bin/clang++ -O1 -std=c++17 $SAN -c -o "$OUT/$prog.o" "$HERE/$prog.cpp"
    $HIPCC --offload-arch=$ARCH $SAN -o "$OUT/$prog" "$OUT/$prog.o" "$OUT/hip_shim.o" "$OUT/pclaw_san.o" \
        "$CSRC/kernels_exact.o" "$CSRC/kernels_fast.o" "$CSRC/kernels_strict.o" -ldl
    ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/$prog"
done
