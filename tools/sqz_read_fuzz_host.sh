#!/bin/bash
# ASan + UBSan build of the device reader's arithmetic (gamut_amd/csrc/sqz_read.hpp) under a serial stand-in for its workgroup
# (tools/sqz_read_fuzz_host.cpp), compared with the SQZ host front end and run on the CPU:
#     tools/sqz_read_fuzz_host.sh [iterations per seed, default 1500]
# The seeds are the files under tests/golden/sqz.  Only host code is instrumented (-Xarch_host); nothing here touches a GPU.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off $SAN -c "$ROOT/gamut_amd/csrc/sqz_host.hip" -o "$OUT/sqz_host.o"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $SAN -x hip -c "$ROOT/tools/sqz_read_fuzz_host.cpp" -o "$OUT/driver.o"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fsanitize=address,undefined "$OUT/sqz_host.o" "$OUT/driver.o" -o "$OUT/sqz_read_fuzz_host"
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$OUT/sqz_read_fuzz_host" "${1:-1500}" "$ROOT"/tests/golden/sqz/*.sqz
rm -rf "$OUT"
