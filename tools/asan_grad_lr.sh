#!/bin/bash
# Host-side AddressSanitizer + UndefinedBehaviorSanitizer build of the C-ABI library and the stand-alone
# program tests/asan/asan_grad_lr.cpp, which drives the argument checks of xt_grad_jk2_lr (and the name
# xt_grad_jk2 keeps in the checks they share).  As tools/asan_host.sh: the device code is compiled as
# usual, only the host half is instrumented (each -fsanitize= right after -Xarch_host), and no GPU is
# needed -- every call in the program is refused, or returns, before the first HIP call.  The program has
# its own main; nothing is loaded into Python.  Run from the repo root:  tools/asan_grad_lr.sh
set -euo pipefail
OUT=tools/bin/asan_ub
mkdir -p "$OUT"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN=(-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined)
FLAGS=(--offload-arch=gfx950 -O1 -g -fPIC -std=c++17 -Wno-unused-result "${SAN[@]}" -Xarch_host -fno-omit-frame-pointer)
objs=()
pids=()
rm -f "$OUT"/*.o        # never link a stale object left by an earlier run
for f in xtddft_amd/csrc/*.hip; do
  o="$OUT/$(basename "${f%.hip}").o"
  "$HIPCC" "${FLAGS[@]}" -c "$f" -o "$o" &
  pids+=($!)
  objs+=("$o")
done
for p in "${pids[@]}"; do wait "$p" || { echo "sanitizer compile failed"; exit 1; }; done
echo 'const char* xt_build_id(void) { return "asan-ubsan-host-build"; }' > "$OUT/xt_build_id.c"
gcc -O1 -fPIC -c "$OUT/xt_build_id.c" -o "$OUT/xt_build_id.o"
objs+=("$OUT/xt_build_id.o")
"$HIPCC" --offload-arch=gfx950 -shared -fPIC "${SAN[@]}" -o "$OUT/libxtddft_amd_asan.so" "${objs[@]}"
/opt/rocm/lib/llvm/bin/clang++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-gpu-sanitize \
  -Wno-unused-command-line-argument -fno-omit-frame-pointer tests/asan/asan_grad_lr.cpp \
  -L"$OUT" -lxtddft_amd_asan -Wl,-rpath,"$(pwd)/$OUT" -o "$OUT/asan_grad_lr"
ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/asan_grad_lr"
