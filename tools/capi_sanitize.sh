#!/bin/bash
# The C boundary under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU: tools/capi_sanitize.sh
#
# csrc/nconv_capi.hip, capi_dense.hip and capi_io.hip are host code only (validation and marshalling, no
# launch, no runtime call), so they are compiled here for the host alone with both sanitizers. Every
# tests/host/*_host.c program is compiled the same way and linked with those objects in front of the
# ordinary libnconv.so: the library supplies the launchers, the executable's own boundary definitions
# take precedence over the library's. Each program must exit 0 without a sanitizer report and print the
# JSON it prints when built the ordinary way (gcc against the library alone, as the tests build it).
# Stand-alone executables that carry their own sanitizer runtime: nothing is preloaded, nothing is
# loaded into Python, no GPU is used. Leak detection is off: the leak checker would report what the HIP
# runtime, loaded with the library, allocates at start-up and keeps.
# Needs a built library (realtime-depth-estimation-nconv_amd/build.py).
set -euo pipefail
root="$(cd "$(dirname "$0")/.." && pwd)"
pkg="$root/realtime-depth-estimation-nconv_amd"
lib="$pkg/libnconv.so"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
CLANG=${CLANG:-/opt/rocm/lib/llvm/bin/clang}
SAN="-fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer"
[ -f "$lib" ] || { echo "no $lib: run build.py first" >&2; exit 2; }
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT

objs=()
for f in nconv_capi capi_dense capi_io; do
  xsan=""
  for flag in $SAN; do xsan="$xsan -Xarch_host $flag"; done
  # shellcheck disable=SC2086
  "$HIPCC" -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 --offload-host-only $xsan -I "$root/include" \
    -c "$pkg/csrc/$f.hip" -o "$tmp/$f.o"
  if nm -u "$tmp/$f.o" | grep -E ' U _?hip[A-Z_]'; then echo "$f.hip calls the HIP runtime" >&2; exit 1; fi
  objs+=("$tmp/$f.o")
done

export ASAN_OPTIONS=detect_leaks=0:abort_on_error=0 UBSAN_OPTIONS=print_stacktrace=1
status=0
for src in "$root"/tests/host/*_host.c; do
  name=$(basename "$src" .c)
  gcc -std=c99 -Wall -Werror -I "$root/include" -I "$pkg/csrc" "$src" -o "$tmp/$name.plain" "$lib" \
    "-Wl,-rpath,$pkg"
  # shellcheck disable=SC2086
  "$CLANG" -std=c99 -O1 -g $SAN -I "$root/include" -I "$pkg/csrc" -c "$src" -o "$tmp/$name.o"
  # shellcheck disable=SC2086
  "$CLANG"++ $SAN "$tmp/$name.o" "${objs[@]}" "$lib" "-Wl,-rpath,$pkg" -o "$tmp/$name.san"
  "$tmp/$name.plain" > "$tmp/$name.plain.json"
  if ! "$tmp/$name.san" > "$tmp/$name.san.json" 2> "$tmp/$name.san.err"; then
    echo "FAIL $name: exit status or sanitizer report"; cat "$tmp/$name.san.err"; status=1
  elif [ -s "$tmp/$name.san.err" ]; then
    echo "FAIL $name: wrote to stderr"; cat "$tmp/$name.san.err"; status=1
  elif ! cmp -s "$tmp/$name.plain.json" "$tmp/$name.san.json"; then
    echo "FAIL $name: JSON differs from the ordinary build's"; diff "$tmp/$name.plain.json" "$tmp/$name.san.json" || true
    status=1
  else
    echo "ok   $name ($(wc -c < "$tmp/$name.san.json") bytes of JSON, identical)"
  fi
done
exit $status
