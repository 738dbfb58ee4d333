#!/bin/bash
# ThreadSanitizer and AddressSanitizer runs of the collector's host-side cast pool (csrc/host_step.h: persistent worker threads,
# spin / sleep / wake, static partition with claim flags, the pool-owned job slot and its open / busy handshake, AVX-512 and scalar
# casts) through tools/host/cast_pool_check.cpp, each also with -DV4L_CAST_POOL_TEST_STALL (workers register late on purpose).
# Host code only — GPU sanitizers are not available on this pool. usage (repo root): tools/host_step_sanitize.sh [out.txt]
set -u
OUT=${1:-/dev/stdout}
CXX=${CXX:-/opt/rocm/lib/llvm/bin/clang++}
{
  echo "# tools/host_step_sanitize.sh: $CXX -fsanitize={thread,address} of tools/host/cast_pool_check.cpp (includes csrc/host_step.h)"
  for san in thread "address -fsanitize-address-use-after-return=always"; do
    for stall in "" -DV4L_CAST_POOL_TEST_STALL; do
      $CXX -std=c++17 -O1 -g -fsanitize=$san $stall -fno-omit-frame-pointer -pthread tools/host/cast_pool_check.cpp -o /tmp/cast_check_san || exit 1
      echo "== -fsanitize=$san $stall"
      timeout 1200 /tmp/cast_check_san 240 2>&1 | tail -20
      echo "exit code: ${PIPESTATUS[0]}"
    done
  done
} > "$OUT"
