#!/bin/bash
# ASan+UBSan lane for the native host core (the C++ rewrite
# replaces Rust's compile-time safety with sanitizer lanes).
set -e
cd "$(dirname "$0")/.."
mkdir -p build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer \
    -I csrc csrc/tests/test_native.cpp -o build/test_native_asan -lpthread
./build/test_native_asan
# TSan lane: the pump runs a live epoll thread — race-check it
g++ -O1 -g -std=c++17 -fsanitize=thread -fno-omit-frame-pointer \
    -I csrc csrc/tests/test_native.cpp -o build/test_native_tsan -lpthread
# On kernels with high mmap ASLR entropy (vm.mmap_rnd_bits > 28) the TSan
# runtime aborts at startup, before main(), with "unexpected memory mapping":
# rerun it then with ASLR off for this one process.
rc=0
./build/test_native_tsan 2> build/test_native_tsan.err || rc=$?
cat build/test_native_tsan.err >&2
if [ $rc -ne 0 ]; then
    grep -q "unexpected memory mapping" build/test_native_tsan.err
    setarch "$(uname -m)" -R ./build/test_native_tsan
fi
echo "sanitizer lane OK"
