// Host-visible interface of csrc/hip/bls_kernels.hip: the prototype of every
// K1 (BLS-over-BN254) launcher.  Plain C++, included by csrc/gpu_bindings.cpp
// and by bls_kernels.hip itself, so the compiler checks each C-linkage
// definition against the prototype its caller sees.
//
// Layouts: vks [N][128], sigs [N][64], msgs = flat namespaced messages with
// one spare byte each, moff [N+1] byte offsets into msgs, ok [N].
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

extern "C" {

void launch_k1_bls_verify(const uint8_t* vks, const uint8_t* sigs, uint8_t* msgs,
                          const int64_t* moff, int32_t N, int32_t* ok, hipStream_t s);
void launch_k1_hash_to_g1(uint8_t* msgs, const int64_t* moff, int32_t N, uint8_t* out,
                          hipStream_t s);
void launch_k1_precompute_g2_lines(uint8_t* out, int32_t* n_out, hipStream_t s);
void launch_k1_bls_verify2(const uint8_t* vks, const uint8_t* sigs, uint8_t* msgs,
                           const int64_t* moff, const uint8_t* g2_lines, int32_t N,
                           int32_t* ok, hipStream_t s);
void launch_k1_bls_verify_wave(const uint8_t* vks, const uint8_t* sigs, uint8_t* msgs,
                               const int64_t* moff, const uint8_t* g2_lines,
                               const uint64_t* rand_r, int32_t N, int32_t* ok,
                               hipStream_t s);

}  // extern "C"
