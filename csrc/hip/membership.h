// Host-visible interface of csrc/hip/membership.hip: device-state
// maintenance kernels that run between ticks, kept apart from the tick
// kernels of dataplane.hip.  Plain C++ — csrc/gpu_ctl_bindings.cpp
// (host-only) and membership.hip both include it, so the compiler checks the
// definition against the prototype its caller sees.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

// One membership row is MEMBERSHIP_WORDS int64 words:
//   [0]     recipient index r (a user slot, or n_users + p for peer slot p)
//   [1]     flags; bit 0 = reset the recipient's ring cursor to 0
//   [2..5]  clear: 256-bit topic set, topic t = bit (t & 63) of word 2 + (t >> 6)
//   [6..9]  set:   the same layout
#define MEMBERSHIP_WORDS 10
#define MEMBERSHIP_RESET 1

// Grid cap of k8_membership_apply; rows beyond it are taken by the
// grid-stride loop.
#define K8_MAX_BLOCKS 1024

extern "C" {

// K8: apply n coalesced membership rows to sub_bitmap [256][W] and
// ring_wpos [R].  n <= 0 launches nothing.
void launch_k8_membership_apply(uint64_t* sub_bitmap, int64_t* ring_wpos, const int64_t* recs,
                                int32_t n, int32_t W, int32_t R, hipStream_t s);

}  // extern "C"
