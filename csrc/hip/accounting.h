// Host-visible interface of csrc/hip/accounting.hip: per-recipient loss
// accounting for the egress rings.  Plain C++ — csrc/gpu_acct_bindings.cpp
// (host-only) and accounting.hip both include it, so the compiler checks the
// definition against the prototype its caller sees.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

// Threads of a k9_recipient_demand workgroup: K9_WAVES waves split the
// message range of one mask word.
#define K9_THREADS 1024
#define K9_WAVES (K9_THREADS / 64)

// One entry of k10_loss_scan's compact list: recipient r lost `bytes` ring
// bytes since the previous scan.  Stored as two int64 words.
struct alignas(16) LossRec { int64_t recipient; int64_t bytes; };
static_assert(sizeof(LossRec) == 16, "LossRec must be one dword4");

extern "C" {

// K9: demand[r] += the ring bytes this tick wants to deliver to r.
// mask_t is [W][M] (origin clearing applied), ring_len [M] what K2b / K5b
// claim ring space from.  owner == nullptr: the tick routes no Directs.
// origin == nullptr: every message is local-origin.  demand has
// n_users + n_peers <= W * 64 elements.  One launch; M <= 0 launches nothing.
void launch_k9_recipient_demand(const uint64_t* mask_t, const int32_t* ring_len,
                                const int32_t* disc, const int32_t* owner,
                                const int32_t* origin, int32_t M, int32_t W, int32_t n_users,
                                int32_t n_peers, uint64_t* demand, hipStream_t s);

// K10: for every r < R with demand[r] != ring_wpos[r], append
// {r, demand[r] - ring_wpos[r]} to lossy (capacity R, order unspecified) and
// count it in n_lossy[0], which is zeroed first; demand is zeroed, ring_wpos
// only read.  Two stream operations: the zeroing, whose status is returned,
// and one launch.
hipError_t launch_k10_loss_scan(uint64_t* demand, const int64_t* ring_wpos, LossRec* lossy,
                                int32_t* n_lossy, int32_t R, hipStream_t s);

}  // extern "C"
