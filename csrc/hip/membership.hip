// Device-state maintenance kernels for the MI355X broker (gfx950): what
// changes the HBM-resident routing state between ticks, as opposed to the
// tick kernels of dataplane.hip that read it.
//
//   K8  k8_membership_apply — one launch applies a batch of coalesced
//       per-recipient membership rows (joins, leaves, subscription changes)
//       to the subscription bitmap and the ring cursors.

#include <hip/hip_runtime.h>

#include "membership.h"

// ---------------------------------------------------------------------------
// K8: membership rows -> sub_bitmap bits + ring cursor resets.
//
// One 256-thread block per row, thread t owns topic t.  For its topic the
// thread makes bit r of sub_bitmap[t][r >> 6] 1 if the row's `set` has t, 0 if
// only `clear` has t, and leaves it alone otherwise ("set wins").  The four
// waves of a block cover the four 64-topic words of `clear` / `set`, so each
// wave reads ONE clear word and ONE set word: the word index goes through
// readfirstlane, which makes the loads wave-uniform.
//
// Up to 64 rows of one launch share a bitmap word (64 recipients per word),
// so the bit changes are 64-bit atomics; their results are not used, which
// lets the compiler pick the no-return form.  A thread whose topic is in
// neither set issues nothing.  Contract: a recipient appears in at most one
// row of a launch (the host coalesces), so each (recipient, topic) bit is
// touched at most once and the result does not depend on arrival order.
//
// A row whose r is outside [0, R) is skipped whole (block-uniform branch):
// no bitmap word and no cursor is touched for it.  R <= W * 64 is checked by
// the binding, so r >> 6 < W for every row that passes.
//
// Grid: min(n, K8_MAX_BLOCKS) blocks with a grid-stride loop over rows.
// 1024 blocks x 4 waves is four waves per SIMD on all 256 CUs, enough
// outstanding atomics to cover their latency; a larger grid only adds
// launch work for a kernel that moves 80 B + at most 256 atomics per row.
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256) void k8_membership_apply(
    uint64_t* __restrict__ sub_bitmap,   // [256][W]
    int64_t* __restrict__ ring_wpos,     // [R]
    const int64_t* __restrict__ recs,    // [n][MEMBERSHIP_WORDS]
    int32_t n, int32_t W, int32_t R)
{
    const int t = threadIdx.x;                                 // topic
    const int k = __builtin_amdgcn_readfirstlane(t >> 6);      // wave = topic word
    const uint64_t tbit = 1ull << (t & 63);
    for (int32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int64_t* row = recs + (int64_t)i * MEMBERSHIP_WORDS;
        const int64_t r = row[0];
        if (r < 0 || r >= (int64_t)R) continue;
        const uint64_t clr = (uint64_t)row[2 + k];
        const uint64_t set = (uint64_t)row[6 + k];
        unsigned long long* word =
            (unsigned long long*)(sub_bitmap + (int64_t)t * W + (r >> 6));
        const unsigned long long rbit = 1ull << (r & 63);
        if (set & tbit)
            atomicOr(word, rbit);
        else if (clr & tbit)
            atomicAnd(word, ~rbit);
        if (t == 0 && (row[1] & MEMBERSHIP_RESET)) ring_wpos[r] = 0;
    }
}

extern "C" {

void launch_k8_membership_apply(uint64_t* sub_bitmap, int64_t* ring_wpos, const int64_t* recs,
                                int32_t n, int32_t W, int32_t R, hipStream_t s) {
    if (n <= 0) return;
    const int blocks = n < K8_MAX_BLOCKS ? n : K8_MAX_BLOCKS;
    hipLaunchKernelGGL(k8_membership_apply, dim3(blocks), dim3(256), 0, s, sub_bitmap, ring_wpos,
                       recs, n, W, R);
}

}  // extern "C"
