// Per-recipient loss accounting for the MI355X broker's egress rings (gfx950).
//
// A delivery that does not fit its recipient's ring, or that finds the pair
// list full, is dropped by the tick kernels of dataplane.hip, and nothing they
// leave behind says WHO lost it.  These two kernels find out without touching
// them: between two drains ring_wpos[r] is exactly the ring bytes delivered to
// r, so a second accumulator with the bytes the ticks WANTED to deliver to r
// differs from it exactly by the bytes r lost.
//
//   K9   k9_recipient_demand — once per tick: demand[r] += ring_rec(ring_len[m])
//        over the tick's messages that address r (Broadcasts through the
//        transposed mask, Directs through K5's owner).
//   K10  k10_loss_scan — once per drain, before the cursors are reset:
//        compact list of (r, demand[r] - ring_wpos[r]) over the recipients
//        where the two differ; demand is zeroed.

#include <hip/hip_runtime.h>

#include "accounting.h"

// Egress ring record stride; the definition of dataplane.hip's ring_rec.
__device__ __forceinline__ uint64_t acct_ring_rec(int32_t len) {
    return ((uint64_t)len + 16 + 15) & ~15ull;
}

// ---------------------------------------------------------------------------
// K9: one launch, two kinds of workgroup.
//
// Workgroups [0, W) — Broadcasts.  Workgroup w owns mask word w: lane l of
// every wave is recipient w * 64 + l, and the K9_WAVES waves take contiguous
// slices of the message range.  mask_t[w * M + m] and ring_len[m] depend only
// on blockIdx, the wave index (made uniform with readfirstlane) and the loop
// counter, so both loads are wave-uniform scalar loads and the record stride
// is scalar arithmetic; a lane's own work is one bit test and one 64-bit add.
// The waves' partial sums meet in LDS (8 KiB), wave 0 adds them up and one
// atomic per recipient with a non-zero sum reaches `demand`.  The add is
// atomic because the Direct workgroups of the same launch add to the same
// words.
//
// Workgroups [W, W + ceil(M / K9_THREADS)) — Directs, one thread per message.
// The recipient is resolved exactly as k5b_emit_direct_peers resolves it:
// disc == 3; 0 <= owner < n_users is that user; owner <= -2 is peer slot
// p = -owner - 2, which counts only if p < n_peers and the message is
// local-origin, and is recipient n_users + p.  Not-found (INT32_MIN), -1,
// owners >= n_users and remote-origin peer Directs demand nothing.
//
// Bounds: mask_t holds W * M words and demand n_users + n_peers <= W * 64
// (checked by the binding); a broadcast lane is guarded with u < R, a Direct
// recipient is below R by construction.
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(K9_THREADS) void k9_recipient_demand(
    const uint64_t* __restrict__ mask_t,     // [W][M]
    const int32_t* __restrict__ ring_len,    // [M]
    const int32_t* __restrict__ disc,        // [M]
    const int32_t* __restrict__ owner,       // [M] K5 output, or nullptr
    const int32_t* __restrict__ origin,      // [M] 0 = local, or nullptr = all local
    int32_t M, int32_t W, int32_t n_users, int32_t n_peers,
    uint64_t* __restrict__ demand)           // [n_users + n_peers]
{
    __shared__ uint64_t part[K9_WAVES][64];

    if ((int32_t)blockIdx.x >= W) {
        const int64_t i = (int64_t)(blockIdx.x - W) * K9_THREADS + threadIdx.x;
        if (i >= M || disc[i] != 3) return;
        const int32_t o = owner[i];
        int32_t u;
        if (o >= 0) {
            if (o >= n_users) return;
            u = o;
        } else {
            // o <= -2 -> p >= 0; o == -1 -> p == -1; INT32_MIN -> p == 2^31 - 2
            const int64_t p = -(int64_t)o - 2;
            if (p < 0 || p >= (int64_t)n_peers) return;
            if (origin != nullptr && origin[i] != 0) return;
            u = n_users + (int32_t)p;
        }
        atomicAdd((unsigned long long*)(demand + u),
                  (unsigned long long)acct_ring_rec(ring_len[i]));
        return;
    }

    const int32_t w = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int32_t per = (M + K9_WAVES - 1) / K9_WAVES;
    const int32_t m0 = wave * per;
    const int32_t m1 = min(M, m0 + per);
    const uint64_t* __restrict__ col = mask_t + (int64_t)w * M;
    uint64_t acc = 0;
#pragma unroll 4
    for (int32_t m = m0; m < m1; ++m) {
        const uint64_t word = col[m];
        const uint64_t rec = acct_ring_rec(ring_len[m]);
        acc += ((word >> lane) & 1ull) ? rec : 0ull;
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave != 0) return;
    uint64_t sum = 0;
#pragma unroll
    for (int v = 0; v < K9_WAVES; ++v) sum += part[v][lane];
    const int32_t u = w * 64 + lane;
    if (u < n_users + n_peers && sum != 0)
        atomicAdd((unsigned long long*)(demand + u), (unsigned long long)sum);
}

// ---------------------------------------------------------------------------
// K10: one thread per recipient.  d = demand[r] - ring_wpos[r] is the bytes r
// lost since the last scan (u64 arithmetic; demand >= cursor whenever both
// were reset together).  Lossy lanes of a wave claim consecutive list slots:
// ballot + popcount give the wave's count and each lane's rank, lane 0 takes
// the base with ONE atomic on n_lossy and broadcasts it.  At most R entries
// are ever claimed, which is the list's capacity.  No thread leaves before the
// ballot, so every lane of every wave takes part in it.
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256) void k10_loss_scan(
    uint64_t* __restrict__ demand,           // [R], zeroed
    const int64_t* __restrict__ ring_wpos,   // [R], read only
    LossRec* __restrict__ lossy,             // [R]
    int32_t* __restrict__ n_lossy,           // [1], zeroed by the launcher
    int32_t R)
{
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint64_t d = 0;
    if (r < R) {
        const uint64_t dem = demand[r];
        d = dem - (uint64_t)ring_wpos[r];
        if (dem != 0) demand[r] = 0;
    }
    const unsigned long long lost = __ballot(d != 0);
    if (lost == 0) return;   // wave-uniform
    int32_t base = 0;
    if (lane == 0) base = atomicAdd(n_lossy, (int32_t)__popcll(lost));
    base = __shfl(base, 0);
    if (d != 0) {
        const int32_t slot = base + (int32_t)__popcll(lost & ((1ull << lane) - 1ull));
        lossy[slot] = LossRec{(int64_t)r, (int64_t)d};
    }
}

extern "C" {

void launch_k9_recipient_demand(const uint64_t* mask_t, const int32_t* ring_len,
                                const int32_t* disc, const int32_t* owner,
                                const int32_t* origin, int32_t M, int32_t W, int32_t n_users,
                                int32_t n_peers, uint64_t* demand, hipStream_t s) {
    if (M <= 0 || W <= 0) return;
    const int direct_blocks = owner != nullptr ? (M + K9_THREADS - 1) / K9_THREADS : 0;
    hipLaunchKernelGGL(k9_recipient_demand, dim3(W + direct_blocks), dim3(K9_THREADS), 0, s,
                       mask_t, ring_len, disc, owner, origin, M, W, n_users, n_peers, demand);
}

hipError_t launch_k10_loss_scan(uint64_t* demand, const int64_t* ring_wpos, LossRec* lossy,
                                int32_t* n_lossy, int32_t R, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(n_lossy, 0, sizeof(int32_t), s);
    if (e != hipSuccess || R <= 0) return e;
    hipLaunchKernelGGL(k10_loss_scan, dim3((R + 255) / 256), dim3(256), 0, s, demand, ring_wpos,
                       lossy, n_lossy, R);
    return hipSuccess;
}

}  // extern "C"
