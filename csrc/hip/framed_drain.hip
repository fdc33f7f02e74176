// K11: the framed drain.  Where K7 (dataplane.hip) gathers every ring's used
// prefix as it lies, K11 gathers it as the socket needs it: every record
// {u32 len, u32 seq, u64 pad} + payload becomes a frame
// [u32 big-endian len][payload], frames back to back, in the order
// ring_format.parse_ring_records returns (circular-minimum base, ascending
// (seq - base) mod 2^32, ties in ring order).  The host is left with one
// header walk and one memcpy per recipient.
//
//   k11_ring_index  one workgroup per ring.  Wave 0 walks the record chain
//                   (a dependent walk: it stays wave-uniform), writes one
//                   FrameIdx per record and notes whether the ring is in seq
//                   order.  An out-of-order ring of at most FRAME_SORT_MAX
//                   records is then sorted by the whole workgroup in LDS and
//                   its index rewritten in output order.
//   k11_frame_copy  grid (ring, chunk of the framed output).  A wave copies
//                   one record at a time from the index: the length prefix,
//                   then the body, which lands at an arbitrary byte alignment
//                   from a 16-aligned source.
//
// Both kernels are memory-safe on arbitrary ring bytes: a record whose len
// has the by-reference flag, exceeds the framing limit or does not fit below
// the cursor ends the walk, and the records before it are emitted.  Every
// loop has a bound in its header.
//
// gfx950, wave64.  Built into its own extension (pushcdn_gpu_drain).

#include <hip/hip_runtime.h>

#include "framed_drain.h"

typedef uint32_t k11_v4u __attribute__((ext_vector_type(4)));
typedef uint32_t k11_v2u __attribute__((ext_vector_type(2)));

// The bytes of ring r that the drain looks at, and whether its region lies
// inside the staging buffer.  Both kernels decide these the same way.
__device__ __forceinline__ int64_t k11_used(int64_t w, int64_t ring_bytes) {
    return w < 0 ? 0 : (w > ring_bytes ? ring_bytes : w);
}
__device__ __forceinline__ bool k11_region_ok(int64_t off, int64_t used, int64_t staging_bytes) {
    return off >= 0 && used <= staging_bytes && off <= staging_bytes - used;
}

// Records a thread carries through the sorted rewrite: FRAME_SORT_MAX of them
// over the workgroup.
#define K11_PER_THREAD (FRAME_SORT_MAX / K11_THREADS)
static_assert(K11_PER_THREAD * K11_THREADS == FRAME_SORT_MAX, "FRAME_SORT_MAX per thread");
static_assert((FRAME_SORT_MAX & (FRAME_SORT_MAX - 1)) == 0, "FRAME_SORT_MAX is a power of two");

extern "C" __global__ __launch_bounds__(K11_THREADS) void k11_ring_index(
    const uint8_t* __restrict__ egress, int64_t ring_bytes,
    const int64_t* __restrict__ wpos, const int64_t* __restrict__ dst_off,
    int64_t staging_bytes, int64_t* __restrict__ frame_len, int32_t* __restrict__ frame_cnt,
    FrameIdx* index)
{
    // (seq - base) << 32 | ring order, of the first FRAME_SORT_MAX records
    __shared__ uint64_t s_key[FRAME_SORT_MAX];
    __shared__ uint32_t s_scan[K11_THREADS];
    __shared__ uint32_t s_n, s_flen, s_base, s_ordered;

    const int r = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int64_t used = k11_used(wpos[r], ring_bytes);
    const int64_t off = dst_off[r];
    // block-uniform: nothing to walk, or a region that is not ours to write
    if (used < 16 || !k11_region_ok(off, used, staging_bytes)) {
        if (tid == 0) { frame_len[r] = 0; frame_cnt[r] = 0; }
        return;
    }
    const uint8_t* ring = egress + (int64_t)r * ring_bytes;
    // floor(off / 16) + floor(used / 16) <= floor((off + used) / 16): the
    // entries of neighbouring rings never overlap, aligned cursors or not
    FrameIdx* idx = index + (off >> 4);

    if (tid < 64) {
        const uint32_t U = (uint32_t)used;          // ring_bytes < 2^32
        const uint32_t max_steps = (uint32_t)(ring_bytes >> 4);
        uint32_t pos = 0, n = 0, foff = 0, base = 0, prev = 0, ordered = 1;
        // the window: lane l holds {len, seq} of the 16 B unit at win + 16 l,
        // so a run of small records costs one coalesced load, not one each
        uint32_t win = 0, wl = 0, ws = 0;
        bool have_win = false;
        FrameIdx mine = {0, 0, 0, 0};
        for (uint32_t step = 0; step < max_steps; ++step) {   // >= 16 B a step
            if (U - pos < 16) break;                           // pos <= U always
            if (!have_win || pos - win >= 64 * 16) {
                win = pos;
                have_win = true;
                const uint32_t p = win + (uint32_t)lane * 16;
                wl = ws = 0;
                if (p <= U && U - p >= 16) {
                    const k11_v2u h = *(const k11_v2u*)(ring + p);
                    wl = h.x;
                    ws = h.y;
                }
            }
            const int j = (int)((pos - win) >> 4);
            const uint32_t len = __builtin_amdgcn_readlane(wl, j);
            const uint32_t seq = __builtin_amdgcn_readlane(ws, j);
            if ((len & K11_REF_FLAG) || len > K11_MAX_MESSAGE_SIZE
                || (uint64_t)pos + 16 + len > U)
                break;
            if (n == 0) {
                base = seq;
            } else {
                if ((uint32_t)(seq - prev) > 0x80000000u) ordered = 0;
                if ((uint32_t)(seq - base) > 0x80000000u) base = seq;
            }
            prev = seq;
            if (lane == 0 && n < FRAME_SORT_MAX) s_key[n] = seq;
            if (lane == (int)(n & 63)) mine = FrameIdx{pos, len, seq, foff};
            foff += 4 + len;                                   // <= pos + 16 + len <= U
            ++n;
            if ((n & 63) == 0) idx[n - 64 + lane] = mine;      // 64 entries, coalesced
            pos += 16 + ((len + 15) & ~15u);
        }
        const uint32_t rem = n & 63;
        if ((uint32_t)lane < rem) idx[n - rem + lane] = mine;
        if (lane == 0) { s_n = n; s_flen = foff; s_base = base; s_ordered = ordered; }
    }
    __threadfence_block();
    __syncthreads();

    const uint32_t n = s_n;
    if (n == 0 || s_ordered) {
        if (tid == 0) { frame_len[r] = s_flen; frame_cnt[r] = (int32_t)n; }
        return;
    }
    if (n > FRAME_SORT_MAX) {                                  // ring mode
        if (tid == 0) { frame_len[r] = used; frame_cnt[r] = -1; }
        return;
    }

    // ---- sort (key, ring order) in LDS: bitonic over P >= n slots ----
    uint32_t P = 2;
    for (int b = 1; b < 12 && P < n; ++b) P <<= 1;             // P <= FRAME_SORT_MAX = 2^12
    const uint32_t base = s_base;
    for (uint32_t i = tid; i < P; i += K11_THREADS)
        s_key[i] = i < n ? ((uint64_t)(uint32_t)((uint32_t)s_key[i] - base) << 32) | i : ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1) {                    // P <= FRAME_SORT_MAX
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < (P >> 1); t += K11_THREADS) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const uint32_t l = i | j;
                const uint64_t a = s_key[i], b = s_key[l];
                if ((a > b) == ((i & k) == 0)) { s_key[i] = b; s_key[l] = a; }
            }
            __syncthreads();
        }
    }

    // ---- rewrite the index in sorted order.  Thread t owns output slots
    // [t * K11_PER_THREAD, ...): it gathers their records into registers,
    // and only after every gather is done does anyone overwrite an entry ----
    uint32_t e_pos[K11_PER_THREAD], e_len[K11_PER_THREAD], e_seq[K11_PER_THREAD];
    uint32_t sum = 0;
    const uint32_t first = (uint32_t)tid * K11_PER_THREAD;
#pragma unroll
    for (int k = 0; k < K11_PER_THREAD; ++k) {
        // branch-free (a slot past n re-reads the last one and counts nothing),
        // so the three arrays stay plain registers
        const bool live = first + k < n;
        const FrameIdx x = idx[(uint32_t)s_key[live ? first + k : n - 1]];
        e_pos[k] = x.ring_pos;
        e_len[k] = x.len;
        e_seq[k] = x.seq;
        sum += live ? 4 + x.len : 0;
    }
    s_scan[tid] = sum;
    __syncthreads();
    for (int d = 1; d < K11_THREADS; d <<= 1) {                // inclusive scan, 8 steps
        const uint32_t v = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    uint32_t foff = s_scan[tid] - sum;
#pragma unroll
    for (int k = 0; k < K11_PER_THREAD; ++k) {
        if (first + k < n) {
            idx[first + k] = FrameIdx{e_pos[k], e_len[k], e_seq[k], foff};
            foff += 4 + e_len[k];
        }
    }
    if (tid == 0) { frame_len[r] = s_flen; frame_cnt[r] = (int32_t)n; }
}

// One frame, by one wave.  d is the frame's first byte (any alignment), src
// the record's body (16-aligned, zero-padded to 16 in the ring).  The frame
// is F = 4 + len bytes: bytes [0, H) by byte stores up to the first dword
// boundary at or after the prefix, then aligned dwords each composed from two
// source dwords, then at most 3 tail bytes.  No store covers a byte outside
// [d, d + F): the neighbouring frames share dwords with this one and belong
// to other waves.
__device__ __forceinline__ void k11_copy_frame(const uint8_t* __restrict__ src,
                                               uint8_t* __restrict__ d, uint32_t len, int lane)
{
    const uint32_t F = len + 4;                                // len <= 2^29
    uint32_t H = 4 + ((0u - (uint32_t)(uintptr_t)(d + 4)) & 3u);
    if (H > F) H = F;
    if ((uint32_t)lane < H)
        d[lane] = lane < 4 ? (uint8_t)(len >> (8 * (3 - lane))) : src[lane - 4];
    const uint32_t nmid = (F - H) >> 2;
    const uint32_t sh = H & 3u;                                // (H - 4) mod 4: source skew
    for (uint32_t m = lane; m < nmid; m += 64) {               // passes: len / 256 + 1
        const uint32_t k = H + 4 * m;                          // frame byte of this dword
        const uint32_t sa = (k - 4) & ~3u;                     // k + 4 <= F: source bytes < len
        const uint32_t lo = *(const uint32_t*)(src + sa);
        // sh != 0: sa + 4 <= k - 4 + 3 < len, the dword starts inside the body
        const uint32_t hi = sh ? *(const uint32_t*)(src + sa + 4) : 0u;
        *(uint32_t*)(d + k) = __builtin_amdgcn_alignbyte(hi, lo, sh);
    }
    const uint32_t T = H + 4 * nmid;
    const uint32_t t = (uint32_t)lane - 8u;                    // lanes 8..10
    if (lane >= 8 && t < F - T) d[T + t] = src[T - 4 + t];
}

extern "C" __global__ __launch_bounds__(K11_THREADS) void k11_frame_copy(
    const uint8_t* __restrict__ egress, int64_t ring_bytes,
    const int64_t* __restrict__ wpos, const int64_t* __restrict__ dst_off,
    uint8_t* __restrict__ staging, int64_t staging_bytes,
    const int64_t* __restrict__ frame_len, const int32_t* __restrict__ frame_cnt,
    const FrameIdx* __restrict__ index)
{
    const int r = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t used = k11_used(wpos[r], ring_bytes);
    const int64_t off = dst_off[r];
    if (used < 16 || !k11_region_ok(off, used, staging_bytes)) return;
    const int32_t cnt = frame_cnt[r];
    const int64_t chunk = (int64_t)blockIdx.y * K11_CHUNK;
    const uint8_t* ring = egress + (int64_t)r * ring_bytes;
    uint8_t* dst = staging + off;

    if (cnt < 0) {
        // ring mode: K7's copy of the raw prefix
        if (chunk >= used) return;
        const int64_t end = used < chunk + K11_CHUNK ? used : chunk + K11_CHUNK;
        if (((off | used) & 15) == 0) {
            for (int64_t p = chunk + (int64_t)tid * 16; p < end; p += (int64_t)K11_THREADS * 16)
                *(k11_v4u*)(dst + p) = *(const k11_v4u*)(ring + p);
        } else {
            for (int64_t p = chunk + tid; p < end; p += K11_THREADS) dst[p] = ring[p];
        }
        return;
    }
    if (chunk >= frame_len[r]) return;
    const FrameIdx* idx = index + (off >> 4);
    // first frame that starts in this chunk: frame_off ascends along the index
    uint32_t lo = 0, hi = (uint32_t)cnt;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)idx[mid].frame_off < chunk) lo = mid + 1; else hi = mid;
    }
    const int64_t end = chunk + K11_CHUNK;
    const int lane = tid & 63;
    for (uint32_t e = lo + (uint32_t)(tid >> 6); e < (uint32_t)cnt; e += K11_THREADS / 64) {
        const FrameIdx x = idx[e];
        if ((int64_t)x.frame_off >= end) break;
        k11_copy_frame(ring + x.ring_pos + 16, dst + x.frame_off, x.len, lane);
    }
}

extern "C" void launch_k11_frame_rings(const uint8_t* egress, int64_t ring_bytes,
                                       const int64_t* wpos, const int64_t* dst_off,
                                       uint8_t* staging, int64_t staging_bytes,
                                       int64_t* frame_len, int32_t* frame_cnt, FrameIdx* index,
                                       int32_t n_rings, int32_t max_chunks, hipStream_t s) {
    if (n_rings <= 0) return;
    hipLaunchKernelGGL(k11_ring_index, dim3(n_rings), dim3(K11_THREADS), 0, s, egress,
                       ring_bytes, wpos, dst_off, staging_bytes, frame_len, frame_cnt, index);
    if (max_chunks <= 0) return;
    hipLaunchKernelGGL(k11_frame_copy, dim3(n_rings, max_chunks), dim3(K11_THREADS), 0, s,
                       egress, ring_bytes, wpos, dst_off, staging, staging_bytes, frame_len,
                       frame_cnt, index);
}
