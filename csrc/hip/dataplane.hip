// MI355X (gfx950) data-plane kernels for the GPU broker.
//
// These implement the per-message hot path of the reference broker
// (cdn-broker/src/tasks/user/handler.rs:95-163 + broker/handler.rs:197-272)
// as batched CDNA4 kernels over HBM-resident tables:
//
//   K4  k4_parse_batch — on-device Cap'n Proto validation/field extraction
//                        (reference cdn-proto/src/message.rs:212-312)
//   K2a k2a_topic_mask[_t] — per-message OR of subscription-bitmap topic
//                        rows (reference connections/mod.rs:94-124);
//                        the _t variant writes the mask TRANSPOSED [W][M]
//                        so K2b scans contiguous memory
//   K2b k2b_p1_count / k2b_p2_bases / k2b_p3_emit — the production emit
//                        for uniform records: per-(user, 32-msg block)
//                        counts, then per-user closed-form ring math with
//                        wave-aggregated span claims (one atomic per
//                        wave64), then block-parallel emission — fills the
//                        chip at any population (one-lane-per-user runs
//                        only W waves).  k2b_fused_t is the one-kernel
//                        variant (non-uniform records + golden tests);
//                        k2b_count/k2b_emit the two-pass reference pair.
//                        All preserve the per-connection FIFO the
//                        reference gets from its per-conn channel actors
//                        (protocols/mod.rs:139-217).
//   K3  k3_fanout_flat_t — the production fan-out for uniform records
//                        (unit-per-lane flat index, ~100% lane utilization,
//                        non-temporal 16 B stores; seq from value or device
//                        counter for hipGraph capture); k3_fanout_wave_t is
//                        the general mixed-size path (one wave per pair,
//                        best for records >= 4 KiB); k3_fanout is the plain
//                        reference variant for golden tests. All mirror the
//                        reference's raw-bytes Arc-clone push
//                        (user/sender.rs:16-33).
//   K3r k3_fanout_ref_t — the mixed-size fan-out with by-reference records:
//                        a message at or above ref_threshold is delivered
//                        as a bare 16 B header that points into the host's
//                        copy of the batch (up to 64 pairs per wave)
//   K5  k5_direct_lookup — open-addressing probe user-hash -> owner
//                        (reference connections/mod.rs:69-71 DirectMap get)
//   K5b k5b_emit_direct — on-device direct-delivery pair emission (appends
//                        to the same pair list; no host sync)
//   K2c k2c_apply_subs — ordered subscription updates
//   K2a k2a_topic_mask_origin_t / K5b k5b_emit_direct_peers — the same two
//                        steps with peer-broker recipient slots and a
//                        per-message origin (single-hop broker plane)
//   K6  k6_direct_apply — batched DirectMap upserts/deletes (CAS insert,
//                        tombstoned values)
//   K7  k7_compact_rings — gather used ring prefixes into one staging buffer
//   fused uniform broadcast tick (launch_tick_uniform_broadcast, end of this
//                        file) — the broadcast-only uniform shape as one
//                        launcher call of three launches: k_tick_prologue (K4,
//                        the dense fan-out's record image, counters zeroed),
//                        k_route_word (K2a, P1, P2 plus a dense / sparse sort
//                        of the (user, block) tiles, and pairs for the sparse
//                        tiles only, one mask word per workgroup, in LDS) and
//                        k3_fanout_dense_tail_t (dense tiles stored from
//                        registers, no pair records, and behind them the flat
//                        K3 over the sparse list).  Above ROUTE_MAX_M messages
//                        k2a_topic_mask_t, k2b_p1_count_z, k2b_p2_tiles and
//                        k2b_p3_sparse route through scratch.
//                        k_drain_cursors is the fused drain
//
// Shared device building blocks, each defined once and force-inlined:
//   store16<NT>        the only place the non-temporal store choice is made
//   store_pair         one dword4 store of a PairRec
//   copy_record<NT>    record header + aligned/unaligned 16 B loop + byte
//                      tail over (lane, lane count) — k3_fanout, _wave_t, _ref_t
//   topic_row_or       OR of a message's topic rows for one mask word — the
//                      three K2a kernels
//   wave_claim_span    wave64 inclusive scan + one atomicAdd per wave —
//                      k2b_fused_t, k2b_p2_bases
//   k4_parse_body      one message's parse — k4_parse_batch, k_tick_prologue
//   k3d_image_body     one unit of the record image — k_tick_prologue
//   k3_flat_body       one workgroup of the flat fan-out — k3_fanout_flat_t,
//                      k3_fanout_dense_tail_t
//   k2b_tile_count, k2b_p2_body, k2b_tiles_body, k2b_p3_sparse_body
//                      P1, P2, the tile sort and P3 over tiles in scratch or
//                      in LDS — the k2b_p* kernels and k_route_word
//   k5b_claim_emit     pair-slot claim, CAS ring claim, placeholder and drop
//                      — both K5b kernels
// The launcher prototypes and the PairRec / ParseOut structs are in
// dataplane.h, shared with the host-only bindings.
//
// Design notes (per /opt/skills/guides/cdna_hip_programming.md):
//  - wave = 64; all copies are uint4 (16 B/lane) vectorized
//  - K3 uses a grid-stride loop over delivery pairs with >> 256 workgroups so
//    all 8 XCDs fill; the payload source is usually L2/LLC-hit after the
//    first recipient of a message on that XCD
//  - no cross-workgroup hand-off inside a launch: every kernel's outputs are
//    consumed by the *next* launch on the stream (boundary ≈1.5 us), so no
//    agent-scope fencing is needed
//  - tables are torch tensors: PyTorch owns the HBM, kernels are raw HIP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/divmagic.h"
#include "dataplane.h"

#define WAVE 64
#ifndef CDN_CHECK
#define CDN_CHECK 1
#endif

// Egress ring record stride: 16 B header + payload padded to 16 B, so every
// record start stays uint4-aligned.  Pairs are emitted grouped by user with
// messages in order, so a user's records are back-to-back in the ring and
// the flat K3 writes them as one contiguous streaming range (full-stride,
// zero-padded tail) — 64 B alignment was MEASURED SLOWER (261k vs 285k
// msgs/s headline: +8.6% stored bytes buys no RMW savings).  Host mirrors:
// pushcdn_amd/broker/gpu_engine.py ring_rec / ops/reference.py.
#define RING_ALIGN 16ull
__host__ __device__ inline uint64_t ring_rec(int32_t len) {
    return ((uint64_t)len + 16 + (RING_ALIGN - 1)) & ~(RING_ALIGN - 1);
}

// One 16-byte (dword4) store to a 16-aligned address.  NT=1 is non-temporal:
// egress bytes are written once and consumed by the D2H drain, so they should
// not evict the hot message source bytes from the per-XCD L2.
typedef unsigned int cdn_v4u __attribute__((ext_vector_type(4)));
template <int NT>
__device__ __forceinline__ void store16(void* dst, cdn_v4u v) {
    if (NT) __builtin_nontemporal_store(v, (cdn_v4u*)dst);
    else *(cdn_v4u*)dst = v;
}

// A delivery pair (PairRec, dataplane.h) is stored as ONE dword4.
__device__ __forceinline__ void store_pair(PairRec* p, int32_t u, int32_t m, int64_t d) {
    PairRec r{u, m, d};
    cdn_v4u v; memcpy(&v, &r, 16);
    store16<0>(p, v);
}

// ---------------------------------------------------------------------------
// 64-bit FNV-1a — the routing hash for user public keys. Host mirror in
// pushcdn_amd/utils/keyhash.py must match bit-for-bit.
// `seed` XORs into the offset basis: brokers derive it from the cluster
// private key, so an attacker cannot grind out hash collisions offline
// (FNV alone is byte-invertible). seed=0 == classic FNV-1a.
// ---------------------------------------------------------------------------
__host__ __device__ inline uint64_t fnv1a64(const uint8_t* data, uint32_t len,
                                            uint64_t seed = 0) {
    uint64_t h = 0xcbf29ce484222325ull ^ seed;
    for (uint32_t i = 0; i < len; ++i) {
        h ^= (uint64_t)data[i];
        h *= 0x100000001b3ull;
    }
    return h;
}

// ---------------------------------------------------------------------------
// K4: parse a batch of concatenated serialized Messages (capnp stream format,
// single segment each). One thread per message: the pointer graph is 3-5
// words deep, so a thread walks it; payload bytes are never touched here.
//
// Outputs (all int32/int64 tensors, -1/0 on invalid):
//   disc[i]         discriminant 0..8, or -1 if malformed
//   payload_off/len payload ("message" field / sync Data / topic list) byte
//                   range within the batch buffer
//   topics_off/cnt  topic list byte range (Broadcast/Subscribe/Unsubscribe)
//   recip_hash      fnv1a64 of the recipient key (Direct), else 0
//   timestamp       AuthenticateWithKey.timestamp, else 0
// (struct ParseOut, dataplane.h)
// ---------------------------------------------------------------------------

__device__ inline uint64_t ld_u64(const uint8_t* p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}

// Decode a struct pointer at word `pw` (relative to segment base `seg` of
// `nwords`). Returns false if malformed. Out: target word, data words, ptr words.
__device__ inline bool read_struct_ptr(const uint8_t* seg, int64_t nwords, int64_t pw,
                                       int64_t* tgt, int32_t* dw, int32_t* ptrw) {
    if (pw < 0 || pw >= nwords) return false;
    uint64_t v = ld_u64(seg + pw * 8);
    if (v == 0 || (v & 3) != 0) return false;
    int64_t b = (v >> 2) & 0x3fffffff;
    if (b & 0x20000000) b -= 0x40000000;
    int32_t d = (v >> 32) & 0xffff;
    int32_t p = (v >> 48) & 0xffff;
    int64_t t = pw + 1 + b;
    if (t < 0 || t + d + p > nwords) return false;
    *tgt = t; *dw = d; *ptrw = p;
    return true;
}

// Decode a byte-list pointer (Data / Text / List(UInt8), element code 2).
__device__ inline bool read_byte_list(const uint8_t* seg, int64_t nwords, int64_t pw,
                                      int64_t* off, int32_t* len) {
    if (pw < 0 || pw >= nwords) return false;
    uint64_t v = ld_u64(seg + pw * 8);
    if (v == 0) { *off = pw; *len = 0; return true; }  // null ptr -> empty
    if ((v & 3) != 1) return false;
    int64_t b = (v >> 2) & 0x3fffffff;
    if (b & 0x20000000) b -= 0x40000000;
    uint32_t code = (v >> 32) & 7;
    int64_t count = (v >> 35) & 0x1fffffff;
    if (code != 2) return false;
    int64_t t = pw + 1 + b;
    if (t < 0 || t * 8 + count > nwords * 8) return false;
    *off = t * 8;
    *len = (int32_t)count;
    return true;
}

// Message i of the batch; shared by k4_parse_batch and the fused tick's
// prologue (k_tick_prologue).
__device__ __forceinline__ void k4_parse_body(
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ offsets,  // [M+1] byte offsets into buf
    int32_t M, uint64_t hash_seed, const ParseOut& out, int i)
{
    if (i >= M) return;
    // defaults; field values are buffered in locals and committed only
    // once the whole frame validates, so rejected records are all-zero
    // (bit-identical to the host mirror, proto/message.py parse_offsets)
    out.disc[i] = -1;
    out.payload_off[i] = 0; out.payload_len[i] = 0;
    out.topics_off[i] = 0;  out.topics_cnt[i] = 0;
    out.recip_hash[i] = 0;  out.timestamp[i] = 0;
    int64_t o_poff = 0, o_toff = 0, o_ts = 0;
    uint64_t o_rhash = 0;
    int32_t o_plen = 0, o_tcnt = 0;

    int64_t beg = offsets[i], end = offsets[i + 1];
    if (end - beg < 8 + 8) return;  // header + root ptr
    const uint8_t* p = buf + beg;
    uint32_t seg_m1, nw;
    memcpy(&seg_m1, p, 4); memcpy(&nw, p + 4, 4);
    if (seg_m1 != 0) return;
    if (8 + (int64_t)nw * 8 > end - beg) return;
    const uint8_t* seg = p + 8;
    int64_t nwords = nw;

    int64_t mt; int32_t mdw, mpw;
    if (!read_struct_ptr(seg, nwords, 0, &mt, &mdw, &mpw)) return;
    if (mdw < 1 || mpw < 1) return;
    uint16_t disc;
    memcpy(&disc, seg + mt * 8, 2);
    int64_t up = mt + mdw;  // union pointer word

    int64_t seg_base = (seg - buf);  // byte offset of segment within buf

    switch (disc) {
    case 0: {  // AuthenticateWithKey
        int64_t it; int32_t idw, ipw;
        if (!read_struct_ptr(seg, nwords, up, &it, &idw, &ipw)) return;
        if (idw < 1 || ipw < 2) return;
        o_ts = (int64_t)ld_u64(seg + it * 8);
        int64_t ko; int32_t kl;
        if (!read_byte_list(seg, nwords, it + idw, &ko, &kl)) return;
        o_poff = kl ? seg_base + ko : 0;  // public key bytes
        o_plen = kl;
        int64_t so; int32_t sl;
        if (!read_byte_list(seg, nwords, it + idw + 1, &so, &sl)) return;
        o_toff = sl ? seg_base + so : 0;   // signature bytes (reused slot)
        o_tcnt = sl;
        break;
    }
    case 1: {  // AuthenticateWithPermit
        int64_t it; int32_t idw, ipw;
        if (!read_struct_ptr(seg, nwords, up, &it, &idw, &ipw)) return;
        if (idw < 1) return;
        o_ts = (int64_t)ld_u64(seg + it * 8);  // permit
        break;
    }
    case 2: {  // AuthenticateResponse
        int64_t it; int32_t idw, ipw;
        if (!read_struct_ptr(seg, nwords, up, &it, &idw, &ipw)) return;
        if (idw < 1 || ipw < 1) return;
        o_ts = (int64_t)ld_u64(seg + it * 8);  // permit
        int64_t co; int32_t cl;
        if (!read_byte_list(seg, nwords, it + idw, &co, &cl)) return;
        o_poff = cl ? seg_base + co : 0; o_plen = cl;
        break;
    }
    case 3: {  // Direct
        int64_t it; int32_t idw, ipw;
        if (!read_struct_ptr(seg, nwords, up, &it, &idw, &ipw)) return;
        if (ipw < 2) return;
        int64_t ro; int32_t rl;
        if (!read_byte_list(seg, nwords, it + idw, &ro, &rl)) return;
        o_rhash = fnv1a64(seg + ro, rl, hash_seed);
        int64_t mo; int32_t ml;
        if (!read_byte_list(seg, nwords, it + idw + 1, &mo, &ml)) return;
        o_poff = ml ? seg_base + mo : 0; o_plen = ml;
        break;
    }
    case 4: {  // Broadcast
        int64_t it; int32_t idw, ipw;
        if (!read_struct_ptr(seg, nwords, up, &it, &idw, &ipw)) return;
        if (ipw < 2) return;
        int64_t to; int32_t tc;
        if (!read_byte_list(seg, nwords, it + idw, &to, &tc)) return;
        o_toff = tc ? seg_base + to : 0; o_tcnt = tc;
        int64_t mo; int32_t ml;
        if (!read_byte_list(seg, nwords, it + idw + 1, &mo, &ml)) return;
        o_poff = ml ? seg_base + mo : 0; o_plen = ml;
        break;
    }
    case 5: case 6: {  // Subscribe / Unsubscribe
        int64_t to; int32_t tc;
        if (!read_byte_list(seg, nwords, up, &to, &tc)) return;
        o_toff = tc ? seg_base + to : 0; o_tcnt = tc;
        break;
    }
    case 7: case 8: {  // UserSync / TopicSync
        int64_t dof; int32_t dl;
        if (!read_byte_list(seg, nwords, up, &dof, &dl)) return;
        o_poff = dl ? seg_base + dof : 0; o_plen = dl;
        break;
    }
    default:
        return;
    }
    out.payload_off[i] = o_poff; out.payload_len[i] = o_plen;
    out.topics_off[i] = o_toff;  out.topics_cnt[i] = o_tcnt;
    out.recip_hash[i] = (int64_t)o_rhash; out.timestamp[i] = o_ts;
    out.disc[i] = (int32_t)disc;
}

extern "C" __global__ void k4_parse_batch(
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ offsets,  // [M+1] byte offsets into buf
    int32_t M, uint64_t hash_seed, ParseOut out)
{
    k4_parse_body(buf, offsets, M, hash_seed, out, blockIdx.x * blockDim.x + threadIdx.x);
}

// ---------------------------------------------------------------------------
// K2a: per-message recipient mask.
//   sub_bitmap: [256][W] uint64 — bit u of word w set iff user (w*64+u)
//               subscribes to the topic
//   mask:       [M][W] uint64 out — OR of the message's topic rows
// Grid: one thread per (message, word): M*W threads. Broadcast-only messages
// (disc==4) produce a mask; everything else produces zeros.
// exclude_user: for no-echo semantics the caller can exclude the sender
// (reference tests: no echo to the originating connection is NOT default —
// the reference DOES echo to the sender if subscribed; keep -1 to disable).
// ---------------------------------------------------------------------------

// Bits of mask word w that belong to local users (recipients < n_users).
__device__ __forceinline__ uint64_t user_bits_of_word(int32_t w, int32_t n_users) {
    const int64_t lo = (int64_t)w * 64;
    if ((int64_t)n_users >= lo + 64) return ~0ull;
    if ((int64_t)n_users <= lo) return 0ull;
    return (1ull << (n_users - lo)) - 1ull;
}

// Word w of message m's recipient mask: the OR of its topic rows, or 0 for
// anything but a Broadcast.  Shared by the three K2a kernels, which differ
// only in where they store the word and in the origin filter: with
// SINGLE_HOP, a message that arrived from a peer broker (origin[m] != 0)
// keeps only its local-user bits (see "Peer-broker recipients").  m is taken
// as int64_t so that the caller's one widening of the message index serves
// the loads here and its own store index (with int m the origin kernel came
// out two VGPRs larger).
template <bool SINGLE_HOP>
__device__ __forceinline__ uint64_t topic_row_or(
    const uint64_t* __restrict__ sub_bitmap, const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ topics_off, const int32_t* __restrict__ topics_cnt,
    const int32_t* __restrict__ disc, int64_t m, int w, int32_t W,
    const int32_t* __restrict__ origin, int32_t n_users)
{
    uint64_t acc = 0;
    if (disc[m] == 4) {
        const uint8_t* topics = buf + topics_off[m];
        int n = topics_cnt[m];
        for (int t = 0; t < n; ++t) acc |= sub_bitmap[(int64_t)topics[t] * W + w];
        if (SINGLE_HOP && origin[m] != 0) acc &= user_bits_of_word(w, n_users);
    }
    return acc;
}

extern "C" __global__ void k2a_topic_mask(
    const uint64_t* __restrict__ sub_bitmap,  // [256][W]
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ topics_off,
    const int32_t* __restrict__ topics_cnt,
    const int32_t* __restrict__ disc,
    uint64_t* __restrict__ mask,              // [M][W]
    int32_t M, int32_t W)
{
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)M * W) return;
    int m = idx / W;
    int w = idx % W;
    mask[idx] = topic_row_or<false>(sub_bitmap, buf, topics_off, topics_cnt, disc, m, w, W,
                                    nullptr, 0);
}

// ---------------------------------------------------------------------------
// K2b: per-user ordered assignment + pair emission.
// One thread per user walks the M messages IN ORDER (per-(sender,recipient)
// FIFO), assigns consecutive ring offsets in its egress ring, and appends
// delivery pairs. Pair slots are claimed per-user via an exclusive scan over
// delivery counts computed in pass 0 (count_only=1), so the pair list is
// grouped by user and ordered by message within each user.
//
// egress ring layout: ring_bytes per user within a single [N_users][ring_bytes]
// tensor. Each delivery writes a 16-byte record header {u32 len, u32 msg_seq,
// 0, 0} followed by the payload, padded to a 16-byte stride (ring_rec; the
// host-side drain parses this).
// If the ring fills, the remaining deliveries for that user are dropped and
// counted (best-effort semantics = reference eviction-on-full, sender.rs).
// ---------------------------------------------------------------------------
extern "C" __global__ void k2b_count(
    const uint64_t* __restrict__ mask,   // [M][W]
    int32_t M, int32_t W, int32_t n_users,
    int32_t* __restrict__ counts)        // [n_users]
{
    int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_users) return;
    int w = u >> 6;
    uint64_t bit = 1ull << (u & 63);
    int c = 0;
    for (int m = 0; m < M; ++m) c += (mask[(int64_t)m * W + w] & bit) ? 1 : 0;
    counts[u] = c;
}

extern "C" __global__ void k2b_emit(
    const uint64_t* __restrict__ mask,        // [M][W]
    const int64_t* __restrict__ payload_off,  // [M]
    const int32_t* __restrict__ payload_len,  // [M]
    const int32_t* __restrict__ pair_base,    // [n_users] exclusive scan of counts
    int32_t M, int32_t W, int32_t n_users,
    int64_t ring_bytes,
    uint64_t* __restrict__ ring_wpos,         // [n_users] persistent write cursor
    PairRec* __restrict__ pairs,              // [total] {user,msg,dst}
    uint32_t* __restrict__ drops)             // [1] dropped deliveries (ring full)
{
    int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_users) return;
    int w = u >> 6;
    uint64_t bit = 1ull << (u & 63);
    int slot = pair_base[u];
    uint64_t wpos = ring_wpos[u];
    uint32_t dropped = 0;
    for (int m = 0; m < M; ++m) {
        if (!(mask[(int64_t)m * W + w] & bit)) continue;
        int32_t len = payload_len[m];
        // 16-aligned record stride (see ring_rec)
        uint64_t rec = ring_rec(len);
        if (wpos + rec > (uint64_t)ring_bytes) {
            store_pair(pairs + slot, -1, m, 0);
            slot++; dropped++; continue;
        }
        store_pair(pairs + slot, u, m, (int64_t)u * ring_bytes + wpos);
        slot++;
        wpos += rec;
    }
    ring_wpos[u] = wpos;
    if (dropped) atomicAdd(drops, dropped);
}

// ---------------------------------------------------------------------------
// K3: fan-out payload copy. Grid-stride over delivery pairs; each workgroup
// copies one pair per iteration with 16 B/lane vector loads/stores. Writes
// the 16-byte record header, then the payload. Source bytes for a hot message
// are L2/LLC-resident after the first few recipients.
// ---------------------------------------------------------------------------

// Cooperative copy of one inline record by `nlanes` lanes, this one being
// `lane`: lane 0 stores the header {len, seq, 0, 0}, then all lanes copy the
// payload in 16 B chunks and the last len % 16 bytes one by one.  dst is a
// record start, so it is 16-aligned (ring base and ring_rec stride are); a
// source that is not takes the byte-wise chunk loop, which stores plainly at
// either NT.  The one definition of an inline record's bytes: k3_fanout
// (a workgroup per record), k3_fanout_wave_t and k3_fanout_ref_t (a wave per
// record) all call it.
template <int NT>
__device__ __forceinline__ void copy_record(uint8_t* dst, const uint8_t* src, int32_t len,
                                            uint32_t seq, int lane, int nlanes)
{
    if (lane == 0) store16<NT>(dst, cdn_v4u{(uint32_t)len, seq, 0u, 0u});
    dst += 16;
    const int32_t nvec = len >> 4;  // full 16-byte chunks
    if ((((uintptr_t)src) & 15) == 0) {
        const cdn_v4u* s4 = (const cdn_v4u*)src;
        cdn_v4u* d4 = (cdn_v4u*)dst;
        for (int k = lane; k < nvec; k += nlanes) store16<NT>(d4 + k, s4[k]);
    } else {
        for (int k = lane; k < nvec; k += nlanes) {
            uint8_t tmp[16];
            memcpy(tmp, src + (size_t)k * 16, 16);
            memcpy(dst + (size_t)k * 16, tmp, 16);
        }
    }
    for (int k = (nvec << 4) + lane; k < len; k += nlanes) dst[k] = src[k];
}

extern "C" __global__ void k3_fanout(
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ payload_off,
    const int32_t* __restrict__ payload_len,
    const PairRec* __restrict__ pairs,
    const uint32_t* __restrict__ msg_seq,   // [M] global sequence numbers
    int32_t n_pairs,
    uint8_t* __restrict__ egress)
{
    for (int p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const PairRec pr = pairs[p];
        if (pr.user < 0) continue;  // dropped (ring full)
        int m = pr.msg;
        copy_record<0>(egress + pr.dst, buf + payload_off[m], payload_len[m], msg_seq[m],
                       threadIdx.x, blockDim.x);
    }
}

// ---------------------------------------------------------------------------
// K5: batched direct-route lookup. Open-addressing (linear probe) hash table
// over HBM: keys[S] = fnv1a64(pubkey) (0 = empty), vals[S] = owner id
// (>=0: local user index; <0: -(broker_rank+2); reference DirectMap).
// ---------------------------------------------------------------------------
extern "C" __global__ void k5_direct_lookup(
    const uint64_t* __restrict__ table_keys,
    const int32_t* __restrict__ table_vals,
    int64_t table_size,                      // power of two
    const uint64_t* __restrict__ query,      // [N]
    int32_t N,
    int32_t* __restrict__ owner)             // [N] out; INT32_MIN = not found
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    uint64_t h = query[i];
    if (h == 0) { owner[i] = INT32_MIN; return; }
    uint64_t mask = (uint64_t)table_size - 1;
    uint64_t s = h & mask;
    for (int64_t probe = 0; probe < table_size; ++probe) {
        uint64_t k = table_keys[(s + probe) & mask];
        if (k == h) { owner[i] = table_vals[(s + probe) & mask]; return; }
        if (k == 0) { owner[i] = INT32_MIN; return; }
    }
    owner[i] = INT32_MIN;
}

// ---------------------------------------------------------------------------
// Subscription updates (Subscribe/Unsubscribe batches) applied on-device.
// One thread per (update). Bitmap bit flips must be atomic (two users in one
// word updated concurrently).
// ---------------------------------------------------------------------------
extern "C" __global__ void k2c_apply_subs(
    uint64_t* __restrict__ sub_bitmap,       // [256][W]
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ topics_off,
    const int32_t* __restrict__ topics_cnt,
    const int32_t* __restrict__ disc,        // 5=subscribe 6=unsubscribe
    const int32_t* __restrict__ user_idx,    // [M] local user index per message
    int32_t M, int32_t W)
{
    // One thread applies the whole batch IN MESSAGE ORDER: a subscribe and
    // a later unsubscribe of the same (user, topic) in one batch must land
    // in order (subscription updates are control-plane-rate, so the serial
    // walk is microseconds; the data-plane kernels stay fully parallel).
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int m = 0; m < M; ++m) {
        int d = disc[m];
        if (d != 5 && d != 6) continue;
        int u = user_idx[m];
        if (u < 0) continue;
        int w = u >> 6;
        uint64_t bit = 1ull << (u & 63);
        const uint8_t* topics = buf + topics_off[m];
        int n = topics_cnt[m];
        for (int t = 0; t < n; ++t) {
            uint64_t* word = sub_bitmap + ((int64_t)topics[t] * W + w);
            if (d == 5) *word |= bit;
            else        *word &= ~bit;
        }
    }
}

// ---------------------------------------------------------------------------
// Host-side launchers (called from the torch-extension bindings, which are
// compiled as plain host C++ and cannot reference __global__ symbols).
// ---------------------------------------------------------------------------

// Runs `launch` with NT bound to the compile-time constant 1 or 0 according
// to the launcher's run-time `nt` flag (the kernels take NT as a template
// parameter).
#define DISPATCH_NT(nt, launch)                   \
    do {                                          \
        if (nt) { constexpr int NT = 1; launch; } \
        else    { constexpr int NT = 0; launch; } \
    } while (0)

// K2a grid: one thread per (message, mask word).
#define K2A_THREADS 256
static inline dim3 k2a_grid(int32_t M, int32_t W) {
    return dim3((uint32_t)(((int64_t)M * W + K2A_THREADS - 1) / K2A_THREADS));
}

extern "C" {

void launch_k4_parse(const uint8_t* buf, const int64_t* offsets, int32_t M, uint64_t hash_seed,
                     ParseOut out, hipStream_t s) {
    if (M <= 0) return;
    int threads = 256, blocks = (M + threads - 1) / threads;
    hipLaunchKernelGGL(k4_parse_batch, dim3(blocks), dim3(threads), 0, s, buf, offsets, M,
                       hash_seed, out);
}

void launch_k2a_topic_mask(const uint64_t* sub_bitmap, const uint8_t* buf,
                           const int64_t* topics_off, const int32_t* topics_cnt,
                           const int32_t* disc, uint64_t* mask, int32_t M, int32_t W,
                           hipStream_t s) {
    if (M <= 0) return;
    hipLaunchKernelGGL(k2a_topic_mask, k2a_grid(M, W), dim3(K2A_THREADS), 0, s, sub_bitmap, buf,
                       topics_off, topics_cnt, disc, mask, M, W);
}

void launch_k2b_count(const uint64_t* mask, int32_t M, int32_t W, int32_t n_users,
                      int32_t* counts, hipStream_t s) {
    int threads = 256, blocks = (n_users + threads - 1) / threads;
    hipLaunchKernelGGL(k2b_count, dim3(blocks), dim3(threads), 0, s, mask, M, W, n_users, counts);
}

void launch_k2b_emit(const uint64_t* mask, const int64_t* payload_off,
                     const int32_t* payload_len, const int32_t* pair_base, int32_t M, int32_t W,
                     int32_t n_users, int64_t ring_bytes, uint64_t* ring_wpos, PairRec* pairs,
                     uint32_t* drops, hipStream_t s) {
    int threads = 256, blocks = (n_users + threads - 1) / threads;
    hipLaunchKernelGGL(k2b_emit, dim3(blocks), dim3(threads), 0, s, mask, payload_off,
                       payload_len, pair_base, M, W, n_users, ring_bytes, ring_wpos, pairs,
                       drops);
}

void launch_k3_fanout(const uint8_t* buf, const int64_t* payload_off,
                      const int32_t* payload_len, const PairRec* pairs, const uint32_t* msg_seq,
                      int32_t n_pairs, uint8_t* egress, hipStream_t s) {
    int blocks = n_pairs < 16384 ? n_pairs : 16384;
    if (blocks == 0) return;
    hipLaunchKernelGGL(k3_fanout, dim3(blocks), dim3(128), 0, s, buf, payload_off, payload_len,
                       pairs, msg_seq, n_pairs, egress);
}

void launch_k5_direct_lookup(const uint64_t* table_keys, const int32_t* table_vals,
                             int64_t table_size, const uint64_t* query, int32_t N,
                             int32_t* owner, hipStream_t s) {
    int threads = 256, blocks = (N + threads - 1) / threads;
    hipLaunchKernelGGL(k5_direct_lookup, dim3(blocks), dim3(threads), 0, s, table_keys,
                       table_vals, table_size, query, N, owner);
}

void launch_k2c_apply_subs(uint64_t* sub_bitmap, const uint8_t* buf, const int64_t* topics_off,
                           const int32_t* topics_cnt, const int32_t* disc,
                           const int32_t* user_idx, int32_t M, int32_t W, hipStream_t s) {
    int threads = 256, blocks = (M + threads - 1) / threads;
    hipLaunchKernelGGL(k2c_apply_subs, dim3(blocks), dim3(threads), 0, s, sub_bitmap, buf,
                       topics_off, topics_cnt, disc, user_idx, M, W);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// K3v2: wave-per-pair fan-out. 256-thread workgroups = 4 waves; each wave
// owns one delivery pair per grid-stride iteration (64 lanes x 16 B = 1 KiB
// per pass — matches the 1 KiB-payload sweet spot; a 64 KiB payload takes 64
// passes). n_pairs is read from a device pointer so the host never syncs on
// the pair count. NT=1 uses non-temporal stores for the egress payload
// (written once, consumed by the D2H drain) to keep the per-XCD L2 for the
// hot message source bytes instead of the streaming egress.
// ---------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(256) k3_fanout_wave_t(
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ payload_off,
    const int32_t* __restrict__ payload_len,
    const PairRec* __restrict__ pairs,
    const uint32_t* __restrict__ msg_seq,
    const int32_t* __restrict__ n_pairs_ptr,
    int32_t capacity,
    uint8_t* __restrict__ egress)
{
    // clamp: the claim counter keeps counting past the pair buffer when a
    // tick oversubscribes pair_capacity (claims beyond it are recorded as
    // drops, never stored) — reading pairs[] to the raw counter walked off
    // the buffer and faulted (batch 1024 x 12.5k-subscriber mixed config)
    int n_pairs = *n_pairs_ptr;
    if (n_pairs > capacity) n_pairs = capacity;
    const int lane = threadIdx.x & 63;
    const int wave_in_wg = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    for (int p = blockIdx.x * 4 + wave_in_wg; p < n_pairs; p += waves_total) {
        const PairRec pr = pairs[p];
        if (pr.user < 0) continue;
        const int mi = pr.msg;
        const int32_t len = payload_len[mi];
        copy_record<NT>(egress + pr.dst, buf + payload_off[mi], len, msg_seq[mi], lane, WAVE);
    }
}

extern "C" {

void launch_k3_fanout_wave(const uint8_t* buf, const int64_t* payload_off,
                           const int32_t* payload_len, const PairRec* pairs,
                           const uint32_t* msg_seq, const int32_t* n_pairs_ptr,
                           int32_t capacity,
                           uint8_t* egress, int nt, int grid, hipStream_t s) {
    if (grid <= 0) grid = 4096;  // 4096 WGs x 4 waves = 16384 concurrent pairs
    DISPATCH_NT(nt, hipLaunchKernelGGL((k3_fanout_wave_t<NT>), dim3(grid), dim3(256), 0, s, buf,
                                       payload_off, payload_len, pairs, msg_seq, n_pairs_ptr,
                                       capacity, egress));
}

}  // extern "C"

// ---------------------------------------------------------------------------
// K3r: fan-out with by-reference delivery.  Same pair list as the wave
// kernel; a message of at least ref_threshold bytes is delivered as a bare
// 16 B header {u32 len | REF_FLAG, u32 seq, u64 ref_base + payload_off[msg]}
// and its payload stays in the host's copy of the batch; any shorter message
// is written by copy_record, the same call k3_fanout_wave_t makes.
//
// Work split: a wave owns G CONSECUTIVE pairs per grid-stride step, one
// pair per lane (lanes >= G hold none).  The by-reference lanes store their
// header together (one dword4 store per lane, one wave instruction for up to
// G pairs) — a wave per pair would spend a whole wave on each 16 B store.
// The wave then walks the ballot of inline lanes, broadcasts that lane's
// pair through __shfl and copies the record cooperatively with copy_record
// (64 lanes x 16 B per pass).
//
// G is the smallest power of two, at most 64, at which one step of all the
// grid's waves covers the pair list.  A fixed G = 64 was measured first: it
// leaves a small tick on n_pairs / 64 waves, each copying its inline records
// one after the other (8,000 inline pairs of 64 KiB: 1.24 ms against the
// wave kernel's 0.16 ms; profiles/byref_delivery_fixed64.json).  With the adaptive G a list
// shorter than the grid runs one pair per wave, exactly the wave kernel's
// schedule, and only a list that oversubscribes the grid is packed, which is
// also where the header stores are many enough to be worth packing.
// ---------------------------------------------------------------------------
#define REF_FLAG 0x80000000u

template <int NT>
__global__ void __launch_bounds__(256) k3_fanout_ref_t(
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ payload_off,
    const int32_t* __restrict__ payload_len,
    const PairRec* __restrict__ pairs,
    const uint32_t* __restrict__ msg_seq,
    const int32_t* __restrict__ n_pairs_ptr,
    int32_t capacity,
    int32_t ref_threshold,
    int64_t ref_base,
    uint8_t* __restrict__ egress)
{
    int n_pairs = *n_pairs_ptr;
    if (n_pairs > capacity) n_pairs = capacity;  // see k3_fanout_wave_t
    const int lane = threadIdx.x & 63;
    const int wave_in_wg = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    int gs = 0;  // log2(G); n_pairs is wave-uniform, so this loop is scalar
    while (gs < 6 && ((n_pairs - 1) >> gs) + 1 > waves_total) ++gs;
    const int n_groups = n_pairs > 0 ? ((n_pairs - 1) >> gs) + 1 : 0;
    for (int g = blockIdx.x * 4 + wave_in_wg; g < n_groups; g += waves_total) {
        const int64_t p = ((int64_t)g << gs) + lane;
        int32_t len = 0;
        uint32_t seq = 0;
        int64_t off = 0, dsto = 0;
        bool live = false;
        if (lane < (1 << gs) && p < n_pairs) {
            const PairRec pr = pairs[p];
            if (pr.user >= 0) {
                live = true;
                len = payload_len[pr.msg];
                off = payload_off[pr.msg];
                seq = msg_seq[pr.msg];
                dsto = pr.dst;
            }
        }
        const bool by_ref = live && len >= ref_threshold;
        if (by_ref) {
            const uint64_t ro = (uint64_t)(ref_base + off);
            store16<NT>(egress + dsto, cdn_v4u{(uint32_t)len | REF_FLAG, seq, (uint32_t)ro,
                                               (uint32_t)(ro >> 32)});
        }
        // every lane of the wave reaches the ballot and the shuffles below
        unsigned long long inl = __ballot(live && !by_ref);
        while (inl) {
            const int j = __ffsll((long long)inl) - 1;
            inl &= inl - 1;
            const int32_t jlen = __shfl(len, j);
            const uint32_t jseq = (uint32_t)__shfl((int)seq, j);
            const int64_t joff = ((int64_t)__shfl((int)(off >> 32), j) << 32)
                                 | (uint32_t)__shfl((int)off, j);
            const int64_t jdst = ((int64_t)__shfl((int)(dsto >> 32), j) << 32)
                                 | (uint32_t)__shfl((int)dsto, j);
            copy_record<NT>(egress + jdst, buf + joff, jlen, jseq, lane, WAVE);
        }
    }
}

extern "C" {

void launch_k3_fanout_ref(const uint8_t* buf, const int64_t* payload_off,
                          const int32_t* payload_len, const PairRec* pairs,
                          const uint32_t* msg_seq, const int32_t* n_pairs_ptr,
                          int32_t capacity, int32_t ref_threshold, int64_t ref_base,
                          uint8_t* egress, int nt, int grid, hipStream_t s) {
    if (grid <= 0) grid = 4096;  // 4096 WGs x 4 waves, up to 64 pairs per wave and step
    DISPATCH_NT(nt, hipLaunchKernelGGL((k3_fanout_ref_t<NT>), dim3(grid), dim3(256), 0, s, buf,
                                       payload_off, payload_len, pairs, msg_seq, n_pairs_ptr,
                                       capacity, ref_threshold, ref_base, egress));
}

}  // extern "C"

// ---------------------------------------------------------------------------
// K3 flat fan-out for UNIFORM record sizes: work unit = one 16 B chunk of
// one delivery record, lane -> consecutive flat units (~100% lane
// utilization at any payload size; the wave-per-pair variant idles lanes on
// the tail pass). Two entry points share the template:
//   flat2: seq base passed by value (eager path)
//   flat3: seq base read from a device counter (hipGraph-capturable; a
//          host-passed base would be frozen into the captured graph)
// n_pairs is read from a device pointer and clamped to the buffer capacity.
// ---------------------------------------------------------------------------
// The 16 bytes a full-stride record holds at payload byte offset coff (a
// multiple of 16) of the len-byte message at msg: the source bytes, zeros
// past the message's end.  The one definition of those bytes: the flat
// kernels call it per delivered unit, the dense fan-out once per image unit.
__device__ __forceinline__ cdn_v4u payload_unit(const uint8_t* __restrict__ msg, int32_t coff,
                                                int32_t len)
{
    const uint8_t* src = msg + coff;
    if (coff + 16 <= len && (((uintptr_t)src) & 15) == 0) return *(const cdn_v4u*)src;
    // pure pad unit: zeros, so the record stride is fully written
    // (full-line NT writes, no RMW at record boundaries)
    if (coff >= len) return cdn_v4u{0u, 0u, 0u, 0u};
    // misaligned source or partial tail unit: zero-fill to one full 16 B store
    uint8_t tmp[16];
    #pragma unroll
    for (int b = 0; b < 16; ++b) tmp[b] = (coff + b < len) ? src[b] : 0;
    cdn_v4u v; memcpy(&v, tmp, 16);
    return v;
}

// The flat fan-out as workgroup `block` of `n_blocks`: the count read and
// clamped, then a grid-stride walk over the list's units.  The one definition
// of that walk: k3_fanout_flat_t is a grid of these, and the fused tick's
// k3_fanout_dense_tail_t runs them behind its dense workgroups.
template <int NT>
__device__ __forceinline__ void k3_flat_body(
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ payload_off,
    const int32_t* __restrict__ payload_len,
    const PairRec* __restrict__ pairs,
    uint32_t seq_base,
    const int32_t* __restrict__ n_pairs_ptr,
    int32_t capacity,
    int32_t units_per_pair,
    uint32_t div_magic,                   // Granlund-Montgomery multiplier for
    int32_t div_shift,                    // f/units_per_pair (exact for f<2^31,
                                          // d<=2^21; a per-unit 64-bit idiv was
                                          // ~25 VALU ops on the hottest loop)
    int32_t uniform_len,                  // >0: every record is this long —
                                          // skips the per-unit length load
    uint8_t* __restrict__ egress,
    uint32_t block, uint32_t n_blocks)
{
    int np = *n_pairs_ptr;
    if (np > capacity) np = capacity;
    const int64_t n_units = (int64_t)np * units_per_pair;
    const int64_t stride = (int64_t)n_blocks * blockDim.x;
    for (int64_t f = (int64_t)block * blockDim.x + threadIdx.x; f < n_units; f += stride) {
        const uint32_t f32 = (uint32_t)f;  // n_units < 2^31 (capacity*units)
        const int p = (int)(((uint64_t)f32 * div_magic) >> div_shift);
        const int unit = (int)(f32 - (uint32_t)p * (uint32_t)units_per_pair);
        const PairRec pr = pairs[p];   // one dword4 load
        if (pr.user < 0) continue;
        const int mi = pr.msg;
        const int32_t len = uniform_len > 0 ? uniform_len : payload_len[mi];
        uint8_t* dst = egress + pr.dst + (size_t)unit * 16;
        if (unit == 0) {
            store16<NT>(dst, cdn_v4u{(uint32_t)len, seq_base + (uint32_t)mi, 0u, 0u});
            continue;
        }
        store16<NT>(dst, payload_unit(buf + payload_off[mi], (unit - 1) * 16, len));
    }
}

template <int NT, bool SEQ_FROM_PTR>
__global__ void __launch_bounds__(256) k3_fanout_flat_t(
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ payload_off,
    const int32_t* __restrict__ payload_len,
    const PairRec* __restrict__ pairs,
    uint32_t seq_base_val,
    const uint32_t* __restrict__ seq_state,
    const int32_t* __restrict__ n_pairs_ptr,
    int32_t capacity,
    int32_t units_per_pair,
    uint32_t div_magic, int32_t div_shift,
    int32_t uniform_len,
    uint8_t* __restrict__ egress)
{
    const uint32_t seq_base = SEQ_FROM_PTR ? seq_state[0] : seq_base_val;
    k3_flat_body<NT>(buf, payload_off, payload_len, pairs, seq_base, n_pairs_ptr, capacity,
                     units_per_pair, div_magic, div_shift, uniform_len, egress, blockIdx.x,
                     gridDim.x);
}

// u32_div_magic (csrc/common/divmagic.h): p = (f * m) >> sh, exact for all
// f < 2^31 and 1 <= d <= 2^21 — the bindings enforce both bounds
// (units_per_pair <= 2^21, capacity * units_per_pair < 2^31) before launch.

template <bool SEQ_FROM_PTR>
static void launch_flat(const uint8_t* buf, const int64_t* payload_off,
                        const int32_t* payload_len, const PairRec* pairs, uint32_t seq_base,
                        const uint32_t* seq_state, const int32_t* n_pairs_ptr, int32_t capacity,
                        int32_t units_per_pair, int32_t uniform_len, uint8_t* egress, int nt,
                        int grid, hipStream_t s) {
    if (grid <= 0) grid = 16384;  // swept: 16384 > 8192 > 4096 (~0.5% each)
    uint32_t dm; int32_t dsh;
    u32_div_magic(units_per_pair, &dm, &dsh);
    DISPATCH_NT(nt, hipLaunchKernelGGL((k3_fanout_flat_t<NT, SEQ_FROM_PTR>), dim3(grid),
                                       dim3(256), 0, s, buf, payload_off, payload_len, pairs,
                                       seq_base, seq_state, n_pairs_ptr, capacity,
                                       units_per_pair, dm, dsh, uniform_len, egress));
}

extern "C" __global__ void k_seq_advance(uint32_t* seq_state, int32_t m) {
    if (blockIdx.x == 0 && threadIdx.x == 0) seq_state[0] += (uint32_t)m;
}

extern "C" {

void launch_k3_fanout_flat2(const uint8_t* buf, const int64_t* payload_off,
                            const int32_t* payload_len, const PairRec* pairs,
                            uint32_t seq_base, const int32_t* n_pairs_ptr, int32_t capacity,
                            int32_t units_per_pair, int32_t uniform_len, uint8_t* egress,
                            int nt, int grid, hipStream_t s) {
    launch_flat<false>(buf, payload_off, payload_len, pairs, seq_base, nullptr, n_pairs_ptr,
                       capacity, units_per_pair, uniform_len, egress, nt, grid, s);
}

void launch_k3_fanout_flat3(const uint8_t* buf, const int64_t* payload_off,
                            const int32_t* payload_len, const PairRec* pairs,
                            const uint32_t* seq_state, const int32_t* n_pairs_ptr,
                            int32_t capacity, int32_t units_per_pair, int32_t uniform_len,
                            uint8_t* egress, int nt, int grid, hipStream_t s) {
    launch_flat<true>(buf, payload_off, payload_len, pairs, 0u, seq_state, n_pairs_ptr,
                      capacity, units_per_pair, uniform_len, egress, nt, grid, s);
}

void launch_k_seq_advance(uint32_t* seq_state, int32_t m, hipStream_t s) {
    hipLaunchKernelGGL(k_seq_advance, dim3(1), dim3(1), 0, s, seq_state, m);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Transposed-mask pipeline: mask_t[W][M] instead of [M][W] so K2b's per-user
// scan over messages reads CONTIGUOUS memory (wide loads + ILP instead of a
// 1.2 KB stride per iteration — K2b is latency-bound at ~157 waves).
// ---------------------------------------------------------------------------
extern "C" __global__ void k2a_topic_mask_t(
    const uint64_t* __restrict__ sub_bitmap,  // [256][W]
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ topics_off,
    const int32_t* __restrict__ topics_cnt,
    const int32_t* __restrict__ disc,
    uint64_t* __restrict__ mask_t,            // [W][M]
    int32_t M, int32_t W)
{
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)M * W) return;
    int m = idx / W;
    int w = idx % W;
    mask_t[(int64_t)w * M + m] =
        topic_row_or<false>(sub_bitmap, buf, topics_off, topics_cnt, disc, m, w, W, nullptr, 0);
}

// Wave-aggregated span claim: a wave64 inclusive scan of the lanes' counts
// and ONE atomicAdd of the wave's total on `counter` (157 atomics for 10k
// users instead of 10k — a single counter word saturates at ~88 atomics/us,
// MI355X_MICROARCH 'dequeue' row).  Returns the first slot of this lane's
// `count` consecutive slots; the wave's spans are contiguous in lane order.
// EVERY lane of the wave must reach this call (it shuffles): a caller whose
// lane has no work passes count = 0 and returns only afterwards.
__device__ __forceinline__ int wave_claim_span(int count, int32_t* __restrict__ counter) {
    const int lane = threadIdx.x & 63;
    int incl = count;
    for (int d = 1; d < 64; d <<= 1) {
        int ngh = __shfl_up(incl, d);
        if (lane >= d) incl += ngh;
    }
    int wave_total = __shfl(incl, 63);
    int base = 0;
    if (lane == 0 && wave_total > 0) base = atomicAdd(counter, wave_total);
    base = __shfl(base, 0);
    return base + incl - count;
}

// uniform_rec != 0: every record in this tick is uniform_rec bytes (the
// uniform-wire broadcast shape) — ring math is closed-form and payload_len
// is never loaded. Slot claims are wave-aggregated (wave_claim_span), which
// keeps the pair list contiguous.
extern "C" __global__ void k2b_fused_t(
    const uint64_t* __restrict__ mask_t,      // [W][M]
    const int32_t* __restrict__ payload_len,
    int32_t M, int32_t W, int32_t n_users,
    int64_t ring_bytes, int32_t capacity, int32_t uniform_rec,
    uint64_t* __restrict__ ring_wpos,
    int32_t* __restrict__ n_pairs,            // [1] global pair counter (zeroed)
    PairRec* __restrict__ pairs,
    uint32_t* __restrict__ drops)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = u < n_users;
    const int w = u >> 6;
    const uint64_t bit = 1ull << (u & 63);
    const uint64_t* col = mask_t + (int64_t)w * M;
    int count = 0;
    if (active) {
#pragma unroll 8
        for (int m = 0; m < M; ++m) count += (col[m] & bit) ? 1 : 0;
    }
    // inactive lanes carry count = 0 through the wave-wide claim
    int slot = wave_claim_span(count, n_pairs);
    if (!active || count == 0) return;

    if (uniform_rec) {
        uint64_t wpos = ring_wpos[u];
        const int32_t fit = (int32_t)((ring_bytes - wpos) / (uint64_t)uniform_rec);
        uint32_t dropped = 0;
        int emitted = 0;
        const int64_t dst_base = (int64_t)u * ring_bytes + (int64_t)wpos;
        for (int m = 0; m < M; ++m) {
            if (!(col[m] & bit)) continue;
            const bool ok = (emitted < fit) && (slot < capacity);
            if (!ok) {
                if (slot < capacity) { store_pair(pairs + slot, -1, m, 0); slot++; }
                dropped++;
                continue;
            }
            store_pair(pairs + slot, u, m, dst_base + (int64_t)emitted * uniform_rec);
            slot++;
            emitted++;
        }
        ring_wpos[u] = wpos + (uint64_t)emitted * uniform_rec;
        if (dropped) atomicAdd(drops, dropped);
        return;
    }

    uint64_t wpos = ring_wpos[u];
    uint32_t dropped = 0;
    for (int m = 0; m < M; ++m) {
        if (!(col[m] & bit)) continue;
        int32_t len = payload_len[m];
        uint64_t rec = ring_rec(len);
        bool fits_ring = (wpos + rec <= (uint64_t)ring_bytes);
        bool fits_cap = (slot < capacity);
        if (!fits_ring || !fits_cap) {
            if (fits_cap) { store_pair(pairs + slot, -1, m, 0); slot++; }
            dropped++;
            continue;
        }
        store_pair(pairs + slot, u, m, (int64_t)u * ring_bytes + wpos);
        slot++;
        wpos += rec;
    }
    ring_wpos[u] = wpos;
    if (dropped) atomicAdd(drops, dropped);
}

extern "C" {

void launch_k2a_topic_mask_t(const uint64_t* sub_bitmap, const uint8_t* buf,
                             const int64_t* topics_off, const int32_t* topics_cnt,
                             const int32_t* disc, uint64_t* mask_t, int32_t M, int32_t W,
                             hipStream_t s) {
    if (M <= 0) return;
    hipLaunchKernelGGL(k2a_topic_mask_t, k2a_grid(M, W), dim3(K2A_THREADS), 0, s, sub_bitmap,
                       buf, topics_off, topics_cnt, disc, mask_t, M, W);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// K2b block-parallel variant for UNIFORM records.  The fused kernel above
// runs one lane per user, so a 10k-user broker fills only ~157 wave slots
// of the 1024 SIMDs (measured 142 us/tick = 15% of the broadcast tick).
// This three-launch pipeline parallelizes over (user-wave, message-block)
// while producing a BIT-IDENTICAL pair list (grouped per user, messages in
// order, same placeholder/drop semantics):
//   P1  per-(user, 32-msg block) set-bit counts
//   P2  per-user totals -> wave-aggregated pair-span claim + closed-form
//       ring math (emitted = min(total, ring fit, pair-capacity headroom))
//       + per-block exclusive prefixes
//   P3  per-(user, block) emission at precomputed offsets
// ---------------------------------------------------------------------------
// (K2B_BLK, the block size, is in dataplane.h)

// The K2b bodies below serve two layouts of the per-tile arrays (bcount,
// pprefix, tslot): [NB][W*64] int32 in global scratch, indexed by the user u
// (stride = W * 64, col = u), and the route kernel's [NB][64] narrow arrays
// in LDS, one mask word's users indexed by lane (stride = 64, col = lane;
// RouteLds, tick_geom.h).  `wcol` is the [M] column of mask words of the
// wave's mask word, in mask_t or in LDS.  Tile (b, user) is at b * stride + col.

// P1 for one tile: how many of block b's messages go to this lane's user.
__device__ __forceinline__ int k2b_tile_count(const uint64_t* __restrict__ wcol, int32_t M, int b)
{
    const uint64_t bit = 1ull << (threadIdx.x & 63);
    const int m0 = b * K2B_BLK, m1 = min(M, m0 + K2B_BLK);
    int c = 0;
    for (int m = m0; m < m1; ++m) c += (wcol[m] & bit) ? 1 : 0;
    return c;
}

// P1 body, shared with the fused tick's k2b_p1_count_z.
__device__ __forceinline__ void k2b_p1_body(
    const uint64_t* __restrict__ mask_t,   // [W][M]
    int32_t M, int32_t W, int32_t NB,
    int32_t* __restrict__ bcount)          // [NB][W*64]
{
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave >= W * NB) return;
    const int w = wave / NB, b = wave - (int64_t)(wave / NB) * NB;
    const int lane = threadIdx.x & 63;
    bcount[(int64_t)b * (W * 64) + (w * 64 + lane)] = k2b_tile_count(mask_t + (int64_t)w * M, M, b);
}

extern "C" __global__ void k2b_p1_count(
    const uint64_t* __restrict__ mask_t, int32_t M, int32_t W, int32_t NB,
    int32_t* __restrict__ bcount)
{
    k2b_p1_body(mask_t, M, W, NB, bcount);
}

// What P2 settles for one user (lane): the pair-slot base of its span, how
// many records its ring still takes, and where the first of them goes.
struct K2bUser { int32_t base; int32_t fit; int64_t dst; };

// P2 body, shared by k2b_p2_bases and the fused tick's k2b_p2_tiles: per-user
// totals and block prefixes, the wave-aggregated span claim, the closed-form
// ring math (cursor advance) and the drop count.  Every lane of the wave
// must call it (it shuffles); an inactive lane gets zeros back.
template <class Cnt, class Pre>
__device__ __forceinline__ K2bUser k2b_p2_body(
    const Cnt* __restrict__ bcount,        // tiles
    int u, bool active, int32_t stride, int col, int32_t NB,
    int64_t ring_bytes, int32_t capacity, int32_t uniform_rec,
    uint64_t* __restrict__ ring_wpos,
    int32_t* __restrict__ n_pairs,
    Pre* __restrict__ pprefix,             // tiles, out: per-block p-offset
    uint32_t* __restrict__ drops)
{
    const int lane = threadIdx.x & 63;
    int total = 0;
    if (active) {
        for (int b = 0; b < NB; ++b) {
            pprefix[(int64_t)b * stride + col] = (Pre)total;
            total += bcount[(int64_t)b * stride + col];
        }
    }
    // the contiguous per-user span; inactive lanes carry total = 0 through it
    K2bUser r{wave_claim_span(total, n_pairs), 0, 0};
    uint32_t dropped = 0;
    if (active) {
        const uint64_t wpos = ring_wpos[u];
        r.fit = (int32_t)((ring_bytes - wpos) / (uint64_t)uniform_rec);
        r.dst = (int64_t)u * ring_bytes + (int64_t)wpos;
        int cap_room = capacity - r.base; if (cap_room < 0) cap_room = 0;
        int emitted = total; if (emitted > r.fit) emitted = r.fit; if (emitted > cap_room) emitted = cap_room;
        ring_wpos[u] = wpos + (uint64_t)emitted * uniform_rec;
        dropped = (uint32_t)(total - emitted);
    }
    // one drops atomic per wave
    for (int d = 1; d < 64; d <<= 1) dropped += __shfl_down(dropped, d);
    if (lane == 0 && dropped) atomicAdd(drops, dropped);
    return r;
}

extern "C" __global__ void k2b_p2_bases(
    const int32_t* __restrict__ bcount,    // [NB][W*64]
    int32_t W, int32_t NB, int32_t n_users,
    int64_t ring_bytes, int32_t capacity, int32_t uniform_rec,
    uint64_t* __restrict__ ring_wpos,
    int32_t* __restrict__ n_pairs,
    int32_t* __restrict__ pprefix,         // [NB][W*64] out: per-block p-offset
    int32_t* __restrict__ ubase,           // [W*64] out: pair-slot base
    int32_t* __restrict__ ufit,            // [W*64] out: ring fit (records)
    int64_t* __restrict__ udst,            // [W*64] out: ring dst base
    uint32_t* __restrict__ drops)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = u < n_users;
    const K2bUser r = k2b_p2_body(bcount, u, active, W * 64, u, NB, ring_bytes, capacity,
                                  uniform_rec, ring_wpos, n_pairs, pprefix, drops);
    if (active) {
        ubase[u] = r.base;
        ufit[u] = r.fit;
        udst[u] = r.dst;
    }
}

extern "C" __global__ void k2b_p3_emit(
    const uint64_t* __restrict__ mask_t,   // [W][M]
    const int32_t* __restrict__ pprefix,   // [NB][W*64]
    const int32_t* __restrict__ ubase,
    const int32_t* __restrict__ ufit,
    const int64_t* __restrict__ udst,
    int32_t M, int32_t W, int32_t NB, int32_t n_users,
    int32_t capacity, int32_t uniform_rec,
    PairRec* __restrict__ pairs)
{
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave >= W * NB) return;
    const int w = wave / NB, b = wave - (int64_t)(wave / NB) * NB;
    const int lane = threadIdx.x & 63;
    const int u = w * 64 + lane;
    if (u >= n_users) return;
    const uint64_t bit = 1ull << lane;
    const uint64_t* col = mask_t + (int64_t)w * M;
    int p = pprefix[(int64_t)b * (W * 64) + u];
    const int base = ubase[u], fit = ufit[u];
    const int64_t dstb = udst[u];
    const int m0 = b * K2B_BLK, m1 = min(M, m0 + K2B_BLK);
    for (int m = m0; m < m1; ++m) {
        if (!(col[m] & bit)) continue;
        const int slot = base + p;
        if (slot < capacity) {
            if (p < fit)
                store_pair(pairs + slot, u, m, dstb + (int64_t)p * uniform_rec);
            else  // ring full: placeholder, counted in P2
                store_pair(pairs + slot, -1, m, 0);
        }
        p++;
    }
}

extern "C" void launch_k2b_blocks_t(
    const uint64_t* mask_t, int32_t M, int32_t W, int32_t n_users,
    int64_t ring_bytes, int32_t capacity, int32_t uniform_rec,
    uint64_t* ring_wpos, int32_t* n_pairs,
    int32_t* bcount, int32_t* pprefix, int32_t* ubase, int32_t* ufit, int64_t* udst,
    PairRec* pairs,
    uint32_t* drops, hipStream_t s) {
    if (M <= 0) return;
    const int NB = (M + K2B_BLK - 1) / K2B_BLK;
    const int waves = W * NB;
    const int threads = 256;
    const int blocks_wb = (waves * 64 + threads - 1) / threads;
    const int blocks_u = (n_users + threads - 1) / threads;
    hipLaunchKernelGGL(k2b_p1_count, dim3(blocks_wb), dim3(threads), 0, s,
                       mask_t, M, W, NB, bcount);
    hipLaunchKernelGGL(k2b_p2_bases, dim3(blocks_u), dim3(threads), 0, s,
                       bcount, W, NB, n_users, ring_bytes, capacity, uniform_rec,
                       ring_wpos, n_pairs, pprefix, ubase, ufit, udst, drops);
    hipLaunchKernelGGL(k2b_p3_emit, dim3(blocks_wb), dim3(threads), 0, s,
                       mask_t, pprefix, ubase, ufit, udst, M, W, NB, n_users,
                       capacity, uniform_rec, pairs);
}

extern "C" {

void launch_k2b_fused_t(const uint64_t* mask_t, const int32_t* payload_len, int32_t M,
                        int32_t W, int32_t n_users, int64_t ring_bytes, int32_t capacity,
                        int32_t uniform_rec, uint64_t* ring_wpos, int32_t* n_pairs,
                        PairRec* pairs,
                        uint32_t* drops, hipStream_t s) {
    int threads = 256, blocks = (n_users + threads - 1) / threads;
    hipLaunchKernelGGL(k2b_fused_t, dim3(blocks), dim3(threads), 0, s, mask_t, payload_len, M,
                       W, n_users, ring_bytes, capacity, uniform_rec, ring_wpos, n_pairs,
                       pairs, drops);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// K5b: on-device direct-message delivery pair emission. For each Direct
// message whose K5 owner lookup resolved to a LOCAL user, claim ring space
// (atomic on the user's cursor — per-sender order within a tick is
// preserved by message index only per thread; cross-sender order is
// unspecified, as in the reference's independent per-conn tasks) and append
// a delivery pair. Replaces the host-side direct routing loop (which cost a
// D2H sync per tick).
// ---------------------------------------------------------------------------

// Claim a pair slot and `len` payload bytes of ring u for message i, then
// store the pair.  No pair slot left: count a drop, store nothing.  Ring
// full: store a user = -1 placeholder (K3 skips it) and count a drop.
// Shared by both K5b kernels, which only decide u.
__device__ __forceinline__ void k5b_claim_emit(
    int u, int i, int32_t len, int64_t ring_bytes, int32_t capacity,
    uint64_t* __restrict__ ring_wpos, int32_t* __restrict__ n_pairs,
    PairRec* __restrict__ pairs, uint32_t* __restrict__ drops)
{
    uint64_t rec = ring_rec(len);
    int slot = atomicAdd(n_pairs, 1);
    if (slot >= capacity) {
        atomicAdd(drops, 1u);
        return;
    }
    // CAS claim: the round-1 add-then-rollback scheme could, with two
    // concurrent overshooters and an interleaved accept, leave an accepted
    // interval ABOVE a rolled-back one and let later claims overlap it.
    // CAS never inflates the cursor, so accepted intervals are exact and
    // a full ring drops cleanly (counted) with no spurious rollback race.
    unsigned long long cur = atomicAdd((unsigned long long*)&ring_wpos[u], 0ull);
    while (true) {
        if (cur + rec > (uint64_t)ring_bytes) {
            store_pair(pairs + slot, -1, i, 0);
            atomicAdd(drops, 1u);
            return;
        }
        unsigned long long prev = atomicCAS((unsigned long long*)&ring_wpos[u], cur,
                                            cur + (unsigned long long)rec);
        if (prev == cur) break;
        cur = prev;
    }
    store_pair(pairs + slot, u, i, (int64_t)u * ring_bytes + (int64_t)cur);
}

extern "C" __global__ void k5b_emit_direct(
    const int32_t* __restrict__ disc,
    const int32_t* __restrict__ owner,        // K5 output; >=0 = local user
    const int64_t* __restrict__ payload_off,  // wire offsets (fanout_wire)
    const int32_t* __restrict__ payload_len,
    int32_t M,
    int64_t ring_bytes, int32_t capacity,
    uint64_t* __restrict__ ring_wpos,
    int32_t* __restrict__ n_pairs,
    PairRec* __restrict__ pairs,
    uint32_t* __restrict__ drops)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    if (disc[i] != 3) return;
    int u = owner[i];
    if (u < 0) return;
    k5b_claim_emit(u, i, payload_len[i], ring_bytes, capacity, ring_wpos, n_pairs, pairs,
                   drops);
}

extern "C" void launch_k5b_emit_direct(
    const int32_t* disc, const int32_t* owner, const int64_t* payload_off,
    const int32_t* payload_len, int32_t M, int64_t ring_bytes, int32_t capacity,
    uint64_t* ring_wpos, int32_t* n_pairs, PairRec* pairs, uint32_t* drops, hipStream_t s) {
    int threads = 256, blocks = (M + threads - 1) / threads;
    hipLaunchKernelGGL(k5b_emit_direct, dim3(blocks), dim3(threads), 0, s, disc, owner,
                       payload_off, payload_len, M, ring_bytes, capacity, ring_wpos, n_pairs,
                       pairs, drops);
}

// ---------------------------------------------------------------------------
// K7: egress-ring compaction. Gathers every ring's used prefix into one
// contiguous staging buffer so the per-tick drain is ONE D2H copy + ONE
// C++ pump call instead of one of each per user (the socket-path
// bottleneck: reference Arc-clone forwarding has no per-recipient copies
// either, sender.rs:16-33).  wpos/dst_off are device tensors; records are
// 16-aligned so 16 B vector copies cover exactly the used bytes.
//   grid.x = ring (user), grid.y = 64 KiB chunk of that ring
// ---------------------------------------------------------------------------
#define K7_CHUNK (64 * 1024)

extern "C" __global__ void k7_compact_rings(
    const uint8_t* __restrict__ egress,
    int64_t ring_bytes,
    const int64_t* __restrict__ wpos,     // [N] used bytes per ring
    const int64_t* __restrict__ dst_off,  // [N] exclusive scan of wpos
    uint8_t* __restrict__ staging)
{
    int u = blockIdx.x;
    int64_t used = wpos[u];
    int64_t chunk = (int64_t)blockIdx.y * K7_CHUNK;
    if (chunk >= used) return;
    int64_t end = used < chunk + K7_CHUNK ? used : chunk + K7_CHUNK;
    const uint8_t* src = egress + (int64_t)u * ring_bytes;
    uint8_t* dst = staging + dst_off[u];
    for (int64_t pos = chunk + (int64_t)threadIdx.x * 16; pos < end;
         pos += (int64_t)blockDim.x * 16) {
        cdn_v4u v;
        memcpy(&v, src + pos, 16);
        *(cdn_v4u*)(dst + pos) = v;
    }
}

extern "C" void launch_k7_compact_rings(const uint8_t* egress, int64_t ring_bytes,
                                        const int64_t* wpos, const int64_t* dst_off,
                                        uint8_t* staging, int32_t n_rings,
                                        int32_t max_chunks, hipStream_t s) {
    if (n_rings <= 0 || max_chunks <= 0) return;
    hipLaunchKernelGGL(k7_compact_rings, dim3(n_rings, max_chunks), dim3(256), 0, s,
                       egress, ring_bytes, wpos, dst_off, staging);
}

// ---------------------------------------------------------------------------
// Peer-broker recipients.  The recipient index space is R = n_users + P:
// recipient n_users + p is the egress ring of peer slot p, which takes each
// message at most once per tick like a user subscribed to the peer's topics,
// so K2b / K3 / K7 serve it unchanged.  The two kernels below add the
// single-hop rule (reference to_users_only, broker/handler.rs:197-272): a
// message that ARRIVED from a peer broker (origin != 0) never reaches a peer
// ring.
// ---------------------------------------------------------------------------

// K2a with origin: k2a_topic_mask_t, except that a remote-origin message
// keeps only its local-user bits (topic_row_or applies user_bits_of_word).
extern "C" __global__ void k2a_topic_mask_origin_t(
    const uint64_t* __restrict__ sub_bitmap,  // [256][W], W = ceil(R/64)
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ topics_off,
    const int32_t* __restrict__ topics_cnt,
    const int32_t* __restrict__ disc,
    const int32_t* __restrict__ origin,       // [M] 0 = local user, else peer broker
    uint64_t* __restrict__ mask_t,            // [W][M]
    int32_t M, int32_t W, int32_t n_users)
{
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)M * W) return;
    int m = idx / W;
    int w = idx % W;
    mask_t[(int64_t)w * M + m] =
        topic_row_or<true>(sub_bitmap, buf, topics_off, topics_cnt, disc, m, w, W, origin,
                           n_users);
}

// K5b with peers: k5b_emit_direct's claim, plus owner <= -2 -> peer slot
// p = -owner-2.  A local-origin Direct to a key owned by peer p < P claims
// space in ring n_users + p; a remote-origin one, a slot >= P and the
// not-found value emit nothing and count no drop.  A non-negative owner
// outside [0, n_users) is not a user ring and emits nothing either.
extern "C" __global__ void k5b_emit_direct_peers(
    const int32_t* __restrict__ disc,
    const int32_t* __restrict__ owner,        // K5 output
    const int32_t* __restrict__ origin,       // [M]
    const int64_t* __restrict__ payload_off,
    const int32_t* __restrict__ payload_len,
    int32_t M, int32_t n_users, int32_t n_peers,
    int64_t ring_bytes, int32_t capacity,
    uint64_t* __restrict__ ring_wpos,         // [n_users + n_peers]
    int32_t* __restrict__ n_pairs,
    PairRec* __restrict__ pairs,
    uint32_t* __restrict__ drops)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    if (disc[i] != 3) return;
    const int32_t o = owner[i];
    int u;
    if (o >= 0) {
        if (o >= n_users) return;
        u = o;
    } else {
        // o <= -2 -> p >= 0; o == -1 -> p == -1; INT32_MIN -> p == 2^31 - 2
        const int64_t p = -(int64_t)o - 2;
        if (p < 0 || p >= (int64_t)n_peers || origin[i] != 0) return;
        u = n_users + (int)p;
    }
    k5b_claim_emit(u, i, payload_len[i], ring_bytes, capacity, ring_wpos, n_pairs, pairs,
                   drops);
}

// ---------------------------------------------------------------------------
// K6: batched incremental DirectMap updates.  One thread per update; the
// first n_up threads upsert {key, owner}, the next n_del delete {key}.
//   upsert: linear probe from key & mask with a 64-bit CAS(keys[slot], 0,
//           key); an old value of 0 (claimed now) or key (already present)
//           means the slot is this key's -> vals[slot] = owner.
//   delete: probe to the key and store vals[slot] = INT32_MIN (K5's
//           not-found value); the KEY STAYS.  Keys are never cleared, so
//           "no empty slot between a key's home and the key" holds under
//           concurrent inserts, and a re-upsert of a deleted key finds its
//           old slot again.
// Probing is bounded by table_size; an upsert that finds no slot bumps
// n_failed[0] (read by the host on the control path only).  Key 0 is the
// empty marker and is skipped.  Contract: the keys of one batch are
// distinct (the host deduplicates, last write wins).
// Between the key CAS and the value store a NEW slot holds its key with
// whatever value the slot had (0 = local user 0 in a fresh table), so every
// K5 reader must be ordered after this launch: K6 and the tick's K5 are
// issued on the same stream, and nothing may look the table up from another
// stream while a K6 launch is in flight.
// When two NEW keys race for one probe chain, which of them gets the
// earlier slot depends on CAS arrival order, so slot placement may differ
// from run to run; lookup results do not.
// ---------------------------------------------------------------------------
extern "C" __global__ void k6_direct_apply(
    uint64_t* __restrict__ table_keys,
    int32_t* __restrict__ table_vals,
    int64_t table_size,                      // power of two
    const uint64_t* __restrict__ up_keys,    // [n_up]
    const int32_t* __restrict__ up_owners,   // [n_up]
    int32_t n_up,
    const uint64_t* __restrict__ del_keys,   // [n_del]
    int32_t n_del,
    uint32_t* __restrict__ n_failed)         // [1]
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_up + n_del) return;
    const uint64_t mask = (uint64_t)table_size - 1;
    if (i < n_up) {
        const uint64_t key = up_keys[i];
        if (key == 0) return;
        const uint64_t s = key & mask;
        for (int64_t probe = 0; probe < table_size; ++probe) {
            const uint64_t slot = (s + probe) & mask;
            const unsigned long long old = atomicCAS(
                (unsigned long long*)&table_keys[slot], 0ull, (unsigned long long)key);
            if (old == 0ull || old == (unsigned long long)key) {
                table_vals[slot] = up_owners[i];
                return;
            }
        }
        atomicAdd(n_failed, 1u);
        return;
    }
    const uint64_t key = del_keys[i - n_up];
    if (key == 0) return;
    const uint64_t s = key & mask;
    for (int64_t probe = 0; probe < table_size; ++probe) {
        const uint64_t slot = (s + probe) & mask;
        const uint64_t k = __hip_atomic_load(&table_keys[slot], __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        if (k == key) { table_vals[slot] = INT32_MIN; return; }
        if (k == 0) return;   // absent: nothing to delete
    }
}

extern "C" {

void launch_k2a_topic_mask_origin_t(const uint64_t* sub_bitmap, const uint8_t* buf,
                                    const int64_t* topics_off, const int32_t* topics_cnt,
                                    const int32_t* disc, const int32_t* origin,
                                    uint64_t* mask_t, int32_t M, int32_t W, int32_t n_users,
                                    hipStream_t s) {
    if (M <= 0) return;
    hipLaunchKernelGGL(k2a_topic_mask_origin_t, k2a_grid(M, W), dim3(K2A_THREADS), 0, s,
                       sub_bitmap, buf, topics_off, topics_cnt, disc, origin, mask_t, M, W,
                       n_users);
}

void launch_k5b_emit_direct_peers(
    const int32_t* disc, const int32_t* owner, const int32_t* origin,
    const int64_t* payload_off, const int32_t* payload_len, int32_t M, int32_t n_users,
    int32_t n_peers, int64_t ring_bytes, int32_t capacity, uint64_t* ring_wpos,
    int32_t* n_pairs, PairRec* pairs, uint32_t* drops, hipStream_t s) {
    if (M <= 0) return;
    int threads = 256, blocks = (M + threads - 1) / threads;
    hipLaunchKernelGGL(k5b_emit_direct_peers, dim3(blocks), dim3(threads), 0, s, disc, owner,
                       origin, payload_off, payload_len, M, n_users, n_peers, ring_bytes,
                       capacity, ring_wpos, n_pairs, pairs, drops);
}

void launch_k6_direct_apply(uint64_t* table_keys, int32_t* table_vals, int64_t table_size,
                            const uint64_t* up_keys, const int32_t* up_owners, int32_t n_up,
                            const uint64_t* del_keys, int32_t n_del, uint32_t* n_failed,
                            hipStream_t s) {
    const int total = n_up + n_del;
    if (total <= 0) return;
    int threads = 256, blocks = (total + threads - 1) / threads;
    hipLaunchKernelGGL(k6_direct_apply, dim3(blocks), dim3(threads), 0, s, table_keys,
                       table_vals, table_size, up_keys, up_owners, n_up, del_keys, n_del,
                       n_failed);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Fused uniform broadcast tick.  The broadcast-only uniform shape (every
// message the same wire length, no Direct routing, no peer slots, no
// by-reference records) runs as ONE launcher call:
//
//   k_tick_prologue   K4 into scratch, the dense fan-out's record image, and
//                     the tick's two counters zeroed: all that reads only
//                     the batch
//   k_route_word      K2a, P1, P2 (same claims, cursors and drops) with the
//                     sort of each (user, 32-message block) TILE into dense
//                     or sparse, and P3's pair records for the sparse tiles
//                     only; one workgroup per mask word, tiles in LDS
//   k3_fanout_dense_tail_t  one launch of two kinds of workgroup:
//     K3d k3_dense_body    the dense tiles, from registers
//     K3  k3_flat_body     the sparse list (flat2, as on the per-op path)
//
// Two launches stand ahead of the dense fan-out because the step starts on
// an empty queue and every launch ahead of it is host time the GPU waits
// out (profiles/route_kernel_stats_before.txt: six launches of 2.5 - 9 us
// each started 8 - 9 us apart).  A batch above ROUTE_MAX_M messages routes
// by the chain the route kernel merges, with the tiles in scratch:
// k2a_topic_mask_t, k2b_p1_count_z (P1; zeroes the counters again),
// k2b_p2_tiles (P2 and the tile sort), k2b_p3_sparse.
//
// A tile is DENSE when its user takes every message of the block and all of
// them are delivered (they fit the ring and lie within pair capacity).  The
// bytes such a tile puts into the ring are the block's records back to back
// — the same bytes for every dense user — so the prologue builds the tick's
// record image once and K3d loads a chunk of it per workgroup and stores it
// to one user after another: one store instruction per KiB and nothing else
// in the loop, where the flat kernel spends a pair load, an offset load, a
// source load and a division per 16 bytes of every delivery.  No pair
// record is written for a dense tile; tdst[b][u] holds its ring address
// (-1: not dense).
//
// Every other tile's deliverable pairs go to the SPARSE list: pairs[0 ..
// *n_sparse), grouped by user with messages in order like P3's list, but
// without placeholders (an undeliverable pair is only counted, in P2).  A
// user's pairs start at usbase[u] + tslot[b][u]; P2 claims the spans with a
// second wave_claim_span, so P3 needs no atomics.  The list can never
// outgrow the pair buffer: a pair is deliverable only if its slot in P2's
// claim order is below capacity, so there are at most capacity of them.
// ---------------------------------------------------------------------------
extern "C" __global__ void k2b_p1_count_z(
    const uint64_t* __restrict__ mask_t, int32_t M, int32_t W, int32_t NB,
    int32_t* __restrict__ bcount, int32_t* __restrict__ n_pairs, int32_t* __restrict__ n_sparse)
{
    // read next by P2, a later launch on the same stream
    if (blockIdx.x == 0 && threadIdx.x == 0) { *n_pairs = 0; *n_sparse = 0; }
    k2b_p1_body(mask_t, M, W, NB, bcount);
}

// What the tile sort settles for one user (lane): how many records are
// delivered at most, the user's first sparse-list slot, and where its first
// record goes.
struct K2bTiles { int32_t lim; int32_t sbase; int64_t dst; };

// P2 and the tile sort, shared by k2b_p2_tiles and the route kernel: P2's
// claim, cursor advance and drop count (k2b_p2_body), then every tile of the
// user classified dense or sparse, tdst and tslot written, and the user's
// span of the sparse list claimed.  Every lane of the wave must call it.
// tdst is always the global [NB][W*64] array: the dense fan-out reads it.
template <class Cnt, class Pre, class Slot>
__device__ __forceinline__ K2bTiles k2b_tiles_body(
    const Cnt* __restrict__ bcount,        // tiles
    int u, bool active, int32_t stride, int col, int32_t M, int32_t W, int32_t NB,
    int64_t ring_bytes, int32_t capacity, int32_t uniform_rec, int32_t use_dense,
    uint64_t* __restrict__ ring_wpos,
    int32_t* __restrict__ n_pairs,
    int32_t* __restrict__ n_sparse,
    Pre* __restrict__ pprefix,             // tiles, out
    Slot* __restrict__ tslot,              // tiles, out
    int64_t* __restrict__ tdst,            // [NB][W*64] out
    uint32_t* __restrict__ drops)
{
    const K2bUser r = k2b_p2_body(bcount, u, active, stride, col, NB, ring_bytes, capacity,
                                  uniform_rec, ring_wpos, n_pairs, pprefix, drops);
    int cap_room = capacity - r.base; if (cap_room < 0) cap_room = 0;
    const int lim = r.fit < cap_room ? r.fit : cap_room;
    int n_sp = 0;
    if (active) {
        int p = 0;
        for (int b = 0; b < NB; ++b) {
            const int64_t i = (int64_t)b * stride + col;
            const int cnt = bcount[i];
            const int nm = min(M - b * K2B_BLK, K2B_BLK);
            const bool dense = use_dense && cnt == nm && p + cnt <= lim;
            tdst[(int64_t)b * (W * 64) + u] = dense ? r.dst + (int64_t)p * uniform_rec : -1;
            tslot[i] = (Slot)n_sp;
            if (!dense) n_sp += max(0, min(cnt, lim - p));
            p += cnt;
        }
    }
    return K2bTiles{lim, wave_claim_span(n_sp, n_sparse), r.dst};
}

extern "C" __global__ void k2b_p2_tiles(
    const int32_t* __restrict__ bcount,    // [NB][W*64]
    int32_t M, int32_t W, int32_t NB, int32_t n_users,
    int64_t ring_bytes, int32_t capacity, int32_t uniform_rec, int32_t use_dense,
    uint64_t* __restrict__ ring_wpos,
    int32_t* __restrict__ n_pairs,
    int32_t* __restrict__ n_sparse,
    int32_t* __restrict__ pprefix,         // [NB][W*64] out: per-block p-offset
    int32_t* __restrict__ tslot,           // [NB][W*64] out: sparse slot, relative to usbase
    int64_t* __restrict__ tdst,            // [NB][W*64] out: dense tile ring address, or -1
    int32_t* __restrict__ ulim,            // [W*64] out: records delivered at most
    int32_t* __restrict__ usbase,          // [W*64] out: first sparse-list slot
    int64_t* __restrict__ udst,            // [W*64] out: ring dst base
    uint32_t* __restrict__ drops)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = u < n_users;
    const K2bTiles r = k2b_tiles_body(bcount, u, active, W * 64, u, M, W, NB, ring_bytes, capacity,
                                      uniform_rec, use_dense, ring_wpos, n_pairs, n_sparse,
                                      pprefix, tslot, tdst, drops);
    if (active) {
        ulim[u] = r.lim;
        usbase[u] = r.sbase;
        udst[u] = r.dst;
    }
}

// One wave per (mask word, block), like P3.  Each lane first looks at its own
// user's tile; the wave then takes the sparse tiles one at a time with lanes
// spread over the block's MESSAGES, so a tile's pairs are stored side by
// side (ballot + popcount give the slot) and not one lane per user at a
// 4 KiB stride.  All tiles dense or empty: the wave leaves after the ballot.
// The body for the wave's (mask word w, block b), shared by k2b_p3_sparse and
// the route kernel.  The per-user arrays (ulim, usbase, udst) are indexed by
// `col` like the tiles; tdst is the global [NB][W*64] array.
template <class Cnt, class Pre, class Slot>
__device__ __forceinline__ void k2b_p3_sparse_body(
    const uint64_t* __restrict__ wcol,     // [M] mask words of word w
    const Cnt* __restrict__ bcount,
    const Pre* __restrict__ pprefix,
    const Slot* __restrict__ tslot,
    const int64_t* __restrict__ tdst,
    const int32_t* __restrict__ ulim,
    const int32_t* __restrict__ usbase,
    const int64_t* __restrict__ udst,
    int w, int b, int32_t stride, int col,
    int32_t M, int32_t W, int32_t n_users, int32_t uniform_rec,
    PairRec* __restrict__ pairs)
{
    const int lane = threadIdx.x & 63;
    const int u = w * 64 + lane;
    int p0 = 0, lim = 0, slot0 = 0;
    int64_t dstb = 0;
    bool sparse = false;
    if (u < n_users) {
        const int64_t i = (int64_t)b * stride + col;
        p0 = pprefix[i];
        lim = ulim[col];
        sparse = tdst[(int64_t)b * (W * 64) + u] < 0 && bcount[i] > 0 && p0 < lim;
        slot0 = usbase[col] + tslot[i];
        dstb = udst[col];
    }
    unsigned long long todo = __ballot(sparse);
    if (!todo) return;
    const int m0 = b * K2B_BLK, nm = min(M - m0, K2B_BLK);
    const uint64_t word = lane < nm ? wcol[m0 + lane] : 0ull;
    while (todo) {
        const int j = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int jp0 = __shfl(p0, j), jlim = __shfl(lim, j), jslot = __shfl(slot0, j);
        const int64_t jdst = ((int64_t)__shfl((int)(dstb >> 32), j) << 32)
                             | (uint32_t)__shfl((int)dstb, j);
        const bool bit = (word >> j) & 1ull;
        const unsigned long long mb = __ballot(bit);
        const int rank = __popcll(mb & ((1ull << lane) - 1ull));
        const int p = jp0 + rank;
        if (bit && p < jlim)
            store_pair(pairs + jslot + rank, w * 64 + j, m0 + lane,
                       jdst + (int64_t)p * uniform_rec);
    }
}

extern "C" __global__ void k2b_p3_sparse(
    const uint64_t* __restrict__ mask_t,   // [W][M]
    const int32_t* __restrict__ bcount,
    const int32_t* __restrict__ pprefix,
    const int32_t* __restrict__ tslot,
    const int64_t* __restrict__ tdst,
    const int32_t* __restrict__ ulim,
    const int32_t* __restrict__ usbase,
    const int64_t* __restrict__ udst,
    int32_t M, int32_t W, int32_t NB, int32_t n_users, int32_t uniform_rec,
    PairRec* __restrict__ pairs)
{
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave >= W * NB) return;
    const int w = wave / NB, b = wave - (wave / NB) * NB;
    k2b_p3_sparse_body(mask_t + (int64_t)w * M, bcount, pprefix, tslot, tdst, ulim, usbase, udst,
                       w, b, W * 64, w * 64 + (int)(threadIdx.x & 63), M, W, n_users,
                       uniform_rec, pairs);
}

// The route kernel: K2a, P1, P2 with the tile sort, and P3 for ONE mask word
// (64 users) per workgroup, in one launch.  Everything those four kernels
// hand each other depends on the user's own mask word only, so it stays in
// LDS (RouteLds, tick_geom.h) and the phases are separated by workgroup
// barriers where the chain has launch boundaries.  Across workgroups there
// are only the n_pairs / n_sparse / drops atomics, as in the chain.  P2 is
// one wave's work (a lane per user); the other phases are spread over the
// workgroup's waves.  The bodies are the chain's own.
extern "C" __global__ void __launch_bounds__(ROUTE_THREADS) k_route_word(
    const uint64_t* __restrict__ sub_bitmap,  // [256][W]
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ topics_off,
    const int32_t* __restrict__ topics_cnt,
    const int32_t* __restrict__ disc,
    int32_t M, int32_t W, int32_t NB, int32_t n_users,
    int64_t ring_bytes, int32_t capacity, int32_t uniform_rec, int32_t use_dense,
    uint64_t* __restrict__ ring_wpos,
    int32_t* __restrict__ n_pairs,
    int32_t* __restrict__ n_sparse,
    int64_t* __restrict__ tdst,               // [NB][W*64] out: dense tile ring address, or -1
    PairRec* __restrict__ pairs,
    uint32_t* __restrict__ drops)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t route_smem[];
    const RouteLds l = route_lds(M);
    uint64_t* wcol = (uint64_t*)(route_smem + l.mask);
    int64_t* udst = (int64_t*)(route_smem + l.udst);
    int32_t* ulim = (int32_t*)(route_smem + l.ulim);
    int32_t* usbase = (int32_t*)(route_smem + l.usbase);
    uint16_t* pprefix = (uint16_t*)(route_smem + l.pprefix);
    uint16_t* tslot = (uint16_t*)(route_smem + l.tslot);
    uint8_t* bcount = route_smem + l.bcount;

    const int w = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const int u = w * 64 + lane;

    // K2a
    for (int m = threadIdx.x; m < M; m += blockDim.x)
        wcol[m] = topic_row_or<false>(sub_bitmap, buf, topics_off, topics_cnt, disc, m, w, W,
                                      nullptr, 0);
    __syncthreads();
    // P1
    for (int b = wave; b < NB; b += n_waves)
        bcount[b * 64 + lane] = (uint8_t)k2b_tile_count(wcol, M, b);
    __syncthreads();
    // P2 and the tile sort: the whole of wave 0, inactive users included
    if (wave == 0) {
        const bool active = u < n_users;
        const K2bTiles r = k2b_tiles_body(bcount, u, active, 64, lane, M, W, NB, ring_bytes,
                                          capacity, uniform_rec, use_dense, ring_wpos, n_pairs,
                                          n_sparse, pprefix, tslot, tdst, drops);
        ulim[lane] = r.lim;
        usbase[lane] = r.sbase;
        udst[lane] = r.dst;
    }
    // also makes wave 0's tdst stores visible to the other waves' loads below
    __syncthreads();
    // P3
    for (int b = wave; b < NB; b += n_waves)
        k2b_p3_sparse_body(wcol, bcount, pprefix, tslot, tdst, ulim, usbase, udst, w, b, 64, lane,
                           M, W, n_users, uniform_rec, pairs);
}

// The record image: the M records of this tick, back to back at full stride,
// exactly the bytes the flat kernel stores for each of them — header
// {len, seq_base + m, 0, 0}, then payload_unit values.  One thread per unit,
// so a misaligned source or a partial tail is handled once per image unit
// and not once per delivery; K3d then only does aligned dword4 loads.
__device__ __forceinline__ void k3d_image_body(
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ offsets,   // [M+1]
    int32_t M, int32_t units_per_rec, uint32_t div_magic, int32_t div_shift,
    int32_t uniform_len, uint32_t seq_base,
    cdn_v4u* __restrict__ image,           // [M * units_per_rec]
    uint32_t i)
{
    if (i >= (uint32_t)(M * units_per_rec)) return;
    const int m = (int)(((uint64_t)i * div_magic) >> div_shift);
    const int q = (int)i - m * units_per_rec;
    image[i] = q == 0 ? cdn_v4u{(uint32_t)uniform_len, seq_base + (uint32_t)m, 0u, 0u}
                      : payload_unit(buf + offsets[m], (q - 1) * 16, uniform_len);
}

// The prologue: everything of the tick that reads only the batch itself, in
// one launch.  The first parse_blocks workgroups parse (K4, a thread per
// message), the rest build the record image (a thread per unit; none when
// the dense fan-out is off), and the first thread zeroes the tick's two
// counters, which the route kernel, the next launch, claims from.
extern "C" __global__ void __launch_bounds__(256) k_tick_prologue(
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ offsets,   // [M+1]
    int32_t M, uint64_t hash_seed, ParseOut out, int32_t parse_blocks,
    int32_t units_per_rec, uint32_t div_magic, int32_t div_shift,
    int32_t uniform_len, uint32_t seq_base,
    cdn_v4u* __restrict__ image,
    int32_t* __restrict__ n_pairs, int32_t* __restrict__ n_sparse)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) { *n_pairs = 0; *n_sparse = 0; }
    if ((int32_t)blockIdx.x < parse_blocks)
        k4_parse_body(buf, offsets, M, hash_seed, out, blockIdx.x * blockDim.x + threadIdx.x);
    else
        k3d_image_body(buf, offsets, M, units_per_rec, div_magic, div_shift, uniform_len, seq_base,
                       image, (blockIdx.x - parse_blocks) * blockDim.x + threadIdx.x);
}

// K3d.  blockIdx.x = (group * NB + block) * n_chunks + chunk: a workgroup
// loads units [chunk * chunk_units, + chunk_units) of the block's part of the
// image (dense_geom) into registers and then walks `group` consecutive
// users, storing the chunk to each dense one.  The user index, the density
// test and the address are wave-uniform.  Neighbouring workgroups write
// neighbouring spans of the same users' rings.  Stores are plain at either
// nt_fanout setting: on the bench's layout this shape measured 510 us plain
// against 540 us non-temporal (profiles/k3_write_shapes.txt), the opposite
// of the flat kernel.
__device__ __forceinline__ void k3_dense_body(
    const cdn_v4u* __restrict__ image,     // [M * units_per_rec]
    const int64_t* __restrict__ tdst,      // [NB][users64]
    int32_t M, int32_t NB, int32_t users64, int32_t n_users, int32_t units_per_rec,
    int32_t n_chunks, int32_t chunk_units, int32_t group,
    uint8_t* __restrict__ egress, uint32_t block)
{
    const int per_group = NB * n_chunks;
    const int g = block / per_group, bc = block - g * per_group;
    const int b = bc / n_chunks, c = bc - b * n_chunks;
    const int m0 = b * K2B_BLK, nm = min(M - m0, K2B_BLK);
    const int lo = c * chunk_units + (int)threadIdx.x;
    const int hi = min(nm * units_per_rec, (c + 1) * chunk_units);
    if (lo >= hi) return;
    const cdn_v4u* __restrict__ img = image + (size_t)m0 * units_per_rec;
    cdn_v4u v[DENSE_MAX_V];
    #pragma unroll
    for (int k = 0; k < DENSE_MAX_V; ++k) {
        const int unit = lo + k * DENSE_THREADS;
        v[k] = unit < hi ? img[unit] : cdn_v4u{0u, 0u, 0u, 0u};
    }
    const int64_t* __restrict__ trow = tdst + (int64_t)b * users64;
    const int u1 = min(n_users, (g + 1) * group);
    for (int u = g * group; u < u1; ++u) {
        const int64_t d = trow[u];
        if (d < 0) continue;
        uint8_t* dst = egress + d + (size_t)lo * 16;
        #pragma unroll
        for (int k = 0; k < DENSE_MAX_V; ++k)
            if (lo + k * DENSE_THREADS < hi)
                store16<0>(dst + (size_t)k * (DENSE_THREADS * 16), v[k]);
    }
}

// The fused tick's one fan-out launch.  Workgroups [0, dense_blocks) are K3d;
// the SPARSE_TAIL_BLOCKS behind them are the flat K3 over the sparse list
// (pairs[0 .. *n_sparse), offsets as payload_off, the length a scalar), with
// the stores NT chooses.  The two halves write disjoint ring spans, both
// handed out by the routing launch before this one, so nothing orders them
// and no workgroup waits for another.  The tail is dispatched behind the
// dense workgroups: with an empty list it reads the count and is gone while
// the last of them still store, where a launch of its own stood between the
// fan-out and the drain.
static_assert(DENSE_THREADS == 256, "the tail runs the flat body, 256 threads per workgroup");
template <int NT>
__global__ void __launch_bounds__(DENSE_THREADS) k3_fanout_dense_tail_t(
    const cdn_v4u* __restrict__ image,
    const int64_t* __restrict__ tdst,
    int32_t M, int32_t NB, int32_t users64, int32_t n_users, int32_t units_per_rec,
    int32_t n_chunks, int32_t chunk_units, int32_t group, uint32_t dense_blocks,
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ offsets,
    const int32_t* __restrict__ payload_len,
    const PairRec* __restrict__ pairs,
    uint32_t seq_base,
    const int32_t* __restrict__ n_sparse,
    int32_t capacity, uint32_t div_magic, int32_t div_shift, int32_t uniform_len,
    uint8_t* __restrict__ egress)
{
    if (blockIdx.x < dense_blocks)
        k3_dense_body(image, tdst, M, NB, users64, n_users, units_per_rec, n_chunks, chunk_units,
                      group, egress, blockIdx.x);
    else
        k3_flat_body<NT>(buf, offsets, payload_len, pairs, seq_base, n_sparse, capacity,
                         units_per_rec, div_magic, div_shift, uniform_len, egress,
                         blockIdx.x - dense_blocks, gridDim.x - dense_blocks);
}

// `out` is the device-visible address of the engine's pinned host buffer, or
// a device staging buffer where the host buffer has none.
extern "C" __global__ void k_drain_cursors(int64_t* __restrict__ ring_wpos,
                                           int64_t* __restrict__ out, int32_t n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = ring_wpos[i];
    ring_wpos[i] = 0;
}

extern "C" {

void launch_tick_uniform_broadcast(const UniformTick* t, hipStream_t s) {
    const int32_t M = t->M, W = t->W;
    if (M <= 0) return;
    const int32_t NB = (int32_t)k2b_blocks(M);
    const int64_t U = (int64_t)W * 64, T = (int64_t)NB * U;
    // carve the scratch (sizes: uniform_tick_scratch64 / 32 in dataplane.h)
    const int32_t units = t->rec / 16;
    int64_t* p64 = t->scratch64;
    cdn_v4u* image = (cdn_v4u*)p64;  p64 += 2 * (int64_t)M * units;  // first: 16-aligned
    int64_t* payload_off = p64;  p64 += M;
    int64_t* topics_off = p64;   p64 += M;
    int64_t* recip_hash = p64;   p64 += M;
    int64_t* timestamp = p64;    p64 += M;
    uint64_t* mask_t = (uint64_t*)p64;  p64 += (int64_t)W * M;
    int64_t* tdst = p64;         p64 += T;
    int64_t* udst = p64;
    int32_t* p32 = t->scratch32;
    int32_t* disc = p32;         p32 += M;
    int32_t* payload_len = p32;  p32 += M;
    int32_t* topics_cnt = p32;   p32 += M;
    int32_t* bcount = p32;       p32 += T;
    int32_t* pprefix = p32;      p32 += T;
    int32_t* tslot = p32;        p32 += T;
    int32_t* ulim = p32;         p32 += U;
    int32_t* usbase = p32;

    // 1. the prologue: parse, record image, counters zeroed
    const int threads = 256;
    const int parse_blocks = (M + threads - 1) / threads;
    const int image_blocks = t->dense ? (M * units + threads - 1) / threads : 0;
    uint32_t dm; int32_t dsh;
    u32_div_magic(units, &dm, &dsh);
    hipLaunchKernelGGL(k_tick_prologue, dim3(parse_blocks + image_blocks), dim3(threads), 0, s,
                       t->buf, t->offsets, M, t->hash_seed,
                       ParseOut{disc, payload_off, payload_len, topics_off, topics_cnt,
                                (uint64_t*)recip_hash, (uint64_t*)timestamp},
                       parse_blocks, units, dm, dsh, t->uniform_len, t->seq_base, image,
                       t->n_pairs, t->n_sparse);

    // 2. routing: one launch, or for a batch whose mask column does not fit
    // a workgroup's LDS the chain of four through scratch
    if (M <= ROUTE_MAX_M) {
        hipLaunchKernelGGL(k_route_word, dim3(W), dim3(ROUTE_THREADS), route_lds(M).bytes, s,
                           t->sub_bitmap, t->buf, topics_off, topics_cnt, disc, M, W, NB,
                           t->n_users, t->ring_bytes, t->capacity, t->rec, t->dense ? 1 : 0,
                           t->ring_wpos, t->n_pairs, t->n_sparse, tdst, t->pairs, t->drops);
    } else {
        launch_k2a_topic_mask_t(t->sub_bitmap, t->buf, topics_off, topics_cnt, disc, mask_t, M, W,
                                s);
        const int blocks_wb = (W * NB * 64 + threads - 1) / threads;
        const int blocks_u = (t->n_users + threads - 1) / threads;
        // zeroes the two counters once more, still ahead of P2's first claim
        hipLaunchKernelGGL(k2b_p1_count_z, dim3(blocks_wb), dim3(threads), 0, s, mask_t, M, W, NB,
                           bcount, t->n_pairs, t->n_sparse);
        hipLaunchKernelGGL(k2b_p2_tiles, dim3(blocks_u), dim3(threads), 0, s, bcount, M, W, NB,
                           t->n_users, t->ring_bytes, t->capacity, t->rec, t->dense ? 1 : 0,
                           t->ring_wpos, t->n_pairs, t->n_sparse, pprefix, tslot, tdst, ulim,
                           usbase, udst, t->drops);
        hipLaunchKernelGGL(k2b_p3_sparse, dim3(blocks_wb), dim3(threads), 0, s, mask_t, bcount,
                           pprefix, tslot, tdst, ulim, usbase, udst, M, W, NB, t->n_users, t->rec,
                           t->pairs);
    }

    // 3. the fan-out: one launch, the sparse list behind the dense tiles; the
    // flat kernel alone with the dense fan-out off.  offsets is payload_off
    // (fanout_wire), the length a scalar.
    if (t->dense) {
        const DenseGeom geo = dense_geom(units);
        const uint32_t dense_blocks =
            (uint32_t)(dense_grid_x(t->n_users, DENSE_GROUP, geo.n_chunks) * NB);
        DISPATCH_NT(t->nt, hipLaunchKernelGGL(
            (k3_fanout_dense_tail_t<NT>), dim3(dense_blocks + SPARSE_TAIL_BLOCKS),
            dim3(DENSE_THREADS), 0, s, image, tdst, M, NB, (int32_t)U, t->n_users, units,
            geo.n_chunks, geo.chunk_units, DENSE_GROUP, dense_blocks, t->buf, t->offsets,
            payload_len, t->pairs, t->seq_base, t->n_sparse, t->capacity, dm, dsh,
            t->uniform_len, t->egress));
    } else {
        launch_flat<false>(t->buf, t->offsets, payload_len, t->pairs, t->seq_base, nullptr,
                           t->n_sparse, t->capacity, units, t->uniform_len, t->egress, t->nt, 0,
                           s);
    }
}

void launch_drain_cursors(int64_t* ring_wpos, int64_t* out, int32_t n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_drain_cursors, dim3((n + 255) / 256), dim3(256), 0, s, ring_wpos, out,
                       n);
}

}  // extern "C"
