// Host-visible interface of csrc/hip/dataplane.hip: the structs that cross
// the launcher boundary and the prototype of every data-plane launcher.
// Plain C++ — csrc/gpu_bindings.cpp (host-only) and dataplane.hip both include
// it, so the compiler checks each definition against the prototype its
// caller sees.  The launchers have C linkage: without this header a
// prototype that drifted from its definition would still link and pass
// arguments in the wrong slots.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../common/tick_geom.h"

// A delivery pair as ONE 16-byte record {user, msg, ring dst}: emitters do a
// single dword4 store per pair and K3 a single dword4 load per unit.  The
// SoA layout (three arrays) cost ~3x scattered sub-line stores per pair —
// measured 100 us/tick in k2b_p3_emit at 2.56M pairs before this change.
// user < 0 marks a dropped delivery (ring full); K3 skips it.
struct alignas(16) PairRec { int32_t user; int32_t msg; int64_t dst; };
static_assert(sizeof(PairRec) == 16, "PairRec must be one dword4");

// K4 outputs, one element per message (see k4_parse_batch).
struct ParseOut {
    int32_t* disc;
    int64_t* payload_off;
    int32_t* payload_len;
    int64_t* topics_off;
    int32_t* topics_cnt;
    uint64_t* recip_hash;
    uint64_t* timestamp;
};

// Everything one fused uniform broadcast tick needs.  All pointers are
// device memory owned by the caller; the launcher allocates nothing and
// never synchronises.
struct UniformTick {
    const uint8_t* buf;          // the ingested batch
    const int64_t* offsets;      // [M+1] message starts (also K3's payload_off)
    int32_t M;
    uint64_t hash_seed;
    const uint64_t* sub_bitmap;  // [256][W]
    int32_t W;
    int32_t n_users;
    int64_t ring_bytes;
    int32_t capacity;            // rows of pairs
    int32_t uniform_len;         // wire bytes of every message
    int32_t rec;                 // ring_rec(uniform_len)
    uint32_t seq_base;
    uint64_t* ring_wpos;         // [n_users]
    int32_t* n_pairs;            // [1] pair slots claimed (zeroed by the tick)
    int32_t* n_sparse;           // [1] pairs in the sparse list (zeroed by the tick)
    PairRec* pairs;              // the sparse list
    uint32_t* drops;
    int64_t* scratch64;          // uniform_tick_scratch64(M, W, rec / 16) elements
    int32_t* scratch32;          // uniform_tick_scratch32(M, W) elements
    uint8_t* egress;
    int nt;                      // non-temporal egress stores (flat fan-out)
    int dense;                   // != 0: dense tiles go to the dense fan-out
};

extern "C" {

void launch_k4_parse(const uint8_t* buf, const int64_t* offsets, int32_t M, uint64_t hash_seed,
                     ParseOut out, hipStream_t s);

// K2a: mask is [M][W]; mask_t is [W][M]
void launch_k2a_topic_mask(const uint64_t* sub_bitmap, const uint8_t* buf,
                           const int64_t* topics_off, const int32_t* topics_cnt,
                           const int32_t* disc, uint64_t* mask, int32_t M, int32_t W,
                           hipStream_t s);
void launch_k2a_topic_mask_t(const uint64_t* sub_bitmap, const uint8_t* buf,
                             const int64_t* topics_off, const int32_t* topics_cnt,
                             const int32_t* disc, uint64_t* mask_t, int32_t M, int32_t W,
                             hipStream_t s);
void launch_k2a_topic_mask_origin_t(const uint64_t* sub_bitmap, const uint8_t* buf,
                                    const int64_t* topics_off, const int32_t* topics_cnt,
                                    const int32_t* disc, const int32_t* origin,
                                    uint64_t* mask_t, int32_t M, int32_t W, int32_t n_users,
                                    hipStream_t s);
void launch_k2c_apply_subs(uint64_t* sub_bitmap, const uint8_t* buf, const int64_t* topics_off,
                           const int32_t* topics_cnt, const int32_t* disc,
                           const int32_t* user_idx, int32_t M, int32_t W, hipStream_t s);

// K2b
void launch_k2b_count(const uint64_t* mask, int32_t M, int32_t W, int32_t n_users,
                      int32_t* counts, hipStream_t s);
void launch_k2b_emit(const uint64_t* mask, const int64_t* payload_off,
                     const int32_t* payload_len, const int32_t* pair_base, int32_t M, int32_t W,
                     int32_t n_users, int64_t ring_bytes, uint64_t* ring_wpos, PairRec* pairs,
                     uint32_t* drops, hipStream_t s);
void launch_k2b_fused_t(const uint64_t* mask_t, const int32_t* payload_len, int32_t M,
                        int32_t W, int32_t n_users, int64_t ring_bytes, int32_t capacity,
                        int32_t uniform_rec, uint64_t* ring_wpos, int32_t* n_pairs,
                        PairRec* pairs, uint32_t* drops, hipStream_t s);
void launch_k2b_blocks_t(const uint64_t* mask_t, int32_t M, int32_t W, int32_t n_users,
                         int64_t ring_bytes, int32_t capacity, int32_t uniform_rec,
                         uint64_t* ring_wpos, int32_t* n_pairs, int32_t* bcount,
                         int32_t* pprefix, int32_t* ubase, int32_t* ufit, int64_t* udst,
                         PairRec* pairs, uint32_t* drops, hipStream_t s);

// K3: nt != 0 selects non-temporal egress stores; grid <= 0 the default grid
void launch_k3_fanout(const uint8_t* buf, const int64_t* payload_off,
                      const int32_t* payload_len, const PairRec* pairs, const uint32_t* msg_seq,
                      int32_t n_pairs, uint8_t* egress, hipStream_t s);
void launch_k3_fanout_wave(const uint8_t* buf, const int64_t* payload_off,
                           const int32_t* payload_len, const PairRec* pairs,
                           const uint32_t* msg_seq, const int32_t* n_pairs_ptr,
                           int32_t capacity, uint8_t* egress, int nt, int grid, hipStream_t s);
void launch_k3_fanout_ref(const uint8_t* buf, const int64_t* payload_off,
                          const int32_t* payload_len, const PairRec* pairs,
                          const uint32_t* msg_seq, const int32_t* n_pairs_ptr,
                          int32_t capacity, int32_t ref_threshold, int64_t ref_base,
                          uint8_t* egress, int nt, int grid, hipStream_t s);
void launch_k3_fanout_flat2(const uint8_t* buf, const int64_t* payload_off,
                            const int32_t* payload_len, const PairRec* pairs,
                            uint32_t seq_base, const int32_t* n_pairs_ptr, int32_t capacity,
                            int32_t units_per_pair, int32_t uniform_len, uint8_t* egress,
                            int nt, int grid, hipStream_t s);
void launch_k3_fanout_flat3(const uint8_t* buf, const int64_t* payload_off,
                            const int32_t* payload_len, const PairRec* pairs,
                            const uint32_t* seq_state, const int32_t* n_pairs_ptr,
                            int32_t capacity, int32_t units_per_pair, int32_t uniform_len,
                            uint8_t* egress, int nt, int grid, hipStream_t s);
void launch_k_seq_advance(uint32_t* seq_state, int32_t m, hipStream_t s);

// K5 / K5b / K6
void launch_k5_direct_lookup(const uint64_t* table_keys, const int32_t* table_vals,
                             int64_t table_size, const uint64_t* query, int32_t N,
                             int32_t* owner, hipStream_t s);
void launch_k5b_emit_direct(const int32_t* disc, const int32_t* owner,
                            const int64_t* payload_off, const int32_t* payload_len, int32_t M,
                            int64_t ring_bytes, int32_t capacity, uint64_t* ring_wpos,
                            int32_t* n_pairs, PairRec* pairs, uint32_t* drops, hipStream_t s);
void launch_k5b_emit_direct_peers(const int32_t* disc, const int32_t* owner,
                                  const int32_t* origin, const int64_t* payload_off,
                                  const int32_t* payload_len, int32_t M, int32_t n_users,
                                  int32_t n_peers, int64_t ring_bytes, int32_t capacity,
                                  uint64_t* ring_wpos, int32_t* n_pairs, PairRec* pairs,
                                  uint32_t* drops, hipStream_t s);
void launch_k6_direct_apply(uint64_t* table_keys, int32_t* table_vals, int64_t table_size,
                            const uint64_t* up_keys, const int32_t* up_owners, int32_t n_up,
                            const uint64_t* del_keys, int32_t n_del, uint32_t* n_failed,
                            hipStream_t s);

// Fused uniform broadcast tick: K4, K2a, K2b (tiles), the dense fan-out and
// the flat fan-out over the sparse list (one launch for the two), back to back
// on one stream.
void launch_tick_uniform_broadcast(const UniformTick* t, hipStream_t s);

// Drain: out[i] = ring_wpos[i]; ring_wpos[i] = 0.  `out` is any address the
// device can store to: a device buffer or the device view of pinned host memory.
void launch_drain_cursors(int64_t* ring_wpos, int64_t* out, int32_t n, hipStream_t s);

// K7
void launch_k7_compact_rings(const uint8_t* egress, int64_t ring_bytes, const int64_t* wpos,
                             const int64_t* dst_off, uint8_t* staging, int32_t n_rings,
                             int32_t max_chunks, hipStream_t s);

}  // extern "C"
