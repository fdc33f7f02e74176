// Host-side geometry of the fused uniform broadcast tick
// (launch_tick_uniform_broadcast, csrc/hip/dataplane.hip): block size, dense
// fan-out chunking and scratch sizes.  Plain C++ with no HIP dependency, so
// csrc/tests/test_native.cpp checks it on the CPU.
#pragma once

#include <stdint.h>

// Messages per K2b block (one tile = one user x one block of messages).
#define K2B_BLK 32

// The dense fan-out works on the concatenated image of a block's records in
// chunks of at most DENSE_THREADS * DENSE_MAX_V 16-byte units (32 KiB, eight
// dword4 registers per thread), whatever the record size.  A full block's
// image is split into the fewest such chunks, of equal size rounded up to a
// whole wave, so every chunk's workgroup stores about the same amount.
#define DENSE_THREADS 256
#define DENSE_MAX_V 8
// Users per dense fan-out workgroup: 8, 16 and 32 measured within 1% of each
// other (profiles/k3_write_shapes.txt); 8 leaves the most workgroups to
// balance.
#define DENSE_GROUP 8
struct DenseGeom { int32_t n_chunks; int32_t chunk_units; };
static inline DenseGeom dense_geom(int32_t units_per_rec) {
    const int32_t cap = DENSE_THREADS * DENSE_MAX_V;
    const int32_t image = units_per_rec * K2B_BLK;
    DenseGeom g;
    g.n_chunks = (image + cap - 1) / cap;
    g.chunk_units = ((image + g.n_chunks - 1) / g.n_chunks + 63) & ~63;
    return g;
}
// Workgroups per message block: one per (group of `group` users, chunk);
// the launch has that many for each of the tick's blocks.
static inline int64_t dense_grid_x(int32_t n_users, int32_t group, int32_t n_chunks) {
    return ((int64_t)n_users + group - 1) / group * n_chunks;
}

// Elements of the two scratch tensors the fused tick carves its per-tick
// arrays from, for a batch of M messages and W mask words (NB = blocks of
// K2B_BLK messages, U = W * 64 user slots):
//   64-bit: the dense fan-out's record image first (M records of
//           units_per_rec 16-byte units; the tensor must be 16-byte aligned),
//           payload_off, topics_off, recip_hash, timestamp [M] each,
//           mask_t [W][M], tdst [NB][U], udst [U]
//   32-bit: disc, payload_len, topics_cnt [M] each, bcount, pprefix,
//           tslot [NB][U] each, ulim, usbase [U] each
static inline int64_t k2b_blocks(int64_t M) { return (M + K2B_BLK - 1) / K2B_BLK; }
static inline int64_t uniform_tick_scratch64(int64_t M, int64_t W, int64_t units_per_rec) {
    return 4 * M + W * M + k2b_blocks(M) * W * 64 + W * 64 + 2 * M * units_per_rec;
}
static inline int64_t uniform_tick_scratch32(int64_t M, int64_t W) {
    return 3 * M + 3 * k2b_blocks(M) * W * 64 + 2 * W * 64;
}
