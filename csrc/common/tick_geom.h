// Host-side geometry of the fused uniform broadcast tick
// (launch_tick_uniform_broadcast, csrc/hip/dataplane.hip): block size, dense
// fan-out chunking, scratch sizes and the route kernel's LDS layout.  Plain
// C++ with no HIP dependency, so csrc/tests/test_native.cpp checks it on the
// CPU.
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

// Flat fan-out workgroups (256 threads each) that follow the dense ones in the
// fused tick's fan-out launch and walk the sparse list.  16,384 is the grid
// swept for the flat kernel where the list carries the whole fan-out
// (16384 > 8192 > 4096, about 0.5% each), which a population with no dense
// tile still is.
#define SPARSE_TAIL_BLOCKS 16384

// Elements of the two scratch tensors the fused tick carves its per-tick
// arrays from, for a batch of M messages and W mask words (NB = blocks of
// K2B_BLK messages, U = W * 64 user slots):
//   64-bit: the dense fan-out's record image first (M records of
//           units_per_rec 16-byte units; the tensor must be 16-byte aligned),
//           payload_off, topics_off, recip_hash, timestamp [M] each,
//           mask_t [W][M], tdst [NB][U], udst [U]
//   32-bit: disc, payload_len, topics_cnt [M] each, bcount, pprefix,
//           tslot [NB][U] each, ulim, usbase [U] each
// mask_t, udst and the 32-bit tile and user arrays are touched only by a
// batch above ROUTE_MAX_M (below); the sizes and the carve order do not
// depend on that.
static inline int64_t k2b_blocks(int64_t M) { return (M + K2B_BLK - 1) / K2B_BLK; }
static inline int64_t uniform_tick_scratch64(int64_t M, int64_t W, int64_t units_per_rec) {
    return 4 * M + W * M + k2b_blocks(M) * W * 64 + W * 64 + 2 * M * units_per_rec;
}
static inline int64_t uniform_tick_scratch32(int64_t M, int64_t W) {
    return 3 * M + 3 * k2b_blocks(M) * W * 64 + 2 * W * 64;
}

// The route kernel (k_route_word) runs K2a, P1, P2 and P3 for one mask word,
// 64 users, in one workgroup and keeps what those kernels hand each other in
// LDS.  Byte offsets of its arrays for a batch of M messages (NB blocks),
// widest element first so each is aligned to its own type:
//   mask    uint64 [M]        the word of every message's recipient mask
//   udst    int64  [64]       ring address of the user's first record
//   ulim    int32  [64]       records delivered at most
//   usbase  int32  [64]       first sparse-list slot
//   pprefix uint16 [NB][64]   deliveries before the block (<= M - 1)
//   tslot   uint16 [NB][64]   sparse slot relative to usbase (<= M - 1)
//   bcount  uint8  [NB][64]   set bits of the tile (<= K2B_BLK)
// tdst is not here: the dense fan-out, a later launch, reads it from scratch.
#define ROUTE_THREADS 256
struct RouteLds { int32_t mask, udst, ulim, usbase, pprefix, tslot, bcount, bytes; };
constexpr RouteLds route_lds(int32_t M) {
    const int32_t tiles = (M + K2B_BLK - 1) / K2B_BLK * 64;
    RouteLds l{};
    l.mask = 0;
    l.udst = l.mask + 8 * M;
    l.ulim = l.udst + 8 * 64;
    l.usbase = l.ulim + 4 * 64;
    l.pprefix = l.usbase + 4 * 64;
    l.tslot = l.pprefix + 2 * tiles;
    l.bcount = l.tslot + 2 * tiles;
    l.bytes = l.bcount + tiles;
    return l;
}
// Largest batch the route kernel takes; a larger one runs the four kernels.
// 18 bytes per message and 1 KiB per workgroup: 3,584 messages fill 64 KiB.
#define ROUTE_MAX_M 3584
static_assert(route_lds(ROUTE_MAX_M).bytes <= 64 * 1024, "route kernel LDS exceeds a workgroup's 64 KiB");
static_assert(route_lds(ROUTE_MAX_M + 1).bytes > 64 * 1024, "ROUTE_MAX_M is not the largest batch that fits");
static_assert(ROUTE_MAX_M >= 2048, "the 8-GPU bench routes 8 x 256 gathered messages per tick");
static_assert(ROUTE_MAX_M <= 65535 && K2B_BLK <= 255, "prefixes are 16-bit, tile counts 8-bit");
static_assert(route_lds(33).udst % 8 == 0 && route_lds(33).ulim % 4 == 0 && route_lds(33).pprefix % 2 == 0,
              "route kernel LDS arrays are aligned to their element types");
