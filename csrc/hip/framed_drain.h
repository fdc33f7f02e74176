// Host-visible interface of csrc/hip/framed_drain.hip: the framed drain (K11),
// which turns every egress ring's records into socket-ready
// [u32 big-endian length][wire message] frames in arrival order.  Plain C++ —
// csrc/gpu_drain_bindings.cpp (host-only) and framed_drain.hip both include
// it, so the compiler checks the definition against the prototype its caller
// sees.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

// Most records of an out-of-order ring that K11 still sorts (in LDS, 8 B per
// record).  A ring that is out of order AND holds more is handed over raw
// ("ring mode", frame_cnt = -1); an in-order ring is framed at any count.
#define FRAME_SORT_MAX 4096

// Threads of a k11_ring_index workgroup (wave 0 walks, all of them sort) and
// of a k11_frame_copy workgroup (one record per wave at a time).
#define K11_THREADS 256

// A k11_frame_copy workgroup serves the frames that START in one chunk of this
// many bytes of its recipient's framed output (or, in ring mode, that chunk
// of the raw ring prefix).
#define K11_CHUNK (16 * 1024)

// Limits a ring record must respect to be framed: the by-reference flag in
// its len word, and the wire framing limit (proto/transports/base.py
// MAX_MESSAGE_SIZE, csrc/net/pump.h kMaxMessageSize).
#define K11_REF_FLAG 0x80000000u
#define K11_MAX_MESSAGE_SIZE (0xFFFFFFFFu / 8)

// One entry of the index k11_ring_index leaves for k11_frame_copy, in OUTPUT
// order: the record's header position in its ring, its body length, its seq
// (the sort key is seq minus the ring's circular-minimum seq) and where its
// frame starts in the recipient's region.
struct alignas(16) FrameIdx { uint32_t ring_pos, len, seq, frame_off; };
static_assert(sizeof(FrameIdx) == 16, "FrameIdx must be one dword4");

extern "C" {

// K11: for every ring r < n_rings with used = min(max(wpos[r], 0), ring_bytes)
// bytes, write into staging[dst_off[r], dst_off[r] + used) either frame_cnt[r]
// frames of frame_len[r] <= used bytes in all, or (frame_cnt[r] = -1,
// frame_len[r] = used) the raw ring prefix.  A ring whose region leaves
// [0, staging_bytes) is treated as empty.  index has room for
// staging_bytes / 16 entries.  wpos is only read.  Two launches; the copy's
// grid is n_rings x max_chunks, max_chunks >= ceil(max used / K11_CHUNK).
// Needs ring_bytes a multiple of 16 and at most 65535 * K11_CHUNK (the grid).
void launch_k11_frame_rings(const uint8_t* egress, int64_t ring_bytes, const int64_t* wpos,
                            const int64_t* dst_off, uint8_t* staging, int64_t staging_bytes,
                            int64_t* frame_len, int32_t* frame_cnt, FrameIdx* index,
                            int32_t n_rings, int32_t max_chunks, hipStream_t s);

}  // extern "C"
