"""The egress ring's delivery record format, shared by the engine, the
reference models and everything that reads a drained ring.

A record is {u32 len, u32 seq, u64 pad} + payload, 16-byte aligned.  A
by-reference record is the bare 16-byte header {u32 len | REF_FLAG, u32 seq,
u64 ref_off}: its bytes stay in the host batch that ref_off indexes.
"""

from __future__ import annotations

from typing import List, Tuple

RING_ALIGN = 16
REF_FLAG = 0x80000000  # top bit of a record's len word: by-reference record
# The framed drain sorts an out-of-order ring of at most this many records;
# one with more comes back raw.  Host mirror of csrc/hip/framed_drain.h.
FRAME_SORT_MAX = 4096


def ring_rec(length: int) -> int:
    """Egress ring record stride: 16 B header + payload padded to 16 B
    (uint4-aligned record starts).  Host mirror of csrc/hip/dataplane.hip
    ring_rec; K3 zero-pads the tail unit so each record is written with
    full vector stores."""
    return (length + 16 + (RING_ALIGN - 1)) & ~(RING_ALIGN - 1)


def parse_ring_records(ring: bytes, wpos: int, refbuf=None) -> List[Tuple[int, bytes]]:
    """Parse delivery records out of a drained ring, ordered by sequence
    number: [(seq, payload), ...].

    A by-reference record (REF_FLAG set in its len word, no payload in the
    ring) resolves to refbuf[ref_off : ref_off + len]; without a refbuf, or
    with a range outside it, it raises ValueError.

    Ring WRITE order is claim order: broadcasts are per-user ordered by
    K2b, but K5b's direct-delivery claims are atomic and may interleave
    out of order within a tick — the seq header restores the global
    per-tick arrival order (stronger than the reference's per-connection
    FIFO, sender.rs).  The sort is wrap-aware relative to the batch's
    lowest seq."""
    out = []
    pos = 0
    while pos + 16 <= wpos:
        length = int.from_bytes(ring[pos : pos + 4], "little")
        seq = int.from_bytes(ring[pos + 4 : pos + 8], "little")
        if length & REF_FLAG:
            length &= REF_FLAG - 1
            ref_off = int.from_bytes(ring[pos + 8 : pos + 16], "little")
            if refbuf is None:
                raise ValueError("by-reference record without a reference buffer")
            if ref_off + length > len(refbuf):
                raise ValueError(
                    f"by-reference record [{ref_off}, {ref_off + length}) outside "
                    f"the {len(refbuf)}-byte reference buffer")
            out.append((seq, bytes(refbuf[ref_off : ref_off + length])))
            pos += RING_ALIGN
            continue
        payload = ring[pos + 16 : pos + 16 + length]
        out.append((seq, payload))
        pos += ring_rec(length)
    if len(out) > 1:
        # circular minimum (handles u32 seq wrap mid-batch)
        base = out[0][0]
        for s_, _ in out:
            if (s_ - base) & 0xFFFFFFFF > 0x80000000:
                base = s_
        out.sort(key=lambda r: (r[0] - base) & 0xFFFFFFFF)
    return out


def parse_frames(buf) -> List[bytes]:
    """Split socket-ready frames, [u32 big-endian length][body] back to back
    (what the framed drain leaves per recipient), into their bodies.  Strict:
    the frames must tile `buf` exactly, else ValueError."""
    buf = bytes(buf)
    out = []
    pos = 0
    while pos < len(buf):
        if pos + 4 > len(buf):
            raise ValueError(f"{len(buf) - pos} stray bytes after the last frame")
        length = int.from_bytes(buf[pos : pos + 4], "big")
        if pos + 4 + length > len(buf):
            raise ValueError(
                f"frame at {pos} claims {length} bytes, {len(buf) - pos - 4} are left")
        out.append(buf[pos + 4 : pos + 4 + length])
        pos += 4 + length
    return out
