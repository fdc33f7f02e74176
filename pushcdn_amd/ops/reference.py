"""CPU reference implementations of the data-plane kernels.

Pure Python/torch mirrors of csrc/hip/dataplane.hip, used for:
  - golden-testing each HIP kernel (GPU result == this, bit-for-bit)
  - running the broker engine on CPU (tests without a GPU)

Semantics match the reference broker: topic match = union of subscriber sets
(connections/mod.rs:94-124), fan-out copies the raw payload per recipient
(sender.rs), per-(sender->recipient) FIFO order preserved.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from ..utils.keyhash import as_i64 as _i64, fnv1a64
from .ring_format import FRAME_SORT_MAX, REF_FLAG, ring_rec


@dataclass
class ParseResult:
    disc: torch.Tensor         # int32 [M]
    payload_off: torch.Tensor  # int64 [M]
    payload_len: torch.Tensor  # int32 [M]
    topics_off: torch.Tensor   # int64 [M]
    topics_cnt: torch.Tensor   # int32 [M]
    recip_hash: torch.Tensor   # int64 [M] (bit-cast u64)
    timestamp: torch.Tensor    # int64 [M]


def parse_batch(buf: bytes, offsets: List[int], hash_seed: int = 0) -> ParseResult:
    """Mirror of k4_parse_batch. `buf` is concatenated serialized Messages."""
    from ..proto import message as msglib

    M = len(offsets) - 1
    disc = torch.full((M,), -1, dtype=torch.int32)
    payload_off = torch.zeros(M, dtype=torch.int64)
    payload_len = torch.zeros(M, dtype=torch.int32)
    topics_off = torch.zeros(M, dtype=torch.int64)
    topics_cnt = torch.zeros(M, dtype=torch.int32)
    recip_hash = torch.zeros(M, dtype=torch.int64)
    timestamp = torch.zeros(M, dtype=torch.int64)

    for i in range(M):
        raw = buf[offsets[i] : offsets[i + 1]]
        base = offsets[i]
        try:
            r = msglib.parse_offsets(raw)
        except Exception:
            continue
        disc[i] = r["disc"]
        payload_off[i] = base + r["payload_off"] if r["payload_len"] else 0
        payload_len[i] = r["payload_len"]
        topics_off[i] = base + r["topics_off"] if r["topics_cnt"] else 0
        topics_cnt[i] = r["topics_cnt"]
        timestamp[i] = _i64(r["timestamp"])
        if r["disc"] == 3:
            recip_hash[i] = _i64(fnv1a64(r["recipient"], hash_seed))
    return ParseResult(disc, payload_off, payload_len, topics_off, topics_cnt, recip_hash, timestamp)


def topic_mask(
    sub_bitmap: torch.Tensor,  # int64 [256][W] (bit-cast u64)
    buf: bytes,
    topics_off: torch.Tensor,
    topics_cnt: torch.Tensor,
    disc: torch.Tensor,
) -> torch.Tensor:
    """Mirror of k2a_topic_mask: OR of topic rows for broadcast messages."""
    M = disc.shape[0]
    W = sub_bitmap.shape[1]
    mask = torch.zeros((M, W), dtype=torch.int64)
    for m in range(M):
        if int(disc[m]) != 4:
            continue
        off, cnt = int(topics_off[m]), int(topics_cnt[m])
        acc = torch.zeros(W, dtype=torch.int64)
        for t in buf[off : off + cnt]:
            acc |= sub_bitmap[t]
        mask[m] = acc
    return mask


def user_bits_of_word(w: int, n_users: int) -> int:
    """Bits of mask word w that belong to local users (recipients below
    n_users), as an unsigned 64-bit value — the kernels' closed form."""
    lo = w * 64
    if n_users >= lo + 64:
        return (1 << 64) - 1
    if n_users <= lo:
        return 0
    return (1 << (n_users - lo)) - 1


def topic_mask_origin(
    sub_bitmap: torch.Tensor,  # int64 [256][W], W = ceil((n_users + P) / 64)
    buf: bytes,
    topics_off: torch.Tensor,
    topics_cnt: torch.Tensor,
    disc: torch.Tensor,
    origin,                    # [M] 0 = from a local user, else from a peer broker
    n_users: int,
) -> torch.Tensor:
    """Mirror of k2a_topic_mask_origin_t (untransposed, [M][W]): topic_mask,
    then every recipient bit >= n_users (the peer slots) is cleared for a
    remote-origin message — single hop, the reference's to_users_only."""
    mask = topic_mask(sub_bitmap, buf, topics_off, topics_cnt, disc)
    W = sub_bitmap.shape[1]
    for m in range(disc.shape[0]):
        if int(origin[m]) == 0:
            continue
        for w in range(W):
            word = int(mask[m, w]) & ((1 << 64) - 1)
            mask[m, w] = _i64(word & user_bits_of_word(w, n_users))
    return mask


def emit_direct_peers(
    disc: torch.Tensor,
    owner: torch.Tensor,        # direct_lookup output
    origin,                     # [M]
    payload_len: torch.Tensor,
    ring_wpos: torch.Tensor,    # int64 [n_users + n_peers], mutated
    ring_bytes: int,
    n_users: int,
    n_peers: int,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    """Mirror of k5b_emit_direct_peers, serial in message order (the kernel
    claims atomically, so its pair ORDER is unspecified; the set of pairs
    and the cursor totals are the same whenever no ring fills).  owner in
    [0, n_users) is a local user; owner <= -2 is peer slot p = -owner-2,
    reached only by a local-origin message and only if p < n_peers.
    Returns (pair_user, pair_msg, pair_dst, drops); a full ring gives a
    (-1, msg, 0) placeholder and one drop."""
    pair_user: List[int] = []
    pair_msg: List[int] = []
    pair_dst: List[int] = []
    drops = 0
    for i in range(disc.shape[0]):
        if int(disc[i]) != 3:
            continue
        o = int(owner[i])
        if o >= 0:
            if o >= n_users:
                continue
            u = o
        else:
            p = -o - 2
            if p < 0 or p >= n_peers or int(origin[i]) != 0:
                continue
            u = n_users + p
        rec = ring_rec(int(payload_len[i]))
        wpos = int(ring_wpos[u])
        if wpos + rec > ring_bytes:
            pair_user.append(-1)
            pair_msg.append(i)
            pair_dst.append(0)
            drops += 1
            continue
        pair_user.append(u)
        pair_msg.append(i)
        pair_dst.append(u * ring_bytes + wpos)
        ring_wpos[u] = wpos + rec
    return (
        torch.tensor(pair_user, dtype=torch.int32),
        torch.tensor(pair_msg, dtype=torch.int32),
        torch.tensor(pair_dst, dtype=torch.int64),
        drops,
    )


def assign_emit(
    mask: torch.Tensor,         # int64 [M][W]
    payload_len: torch.Tensor,  # int32 [M]
    ring_wpos: torch.Tensor,    # int64 [n_users]
    ring_bytes: int,
    n_users: int,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    """Mirror of k2b: per-user ordered ring assignment. Returns
    (pair_user, pair_msg, pair_dst, drops); mutates ring_wpos."""
    M, W = mask.shape
    pair_user: List[int] = []
    pair_msg: List[int] = []
    pair_dst: List[int] = []
    drops = 0
    # Same grouping as the kernel: pairs grouped by user, messages in order.
    for u in range(n_users):
        w, bit = u >> 6, 1 << (u & 63)
        wpos = int(ring_wpos[u])
        for m in range(M):
            # Python's & on negative ints is two's-complement with infinite
            # sign extension, so this is correct for bit 63 too.
            if not (int(mask[m, w]) & bit):
                continue
            length = int(payload_len[m])
            rec = ring_rec(length)
            if wpos + rec > ring_bytes:
                drops += 1
                pair_user.append(-1)
                pair_msg.append(m)
                pair_dst.append(0)
                continue
            pair_user.append(u)
            pair_msg.append(m)
            pair_dst.append(u * ring_bytes + wpos)
            wpos += rec
        ring_wpos[u] = wpos
    return (
        torch.tensor(pair_user, dtype=torch.int32),
        torch.tensor(pair_msg, dtype=torch.int32),
        torch.tensor(pair_dst, dtype=torch.int64),
        drops,
    )


def fanout(
    buf: bytes,
    payload_off: torch.Tensor,
    payload_len: torch.Tensor,
    pair_user: torch.Tensor,
    pair_msg: torch.Tensor,
    pair_dst: torch.Tensor,
    msg_seq: torch.Tensor,
    egress: bytearray,
    zero_pad_to: Optional[int] = None,
) -> None:
    """Mirror of k3_fanout: write {u32 len, u32 seq, 8B pad} + payload.

    By default exactly 16+len bytes are written per record (k3_fanout and
    the wave kernel).  ``zero_pad_to=rec`` additionally zeroes
    [dst+16+len, dst+rec): the flat kernels' full-stride contract (every
    16 B unit of the record stride is stored, pad units as zeros)."""
    import struct

    for p in range(pair_user.shape[0]):
        u = int(pair_user[p])
        if u < 0:
            continue
        m = int(pair_msg[p])
        off, length = int(payload_off[m]), int(payload_len[m])
        dst = int(pair_dst[p])
        struct.pack_into("<IIII", egress, dst, length, int(msg_seq[m]) & 0xFFFFFFFF, 0, 0)
        egress[dst + 16 : dst + 16 + length] = buf[off : off + length]
        if zero_pad_to is not None and zero_pad_to > 16 + length:
            egress[dst + 16 + length : dst + zero_pad_to] = bytes(zero_pad_to - 16 - length)


def ring_lengths(payload_len: torch.Tensor, ref_threshold: int) -> torch.Tensor:
    """The by-reference ring-length split: the length K2b / K5b claim ring
    space for.  A message of at least ref_threshold bytes takes a bare
    header (length 0 -> ring_rec(0) = 16 B); a shorter one its own length."""
    return torch.where(payload_len >= ref_threshold,
                       torch.zeros_like(payload_len), payload_len)


def fanout_ref(
    buf: bytes,
    payload_off: torch.Tensor,
    payload_len: torch.Tensor,
    pair_user: torch.Tensor,
    pair_msg: torch.Tensor,
    pair_dst: torch.Tensor,
    msg_seq: torch.Tensor,
    egress: bytearray,
    ref_threshold: int,
    ref_base: int,
) -> None:
    """Mirror of k3_fanout_ref: a pair whose message is shorter than
    ref_threshold is written exactly as fanout writes it; any other gets the
    16 B header {u32 len | REF_FLAG, u32 seq, u64 ref_base + payload_off}
    and nothing else."""
    import struct

    for p in range(pair_user.shape[0]):
        u = int(pair_user[p])
        if u < 0:
            continue
        m = int(pair_msg[p])
        off, length = int(payload_off[m]), int(payload_len[m])
        dst = int(pair_dst[p])
        seq = int(msg_seq[m]) & 0xFFFFFFFF
        if length >= ref_threshold:
            struct.pack_into("<IIQ", egress, dst, length | REF_FLAG, seq, ref_base + off)
            continue
        struct.pack_into("<IIII", egress, dst, length, seq, 0, 0)
        egress[dst + 16 : dst + 16 + length] = buf[off : off + length]


def apply_subs(
    sub_bitmap: torch.Tensor,  # int64 [256][W] (bit-cast u64), mutated
    buf: bytes,
    topics_off: torch.Tensor,
    topics_cnt: torch.Tensor,
    disc: torch.Tensor,
    user_idx: torch.Tensor,
) -> None:
    """Mirror of k2c_apply_subs: Subscribe (5) / Unsubscribe (6) updates
    applied serially IN MESSAGE ORDER; other kinds and user_idx < 0 skipped."""
    for m in range(disc.shape[0]):
        d = int(disc[m])
        if d != 5 and d != 6:
            continue
        u = int(user_idx[m])
        if u < 0:
            continue
        w, bit = u >> 6, 1 << (u & 63)
        off, cnt = int(topics_off[m]), int(topics_cnt[m])
        for t in buf[off : off + cnt]:
            # u64 arithmetic, then the two's-complement cast back (bit 63)
            word = int(sub_bitmap[t, w]) & ((1 << 64) - 1)
            word = (word | bit) if d == 5 else (word & ~bit & ((1 << 64) - 1))
            sub_bitmap[t, w] = _i64(word)


MEMBERSHIP_WORDS = 10   # row: r, flags, clear[4], set[4]
MEMBERSHIP_RESET = 1    # flags bit 0: reset the recipient's ring cursor


def membership_apply(
    sub_bitmap: torch.Tensor,  # int64 [256][W] (bit-cast u64), mutated
    ring_wpos: torch.Tensor,   # int64 [R], mutated
    recs: torch.Tensor,        # int64 [n][MEMBERSHIP_WORDS]
) -> None:
    """Mirror of k8_membership_apply, serial.  Row = (r, flags, clear[4],
    set[4]); topic t is bit t & 63 of word t >> 6 of a 256-bit set.  For
    every topic, bit r of sub_bitmap[t][r >> 6] becomes 1 if `set` has t, 0
    if only `clear` has t (set wins), and is otherwise untouched; flags bit 0
    zeroes ring_wpos[r].  A row with r outside [0, R) is skipped whole."""
    R = ring_wpos.shape[0]
    u64 = (1 << 64) - 1
    for row in recs.tolist():
        r, flags = row[0], row[1]
        if r < 0 or r >= R:
            continue
        w, bit = r >> 6, 1 << (r & 63)
        col = sub_bitmap[:, w].tolist()   # the recipient's word of every topic
        for t in range(256):
            tbit = 1 << (t & 63)
            # u64 arithmetic, then the two's-complement cast back (bit 63)
            if row[6 + (t >> 6)] & tbit:
                col[t] = _i64((col[t] & u64) | bit)
            elif row[2 + (t >> 6)] & tbit:
                col[t] = _i64(col[t] & u64 & ~bit)
        sub_bitmap[:, w] = torch.tensor(col, dtype=torch.int64)
        if flags & MEMBERSHIP_RESET:
            ring_wpos[r] = 0


def recipient_demand(
    mask: torch.Tensor,         # int64 [M][W], origin clearing applied
    ring_len: torch.Tensor,     # int32 [M], what K2b / K5b claim ring space from
    disc: torch.Tensor,
    owner: Optional[torch.Tensor],   # direct_lookup output; None = no Directs routed
    origin,                     # [M] 0 = local; None = all local
    n_users: int,
    n_peers: int,
    demand: torch.Tensor,       # int64 [n_users + n_peers], mutated
) -> None:
    """Mirror of k9_recipient_demand (mask untransposed, [M][W]):
    demand[r] += ring_rec(ring_len[m]) for every message m of the tick that
    addresses recipient r — a Broadcast through bit r of its mask row, a
    Direct through the recipient emit_direct_peers resolves (which see).
    Whether the delivery then fits the ring plays no part."""
    M = int(ring_len.shape[0])
    R = n_users + n_peers
    add = [0] * R
    for m in range(M):
        rec = ring_rec(int(ring_len[m]))
        for w, word in enumerate(mask[m].tolist()):
            word &= (1 << 64) - 1
            while word:
                low = word & -word
                r = w * 64 + low.bit_length() - 1
                if r < R:
                    add[r] += rec
                word ^= low
        if owner is None or int(disc[m]) != 3:
            continue
        o = int(owner[m])
        if o >= 0:
            if o < n_users:
                add[o] += rec
        else:
            p = -o - 2
            if 0 <= p < n_peers and (origin is None or int(origin[m]) == 0):
                add[n_users + p] += rec
    demand += torch.tensor(add, dtype=torch.int64)


def loss_scan(demand: torch.Tensor, ring_wpos: torch.Tensor) -> List[Tuple[int, int]]:
    """Mirror of k10_loss_scan: [(r, demand[r] - ring_wpos[r])] over the
    recipients where the two differ, in recipient order (the kernel's order
    is unspecified); demand is zeroed, ring_wpos only read."""
    out = [(r, int(d) - int(w))
           for r, (d, w) in enumerate(zip(demand.tolist(), ring_wpos.tolist())) if d != w]
    demand.zero_()
    return out


def compact_rings(egress: bytes, ring_bytes: int, wpos) -> Tuple[List[int], bytes]:
    """Mirror of k7_compact_rings: every ring's used prefix, concatenated in
    ring order.  Returns (offsets, staging bytes); offsets is the exclusive
    scan of wpos with N+1 entries (ring u occupies [offsets[u], offsets[u+1]))."""
    offsets = [0]
    out = bytearray()
    for u, n in enumerate(int(x) for x in wpos):
        out += egress[u * ring_bytes : u * ring_bytes + n]
        offsets.append(offsets[-1] + n)
    return offsets, bytes(out)


def direct_lookup(table_keys: torch.Tensor, table_vals: torch.Tensor, query: torch.Tensor) -> torch.Tensor:
    """Mirror of k5_direct_lookup (linear probe, 0 = empty key)."""
    S = table_keys.shape[0]
    maskv = S - 1
    out = torch.full((query.shape[0],), -(2**31), dtype=torch.int32)
    for i in range(query.shape[0]):
        h = int(query[i]) & ((1 << 64) - 1)
        if h == 0:
            continue
        s = h & maskv
        for probe in range(S):
            k = int(table_keys[(s + probe) & maskv]) & ((1 << 64) - 1)
            if k == h:
                out[i] = table_vals[(s + probe) & maskv]
                break
            if k == 0:
                break
    return out


DIRECT_TOMBSTONE = -(2**31)  # INT32_MIN: direct_lookup's not-found value


def direct_apply(
    table_keys: torch.Tensor,   # int64 [S] (bit-cast u64), mutated
    table_vals: torch.Tensor,   # int32 [S], mutated
    upserts: List[Tuple[int, int]],   # (u64 key, owner)
    deletes: List[int],               # u64 keys
) -> int:
    """Mirror of k6_direct_apply, serial: upserts in order, then deletes.
    An upsert takes the first slot of its probe chain that is empty or
    already holds the key; a delete stores the tombstone value and LEAVES
    the key, so chains never break and a re-upsert reuses the slot.  Key 0
    is skipped.  Returns the number of upserts that found no slot."""
    S = table_keys.shape[0]
    assert S & (S - 1) == 0
    maskv = S - 1
    u64 = (1 << 64) - 1
    failed = 0
    for h, owner in upserts:
        h &= u64
        if h == 0:
            continue
        s = h & maskv
        for probe in range(S):
            slot = (s + probe) & maskv
            k = int(table_keys[slot]) & u64
            if k == 0 or k == h:
                table_keys[slot] = _i64(h)
                table_vals[slot] = owner
                break
        else:
            failed += 1
    for h in deletes:
        h &= u64
        if h == 0:
            continue
        s = h & maskv
        for probe in range(S):
            slot = (s + probe) & maskv
            k = int(table_keys[slot]) & u64
            if k == h:
                table_vals[slot] = DIRECT_TOMBSTONE
                break
            if k == 0:
                break
    return failed


def build_direct_table(entries: List[Tuple[int, int]], size: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host-side construction of the open-addressing table (u64 hash -> owner)."""
    assert size & (size - 1) == 0
    keys = torch.zeros(size, dtype=torch.int64)
    vals = torch.zeros(size, dtype=torch.int32)
    maskv = size - 1
    for h, owner in entries:
        h &= (1 << 64) - 1
        assert h != 0
        s = h & maskv
        for probe in range(size):
            slot = (s + probe) & maskv
            k = int(keys[slot]) & ((1 << 64) - 1)
            if k == 0 or k == h:
                keys[slot] = _i64(h)
                vals[slot] = owner
                break
        else:
            # DirectMap admits no more entries than slots: not reached from it
            raise RuntimeError(f"no free slot in a table of {size}")
    return keys, vals


def frame_rings(
    egress: torch.Tensor,      # uint8 [R * ring_bytes]
    ring_bytes: int,
    wpos: torch.Tensor,        # int64 [R], only read
    dst_off: torch.Tensor,     # int64 [R], the exclusive scan of wpos
    staging: torch.Tensor,     # uint8, mutated
    frame_len: torch.Tensor,   # int64 [R], mutated
    frame_cnt: torch.Tensor,   # int32 [R], mutated
) -> None:
    """Model of K11 (csrc/hip/framed_drain.hip): ring r's records as
    [u32 big-endian len][body] frames at staging[dst_off[r]:], frame_len[r]
    bytes of frame_cnt[r] frames, in seq order (circular-minimum base,
    ascending (seq - base) mod 2^32, ties in ring order).

    The cursor is clamped to [0, ring_bytes].  A record whose len has
    REF_FLAG set, exceeds MAX_MESSAGE_SIZE or does not fit below the cursor
    ends the ring there; the records before it are framed.  A ring is in
    order when no record's seq is circularly below its predecessor's; one
    that is not and holds more than FRAME_SORT_MAX records is copied raw
    (frame_cnt -1, frame_len = the cursor).  A region that leaves the staging
    buffer is treated as an empty ring."""
    import numpy as np

    from ..proto.message import MAX_MESSAGE_SIZE

    u32 = 0xFFFFFFFF
    eg = egress.numpy()
    st = staging.numpy()
    for r in range(wpos.shape[0]):
        used = min(max(int(wpos[r]), 0), ring_bytes)
        off = int(dst_off[r])
        frame_len[r] = 0
        frame_cnt[r] = 0
        if used < 16 or off < 0 or off + used > st.shape[0]:
            continue
        ring = eg[r * ring_bytes : r * ring_bytes + used].tobytes()
        recs = []   # (seq, body)
        pos = 0
        while pos + 16 <= used:
            length = int.from_bytes(ring[pos : pos + 4], "little")
            if length & REF_FLAG or length > MAX_MESSAGE_SIZE or pos + 16 + length > used:
                break
            recs.append((int.from_bytes(ring[pos + 4 : pos + 8], "little"),
                         ring[pos + 16 : pos + 16 + length]))
            pos += ring_rec(length)
        in_order = all(((b[0] - a[0]) & u32) <= 0x80000000 for a, b in zip(recs, recs[1:]))
        if not in_order:
            if len(recs) > FRAME_SORT_MAX:
                st[off : off + used] = eg[r * ring_bytes : r * ring_bytes + used]
                frame_len[r] = used
                frame_cnt[r] = -1
                continue
            base = recs[0][0]
            for seq, _ in recs:
                if (seq - base) & u32 > 0x80000000:
                    base = seq
            recs.sort(key=lambda rec: (rec[0] - base) & u32)   # stable: ties in ring order
        framed = b"".join(len(body).to_bytes(4, "big") + body for _, body in recs)
        assert len(framed) <= used
        st[off : off + len(framed)] = np.frombuffer(framed, dtype=np.uint8)
        frame_len[r] = len(framed)
        frame_cnt[r] = len(recs)
