"""Hand-built egress rings for the framed drain (K11), shared by the CPU tests
(the model, ops.reference.frame_rings) and the GPU tests (the kernels).

A Case is one call of the op: a ring size and a list of rings.  What a ring
must come out as is derived here from ring_format.parse_ring_records over the
ring's well-formed prefix, so neither the model nor the kernel checks itself.
The staging buffer is pre-filled with a sentinel, with a margin in front of
the first region and behind the last, so a stray store shows."""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from pushcdn_amd.ops.ring_format import (FRAME_SORT_MAX, REF_FLAG, parse_ring_records,
                                         ring_rec)
from pushcdn_amd.proto.message import MAX_MESSAGE_SIZE

SENTINEL = 0xA5
MARGIN = 48           # sentinel bytes in front of and behind the regions
FILL = 0xEE           # what a ring holds past its records


@dataclass
class Ring:
    data: bytes                 # the ring's bytes from its start (at most ring_bytes)
    wpos: int                   # the cursor handed to the op
    good: Optional[int] = None  # bytes of well-formed records (None: all of wpos)
    raw: bool = False           # must come back in ring mode


@dataclass
class Case:
    name: str
    ring_bytes: int
    rings: List[Ring] = field(default_factory=list)


def body(tag: int, n: int) -> bytes:
    return bytes((tag * 7 + k * 13 + 1) & 0xFF for k in range(n))


def rec(seq: int, payload: bytes) -> bytes:
    """One ring record; the 8 pad bytes are not zero, nobody may read them."""
    out = len(payload).to_bytes(4, "little") + (seq & 0xFFFFFFFF).to_bytes(4, "little") \
        + b"\xAB" * 8 + payload
    return out + b"\x00" * (ring_rec(len(payload)) - len(out))


def ring_of(seqs, lengths=None) -> Ring:
    """Records with the given seqs in ring order; record i's body is
    body(seq, lengths[i]) (default: i % 37 bytes)."""
    data = b"".join(
        rec(s, body(s, lengths[i] if lengths is not None else i % 37))
        for i, s in enumerate(seqs))
    return Ring(data, len(data))


EMPTY = Ring(b"", 0)


# ------------------------------- the cases -------------------------------

def alignment_rings() -> List[Ring]:
    up = list(range(41))
    return [ring_of(range(100, 141), up), ring_of(range(100, 141), up[::-1])]


def large_rings() -> List[Ring]:
    return [ring_of([7, 8], [1, 65_539])]


def order_rings() -> List[Ring]:
    out = [ring_of(list(range(50, 50 + n))[::-1]) for n in (2, 3, 64, 65, 130)]
    # a tick's broadcasts (claimed first, ascending) then its directs, whose
    # claims race: lower and higher seqs interleaved
    tick1 = list(range(0, 40, 2)) + [21, 5, 41, 13, 39, 1, 45, 43, 3]
    tick2 = [60 + s for s in tick1]
    out.append(ring_of(tick1))
    out.append(ring_of(tick1 + tick2))
    wrap = [(0xFFFFFFF0 + i) & 0xFFFFFFFF for i in range(40)]
    out.append(ring_of(wrap))
    out.append(ring_of([wrap[(i * 17) % 40] for i in range(40)]))
    return out


def cap_rings() -> List[Ring]:
    def lengths(n):
        return [1 if i % 4 == 0 else 0 for i in range(n)]

    def scrambled(n):
        return [(i * 2053) % n for i in range(n)]      # 2053 is coprime to both counts

    n = FRAME_SORT_MAX
    over = ring_of(scrambled(n + 1), lengths(n + 1))
    over.raw = True
    return [ring_of(scrambled(n), lengths(n)), over,
            ring_of(range(n + 1), lengths(n + 1))]


def malformed_rings(ring_bytes: int) -> List[Ring]:
    three = ring_of([1, 2, 3], [5, 20, 33])
    two = len(rec(1, body(1, 5))) + len(rec(2, body(2, 20)))
    flag = rec(1, body(1, 9)) + rec(2, body(2, 3)) \
        + (12 | REF_FLAG).to_bytes(4, "little") + (3).to_bytes(4, "little") + b"\x00" * 8 \
        + rec(4, body(4, 2))
    huge = rec(9, body(9, 17)) \
        + (MAX_MESSAGE_SIZE + 1).to_bytes(4, "little") + (10).to_bytes(4, "little") \
        + b"\x00" * 8 + rec(11, body(11, 4))
    # records that tile the ring to its last byte, and a cursor beyond it
    n_full = ring_bytes // 256
    full = ring_of(range(n_full), [256 - 16 - (i % 16) for i in range(n_full)])
    assert len(full.data) == ring_bytes
    return [
        Ring(three.data, 8, good=0),
        Ring(three.data, len(three.data) - 20, good=two),
        Ring(flag, len(flag), good=len(rec(1, body(1, 9))) + len(rec(2, body(2, 3)))),
        Ring(huge, len(huge), good=len(rec(9, body(9, 17)))),
        Ring(full.data, ring_bytes + 4096, good=ring_bytes),
    ]


def many_rings(ring_bytes: int, R: int = 70) -> List[Ring]:
    pool = (alignment_rings() + large_rings() + order_rings() + cap_rings()
            + malformed_rings(ring_bytes))
    out, k = [], 0
    for i in range(R):
        if i % 3 == 0 or i == R - 1:
            out.append(EMPTY)
        else:
            out.append(pool[k % len(pool)])
            k += 1
    assert k >= len(pool)
    return out


def all_cases() -> List[Case]:
    return [
        Case("alignment", 2048, alignment_rings()),
        Case("large", 128 << 10, large_rings()),
        Case("order", 16 << 10, order_rings()),
        Case("cap", 128 << 10, cap_rings()),
        Case("malformed", 1024, malformed_rings(1024)),
        Case("many", 128 << 10, many_rings(128 << 10)),
    ]


# --------------------------- running and checking ---------------------------

def expected_frames(ring: Ring, ring_bytes: int) -> List[bytes]:
    """The ring's bodies in delivery order, from parse_ring_records over the
    well-formed prefix."""
    good = min(ring.wpos, ring_bytes) if ring.good is None else ring.good
    return [bytes(p) for _seq, p in parse_ring_records(ring.data, good)]


def build_inputs(case: Case, device="cpu"):
    """(egress, wpos, dst_off, staging, frame_len, frame_cnt) for the op;
    frame_len / frame_cnt start as junk."""
    R = len(case.rings)
    eg = bytearray([FILL]) * (R * case.ring_bytes)
    for r, ring in enumerate(case.rings):
        assert len(ring.data) <= case.ring_bytes
        eg[r * case.ring_bytes : r * case.ring_bytes + len(ring.data)] = ring.data
    wpos = torch.tensor([ring.wpos for ring in case.rings], dtype=torch.int64)
    dst_off = MARGIN + torch.cumsum(wpos, 0) - wpos
    total = int(wpos.sum()) + 2 * MARGIN
    staging = torch.full((total,), SENTINEL, dtype=torch.uint8)
    egress = torch.frombuffer(eg, dtype=torch.uint8)
    frame_len = torch.full((R,), -7, dtype=torch.int64)
    frame_cnt = torch.full((R,), -7, dtype=torch.int32)
    return tuple(t.to(device) for t in (egress, wpos, dst_off, staging, frame_len, frame_cnt))


def check_outputs(case: Case, dst_off, staging, frame_len, frame_cnt) -> None:
    """Exact check of one call's outputs (CPU tensors)."""
    st = staging.numpy().tobytes()
    outside = np.ones(len(st), dtype=bool)
    for r, ring in enumerate(case.rings):
        off = int(dst_off[r])
        outside[off : off + max(ring.wpos, 0)] = False
        where = f"{case.name} ring {r}"
        if ring.raw:
            used = min(ring.wpos, case.ring_bytes)
            assert int(frame_cnt[r]) == -1, where
            assert int(frame_len[r]) == used, where
            assert st[off : off + used] == ring.data[:used], where
            continue
        frames = expected_frames(ring, case.ring_bytes)
        want = b"".join(len(f).to_bytes(4, "big") + f for f in frames)
        assert int(frame_cnt[r]) == len(frames), (where, int(frame_cnt[r]), len(frames))
        assert int(frame_len[r]) == len(want), (where, int(frame_len[r]), len(want))
        got = st[off : off + len(want)]
        if got != want:
            bad = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError(f"{where}: region differs first at byte {bad} of {len(want)}")
    stray = np.flatnonzero(outside & (staging.numpy() != SENTINEL))[:8].tolist()
    assert not stray, f"{case.name}: stores outside every region, first at {stray}"


# ----------------------------- engine scenarios -----------------------------

NU, NP = 67, 3
DIRECT_USERS = (1, 2, 10, 66)
REMOTE_KEY = b"framed-remote-user"      # owned by peer slot 1


def make_engine(device, **kw):
    from pushcdn_amd.broker.gpu_engine import GpuBrokerEngine

    kw.setdefault("ring_bytes", 1 << 14)
    return GpuBrokerEngine(device=device, n_users=NU, n_peer_slots=NP,
                           direct_table_size=256, fanout_wire=True, hash_seed=0xF7A3, **kw)


def _tick(eng, msgs):
    from pushcdn_amd.proto import message as m

    batch, offsets = b"", [0]
    for msg in msgs:
        batch += m.serialize(msg)
        offsets.append(len(batch))
    buf, off = eng.ingest(batch, offsets)
    eng.tick(buf, off, host_batch=batch, host_offsets=offsets)


def mixed_tick(tag: int):
    """Broadcasts on two topics with Directs between them, bodies of many
    lengths: a user of DIRECT_USERS gets both kinds in one tick."""
    from pushcdn_amd.proto import message as m

    msgs = []
    for i in range(24):
        msgs.append(m.Broadcast([5 + i % 2], body(tag + i, 3 + (i * 11) % 70)))
        if i % 3 == 0:
            u = DIRECT_USERS[(i // 3) % len(DIRECT_USERS)]
            msgs.append(m.Direct(b"framed-user-%d" % u, body(tag + 100 + i, (i * 7) % 50)))
        if i % 8 == 0:
            msgs.append(m.Direct(REMOTE_KEY, body(tag + 200 + i, 9)))
    return msgs


def run_scenario(device, framed: bool, join: bool = False, burst: bool = False, **kw):
    """Two mixed ticks (a queued join between them, a burst of 40 Directs to
    one user after them) and one drain.  Returns (engine, cursors, messages
    per recipient in delivery order, losses)."""
    from pushcdn_amd.broker.gpu_engine import parse_frames
    from pushcdn_amd.proto import message as m

    eng = make_engine(device, **kw)
    for u in range(NU):
        topics = ([5] if u % 2 == 0 else []) + ([6] if u % 3 == 0 else [])
        if topics:
            eng.subscribe(u, topics)
    eng.set_peer_topics(0, [5])
    eng.register_direct_bulk([(b"framed-user-%d" % u, u) for u in DIRECT_USERS]
                             + [(REMOTE_KEY, -(1 + 2))])
    _tick(eng, mixed_tick(0))
    if join:
        eng.queue_join(7, b"framed-joiner", [5, 6])
    _tick(eng, mixed_tick(1000))
    if burst:
        _tick(eng, [m.Direct(b"framed-user-1", body(i, 1 + i % 29)) for i in range(40)])
    R = NU + NP
    if framed:
        wpos, offsets, frame_len, frame_cnt, staging = eng.drain_framed()
        per = []
        for r in range(R):
            data = staging[int(offsets[r]) : int(offsets[r]) + int(frame_len[r])]
            data = data.numpy().tobytes()
            if int(frame_cnt[r]) < 0:
                per.append([bytes(p) for _s, p in parse_ring_records(data, int(wpos[r]))])
            else:
                per.append(parse_frames(data))
                assert len(per[-1]) == int(frame_cnt[r])
    else:
        wpos, offsets, staging = eng.drain_compact()
        per = [[bytes(p) for _s, p in parse_ring_records(
                    staging[int(offsets[r]):int(offsets[r + 1])].numpy().tobytes(),
                    int(wpos[r]))] for r in range(R)]
    return eng, [int(x) for x in wpos], per, eng.take_losses()
