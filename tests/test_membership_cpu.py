"""The engine's coalesced membership log on the CPU engine (device="cpu":
the serial models in pushcdn_amd.ops.reference).

queue_join / queue_leave / queue_subscribe / queue_unsubscribe record a
user's changes on the host; flush_membership() (run by every tick, drain and
immediate state-changing method) applies them as one batch of rows
(ref.membership_apply, the model of K8) plus one incremental DirectMap
update.  The result must be what the immediate methods give in program
order."""

import random

import pytest
import torch

from pushcdn_amd.broker.gpu_engine import GpuBrokerEngine, parse_ring_records
from pushcdn_amd.ops import reference as ref
from pushcdn_amd.proto import message as m
from pushcdn_amd.utils.keyhash import fnv1a64

INT32_MIN = -(2**31)
N_USERS, P = 70, 4
SEED = 0xFEED
U64 = (1 << 64) - 1


def _i64(x):
    return x - (1 << 64) if x >= (1 << 63) else x


def make_engine(device="cpu", **kw):
    kw.setdefault("n_users", N_USERS)
    kw.setdefault("n_peer_slots", P)
    kw.setdefault("ring_bytes", 4096)
    kw.setdefault("direct_table_size", 256)
    kw.setdefault("hash_seed", SEED)
    return GpuBrokerEngine(device=device, fanout_wire=True, **kw)


def make_batch(msgs):
    offsets, buf = [0], b""
    for msg in msgs:
        buf += m.serialize(msg)
        offsets.append(len(buf))
    return buf, offsets


def tick(eng, msgs, origin=None):
    batch, offsets = make_batch(msgs)
    if origin is None:
        buf, off = eng.ingest(batch, offsets)
    else:
        buf, off, origin = eng.ingest(batch, offsets, origin=origin)
    return eng.tick(buf, off, host_batch=batch, host_offsets=offsets, origin=origin)


def drain(eng):
    """{recipient: [wire bytes, ...]} of one drain_compact, in seq order."""
    _wpos, offsets, staging = eng.drain_compact()
    raw = staging.cpu().numpy().tobytes()
    out = {}
    for r in range(eng.n_recipients):
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        if hi > lo:
            out[r] = [p for _s, p in parse_ring_records(raw[lo:hi], hi - lo)]
    return out


def lookup(eng, keys):
    q = torch.tensor([_i64(fnv1a64(k, eng.hash_seed)) for k in keys], dtype=torch.int64)
    return ref.direct_lookup(eng.direct_keys.cpu(), eng.direct_vals.cpu(), q).tolist()


def has_bit(eng, r, t):
    return bool((int(eng.sub_bitmap[t, r >> 6]) & U64) >> (r & 63) & 1)


def topics_of(eng, r):
    return [t for t in range(256) if has_bit(eng, r, t)]


# ===========================================================================
# the model against a naive bit-by-bit application
# ===========================================================================

def pack_row(r, reset, clear, set_):
    """One membership row from topic lists."""
    words = [0] * 8
    for base, topics in ((0, clear), (4, set_)):
        for t in topics:
            words[base + (t >> 6)] |= 1 << (t & 63)
    return [r, 1 if reset else 0] + [_i64(w) for w in words]


def random_state(R, W, seed):
    """A sentinel-filled bitmap (random words) and non-zero cursors."""
    g = torch.Generator().manual_seed(seed)
    bitmap = torch.randint(0, 256, (256 * W * 8,), dtype=torch.uint8,
                           generator=g).view(torch.int64).reshape(256, W).clone()
    wpos = torch.randint(1, 1 << 20, (R,), dtype=torch.int64, generator=g) * 16
    return bitmap, wpos


def naive_apply(bitmap, wpos, rows):
    """Bits as Python sets: the contract spelled out without word tricks."""
    R = wpos.shape[0]
    bits = {(t, r) for t in range(256) for r in range(bitmap.shape[1] * 64)
            if (int(bitmap[t, r >> 6]) & U64) >> (r & 63) & 1}
    cursors = wpos.tolist()
    for r, reset, clear, set_ in rows:
        if r < 0 or r >= R:
            continue
        for t in clear:
            if t not in set_:
                bits.discard((t, r))
        for t in set_:
            bits.add((t, r))
        if reset:
            cursors[r] = 0
    out = torch.zeros_like(bitmap)
    for t, r in bits:
        out[t, r >> 6] = _i64((int(out[t, r >> 6]) & U64) | (1 << (r & 63)))
    return out, torch.tensor(cursors, dtype=torch.int64)


def test_model_matches_naive_application():
    rnd = random.Random(7)
    R, W = 70, 2
    bitmap, wpos = random_state(R, W, 11)
    recipients = rnd.sample(range(R), 20) + [-1, R, R + 57, 1 << 40]
    rows = []
    for r in recipients:
        clear = rnd.sample(range(256), rnd.choice([0, 3, 40, 256]))
        set_ = rnd.sample(range(256), rnd.choice([0, 2, 17]))
        rows.append((r, rnd.random() < 0.5, clear, set_))
    want_bitmap, want_wpos = naive_apply(bitmap, wpos, rows)
    recs = torch.tensor([pack_row(*row) for row in rows], dtype=torch.int64)
    ref.membership_apply(bitmap, wpos, recs)
    assert torch.equal(bitmap, want_bitmap)
    assert torch.equal(wpos, want_wpos)
    # bits of recipients 70..127 (no such recipient) kept their sentinels
    assert any(has_bit_raw(bitmap, r, 0) for r in range(R, W * 64))


def has_bit_raw(bitmap, r, t):
    return bool((int(bitmap[t, r >> 6]) & U64) >> (r & 63) & 1)


def test_model_set_wins_and_empty_batch():
    bitmap, wpos = random_state(3, 1, 3)
    before, wbefore = bitmap.clone(), wpos.clone()
    ref.membership_apply(bitmap, wpos, torch.zeros((0, 10), dtype=torch.int64))
    assert torch.equal(bitmap, before) and torch.equal(wpos, wbefore)
    recs = torch.tensor([pack_row(2, False, list(range(256)), [63, 64])], dtype=torch.int64)
    ref.membership_apply(bitmap, wpos, recs)
    assert [t for t in range(256) if has_bit_raw(bitmap, 2, t)] == [63, 64]
    assert torch.equal(wpos, wbefore)
    for r in (0, 1):   # the neighbours' bits are untouched
        assert all(has_bit_raw(bitmap, r, t) == has_bit_raw(before, r, t) for t in range(256))


# ===========================================================================
# folding inside one flush
# ===========================================================================

def test_subscribe_then_unsubscribe_leaves_the_bit_off():
    eng = make_engine()
    eng.queue_subscribe(5, [9, 10])
    eng.queue_unsubscribe(5, [9])
    assert eng.pending_membership == 1
    assert topics_of(eng, 5) == []          # nothing applied before the flush
    eng.flush_membership()
    assert eng.pending_membership == 0
    assert topics_of(eng, 5) == [10]


def test_unsubscribe_then_subscribe_leaves_the_bit_on():
    eng = make_engine()
    eng.subscribe(5, [9])
    eng.queue_unsubscribe(5, [9, 10])
    eng.queue_subscribe(5, [9])
    eng.flush_membership()
    assert topics_of(eng, 5) == [9]


def test_leave_then_join_of_the_slot_by_another_key():
    eng = make_engine()
    eng.queue_join(7, b"old-key", [1, 2, 200])
    eng.flush_membership()
    eng.ring_wpos[7] = 160
    assert topics_of(eng, 7) == [1, 2, 200] and lookup(eng, [b"old-key"]) == [7]
    eng.queue_leave(7, b"old-key")
    eng.queue_join(7, b"new-key", [2, 3])
    assert eng.pending_membership == 1
    eng.flush_membership()
    assert topics_of(eng, 7) == [2, 3]
    assert lookup(eng, [b"old-key", b"new-key"]) == [INT32_MIN, 7]
    assert int(eng.ring_wpos[7]) == 0
    assert eng.direct_keys_owned_by(7) == [b"new-key"]


def test_join_and_leave_inside_one_flush_never_reach_the_table():
    eng = make_engine()
    eng.queue_join(3, b"brief", [4])
    eng.queue_leave(3, b"brief")
    eng.flush_membership()
    assert topics_of(eng, 3) == [] and lookup(eng, [b"brief"]) == [INT32_MIN]
    assert int((eng.direct_keys != 0).sum()) == 0 and not eng.directs.tombstones
    assert not eng.directs.entries and not eng.directs.pubkeys


def test_leave_keeps_an_entry_that_moved_to_another_key_or_slot():
    """queue_leave deletes the DirectMap entry only while it still belongs
    to the departing key."""
    eng = make_engine()
    eng.queue_join(1, b"k", [1])
    eng.queue_join(2, b"k", [1])     # the same key connects again: slot 2 now
    eng.queue_leave(1, b"k2")        # an unrelated key leaves slot 1
    eng.flush_membership()
    assert lookup(eng, [b"k"]) == [2]
    assert topics_of(eng, 1) == [] and topics_of(eng, 2) == [1]


def test_log_is_bounded_by_recipients():
    eng = make_engine()
    for i in range(10_000):
        (eng.queue_subscribe if i % 2 == 0 else eng.queue_unsubscribe)(11, [i & 0xFF])
    assert eng.pending_membership == 1
    for slot in range(N_USERS):
        eng.queue_join(slot, b"u-%d" % slot, [slot])
        eng.queue_leave(slot, b"u-%d" % slot)
        eng.queue_join(slot, b"v-%d" % slot, [slot + 1])
    assert eng.pending_membership == N_USERS
    assert len(eng.directs.pending) <= 2 * N_USERS
    with pytest.raises(IndexError):
        eng.queue_subscribe(N_USERS + P, [1])
    with pytest.raises(IndexError):
        eng.queue_join(N_USERS, b"a-peer-slot-is-no-user", [1])


# ===========================================================================
# refusal, program order with the immediate API, the empty flush
# ===========================================================================

# every way to register `key` for user `slot`; the bulk call has an entry on
# either side of it, which a refusal must leave out as well
REGISTRATIONS = {
    "queue_join": lambda eng, slot, key: eng.queue_join(slot, key, [5]),
    "register_direct": lambda eng, slot, key: eng.register_direct(key, slot),
    "register_direct_bulk": lambda eng, slot, key: eng.register_direct_bulk(
        [(b"ahead", 3), (key, slot), (b"behind", 4)]),
}


def mirror_state(eng):
    """Copies of the log, the DirectMap's host mirror and its device table."""
    d = eng.directs
    return dict(rows={r: list(v) for r, v in eng._mship_rows.items()},
                pending=dict(d.pending), entries=dict(d.entries), pubkeys=dict(d.pubkeys),
                tombstones=set(d.tombstones), direct_keys=eng.direct_keys.clone(),
                direct_vals=eng.direct_vals.clone())


def assert_mirror_unchanged(eng, before, what):
    for name, now in mirror_state(eng).items():
        same = torch.equal(now, before[name]) if torch.is_tensor(now) else now == before[name]
        assert same, f"{what}: {name} changed"


def test_collision_refusal_changes_nothing():
    for name, register in REGISTRATIONS.items():
        eng = make_engine()
        eng.queue_join(1, b"first", [1])
        if name != "queue_join":
            eng.flush_membership()   # the immediate methods flush first, refused or not
        h = fnv1a64(b"victim", SEED)
        eng.directs.pubkeys[h] = b"someone-else"     # forge the collision
        eng.directs.entries[h] = 9
        before = mirror_state(eng)
        with pytest.raises(ValueError, match="collision"):
            register(eng, 2, b"victim")
        assert_mirror_unchanged(eng, before, name)
        assert eng.pending_membership == (1 if name == "queue_join" else 0)


def test_full_table_refusal_changes_nothing():
    eng = make_engine(direct_table_size=2)
    eng.queue_join(0, b"a", [1])
    eng.queue_join(1, b"b", [1])
    with pytest.raises(RuntimeError, match="direct table full"):
        eng.queue_join(2, b"c", [1])
    assert eng.pending_membership == 2 and len(eng.directs.entries) == 2
    eng.queue_join(1, b"b", [2])                 # a key that is in: no refusal
    eng.flush_membership()
    assert lookup(eng, [b"a", b"b", b"c"]) == [0, 1, INT32_MIN]
    # the immediate methods: the same refusal, and the table still rebuilds after it
    for name in ("register_direct", "register_direct_bulk"):
        eng = make_engine(direct_table_size=2)
        eng.register_direct(b"a", 0)
        eng.register_direct(b"b", 1)
        before = mirror_state(eng)
        with pytest.raises(RuntimeError, match="direct table full"):
            if name == "register_direct":
                eng.register_direct(b"c", 2)
            else:
                eng.register_direct_bulk([(b"b", 5), (b"c", 2)])
        assert_mirror_unchanged(eng, before, name)
        eng.register_direct(b"b", 6)             # a key that is in: no refusal
        assert lookup(eng, [b"a", b"b", b"c"]) == [0, 6, INT32_MIN]


def test_hash_zero_refusal_changes_nothing(monkeypatch):
    """Routing hash 0 is the table's empty marker: a key that hashes to it is
    refused like a collision, before anything changes; a remote entry with
    it is skipped."""
    from pushcdn_amd.broker import direct_map

    monkeypatch.setattr(direct_map, "fnv1a64",
                        lambda key, seed=0: 0 if key == b"zero" else fnv1a64(key, seed))
    for name, register in REGISTRATIONS.items():
        eng = make_engine()
        eng.queue_join(1, b"first", [1])
        if name != "queue_join":
            eng.flush_membership()
        before = mirror_state(eng)
        with pytest.raises(ValueError, match="hash 0"):
            register(eng, 2, b"zero")
        assert_mirror_unchanged(eng, before, name)
    eng = make_engine()
    eng.apply_direct_updates([(b"remote", -2), (b"zero", -3)], [b"zero"])
    assert list(eng.directs.pubkeys.values()) == [b"remote"]
    assert lookup(eng, [b"remote"]) == [-2]
    assert int((eng.direct_keys != 0).sum()) == 1


def test_immediate_call_flushes_the_pending_log_first():
    eng = make_engine()
    eng.queue_subscribe(4, [1, 2])
    eng.unsubscribe(4, [2])                      # after the queued subscribe
    assert eng.pending_membership == 0
    assert topics_of(eng, 4) == [1]
    eng.queue_join(6, b"six", [8])
    eng.unregister_direct(b"six")                # after the queued join
    assert lookup(eng, [b"six"]) == [INT32_MIN] and topics_of(eng, 6) == [8]
    eng.queue_leave(6, None)
    eng.register_direct(b"six", 6)
    assert lookup(eng, [b"six"]) == [6] and topics_of(eng, 6) == []
    eng.queue_subscribe(N_USERS + 1, [3])        # a peer recipient, by index
    eng.set_peer_topics(1, [7])                  # exact interest: replaces it
    assert topics_of(eng, N_USERS + 1) == [7]
    eng.queue_unsubscribe(4, [1])
    eng.apply_direct_updates([(b"remote", -2)], [])
    assert topics_of(eng, 4) == [] and lookup(eng, [b"remote"]) == [-2]


def test_tick_and_drain_flush_first():
    eng = make_engine()
    eng.queue_join(2, b"two", [5])
    tick(eng, [m.Broadcast([5], b"hello"), m.Direct(b"two", b"direct")])
    assert eng.pending_membership == 0
    eng.queue_leave(2, b"two")                   # before the drain: ring discarded
    assert drain(eng) == {}
    eng.queue_join(2, b"next", [6])
    tick(eng, [m.Broadcast([5], b"old-topic"), m.Direct(b"two", b"gone"),
               m.Broadcast([6], b"new-topic")])
    assert drain(eng) == {2: [m.serialize(m.Broadcast([6], b"new-topic"))]}


def test_empty_flush_performs_no_op_call(monkeypatch):
    eng = make_engine()
    calls = []
    monkeypatch.setattr(ref, "membership_apply", lambda *a: calls.append("membership_apply"))
    monkeypatch.setattr(ref, "direct_apply", lambda *a: calls.append("direct_apply"))
    monkeypatch.setattr(eng.directs, "rebuild", lambda: calls.append("rebuild"))
    eng.flush_membership()
    eng.drain_cursors()
    eng.drain_compact()
    eng.subscribe(1, [1])
    assert calls == []
    eng.queue_subscribe(1, [2])
    eng.flush_membership()
    assert calls == ["membership_apply"]         # no DirectMap change: no K6 either
    eng.flush_membership()
    assert calls == ["membership_apply"]


# ===========================================================================
# equivalence with the immediate API on a random sequence
# ===========================================================================

TOPICS = [0, 1, 5, 63, 64, 127, 128, 255]
PEER_KEYS = [b"peer-key-%d" % i for i in range(6)]


def make_sequence(seed=20240611, n_ops=300, tick_every=20):
    """A seeded program of joins, leaves, subscribes and unsubscribes over
    the user slots (LIFO free list, as the service hands them out), with a
    tick of mixed Broadcast/Direct every ~tick_every ops.  Returns
    (ops, every key ever used)."""
    rnd = random.Random(seed)
    free = list(range(N_USERS - 1, -1, -1))
    # the slots the kernel tests care about come out first
    for s in (69, 64, 63, 0):
        free.remove(s)
        free.append(s)
    live, keys, ops, n_keys = {}, [], [], 0

    def a_tick():
        msgs, origin = [], []
        for _ in range(rnd.randint(4, 8)):
            if rnd.random() < 0.6 or not keys:
                msgs.append(m.Broadcast(rnd.sample(TOPICS, rnd.randint(1, 3)),
                                        b"b" * rnd.randint(0, 40)))
            else:
                msgs.append(m.Direct(rnd.choice(keys + PEER_KEYS), b"d" * rnd.randint(1, 40)))
            origin.append(1 if rnd.random() < 0.25 else 0)
        ops.append(("tick", msgs, origin))

    for i in range(n_ops):
        roll = rnd.random()
        if roll < 0.35 and free or not live:
            slot = free.pop()
            if live and rnd.random() < 0.15:
                # a key that is connected connects again: its old session is
                # kicked first, and the LIFO list may hand the same slot back
                old = rnd.choice(sorted(live))
                key = live.pop(old)
                ops.append(("leave", old, key))
                free.append(slot)
                free.append(old)
                slot = free.pop()
            else:
                key = b"user-%d" % n_keys
                n_keys += 1
                keys.append(key)
            live[slot] = key
            ops.append(("join", slot, key, rnd.sample(TOPICS, rnd.randint(0, 4))))
        elif roll < 0.55:
            slot = rnd.choice(sorted(live))
            ops.append(("leave", slot, live.pop(slot)))
            free.append(slot)
        elif roll < 0.8:
            ops.append(("sub", rnd.choice(sorted(live)), rnd.sample(TOPICS, rnd.randint(1, 3))))
        else:
            ops.append(("unsub", rnd.choice(sorted(live)), rnd.sample(TOPICS, rnd.randint(1, 3))))
        if i % tick_every == tick_every - 1:
            a_tick()
    a_tick()
    return ops, keys


def setup_peers(eng):
    """Peer interests and peer-owned DirectMap entries, set beforehand."""
    eng.set_peer_topics(0, [0, 63])
    eng.set_peer_topics(1, [64, 255])
    eng.set_peer_topics(2, [5])
    eng.set_peer_topics(3, TOPICS)
    eng.apply_direct_updates([(k, -(2 + i % P)) for i, k in enumerate(PEER_KEYS)], [])


def peer_state(eng):
    bitmap = eng.sub_bitmap.cpu()
    bits = [[has_bit_raw(bitmap, N_USERS + p, t) for t in range(256)] for p in range(P)]
    return bits, lookup(eng, PEER_KEYS)


def run_sequence(eng, ops, keys, batched):
    """Apply `ops` through queue_* (batched) or today's immediate methods.
    Returns what must not depend on the way: the drained rings of every
    tick, the final bitmap and the lookup of every key ever used."""
    drains = []
    for op in ops:
        kind = op[0]
        if kind == "tick":
            tick(eng, op[1], op[2])
            drains.append(drain(eng))
        elif batched:
            {"join": eng.queue_join, "leave": eng.queue_leave,
             "sub": eng.queue_subscribe, "unsub": eng.queue_unsubscribe}[kind](*op[1:])
        elif kind == "join":
            eng.subscribe(op[1], op[3])
            eng.register_direct(op[2], op[1])
        elif kind == "leave":
            eng.unregister_direct(op[2])
            eng.unsubscribe(op[1], list(range(256)))
        elif kind == "sub":
            eng.subscribe(op[1], op[2])
        else:
            eng.unsubscribe(op[1], op[2])
    eng.flush_membership()
    return drains, eng.sub_bitmap.cpu().clone(), lookup(eng, keys + PEER_KEYS)


_cached = {}


def immediate_reference():
    """The sequence on a CPU engine through the immediate API: computed
    once, shared (also by the GPU test), never modified."""
    if not _cached:
        ops, keys = make_sequence()
        eng = make_engine()
        setup_peers(eng)
        peers_before = peer_state(eng)
        result = run_sequence(eng, ops, keys, batched=False)
        _cached.update(ops=ops, keys=keys, peers_before=peers_before, result=result,
                       peers_after=peer_state(eng))
    return _cached


def assert_same_as_immediate(eng):
    """Run the shared sequence on `eng` through queue_* and compare."""
    want = immediate_reference()
    setup_peers(eng)
    assert peer_state(eng) == want["peers_before"]
    drains, bitmap, lookups = run_sequence(eng, want["ops"], want["keys"], batched=True)
    w_drains, w_bitmap, w_lookups = want["result"]
    assert len(drains) == len(w_drains) >= 15
    for i, (got, exp) in enumerate(zip(drains, w_drains)):
        assert got == exp, f"tick {i}"
    assert torch.equal(bitmap, w_bitmap)
    assert lookups == w_lookups
    # a user's rows never touch a peer's bits or a peer's DirectMap entries
    assert peer_state(eng) == want["peers_before"] == want["peers_after"]
    assert eng.pending_membership == 0


def test_sequence_is_a_real_workload():
    want = immediate_reference()
    kinds = [op[0] for op in want["ops"]]
    assert min(kinds.count(k) for k in ("join", "leave", "sub", "unsub")) >= 30
    delivered = sum(len(v) for d in want["result"][0] for v in d.values())
    to_peers = sum(len(v) for d in want["result"][0] for r, v in d.items() if r >= N_USERS)
    assert delivered >= 100 and to_peers >= 10
    assert INT32_MIN in want["result"][2] and any(o >= 0 for o in want["result"][2])


def test_batched_sequence_equals_immediate_api(monkeypatch):
    eng = make_engine()
    rebuilds = []
    real = eng.directs.rebuild
    monkeypatch.setattr(eng.directs, "rebuild",
                        lambda: (rebuilds.append(1), real())[1])
    assert_same_as_immediate(eng)
    # the point of the log: not one rebuild per connect and disconnect
    kinds = [op[0] for op in immediate_reference()["ops"]]
    assert len(rebuilds) < (kinds.count("join") + kinds.count("leave")) // 4
