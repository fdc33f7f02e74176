"""Peer-broker recipient slots and incremental DirectMap updates on the CPU
engine (device="cpu": the serial models in pushcdn_amd.ops.reference).

The recipient index space is R = n_users + P; peer slot p is ring
n_users + p and DirectMap owner -(p+2).  A message that arrived from a peer
broker (origin 1) never reaches a peer ring (single hop)."""

import pytest
import torch

from pushcdn_amd.broker.gpu_engine import GpuBrokerEngine, parse_ring_records
from pushcdn_amd.ops import reference as ref
from pushcdn_amd.proto import message as m
from pushcdn_amd.utils.keyhash import fnv1a64

INT32_MIN = -(2**31)
N_USERS, P = 70, 3


def make_batch(msgs):
    offsets, buf = [0], b""
    for msg in msgs:
        buf += m.serialize(msg)
        offsets.append(len(buf))
    return buf, offsets


def make_engine(n_users=N_USERS, n_peer_slots=P, **kw):
    kw.setdefault("ring_bytes", 4096)
    kw.setdefault("direct_table_size", 64)
    return GpuBrokerEngine(device="cpu", n_users=n_users, n_peer_slots=n_peer_slots,
                           fanout_wire=True, **kw)


def tick(eng, msgs, origin=None):
    batch, offsets = make_batch(msgs)
    if origin is None:
        buf, off = eng.ingest(batch, offsets)
    else:
        buf, off, origin = eng.ingest(batch, offsets, origin=origin)
    return eng.tick(buf, off, host_batch=batch, host_offsets=offsets, origin=origin)


def rings(eng):
    """{recipient: [wire bytes, ...]} for every non-empty ring."""
    wpos = eng.ring_wpos.clone()
    out = {}
    for r in range(eng.n_recipients):
        if int(wpos[r]):
            out[r] = [p for _s, p in parse_ring_records(eng.read_ring(r), int(wpos[r]))]
    return out


def peers_engine():
    eng = make_engine()
    eng.subscribe(1, [5])
    eng.subscribe(69, [5])
    eng.subscribe(2, [9])
    eng.set_peer_topics(0, [5])
    eng.set_peer_topics(1, [5, 6])
    eng.set_peer_topics(2, [7])
    return eng


def test_sizes_cover_peer_slots():
    eng = make_engine()
    assert eng.n_users == N_USERS and eng.n_recipients == N_USERS + P
    assert eng.W == 2 and eng.ring_wpos.numel() == N_USERS + P
    assert eng.egress.numel() == (N_USERS + P) * eng.ring_bytes
    with pytest.raises(IndexError):
        eng.set_peer_topics(P, [1])


def test_local_broadcast_reaches_users_and_each_interested_peer_once():
    eng = peers_engine()
    msg = m.Broadcast([5, 6], b"to-everyone")
    stats = tick(eng, [msg])
    wire = m.serialize(msg)
    # peer 1 is interested in BOTH topics and still gets one copy
    assert rings(eng) == {1: [wire], 69: [wire], N_USERS + 0: [wire], N_USERS + 1: [wire]}
    assert stats.n_drops == 0


def test_remote_origin_broadcast_reaches_only_local_users():
    eng = peers_engine()
    msg = m.Broadcast([5, 6], b"from-a-peer")
    tick(eng, [msg], origin=[1])
    wire = m.serialize(msg)
    assert rings(eng) == {1: [wire], 69: [wire]}


def test_mixed_origins_in_one_batch():
    eng = peers_engine()
    a, b = m.Broadcast([5], b"local"), m.Broadcast([5], b"remote")
    tick(eng, [a, b], origin=torch.tensor([0, 1], dtype=torch.int32))
    wa, wb = m.serialize(a), m.serialize(b)
    assert rings(eng) == {1: [wa, wb], 69: [wa, wb], N_USERS: [wa], N_USERS + 1: [wa]}


def test_subscribe_all_and_modulo_touch_user_bits_only():
    eng = peers_engine()
    eng.subscribe_all([7])
    msg = m.Broadcast([7], b"x")
    tick(eng, [msg])
    got = rings(eng)
    assert sorted(got) == list(range(N_USERS)) + [N_USERS + 2]   # peer 2 only, by its own bit
    eng.drain_cursors()
    eng.subscribe_modulo(4)
    tick(eng, [m.Broadcast([5], b"y")])
    got = rings(eng)
    # topic 5 has no user after the modulo rebuild (topics 0..3 only); the
    # peer bits of the row survived
    assert sorted(got) == [N_USERS, N_USERS + 1]
    eng.clear_peer(1)
    eng.drain_cursors()
    tick(eng, [m.Broadcast([5], b"z")])
    assert sorted(rings(eng)) == [N_USERS]


def test_direct_to_peer_owned_key():
    eng = peers_engine()
    eng.register_direct(b"local-user", 2)
    eng.apply_direct_updates([(b"on-peer-0", -2), (b"on-peer-2", -(2 + 2)),
                              (b"beyond-slots", -(P + 2))], [])
    msgs = [m.Direct(b"on-peer-0", b"d0"), m.Direct(b"on-peer-2", b"d2"),
            m.Direct(b"local-user", b"dl"), m.Direct(b"beyond-slots", b"nope"),
            m.Direct(b"unknown", b"nope")]
    stats = tick(eng, msgs)
    w = [m.serialize(x) for x in msgs]
    assert rings(eng) == {2: [w[2]], N_USERS: [w[0]], N_USERS + 2: [w[1]]}
    assert stats.n_drops == 0


def test_remote_origin_direct_to_peer_owned_key_is_not_forwarded():
    eng = peers_engine()
    eng.register_direct(b"local-user", 2)
    eng.apply_direct_updates([(b"on-peer-0", -2)], [])
    msgs = [m.Direct(b"on-peer-0", b"bounced"), m.Direct(b"local-user", b"ok")]
    stats = tick(eng, msgs, origin=[1, 1])
    assert rings(eng) == {2: [m.serialize(msgs[1])]}
    assert stats.n_drops == 0            # not forwarded is not a drop


def test_direct_to_deleted_key_produces_nothing():
    eng = peers_engine()
    eng.apply_direct_updates([(b"on-peer-0", -2), (b"on-peer-1", -3)], [])
    eng.apply_direct_updates([], [b"on-peer-0"])
    msgs = [m.Direct(b"on-peer-0", b"gone"), m.Direct(b"on-peer-1", b"kept")]
    stats = tick(eng, msgs)
    assert rings(eng) == {N_USERS + 1: [m.serialize(msgs[1])]}
    assert stats.n_drops == 0
    # the key stays in the table with the tombstone value
    h = fnv1a64(b"on-peer-0", 0)
    q = torch.tensor([ref._i64(h)], dtype=torch.int64)
    assert ref.direct_lookup(eng.direct_keys, eng.direct_vals, q).tolist() == [INT32_MIN]
    assert int((eng.direct_keys != 0).sum()) == 2


def test_full_peer_ring_drops_and_counts():
    eng = make_engine(ring_bytes=256)
    eng.set_peer_topics(0, [5])
    eng.apply_direct_updates([(b"on-peer-0", -2)], [])
    big = m.Broadcast([5], b"b" * 100)
    direct = m.Direct(b"on-peer-0", b"d" * 100)
    rec = ref.ring_rec(len(m.serialize(big)))
    n_fit = 256 // rec
    assert n_fit >= 1 and 256 - n_fit * rec < ref.ring_rec(len(m.serialize(direct)))
    msgs = [big] * (n_fit + 1) + [direct]
    stats = tick(eng, msgs)
    assert len(rings(eng)[N_USERS]) == n_fit
    assert stats.n_drops == 2                          # one broadcast + the direct


def test_no_peers_origin_none_equals_zero_origin():
    def run(origin):
        eng = make_engine(n_peer_slots=0)
        for u in range(0, N_USERS, 3):
            eng.subscribe(u, [u % 4])
        eng.register_direct_bulk([(b"u%d" % u, u) for u in range(10)] + [(b"far", -2)])
        msgs = [m.Broadcast([i % 4], b"p%d" % i * (i + 1)) for i in range(6)]
        msgs += [m.Direct(b"u3", b"direct"), m.Direct(b"far", b"remote-owned"),
                 m.Subscribe([1])]
        tick(eng, msgs, origin=origin)
        return eng

    a, b = run(None), run([0] * 9)
    assert torch.equal(a.ring_wpos, b.ring_wpos)
    assert torch.equal(a.egress, b.egress)
    assert int(a.ring_wpos.sum()) > 0


# ---------------------------------------------------------------------------
# topic_mask_origin / emit_direct_peers models
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n_users,n_peers", [(70, 3), (64, 2), (62, 4), (128, 1)])
def test_topic_mask_origin_clears_exactly_the_peer_bits(n_users, n_peers):
    R = n_users + n_peers
    W = (R + 63) // 64
    sub = torch.full((256, W), -1, dtype=torch.int64)
    buf, offsets = make_batch([m.Broadcast([1], b"a"), m.Broadcast([1], b"a"),
                               m.Direct(b"k", b"v")])
    pr = ref.parse_batch(buf, offsets)
    mask = ref.topic_mask_origin(sub, buf, pr.topics_off, pr.topics_cnt, pr.disc,
                                 [0, 1, 1], n_users)
    plain = ref.topic_mask(sub, buf, pr.topics_off, pr.topics_cnt, pr.disc)
    assert torch.equal(mask[0], plain[0]) and torch.equal(mask[2], plain[2])
    for r in range(W * 64):
        bit = (int(mask[1, r >> 6]) >> (r & 63)) & 1
        assert bit == (1 if r < n_users else 0), r


def test_emit_direct_peers_model():
    disc = torch.tensor([3, 3, 3, 3, 3, 3, 4, 3], dtype=torch.int32)
    owner = torch.tensor([1, -2, -(P + 1), -(P + 2), INT32_MIN, -2, -2, N_USERS],
                         dtype=torch.int32)
    origin = [0, 0, 0, 0, 0, 1, 0, 0]
    plen = torch.full((8,), 40, dtype=torch.int32)
    wpos = torch.zeros(N_USERS + P, dtype=torch.int64)
    wpos[N_USERS + P - 1] = 4096 - 32                  # last peer ring is full
    pu, pm, pd, drops = ref.emit_direct_peers(disc, owner, origin, plen, wpos, 4096,
                                              N_USERS, P)
    assert list(zip(pu.tolist(), pm.tolist(), pd.tolist())) == [
        (1, 0, 1 * 4096), (N_USERS, 1, N_USERS * 4096), (-1, 2, 0)]
    assert drops == 1
    assert int(wpos[1]) == 64 and int(wpos[N_USERS]) == 64


# ---------------------------------------------------------------------------
# direct_apply model against a dict, table size 8
# ---------------------------------------------------------------------------

def _lookup(keys, vals, hs):
    q = torch.tensor([ref._i64(h) for h in hs], dtype=torch.int64)
    return ref.direct_lookup(keys, vals, q).tolist()


def _check(keys, vals, model, absent=()):
    hs = list(model) + list(absent)
    want = [model[h] for h in model] + [INT32_MIN] * len(absent)
    assert _lookup(keys, vals, hs) == want


def test_direct_apply_model_wrapping_chain_tombstones_and_full_table():
    S = 8
    keys = torch.zeros(S, dtype=torch.int64)
    vals = torch.zeros(S, dtype=torch.int32)
    chain = [(i + 1) << 8 | 6 for i in range(4)] + [(1 << 63) | 0x506]   # all home to slot 6
    assert all(h & 7 == 6 for h in chain)
    model = {}
    ups = [(h, -(i + 2)) for i, h in enumerate(chain)]
    assert ref.direct_apply(keys, vals, ups, []) == 0
    model.update(ups)
    # the chain wrapped: slots 6, 7, 0, 1, 2
    assert [int(k) != 0 for k in keys] == [True, True, True, False, False, False, True, True]
    _check(keys, vals, model, absent=[0x906, 0x905])
    nonzero = int((keys != 0).sum())

    # delete two (one mid-chain), then re-upsert one with a new owner
    assert ref.direct_apply(keys, vals, [], [chain[1], chain[3]]) == 0
    model[chain[1]] = model[chain[3]] = INT32_MIN
    _check(keys, vals, model)
    assert int((keys != 0).sum()) == nonzero          # keys stay
    assert ref.direct_apply(keys, vals, [(chain[3], 5)], []) == 0
    model[chain[3]] = 5
    _check(keys, vals, model)
    assert int((keys != 0).sum()) == nonzero          # its old slot was reused
    # deleting an absent key and key 0 is a no-op
    before = (keys.clone(), vals.clone())
    assert ref.direct_apply(keys, vals, [(0, 1)], [0x906, 0]) == 0
    assert torch.equal(keys, before[0]) and torch.equal(vals, before[1])

    # fill the table, then a ninth key reports one failure and changes nothing
    fill = [(0x1000 | s, s) for s in (3, 4, 5)]
    assert ref.direct_apply(keys, vals, fill, []) == 0
    model.update(fill)
    assert int((keys != 0).sum()) == S
    before = (keys.clone(), vals.clone())
    assert ref.direct_apply(keys, vals, [(0x2003, 9)], []) == 1
    assert torch.equal(keys, before[0]) and torch.equal(vals, before[1])
    _check(keys, vals, model, absent=[0x2003])


# ---------------------------------------------------------------------------
# GpuBrokerEngine.apply_direct_updates
# ---------------------------------------------------------------------------

def _engine_lookup(eng, pubkeys):
    hs = [fnv1a64(k, eng.hash_seed) for k in pubkeys]
    return _lookup(eng.direct_keys, eng.direct_vals, hs)


def test_apply_direct_updates_compacts_past_half_the_table():
    eng = make_engine(direct_table_size=16, hash_seed=0x1234)
    first = [b"key-%d" % i for i in range(6)]
    eng.apply_direct_updates([(k, -2) for k in first], [])
    assert _engine_lookup(eng, first) == [-2] * 6
    eng.apply_direct_updates([(first[0], -3)], first[2:])         # 4 tombstones
    assert int((eng.direct_keys != 0).sum()) == 6                  # keys stay
    assert len(eng.directs.tombstones) == 4
    assert _engine_lookup(eng, first) == [-3, -2] + [INT32_MIN] * 4
    # 2 live + 4 tombstoned + 3 new = 9 > 16 / 2: compaction by rebuild
    more = [b"more-%d" % i for i in range(3)]
    eng.apply_direct_updates([(k, 7) for k in more], [])
    assert not eng.directs.tombstones
    assert int((eng.direct_keys != 0).sum()) == 5                  # live entries only
    assert _engine_lookup(eng, first + more) == [-3, -2] + [INT32_MIN] * 4 + [7] * 3
    assert sorted(eng.directs.entries.values()) == [-3, -2, 7, 7, 7]
    # a re-upsert of a deleted key after compaction is an ordinary insert
    eng.apply_direct_updates([(first[5], -4)], [])
    assert _engine_lookup(eng, [first[5]]) == [-4]


def test_apply_direct_updates_dedup_collision_and_full():
    eng = make_engine(direct_table_size=8)
    # last upsert wins; an upsert wins over a delete of the same key
    eng.apply_direct_updates([(b"a", -2), (b"b", -2), (b"a", -3)], [b"a", b"zzz"])
    assert _engine_lookup(eng, [b"a", b"b"]) == [-3, -2]
    assert eng.direct_keys_owned_by(-3) == [b"a"]
    # a hash that belongs to a different registered key: skipped, not raised
    h = fnv1a64(b"b", 0)
    eng.directs.pubkeys[h] = b"someone-else"
    eng.apply_direct_updates([(b"b", -4), (b"c", -4)], [b"b"])
    assert _engine_lookup(eng, [b"b", b"c"]) == [-2, -4]
    eng.directs.pubkeys[h] = b"b"
    # the old API still rebuilds and keeps working next to the new one
    eng.register_direct(b"local", 3)
    eng.unregister_direct(b"a")
    assert _engine_lookup(eng, [b"a", b"b", b"c", b"local"]) == [INT32_MIN, -2, -4, 3]
    with pytest.raises(RuntimeError, match="direct table full"):
        eng.apply_direct_updates([(b"fill-%d" % i, 1) for i in range(6)], [])
    assert _engine_lookup(eng, [b"b", b"c", b"local"]) == [-2, -4, 3]


def test_apply_direct_updates_without_tombstones_stays_incremental(monkeypatch):
    """Live entries past half the table, no tombstone to reclaim: still one
    incremental apply, no rebuild.  The first delete after that compacts."""
    eng = make_engine(direct_table_size=16)
    rebuilds = []
    real = eng.directs.rebuild
    monkeypatch.setattr(eng.directs, "rebuild",
                        lambda: (rebuilds.append(1), real())[1])
    keys = [b"k-%d" % i for i in range(10)]
    eng.apply_direct_updates([(k, -2) for k in keys[:6]], [])
    eng.apply_direct_updates([(k, -3) for k in keys[6:]], [])
    assert rebuilds == []
    assert _engine_lookup(eng, keys) == [-2] * 6 + [-3] * 4
    eng.apply_direct_updates([], [keys[0]])
    assert rebuilds == [1] and not eng.directs.tombstones
    assert _engine_lookup(eng, keys) == [INT32_MIN] + [-2] * 5 + [-3] * 4
    assert int((eng.direct_keys != 0).sum()) == 9


def test_apply_direct_updates_failed_apply_resyncs_device_table(monkeypatch):
    eng = make_engine(direct_table_size=16)
    eng.apply_direct_updates([(b"a", -2)], [])

    def boom(*a, **k):
        raise RuntimeError("device apply failed")

    monkeypatch.setattr(ref, "direct_apply", boom)
    with pytest.raises(RuntimeError, match="device apply failed"):
        eng.apply_direct_updates([(b"b", -3)], [b"a"])
    # host dicts and device table agree again
    assert _engine_lookup(eng, [b"a", b"b"]) == [INT32_MIN, -3]
    assert eng.direct_keys_owned_by(-3) == [b"b"] and not eng.directs.tombstones
