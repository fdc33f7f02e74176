"""By-reference delivery of large messages on the GPU data plane, checked on
the CPU engine (device="cpu": the serial models in pushcdn_amd.ops.reference),
the native pump over loopback TCP, and the broker service.

A message of at least ref_threshold wire bytes takes a 16-byte record
{u32 len | 0x80000000, u32 seq, u64 ref_off} in each recipient's ring; its
bytes stay in the host batch, which drain_compact_ref() hands back as the
reference buffer."""

import asyncio
import socket
import struct
import time

import pytest
import torch

from pushcdn_amd.broker.gpu_engine import (REF_FLAG, GpuBrokerEngine, parse_ring_records,
                                           ring_rec)
from pushcdn_amd.ops import reference as ref
from pushcdn_amd.proto import message as m

N_USERS, P = 6, 2
RING = 4096
THR = 1024
TOPIC = 5


def run(coro):
    return asyncio.run(asyncio.wait_for(coro, timeout=100))


def tick_task_alive(broker):
    ticks = [t for t in broker._tasks if t.get_name() == "gpu-tick"]
    return len(ticks) == 1 and not ticks[0].done()


def make_batch(msgs):
    offsets, buf = [0], b""
    for msg in msgs:
        buf += m.serialize(msg)
        offsets.append(len(buf))
    return buf, offsets


def broadcast_of_wire_len(wire_len, fill):
    """A Broadcast on TOPIC whose serialized length is exactly wire_len
    (Cap'n Proto lengths move in 8-byte steps)."""
    assert wire_len % 8 == 0
    for n in range(wire_len, 0, -1):
        msg = m.Broadcast([TOPIC], bytes([fill]) * n)
        if len(m.serialize(msg)) == wire_len:
            return msg
    raise AssertionError(f"no Broadcast serializes to {wire_len} bytes")


def pattern(n, salt):
    return bytes((i * 7 + salt) & 0xFF for i in range(n))


def make_engine(device="cpu", ref_threshold=THR, **kw):
    kw.setdefault("ring_bytes", RING)
    kw.setdefault("direct_table_size", 64)
    kw.setdefault("n_users", N_USERS)
    kw.setdefault("n_peer_slots", P)
    return GpuBrokerEngine(device=device, fanout_wire=True, ref_threshold=ref_threshold, **kw)


def populate(eng):
    """Users 0..2 and peer slot 0 take TOPIC; "dave" is local user 3, "erin"
    lives on peer slot 1."""
    for u in (0, 1, 2):
        eng.subscribe(u, [TOPIC])
    eng.set_peer_topics(0, [TOPIC])
    eng.register_direct_bulk([(b"dave", 3), (b"erin", -(1 + 2))])


def mixed_batch():
    """(msgs, origin): the by-reference acceptance batch."""
    msgs = [
        broadcast_of_wire_len(THR - 8, 0x11),          # just below: inline
        broadcast_of_wire_len(THR, 0x22),              # exactly at: by reference
        m.Broadcast([TOPIC], pattern(8192, 3)),        # larger than a whole ring
        m.Direct(b"dave", pattern(3000, 4)),           # large Direct, local user
        m.Direct(b"erin", pattern(2000, 5)),           # large Direct, peer-owned
        m.Broadcast([TOPIC], pattern(1500, 6)),        # remote origin, large
    ]
    return msgs, [0, 0, 0, 0, 0, 1]


def expected_rings(msgs):
    w = [m.serialize(x) for x in msgs]
    users = [w[0], w[1], w[2], w[5]]
    return {0: users, 1: users, 2: users, 3: [w[3]],
            N_USERS + 0: [w[0], w[1], w[2]],     # never the remote-origin one
            N_USERS + 1: [w[4]]}


def tick(eng, msgs, origin=None):
    batch, offsets = make_batch(msgs)
    if origin is None:
        buf, off = eng.ingest(batch, offsets)
    else:
        buf, off, origin = eng.ingest(batch, offsets, origin=origin)
    return eng.tick(buf, off, host_batch=batch, host_offsets=offsets, origin=origin)


def raw_headers(ring, wpos):
    """[(by_ref, len, seq, ref_off)] in ring write order."""
    out, pos = [], 0
    while pos + 16 <= wpos:
        length, seq, ref_off = struct.unpack_from("<IIQ", ring, pos)
        by_ref = bool(length & REF_FLAG)
        length &= REF_FLAG - 1
        out.append((by_ref, length, seq, ref_off))
        pos += 16 if by_ref else ring_rec(length)
    return out


def drained(eng):
    """Drain with the reference buffer: ({ring: [(seq, bytes)]}, {ring:
    headers}, wpos, refbuf)."""
    wpos, offsets, staging, refbuf = eng.drain_compact_ref()
    recs, hdrs = {}, {}
    for r in range(eng.n_recipients):
        n = int(wpos[r])
        if not n:
            continue
        ring = bytes(staging[int(offsets[r]):int(offsets[r + 1])].numpy().tobytes())
        recs[r] = parse_ring_records(ring, n, refbuf)
        hdrs[r] = raw_headers(ring, n)
    return recs, hdrs, wpos, refbuf


# ------------------------------- 1. engine -------------------------------

def test_mixed_batch_delivers_everything_by_reference():
    eng = make_engine()
    populate(eng)
    msgs, origin = mixed_batch()
    assert [len(m.serialize(x)) for x in msgs[:2]] == [THR - 8, THR]
    assert len(m.serialize(msgs[2])) > RING
    stats = tick(eng, msgs, origin)
    assert stats.n_drops == 0
    recs, hdrs, _wpos, refbuf = drained(eng)
    assert refbuf == make_batch(msgs)[0]
    want = expected_rings(msgs)
    assert {r: [p for _s, p in v] for r, v in recs.items()} == want
    for r, v in recs.items():
        seqs = [s for s, _p in v]
        assert seqs == sorted(seqs)
    # the just-below message is inline, the other two flagged
    by_seq = {seq: by_ref for by_ref, _l, seq, _o in hdrs[0]}
    assert [by_seq[s] for s in sorted(by_seq)] == [False, True, True, True]
    # a by-reference record is a bare header: ring use is 16 B each
    assert int(_wpos[0]) == ring_rec(THR - 8) + 3 * 16
    assert int(_wpos[3]) == 16 and int(_wpos[N_USERS + 1]) == 16


def test_same_batch_without_threshold_drops_the_large_message():
    eng = make_engine(ref_threshold=None)
    populate(eng)
    msgs, origin = mixed_batch()
    stats = tick(eng, msgs, origin)
    # the 8 KiB Broadcast fits no 4 KiB ring: three users and one peer lose it
    assert stats.n_drops == 4
    big = m.serialize(msgs[2])
    wpos = eng.ring_wpos.clone()
    for r in (0, 1, 2, N_USERS):
        got = [p for _s, p in parse_ring_records(eng.read_ring(r), int(wpos[r]))]
        assert big not in got


def test_constructor_and_tick_argument_checks():
    with pytest.raises(AssertionError):
        GpuBrokerEngine(device="cpu", n_users=4, ring_bytes=RING, fanout_wire=False,
                        ref_threshold=THR)
    with pytest.raises(AssertionError):     # an inline message would not fit a ring
        make_engine(ref_threshold=RING)
    make_engine(ref_threshold=RING - 16 + 1)   # ring_rec(RING - 16) == RING: fits
    eng = make_engine()
    batch, offsets = make_batch([m.Broadcast([TOPIC], b"x")])
    buf, off = eng.ingest(batch, offsets)
    with pytest.raises(ValueError):
        eng.tick(buf, off)
    with pytest.raises(ValueError):
        eng.tick(buf, off, host_batch=batch)


def test_parse_ring_records_reference_errors():
    rec = struct.pack("<IIQ", 100 | REF_FLAG, 7, 10)
    refbuf = bytes(range(120))
    assert parse_ring_records(rec, 16, refbuf) == [(7, refbuf[10:110])]
    with pytest.raises(ValueError):
        parse_ring_records(rec, 16)
    with pytest.raises(ValueError):
        parse_ring_records(rec, 16, refbuf[:109])
    # rings without flagged records behave as before, with or without refbuf
    inline = struct.pack("<IIQ", 3, 1, 0) + b"abc" + bytes(13)
    assert parse_ring_records(inline, 32) == [(1, b"abc")]
    assert parse_ring_records(inline, 32, b"") == [(1, b"abc")]


# ---------------------- 2. two ticks before one drain ----------------------

def test_two_ticks_resolve_into_the_joined_refbuf():
    eng = make_engine()
    populate(eng)
    a = [m.Broadcast([TOPIC], pattern(5000, 1)), m.Broadcast([TOPIC], b"small-a")]
    s = [m.Broadcast([TOPIC], b"only-small")]       # not retained
    b = [m.Broadcast([TOPIC], b"small-b"), m.Broadcast([TOPIC], pattern(6000, 2)),
         m.Direct(b"dave", pattern(2048, 9))]
    for msgs in (a, s, b):
        assert tick(eng, msgs).n_drops == 0
    recs, _hdrs, _wpos, refbuf = drained(eng)
    assert refbuf == make_batch(a)[0] + make_batch(b)[0]
    order = [m.serialize(x) for x in a + s + b[:2]]
    assert [p for _s, p in recs[0]] == order
    assert [p for _s, p in recs[N_USERS]] == order
    assert [p for _s, p in recs[3]] == [m.serialize(b[2])]
    # one retained batch comes back as the very object that was handed in
    batch, offsets = make_batch(a)
    buf, off = eng.ingest(batch, offsets)
    eng.tick(buf, off, host_batch=batch, host_offsets=offsets)
    assert eng.drain_compact_ref()[3] is batch
    assert eng.drain_compact_ref()[3] == b""


# ---------------------------- 3. ring-full edges ----------------------------

def test_ring_with_16_bytes_left_takes_a_reference_and_a_full_ring_drops_it():
    eng = make_engine()
    populate(eng)
    eng.ring_wpos[0] = RING - 16
    eng.ring_wpos[1] = RING
    big = m.Broadcast([TOPIC], pattern(3000, 8))
    stats = tick(eng, [big])
    assert stats.n_drops == 1
    assert int(eng.ring_wpos[0]) == RING and int(eng.ring_wpos[1]) == RING
    batch = make_batch([big])[0]
    ring0 = eng.read_ring(0)
    assert parse_ring_records(ring0[RING - 16:], 16, batch) == [(0, m.serialize(big))]
    assert int(eng.ring_wpos[2]) == 16


def test_plain_drains_discard_the_retained_batches():
    eng = make_engine()
    populate(eng)
    tick(eng, [m.Broadcast([TOPIC], pattern(3000, 8))])
    assert eng._ref_batches and eng._ref_base > 0
    wpos, _offsets, _staging = eng.drain_compact()
    assert int(wpos[0]) == 16
    wpos, _offsets, staging, refbuf = eng.drain_compact_ref()
    assert len(refbuf) == 0 and int(wpos.sum()) == 0 and staging.numel() == 0
    tick(eng, [m.Broadcast([TOPIC], pattern(3000, 8))])
    eng.drain_cursors()
    assert len(eng.drain_compact_ref()[3]) == 0
    # ref_base starts from zero again after any drain
    msgs = [m.Broadcast([TOPIC], pattern(2000, 1))]
    tick(eng, msgs)
    recs, hdrs, _wpos, _refbuf = drained(eng)
    assert hdrs[0] == [(True, len(m.serialize(msgs[0])), hdrs[0][0][2], 0)]
    assert [p for _s, p in recs[0]] == [m.serialize(msgs[0])]


# -------------------------------- 4. models --------------------------------

def test_model_fanout_ref_touches_nothing_after_a_reference_header():
    buf = pattern(4000, 1)
    payload_off = torch.tensor([3, 100, 2000], dtype=torch.int64)
    payload_len = torch.tensor([50, 1024, 1500], dtype=torch.int32)
    assert ref.ring_lengths(payload_len, 1024).tolist() == [50, 0, 0]
    assert ref.ring_lengths(payload_len, 1025).tolist() == [50, 1024, 0]
    pair_user = torch.tensor([0, 0, -1, 1], dtype=torch.int32)
    pair_msg = torch.tensor([1, 0, 2, 2], dtype=torch.int32)
    pair_dst = torch.tensor([0, 16, 0, 512], dtype=torch.int64)
    seq = torch.tensor([40, 41, 42], dtype=torch.int32)
    egress = bytearray(b"\xee" * 1024)
    ref.fanout_ref(buf, payload_off, payload_len, pair_user, pair_msg, pair_dst, seq,
                   egress, 1024, 1 << 33)
    want = bytearray(b"\xee" * 1024)
    want[0:16] = struct.pack("<IIQ", 1024 | REF_FLAG, 41, (1 << 33) + 100)
    want[16:32] = struct.pack("<IIQ", 50, 40, 0)
    want[32:82] = buf[3:53]
    want[512:528] = struct.pack("<IIQ", 1500 | REF_FLAG, 42, (1 << 33) + 2000)
    assert egress == want
    # below the threshold everywhere it is the plain fan-out
    a, b = bytearray(b"\xee" * 4096), bytearray(b"\xee" * 4096)
    dst = torch.tensor([0, 2048, 0, 1100], dtype=torch.int64)
    ref.fanout_ref(buf, payload_off, payload_len, pair_user, pair_msg, dst, seq, a, 1 << 20, 0)
    ref.fanout(buf, payload_off, payload_len, pair_user, pair_msg, dst, seq, b)
    assert a == b


# ------------------------- 5. pump over loopback TCP -------------------------

def _tcp_pair():
    srv = socket.socket()
    srv.bind(("127.0.0.1", 0))
    srv.listen(1)
    a = socket.create_connection(srv.getsockname())
    b, _ = srv.accept()
    srv.close()
    return a, b


def _recv_frames(pump, cid, n, timeout=10.0):
    got, deadline = [], time.monotonic() + timeout
    while len(got) < n and time.monotonic() < deadline:
        frames, closed = pump.recv_batch(cid, 1024)
        got.extend(frames)
        if closed:
            break
        if len(got) < n:
            time.sleep(0.002)
    return got


def _inline(seq, payload):
    return struct.pack("<IIQ", len(payload), seq, 0) + payload + bytes(-len(payload) % 16)


def _byref(seq, off, length):
    return struct.pack("<IIQ", length | REF_FLAG, seq, off)


@pytest.fixture()
def pump_pair():
    from pushcdn_amd.ops.build import build_core

    pump = build_core().Pump()
    a, b = _tcp_pair()
    tx, rx = pump.add(a.detach()), pump.add(b.detach())
    yield pump, tx, rx
    pump.stop()


def test_pump_mixes_inline_and_reference_records_in_seq_order(pump_pair):
    pump, tx, rx = pump_pair
    refbuf = pattern(300_000, 5)
    lead = b"\x00" * 32                       # the user's range starts mid-buffer
    ring = (_byref(12, 100_000, 200_000) + _inline(10, b"first") + _byref(13, 0, 1)
            + _inline(11, pattern(33, 2)) + _byref(14, 299_999, 1) + _byref(15, 300_000, 0))
    staging = lead + ring
    flat = pump.send_rings_batch_ref(staging, refbuf, [tx], [len(lead)], [len(staging)])
    want = [b"first", pattern(33, 2), refbuf[100_000:300_000], refbuf[0:1],
            refbuf[299_999:], b""]
    assert list(flat) == [6, sum(len(w) for w in want)]
    assert _recv_frames(pump, rx, 6) == want
    # single-ring sibling
    n, nbytes = pump.send_ring_ref(tx, ring, len(ring), refbuf)
    assert (n, nbytes) == (6, sum(len(w) for w in want))
    assert _recv_frames(pump, rx, 6) == want
    # without a reference buffer a flagged record stops the parse, as before
    n, _nb = pump.send_ring(tx, _inline(1, b"kept") + _byref(2, 0, 1), 48)
    assert n == 1
    assert _recv_frames(pump, rx, 1) == [b"kept"]


def test_pump_stops_at_a_reference_past_the_buffer(pump_pair):
    pump, tx, rx = pump_pair
    refbuf = pattern(1000, 1)
    ring = (_inline(1, b"one") + _byref(2, 10, 20) + _byref(3, 990, 11)
            + _inline(4, b"never"))
    flat = pump.send_rings_batch_ref(ring, refbuf, [tx], [0], [len(ring)])
    assert list(flat) == [2, 23]
    assert _recv_frames(pump, rx, 2) == [b"one", refbuf[10:30]]
    # an offset that would wrap the range check
    bad = _byref(5, (1 << 64) - 4, 8)
    assert list(pump.send_rings_batch_ref(bad, refbuf, [tx], [0], [16])) == [0, 0]
    # ranges are checked against the staging buffer too
    with pytest.raises(RuntimeError):
        pump.send_rings_batch_ref(ring, refbuf, [tx], [0], [len(ring) + 1])
    with pytest.raises(RuntimeError):
        pump.send_ring_ref(tx, ring, len(ring) + 1, refbuf)
    # the connection stays usable
    flat = pump.send_rings_batch_ref(_byref(6, 0, 1000), refbuf, [tx], [0], [16])
    assert list(flat) == [1, 1000]
    assert _recv_frames(pump, rx, 1) == [refbuf]


# -------------------------------- 6. service --------------------------------

def _service_config(db, tag, proto, **kw):
    from pushcdn_amd.broker.service import BrokerConfig
    from pushcdn_amd.crypto import bls

    cfg = dict(
        public_bind_endpoint=f"{tag}-pub", public_advertise_endpoint=f"{tag}-pub",
        private_bind_endpoint=f"{tag}-priv", private_advertise_endpoint=f"{tag}-priv",
        discovery_endpoint=db, keypair=bls.KeyPair.from_seed(1000),
        user_protocol=proto, broker_protocol=proto,
        heartbeat_interval_s=0.2, sync_interval_s=0.2,
        data_plane="gpu", gpu_device="cpu", gpu_max_users=16,
        gpu_ring_bytes=1 << 14, gpu_tick_interval_s=0.005, gpu_ref_threshold=4096,
    )
    cfg.update(kw)
    return BrokerConfig(**cfg)


async def large_and_small_scenario(endpoint, make_client, big=200 << 10):
    """A `big`-byte Broadcast reaches three subscribers intact, a Direct of
    the same size its recipient, and interleaved small messages keep their
    order.  Shared with the cuda:0 service test."""
    sender = make_client(endpoint, 31, [9])
    subs = [make_client(endpoint, 32 + i, [TOPIC]) for i in range(3)]
    for c in [sender] + subs:
        await c.ensure_initialized()
    await asyncio.sleep(0.3)
    body, dbody = pattern(big, 1), pattern(big, 2)
    await sender.send_broadcast_message([TOPIC], b"small-0")
    await sender.send_broadcast_message([TOPIC], body)
    await sender.send_broadcast_message([TOPIC], b"small-1")
    await sender.send_direct_message(subs[0].public_key, dbody)
    await sender.send_broadcast_message([TOPIC], b"small-2")
    for i, c in enumerate(subs):
        n = 5 if i == 0 else 4
        got = [(await asyncio.wait_for(c.receive_message(), timeout=30)).message
               for _ in range(n)]
        want = [b"small-0", body, b"small-1"] + ([dbody] if i == 0 else []) + [b"small-2"]
        assert got == want
    return [sender] + subs


def test_service_delivers_large_messages_through_small_rings(tmp_path):
    from tests.test_integration import make_client, make_marshal, new_db, stop_stack
    from pushcdn_amd.broker.service import Broker
    from pushcdn_amd.proto.transports.memory import Memory

    async def go():
        db = new_db(tmp_path)
        broker = Broker(_service_config(db, "byref", Memory))
        assert broker._engine.ref_threshold == 4096
        await broker.start()
        await broker.discovery.perform_heartbeat(0, 60)
        marshal, endpoint = make_marshal(db)
        await marshal.start()
        clients = await large_and_small_scenario(endpoint, make_client)
        assert int(broker._engine.ring_wpos.sum()) == 0
        assert tick_task_alive(broker)
        await stop_stack([broker], marshal, *clients)

    run(go())


def test_service_40_mib_broadcast_above_the_pool_cap(tmp_path):
    """A tick batch larger than the HBM pool (32 MiB on the CPU engine) is
    ingested without pool staging; the tick task survives it."""
    from tests.test_integration import make_client, make_marshal, new_db, stop_stack
    from pushcdn_amd.broker.service import Broker
    from pushcdn_amd.proto.transports.memory import Memory

    async def go():
        db = new_db(tmp_path)
        broker = Broker(_service_config(db, "byref40", Memory))
        assert broker._hbm_pool.capacity == 32 << 20
        await broker.start()
        await broker.discovery.perform_heartbeat(0, 60)
        marshal, endpoint = make_marshal(db)
        await marshal.start()
        a = make_client(endpoint, 41, [9])
        b = make_client(endpoint, 42, [TOPIC])
        await a.ensure_initialized()
        await b.ensure_initialized()
        await asyncio.sleep(0.3)
        body = pattern(1 << 20, 3) * 40
        await a.send_broadcast_message([TOPIC], body)
        msg = await asyncio.wait_for(b.receive_message(), timeout=60)
        assert msg.message == body
        assert tick_task_alive(broker)
        await a.send_broadcast_message([TOPIC], b"after")
        msg = await asyncio.wait_for(b.receive_message(), timeout=30)
        assert msg.message == b"after"
        assert broker._hbm_pool.used_bytes == 0 or broker._hbm_pool.free_bytes > 0
        await stop_stack([broker], marshal, a, b)

    run(go())


def test_two_brokers_large_broadcast_crosses_the_peer_ring_once(tmp_path):
    from tests.test_integration import new_db, stop_stack
    from pushcdn_amd.broker.service import Broker
    from pushcdn_amd.client import Client, ClientConfig
    from pushcdn_amd.crypto import bls
    from pushcdn_amd.marshal import Marshal, MarshalConfig
    from pushcdn_amd.proto.transports.tcp import Tcp

    async def go():
        db = new_db(tmp_path)

        def mk(port):
            return Broker(_service_config(
                db, "x", Tcp, gpu_peer_forward=True, gpu_max_peers=2,
                gpu_direct_table_size=256,
                public_bind_endpoint=f"127.0.0.1:{port}",
                public_advertise_endpoint=f"127.0.0.1:{port}",
                private_bind_endpoint=f"127.0.0.1:{port + 1}",
                private_advertise_endpoint=f"127.0.0.1:{port + 1}"))

        b1, b2 = mk(25600), mk(25610)
        for b in (b1, b2):
            await b.start()
        for b in (b1, b2):
            await b.discovery.perform_heartbeat(0, 60)
        for _ in range(100):
            if len(b1.connections.brokers) == 1 and len(b2.connections.brokers) == 1:
                break
            await asyncio.sleep(0.05)
        assert b1._peer_slot_of == {b2.identity: 0} and b2._peer_slot_of == {b1.identity: 0}
        marshal = Marshal(MarshalConfig(bind_endpoint="127.0.0.1:25620",
                                        discovery_endpoint=db, protocol=Tcp))
        await marshal.start()

        def client(seed):
            return Client(ClientConfig(endpoint="127.0.0.1:25620",
                                       keypair=bls.KeyPair.from_seed(seed),
                                       subscribed_topics=[TOPIC], protocol=Tcp))

        await b1.discovery.perform_heartbeat(0, 60)
        await b2.discovery.perform_heartbeat(10, 60)
        alice = client(51)
        await alice.ensure_initialized()
        await b1.discovery.perform_heartbeat(10, 60)
        await b2.discovery.perform_heartbeat(0, 60)
        bob = client(52)
        await bob.ensure_initialized()
        r = b1._engine.n_users + 0
        for _ in range(100):
            if (len(b1.connections.users) == 1 and len(b2.connections.users) == 1
                    and (int(b1._engine.sub_bitmap[TOPIC, r >> 6]) >> (r & 63)) & 1
                    and (int(b2._engine.sub_bitmap[TOPIC, r >> 6]) >> (r & 63)) & 1):
                break
            await asyncio.sleep(0.05)
        assert len(b1.connections.users) == 1 and len(b2.connections.users) == 1

        # count the large frames b1 hands to its peer (the asyncio transport
        # takes the parse_ring_records fallback of the peer-ring drain)
        big_sends = []
        orig = b1.try_send_to_broker

        async def spy(broker, raw):
            if len(raw.data) >= 200 << 10:
                big_sends.append(broker)
            return await orig(broker, raw)
        b1.try_send_to_broker = spy

        body = pattern(200 << 10, 4)
        await alice.send_broadcast_message([TOPIC], body)
        for c in (bob, alice):
            msg = await asyncio.wait_for(c.receive_message(), timeout=30)
            assert isinstance(msg, m.Broadcast) and msg.message == body
        await asyncio.sleep(0.3)
        try:
            extra = await asyncio.wait_for(bob.receive_message(), timeout=0.3)
        except asyncio.TimeoutError:
            extra = None
        assert extra is None
        assert big_sends == [b2.identity]
        assert tick_task_alive(b1) and tick_task_alive(b2)
        await stop_stack([b1, b2], marshal, alice, bob)

    run(go())


def test_mesh_broker_ignores_the_threshold():
    from pushcdn_amd.broker.mesh_service import MeshBroker
    from pushcdn_amd.broker.service import Broker

    assert Broker.REF_DELIVERY is True and MeshBroker.REF_DELIVERY is False
