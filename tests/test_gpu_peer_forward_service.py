"""Broker-plane forwarding on the device (gpu_peer_forward=True): the
two-broker framed-TCP scenario of test_gpu_plane_tcp_mesh.py, with the peer
broker as a recipient slot of the engine (CPU reference engine here; the
kernels are the same code path on cuda).  The tick may not do per-message
routing lookups on the host any more, and a lost peer must give its slot
and its DirectMap entries back."""

import asyncio

import torch

from tests.test_integration import new_db, stop_stack
from pushcdn_amd.broker.service import Broker, BrokerConfig
from pushcdn_amd.crypto import bls
from pushcdn_amd.ops import reference as ref
from pushcdn_amd.proto import message as m
from pushcdn_amd.proto.transports.tcp import Tcp
from pushcdn_amd.utils.keyhash import fnv1a64

INT32_MIN = -(2**31)
MAX_PEERS = 4


def run(coro):
    return asyncio.run(asyncio.wait_for(coro, timeout=100))


def make_gpu_broker(db, port_base, kp):
    return Broker(BrokerConfig(
        public_bind_endpoint=f"127.0.0.1:{port_base}",
        public_advertise_endpoint=f"127.0.0.1:{port_base}",
        private_bind_endpoint=f"127.0.0.1:{port_base + 1}",
        private_advertise_endpoint=f"127.0.0.1:{port_base + 1}",
        discovery_endpoint=db,
        keypair=kp,
        user_protocol=Tcp,
        broker_protocol=Tcp,
        heartbeat_interval_s=0.2,
        sync_interval_s=0.2,
        data_plane="gpu",
        gpu_device="cpu",
        gpu_max_users=16,
        gpu_ring_bytes=1 << 14,
        gpu_tick_interval_s=0.01,
        gpu_peer_forward=True,
        gpu_max_peers=MAX_PEERS,
        gpu_direct_table_size=256,
    ))


def device_owner(broker, pubkey):
    """What the engine's device DirectMap answers for a pubkey."""
    eng = broker._engine
    h = fnv1a64(pubkey, eng.hash_seed)
    q = torch.tensor([ref._i64(h)], dtype=torch.int64)
    return int(ref.direct_lookup(eng.direct_keys, eng.direct_vals, q)[0])


async def no_more(client, seconds=0.3):
    try:
        extra = await asyncio.wait_for(client.receive_message(), timeout=seconds)
    except asyncio.TimeoutError:
        return
    raise AssertionError(f"unexpected extra delivery: {extra}")


def test_flag_off_has_no_peer_slots(tmp_path):
    cfg = BrokerConfig(public_bind_endpoint="a", public_advertise_endpoint="a",
                       private_bind_endpoint="b", private_advertise_endpoint="b",
                       discovery_endpoint=new_db(tmp_path), data_plane="gpu",
                       gpu_device="cpu", gpu_max_users=8, gpu_ring_bytes=1 << 12)
    assert (cfg.gpu_peer_forward, cfg.gpu_max_peers, cfg.gpu_direct_table_size) == \
        (False, 32, 1 << 16)
    b = Broker(cfg)
    assert b._engine.n_peer_slots == 0 and b._engine.n_recipients == 8
    assert b._engine.direct_keys.numel() == 1 << 16


def test_gpu_peer_forward_two_broker_tcp_mesh(tmp_path):
    async def go():
        db = new_db(tmp_path)
        kp = bls.KeyPair.from_seed(1000)
        b1 = make_gpu_broker(db, 25500, kp)
        b2 = make_gpu_broker(db, 25510, kp)
        await b1.start()
        await b2.start()
        await b1.discovery.perform_heartbeat(0, 60)
        await b2.discovery.perform_heartbeat(0, 60)
        for _ in range(100):                      # mesh forms over framed TCP
            if len(b1.connections.brokers) == 1 and len(b2.connections.brokers) == 1:
                break
            await asyncio.sleep(0.05)
        assert len(b1.connections.brokers) == 1 and len(b2.connections.brokers) == 1
        # each side gave its peer a device slot
        assert b1._peer_slot_of == {b2.identity: 0} and b2._peer_slot_of == {b1.identity: 0}
        assert b1._engine.n_recipients == 16 + MAX_PEERS

        from pushcdn_amd.marshal import Marshal, MarshalConfig
        from pushcdn_amd.client import Client, ClientConfig

        marshal = Marshal(MarshalConfig(bind_endpoint="127.0.0.1:25520",
                                        discovery_endpoint=db, protocol=Tcp))
        await marshal.start()

        def tcp_client(seed, topics):
            return Client(ClientConfig(endpoint="127.0.0.1:25520",
                                       keypair=bls.KeyPair.from_seed(seed),
                                       subscribed_topics=list(topics), protocol=Tcp))

        # steer alice to b1, bob to b2 via artificial load reports
        await b1.discovery.perform_heartbeat(0, 60)
        await b2.discovery.perform_heartbeat(10, 60)
        alice = tcp_client(21, [5])
        await alice.ensure_initialized()
        await b1.discovery.perform_heartbeat(10, 60)
        await b2.discovery.perform_heartbeat(0, 60)
        bob = tcp_client(22, [5])
        await bob.ensure_initialized()
        for _ in range(100):
            if len(b1.connections.users) == 1 and len(b2.connections.users) == 1:
                break
            await asyncio.sleep(0.05)
        assert len(b1.connections.users) == 1 and len(b2.connections.users) == 1
        # topic/user CRDT syncs land in the DEVICE tables: the peer's users
        # as owner -(slot+2), the peer's topic as a bit of its slot
        for _ in range(100):
            if (device_owner(b1, bob.public_key) == -2
                    and device_owner(b2, alice.public_key) == -2
                    and 5 in b1.connections.broker_topics.get_values_by_key(str(b2.identity))
                    and 5 in b2.connections.broker_topics.get_values_by_key(str(b1.identity))):
                break
            await asyncio.sleep(0.05)
        assert device_owner(b1, bob.public_key) == -2
        assert device_owner(b2, alice.public_key) == -2
        assert device_owner(b1, alice.public_key) >= 0      # local registration path
        await asyncio.sleep(0.3)
        for b in (b1, b2):
            r = b._engine.n_users + 0
            assert (int(b._engine.sub_bitmap[5, r >> 6]) >> (r & 63)) & 1

        # from here on the tick may not route per message on the host
        calls = []
        for b in (b1, b2):
            for name in ("get_interested_by_topic", "get_broker_identifier_of_user"):
                def spy(*a, _name=name, **k):
                    calls.append(_name)
                    raise AssertionError(f"{_name} called on the GPU peer plane")
                setattr(b.connections, name, spy)

        # cross-broker broadcast: b1's kernels write alice's ring AND the
        # peer ring; b2 routes the remote-origin copy to bob only
        await alice.send_broadcast_message([5], b"gpu-mesh-broadcast")
        msg = await asyncio.wait_for(bob.receive_message(), timeout=10)
        assert isinstance(msg, m.Broadcast) and msg.message == b"gpu-mesh-broadcast"
        msg = await asyncio.wait_for(alice.receive_message(), timeout=10)
        assert msg.message == b"gpu-mesh-broadcast"

        # cross-broker direct through the device DirectMap, both directions
        await alice.send_direct_message(bob.public_key, b"gpu-mesh-direct")
        msg = await asyncio.wait_for(bob.receive_message(), timeout=10)
        assert isinstance(msg, m.Direct) and msg.message == b"gpu-mesh-direct"
        await bob.send_direct_message(alice.public_key, b"gpu-mesh-direct-back")
        msg = await asyncio.wait_for(alice.receive_message(), timeout=10)
        assert isinstance(msg, m.Direct) and msg.message == b"gpu-mesh-direct-back"

        # direct to self still local
        await alice.send_direct_message(alice.public_key, b"self")
        msg = await asyncio.wait_for(alice.receive_message(), timeout=10)
        assert msg.message == b"self"

        # exactly once, nothing extra.  bob is checked now; alice's stream
        # is read again below, where any surplus copy would come out first
        # (a timed-out receive is not resumed on a client)
        await asyncio.sleep(0.3)
        await no_more(bob)
        assert calls == []

        # lose the peer: b2 goes away, b1 must release the slot and delete
        # the device entries that pointed at it
        bob_key = bob.public_key
        bob.close()
        await b2.close()
        for _ in range(100):
            if not b1.connections.brokers and not b1._peer_slot_of:
                break
            await asyncio.sleep(0.05)
        assert not b1.connections.brokers
        assert b1._peer_slot_of == {}
        assert sorted(b1._free_peer_slots) == list(range(MAX_PEERS))
        assert b1._engine.direct_keys_owned_by(-2) == []
        assert device_owner(b1, bob_key) == INT32_MIN
        r = b1._engine.n_users + 0
        assert not (int(b1._engine.sub_bitmap[5, r >> 6]) >> (r & 63)) & 1
        # a Direct to the lost peer's user is dropped, not delivered locally:
        # the later self-direct arrives and nothing else does
        await alice.send_direct_message(bob_key, b"to-nobody")
        await alice.send_direct_message(alice.public_key, b"still-here")
        msg = await asyncio.wait_for(alice.receive_message(), timeout=10)
        assert isinstance(msg, m.Direct) and msg.message == b"still-here"
        await no_more(alice)
        assert int(b1._engine.ring_wpos.sum()) == 0
        assert calls == []

        await stop_stack([b1], marshal, alice)

    run(go())
