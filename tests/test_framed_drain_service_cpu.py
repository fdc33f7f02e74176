"""BrokerConfig.gpu_framed_drain on the broker service, CPU engine
(gpu_device="cpu"): one tcp-native client (the pump's send_framed_batch) and
one memory-transport user (parse_frames in Python) get their Broadcasts and
Directs complete and in send order; the overflow policy "evict" still sends
the delivered prefix first; the flag cannot be combined with
gpu_ref_threshold."""

import asyncio

import pytest

T1 = 5
MEM_KEY = b"framed-memory-user"


def run(coro):
    return asyncio.run(asyncio.wait_for(coro, timeout=100))


async def until(cond, what):
    for _ in range(400):
        if cond():
            return
        await asyncio.sleep(0.01)
    raise AssertionError(f"timed out waiting for {what}")


async def stack(tmp_path, port, ring_bytes=1 << 16, **kw):
    """One broker on the CPU engine with the framed drain on and tcp-native
    users, a marshal, a sender, a tcp-native subscriber of T1 and an injected
    memory-transport user subscribed to T1."""
    from tests.test_integration import new_db
    from pushcdn_amd.broker.service import Broker, BrokerConfig, UserHandle
    from pushcdn_amd.client import Client, ClientConfig
    from pushcdn_amd.crypto import bls
    from pushcdn_amd.marshal import Marshal, MarshalConfig
    from pushcdn_amd.proto.transports.memory import gen_testing_connection_pair
    from pushcdn_amd.proto.transports.tcp_native import TcpNative

    kw.setdefault("gpu_tick_interval_s", 0.005)
    db = new_db(tmp_path)
    pub, priv, mar = (f"127.0.0.1:{port + i}" for i in range(3))
    broker = Broker(BrokerConfig(
        public_bind_endpoint=pub, public_advertise_endpoint=pub,
        private_bind_endpoint=priv, private_advertise_endpoint=priv,
        discovery_endpoint=db, keypair=bls.KeyPair.from_seed(1000),
        user_protocol=TcpNative, broker_protocol=TcpNative,
        heartbeat_interval_s=0.2, sync_interval_s=0.2,
        data_plane="gpu", gpu_device="cpu", gpu_max_users=4,
        gpu_ring_bytes=ring_bytes, gpu_framed_drain=True, **kw))
    await broker.start()
    await broker.discovery.perform_heartbeat(0, 60)
    marshal = Marshal(MarshalConfig(bind_endpoint=mar, discovery_endpoint=db,
                                    protocol=TcpNative))
    await marshal.start()

    def client(seed, topics):
        return Client(ClientConfig(endpoint=mar, keypair=bls.KeyPair.from_seed(seed),
                                   subscribed_topics=topics, protocol=TcpNative))

    sender, a = client(91, [9]), client(92, [T1])
    for c in (sender, a):
        await c.ensure_initialized()
    # the memory-transport user, injected as broker.testing does, plus its
    # slot on the data plane
    mem, server_half = gen_testing_connection_pair(broker.limiter)
    handle = UserHandle(connection=server_half)
    assert broker.connections.add_user(MEM_KEY, handle, [T1]) is None
    handle.gpu_index = broker._claim_gpu_slot(MEM_KEY)
    broker._gpu_join(handle.gpu_index, MEM_KEY, [T1])
    handle.task = asyncio.get_running_loop().create_task(
        broker._user_receive_loop(MEM_KEY, handle))
    await until(lambda: len(broker.connections.users) == 3, "three users")
    return broker, marshal, sender, a, mem


def test_broadcasts_and_directs_arrive_complete_and_in_send_order(tmp_path):
    from tests.test_integration import stop_stack
    from pushcdn_amd.proto import message as m

    async def go():
        broker, marshal, sender, a, mem = await stack(tmp_path, 25700)
        assert broker._framed_drain
        drains = []
        real = broker._engine.drain_framed

        def spy():
            out = real()
            drains.append(int(out[3].sum()))
            return out

        broker._engine.drain_framed = spy
        assert getattr(broker.connections.users[a.public_key].connection,
                       "pump_handle", None) is not None
        assert getattr(broker.connections.users[MEM_KEY].connection,
                       "pump_handle", None) is None
        want_a, want_m = [], []
        for i in range(60):
            payload = bytes([i]) * (1 + (i * 37) % 300)
            if i % 3 == 0:
                await sender.send_direct_message(a.public_key, b"a" + payload)
                want_a.append(("d", b"a" + payload))
                await sender.send_direct_message(MEM_KEY, b"m" + payload)
                want_m.append(("d", b"m" + payload))
            await sender.send_broadcast_message([T1], payload)
            want_a.append(("b", payload))
            want_m.append(("b", payload))
        got_a = []
        for _ in want_a:
            msg = await asyncio.wait_for(a.receive_message(), timeout=30)
            got_a.append(("d" if isinstance(msg, m.Direct) else "b", bytes(msg.message)))
        got_m = []
        for _ in want_m:
            msg = await asyncio.wait_for(mem.recv_message(), timeout=30)
            got_m.append(("d" if isinstance(msg, m.Direct) else "b", bytes(msg.message)))
        assert got_a == want_a
        assert got_m == want_m
        assert sum(drains) == len(want_a) + len(want_m)      # all of it came framed
        await stop_stack([broker], marshal, sender, a)

    run(go())


def test_evict_still_sends_the_delivered_prefix_first(tmp_path):
    from tests.test_integration import stop_stack

    async def go():
        ring = 4096
        broker, marshal, sender, a, mem = await stack(
            tmp_path, 25705, ring_bytes=ring, gpu_overflow_policy="evict",
            gpu_tick_interval_s=0.2)
        removed = []
        real_remove = broker.remove_user

        async def remove_user(pubkey):
            removed.append(pubkey)
            await real_remove(pubkey)

        broker.remove_user = remove_user
        # one tick: two that fit, then one larger than the whole ring
        await sender.send_broadcast_message([T1], b"first")
        await sender.send_broadcast_message([T1], b"second")
        await sender.send_broadcast_message([T1], b"B" * 5000)
        got = [bytes((await asyncio.wait_for(a.receive_message(), timeout=30)).message)
               for _ in range(2)]
        assert got == [b"first", b"second"]
        await until(lambda: set(removed) == {a.public_key, MEM_KEY}, "both evictions")
        assert [bytes((await asyncio.wait_for(mem.recv_message(), timeout=30)).message)
                for _ in range(2)] == [b"first", b"second"]
        await stop_stack([broker], marshal, sender, a)

    run(go())


def test_the_flag_conflicts_with_by_reference_delivery():
    from pushcdn_amd.broker.service import Broker, BrokerConfig

    def cfg(**kw):
        return BrokerConfig(public_bind_endpoint="p", public_advertise_endpoint="p",
                            private_bind_endpoint="q", private_advertise_endpoint="q",
                            data_plane="gpu", gpu_device="cpu", gpu_max_users=4,
                            gpu_ring_bytes=4096, **kw)

    assert BrokerConfig.__dataclass_fields__["gpu_framed_drain"].default is False
    with pytest.raises(ValueError, match="gpu_ref_threshold"):
        Broker(cfg(gpu_framed_drain=True, gpu_ref_threshold=1024))
    # each alone is fine
    assert Broker(cfg(gpu_framed_drain=True))._framed_drain
    assert not Broker(cfg(gpu_ref_threshold=1024))._framed_drain


def test_the_mesh_broker_opts_out():
    from pushcdn_amd.broker.mesh_service import MeshBroker
    from pushcdn_amd.broker.service import Broker

    assert Broker.FRAMED_DRAIN is True and MeshBroker.FRAMED_DRAIN is False


def test_a_refused_range_costs_the_tick_not_the_connection(tmp_path):
    """The pump's -2: logged, nothing sent, nobody removed."""
    from tests.test_integration import stop_stack

    async def go():
        broker, marshal, sender, a, mem = await stack(tmp_path, 25710)
        removed = []
        real_remove = broker.remove_user

        async def remove_user(pubkey):
            removed.append(pubkey)
            await real_remove(pubkey)

        broker.remove_user = remove_user
        real = broker._engine.drain_framed
        spoil = [True]

        def spoiled():
            wpos, offsets, frame_len, frame_cnt, staging = real()
            if spoil[0] and int(frame_cnt.sum()):
                spoil[0] = False
                frame_cnt = frame_cnt + (frame_cnt > 0).to(frame_cnt.dtype)   # wrong counts
            return wpos, offsets, frame_len, frame_cnt, staging

        broker._engine.drain_framed = spoiled
        await sender.send_broadcast_message([T1], b"lost-to-the-bad-count")
        await until(lambda: not spoil[0], "the spoiled drain")
        await sender.send_broadcast_message([T1], b"marker")
        assert bytes((await asyncio.wait_for(a.receive_message(), timeout=30)).message) \
            == b"marker"
        assert removed == [] and a.public_key in broker.connections.users
        await stop_stack([broker], marshal, sender, a)

    run(go())


def test_cli_flag_reaches_the_config(monkeypatch):
    import argparse

    from pushcdn_amd import cli
    from pushcdn_amd.broker import service

    seen = []

    class FakeBroker:
        def __init__(self, cfg):
            seen.append(cfg.gpu_framed_drain)

        async def run_forever(self):
            return None

    monkeypatch.setattr(service, "Broker", FakeBroker)
    for argv, want in (([], False), (["--gpu-framed-drain"], True)):
        parser = argparse.ArgumentParser()
        cli._broker_args(parser)
        cli.cmd_broker(parser.parse_args(argv))
        assert seen[-1] is want
