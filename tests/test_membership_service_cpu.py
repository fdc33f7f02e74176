"""BrokerConfig.gpu_batched_membership on the broker service, CPU engine
(gpu_device="cpu"): connects, disconnects and Subscribe/Unsubscribe frames
go to the engine's membership log and are applied by the next tick, never
through the per-topic immediate methods or a DirectMap rebuild."""

import asyncio

T1, T2 = 5, 200
IMMEDIATE = ("subscribe", "unsubscribe", "register_direct", "unregister_direct")
REBUILD = ("rebuild",)       # of the engine's DirectMap, eng.directs
QUEUED = ("queue_join", "queue_leave", "queue_subscribe", "queue_unsubscribe")


def run(coro):
    return asyncio.run(asyncio.wait_for(coro, timeout=100))


def spy_on(engine, names):
    """Count the calls of the engine's `names` (the calls still happen)."""
    calls = {n: 0 for n in names}
    for n in names:
        def wrap(real, n=n):
            def spied(*a, **kw):
                calls[n] += 1
                return real(*a, **kw)
            return spied
        setattr(engine, n, wrap(getattr(engine, n)))
    return calls


async def until(cond, what):
    for _ in range(400):
        if cond():
            return
        await asyncio.sleep(0.01)
    raise AssertionError(f"timed out waiting for {what}")


async def recv(client):
    return (await asyncio.wait_for(client.receive_message(), timeout=30)).message


def _config(db, proto, pub, priv, **kw):
    from pushcdn_amd.broker.service import BrokerConfig
    from pushcdn_amd.crypto import bls

    return BrokerConfig(
        public_bind_endpoint=pub, public_advertise_endpoint=pub,
        private_bind_endpoint=priv, private_advertise_endpoint=priv,
        discovery_endpoint=db, keypair=bls.KeyPair.from_seed(1000),
        user_protocol=proto, broker_protocol=proto,
        heartbeat_interval_s=0.2, sync_interval_s=0.2,
        data_plane="gpu", gpu_device="cpu", gpu_max_users=4,
        gpu_ring_bytes=1 << 14, gpu_tick_interval_s=0.005, **kw)


def test_batched_membership_over_tcp(tmp_path):
    from tests.test_integration import new_db, stop_stack
    from pushcdn_amd.broker.service import Broker
    from pushcdn_amd.client import Client, ClientConfig
    from pushcdn_amd.crypto import bls
    from pushcdn_amd.marshal import Marshal, MarshalConfig
    from pushcdn_amd.proto.transports.tcp import Tcp

    async def go():
        db = new_db(tmp_path)
        broker = Broker(_config(db, Tcp, "127.0.0.1:25630", "127.0.0.1:25631",
                                gpu_batched_membership=True))
        eng = broker._engine
        immediate = spy_on(eng, IMMEDIATE)
        rebuilds = spy_on(eng.directs, REBUILD)
        queued = spy_on(eng, QUEUED)
        await broker.start()
        await broker.discovery.perform_heartbeat(0, 60)
        marshal = Marshal(MarshalConfig(bind_endpoint="127.0.0.1:25640",
                                        discovery_endpoint=db, protocol=Tcp))
        await marshal.start()

        def client(seed, topics):
            return Client(ClientConfig(endpoint="127.0.0.1:25640",
                                       keypair=bls.KeyPair.from_seed(seed),
                                       subscribed_topics=topics, protocol=Tcp))

        def topics_of(c):
            return set(broker.connections.user_topics.get_values_by_key(c.public_key))

        sender, c = client(61, [9]), client(62, [T1])
        await sender.ensure_initialized()
        await c.ensure_initialized()
        await until(lambda: len(broker.connections.users) == 2, "two users")
        # nothing routed yet: both joins are still in the log, not on the device
        assert eng.pending_membership == 2 and int((eng.sub_bitmap != 0).sum()) == 0
        assert queued["queue_join"] == 2

        # connect, then a broadcast on the topic of the connect
        await sender.send_broadcast_message([T1], b"one")
        assert await recv(c) == b"one"
        assert eng.pending_membership == 0

        # Subscribe to a second topic and receive on it
        await c.subscribe([T2])
        await until(lambda: topics_of(c) == {T1, T2}, "the Subscribe frame")
        await sender.send_broadcast_message([T2], b"two")
        assert await recv(c) == b"two"
        await sender.send_direct_message(c.public_key, b"direct")
        assert await recv(c) == b"direct"

        # Unsubscribe: nothing more on it (the next thing c sees is the marker)
        await c.unsubscribe([T2])
        await until(lambda: topics_of(c) == {T1}, "the Unsubscribe frame")
        await sender.send_broadcast_message([T2], b"must-not-arrive")
        await sender.send_broadcast_message([T1], b"marker")
        assert await recv(c) == b"marker"

        # disconnect: a Direct to the departed key is dropped, and the next
        # user of the slot sees nothing stale
        slot = broker.connections.users[c.public_key].gpu_index
        departed = c.public_key
        c.close()
        await until(lambda: departed not in broker.connections.users, "the disconnect")
        await sender.send_broadcast_message([T1], b"for-nobody")
        await sender.send_direct_message(departed, b"to-the-departed")
        d = client(63, [T1])
        await d.ensure_initialized()
        await until(lambda: d.public_key in broker.connections.users, "the new user")
        assert broker.connections.users[d.public_key].gpu_index == slot
        await sender.send_direct_message(departed, b"to-the-departed-again")
        await sender.send_broadcast_message([T1], b"fresh")
        assert await recv(d) == b"fresh"

        assert immediate == {n: 0 for n in IMMEDIATE} and rebuilds == {"rebuild": 0}
        assert queued == {"queue_join": 3, "queue_leave": 1, "queue_subscribe": 1,
                          "queue_unsubscribe": 1}
        ticks = [t for t in broker._tasks if t.get_name() == "gpu-tick"]
        assert len(ticks) == 1 and not ticks[0].done()
        await stop_stack([broker], marshal, sender, d)

    run(go())


def test_flag_defaults_to_off_and_off_means_the_immediate_methods(tmp_path):
    from tests.test_integration import make_client, make_marshal, new_db, stop_stack
    from pushcdn_amd.broker.service import Broker, BrokerConfig
    from pushcdn_amd.proto.transports.memory import Memory

    assert BrokerConfig.__dataclass_fields__["gpu_batched_membership"].default is False

    async def go():
        db = new_db(tmp_path)
        cfg = _config(db, Memory, "mship-off-pub", "mship-off-priv")
        assert cfg.gpu_batched_membership is False
        broker = Broker(cfg)
        eng = broker._engine
        immediate = spy_on(eng, IMMEDIATE)
        queued = spy_on(eng, QUEUED)
        await broker.start()
        await broker.discovery.perform_heartbeat(0, 60)
        marshal, endpoint = make_marshal(db)
        await marshal.start()
        a = make_client(endpoint, 71, [T1])
        await a.ensure_initialized()
        await until(lambda: len(broker.connections.users) == 1, "the user")
        # applied at once: on the device before anything is routed
        assert eng.pending_membership == 0 and int((eng.sub_bitmap != 0).sum()) == 1
        await a.subscribe([T2])
        await until(lambda: immediate["subscribe"] == 2, "the Subscribe frame")
        await a.unsubscribe([T2])
        await until(lambda: immediate["unsubscribe"] == 1, "the Unsubscribe frame")
        await a.send_broadcast_message([T1], b"echo")
        assert await recv(a) == b"echo"
        a.close()
        await until(lambda: not broker.connections.users, "the disconnect")
        assert immediate["register_direct"] == 1 and immediate["unregister_direct"] == 1
        assert immediate["unsubscribe"] == 2          # the slot's release clears all 256
        assert queued == {n: 0 for n in QUEUED}
        await stop_stack([broker], marshal, a)

    run(go())


def test_cli_flag_reaches_the_config(monkeypatch):
    import argparse

    from pushcdn_amd import cli
    from pushcdn_amd.broker import service

    seen = []

    class FakeBroker:
        def __init__(self, cfg):
            seen.append(cfg.gpu_batched_membership)

        async def run_forever(self):
            return None

    monkeypatch.setattr(service, "Broker", FakeBroker)
    for argv, want in (([], False), (["--gpu-batched-membership"], True)):
        parser = argparse.ArgumentParser()
        cli._broker_args(parser)
        cli.cmd_broker(parser.parse_args(argv))
        assert seen[-1] is want
