"""BrokerConfig.gpu_overflow_policy on the broker service, CPU engine
(gpu_device="cpu"), real TCP: a Broadcast that cannot fit its subscriber's
egress ring is dropped on the data plane, and the policy decides whether the
broker says nothing ("ignore", the default), counts it ("count") or also
removes the subscriber once what did fit was sent ("evict")."""

import asyncio

import pytest

from pushcdn_amd.broker.gpu_engine import ring_rec

T1, T2 = 5, 200
RING = 4096
BIG = b"B" * 5000          # its record is larger than the whole ring


def run(coro):
    return asyncio.run(asyncio.wait_for(coro, timeout=100))


async def until(cond, what):
    for _ in range(400):
        if cond():
            return
        await asyncio.sleep(0.01)
    raise AssertionError(f"timed out waiting for {what}")


async def recv(client):
    return (await asyncio.wait_for(client.receive_message(), timeout=30)).message


def value(counter):
    """Current value of a metrics counter (prometheus_client or the fallback)."""
    inner = getattr(counter, "_value", None)
    return inner.get() if inner is not None else counter.value


def counters():
    from pushcdn_amd.utils import metrics

    return {name: value(getattr(metrics, name))
            for name in ("GPU_RING_LOST_BYTES", "GPU_RING_OVERFLOWS", "GPU_RING_EVICTIONS")}


def moved(before):
    return {k: v - before[k] for k, v in counters().items()}


def big_record():
    from pushcdn_amd.proto import message as m

    rec = ring_rec(len(m.serialize(m.Broadcast([T1], BIG))))
    assert rec > RING
    return rec


async def stack(tmp_path, port, **kw):
    """One broker on the CPU engine with 4096-byte rings, a marshal, a sender
    subscribed to nothing that is sent, A on T1 and B on T2."""
    from tests.test_integration import new_db
    from pushcdn_amd.broker.service import Broker, BrokerConfig
    from pushcdn_amd.client import Client, ClientConfig
    from pushcdn_amd.crypto import bls
    from pushcdn_amd.marshal import Marshal, MarshalConfig
    from pushcdn_amd.proto.transports.tcp import Tcp

    db = new_db(tmp_path)
    pub, priv, mar = (f"127.0.0.1:{port + i}" for i in range(3))
    broker = Broker(BrokerConfig(
        public_bind_endpoint=pub, public_advertise_endpoint=pub,
        private_bind_endpoint=priv, private_advertise_endpoint=priv,
        discovery_endpoint=db, keypair=bls.KeyPair.from_seed(1000),
        user_protocol=Tcp, broker_protocol=Tcp,
        heartbeat_interval_s=0.2, sync_interval_s=0.2,
        data_plane="gpu", gpu_device="cpu", gpu_max_users=4,
        gpu_ring_bytes=RING, gpu_tick_interval_s=0.005, **kw))
    removed = []
    real_remove = broker.remove_user

    async def remove_user(pubkey):
        removed.append(pubkey)
        await real_remove(pubkey)

    broker.remove_user = remove_user
    await broker.start()
    await broker.discovery.perform_heartbeat(0, 60)
    marshal = Marshal(MarshalConfig(bind_endpoint=mar, discovery_endpoint=db, protocol=Tcp))
    await marshal.start()

    def client(seed, topics):
        return Client(ClientConfig(endpoint=mar, keypair=bls.KeyPair.from_seed(seed),
                                   subscribed_topics=topics, protocol=Tcp))

    sender, a, b = client(81, [9]), client(82, [T1]), client(83, [T2])
    for c in (sender, a, b):
        await c.ensure_initialized()
    await until(lambda: len(broker.connections.users) == 3, "three users")
    return broker, marshal, removed, sender, a, b


def test_evict_removes_the_subscriber_that_lost_data(tmp_path):
    from tests.test_integration import stop_stack

    async def go():
        broker, marshal, removed, sender, a, b = await stack(
            tmp_path, 25650, gpu_overflow_policy="evict")
        assert broker._engine.loss_accounting
        before = counters()
        await sender.send_broadcast_message([T1], BIG)
        await until(lambda: moved(before)["GPU_RING_EVICTIONS"] == 1, "the eviction")
        assert moved(before) == {"GPU_RING_LOST_BYTES": big_record(),
                                 "GPU_RING_OVERFLOWS": 1, "GPU_RING_EVICTIONS": 1}
        assert set(removed) == {a.public_key}
        # B, on another topic, is untouched
        assert b.public_key in broker.connections.users
        await sender.send_broadcast_message([T2], b"for-b")
        assert await recv(b) == b"for-b"
        assert moved(before)["GPU_RING_EVICTIONS"] == 1
        ticks = [t for t in broker._tasks if t.get_name() == "gpu-tick"]
        assert len(ticks) == 1 and not ticks[0].done()
        await stop_stack([broker], marshal, sender, a, b)

    run(go())


def test_count_reports_the_loss_and_keeps_the_subscriber(tmp_path):
    from tests.test_integration import stop_stack

    async def go():
        broker, marshal, removed, sender, a, b = await stack(
            tmp_path, 25655, gpu_overflow_policy="count")
        assert broker._engine.loss_accounting
        before = counters()
        await sender.send_broadcast_message([T1], BIG)
        await until(lambda: moved(before)["GPU_RING_OVERFLOWS"] == 1, "the overflow")
        assert moved(before) == {"GPU_RING_LOST_BYTES": big_record(),
                                 "GPU_RING_OVERFLOWS": 1, "GPU_RING_EVICTIONS": 0}
        # A stays connected and keeps receiving
        await sender.send_broadcast_message([T1], b"small")
        assert await recv(a) == b"small"
        assert removed == [] and a.public_key in broker.connections.users
        assert moved(before)["GPU_RING_OVERFLOWS"] == 1
        await stop_stack([broker], marshal, sender, a, b)

    run(go())


def test_default_is_ignore_and_ignore_builds_no_accounting(tmp_path):
    from tests.test_integration import stop_stack
    from pushcdn_amd.broker.service import BrokerConfig

    assert BrokerConfig.__dataclass_fields__["gpu_overflow_policy"].default == "ignore"

    async def go():
        broker, marshal, removed, sender, a, b = await stack(tmp_path, 25660)
        eng = broker._engine
        assert not eng.loss_accounting and eng._acct_ops is None
        assert not hasattr(eng, "demand")
        before = counters()
        await sender.send_broadcast_message([T1], BIG)
        # the marker is routed after BIG: once it arrives BIG's tick has drained
        await sender.send_broadcast_message([T1], b"marker")
        assert await recv(a) == b"marker"
        assert moved(before) == {"GPU_RING_LOST_BYTES": 0, "GPU_RING_OVERFLOWS": 0,
                                 "GPU_RING_EVICTIONS": 0}
        assert removed == []
        await stop_stack([broker], marshal, sender, a, b)

    run(go())


def test_an_unknown_policy_is_refused(tmp_path):
    from pushcdn_amd.broker.service import Broker, BrokerConfig

    cfg = BrokerConfig(public_bind_endpoint="p", public_advertise_endpoint="p",
                       private_bind_endpoint="q", private_advertise_endpoint="q",
                       gpu_overflow_policy="retry")
    with pytest.raises(ValueError, match="gpu_overflow_policy"):
        Broker(cfg)


def test_the_mesh_broker_opts_out():
    from pushcdn_amd.broker.mesh_service import MeshBroker
    from pushcdn_amd.broker.service import Broker

    assert Broker.OVERFLOW_POLICY is True and MeshBroker.OVERFLOW_POLICY is False


def test_cli_flag_reaches_the_config(monkeypatch):
    import argparse

    from pushcdn_amd import cli
    from pushcdn_amd.broker import service

    seen = []

    class FakeBroker:
        def __init__(self, cfg):
            seen.append(cfg.gpu_overflow_policy)

        async def run_forever(self):
            return None

    monkeypatch.setattr(service, "Broker", FakeBroker)
    for argv, want in (([], "ignore"), (["--gpu-overflow-policy", "count"], "count"),
                       (["--gpu-overflow-policy", "evict"], "evict")):
        parser = argparse.ArgumentParser()
        cli._broker_args(parser)
        cli.cmd_broker(parser.parse_args(argv))
        assert seen[-1] == want
