"""By-reference delivery on the device: k3_fanout_ref against its model on
sentinel-filled egress, the cuda engine against the CPU engine, and the
service over native TCP.  Populations and batches come from
tests/test_byref_cpu.py."""

import asyncio

import numpy as np
import pytest
import torch

from pushcdn_amd.broker.gpu_engine import parse_ring_records, ring_rec
from pushcdn_amd.ops import reference as ref
from pushcdn_amd.proto import message as m
from tests.test_byref_cpu import (N_USERS, RING, THR, TOPIC, expected_rings,
                                  large_and_small_scenario, make_batch, make_engine,
                                  mixed_batch, pattern, populate, raw_headers, run,
                                  tick_task_alive, _service_config)

pytestmark = pytest.mark.gpu

SENT = 0xA5
PAIR_DT = np.dtype([("user", "<i4"), ("msg", "<i4"), ("dst", "<i8")])
REF_BASE = (1 << 33) + 8          # ref_off needs all 64 bits
# messages 0..5 inline (the lengths where the copy changes path), 6..8 by reference
LENS = [0, 1, 15, 16, 17, THR - 8, THR, 1500, 5000]
INLINE, FLAGGED = [0, 1, 2, 3, 4, 5], [6, 7, 8]


@pytest.fixture(scope="module")
def ops():
    from pushcdn_amd.ops import get_gpu_ops

    return get_gpu_ops()


class Case:
    """`msgs[i]` is the message of pair i (None: a user = -1 pair).  Every
    record gets its own slot in the egress with a 16 B sentinel gap after it."""

    def __init__(self, msgs):
        # unaligned sources: message k starts at an offset = 1, 8, 15, 3, ... mod 16
        self.poff, pos = [], 0
        for k, ln in enumerate(LENS):
            pos += (-pos % 16) + (1, 8, 15, 3)[k % 4]
            self.poff.append(pos)
            pos += ln
        self.buf = pattern(pos + 16, 11)
        self.seq = [(0xFFFFFFFC + k) & 0xFFFFFFFF for k in range(len(LENS))]  # wraps
        self.rows, dst = [], 0
        for i, mi in enumerate(msgs):
            if mi is None:
                self.rows.append((-1, FLAGGED[i % 3] if i % 2 else INLINE[i % 6], 0))
                continue
            self.rows.append((i % 7, mi, dst))
            dst += (16 if LENS[mi] >= THR else ring_rec(LENS[mi])) + 16
        self.egress_bytes = dst + 64

    def tensors(self):
        arr = np.zeros(len(self.rows), dtype=PAIR_DT)
        for i, row in enumerate(self.rows):
            arr[i] = row
        seq = torch.tensor([s - (1 << 32) if s >= (1 << 31) else s for s in self.seq],
                           dtype=torch.int32)
        return dict(
            buf=torch.frombuffer(bytearray(self.buf), dtype=torch.uint8).to("cuda"),
            poff=torch.tensor(self.poff, dtype=torch.int64, device="cuda"),
            plen=torch.tensor(LENS, dtype=torch.int32, device="cuda"),
            pairs=torch.from_numpy(arr.view("<i4").reshape(-1, 4).copy()).to("cuda"),
            seq=seq.to("cuda"), seq_host=seq)

    def expected(self):
        want = bytearray([SENT]) * self.egress_bytes
        ref.fanout_ref(self.buf, torch.tensor(self.poff, dtype=torch.int64),
                       torch.tensor(LENS, dtype=torch.int32),
                       torch.tensor([r[0] for r in self.rows], dtype=torch.int32),
                       torch.tensor([r[1] for r in self.rows], dtype=torch.int32),
                       torch.tensor([r[2] for r in self.rows], dtype=torch.int64),
                       torch.tensor(self.seq, dtype=torch.int64), want, THR, REF_BASE)
        return bytes(want)


def _run_layout(layout):
    i, f = INLINE, FLAGGED
    if layout == "run64":
        # three inline pairs, a run of 64 flagged ones across both groups,
        # then three inline pairs in the partial second group
        msgs = [i[0], i[1], i[2]] + [f[k % 3] for k in range(64)] + [i[3], i[4], i[5]]
    elif layout == "mixed":
        # lone flagged pairs between inline ones, user = -1 pairs of both kinds
        unit = [i[0], f[0], i[1], None, i[2], i[5], f[1], i[3], None, i[4]]
        msgs = unit * 7
        assert msgs[1] in f and msgs[0] in i and msgs[2] in i
    elif layout == "run64x5":
        # the same runs where a wave owns 64 pairs: they cross group borders
        msgs = _run_layout("run64") * 5
    else:
        # more than 4 groups of 64: with grid=1 (4 waves) the stride loop repeats
        unit = [i[5], f[2], None, i[4], f[0], f[1], i[0], i[1], i[2], i[3], None]
        msgs = unit * 30
        assert len(msgs) > 4 * 64
    return msgs


@pytest.mark.parametrize("grid", [1, 3, 0])
@pytest.mark.parametrize("layout", ["run64", "mixed", "run64x5", "stride"])
def test_fanout_ref_sentinel(ops, layout, grid):
    """Exact equality with the model over the whole sentinel-filled egress,
    nt 0 and 1, then once more with *n_pairs above capacity.  The kernel
    packs G pairs per wave, G the smallest power of two at which one step of
    the grid covers the list: with 70 pairs grid=1 (4 waves) gives G = 32
    and a partial last group, grid=3 gives G = 8, the default grid G = 1;
    the two longer layouts reach G = 64, and with grid=1 the stride loop."""
    msgs = _run_layout(layout)
    if layout in ("run64", "mixed"):
        assert len(msgs) == 70
    case = Case(msgs)
    want = case.expected()
    d = case.tensors()
    n = len(case.rows)
    for nt in (0, 1):
        for claimed in (n, n + 1000):
            egress = torch.full((case.egress_bytes,), SENT, dtype=torch.uint8, device="cuda")
            n_pairs = torch.tensor([claimed], dtype=torch.int32, device="cuda")
            ops.fanout_ref(d["buf"], d["poff"], d["plen"], d["pairs"], d["seq"], n_pairs,
                           egress, nt, grid, THR, REF_BASE)
            got = bytes(egress.cpu().numpy().tobytes())
            if got != want:
                at = next(k for k in range(len(want)) if got[k] != want[k])
                raise AssertionError(f"{layout} grid={grid} nt={nt} n_pairs={claimed}: first "
                                     f"difference at byte {at}")


def test_fanout_ref_below_threshold_equals_fanout_wave(ops):
    """With no message at the threshold the kernel is the wave kernel."""
    case = Case(_run_layout("mixed"))
    d = case.tensors()
    n_pairs = torch.tensor([len(case.rows)], dtype=torch.int32, device="cuda")
    out = []
    for call in ("ref", "wave"):
        egress = torch.full((case.egress_bytes + 8192 * 70,), SENT, dtype=torch.uint8,
                            device="cuda")
        # spread the records: inline copies of the 5000-byte message need room
        pairs = d["pairs"].clone()
        rows = [(u, mi, k * 8192) for k, (u, mi, _d) in enumerate(case.rows)]
        arr = np.zeros(len(rows), dtype=PAIR_DT)
        for k, row in enumerate(rows):
            arr[k] = row
        pairs.copy_(torch.from_numpy(arr.view("<i4").reshape(-1, 4).copy()))
        if call == "ref":
            ops.fanout_ref(d["buf"], d["poff"], d["plen"], pairs, d["seq"], n_pairs, egress,
                           1, 1, 1 << 20, 0)
        else:
            ops.fanout_wave(d["buf"], d["poff"], d["plen"], pairs, d["seq"], n_pairs, egress,
                            1, 1)
        out.append(egress.cpu())
    assert torch.equal(out[0], out[1])


# ------------------------- engine: cuda against cpu -------------------------

def _tick(eng, msgs, origin=None):
    batch, offsets = make_batch(msgs)
    if origin is None:
        buf, off = eng.ingest(batch, offsets)
    else:
        buf, off, origin = eng.ingest(batch, offsets, origin=origin)
    stats = eng.tick(buf, off, host_batch=batch, host_offsets=offsets, origin=origin)
    if eng.use_gpu_ops:
        torch.cuda.synchronize()
        return int(eng._drops.cpu()[0])
    return stats.n_drops


def _drain(eng):
    """(cursors, {ring: seq-sorted [(seq, bytes)]}, {ring: seq-sorted headers})."""
    wpos, offsets, staging, refbuf = eng.drain_compact_ref()
    recs, hdrs = {}, {}
    for r in range(eng.n_recipients):
        n = int(wpos[r])
        if n:
            ring = bytes(staging[int(offsets[r]):int(offsets[r + 1])].numpy().tobytes())
            recs[r] = parse_ring_records(ring, n, refbuf)
            hdrs[r] = sorted(raw_headers(ring, n), key=lambda h: h[2])
    return wpos.tolist(), recs, hdrs


def test_engine_cuda_matches_cpu_engine():
    msgs, origin = mixed_batch()
    out = {}
    for dev in ("cpu", "cuda:0"):
        eng = make_engine(device=dev)
        populate(eng)
        drops = _tick(eng, msgs, origin)
        # a second tick before the drain: offsets continue in the joined buffer
        drops2 = _tick(eng, [m.Broadcast([TOPIC], pattern(2000, 7)),
                             m.Broadcast([TOPIC], b"tiny")])
        out[dev] = (drops, drops2) + _drain(eng)
    assert out["cpu"] == out["cuda:0"]
    assert out["cuda:0"][:2] == (0, 0)
    want = expected_rings(msgs)
    got = {r: [p for _s, p in v][:len(want[r])] for r, v in out["cuda:0"][3].items()}
    assert got == want


def test_engine_130_reference_only_deliveries():
    big = m.Broadcast([TOPIC], pattern(3000, 12))
    out = {}
    for dev in ("cpu", "cuda:0"):
        eng = make_engine(device=dev, n_users=130, n_peer_slots=0, direct_table_size=64)
        eng.subscribe_all([TOPIC])
        drops = _tick(eng, [big])
        out[dev] = (drops,) + _drain(eng)
    assert out["cpu"] == out["cuda:0"]
    drops, wpos, recs, hdrs = out["cuda:0"]
    assert drops == 0 and wpos == [16] * 130
    wire = m.serialize(big)
    assert all(recs[r] == [(0, wire)] for r in range(130))
    assert all(hdrs[r] == [(True, len(wire), 0, 0)] for r in range(130))


def test_8k_message_reaches_every_recipient_of_a_4k_ring():
    eng = make_engine(device="cuda:0")
    populate(eng)
    big = m.Broadcast([TOPIC], pattern(8192, 3))
    assert len(m.serialize(big)) > RING
    assert _tick(eng, [big]) == 0
    _wpos, recs, _hdrs = _drain(eng)
    wire = m.serialize(big)
    assert recs == {r: [(0, wire)] for r in (0, 1, 2, N_USERS)}


def test_uniform_lengths_and_graph_path_with_a_threshold():
    """A uniform_wire_len below the threshold keeps the flat path and gives
    inline records; one at or above it goes by reference; tick_graphed
    refuses such a length."""
    eng = make_engine(device="cuda:0", direct_enabled=False)
    populate(eng)
    for body, by_ref in ((b"s" * 100, False), (pattern(2000, 1), True)):
        msgs = [m.Broadcast([TOPIC], body)] * 3
        batch, offsets = make_batch(msgs)
        buf, off = eng.ingest(batch, offsets)
        eng.tick(buf, off, host_batch=batch, host_offsets=offsets,
                 uniform_wire_len=offsets[1])
        _wpos, recs, hdrs = _drain(eng)
        assert [p for _s, p in recs[0]] == [m.serialize(x) for x in msgs]
        assert [h[0] for h in hdrs[0]] == [by_ref] * 3
    with pytest.raises(ValueError):
        eng.tick_graphed(buf, off, offsets[1])


# --------------------------------- service ---------------------------------

def test_service_large_messages_over_native_tcp_cuda(tmp_path):
    from pushcdn_amd.broker.service import Broker
    from pushcdn_amd.client import Client, ClientConfig
    from pushcdn_amd.crypto import bls
    from pushcdn_amd.discovery import BrokerIdentifier
    from pushcdn_amd.marshal import Marshal, MarshalConfig
    from pushcdn_amd.proto.transports.tcp_native import TcpNative

    async def go():
        db = str(tmp_path / "byref-cuda.db")
        broker = Broker(_service_config(
            db, "x", TcpNative, gpu_device="cuda:0",
            public_bind_endpoint="127.0.0.1:0", public_advertise_endpoint="127.0.0.1:0",
            private_bind_endpoint="127.0.0.1:0", private_advertise_endpoint="127.0.0.1:0"))
        await broker.start()
        pub = f"127.0.0.1:{broker._user_listener.port}"
        priv = f"127.0.0.1:{broker._broker_listener.port}"
        broker.config.public_advertise_endpoint = pub
        broker.config.private_advertise_endpoint = priv
        broker.identity = BrokerIdentifier(pub, priv)
        broker.discovery.identity = broker.identity
        broker.connections.identity = broker.identity
        await broker.discovery.perform_heartbeat(0, 600)
        marshal = Marshal(MarshalConfig(bind_endpoint="127.0.0.1:0",
                                        discovery_endpoint=db, protocol=TcpNative))
        await marshal.start()
        ep = f"127.0.0.1:{marshal._listener.port}"

        def client(endpoint, seed, topics):
            return Client(ClientConfig(endpoint=endpoint, keypair=bls.KeyPair.from_seed(seed),
                                       subscribed_topics=list(topics), protocol=TcpNative))

        clients = await large_and_small_scenario(ep, client)
        assert tick_task_alive(broker)
        for c in clients:
            c.close()
        await marshal.close()
        await broker.close()

    run(go())
