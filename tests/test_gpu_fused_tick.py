"""The fused uniform broadcast tick (tick_uniform_broadcast: K2b tiles, the
dense fan-out, the sparse pair list) and the fused drain, against the CPU
engine and against the same GPU engine with fused_tick=False.

Both engines' rings are prefilled with 0xA5 and the WHOLE egress tensor is
compared, so a store past a cursor or an unwritten pad byte shows.  The
uniform GPU path writes every record at full stride (pad bytes past the
message as zeros, ops.reference.fanout's zero_pad_to contract); the CPU
engine writes 16 + len bytes per record, so the expected image is the CPU
engine's with the pad of every delivered record zeroed.

A serialized Broadcast is at least 56 bytes, so the 16- and 48-byte wire
lengths (32- and 64-byte records) cannot carry one: those batches are bytes
K4 rejects and every engine must deliver nothing.  The 64-byte wire length
(80-byte records) is the smallest that delivers."""

import random

import pytest
import torch

from pushcdn_amd.broker.gpu_engine import GpuBrokerEngine, ring_rec
from pushcdn_amd.proto import message as m

pytestmark = pytest.mark.gpu

SENT = 0xA5


def uniform_batch(M, wire_len, topic_of, seed, pad_byte=0):
    """M Broadcasts of exactly wire_len bytes each (the serialized message
    plus trailing bytes the parser never reads), message i on topic
    topic_of(i); bytes no parser accepts when wire_len cannot hold one."""
    rng = random.Random(seed)
    if wire_len < 64:
        buf = rng.randbytes(M * wire_len)
    else:
        payload = (wire_len - 56) // 8 * 8
        buf = b""
        for i in range(M):
            raw = m.serialize(m.Broadcast([topic_of(i)], rng.randbytes(payload)))
            assert len(raw) <= wire_len, (len(raw), wire_len)
            buf += raw + bytes([pad_byte]) * (wire_len - len(raw))
    return buf, [i * wire_len for i in range(M + 1)]


def make_engines(n_users, ring_bytes, subscribe, **kw):
    """(cpu oracle, fused GPU engine, per-op GPU engine), same population,
    rings prefilled with the sentinel."""
    common = dict(n_users=n_users, ring_bytes=ring_bytes, direct_table_size=64,
                  fanout_wire=True)
    cpu = GpuBrokerEngine(device="cpu", use_gpu_ops=False, **common)
    gkw = dict(device="cuda:0", direct_enabled=False, pair_capacity=1 << 15, **common)
    gkw.update(kw)
    fused = GpuBrokerEngine(fused_tick=True, **gkw)
    plain = GpuBrokerEngine(fused_tick=False, **gkw)
    for eng in (cpu, fused, plain):
        subscribe(eng)
        eng.egress.fill_(SENT)
    return cpu, fused, plain


def tick_all(engines, batch, offsets, wire_len):
    """One tick on every engine; returns the CPU engine's drop count."""
    cpu, fused, plain = engines
    bc, oc = cpu.ingest(batch, offsets)
    drops = cpu.tick(bc, oc, host_batch=batch, host_offsets=offsets).n_drops
    for eng in (fused, plain):
        bg, og = eng.ingest(batch, offsets)
        eng.tick(bg, og, uniform_wire_len=wire_len)
    return drops


def expected_egress(cpu, wire_len):
    """The CPU engine's rings with each delivered record's pad zeroed."""
    rec = ring_rec(wire_len)
    want = cpu.egress.clone()
    if rec > 16 + wire_len:
        rings = want.view(cpu.n_users, cpu.ring_bytes)
        for u, wpos in enumerate(cpu.ring_wpos.tolist()):
            recs = rings[u, :wpos].view(-1, rec)
            recs[:, 16 + wire_len:] = 0
    return want


def assert_same(engines, wire_len, cpu_drops):
    cpu, fused, plain = engines
    torch.cuda.synchronize()
    want = expected_egress(cpu, wire_len)
    for name, eng in (("fused", fused), ("per-op", plain)):
        assert torch.equal(eng.ring_wpos.cpu(), cpu.ring_wpos), name
        assert int(eng._drops.cpu()[0]) == cpu_drops, name
        assert eng.seq == cpu.seq, name
        got = eng.egress.cpu()
        if not torch.equal(got, want):
            bad = torch.nonzero(got != want).flatten()
            first = int(bad[0])
            pytest.fail(f"{name}: {bad.numel()} egress bytes differ, first at ring "
                        f"{first // cpu.ring_bytes} offset {first % cpu.ring_bytes}")
    assert fused.fused_ticks > 0 and plain.fused_ticks == 0


def sub_all(topics):
    def f(eng):
        eng.subscribe_all(topics)
    return f


# --------------------------- 1. dense tiles ---------------------------------

@pytest.mark.parametrize("wire_len", [16, 48, 64, 1104, 4080])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 70])
def test_dense_tiles(M, wire_len):
    """Every user on every topic: all tiles dense (full and partial blocks),
    two ticks without a drain, rings exactly large enough for both."""
    rec = ring_rec(wire_len)
    engines = make_engines(130, 2 * M * rec, sub_all([0, 1, 2]))
    drops = 0
    for tick in range(2):
        batch, offsets = uniform_batch(M, wire_len, lambda i: i % 3, seed=10 * M + tick)
        drops += tick_all(engines, batch, offsets, wire_len)
    assert_same(engines, wire_len, drops)
    cpu, fused, _ = engines
    delivers = wire_len >= 64
    assert drops == 0
    assert cpu.ring_wpos.tolist() == [2 * M * rec if delivers else 0] * 130
    assert int(fused._n_sparse.cpu()[0]) == 0          # no pair record written


def test_dense_tiles_one_mask_word():
    """n_users = 64: one full mask word, no partial one."""
    M, wire_len = 33, 1104
    rec = ring_rec(wire_len)
    engines = make_engines(64, 2 * M * rec, sub_all([0]))
    for tick in range(2):
        batch, offsets = uniform_batch(M, wire_len, lambda i: 0, seed=tick)
        assert tick_all(engines, batch, offsets, wire_len) == 0
    assert_same(engines, wire_len, 0)
    assert engines[0].ring_wpos.tolist() == [2 * M * rec] * 64


# --------------------------- 2. mixed density -------------------------------

def test_mixed_density_in_one_mask_word():
    """Dense, sparse and empty tiles for neighbouring users: users take all
    four topics, only topic u % 4, or nothing, interleaved."""
    M, wire_len, n_users = 70, 1104, 130

    def subscribe(eng):
        for u in range(n_users):
            if u % 3 == 0:
                eng.subscribe(u, [0, 1, 2, 3])
            elif u % 3 == 1:
                eng.subscribe(u, [u % 4])

    engines = make_engines(n_users, M * ring_rec(wire_len), subscribe)
    batch, offsets = uniform_batch(M, wire_len, lambda i: i % 4, seed=2)
    drops = tick_all(engines, batch, offsets, wire_len)
    assert_same(engines, wire_len, drops)
    sparse = sum(sum(1 for i in range(M) if i % 4 == u % 4)
                 for u in range(n_users) if u % 3 == 1)
    assert drops == 0 and sparse > 0
    assert int(engines[1]._n_sparse.cpu()[0]) == sparse


# --------------------------- 3. ring limits ---------------------------------

def test_ring_limits_clip_mid_block():
    """A ring of 40 records under 70 messages: block 0 dense, block 1
    clipped, block 2 dropped; users advanced by an earlier tick clip
    earlier."""
    M, wire_len, n_users = 70, 1104, 130
    rec = ring_rec(wire_len)

    def subscribe(eng):
        eng.subscribe_all([0])
        for u in range(0, n_users, 3):
            eng.subscribe(u, [1])
        for u in range(1, n_users, 7):
            eng.subscribe(u, [2])

    engines = make_engines(n_users, 40 * rec, subscribe)
    # the earlier tick: 3 messages for every third user, 9 more for every seventh
    batch, offsets = uniform_batch(12, wire_len, lambda i: 1 if i < 3 else 2, seed=30)
    drops = tick_all(engines, batch, offsets, wire_len)
    assert drops == 0
    batch, offsets = uniform_batch(M, wire_len, lambda i: 0, seed=31)
    drops += tick_all(engines, batch, offsets, wire_len)
    assert_same(engines, wire_len, drops)
    cpu = engines[0]
    assert drops == 30 * n_users + 3 * len(range(0, n_users, 3)) + 9 * len(range(1, n_users, 7))
    assert cpu.ring_wpos.tolist() == [40 * rec] * n_users


# --------------------------- 4. pair capacity -------------------------------

def test_pair_capacity_invariants():
    """pair_capacity at about half the deliveries.  Which users lose records
    depends on the order of the span claims, so only invariants hold."""
    M, wire_len, n_users = 70, 1104, 130
    rec = ring_rec(wire_len)
    ring_bytes = M * rec
    eng = GpuBrokerEngine(device="cuda:0", n_users=n_users, ring_bytes=ring_bytes,
                          direct_table_size=64, fanout_wire=True, direct_enabled=False,
                          pair_capacity=M * n_users // 2)
    eng.subscribe_all([0])
    eng.egress.fill_(SENT)
    batch, offsets = uniform_batch(M, wire_len, lambda i: 0, seed=4)
    bg, og = eng.ingest(batch, offsets)
    eng.tick(bg, og, uniform_wire_len=wire_len)
    torch.cuda.synchronize()
    assert eng.fused_ticks == 1
    wpos = eng.ring_wpos.cpu().tolist()
    drops = int(eng._drops.cpu()[0])
    assert all(w % rec == 0 for w in wpos)
    assert sum(w // rec for w in wpos) + drops == M * n_users
    assert 0 < drops < M * n_users
    # the record stream every user expects, message order
    stream = b""
    for i in range(M):
        stream += (wire_len.to_bytes(4, "little") + i.to_bytes(4, "little") + bytes(8)
                   + batch[offsets[i]:offsets[i + 1]])
    rings = eng.egress.cpu().view(n_users, ring_bytes)
    want = torch.frombuffer(bytearray(stream), dtype=torch.uint8)
    for u, w in enumerate(wpos):
        assert torch.equal(rings[u, :w], want[:w]), f"user {u}: not a prefix"
        assert bool((rings[u, w:] == SENT).all()), f"user {u}: bytes past the cursor"


# --------------------------- 5. unaligned messages --------------------------

@pytest.mark.parametrize("wire_len", [69, 1101])
def test_unaligned_uniform_messages(wire_len):
    """One wire length that is no multiple of 16: message starts at every
    alignment, a partial tail unit in every record."""
    M = 70
    engines = make_engines(130, M * ring_rec(wire_len), sub_all([0, 1]))
    batch, offsets = uniform_batch(M, wire_len, lambda i: i % 2, seed=wire_len, pad_byte=0xEE)
    assert len({o % 16 for o in offsets}) == 16
    drops = tick_all(engines, batch, offsets, wire_len)
    assert_same(engines, wire_len, drops)
    assert drops == 0 and engines[0].ring_wpos.tolist() == [M * ring_rec(wire_len)] * 130


# --------------------------- 6. drain ---------------------------------------

def test_fused_drain():
    M, wire_len = 33, 1104
    rec = ring_rec(wire_len)
    engines = make_engines(130, M * rec, sub_all([0]))
    batch, offsets = uniform_batch(M, wire_len, lambda i: 0, seed=6)
    tick_all(engines, batch, offsets, wire_len)
    want = engines[0].drain_cursors()
    assert want.tolist() == [M * rec] * 130
    for eng in engines[1:]:
        got = eng.drain_cursors()
        assert got.device.type == "cpu" and got.dtype == want.dtype and got.shape == want.shape
        assert torch.equal(got, want)
        assert int(eng.ring_wpos.abs().sum()) == 0
        assert eng.drain_cursors().tolist() == [0] * 130    # and a fresh tensor each time
        assert got.tolist() == [M * rec] * 130
    # the next tick writes from offset 0 again
    for eng in engines:
        eng.egress.fill_(SENT)
    batch, offsets = uniform_batch(M, wire_len, lambda i: 0, seed=7)
    drops = tick_all(engines, batch, offsets, wire_len)
    assert_same(engines, wire_len, drops)


# --------------------------- 7. dispatch ------------------------------------

@pytest.mark.parametrize("kw,uniform", [
    (dict(direct_enabled=True), True),
    (dict(n_peer_slots=2), True),
    (dict(ref_threshold=4096), True),
    (dict(), False),
    (dict(fused_tick=False), True),
])
def test_dispatch_keeps_other_shapes_on_the_per_op_path(kw, uniform):
    M, wire_len = 5, 1104
    base = dict(device="cuda:0", n_users=64, ring_bytes=M * ring_rec(wire_len),
                direct_table_size=64, fanout_wire=True, direct_enabled=False)
    base.update(kw)
    eng = GpuBrokerEngine(**base)
    eng.subscribe_all([0])
    batch, offsets = uniform_batch(M, wire_len, lambda i: 0, seed=8)
    bg, og = eng.ingest(batch, offsets)
    eng.tick(bg, og, host_batch=batch, host_offsets=offsets,
             uniform_wire_len=wire_len if uniform else None)
    torch.cuda.synchronize()
    assert eng.fused_ticks == 0
    assert eng.ring_wpos.cpu()[:64].tolist() == [M * ring_rec(wire_len)] * 64


def test_dispatch_takes_the_fused_path_by_default():
    M, wire_len = 5, 1104
    eng = GpuBrokerEngine(device="cuda:0", n_users=64, ring_bytes=M * ring_rec(wire_len),
                          direct_table_size=64, fanout_wire=True, direct_enabled=False)
    eng.subscribe_all([0])
    batch, offsets = uniform_batch(M, wire_len, lambda i: 0, seed=9)
    bg, og = eng.ingest(batch, offsets)
    eng.tick(bg, og, uniform_wire_len=wire_len)
    # an explicit origin is peer-plane traffic: per-op path
    eng.tick(bg, og, uniform_wire_len=wire_len, origin=[0] * M)
    torch.cuda.synchronize()
    assert eng.fused_ticks == 1
