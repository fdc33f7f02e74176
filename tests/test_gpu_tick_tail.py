"""The tail of the fused uniform broadcast tick: drain_cursors storing the
cursors straight into the engine's pinned buffer, and the one fan-out launch
(k3_fanout_dense_tail_t) whose last workgroups walk the sparse pair list
behind the dense tiles.

As in test_gpu_fused_tick.py, three engines run the same batches: the CPU
oracle, the fused GPU engine, and the GPU engine with fused_tick=False (the
per-op path: flat fan-out alone, torch drain).  Rings are prefilled with 0xA5
and the WHOLE egress tensor is compared, so a store past a cursor or a
missing store shows.  The expected image is the CPU engine's with the pad of
every delivered record zeroed (the uniform GPU path writes full strides).

Wire lengths: 64 bytes (80-byte records, 5 units) is the smallest Broadcast
that delivers; 1104 bytes (1120-byte records) makes a 32-message block two
dense chunks."""

import random

import pytest
import torch

from pushcdn_amd.broker.gpu_engine import GpuBrokerEngine, ring_rec
from pushcdn_amd.proto import message as m

pytestmark = pytest.mark.gpu

SENT = 0xA5


def uniform_batch(M, wire_len, topic_of, seed):
    """M Broadcasts of exactly wire_len bytes each, message i on topic
    topic_of(i)."""
    rng = random.Random(seed)
    payload = (wire_len - 56) // 8 * 8
    parts = []
    for i in range(M):
        raw = m.serialize(m.Broadcast([topic_of(i)], rng.randbytes(payload)))
        assert len(raw) <= wire_len, (len(raw), wire_len)
        parts.append(raw + bytes(wire_len - len(raw)))
    return b"".join(parts), [i * wire_len for i in range(M + 1)]


def make_engines(n_users, ring_bytes, subscribe, cpu=True, **kw):
    """(cpu oracle or None, fused GPU engine, per-op GPU engine), same
    population, rings prefilled with the sentinel."""
    common = dict(n_users=n_users, ring_bytes=ring_bytes, direct_table_size=64,
                  fanout_wire=True)
    oracle = GpuBrokerEngine(device="cpu", use_gpu_ops=False, **common) if cpu else None
    gkw = dict(device="cuda:0", direct_enabled=False, pair_capacity=1 << 15, **common)
    gkw.update(kw)
    fused = GpuBrokerEngine(fused_tick=True, **gkw)
    plain = GpuBrokerEngine(fused_tick=False, **gkw)
    for eng in (oracle, fused, plain):
        if eng is not None:
            subscribe(eng)
            eng.egress.fill_(SENT)
    return oracle, fused, plain


def tick_all(engines, batch, offsets, wire_len):
    """One tick on every engine; returns the CPU engine's drop count."""
    cpu, fused, plain = engines
    drops = None
    if cpu is not None:
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


def assert_egress_equal(name, got, want, ring_bytes):
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want).flatten()
        first = int(bad[0])
        pytest.fail(f"{name}: {bad.numel()} egress bytes differ, first at ring "
                    f"{first // ring_bytes} offset {first % ring_bytes}")


def assert_same(engines, wire_len, cpu_drops):
    cpu, fused, plain = engines
    torch.cuda.synchronize()
    want = expected_egress(cpu, wire_len)
    for name, eng in (("fused", fused), ("per-op", plain)):
        assert torch.equal(eng.ring_wpos.cpu(), cpu.ring_wpos), name
        assert int(eng._drops.cpu()[0]) == cpu_drops, name
        assert eng.seq == cpu.seq, name
        assert_egress_equal(name, eng.egress.cpu(), want, cpu.ring_bytes)
    assert fused.fused_ticks > 0 and plain.fused_ticks == 0


def n_sparse(eng):
    return int(eng._n_sparse.cpu()[0])


# populations: how user u subscribes, and the topic of message i
def sub_dense(eng):
    eng.subscribe_all([0, 1])


def sub_modulo8(eng):
    eng.subscribe_modulo(8)


def sub_mixed(eng):
    """Dense, sparse and empty tiles for neighbouring users of a mask word."""
    for u in range(eng.n_users):
        if u % 3 == 0:
            eng.subscribe(u, [0, 1, 2, 3])
        elif u % 3 == 1:
            eng.subscribe(u, [u % 4])


# ------------------------------- drain --------------------------------------

class CountingOps:
    """The native module with drain_cursors counted."""

    def __init__(self, ops):
        self._ops = ops
        self.drains = 0

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def drain_cursors(self, *args):
        self.drains += 1
        return self._ops.drain_cursors(*args)


@pytest.mark.parametrize("n_users", [1, 64, 255, 256, 257])
def test_drain_rounds(n_users):
    """Three rounds of tick then drain, user u on topic u % 3 and a different
    number of messages each round: every round's cursors differ from the last
    round's and between users.  Each drain returns the oracle's cursors in a
    fresh tensor, zeroes the device cursors, and leaves every tensor returned
    earlier as it was."""
    wire_len = 64
    rec = ring_rec(wire_len)

    def subscribe(eng):
        for u in range(n_users):
            eng.subscribe(u, [u % 3])

    engines = make_engines(n_users, 8 * rec, subscribe)
    fused = engines[1]
    fused._ops = CountingOps(fused._ops)
    kept = []
    for rnd, M in enumerate([4, 7, 2]):
        batch, offsets = uniform_batch(M, wire_len, lambda i: i % 3, seed=rnd)
        assert tick_all(engines, batch, offsets, wire_len) == 0
        want = engines[0].drain_cursors()
        assert want.tolist() == [len(range(u % 3, M, 3)) * rec for u in range(n_users)]
        for eng in engines[1:]:
            got = eng.drain_cursors()
            assert got.device.type == "cpu" and got.dtype == want.dtype
            assert torch.equal(got, want)
            assert int(eng.ring_wpos.abs().sum()) == 0
            kept.append((got, want.tolist()))
    assert fused._ops.drains == 3
    for got, want in kept:
        assert got.tolist() == want
    assert len({got.data_ptr() for got, _ in kept}) == len(kept)


def test_drain_without_a_tick():
    eng = GpuBrokerEngine(device="cuda:0", n_users=130, ring_bytes=1 << 10,
                          direct_table_size=64, fanout_wire=True, direct_enabled=False)
    first = eng.drain_cursors()
    assert first.tolist() == [0] * 130 and first.dtype == torch.int64
    assert eng.drain_cursors().tolist() == [0] * 130
    assert int(eng.ring_wpos.abs().sum()) == 0


def test_two_engines_drained_alternately():
    """Each engine has a pinned buffer of its own: draining one does not
    disturb what the other returns or returned."""
    wire_len = 64
    rec = ring_rec(wire_len)
    a = make_engines(70, 8 * rec, sub_dense)
    b = make_engines(130, 8 * rec, sub_modulo8)
    kept = []
    for rnd, (ma, mb) in enumerate([(3, 8), (5, 2)]):
        for engines, M in ((a, ma), (b, mb)):
            batch, offsets = uniform_batch(M, wire_len, lambda i: i % 2, seed=rnd)
            assert tick_all(engines, batch, offsets, wire_len) == 0
        want_a, want_b = a[0].drain_cursors(), b[0].drain_cursors()
        assert want_a.tolist() == [ma * rec] * 70
        got_a = a[1].drain_cursors()
        got_b = b[1].drain_cursors()
        assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)
        kept += [(got_a, want_a), (got_b, want_b)]
        a[2].drain_cursors()
        b[2].drain_cursors()
    for got, want in kept:
        assert torch.equal(got, want)


def test_direct_enabled_engine_drains_natively():
    """direct_enabled keeps the ticks on the per-op path; the drain is the
    native op all the same."""
    M, wire_len, n_users = 5, 64, 130
    rec = ring_rec(wire_len)
    common = dict(n_users=n_users, ring_bytes=8 * rec, direct_table_size=64, fanout_wire=True)
    cpu = GpuBrokerEngine(device="cpu", use_gpu_ops=False, **common)
    eng = GpuBrokerEngine(device="cuda:0", direct_enabled=True, **common)
    eng._ops = CountingOps(eng._ops)
    for e in (cpu, eng):
        e.subscribe_modulo(8)
    batch, offsets = uniform_batch(M, wire_len, lambda i: i % 8, seed=11)
    for e in (cpu, eng):
        bd, od = e.ingest(batch, offsets)
        e.tick(bd, od, host_batch=batch, host_offsets=offsets, uniform_wire_len=wire_len)
    want = cpu.drain_cursors()
    got = eng.drain_cursors()
    assert eng.fused_ticks == 0 and eng._ops.drains == 1
    assert want.tolist() == [rec if u % 8 < M else 0 for u in range(n_users)]
    assert torch.equal(got, want)
    assert int(eng.ring_wpos.abs().sum()) == 0


# ------------------------ the one fan-out launch ----------------------------

@pytest.mark.parametrize("nt", [True, False])
@pytest.mark.parametrize("n_users", [1, 8, 9, 65])
@pytest.mark.parametrize("M", [1, 32, 33])
def test_all_dense_leaves_the_tail_idle(M, n_users, nt):
    """Every tile dense, n_sparse == 0: the tail workgroups write nothing."""
    wire_len = 1104
    engines = make_engines(n_users, (M + 1) * ring_rec(wire_len), sub_dense, nt_fanout=nt)
    batch, offsets = uniform_batch(M, wire_len, lambda i: i % 2, seed=M)
    drops = tick_all(engines, batch, offsets, wire_len)
    assert_same(engines, wire_len, drops)
    assert drops == 0 and n_sparse(engines[1]) == 0
    assert engines[0].ring_wpos.tolist() == [M * ring_rec(wire_len)] * n_users


@pytest.mark.parametrize("nt", [True, False])
@pytest.mark.parametrize("n_users", [1, 8, 9, 65])
@pytest.mark.parametrize("M", [32, 70])
def test_all_sparse_behind_no_dense_tile(M, n_users, nt):
    """User u on topic u % 8, message i on topic i % 8, dense fan-out left
    on: no user takes a whole block (the last block of M = 70 has six
    messages on six topics), so the tail carries every delivery."""
    wire_len = 1104
    engines = make_engines(n_users, M * ring_rec(wire_len), sub_modulo8, nt_fanout=nt)
    assert engines[1]._dense_fanout
    batch, offsets = uniform_batch(M, wire_len, lambda i: i % 8, seed=M)
    drops = tick_all(engines, batch, offsets, wire_len)
    assert_same(engines, wire_len, drops)
    deliveries = sum(len(range(u % 8, M, 8)) for u in range(n_users))
    assert drops == 0 and n_sparse(engines[1]) == deliveries


@pytest.mark.parametrize("nt", [True, False])
@pytest.mark.parametrize("n_users", [1, 8, 9, 65])
@pytest.mark.parametrize("M", [1, 32, 33])
def test_dense_sparse_and_empty_tiles_in_one_mask_word(M, n_users, nt):
    wire_len = 1104
    engines = make_engines(n_users, M * ring_rec(wire_len), sub_mixed, nt_fanout=nt)
    batch, offsets = uniform_batch(M, wire_len, lambda i: i % 4, seed=M)
    drops = tick_all(engines, batch, offsets, wire_len)
    assert_same(engines, wire_len, drops)
    assert drops == 0
    if M >= 32 and n_users >= 2:
        assert n_sparse(engines[1]) > 0


@pytest.mark.parametrize("nt", [True, False])
def test_dense_fanout_off_runs_the_flat_kernel_alone(nt):
    M, wire_len, n_users = 33, 1104, 65
    engines = make_engines(n_users, M * ring_rec(wire_len), sub_mixed, nt_fanout=nt)
    engines[1]._dense_fanout = False
    batch, offsets = uniform_batch(M, wire_len, lambda i: i % 4, seed=5)
    drops = tick_all(engines, batch, offsets, wire_len)
    assert_same(engines, wire_len, drops)
    assert drops == 0
    assert n_sparse(engines[1]) == sum(w // ring_rec(wire_len)
                                       for w in engines[0].ring_wpos.tolist())


@pytest.mark.parametrize("nt", [True, False])
def test_pair_capacity_clamps_the_tail_beside_dense_tiles(nt):
    """64 users: even ones take all four topics (64 deliveries each, dense
    tiles), odd ones topic u % 4 (16 each, 512 sparse claims in all); a pair
    capacity of 300 runs out inside user 6's claim.  With one mask word both
    engines make every claim in one wave, in lane order (the same
    k2b_p2_body), so which records are lost is the same on both and the
    per-op engine is a byte-for-byte reference.  The invariants of
    test_pair_capacity_invariants are checked as well: every ring holds a
    prefix of its user's record stream and the sentinel after its cursor."""
    M, wire_len, n_users, capacity = 64, 64, 64, 300
    rec = ring_rec(wire_len)

    def subscribe(eng):
        for u in range(n_users):
            eng.subscribe(u, [0, 1, 2, 3] if u % 2 == 0 else [u % 4])

    _, fused, plain = make_engines(n_users, M * rec, subscribe, cpu=False,
                                   pair_capacity=capacity, nt_fanout=nt)
    batch, offsets = uniform_batch(M, wire_len, lambda i: i % 4, seed=12)
    tick_all((None, fused, plain), batch, offsets, wire_len)
    torch.cuda.synchronize()
    assert fused.fused_ticks == 1 and plain.fused_ticks == 0
    wpos = fused.ring_wpos.cpu()
    drops = int(fused._drops.cpu()[0])
    assert torch.equal(wpos, plain.ring_wpos.cpu())
    assert drops == int(plain._drops.cpu()[0])
    assert int(wpos.sum()) // rec == capacity
    assert drops == 32 * 64 + 32 * 16 - capacity
    assert wpos.tolist()[:7] == [64 * rec, 16 * rec, 64 * rec, 16 * rec, 64 * rec, 16 * rec,
                                 60 * rec]
    assert 0 < n_sparse(fused) <= capacity
    got = fused.egress.cpu()
    assert_egress_equal("fused vs per-op", got, plain.egress.cpu(), M * rec)
    rings = got.view(n_users, M * rec)
    for u, w in enumerate(wpos.tolist()):
        stream = b""
        for i in range(M):
            if u % 2 == 0 or i % 4 == u % 4:
                stream += (wire_len.to_bytes(4, "little") + i.to_bytes(4, "little") + bytes(8)
                           + batch[offsets[i]:offsets[i + 1]])
        want = torch.frombuffer(bytearray(stream), dtype=torch.uint8)
        assert torch.equal(rings[u, :w], want[:w]), f"user {u}: not a prefix"
        assert bool((rings[u, w:] == SENT).all()), f"user {u}: bytes past the cursor"


def test_sparse_list_longer_than_one_pass_of_the_tail():
    """More 16-byte units in the sparse list than the tail has threads, so
    its workgroups go round their grid-stride loop more than once: 64-byte
    wire messages (5 units a record), 2048 messages, user u on topic u % 8,
    and as many users as that takes.  Fused against per-op only: the oracle
    would take too long at a million deliveries, and the other tests tie the
    per-op engine to it."""
    from pushcdn_amd.ops import get_gpu_ops

    tail_threads = get_gpu_ops()._SPARSE_TAIL_BLOCKS * 256
    M, wire_len = 2048, 64
    rec = ring_rec(wire_len)
    units = rec // 16
    per_user = M // 8
    n_users = (tail_threads // units) // per_user + 8
    n_users -= n_users % 8                      # every topic the same number of users
    deliveries = n_users * per_user
    assert deliveries * units > tail_threads
    _, fused, plain = make_engines(n_users, per_user * rec, sub_modulo8, cpu=False,
                                   pair_capacity=deliveries)
    batch, offsets = uniform_batch(M, wire_len, lambda i: i % 8, seed=13)
    tick_all((None, fused, plain), batch, offsets, wire_len)
    torch.cuda.synchronize()
    assert fused.fused_ticks == 1 and n_sparse(fused) == deliveries
    assert int(fused._drops.cpu()[0]) == 0 == int(plain._drops.cpu()[0])
    assert fused.ring_wpos.cpu().tolist() == [per_user * rec] * n_users
    assert torch.equal(fused.ring_wpos.cpu(), plain.ring_wpos.cpu())
    assert_egress_equal("fused vs per-op", fused.egress.cpu(), plain.egress.cpu(),
                        per_user * rec)
