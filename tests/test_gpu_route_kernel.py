"""The fused tick's route kernel (k_route_word: K2a, P1, P2 with the tile
sort and P3 for one mask word per workgroup, intermediates in LDS) and its
prologue (k_tick_prologue), at the route kernel's own edges: batch sizes on
both sides of the 32-message block and of the workgroup's 256 threads, a
partial last mask word, tiles of every kind inside one word, messages that
are no Broadcast, ticks that follow each other without a drain, clipped
rings, a pair capacity reached inside a word, and the boundary to the
four-kernel chain that serves batches above ROUTE_MAX_M.

Every case runs one batch through the CPU engine, a GPU engine with
fused_tick=False and one with fused_tick=True, and compares whole rings
(sentinel-prefilled), cursors, drops and the two counters.  The harness is
tests/test_gpu_fused_tick.py's.

Wire length: a serialized Broadcast is at least 56 bytes, so 64 bytes
(80-byte records) is the smallest uniform length that delivers anything; the
batch-size cases run at 64 and also at 48, where every engine must reject
every message and deliver nothing."""

import random

import pytest
import torch

from pushcdn_amd.broker.gpu_engine import GpuBrokerEngine, ring_rec
from pushcdn_amd.ops import get_gpu_ops
from pushcdn_amd.proto import message as m
from tests.test_gpu_fused_tick import SENT, assert_same, make_engines, tick_all, uniform_batch

pytestmark = pytest.mark.gpu

WIRE = 64
REC = ring_rec(WIRE)
BLK = 32            # K2B_BLK
N_USERS = 130       # three mask words, the last one of two users


def sub_mixed(n_users):
    """Users in turn take all four topics, only topic u % 4, or nothing:
    dense, sparse and empty tiles side by side in every mask word."""
    def f(eng):
        for u in range(n_users):
            if u % 3 == 0:
                eng.subscribe(u, [0, 1, 2, 3])
            elif u % 3 == 1:
                eng.subscribe(u, [u % 4])
    return f


def batch_of(topics_of, M, seed, wire_len=WIRE, special=None):
    """M uniform messages; message i is a Broadcast on topics_of(i) (a list)
    unless special maps i to raw bytes.  Returns (batch, offsets, msg_topics)
    with msg_topics[i] None for a message nobody may receive."""
    rng = random.Random(seed)
    payload = (wire_len - 56) // 8 * 8
    buf, msg_topics = b"", []
    for i in range(M):
        if special and i in special:
            raw, topics = special[i], None
        else:
            topics = topics_of(i)
            raw = m.serialize(m.Broadcast(topics, rng.randbytes(payload)))
        assert len(raw) <= wire_len, (len(raw), wire_len)
        buf += raw + bytes(wire_len - len(raw))
        msg_topics.append(topics)
    return buf, [i * wire_len for i in range(M + 1)], msg_topics


def route_model(cpu, msg_topics, wpos_before, rec=REC):
    """What the tick must leave in the counters, from the CPU engine's
    subscriptions and cursors: n_pairs (every (user, message) match, delivered
    or not), and the sparse list as {(user, msg, dst)}: the delivered pairs
    of every tile that is not dense (a dense tile: the user takes the whole
    block and all of it is delivered)."""
    M = len(msg_topics)
    wpos_after = cpu.ring_wpos.tolist()
    n_pairs, sparse = 0, set()
    for u in range(cpu.n_users):
        col = ((cpu.sub_bitmap[:, u >> 6] >> (u & 63)) & 1).tolist()
        taken = [t is not None and any(col[x] for x in t) for t in msg_topics]
        lim = (wpos_after[u] - wpos_before[u]) // rec
        p = 0
        for m0 in range(0, M, BLK):
            blk = [i for i in range(m0, min(M, m0 + BLK)) if taken[i]]
            dense = len(blk) == min(M, m0 + BLK) - m0 and p + len(blk) <= lim
            if not dense:
                for k, i in enumerate(blk):
                    if p + k < lim:
                        sparse.add((u, i, u * cpu.ring_bytes + wpos_before[u] + (p + k) * rec))
            p += len(blk)
        n_pairs += p
    return n_pairs, sparse


def assert_counters(engines, msg_topics, wpos_before, rec=REC):
    """_n_pairs on both GPU engines, _n_sparse and the sparse list itself on
    the fused one: the model's set, grouped by user, messages in order."""
    cpu, fused, plain = engines
    n_pairs, sparse = route_model(cpu, msg_topics, wpos_before, rec)
    assert int(fused._n_pairs.cpu()[0]) == n_pairs
    assert int(plain._n_pairs.cpu()[0]) == n_pairs
    n = int(fused._n_sparse.cpu()[0])
    assert n == len(sparse)
    rows = fused._pairs[:n].cpu()
    dst = rows.view(torch.int64)[:, 1].tolist() if n else []
    got = list(zip(rows[:, 0].tolist(), rows[:, 1].tolist(), dst))
    assert set(got) == sparse
    seen, prev = set(), None
    for u, i, _d in got:
        if prev is None or u != prev[0]:
            assert u not in seen, f"user {u}'s pairs are not contiguous"
            seen.add(u)
        else:
            assert i > prev[1], f"user {u}: message {i} after {prev[1]}"
        prev = (u, i)
    return n


# --------------------------- 1. batch sizes ---------------------------------

@pytest.mark.parametrize("wire_len", [48, 64])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 255, 256, 257, 300])
def test_batch_sizes(M, wire_len):
    rec = ring_rec(wire_len)
    engines = make_engines(N_USERS, M * rec, sub_mixed(N_USERS), pair_capacity=1 << 16)
    if wire_len >= 64:
        batch, offsets, topics = batch_of(lambda i: [i % 4], M, seed=M, wire_len=wire_len)
    else:
        batch, offsets = uniform_batch(M, wire_len, None, seed=M)
        topics = [None] * M
    drops = tick_all(engines, batch, offsets, wire_len)
    assert_same(engines, wire_len, drops)
    assert drops == 0
    n = assert_counters(engines, topics, [0] * N_USERS, rec)
    if wire_len >= 64:
        assert engines[0].ring_wpos.tolist()[:3] == [M * rec, (M + 2) // 4 * rec, 0]
        assert n > 0 or M == 1
    else:
        assert n == 0 and int(engines[0].ring_wpos.sum()) == 0


@pytest.mark.parametrize("n_users", [64, 65])
def test_one_word_and_one_user_more(n_users):
    M = 70
    engines = make_engines(n_users, M * REC, sub_mixed(n_users))
    batch, offsets, topics = batch_of(lambda i: [i % 4], M, seed=n_users)
    drops = tick_all(engines, batch, offsets, WIRE)
    assert_same(engines, WIRE, drops)
    assert drops == 0
    assert_counters(engines, topics, [0] * n_users)


# --------------------------- 2. the fallback boundary -----------------------

@pytest.fixture(scope="module")
def route_max_m():
    return int(get_gpu_ops()._ROUTE_MAX_M)


@pytest.mark.parametrize("over", [0, 1])
def test_fallback_boundary(route_max_m, over):
    """M = ROUTE_MAX_M takes the route kernel, one more the four-kernel
    chain; both must agree with the per-op engine (the CPU engine's Python
    loops over half a million pairs are left out here)."""
    assert route_max_m >= 2048
    M = route_max_m + over
    common = dict(device="cuda:0", n_users=N_USERS, ring_bytes=M * REC, direct_table_size=64,
                  fanout_wire=True, direct_enabled=False, pair_capacity=1 << 19)
    fused = GpuBrokerEngine(fused_tick=True, **common)
    plain = GpuBrokerEngine(fused_tick=False, **common)
    batch, offsets, _ = batch_of(lambda i: [i % 4], M, seed=over)
    for eng in (fused, plain):
        sub_mixed(N_USERS)(eng)
        eng.egress.fill_(SENT)
        bg, og = eng.ingest(batch, offsets)
        eng.tick(bg, og, uniform_wire_len=WIRE)
    torch.cuda.synchronize()
    assert fused.fused_ticks == 1 and plain.fused_ticks == 0
    want = [M * REC if u % 3 == 0 else
            len(range(u % 4, M, 4)) * REC if u % 3 == 1 else 0 for u in range(N_USERS)]
    for eng in (fused, plain):
        assert eng.ring_wpos.cpu().tolist() == want
        assert int(eng._drops.cpu()[0]) == 0
        assert int(eng._n_pairs.cpu()[0]) == sum(want) // REC
    # a one-topic user's tiles are sparse, but for a last block of one message it takes
    sparse = 0
    for u in range(1, N_USERS, 3):
        for m0 in range(0, M, BLK):
            m1 = min(M, m0 + BLK)
            cnt = len([i for i in range(m0, m1) if i % 4 == u % 4])
            sparse += cnt if cnt < m1 - m0 else 0
    assert int(fused._n_sparse.cpu()[0]) == sparse
    assert torch.equal(fused.egress, plain.egress)


# --------------------------- 3. tiles of every kind -------------------------

def test_dense_sparse_and_empty_tiles_in_one_word():
    M = 75      # two full blocks and one of 11
    engines = make_engines(N_USERS, M * REC, sub_mixed(N_USERS))
    batch, offsets, topics = batch_of(lambda i: [i % 4], M, seed=3)
    drops = tick_all(engines, batch, offsets, WIRE)
    assert_same(engines, WIRE, drops)
    assert drops == 0
    n = assert_counters(engines, topics, [0] * N_USERS)
    assert n == sum(len(range(u % 4, M, 4)) for u in range(N_USERS) if u % 3 == 1)


# --------------------------- 4. other messages in the batch -----------------

def test_several_topics_and_messages_nobody_receives():
    """Two-topic messages, a Subscribe padded to the uniform length in block
    0 and a Broadcast with its root pointer zeroed in block 2: neither is
    delivered, and their blocks' tiles are sparse for every user."""
    M = 75
    bad = bytearray(m.serialize(m.Broadcast([0], bytes(8))))
    bad[8:16] = bytes(8)
    special = {5: m.serialize(m.Subscribe([0, 1])), 70: bytes(bad)}
    engines = make_engines(N_USERS, M * REC, sub_mixed(N_USERS))
    batch, offsets, topics = batch_of(lambda i: [i % 4, (i + 1) % 4] if i % 5 == 0 else [i % 4],
                                      M, seed=4, special=special)
    drops = tick_all(engines, batch, offsets, WIRE)
    assert_same(engines, WIRE, drops)
    assert drops == 0
    cpu = engines[0]
    assert cpu.ring_wpos.tolist()[0] == (M - 2) * REC
    _, sparse = route_model(cpu, topics, [0] * N_USERS)
    assert_counters(engines, topics, [0] * N_USERS)
    # user 0 takes everything: block 1 dense, blocks 0 and 2 on the sparse list
    assert sorted(i for u, i, _ in sparse if u == 0) == \
        [i for i in range(M) if not 32 <= i < 64 and i not in special]


# --------------------------- 5. ticks in a row ------------------------------

def test_two_ticks_without_a_drain_then_one_after():
    M = 33
    engines = make_engines(N_USERS, 2 * M * REC, sub_mixed(N_USERS))
    cpu, fused, plain = engines
    drops = 0
    for tick in range(2):
        before = cpu.ring_wpos.tolist()
        batch, offsets, topics = batch_of(lambda i: [(i + tick) % 4], M, seed=50 + tick)
        drops += tick_all(engines, batch, offsets, WIRE)
        torch.cuda.synchronize()
        assert_counters(engines, topics, before)     # the counters restart every tick
    assert drops == 0
    assert_same(engines, WIRE, drops)                # tick 2's records follow tick 1's
    assert cpu.ring_wpos.tolist()[0] == 2 * M * REC
    want = cpu.drain_cursors()
    for eng in (fused, plain):
        assert torch.equal(eng.drain_cursors(), want)
    for eng in engines:
        eng.egress.fill_(SENT)
    batch, offsets, topics = batch_of(lambda i: [i % 4], M, seed=52)
    drops += tick_all(engines, batch, offsets, WIRE)
    assert_same(engines, WIRE, drops)
    assert_counters(engines, topics, [0] * N_USERS)
    assert cpu.ring_wpos.tolist()[0] == M * REC


# --------------------------- 6. ring and pair limits ------------------------

@pytest.mark.parametrize("M,ring_recs", [(33, 20), (257, 200)])
def test_ring_limits_clip_mid_block(M, ring_recs):
    """The ring ends inside a block: the blocks before it dense, that one
    clipped, the rest dropped; users advanced by an earlier tick clip
    earlier."""
    def subscribe(eng):
        eng.subscribe_all([0])
        for u in range(0, N_USERS, 3):
            eng.subscribe(u, [1])
        for u in range(1, N_USERS, 7):
            eng.subscribe(u, [2])

    engines = make_engines(N_USERS, ring_recs * REC, subscribe, pair_capacity=1 << 16)
    batch, offsets, _ = batch_of(lambda i: [1] if i < 3 else [2], 12, seed=60)
    drops = tick_all(engines, batch, offsets, WIRE)
    assert drops == 0
    before = engines[0].ring_wpos.tolist()
    batch, offsets, topics = batch_of(lambda i: [0], M, seed=61)
    drops += tick_all(engines, batch, offsets, WIRE)
    assert_same(engines, WIRE, drops)
    assert_counters(engines, topics, before)
    assert drops == ((M - ring_recs) * N_USERS + 3 * len(range(0, N_USERS, 3))
                     + 9 * len(range(1, N_USERS, 7)))
    assert engines[0].ring_wpos.tolist() == [ring_recs * REC] * N_USERS


@pytest.mark.parametrize("M", [33, 257])
def test_pair_capacity_invariants(M):
    """pair_capacity at about half the deliveries, so it is reached inside a
    mask word.  Which users lose records depends on the order of the span
    claims, so only invariants hold."""
    ring_bytes = M * REC
    eng = GpuBrokerEngine(device="cuda:0", n_users=N_USERS, ring_bytes=ring_bytes,
                          direct_table_size=64, fanout_wire=True, direct_enabled=False,
                          pair_capacity=M * N_USERS // 2)
    eng.subscribe_all([0])
    eng.egress.fill_(SENT)
    batch, offsets, _ = batch_of(lambda i: [0], M, seed=7)
    bg, og = eng.ingest(batch, offsets)
    eng.tick(bg, og, uniform_wire_len=WIRE)
    torch.cuda.synchronize()
    assert eng.fused_ticks == 1
    wpos = eng.ring_wpos.cpu().tolist()
    drops = int(eng._drops.cpu()[0])
    assert all(w % REC == 0 for w in wpos)
    assert sum(w // REC for w in wpos) + drops == M * N_USERS
    assert 0 < drops < M * N_USERS
    assert int(eng._n_pairs.cpu()[0]) == M * N_USERS
    stream = b""
    for i in range(M):
        stream += (WIRE.to_bytes(4, "little") + i.to_bytes(4, "little") + bytes(8)
                   + batch[offsets[i]:offsets[i + 1]])
    rings = eng.egress.cpu().view(N_USERS, ring_bytes)
    want = torch.frombuffer(bytearray(stream), dtype=torch.uint8)
    for u, w in enumerate(wpos):
        assert torch.equal(rings[u, :w], want[:w]), f"user {u}: not a prefix"
        assert bool((rings[u, w:] == SENT).all()), f"user {u}: bytes past the cursor"
