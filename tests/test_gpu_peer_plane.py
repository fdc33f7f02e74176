"""GPU goldens for the peer-broker plane: k2a_topic_mask_origin_t,
k5b_emit_direct_peers, k6_direct_apply and the engine end to end.

Same style as test_gpu_dataplane_edges.py: outputs start sentinel-filled and
every comparison against the serial models in pushcdn_amd.ops.reference is
exact.  Where the kernel claims with atomics the ORDER is unspecified, so
those tests assert order-free invariants (sets, disjoint tiling intervals,
cursor totals) and exact equality wherever the outcome is determined."""

import random

import numpy as np
import pytest
import torch

from pushcdn_amd.broker.gpu_engine import GpuBrokerEngine, parse_ring_records, ring_rec
from pushcdn_amd.ops import reference as ref
from pushcdn_amd.proto import message as m

pytestmark = pytest.mark.gpu

INT32_MIN = -(2**31)
PAIR_DT = np.dtype([("user", "<i4"), ("msg", "<i4"), ("dst", "<i8")])
UNWRITTEN = (-7, -7, -7 * (1 << 32) + 0xFFFFFFF9)   # a pair row still holding the -7 fill


@pytest.fixture(scope="module")
def ops():
    from pushcdn_amd.ops import get_gpu_ops

    return get_gpu_ops()


def _i64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= (1 << 63) else x


def make_batch(msgs):
    offsets, buf = [0], b""
    for msg in msgs:
        buf += m.serialize(msg)
        offsets.append(len(buf))
    return buf, offsets


def dev_bytes(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")


def i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device="cuda")


def i64(xs):
    return torch.tensor([_i64(x) for x in xs], dtype=torch.int64, device="cuda")


def pairs_from_dev(pairs):
    arr = pairs.cpu().contiguous().numpy().reshape(-1).view(PAIR_DT)
    return [(int(r["user"]), int(r["msg"]), int(r["dst"])) for r in arr]


# ===========================================================================
# k2a_topic_mask_origin_t
# ===========================================================================

@pytest.mark.parametrize("n_users,n_peers", [(70, 3), (64, 2), (62, 4)])
def test_topic_mask_origin_t_matches_reference(ops, n_users, n_peers):
    """Peer bits in mid-word after the user tail (70, 3), starting a word
    (64, 2) and straddling two words (62, 4).  Remote-origin Broadcasts keep
    exactly their user bits; non-Broadcast rows are zero although the output
    is torch.empty; with an all-zero origin the result is topic_mask_t's."""
    rng = random.Random(n_users * 10 + n_peers)
    R = n_users + n_peers
    W = (R + 63) // 64
    sub = torch.tensor([[_i64(rng.getrandbits(64)) for _ in range(W)] for _ in range(256)],
                       dtype=torch.int64)
    # every peer subscribes to topics 3 and 200, so clearing really happens
    for r in range(n_users, R):
        for t in (3, 200):
            sub[t, r >> 6] = _i64(int(sub[t, r >> 6]) | (1 << (r & 63)))
    msgs = [m.Broadcast([3], b"local"), m.Broadcast([3], b"local"), m.Direct(b"key", b"d"),
            m.Broadcast([200, 17], b"two-topics"), m.Subscribe([3, 200])]
    origin = [0, 1, 0, 1, 0]
    buf, offsets = make_batch(msgs)
    pr = ref.parse_batch(buf, offsets)
    want = ref.topic_mask_origin(sub, buf, pr.topics_off, pr.topics_cnt, pr.disc, origin,
                                 n_users).T.contiguous()
    plain = ref.topic_mask(sub, buf, pr.topics_off, pr.topics_cnt, pr.disc).T.contiguous()
    assert not torch.equal(want, plain)
    for r in range(n_users, R):                       # the model itself: peers cut off
        assert (int(want[r >> 6, 0]) >> (r & 63)) & 1 == 1
        assert (int(want[r >> 6, 1]) >> (r & 63)) & 1 == 0
        assert (int(want[r >> 6, 3]) >> (r & 63)) & 1 == 0
    args = (sub.to("cuda"), dev_bytes(buf), pr.topics_off.to("cuda"), pr.topics_cnt.to("cuda"),
            pr.disc.to("cuda"))
    # dirty the allocator block the kernel's torch.empty output will reuse
    junk = torch.full((W, len(msgs)), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    del junk
    got = ops.topic_mask_origin_t(*args, i32(origin), n_users)
    zero = ops.topic_mask_origin_t(*args, i32([0] * len(msgs)), n_users)
    base = ops.topic_mask_t(*args)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (W, len(msgs))
    assert torch.equal(got.cpu(), want)
    assert torch.equal(zero.cpu(), base.cpu()) and torch.equal(base.cpu(), plain)
    assert not bool(got[:, 2].cpu().any()) and not bool(got[:, 4].cpu().any())


# ===========================================================================
# k5b_emit_direct_peers
# ===========================================================================

N_USERS, P = 70, 3
PEER0, PEER1, PEER_LAST = N_USERS, N_USERS + 1, N_USERS + P - 1
PRESET = [(9, 1, 16 * 1234), (-1, 2, 0), (7, 3, 16)]


@pytest.fixture(scope="module")
def k5p_inputs():
    rng = random.Random(91)
    M = 320
    kinds = [0, 69, -2, -3, -(P + 1), -(P + 2), INT32_MIN, "remote-peer", N_USERS + 1]
    disc, owner, origin, plen = [], [], [], []
    for i in range(M):
        disc.append(3 if rng.random() < 0.75 else rng.choice([0, 4, 5, 7, -1]))
        k = kinds[i % len(kinds)] if i < 4 * len(kinds) else rng.choice(kinds)
        if k == "remote-peer":
            owner.append(rng.choice([-2, -3, -(P + 1)]))
            origin.append(1)
        else:
            owner.append(k)
            # a LOCAL owner is served whatever the origin
            origin.append(rng.choice([0, 1]) if isinstance(k, int) and 0 <= k < N_USERS else 0)
        plen.append(rng.randrange(1, 301))

    def recipient(i):
        if disc[i] != 3:
            return None
        o = owner[i]
        if 0 <= o < N_USERS:
            return o
        if -(P + 1) <= o <= -2 and origin[i] == 0:
            return N_USERS + (-o - 2)
        return None

    want = {i: recipient(i) for i in range(M) if recipient(i) is not None}
    need = {r: sum(ring_rec(plen[i]) for i, x in want.items() if x == r)
            for r in (0, 69, PEER0, PEER1, PEER_LAST)}
    assert min(need.values()) > 2000 and set(want.values()) == set(need)
    ring_bytes = (max(need.values()) + 64) & ~15
    wpos0 = [0] * (N_USERS + P)
    wpos0[69] = 48
    wpos0[PEER1] = (ring_bytes - need[PEER1] // 2) & ~15   # about half of its claims fit
    wpos0[PEER_LAST] = ring_bytes - 16                      # full: nothing ever fits
    wpos0[5] = 160                                          # a bystander ring
    return dict(M=M, disc=disc, owner=owner, origin=origin, plen=plen, want=want,
                ring_bytes=ring_bytes, wpos0=wpos0)


def _run_k5p(ops, inp, capacity):
    K = len(PRESET)
    pairs = torch.full((capacity, 4), -7, dtype=torch.int32, device="cuda")
    arr = np.zeros(K, dtype=PAIR_DT)
    for i, row in enumerate(PRESET):
        arr[i] = row
    pairs[:K] = torch.from_numpy(arr.view("<i4").reshape(-1, 4).copy()).to("cuda")
    wpos = torch.tensor(inp["wpos0"], dtype=torch.int64, device="cuda")
    n_pairs = i32([K])
    drops = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.emit_direct_peers(i32(inp["disc"]), i32(inp["owner"]), i32(inp["origin"]),
                          torch.zeros(inp["M"], dtype=torch.int64, device="cuda"),
                          i32(inp["plen"]), inp["ring_bytes"], N_USERS, P, wpos, n_pairs,
                          pairs, drops)
    torch.cuda.synchronize()
    return (pairs_from_dev(pairs), wpos.cpu().tolist(), int(n_pairs.cpu()[0]),
            int(drops.cpu()[0]))


def _check_k5p_rows(inp, rows, wpos):
    """Claim invariants over the rows the kernel wrote after the preset."""
    K = len(PRESET)
    ring_bytes, plen, want = inp["ring_bytes"], inp["plen"], inp["want"]
    assert rows[:K] == PRESET, "existing pairs must stay untouched"
    written = rows[K:]
    msgs = [mi for _, mi, _ in written]
    assert len(set(msgs)) == len(msgs), "one row per message at most"
    assert set(msgs) <= set(want), "out-of-range / missing / remote-origin rows emit nothing"
    accepted, dropped = {}, []
    for u, mi, dst in written:
        if u < 0:
            assert (u, dst) == (-1, 0)
            dropped.append(mi)
            continue
        assert u == want[mi], f"msg {mi}: recipient {u}, expected {want[mi]}"
        off = dst - u * ring_bytes
        accepted.setdefault(u, []).append((off, off + ring_rec(plen[mi])))
    for r in range(N_USERS + P):
        # pairwise disjoint, in bounds, tiling [wpos0, wpos_final) exactly
        pos = inp["wpos0"][r]
        for lo, hi in sorted(accepted.get(r, [])):
            assert lo == pos, f"ring {r}: gap or overlap at {lo} (expected {pos})"
            pos = hi
        assert pos == wpos[r] <= ring_bytes, f"ring {r}"
    for mi in dropped:
        assert wpos[want[mi]] + ring_rec(plen[mi]) > ring_bytes, "dropped although it fits"
    return accepted, dropped


def test_emit_direct_peers_invariants(ops, k5p_inputs):
    """Owners: local users (either origin), -2, the last valid peer -(P+1),
    -(P+2) out of range, INT32_MIN, an owner >= n_users, a peer owner with
    remote origin, non-Direct rows; appended behind existing pairs.  The
    last peer's ring is full: a placeholder and one counted drop per claim."""
    inp = k5p_inputs
    K, want = len(PRESET), inp["want"]
    cap = K + len(want) + 8
    rows, wpos, n_pairs, drops = _run_k5p(ops, inp, cap)
    assert n_pairs == K + len(want)
    assert all(r == UNWRITTEN for r in rows[n_pairs:])
    assert all(r != UNWRITTEN for r in rows[K:n_pairs])
    accepted, dropped = _check_k5p_rows(inp, rows[:n_pairs], wpos)
    assert {mi for _, mi, _ in rows[K:n_pairs]} == set(want)
    assert drops == len(dropped)
    # determined outcomes equal the serial model exactly
    mw = torch.tensor(inp["wpos0"], dtype=torch.int64)
    pu, pm, _pd, _drops = ref.emit_direct_peers(
        torch.tensor(inp["disc"]), torch.tensor(inp["owner"]), inp["origin"],
        torch.tensor(inp["plen"]), mw, inp["ring_bytes"], N_USERS, P)
    assert set(pm.tolist()) == set(want)
    for r in (0, 69, PEER0, PEER_LAST, 5):
        assert wpos[r] == int(mw[r]), f"ring {r}"
    full = [mi for mi, r in want.items() if r == PEER_LAST]
    assert full and set(full) <= set(dropped) and PEER_LAST not in accepted
    assert wpos[PEER_LAST] == inp["wpos0"][PEER_LAST]
    n1 = sum(1 for r in want.values() if r == PEER1)
    assert 0 < len(accepted[PEER1]) < n1              # the half-full ring really filled
    assert all(want[mi] in (PEER1, PEER_LAST) for mi in dropped)


def test_emit_direct_peers_pair_capacity(ops, k5p_inputs):
    """capacity < preset + eligible: every claim counted, the excess dropped,
    exactly `capacity` rows written and none past them touched."""
    inp = k5p_inputs
    K, n_elig = len(PRESET), len(inp["want"])
    cap = K + n_elig // 2
    rows, wpos, n_pairs, drops = _run_k5p(ops, inp, cap)
    assert len(rows) == cap and n_pairs == K + n_elig
    assert all(r != UNWRITTEN for r in rows[K:])
    accepted, dropped = _check_k5p_rows(inp, rows, wpos)
    assert sum(len(v) for v in accepted.values()) + len(dropped) == cap - K
    assert drops == (K + n_elig - cap) + len(dropped)


def test_emit_direct_peers_single_full_ring(ops):
    """One local Direct to a peer whose ring is full: one placeholder pair,
    one drop, cursor unchanged; the same message with remote origin: nothing."""
    for origin, want_rows, want_drops in ((0, [(-1, 0, 0)], 1), (1, [UNWRITTEN], 0)):
        pairs = torch.full((2, 4), -7, dtype=torch.int32, device="cuda")
        wpos = torch.tensor([0, 0, 256 - 16], dtype=torch.int64, device="cuda")
        n_pairs = i32([0])
        drops = i32([0])
        ops.emit_direct_peers(i32([3]), i32([-2]), i32([origin]),
                              torch.zeros(1, dtype=torch.int64, device="cuda"), i32([40]),
                              256, 2, 1, wpos, n_pairs, pairs, drops)
        torch.cuda.synchronize()
        assert pairs_from_dev(pairs)[:1] == want_rows
        assert pairs_from_dev(pairs)[1] == UNWRITTEN
        assert int(drops.cpu()[0]) == want_drops
        assert wpos.cpu().tolist() == [0, 0, 240]


# ===========================================================================
# k6_direct_apply, checked through k5_direct_lookup
# ===========================================================================

class DevTable:
    def __init__(self, ops, size):
        self.ops = ops
        self.keys = torch.zeros(size, dtype=torch.int64, device="cuda")
        self.vals = torch.full((size,), -99, dtype=torch.int32, device="cuda")
        self.failed = torch.zeros(1, dtype=torch.int32, device="cuda")

    def apply(self, upserts, deletes):
        """One launch; returns the failure count of THIS launch."""
        before = int(self.failed.cpu()[0])
        self.ops.direct_apply(self.keys, self.vals, i64([h for h, _ in upserts]),
                              i32([o for _, o in upserts]), i64(deletes), self.failed)
        torch.cuda.synchronize()
        return int(self.failed.cpu()[0]) - before

    def lookup(self, hs):
        got = self.ops.direct_lookup(self.keys, self.vals, i64(hs))
        torch.cuda.synchronize()
        return got.cpu().tolist()

    def check(self, model, absent=()):
        hs = list(model) + list(absent)
        assert self.lookup(hs) == [model[h] for h in model] + [INT32_MIN] * len(absent)

    def nonzero(self):
        return int((self.keys != 0).sum().cpu())


def test_direct_apply_size8_chain_tombstones_full(ops):
    """Table of 8: five keys homed at slot 6 inserted in ONE launch (the
    chain wraps to slots 0..2; which key lands where is up to the CAS
    race, lookups are not), deletes leave keys in place, a re-upsert reuses
    the slot, a ninth key into the full table reports one failure."""
    t = DevTable(ops, 8)
    chain = [(i + 1) << 8 | 6 for i in range(4)] + [(1 << 63) | 0x506]
    model = {}
    ups = [(h, -(i + 2)) for i, h in enumerate(chain)]
    assert t.apply(ups, []) == 0
    model.update(ups)
    t.check(model, absent=[0x906, 0x905])
    assert [int(k) != 0 for k in t.keys.cpu()] == [True, True, True, False, False, False,
                                                   True, True]
    assert sorted(int(k) & ((1 << 64) - 1) for k in t.keys.cpu() if int(k)) == sorted(chain)
    assert t.vals.cpu().tolist()[3:6] == [-99] * 3       # untouched slots
    # delete two and upsert an unrelated key in the same launch
    assert t.apply([(0x1003, 33)], [chain[1], chain[3], 0x906]) == 0
    model[chain[1]] = model[chain[3]] = INT32_MIN
    model[0x1003] = 33
    t.check(model, absent=[0x906])
    assert t.nonzero() == 6
    # later launch: re-upsert a deleted key with a new owner -> same slot
    assert t.apply([(chain[3], 5)], []) == 0
    model[chain[3]] = 5
    t.check(model)
    assert t.nonzero() == 6
    # fill the table; the ninth key fails and changes nothing
    fill = [(0x1004, 4), (0x1005, 5)]
    assert t.apply(fill, []) == 0
    model.update(fill)
    assert t.nonzero() == 8
    snap = (t.keys.clone(), t.vals.clone())
    assert t.apply([(0x2003, 9)], []) == 1
    assert torch.equal(t.keys, snap[0]) and torch.equal(t.vals, snap[1])
    t.check(model, absent=[0x2003])
    # an update of a PRESENT key still works in the full table
    assert t.apply([(chain[0], 77)], [chain[4]]) == 0
    model[chain[0]], model[chain[4]] = 77, INT32_MIN
    t.check(model, absent=[0x2003])


def test_direct_apply_contended_inserts_match_dict(ops):
    """200 distinct random keys (bit 63 set in about half) into a table of
    256 in one launch: four waves contend on CAS over shared probe chains.
    Every lookup equals the dict; then a mixed launch of deletes, re-upserts
    and new keys."""
    rng = random.Random(256)
    t = DevTable(ops, 256)
    hs = set()
    while len(hs) < 200:
        hs.add(rng.getrandbits(64) | 1)
    hs = sorted(hs)
    assert any(h >> 63 for h in hs)
    model = {h: rng.choice([rng.randrange(1000), -rng.randrange(2, 40)]) for h in hs}
    absent = [h ^ (1 << 40) for h in hs[:20] if h ^ (1 << 40) not in model]
    assert t.apply(list(model.items()), []) == 0
    assert t.nonzero() == 200
    t.check(model, absent=absent)
    assert sorted(int(k) & ((1 << 64) - 1) for k in t.keys.cpu() if int(k)) == hs
    # second launch: delete 60, change the owner of 50 others, add 30 new keys
    dels, chg = hs[:60], hs[60:110]
    new = []
    while len(new) < 30:
        h = rng.getrandbits(64) | 1
        if h not in model and h not in new:
            new.append(h)
    ups = [(h, 5000 + i) for i, h in enumerate(chg)] + [(h, -5) for h in new]
    assert t.apply(ups, dels) == 0
    for h in dels:
        model[h] = INT32_MIN
    model.update(ups)
    assert t.nonzero() == 230
    t.check(model, absent=[a for a in absent if a not in model])
    # third launch: re-upsert the deleted keys; no new slot is taken
    assert t.apply([(h, 7) for h in dels], []) == 0
    model.update((h, 7) for h in dels)
    assert t.nonzero() == 230
    t.check(model)


def test_direct_apply_empty_batch_and_key_zero(ops):
    t = DevTable(ops, 8)
    assert t.apply([], []) == 0
    assert t.nonzero() == 0 and t.vals.cpu().tolist() == [-99] * 8
    assert t.apply([(0, 5), (0x11, 1)], [0]) == 0
    assert t.nonzero() == 1
    t.check({0x11: 1}, absent=[0x19])
    assert t.lookup([0]) == [INT32_MIN]
    assert t.vals.cpu().tolist().count(-99) == 7


# ===========================================================================
# engine end to end
# ===========================================================================

def test_engine_peer_plane_matches_cpu(ops):
    """GpuBrokerEngine(n_users=70, n_peer_slots=3) on the GPU against the
    same engine on the CPU models: one mixed batch of both origins with
    Broadcast and Direct, a peer ring that overflows on Broadcasts, DirectMap
    built through apply_direct_updates (K6 on the GPU) including a delete."""
    kw = dict(n_users=N_USERS, n_peer_slots=P, ring_bytes=4096, fanout_wire=True,
              direct_table_size=64, hash_seed=0xFEED)
    cpu = GpuBrokerEngine(device="cpu", **kw)
    gpu = GpuBrokerEngine(device="cuda:0", pair_capacity=1 << 10, **kw)
    for eng in (cpu, gpu):
        for u in (0, 63, 64, 69):
            eng.subscribe(u, [1])
        eng.subscribe(5, [2])
        eng.set_peer_topics(0, [1, 2])
        eng.set_peer_topics(1, [9])          # the big topic: overflows
        eng.set_peer_topics(2, [2])
        eng.register_direct(b"local-5", 5)
        eng.apply_direct_updates([(b"on-peer-0", -2), (b"on-peer-2", -4),
                                  (b"moved-away", -3), (b"beyond", -(P + 2))], [])
        eng.apply_direct_updates([(b"on-peer-2b", -4)], [b"moved-away"])
    big = [m.Broadcast([9], bytes([65 + i]) * 1500) for i in range(3)]
    msgs = [
        (m.Broadcast([1], b"local-one"), 0),
        (m.Broadcast([1, 2], b"remote-one-two" * 3), 1),
        (big[0], 0),
        (m.Direct(b"on-peer-0", b"direct-to-peer-0"), 0),
        (m.Direct(b"on-peer-0", b"bounced"), 1),
        (big[1], 0),
        (m.Direct(b"local-5", b"direct-local-from-peer" * 5), 1),
        (m.Direct(b"on-peer-2b", b"x" * 333), 0),
        (big[2], 0),
        (m.Direct(b"moved-away", b"deleted-key"), 0),
        (m.Direct(b"beyond", b"slot-out-of-range"), 0),
        (m.Broadcast([2], b""), 0),
        (m.Subscribe([1]), 0),
    ]
    batch, offsets = make_batch([x for x, _ in msgs])
    origin = [o for _, o in msgs]
    bc, oc, orc = cpu.ingest(batch, offsets, origin=origin)
    stats = cpu.tick(bc, oc, host_batch=batch, host_offsets=offsets, origin=orc)
    bg, og, org = gpu.ingest(batch, offsets, origin=origin)
    gpu.tick(bg, og, origin=org)
    torch.cuda.synchronize()
    assert stats.n_drops == 1 and int(gpu._drops.cpu()[0]) == 1   # the third big one

    wc, offc, sc = cpu.drain_compact()
    wg, offg, sg = gpu.drain_compact()
    assert wc.numel() == N_USERS + P
    assert torch.equal(wc, wg) and torch.equal(offc, offg)
    rc, rg = sc.numpy().tobytes(), sg.numpy().tobytes()
    wire = [m.serialize(x) for x, _ in msgs]
    got = {}
    for r in range(N_USERS + P):
        lo, hi = int(offc[r]), int(offc[r + 1])
        recs_c = parse_ring_records(rc[lo:hi], hi - lo)
        recs_g = parse_ring_records(rg[lo:hi], hi - lo)
        assert recs_c == recs_g, f"recipient {r}"
        if recs_g:
            got[r] = [p for _s, p in recs_g]
    # and both equal the routing worked out by hand
    assert got == {
        0: [wire[0], wire[1]], 63: [wire[0], wire[1]], 64: [wire[0], wire[1]],
        69: [wire[0], wire[1]],
        5: [wire[1], wire[6], wire[11]],
        PEER0: [wire[0], wire[3], wire[11]],
        PEER1: [wire[2], wire[5]],
        PEER_LAST: [wire[7], wire[11]],
    }
    assert int(gpu.ring_wpos.cpu().sum()) == 0
