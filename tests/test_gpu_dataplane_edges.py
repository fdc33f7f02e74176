"""Edge-case golden tests for the LIVE tick path (K2b non-uniform, K5/K5b,
K3 wave/flat, K7) plus the small kernels (K2a_t, K2c).

The bench-shape goldens in test_gpu_kernels.py use uniform 16 B-padded
records, 16-aligned sources, zeroed egress and the default grid.  Here every
kernel is compared bit-for-bit against the plain Python models in
pushcdn_amd.ops.reference at the shapes where index math goes wrong:
unaligned sources, partial/pure-pad units, multi-iteration grid-stride
loops, mask tail words, ring-full mid-stream, multi-chunk compaction — and
always on SENTINEL-filled (0xA5) outputs, so a stray byte outside a record
is as visible as a wrong byte inside one.  All inputs are valid and in
bounds; every comparison is exact."""

import itertools
import random

import numpy as np
import pytest
import torch

from pushcdn_amd.broker.gpu_engine import GpuBrokerEngine, parse_ring_records, ring_rec
from pushcdn_amd.ops import reference as ref
from pushcdn_amd.proto import message as m

pytestmark = pytest.mark.gpu

SENT = 0xA5
INT32_MIN = -(2**31)
PAIR_DT = np.dtype([("user", "<i4"), ("msg", "<i4"), ("dst", "<i8")])
SEQ_BASE = 0xFFFFFFF0   # wraps past 2^32 after 16 messages
# a pair row still holding the -7 fill: nothing stored to it
UNWRITTEN = (-7, -7, -7 * (1 << 32) + 0xFFFFFFF9)


@pytest.fixture(scope="module")
def ops():
    from pushcdn_amd.ops import get_gpu_ops

    return get_gpu_ops()


def _i64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= (1 << 63) else x


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def make_batch(msgs):
    offsets, buf = [0], b""
    for msg in msgs:
        buf += m.serialize(msg)
        offsets.append(len(buf))
    return buf, offsets


def dev_bytes(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")


def pairs_to_dev(rows):
    """[(user, msg, dst)] -> int32 [n, 4] device tensor of 16 B PairRecs."""
    arr = np.zeros(len(rows), dtype=PAIR_DT)
    for i, (u, mi, d) in enumerate(rows):
        arr[i] = (u, mi, d)
    return torch.from_numpy(arr.view("<i4").reshape(-1, 4).copy()).to("cuda")


def pairs_from_dev(pairs):
    """int32 [n, 4] tensor -> [(user, msg, dst)]."""
    arr = pairs.cpu().contiguous().numpy().reshape(-1).view(PAIR_DT)
    return [(int(r["user"]), int(r["msg"]), int(r["dst"])) for r in arr]


def first_diff(got: bytes, want: bytes) -> str:
    if len(got) != len(want):
        return f"length {len(got)} != {len(want)}"
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    bad = np.nonzero(a != b)[0]
    if bad.size == 0:
        return "equal"
    i = int(bad[0])
    return (f"{bad.size} bytes differ, first at {i}: got {got[i:i + 16].hex()} "
            f"want {want[i:i + 16].hex()}")


# ===========================================================================
# (a) K3 variant matrix on sentinel-filled egress
# ===========================================================================

N_RINGS = 8           # rings 0..6 carry records, ring 7 is the canary
CANARY = N_RINGS - 1
WAVE_LENS = [0, 1, 15, 16, 17, 31, 1023, 1024, 1025, 4097]


class K3Case:
    """Hand-built source buffer + pair list for one K3 comparison."""

    def __init__(self, lens, rec_of, ring_bytes, n_target, seed):
        rng = random.Random(seed)
        self.M = len(lens)
        self.ring_bytes = ring_bytes
        # source: random bytes everywhere (gaps included, so an over-read
        # that lands in egress shows); payload_off % 16 cycles {0, 1, 8, 15}
        src = bytearray()
        poff = []
        for i, ln in enumerate(lens):
            base = (len(src) + 15) & ~15
            off = base + (0, 1, 8, 15)[i % 4]
            src += rng.randbytes(off + ln + rng.randrange(1, 9) - len(src))
            poff.append(off)
        src += rng.randbytes(64)
        assert {o % 16 for o in poff} == {0, 1, 8, 15}
        self.buf = bytes(src)
        self.poff = torch.tensor(poff, dtype=torch.int64)
        self.plen = torch.tensor(lens, dtype=torch.int32)
        # live pairs: ring 0 starts at 64 so ring 0 offset 0 STAYS sentinel —
        # a consumed user=-1 placeholder (dst=0) would write a header there
        wpos = [64] + [16 * u for u in range(1, CANARY)]
        rows = []
        for i in range(n_target):
            mi = i % self.M
            rec = rec_of(lens[mi])
            room = [u for u in range(CANARY) if wpos[u] + rec <= ring_bytes]
            if not room:
                continue
            u = rng.choice(room)
            rows.append((u, mi, u * ring_bytes + wpos[u]))
            wpos[u] += rec
            if i % 9 == 4:
                rows.append((-1, rng.randrange(self.M), 0))   # ring-full placeholder
        assert {r[1] for r in rows if r[0] >= 0} == set(range(self.M)), "every length used"
        rng.shuffle(rows)
        self.rows = rows
        # rows past *n_pairs: VALID pairs aimed at the canary ring
        self.extra = []
        pos = 0
        for k in range(6):
            rec = rec_of(lens[k % self.M])
            assert pos + rec <= ring_bytes
            self.extra.append((CANARY, k % self.M, CANARY * ring_bytes + pos))
            pos += rec
        self.seq = [(SEQ_BASE + i) & 0xFFFFFFFF for i in range(self.M)]

    def expected(self, zero_pad_to=None) -> bytes:
        eg = bytearray(bytes([SENT]) * (N_RINGS * self.ring_bytes))
        live = self.rows
        ref.fanout(self.buf, self.poff, self.plen,
                   torch.tensor([r[0] for r in live], dtype=torch.int32),
                   torch.tensor([r[1] for r in live], dtype=torch.int32),
                   torch.tensor([r[2] for r in live], dtype=torch.int64),
                   torch.tensor(self.seq, dtype=torch.int64), eg, zero_pad_to=zero_pad_to)
        assert eg[0:16] == bytes([SENT]) * 16
        assert eg[CANARY * self.ring_bytes:] == bytes([SENT]) * self.ring_bytes
        return bytes(eg)

    def device(self):
        return dict(
            buf=dev_bytes(self.buf), poff=self.poff.to("cuda"), plen=self.plen.to("cuda"),
            seq=torch.tensor([_i32(s) for s in self.seq], dtype=torch.int32, device="cuda"),
        )

    def fresh_egress(self):
        return torch.full((N_RINGS * self.ring_bytes,), SENT, dtype=torch.uint8, device="cuda")


def _check_egress(case, egress, want, label):
    torch.cuda.synchronize()
    got = egress.cpu().numpy().tobytes()
    canary = got[CANARY * case.ring_bytes:]
    assert canary == bytes([SENT]) * case.ring_bytes, f"{label}: row past *n_pairs was read"
    assert got == want, f"{label}: {first_diff(got, want)}"
    return got


@pytest.fixture(scope="module")
def wave_case():
    lens = [ln for ln in WAVE_LENS for _ in range(4)]   # each length at all 4 alignments
    case = K3Case(lens, ring_rec, 32 << 10, 80, seed=101)
    # every length really meets every source alignment
    seen = {(ln, int(o) % 16) for ln, o in zip(lens, case.poff.tolist())}
    assert seen == {(ln, a) for ln in WAVE_LENS for a in (0, 1, 8, 15)}
    assert any(s > 0x7FFFFFFF for s in case.seq) and any(s < 16 for s in case.seq)
    return case, case.expected()


def test_k3_fanout_plain_sentinel(ops, wave_case):
    """k3_fanout (golden-test variant): exactly 16+len bytes per record,
    header seq = (base + msg) mod 2^32 from negative int32 values, user=-1
    rows skipped, every byte outside every record still 0xA5."""
    case, want = wave_case
    d = case.device()
    egress = case.fresh_egress()
    rows = case.rows
    ops.fanout(d["buf"], d["poff"], d["plen"],
               torch.tensor([r[0] for r in rows], dtype=torch.int32, device="cuda"),
               torch.tensor([r[1] for r in rows], dtype=torch.int32, device="cuda"),
               torch.tensor([r[2] for r in rows], dtype=torch.int64, device="cuda"),
               d["seq"], egress)
    _check_egress(case, egress, want, "fanout")


@pytest.mark.parametrize("grid", [0, 1, 3])
def test_k3_wave_sentinel(ops, wave_case, grid):
    """k3_fanout_wave, nt 0 and 1: unaligned-source branch, the byte tail
    after the last full 16 B chunk, multi-pass payloads (> 1 KiB), several
    grid-stride iterations (grid 1 = 4 waves, grid 3 = 12 waves for ~90
    rows), rows past *n_pairs unread; writes exactly 16+len per record."""
    case, want = wave_case
    d = case.device()
    pairs = pairs_to_dev(case.rows + case.extra)
    n_pairs = torch.tensor([len(case.rows)], dtype=torch.int32, device="cuda")
    got = {}
    for nt in (0, 1):
        egress = case.fresh_egress()
        ops.fanout_wave(d["buf"], d["poff"], d["plen"], pairs, d["seq"], n_pairs, egress,
                        nt, grid)
        got[nt] = _check_egress(case, egress, want, f"wave nt={nt} grid={grid}")
    assert got[0] == got[1]


FLAT_UNITS = [2, 3, 5, 67, 257]


def _flat_lens(units, mode, rng):
    top = (units - 1) * 16
    if mode == "uniform":
        return [top - 5] * 40          # one partial tail unit in every record
    edge = sorted({x for x in (0, 1, top - 17, top - 16, top - 1, top) if x >= 0})
    lens = [edge[i % len(edge)] if i < 4 * len(edge) else rng.randrange(top + 1)
            for i in range(40)]
    return lens


_flat_cache = {}


def _flat_case(units, mode):
    key = (units, mode)
    if key not in _flat_cache:
        rng = random.Random(1000 + units)
        lens = _flat_lens(units, mode, rng)
        rec = units * 16
        ring_bytes = (16 << 10) if units <= 5 else (32 << 10)
        # enough units that grid=3 (768 lanes) strides >= 4 times
        n_target = max(48, -(-3400 // units))
        case = K3Case(lens, lambda ln: rec, ring_bytes, n_target, seed=200 + units)
        assert len(case.rows) * units >= 4 * 768
        _flat_cache[key] = (case, case.expected(zero_pad_to=rec))
    return _flat_cache[key]


def _run_flat(ops, entry, case, d, pairs, n_pairs, units, uniform_len, nt, grid, egress):
    if entry == "flat2":
        ops.fanout_flat2(d["buf"], d["poff"], d["plen"], pairs, SEQ_BASE, n_pairs, units,
                         egress, nt, grid, uniform_len)
        return None
    seq_state = torch.tensor([_i32(SEQ_BASE)], dtype=torch.int32, device="cuda")
    ops.fanout_flat3(d["buf"], d["poff"], d["plen"], pairs, seq_state, n_pairs, units,
                     egress, nt, grid, uniform_len)
    return seq_state


@pytest.mark.parametrize("mode", ["uniform", "mixed"])
@pytest.mark.parametrize("units", FLAT_UNITS)
@pytest.mark.parametrize("entry", ["flat2", "flat3"])
def test_k3_flat_sentinel(ops, entry, units, mode):
    """k3_fanout_flat_t through both entry points: full-stride contract
    (header + payload + ZERO pad to units*16, nothing else touched) with
    units_per_pair not a power of two, unaligned full units, partial-tail
    and pure-pad units, per-message length load (uniform_len == 0), seq
    wrap at 2^32 from a by-value base (flat2) / the device counter (flat3),
    grid-stride loop iterating >= 4 times, rows past *n_pairs unread."""
    case, want = _flat_case(units, mode)
    d = case.device()
    pairs = pairs_to_dev(case.rows + case.extra)
    n_pairs = torch.tensor([len(case.rows)], dtype=torch.int32, device="cuda")
    uniform_len = int(case.plen[0]) if mode == "uniform" else 0
    if mode == "mixed":
        lens = set(case.plen.tolist())
        assert 0 in lens and (units - 1) * 16 in lens   # pure-pad + full records
    got = {}
    for grid in (0, 1, 3):
        for nt in (0, 1):
            egress = case.fresh_egress()
            seq_state = _run_flat(ops, entry, case, d, pairs, n_pairs, units, uniform_len,
                                  nt, grid, egress)
            got[nt] = _check_egress(case, egress, want,
                                    f"{entry} units={units} {mode} nt={nt} grid={grid}")
            if seq_state is not None:
                # flat3 only READS the counter; seq_advance bumps it mod 2^32
                assert int(seq_state.cpu()[0]) == _i32(SEQ_BASE)
                ops.seq_advance(seq_state, case.M)
                torch.cuda.synchronize()
                assert int(seq_state.cpu()[0]) == _i32(SEQ_BASE + case.M) == case.M - 16
        assert got[0] == got[1]


@pytest.mark.parametrize("variant", ["wave", "flat2", "flat3"])
def test_k3_n_pairs_clamped_to_capacity(ops, wave_case, variant):
    """*n_pairs larger than pairs.shape[0] (the claim counter keeps counting
    past the buffer when a tick oversubscribes pair_capacity): exactly
    `capacity` rows are consumed — the egress equals the reference applied
    to precisely the rows that exist."""
    if variant == "wave":
        case, want = wave_case
        units = 0
    else:
        units = 5
        case, want = _flat_case(units, "mixed")
    d = case.device()
    pairs = pairs_to_dev(case.rows)                       # no spare rows at all
    n_pairs = torch.tensor([len(case.rows) + 1000], dtype=torch.int32, device="cuda")
    egress = case.fresh_egress()
    if variant == "wave":
        ops.fanout_wave(d["buf"], d["poff"], d["plen"], pairs, d["seq"], n_pairs, egress, 1, 3)
    else:
        _run_flat(ops, variant, case, d, pairs, n_pairs, units, 0, 1, 3, egress)
    _check_egress(case, egress, want, f"{variant} clamp")


def test_fanout_flat_rejects_index_overflow(ops):
    """capacity * units_per_pair >= 2^31 would leave the exact range of the
    flat kernel's u32 magic division: the binding refuses it on the host,
    before any launch (the 128 MiB tensor is never read)."""
    big = torch.empty((1 << 23, 4), dtype=torch.int32, device="cuda")
    small = torch.zeros((4, 4), dtype=torch.int32, device="cuda")
    z8 = torch.zeros(64, dtype=torch.uint8, device="cuda")
    z64 = torch.zeros(1, dtype=torch.int64, device="cuda")
    z32 = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        ops.fanout_flat2(z8, z64, z32, big, 0, z32, 257, z8, 0, 1, 0)
    with pytest.raises(RuntimeError):
        ops.fanout_flat3(z8, z64, z32, big, z32, z32, 257, z8, 0, 1, 0)
    for bad_units in (0, -1, (1 << 21) + 1):
        with pytest.raises(RuntimeError):
            ops.fanout_flat2(z8, z64, z32, small, 0, z32, bad_units, z8, 0, 1, 0)
    torch.cuda.synchronize()
    assert bool((z8 == 0).all())


# ===========================================================================
# (b) K2b against ref.assign_emit
# ===========================================================================

K2B_USERS, K2B_M = 130, 70
K2B_W = (K2B_USERS + 63) // 64


@pytest.fixture(scope="module")
def k2b_inputs():
    rng = random.Random(77)
    words = [[0] * K2B_M for _ in range(K2B_W)]
    for u in range(K2B_USERS):
        p = 0.6 if u in (0, 63, 64, 127, 128, 129) else 0.25
        for mi in range(K2B_M):
            if rng.random() < p:
                words[u >> 6][mi] |= 1 << (u & 63)
    clean = [row[:] for row in words]
    # stray bits for users >= n_users in the 2-bit tail word: the kernel's
    # `active` guard must ignore them (the model only walks u < n_users)
    for mi in range(K2B_M):
        words[K2B_W - 1][mi] |= rng.getrandbits(62) << 2
    assert any(w >> 63 for w in words[0]) and any(w >> 63 for w in words[K2B_W - 1])
    mask_t = torch.tensor([[_i64(x) for x in row] for row in words], dtype=torch.int64)
    plen = torch.tensor([rng.randrange(1, 301) for _ in range(K2B_M)], dtype=torch.int32)
    assert sum(1 for x in plen.tolist() if x % 16) > K2B_M // 2
    total = sum(bin(x).count("1") for row in clean for x in row)
    # source bytes for the fan-out leg: records back to back, mostly unaligned
    poff, pos = [], 0
    for ln in plen.tolist():
        poff.append(pos)
        pos += ln
    buf = rng.randbytes(pos + 64)
    return dict(mask_t=mask_t, plen=plen, total=total, buf=buf,
                poff=torch.tensor(poff, dtype=torch.int64))


def _ref_assign(inp, plen, ring_bytes, wpos0):
    wpos = wpos0.clone()
    pu, pm, pd, drops = ref.assign_emit(inp["mask_t"].T.contiguous(), plen, wpos, ring_bytes,
                                        K2B_USERS)
    rows = list(zip(pu.tolist(), pm.tolist(), pd.tolist()))
    # per-user segments (placeholders attributed by position: the model
    # emits user by user), grouped into the 64-user waves that claim spans
    counts = [0] * K2B_USERS
    mt = inp["mask_t"]
    for u in range(K2B_USERS):
        counts[u] = sum(1 for mi in range(K2B_M) if (int(mt[u >> 6, mi]) >> (u & 63)) & 1)
    assert sum(counts) == len(rows) == inp["total"]
    segs, pos = [], 0
    for u in range(K2B_USERS):
        segs.append(rows[pos:pos + counts[u]])
        pos += counts[u]
    return rows, segs, wpos, drops


def _assert_pairs_per_user(got_rows, segs, label):
    """Slot order across waves is decided by atomics; within a wave's span
    users are in lane order and each user's rows in message order.  So the
    GPU list must be the per-user reference sequences, concatenated with the
    64-user waves in SOME order."""
    waves = [sum(segs[w * 64:(w + 1) * 64], []) for w in range(K2B_W)]
    for perm in itertools.permutations(range(K2B_W)):
        if got_rows == sum((waves[w] for w in perm), []):
            return
    want = sum(waves, [])
    bad = next((i for i, (a, b) in enumerate(zip(got_rows, want)) if a != b), None)
    raise AssertionError(f"{label}: pair list matches no wave order; vs identity order "
                         f"first diff at slot {bad}: got {got_rows[bad] if bad is not None else None} "
                         f"want {want[bad] if bad is not None else None} "
                         f"(len {len(got_rows)} vs {len(want)})")


def _gpu_assign(ops, variant, inp, plen, ring_bytes, wpos0, cap, uniform_rec):
    mask_t = inp["mask_t"].to("cuda")
    wpos = wpos0.clone().to("cuda")
    pairs = torch.full((cap, 4), -7, dtype=torch.int32, device="cuda")
    drops = torch.zeros(1, dtype=torch.int32, device="cuda")
    n_pairs = torch.zeros(1, dtype=torch.int32, device="cuda")
    if variant == "fused":
        ops.assign_emit_fused_t(mask_t, plen.to("cuda"), wpos, ring_bytes, K2B_USERS, pairs,
                                drops, n_pairs, uniform_rec)
    else:
        W64, NB = K2B_W * 64, (K2B_M + 31) // 32
        o32 = dict(dtype=torch.int32, device="cuda")
        ops.assign_emit_blocks_t(
            mask_t, wpos, ring_bytes, K2B_USERS,
            torch.empty(NB * W64, **o32), torch.empty(NB * W64, **o32),
            torch.empty(W64, **o32), torch.empty(W64, **o32),
            torch.empty(W64, dtype=torch.int64, device="cuda"),
            pairs, drops, n_pairs, uniform_rec)
    torch.cuda.synchronize()
    return pairs, wpos.cpu(), int(drops.cpu()[0]), int(n_pairs.cpu()[0])


def _wpos_stagger():
    return torch.tensor([16 * (u % 37) for u in range(K2B_USERS)], dtype=torch.int64)


@pytest.mark.parametrize("regime", ["fits", "ring_full_mid_stream", "pre_advanced"])
def test_k2b_nonuniform_matches_reference(ops, k2b_inputs, regime):
    """k2b_fused_t with uniform_rec == 0 (the live service's K2b): mixed
    lengths, 3 mask words with a 2-bit tail word + stray bits, users at the
    word edges; pairs per user, wpos, drops and n_pairs equal the model, and
    the GPU pair list fanned out by k3_fanout_wave reproduces the model's
    rings byte for byte on sentinel egress."""
    inp = k2b_inputs
    plen = inp["plen"]
    ring_bytes, wpos0 = {
        "fits": (1 << 15, torch.zeros(K2B_USERS, dtype=torch.int64)),
        # 2 max-size records long: large records drop, later small ones fit
        "ring_full_mid_stream": (640, torch.zeros(K2B_USERS, dtype=torch.int64)),
        "pre_advanced": (2048, _wpos_stagger()),
    }[regime]
    rows_r, segs, wpos_r, drops_r = _ref_assign(inp, plen, ring_bytes, wpos0)
    if regime == "fits":
        assert drops_r == 0
    else:
        # the regime really shows a drop FOLLOWED by an accept for some user
        assert any(any(a[0] < 0 and b[0] >= 0 for a, b in zip(s, s[1:])) for s in segs)
    for u in (0, 63, 64, 127, 128, 129):
        assert segs[u], f"user {u} receives something"

    cap = inp["total"] + 16
    pairs, wpos, drops, n_pairs = _gpu_assign(ops, "fused", inp, plen, ring_bytes, wpos0,
                                              cap, 0)
    got_rows = pairs_from_dev(pairs)
    assert n_pairs == inp["total"]
    assert drops == drops_r
    assert torch.equal(wpos, wpos_r)
    assert all(r == UNWRITTEN for r in got_rows[n_pairs:])
    _assert_pairs_per_user(got_rows[:n_pairs], segs, regime)

    # fan the GPU pair list out and compare the rings with the model's
    seq = [(SEQ_BASE + i) & 0xFFFFFFFF for i in range(K2B_M)]
    want = bytearray(bytes([SENT]) * (K2B_USERS * ring_bytes))
    ref.fanout(inp["buf"], inp["poff"], plen,
               torch.tensor([r[0] for r in rows_r], dtype=torch.int32),
               torch.tensor([r[1] for r in rows_r], dtype=torch.int32),
               torch.tensor([r[2] for r in rows_r], dtype=torch.int64),
               torch.tensor(seq, dtype=torch.int64), want)
    egress = torch.full((K2B_USERS * ring_bytes,), SENT, dtype=torch.uint8, device="cuda")
    ops.fanout_wave(dev_bytes(inp["buf"]), inp["poff"].to("cuda"), plen.to("cuda"), pairs,
                    torch.tensor([_i32(s) for s in seq], dtype=torch.int32, device="cuda"),
                    torch.tensor([n_pairs], dtype=torch.int32, device="cuda"), egress, 1, 0)
    torch.cuda.synchronize()
    got = egress.cpu().numpy().tobytes()
    assert got == bytes(want), first_diff(got, bytes(want))


def test_k2b_nonuniform_pair_capacity_invariants(ops, k2b_inputs):
    """capacity below the delivery count: WHICH users land under the
    boundary depends on atomic claim order, so only aggregate invariants —
    every claim counted, exactly `capacity` rows written, the excess dropped,
    each user's accepted records consecutive from its start cursor."""
    inp = k2b_inputs
    plen = inp["plen"]
    ring_bytes = 1 << 15                      # everything would fit the rings
    cap = inp["total"] // 2
    wpos0 = _wpos_stagger()
    pairs, wpos, drops, n_pairs = _gpu_assign(ops, "fused", inp, plen, ring_bytes, wpos0,
                                              cap, 0)
    rows = pairs_from_dev(pairs)
    assert n_pairs == inp["total"]
    assert drops == inp["total"] - cap
    assert all(u >= 0 for u, _, _ in rows), "every in-capacity slot holds a real pair"
    assert len({(u, mi) for u, mi, _ in rows}) == cap
    cur = wpos0.tolist()
    last_msg = {}
    mt = inp["mask_t"]
    for u, mi, dst in rows:                   # slot order
        assert 0 <= u < K2B_USERS and (int(mt[u >> 6, mi]) >> (u & 63)) & 1
        assert last_msg.get(u, -1) < mi       # per-user message order
        last_msg[u] = mi
        assert dst == u * ring_bytes + cur[u]
        cur[u] += ring_rec(int(plen[mi]))
    assert wpos.tolist() == cur


@pytest.mark.parametrize("variant", ["fused", "blocks"])
def test_k2b_uniform_matches_reference(ops, k2b_inputs, variant):
    """uniform_rec != 0 branch of k2b_fused_t and the block-parallel
    P1/P2/P3 pipeline at the same 130 x 70 shape (tail word + stray bits,
    M not a multiple of the 32-message block): equal to the model run with a
    constant length, in all three ring regimes."""
    inp = k2b_inputs
    length = 200
    rec = ring_rec(length)
    plen = torch.full((K2B_M,), length, dtype=torch.int32)
    for ring_bytes, wpos0 in [
        (1 << 15, torch.zeros(K2B_USERS, dtype=torch.int64)),
        (rec * 5, torch.zeros(K2B_USERS, dtype=torch.int64)),
        (rec * 8 + 32, _wpos_stagger()),
    ]:
        _rows_r, segs, wpos_r, drops_r = _ref_assign(inp, plen, ring_bytes, wpos0)
        pairs, wpos, drops, n_pairs = _gpu_assign(ops, variant, inp, plen, ring_bytes, wpos0,
                                                  inp["total"] + 16, rec)
        label = f"{variant} ring={ring_bytes}"
        assert n_pairs == inp["total"], label
        assert drops == drops_r, label
        assert torch.equal(wpos, wpos_r), label
        _assert_pairs_per_user(pairs_from_dev(pairs)[:n_pairs], segs, label)


# ===========================================================================
# (c) K5b emit_direct
# ===========================================================================

K5B_LOCAL = 3   # local users 0, 1, 2


@pytest.fixture(scope="module")
def k5b_inputs():
    rng = random.Random(55)
    M = 300
    disc, owner, plen = [], [], []
    for _ in range(M):
        disc.append(3 if rng.random() < 0.67 else rng.choice([0, 4, 5, 7, -1]))
        r = rng.random()
        if r < 0.75:
            owner.append(rng.randrange(K5B_LOCAL))
        elif r < 0.9:
            owner.append(-rng.randrange(2, 9))         # remote broker -(rank+2)
        else:
            owner.append(INT32_MIN)                    # not found
        plen.append(rng.randrange(1, 501))
    elig = [i for i in range(M) if disc[i] == 3 and owner[i] >= 0]
    need = [sum(ring_rec(plen[i]) for i in elig if owner[i] == u) for u in range(K5B_LOCAL)]
    assert min(need) > 4000 and len(elig) < M - 60
    ring_bytes = max(need) + 64
    # user 0 holds everything; user 1's ring holds about half; user 2 starts
    # at a small offset
    wpos0 = [0, (ring_bytes - need[1] // 2) & ~15, 48]
    assert wpos0[0] + need[0] <= ring_bytes and wpos0[1] + need[1] > ring_bytes
    return dict(M=M, disc=disc, owner=owner, plen=plen, elig=elig, ring_bytes=ring_bytes,
                wpos0=wpos0)


K5B_PRESET = [(9, 1, 16 * 1234), (-1, 2, 0), (7, 3, 16), (8, 0, 4096), (9, 4, 160)]


def _run_k5b(ops, inp, capacity):
    K = len(K5B_PRESET)
    pairs = torch.full((capacity, 4), -7, dtype=torch.int32, device="cuda")
    pairs[:K] = pairs_to_dev(K5B_PRESET)
    wpos = torch.tensor(inp["wpos0"], dtype=torch.int64, device="cuda")
    n_pairs = torch.tensor([K], dtype=torch.int32, device="cuda")
    drops = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.emit_direct(torch.tensor(inp["disc"], dtype=torch.int32, device="cuda"),
                    torch.tensor(inp["owner"], dtype=torch.int32, device="cuda"),
                    torch.zeros(inp["M"], dtype=torch.int64, device="cuda"),
                    torch.tensor(inp["plen"], dtype=torch.int32, device="cuda"),
                    inp["ring_bytes"], wpos, n_pairs, pairs, drops)
    torch.cuda.synchronize()
    return (pairs_from_dev(pairs), wpos.cpu().tolist(), int(n_pairs.cpu()[0]),
            int(drops.cpu()[0]))


def _check_k5b_rows(inp, rows, wpos, K):
    """Per-user claim invariants over the rows K5b wrote (rows[K:])."""
    ring_bytes, plen, owner = inp["ring_bytes"], inp["plen"], inp["owner"]
    elig = set(inp["elig"])
    assert rows[:K] == K5B_PRESET, "existing broadcast pairs must stay untouched"
    written = rows[K:]
    msgs = [mi for _, mi, _ in written]
    assert len(set(msgs)) == len(msgs), "one row per message at most"
    assert set(msgs) <= elig, "remote / missing / non-Direct rows emit nothing"
    accepted = {u: [] for u in range(K5B_LOCAL)}
    dropped = []
    for u, mi, dst in written:
        if u < 0:
            assert (u, dst) == (-1, 0)
            dropped.append(mi)
            continue
        assert u == owner[mi]
        off = dst - u * ring_bytes
        accepted[u].append((off, off + ring_rec(plen[mi])))
    for u in range(K5B_LOCAL):
        # pairwise disjoint AND tiling [wpos0, wpos_final) exactly
        pos = inp["wpos0"][u]
        for lo, hi in sorted(accepted[u]):
            assert lo == pos, f"user {u}: gap or overlap at {lo} (expected {pos})"
            pos = hi
        assert pos == wpos[u] <= ring_bytes
    for mi in dropped:
        assert wpos[owner[mi]] + ring_rec(plen[mi]) > ring_bytes, "dropped although it fits"
    return accepted, dropped


def test_k5b_emit_direct_invariants(ops, k5b_inputs):
    """k5b_emit_direct at mixed lengths, three local owners, remote /
    missing owners, non-Direct rows, appended behind K existing pairs."""
    inp = k5b_inputs
    K, n_elig = len(K5B_PRESET), len(inp["elig"])
    cap = K + n_elig + 8
    rows, wpos, n_pairs, drops = _run_k5b(ops, inp, cap)
    assert n_pairs == K + n_elig
    assert all(r == UNWRITTEN for r in rows[n_pairs:])
    assert all(r != UNWRITTEN for r in rows[K:n_pairs])
    accepted, dropped = _check_k5b_rows(inp, rows[:n_pairs], wpos, K)
    assert sum(len(v) for v in accepted.values()) + len(dropped) == n_elig
    assert drops == len(dropped)
    assert {mi for _, mi, _ in rows[K:n_pairs]} == set(inp["elig"])
    # the regimes really happened: user 0 took everything, user 1 about half
    assert all(inp["owner"][mi] != 0 for mi in dropped)
    n1 = sum(1 for mi in inp["elig"] if inp["owner"][mi] == 1)
    assert 0 < len(accepted[1]) < n1


def test_k5b_emit_direct_pair_capacity(ops, k5b_inputs):
    """capacity < K + eligible: every claim is still counted, the excess is
    dropped, and the tensor has EXACTLY `capacity` rows — all of them
    written, none past them touched."""
    inp = k5b_inputs
    K, n_elig = len(K5B_PRESET), len(inp["elig"])
    cap = K + n_elig // 2
    rows, wpos, n_pairs, drops = _run_k5b(ops, inp, cap)
    assert len(rows) == cap
    assert n_pairs == K + n_elig
    assert all(r != UNWRITTEN for r in rows[K:])
    accepted, dropped = _check_k5b_rows(inp, rows, wpos, K)
    assert sum(len(v) for v in accepted.values()) + len(dropped) == cap - K
    assert drops == (K + n_elig - cap) + len(dropped)


# ===========================================================================
# (d) K7 compact_rings / drain_compact
# ===========================================================================

K7_RING = 4 * 65536 + 64
K7_WPOS = [0, 16, 65520, 65536, 65552, 3 * 65536 + 32, 0]


@pytest.fixture(scope="module")
def k7_inputs():
    rng = random.Random(7)
    egress = rng.randbytes(len(K7_WPOS) * K7_RING)
    offsets, want = ref.compact_rings(egress, K7_RING, K7_WPOS)
    assert offsets[-1] == len(want) == sum(K7_WPOS)
    return egress, offsets, want


def _run_k7(ops, egress_dev, wpos, offsets, max_chunks):
    total = offsets[-1]
    staging = torch.full((total + 4096,), SENT, dtype=torch.uint8, device="cuda")
    ops.compact_rings(egress_dev, K7_RING,
                      torch.tensor(wpos, dtype=torch.int64, device="cuda"),
                      torch.tensor(offsets[:-1], dtype=torch.int64, device="cuda"),
                      staging, max_chunks)
    torch.cuda.synchronize()
    return staging.cpu().numpy().tobytes()


@pytest.mark.parametrize("extra_chunks", [0, 5])
def test_k7_compact_rings_multichunk(ops, k7_inputs, extra_chunks):
    """k7_compact_rings called directly: rings spanning 1..4 64 KiB chunks
    (blockIdx.y > 0), used sizes just below / at / just above a chunk
    boundary (the `end` clamp), empty rings first and last; staging beyond
    `total` untouched; surplus chunks are no-ops."""
    egress, offsets, want = k7_inputs
    total = offsets[-1]
    max_chunks = (max(K7_WPOS) + (64 << 10) - 1) // (64 << 10)   # as drain_compact
    assert max_chunks == 4
    got = _run_k7(ops, dev_bytes(egress), K7_WPOS, offsets, max_chunks + extra_chunks)
    assert got[total:] == bytes([SENT]) * 4096, "wrote past the compacted data"
    assert got[:total] == want, first_diff(got[:total], want)


@pytest.mark.parametrize("max_chunks", [0, 2])
def test_k7_compact_rings_all_empty(ops, k7_inputs, max_chunks):
    egress, _, _ = k7_inputs
    zeros = [0] * len(K7_WPOS)
    got = _run_k7(ops, dev_bytes(egress), zeros, [0] * (len(K7_WPOS) + 1), max_chunks)
    assert got == bytes([SENT]) * 4096


def test_drain_compact_matches_ring_reads_regrowth_and_flip(ops):
    """Two identical GPU engines on the same ticks, one drained with
    drain_compact() (K7 + one D2H), one with drain_cursors() + read_ring:
    small drain, a drain > 4 MiB (staging regrowth, multi-chunk rings),
    small drain again.  Each (wpos, offsets, staging) equals the per-ring
    reads, cursors are zero afterwards, and the buffer returned by drain n
    is intact after drain n+1 (double-buffer flip)."""
    n_users, ring_bytes = 6, 1 << 20

    def make():
        eng = GpuBrokerEngine(device="cuda:0", n_users=n_users, ring_bytes=ring_bytes,
                              direct_table_size=64, fanout_wire=True, direct_enabled=True,
                              pair_capacity=1 << 12)
        for u in (0, 1, 2, 4, 5):          # user 3: an empty ring between used ones
            eng.subscribe(u, [1])
        eng.subscribe(0, [2])
        eng.subscribe(5, [2, 9])
        eng.register_direct(b"user-two", 2)
        return eng

    a, b = make(), make()
    rng = random.Random(12)
    small1 = [m.Broadcast([2], rng.randbytes(77)), m.Direct(b"user-two", rng.randbytes(301)),
              m.Broadcast([9], rng.randbytes(5)), m.Broadcast([1], rng.randbytes(1000))]
    large = [m.Broadcast([1], rng.randbytes(4096 + (i % 7))) for i in range(210)]
    small2 = [m.Broadcast([9], rng.randbytes(33)), m.Broadcast([2], rng.randbytes(640)),
              m.Direct(b"user-two", rng.randbytes(9))]
    prev = None
    for n, (msgs, big) in enumerate([(small1, False), (large, True), (small2, False)]):
        batch, offs = make_batch(msgs)
        for eng in (a, b):
            dbuf, doff = eng.ingest(batch, offs)
            eng.tick(dbuf, doff)
        torch.cuda.synchronize()
        wpos, offsets, staging = a.drain_compact()
        wpos_b = b.drain_cursors()
        assert int(a._drops.cpu()[0]) == 0 and int(b._drops.cpu()[0]) == 0
        assert torch.equal(wpos, wpos_b)
        assert int(wpos[3]) == 0 and int(wpos[0]) > 0 and int(wpos[5]) > 0
        assert offsets.tolist() == [0] + list(itertools.accumulate(wpos.tolist()))
        total = int(offsets[-1])
        assert staging.numel() == total
        assert (total > (1 << 22)) == big and total < (8 << 20)
        if big:
            assert int(wpos.max()) > 3 * 65536          # multi-chunk rings
        got = staging.numpy().tobytes()
        for u in range(n_users):
            ring = b.read_ring(u, int(wpos_b[u]))
            lo, hi = int(offsets[u]), int(offsets[u + 1])
            assert got[lo:hi] == ring, f"drain {n} user {u}: {first_diff(got[lo:hi], ring)}"
        assert int(a.ring_wpos.cpu().sum()) == 0 and int(b.ring_wpos.cpu().sum()) == 0
        if prev is not None:
            assert prev[0].numpy().tobytes() == prev[1], f"drain {n} clobbered drain {n - 1}"
        prev = (staging, got)


# ===========================================================================
# (e) small kernels: K2c apply_subs, K2a topic_mask_t, K5 direct_lookup
# ===========================================================================

def test_apply_subs_matches_reference(ops):
    """k2c_apply_subs against the serial model on ~200 mixed updates; the
    WHOLE bitmap is compared."""
    rng = random.Random(31)
    n_users = 200
    W = (n_users + 63) // 64
    edge_users = [0, 63, 64, n_users - 1]
    sub = torch.zeros((256, W), dtype=torch.int64)
    for _ in range(300):                       # pre-existing subscriptions
        t, u = rng.choice([0, 1, 7, 255, rng.randrange(256)]), rng.randrange(n_users)
        sub[t, u >> 6] = _i64(int(sub[t, u >> 6]) | (1 << (u & 63)))
    for u in edge_users:
        sub[255, u >> 6] = _i64(int(sub[255, u >> 6]) | (1 << (u & 63)))
    msgs, uidx = [], []
    for _ in range(200):
        k = rng.randrange(12)
        topics = [rng.choice([0, 1, 7, 255, rng.randrange(256)])
                  for _ in range(rng.choice([0, 1, 1, 2, 3, 6]))]
        if k < 5:
            msgs.append(m.Subscribe(topics + topics[:1]))      # duplicate topic
        elif k < 9:
            msgs.append(m.Unsubscribe(topics))
        elif k == 9:
            msgs.append(m.Broadcast(topics, b"bcast"))
        elif k == 10:
            msgs.append(m.Direct(b"someone", b"direct"))
        else:
            msgs.append(m.UserSync(b"sync"))
        r = rng.random()
        uidx.append(-1 if r < 0.08 else rng.choice(edge_users) if r < 0.5
                    else rng.randrange(n_users))
    # subscribe -> unsubscribe -> subscribe of ONE (user, topic) in one batch,
    # and the reverse: the final state depends on message order
    for u, t in ((63, 200), (64, 201)):
        msgs += [m.Subscribe([t]), m.Unsubscribe([t, t]), m.Subscribe([t])]
        uidx += [u, u, u]
    msgs += [m.Unsubscribe([255]), m.Subscribe([255]), m.Unsubscribe([255])]
    uidx += [n_users - 1] * 3
    buf, offsets = make_batch(msgs)
    pr = ref.parse_batch(buf, offsets)
    want = sub.clone()
    user_idx = torch.tensor(uidx, dtype=torch.int32)
    ref.apply_subs(want, buf, pr.topics_off, pr.topics_cnt, pr.disc, user_idx)
    assert not torch.equal(want, sub)
    assert (int(want[200, 0]) >> 63) & 1 and int(want[201, 1]) & 1
    assert not (int(want[255, (n_users - 1) >> 6]) >> ((n_users - 1) & 63)) & 1

    got = sub.to("cuda")
    ops.apply_subs(got, dev_bytes(buf), pr.topics_off.to("cuda"), pr.topics_cnt.to("cuda"),
                   pr.disc.to("cuda"), user_idx.to("cuda"))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)


def test_topic_mask_t_matches_reference(ops):
    """k2a_topic_mask_t == ref.topic_mask(...).T at W=3, M=70: duplicate
    topics, topic 255, zero topics, non-broadcast rows (which must come back
    ZERO although the output is torch.empty)."""
    rng = random.Random(19)
    W, M = 3, 70
    sub = torch.tensor([[_i64(rng.getrandbits(64)) if rng.random() < 0.5 else 0
                         for _ in range(W)] for _ in range(256)], dtype=torch.int64)
    sub[255, 2] = _i64(1 << 63)
    msgs = []
    for i in range(M):
        k = i % 7
        t = [rng.randrange(256) for _ in range(rng.randrange(1, 5))]
        if k == 0:
            msgs.append(m.Broadcast([], b"no-topics"))
        elif k == 1:
            msgs.append(m.Broadcast(t + t + [255], b"dup"))
        elif k == 2:
            msgs.append(m.Subscribe(t))             # has topics, is no broadcast
        elif k == 3:
            msgs.append(m.Direct(b"key", b"payload"))
        elif k == 4:
            msgs.append(m.Broadcast([255], b"top"))
        else:
            msgs.append(m.Broadcast(t, b"x" * rng.randrange(40)))
    buf, offsets = make_batch(msgs)
    pr = ref.parse_batch(buf, offsets)
    want = ref.topic_mask(sub, buf, pr.topics_off, pr.topics_cnt, pr.disc).T.contiguous()
    assert int((want != 0).sum()) > M
    # dirty the allocator block the kernel's torch.empty output will reuse
    junk = torch.full((W, M), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    del junk
    got = ops.topic_mask_t(sub.to("cuda"), dev_bytes(buf), pr.topics_off.to("cuda"),
                           pr.topics_cnt.to("cuda"), pr.disc.to("cuda"))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (W, M)
    assert torch.equal(got.cpu(), want)
    for i in range(M):
        if int(pr.disc[i]) != 4 or int(pr.topics_cnt[i]) == 0:
            assert not bool(got[:, i].cpu().any()), f"row {i} must be zero"


@pytest.mark.parametrize("size", [8, 64])
def test_direct_lookup_full_table_wrap_and_high_bit(ops, size):
    """k5_direct_lookup on a COMPLETELY full table (the probe loop must end
    by its bound, not by an empty slot), clusters wrapping from slot S-1 to
    slot 0, hashes with bit 63 set, query 0 and negative owners."""
    rng = random.Random(size)
    hi = 1 << 63

    def key_for(slot, high):
        k = (rng.getrandbits(50) << 8 | slot) & ~(size - 1) | slot
        return (k | hi) if high else (k & ~hi)

    def run(entries, queries):
        keys, vals = ref.build_direct_table(entries, size)
        q = torch.tensor([_i64(h) for h in queries], dtype=torch.int64)
        want = ref.direct_lookup(keys, vals, q)
        got = ops.direct_lookup(keys.to("cuda"), vals.to("cuda"), q.to("cuda"))
        torch.cuda.synchronize()
        assert torch.equal(got.cpu(), want)
        return keys, want.tolist()

    # 1) partly filled: a 4-key cluster homed at the LAST slot wraps to 0, 1, 2
    cluster = [(key_for(size - 1, i % 2 == 0), -(i + 2) if i % 2 else i) for i in range(4)]
    others = [(key_for(3, True), 7), (key_for(4, False), INT32_MIN + 1), (key_for(3, False), -2)]
    entries = cluster + others if size > 8 else cluster + others[:2]
    absent = [key_for(size - 1, True), key_for(size - 1, False), key_for(3, True),
              key_for(5, False)]
    assert not {h for h, _ in entries} & set(absent)
    keys, want = run(entries, [h for h, _ in entries] + absent + [0])
    assert int(keys[0]) != 0 and int(keys[1]) != 0 and int(keys[2]) != 0   # wrapped
    assert want == [o for _, o in entries] + [INT32_MIN] * (len(absent) + 1)

    # 2) completely full table
    full = []
    while len(full) < size:
        h = key_for(rng.randrange(size), rng.random() < 0.5)
        if h not in {x for x, _ in full} and h not in absent:
            full.append((h, rng.choice([len(full), -(len(full) + 2)])))
    keys, want = run(full, [h for h, _ in full] + absent + [0])
    assert all(int(k) != 0 for k in keys)
    assert want == [o for _, o in full] + [INT32_MIN] * (len(absent) + 1)


# ===========================================================================
# (f) live-shape engine: non-uniform wire tick, K5/K5b, wave NT, K7 drain
# ===========================================================================

def test_live_shape_engine_matches_cpu(ops):
    """The live broker's configuration (fanout_wire, direct routing, NT
    fan-out, uniform_wire_len=None) against the CPU engine: ~200 users,
    three ticks WITHOUT draining, unpadded Broadcast + Direct messages up to
    ~5 KiB, heavy subscribers overflowing their rings while Direct
    recipients keep room."""
    rng = random.Random(2024)
    n_users, ring_bytes = 200, 32 << 10
    kw = dict(n_users=n_users, ring_bytes=ring_bytes, direct_table_size=512,
              fanout_wire=True)
    cpu = GpuBrokerEngine(device="cpu", use_gpu_ops=False, **kw)
    gpu = GpuBrokerEngine(device="cuda:0", direct_enabled=True, nt_fanout=True,
                          pair_capacity=1 << 15, **kw)
    heavy = [0, 63, 64, 127, 128, 199]                 # every topic: will overflow
    direct_users = list(range(150, 170))               # subscribe to nothing
    keys = {u: b"direct-key-%d" % u for u in direct_users}
    for eng in (cpu, gpu):
        for u in range(n_users):
            if u in heavy:
                eng.subscribe(u, list(range(6)))
            elif u not in direct_users:
                eng.subscribe(u, [u % 6])
        eng.register_direct_bulk([(keys[u], u) for u in direct_users]
                                 + [(b"remote-user", -3)])
    sizes = [0, 1, 15, 16, 17, 100, 1000, 1023, 1025, 3000, 4097, 5000]
    cpu_drops = 0
    for tick in range(3):
        msgs = []
        for i in range(36):
            n = rng.choice(sizes) if i % 3 else rng.randrange(5001)
            r = rng.random()
            if r < 0.55:
                msgs.append(m.Broadcast([rng.randrange(6)], rng.randbytes(n)))
            elif r < 0.85:
                msgs.append(m.Direct(keys[rng.choice(direct_users)], rng.randbytes(n)))
            elif r < 0.9:
                msgs.append(m.Direct(b"remote-user", rng.randbytes(n)))
            elif r < 0.95:
                msgs.append(m.Direct(b"nobody-here", rng.randbytes(n)))
            else:
                msgs.append(m.UserSync(rng.randbytes(n)))
        batch, offsets = make_batch(msgs)
        assert any((b - a) % 16 for a, b in zip(offsets, offsets[1:]))   # unpadded
        bc, oc = cpu.ingest(batch, offsets)
        cpu_drops += cpu.tick(bc, oc, host_batch=batch, host_offsets=offsets).n_drops
        bg, og = gpu.ingest(batch, offsets)
        gpu.tick(bg, og)                                # uniform_wire_len=None
    torch.cuda.synchronize()
    wpos_c, wpos_g = cpu.ring_wpos.clone(), gpu.ring_wpos.cpu()
    assert torch.equal(wpos_c, wpos_g)
    assert cpu_drops > 0, "heavy subscribers must overflow"
    assert int(gpu._drops.cpu()[0]) == cpu_drops
    n_direct = 0
    for u in range(n_users):
        rc = parse_ring_records(cpu.read_ring(u), int(wpos_c[u]))
        rg = parse_ring_records(gpu.read_ring(u), int(wpos_g[u]))
        assert rc == rg, f"user {u}"
        if u in direct_users:
            n_direct += len(rc)
            assert int(wpos_c[u]) < ring_bytes // 2     # direct recipients keep room
    assert n_direct > 15

    wc, oc, sc = cpu.drain_compact()
    wg, og, sg = gpu.drain_compact()
    assert torch.equal(wc, wg) and torch.equal(oc, og) and torch.equal(wc, wpos_c)
    bc, bg = sc.numpy().tobytes(), sg.numpy().tobytes()
    for u in range(n_users):
        lo, hi = int(oc[u]), int(oc[u + 1])
        assert parse_ring_records(bc[lo:hi], hi - lo) == parse_ring_records(bg[lo:hi], hi - lo), \
            f"user {u}"
    assert int(gpu.ring_wpos.cpu().sum()) == 0
