"""Per-recipient loss accounting on the GPU: K9 recipient_demand and K10
loss_scan (module pushcdn_gpu_acct) against their models, and the GPU engine
against the CPU engine against plain arithmetic.

Everything is exact integer equality."""

import random

import pytest
import torch

from pushcdn_amd.broker.gpu_engine import ring_rec
from pushcdn_amd.ops import reference as ref
from tests import loss_accounting_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INT32_MIN = -(2**31)
NU, NP = 67, 3
R, W = NU + NP, 2                 # the last mask word is partial (6 valid lanes)
LENS = (0, 1, 15, 16, 17, 4000)
U64 = (1 << 64) - 1


def _i64(x):
    return x - (1 << 64) if x >= (1 << 63) else x


@pytest.fixture(scope="module")
def acct():
    from pushcdn_amd.ops import get_gpu_acct_ops

    return get_gpu_acct_ops()


def run_demand(acct, mask, ring_len, disc, owner, origin, demand):
    """K9 on the transposed mask; returns the new demand (CPU), the inputs
    untouched."""
    dev = lambda t: None if t is None else t.to(DEV)
    d = demand.to(DEV)
    acct.recipient_demand(d, mask.t().contiguous().to(DEV), dev(ring_len), dev(disc),
                          dev(owner), dev(origin), NU, NP)
    torch.cuda.synchronize()
    return d.cpu()


def model_demand(mask, ring_len, disc, owner, origin, demand):
    want = demand.clone()
    ref.recipient_demand(mask, ring_len, disc, owner, origin, NU, NP, want)
    return want


def mixed_tick(M, seed):
    """M messages: Broadcasts whose mask words cycle through all-ones,
    all-zeros, single bits at lane 0, lane 63 and the last valid lane, and
    random words; every fourth message a Direct."""
    rng = random.Random(seed)
    last_valid = (R - 1) & 63
    words = [U64, 0, 1, 1 << 63, 1 << last_valid]
    mask = torch.zeros((M, W), dtype=torch.int64)
    disc = torch.full((M,), 4, dtype=torch.int32)
    owner = torch.full((M,), INT32_MIN, dtype=torch.int32)
    origin = torch.zeros(M, dtype=torch.int32)
    owners = [0, NU - 1, -2, -(NP + 1), -(NP + 2), -1, NU, INT32_MIN, 2**31 - 1]
    for m in range(M):
        if m % 4 == 3:
            disc[m] = 3
            owner[m] = owners[(m // 4) % len(owners)]
            origin[m] = (m // 4) % 3 == 1
            continue
        for w in range(W):
            k = (m + 2 * w) % (len(words) + 2)
            word = words[k] if k < len(words) else rng.getrandbits(64)
            mask[m, w] = _i64(word)
    ring_len = torch.tensor([LENS[(m * 5 + m // 7) % len(LENS)] for m in range(M)],
                            dtype=torch.int32)
    return mask, ring_len, disc, owner, origin


# 37 crosses a 32-message block and leaves waves without a message; 257 gives
# every wave more than one message and the last one a remainder
@pytest.mark.parametrize("M", [0, 1, 37, 257])
def test_demand_matches_the_model(acct, M):
    per = (M + acct._K9_WAVES - 1) // acct._K9_WAVES
    if M == 257:
        assert per > 1 and M % per != 0
    mask, ring_len, disc, owner, origin = mixed_tick(M, seed=M)
    if M == 1:
        mask[0] = torch.tensor([-1, -1])        # one all-ones Broadcast
    demand = torch.arange(1, R + 1, dtype=torch.int64) * 1000   # accumulates
    want = model_demand(mask, ring_len, disc, owner, origin, demand)
    got = run_demand(acct, mask, ring_len, disc, owner, origin, demand)
    assert got.tolist() == want.tolist()
    if M:
        assert got.tolist() != demand.tolist()
    # no origin: all local; no owner: no Directs
    for own, org in ((owner, None), (None, None)):
        want = model_demand(mask, ring_len, disc, own, org, demand)
        assert run_demand(acct, mask, ring_len, disc, own, org, demand).tolist() \
            == want.tolist()


def test_demand_of_each_direct_case(acct):
    # (owner, origin) -> the recipient it must reach, None = nobody
    rows = [
        ((5, 0), 5),                     # to a user
        ((5, 1), 5),                     # to a user, from a peer broker
        ((-2, 0), NU),                   # to peer slot 0, local origin
        ((-(NP + 1), 0), NU + NP - 1),   # to the last peer slot
        ((-2, 1), None),                 # to a peer from remote origin
        ((-(NP + 2), 0), None),          # p >= n_peers
        ((INT32_MIN, 0), None),          # not found
        ((-1, 0), None),                 # owner -1
        ((NU, 0), None),                 # owner >= n_users
        ((2**31 - 1, 0), None),
    ]
    rows += [((9, 0), 9)] * 64           # contention on one recipient
    M = len(rows)
    mask = torch.zeros((M, W), dtype=torch.int64)
    ring_len = torch.tensor([LENS[i % len(LENS)] for i in range(M)], dtype=torch.int32)
    disc = torch.full((M,), 3, dtype=torch.int32)
    owner = torch.tensor([o for (o, _g), _r in rows], dtype=torch.int32)
    origin = torch.tensor([g for (_o, g), _r in rows], dtype=torch.int32)
    want = [7] * R
    for ((_o, _g), r), n in zip(rows, ring_len.tolist()):
        if r is not None:
            want[r] += ring_rec(n)
    demand = torch.full((R,), 7, dtype=torch.int64)
    assert model_demand(mask, ring_len, disc, owner, origin, demand).tolist() == want
    assert run_demand(acct, mask, ring_len, disc, owner, origin, demand).tolist() == want
    # a disc other than 3 is no Direct
    disc[:] = 4
    assert run_demand(acct, mask, ring_len, disc, owner, origin, demand).tolist() == [7] * R


def run_scan(acct, demand, wpos):
    n = demand.numel()
    d, w = demand.to(DEV), wpos.to(DEV)
    lossy = torch.full((n, 2), -7, dtype=torch.int64, device=DEV)
    n_lossy = torch.full((1,), 99, dtype=torch.int32, device=DEV)   # zeroed by the op
    n_host = torch.full((1,), 99, dtype=torch.int32).pin_memory()
    acct.loss_scan(d, w, lossy, n_lossy, n_host)
    torch.cuda.synchronize()
    k = int(n_host[0])
    assert k == int(n_lossy.cpu()[0])
    assert w.cpu().tolist() == wpos.tolist()            # cursors untouched
    assert d.cpu().tolist() == [0] * n                  # demand zeroed
    assert lossy[k:].cpu().tolist() == [[-7, -7]] * (n - k)   # nothing past the count
    return sorted(tuple(row) for row in lossy[:k].cpu().tolist())


@pytest.mark.parametrize("n", [1, 64, 70])
def test_loss_scan_matches_the_model(acct, n):
    wpos = (torch.arange(n, dtype=torch.int64) % 5) * 256
    scattered = wpos.clone()
    scattered[[i for i in (0, n // 2, n - 1)]] += 16
    if n > 64:
        scattered[[63, 64]] += 4000     # both sides of the wave boundary
    for demand in (wpos.clone(),        # nothing lost, cursors not all zero
                   wpos + 256,          # every recipient: n > 64 takes two waves
                   scattered):
        want = ref.loss_scan(demand.clone(), wpos)
        assert run_scan(acct, demand, wpos) == want
    assert ref.loss_scan(wpos.clone(), wpos) == []
    assert len(ref.loss_scan(wpos + 256, wpos)) == n


# ===========================================================================
# GPU engine against CPU engine against arithmetic
# ===========================================================================

@pytest.mark.parametrize("case", cases.EXPECTED, ids=lambda c: c.__name__)
def test_engine_case(case):
    want = cases.EXPECTED[case]
    assert case("cpu") == want
    assert case(DEV) == want


@pytest.mark.parametrize("how", cases.DRAINS)
@pytest.mark.parametrize("fused_drain", [True, False])
def test_every_drain_scans(how, fused_drain):
    """drain_cursors on both its paths (fused_tick picks the native one),
    drain_compact and drain_compact_ref."""
    eng = cases.make_engine(DEV, fused_tick=fused_drain)
    eng.subscribe(1, [cases.T])
    eng.subscribe(3, [cases.T])
    cases.tick(eng, [cases.bcast()] * 5)
    assert cases.drain(eng, how)[1] == cases.RING
    assert eng.take_losses() == {1: cases.REC, 3: cases.REC}
    cases.tick(eng, [cases.bcast()] * 4)
    assert cases.drain(eng, how)[3] == cases.RING
    assert eng.take_losses() == {}


def test_take_losses_merges_drains_and_clears():
    eng = cases.make_engine(DEV)
    eng.subscribe(1, [cases.T])
    for _ in range(2):
        cases.tick(eng, [cases.bcast()] * 5)
        cases.drain(eng)
    assert eng.take_losses() == {1: 2 * cases.REC}
    assert eng.take_losses() == {}


def test_accounting_off_loads_and_reports_nothing():
    eng = cases.make_engine(DEV, loss_accounting=False)
    assert eng._acct_ops is None and not hasattr(eng, "demand")
    eng.subscribe(1, [cases.T])
    cases.tick(eng, [cases.bcast()] * 5)
    assert cases.drain(eng)[1] == cases.RING
    assert eng.take_losses() == {}


def test_accounting_keeps_the_tick_off_the_fused_and_graphed_paths():
    from pushcdn_amd.broker.gpu_engine import GpuBrokerEngine
    from pushcdn_amd.proto import message as m

    eng = GpuBrokerEngine(device=DEV, n_users=8, ring_bytes=1024, fanout_wire=True,
                          direct_enabled=False, loss_accounting=True)
    eng.subscribe(1, [cases.T])
    msg = cases.bcast()
    offsets = cases.tick(eng, [msg] * 5)
    batch = m.serialize(msg) * 5
    buf, off = eng.ingest(batch, offsets)
    eng.tick(buf, off, uniform_wire_len=offsets[1])     # the fused tick's shape
    assert eng.fused_ticks == 0
    assert cases.drain(eng)[1] == cases.RING
    assert eng.take_losses() == {1: 10 * cases.REC - cases.RING}
    with pytest.raises(ValueError, match="loss_accounting"):
        eng.tick_graphed(buf, off, offsets[1])


def test_pair_list_overflow():
    """12 deliveries into a pair list of 8: which recipients lose is decided
    by claim order, the total is not."""
    eng = cases.make_engine(DEV, pair_capacity=8)
    users = (0, 2, 5)
    for u in users:
        eng.subscribe(u, [cases.T])
    cases.tick(eng, [cases.bcast()] * 4)       # 4 x 256 fills a ring exactly
    wpos = cases.drain(eng)
    losses = eng.take_losses()
    assert sum(losses.values()) == 4 * cases.REC
    demanded = {u: 4 * cases.REC for u in users}
    assert set(losses) <= set(users)
    for u in users:
        assert losses.get(u, 0) == demanded[u] - wpos[u]
    assert sum(wpos) == 8 * cases.REC
