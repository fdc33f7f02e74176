"""Per-recipient loss accounting without a GPU: the models
(ref.recipient_demand, ref.loss_scan) against hand-computed cases, the CPU
engine (device="cpu") against plain arithmetic, and the native boundary of
the accounting extension (csrc/gpu_acct_bindings.cpp, module
pushcdn_gpu_acct), which refuses a bad argument by name.

Everything is exact integer equality."""

import re

import pytest
import torch

from pushcdn_amd.broker.gpu_engine import ring_rec
from pushcdn_amd.ops import reference as ref
from tests import loss_accounting_cases as cases

INT32_MIN = -(2**31)


def i32(xs):
    return torch.tensor(list(xs), dtype=torch.int32)


def _i64(x):
    return x - (1 << 64) if x >= (1 << 63) else x


# ===========================================================================
# the models
# ===========================================================================

def test_recipient_demand_by_hand():
    n_users, n_peers = 66, 2          # R = 68, two mask words, the last partial
    # m0: Broadcast to recipients 0, 63 and 67 (peer slot 1), 100 B -> 128
    # m1: Broadcast to recipient 64, by reference (ring_len 0) -> 16
    # m2: Direct to user 65, 17 B -> 48
    # m3: Direct to peer slot 0 (recipient 66) from local origin, 16 B -> 32
    # m4: the same from remote origin -> nothing
    # m5: a Broadcast whose mask has a bit past R (recipient 68) -> nothing
    mask = torch.tensor([
        [_i64(1 | 1 << 63), 1 << 3],
        [0, 1 << 0],
        [0, 0], [0, 0], [0, 0],
        [0, 1 << 4],
    ], dtype=torch.int64)
    ring_len = i32([100, 0, 17, 16, 16, 4000])
    disc = i32([4, 4, 3, 3, 3, 4])
    owner = i32([INT32_MIN, INT32_MIN, 65, -2, -2, INT32_MIN])
    origin = i32([0, 0, 0, 0, 1, 0])
    demand = torch.zeros(68, dtype=torch.int64)
    demand[0] = 5                      # accumulates
    ref.recipient_demand(mask, ring_len, disc, owner, origin, n_users, n_peers, demand)
    want = [0] * 68
    want[0], want[63], want[67] = 5 + 128, 128, 128
    want[64], want[65], want[66] = 16, 48, 32
    assert demand.tolist() == want


def test_recipient_demand_direct_resolution():
    n_users, n_peers = 4, 2
    owners = [3, 4, -1, -2, -3, -4, INT32_MIN, 0]
    M = len(owners)
    mask = torch.zeros((M, 1), dtype=torch.int64)
    demand = torch.zeros(6, dtype=torch.int64)
    ref.recipient_demand(mask, i32([0] * M), i32([3] * M), i32(owners), None,
                         n_users, n_peers, demand)
    # 3 -> user 3; 4 -> not a user; -1 nothing; -2 -> peer 0; -3 -> peer 1;
    # -4 -> peer 2 >= n_peers; not found; 0 -> user 0
    assert demand.tolist() == [16, 0, 0, 16, 16, 16]
    # a disc other than 3 is no Direct, and owner None means no Directs routed
    demand.zero_()
    ref.recipient_demand(mask, i32([0] * M), i32([4] * M), i32(owners), None,
                         n_users, n_peers, demand)
    ref.recipient_demand(mask, i32([0] * M), i32([3] * M), None, None,
                         n_users, n_peers, demand)
    assert demand.tolist() == [0] * 6


def test_loss_scan_by_hand():
    demand = torch.tensor([0, 256, 1024, 16, 0], dtype=torch.int64)
    wpos = torch.tensor([0, 256, 768, 0, 0], dtype=torch.int64)
    before = wpos.clone()
    assert ref.loss_scan(demand, wpos) == [(2, 256), (3, 16)]
    assert demand.tolist() == [0] * 5 and torch.equal(wpos, before)
    assert ref.loss_scan(demand, torch.zeros(5, dtype=torch.int64)) == []


# ===========================================================================
# the CPU engine against arithmetic
# ===========================================================================

def test_the_messages_take_the_records_the_cases_assume():
    from pushcdn_amd.proto import message as m

    for msg in (cases.bcast(), cases.direct(), cases.direct(cases.REMOTE)):
        assert ring_rec(len(m.serialize(msg))) == cases.REC
    assert ring_rec(len(m.serialize(cases.bcast(rec=cases.BIG_REC)))) == cases.BIG_REC > cases.RING


@pytest.mark.parametrize("case", cases.EXPECTED, ids=lambda c: c.__name__)
def test_cpu_engine_case(case):
    assert case("cpu") == cases.EXPECTED[case]


@pytest.mark.parametrize("how", cases.DRAINS)
def test_every_drain_scans(how):
    assert cases.five_broadcasts("cpu", how) == cases.EXPECTED[cases.five_broadcasts]
    assert cases.four_broadcasts_fill_the_ring("cpu", how) \
        == cases.EXPECTED[cases.four_broadcasts_fill_the_ring]


def test_take_losses_merges_drains_and_clears():
    eng = cases.make_engine("cpu")
    eng.subscribe(1, [cases.T])
    for _ in range(2):
        cases.tick(eng, [cases.bcast()] * 5)
        cases.drain(eng)
    assert eng.take_losses() == {1: 2 * cases.REC}
    assert eng.take_losses() == {}
    # the demand did not outlive its drain
    cases.tick(eng, [cases.bcast()] * 4)
    cases.drain(eng)
    assert eng.take_losses() == {}


def test_accounting_off_allocates_and_reports_nothing():
    eng = cases.make_engine("cpu", loss_accounting=False)
    assert eng._acct_ops is None and not hasattr(eng, "demand")
    eng.subscribe(1, [cases.T])
    cases.tick(eng, [cases.bcast()] * 5)
    assert cases.drain(eng)[1] == cases.RING
    assert eng.take_losses() == {}


def test_accounting_leaves_the_fused_and_graphed_ticks():
    from pushcdn_amd.broker.gpu_engine import GpuBrokerEngine

    kw = dict(device="cpu", n_users=8, ring_bytes=1024, fanout_wire=True,
              direct_enabled=False)
    assert GpuBrokerEngine(**kw)._fused_tick_ok(64, None)
    eng = GpuBrokerEngine(loss_accounting=True, **kw)
    assert not eng._fused_tick_ok(64, None)
    with pytest.raises(ValueError, match="loss_accounting"):
        eng.tick_graphed(torch.zeros(1, dtype=torch.uint8),
                         torch.zeros(2, dtype=torch.int64), 64)


# ===========================================================================
# the native boundary: CPU tensors only, device check last
# ===========================================================================

needs_no_gpu = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="a missing check would launch a kernel on host memory; CPU-only machines only")

NU, NP, M = 67, 3, 5
R, W = NU + NP, 2


def i64(*shape):
    return torch.zeros(*shape, dtype=torch.int64)


def z32(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


@pytest.fixture(scope="module")
def ops():
    from pushcdn_amd.ops import get_gpu_acct_ops

    return get_gpu_acct_ops()


# op -> (valid argument list, {tensor argument: position}, first tensor first)
ROWS = {
    "recipient_demand": (
        lambda: [i64(R), i64(W, M), z32(M), z32(M), z32(M), z32(M), NU, NP],
        {"demand": 0, "mask_t": 1, "ring_len": 2, "disc": 3, "owner": 4, "origin": 5}),
    "loss_scan": (
        lambda: [i64(R), i64(R), i64(R, 2), z32(1), z32(1)],
        {"demand": 0, "ring_wpos": 1, "lossy": 2, "n_lossy": 3, "n_host": 4}),
}

VEC32 = {
    "dtype": lambda t: t.to(torch.int64),
    "strided": lambda t: t.repeat(2)[::2],
    "two dimensions": lambda t: t.reshape(-1, 1),
    "one short": lambda t: t[:-1].clone(),
    "one long": lambda t: z32(t.numel() + 1),
}

BAD = {
    "recipient_demand": {
        "demand": {
            "dtype": lambda t: t.to(torch.int32),
            "strided": lambda t: t.repeat(2)[::2],
            "two dimensions": lambda t: i64(R, 1),
            "not n_users + n_peers": lambda t: i64(R + 1),
        },
        "mask_t": {
            "dtype": lambda t: t.to(torch.int32),
            "strided": lambda t: t.repeat(1, 2)[:, ::2],
            "untransposed": lambda t: i64(M, W),
            "a word short": lambda t: i64(W - 1, M),
            "flat": lambda t: i64(W * M),
        },
        # M is ring_len's length: a wrong one is refused where the others meet it
        "ring_len": {k: VEC32[k] for k in ("dtype", "strided", "two dimensions", "one short")},
        "disc": VEC32,
        "owner": VEC32,
        "origin": VEC32,
    },
    "loss_scan": {
        "demand": {
            "dtype": lambda t: t.to(torch.int32),
            "strided": lambda t: t.repeat(2)[::2],
            "two dimensions": lambda t: i64(R, 1),
        },
        "ring_wpos": {
            "dtype": lambda t: t.to(torch.int32),
            "strided": lambda t: t.repeat(2)[::2],
            "two dimensions": lambda t: i64(R, 1),
            "one short": lambda t: i64(R - 1),
            "one long": lambda t: i64(R + 1),
        },
        "lossy": {
            "dtype": lambda t: t.to(torch.int32),
            "strided": lambda t: t.repeat(1, 2)[:, ::2],
            "three words": lambda t: i64(R, 3),
            "flat": lambda t: i64(R * 2),
            "a row short": lambda t: i64(R - 1, 2),
        },
        "n_lossy": {
            "dtype": lambda t: t.to(torch.int64),
            "empty": lambda t: z32(0),
            "two dimensions": lambda t: z32(1, 1),
        },
        "n_host": {
            "dtype": lambda t: t.to(torch.int64),
            "empty": lambda t: z32(0),
            "two dimensions": lambda t: z32(1, 1),
        },
    },
}


def _refusal(ops, op, args):
    with pytest.raises(RuntimeError) as exc:
        getattr(ops, op)(*args)
    return str(exc.value).splitlines()[0]


def _names(msg, *names):
    return all(re.search(rf"(?<![A-Za-z0-9_]){re.escape(n)}(?![A-Za-z0-9_])", msg)
               for n in names)


def test_table_covers_every_op(ops):
    assert set(ROWS) == {n for n in dir(ops) if not n.startswith("_")}
    assert {op: set(args) for op, args in BAD.items()} \
        == {op: set(tensors) for op, (_b, tensors) in ROWS.items()}


def test_the_other_modules_do_not_export_them():
    from pushcdn_amd.ops import get_gpu_ctl_ops, get_gpu_ops

    for mod in (get_gpu_ops(), get_gpu_ctl_ops()):
        assert not any(hasattr(mod, op) for op in ROWS)


@needs_no_gpu
@pytest.mark.parametrize("op", ROWS)
def test_valid_arguments_reach_the_device_check(ops, op):
    build, tensors = ROWS[op]
    msg = _refusal(ops, op, build())
    assert msg.startswith(f"{op}: {next(iter(tensors))} must be on a GPU, got cpu"), msg


@needs_no_gpu
def test_absent_owner_and_origin_and_an_empty_tick_are_still_checked(ops):
    args = ROWS["recipient_demand"][0]()
    args[4] = args[5] = None
    assert "demand must be on a GPU" in _refusal(ops, "recipient_demand", args)
    empty = [i64(R), i64(W, 0), z32(0), z32(0), None, None, NU, NP]
    assert "demand must be on a GPU" in _refusal(ops, "recipient_demand", empty)


@needs_no_gpu
@pytest.mark.parametrize("op,arg", [(op, arg) for op in BAD for arg in BAD[op]])
def test_each_bad_tensor_is_refused_by_name(ops, op, arg):
    build, tensors = ROWS[op]
    for kind, mutate in BAD[op][arg].items():
        args = build()
        bad = mutate(args[tensors[arg]])
        if kind == "strided":
            assert not bad.is_contiguous()
        args[tensors[arg]] = bad
        msg = _refusal(ops, op, args)
        # a ring_len of another length changes M: refused at the mask
        named = "mask_t" if (arg, kind) == ("ring_len", "one short") else arg
        assert _names(msg, op, named), f"{arg} {kind}: {msg}"
        assert "must be on a GPU" not in msg, f"{arg} {kind}: {msg}"


@needs_no_gpu
@pytest.mark.parametrize("n_users,n_peers,named", [
    (-1, NP + 1, "n_users"), (NU + 1, -1, "n_peers"), (NU, NP + 1, "demand"),
    (2**31, 0, "n_users"), (NU, 2**31, "n_peers"),
])
def test_bad_counts_are_refused_by_name(ops, n_users, n_peers, named):
    args = ROWS["recipient_demand"][0]()
    args[6], args[7] = n_users, n_peers
    msg = _refusal(ops, "recipient_demand", args)
    assert _names(msg, "recipient_demand", named), msg
    assert "must be on a GPU" not in msg, msg
