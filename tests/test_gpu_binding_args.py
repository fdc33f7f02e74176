"""The native boundary (csrc/gpu_bindings.cpp) refuses a bad argument by name.

Every op is called with CPU tensors only.  The bindings check dtype, stated
shape, contiguity and length first and the device LAST, so on a machine
without a GPU a fully valid argument list gets as far as "must be on a GPU"
and a single bad argument is refused before that, with a message that names
the op and the argument.  On a machine WITH a GPU a missing check would
launch a kernel on host or short memory, so the whole file is skipped there.
"""

import re

import pytest
import torch

from pushcdn_amd.ops import get_gpu_ops

pytestmark = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="a missing check would launch a kernel on host memory; CPU-only machines only")

# the smallest consistent shape
M, W, N_USERS, CAP, S, N, RING = 2, 1, 3, 4, 8, 1, 64
UNIFORM_LEN, REC = 16, 32        # ring_rec(16) = 32: two 16 B units per record
W64, NB = W * 64, 1              # the block K2b's scratch: NB = ceil(M / 32)


def u8(*shape):
    return torch.zeros(*shape, dtype=torch.uint8)


def i32(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


def i64(*shape):
    return torch.zeros(*shape, dtype=torch.int64)


@pytest.fixture(scope="module")
def ops():
    return get_gpu_ops()


class Row:
    """One op: `build(ops)` makes a valid argument list at the smallest
    shape; `tensors` maps each tensor argument's name to its position, first
    tensor first; `scalars` maps each narrowed scalar's name to (position,
    whether -1 is invalid).  `free` names the tensors the op asks no length
    of (or whose own length sets the count the others must match, with
    nothing to fall short of); `short` overrides the too-short value where
    dropping one element still leaves a valid, smaller batch."""

    def __init__(self, op, build, tensors, scalars=None, free=(), short=None):
        self.op, self.build, self.tensors = op, build, tensors
        self.scalars, self.free, self.short = scalars or {}, set(free), short or {}


def _topic(extra=()):
    return lambda ops: [i64(256, W), u8(16), i64(M), i32(M), i32(M), *[f() for f in extra]]


TOPIC_T = {"sub_bitmap": 0, "buf": 1, "topics_off": 2, "topics_cnt": 3, "disc": 4}
K1_T = {"vks": 0, "sigs": 1, "msgs": 2, "moff": 3}


def _k1(extra=()):
    return lambda ops: [u8(N * 128), u8(N * 64), u8(8), i64(N + 1), *[f() for f in extra]]


def _fan(*tail):
    """buf, payload_off, payload_len, pairs, then the op's own tail."""
    return lambda ops: [u8(16), i64(M), i32(M), i32(CAP, 4),
                        *[f() if callable(f) else f for f in tail]]


def _egress():
    return u8(N_USERS * RING)


def _tick(ops):
    n64, n32 = ops.uniform_tick_scratch_sizes(M, W, REC)
    return [u8(M * UNIFORM_LEN), i64(M + 1), 0, i64(256, W), i64(N_USERS), RING, N_USERS,
            i32(CAP, 4), i32(1), i32(1), i32(1), i64(n64), i32(n32), UNIFORM_LEN, 0,
            _egress(), 0, 1]


ROWS = [
    Row("parse_batch", lambda ops: [u8(16), i64(M + 1), 0], {"buf": 0, "offsets": 1},
        free={"buf"}, short={"offsets": i64(0)}),
    Row("topic_mask", _topic(), TOPIC_T, free={"buf"}),
    Row("topic_mask_t", _topic(), TOPIC_T, free={"buf"}),
    Row("topic_mask_origin_t", _topic([lambda: i32(M), lambda: N_USERS]),
        {**TOPIC_T, "origin": 5}, {"n_users": (6, True)}, free={"buf"}),
    Row("apply_subs", _topic([lambda: i32(M)]), {**TOPIC_T, "user_idx": 5}, free={"buf"}),
    Row("assign_emit", lambda ops: [i64(M, W), i64(M), i32(M), i64(N_USERS), RING, N_USERS],
        {"mask": 0, "payload_off": 1, "payload_len": 2, "ring_wpos": 3},
        {"n_users": (5, True)}),
    Row("fanout",
        lambda ops: [u8(16), i64(M), i32(M), i32(CAP), i32(CAP), i64(CAP), i32(M), _egress()],
        {"buf": 0, "payload_off": 1, "payload_len": 2, "pair_user": 3, "pair_msg": 4,
         "pair_dst": 5, "msg_seq": 6, "egress": 7}, free={"buf", "egress"}),
    Row("fanout_wave", _fan(lambda: i32(M), lambda: i32(1), _egress, 0, 1),
        {"buf": 0, "payload_off": 1, "payload_len": 2, "pairs": 3, "msg_seq": 4, "n_pairs": 5,
         "egress": 6}, {"grid": (8, True)}, free={"buf", "egress"}),
    Row("fanout_ref", _fan(lambda: i32(M), lambda: i32(1), _egress, 0, 1, 64, 0),
        {"buf": 0, "payload_off": 1, "payload_len": 2, "pairs": 3, "msg_seq": 4, "n_pairs": 5,
         "egress": 6}, {"grid": (8, True), "ref_threshold": (9, True)}, free={"buf", "egress"}),
    Row("fanout_flat2", _fan(0, lambda: i32(1), 2, _egress, 0, 1, 0),
        {"buf": 0, "payload_off": 1, "payload_len": 2, "pairs": 3, "n_pairs": 5, "egress": 7},
        {"units_per_pair": (6, True), "grid": (9, True), "uniform_len": (10, True)},
        free={"buf", "egress"}),
    Row("fanout_flat3", _fan(lambda: i32(1), lambda: i32(1), 2, _egress, 0, 1, 0),
        {"buf": 0, "payload_off": 1, "payload_len": 2, "pairs": 3, "seq_state": 4, "n_pairs": 5,
         "egress": 7},
        {"units_per_pair": (6, True), "grid": (9, True), "uniform_len": (10, True)},
        free={"buf", "egress"}),
    Row("seq_advance", lambda ops: [i32(1), M], {"seq_state": 0}, {"m": (1, True)}),
    Row("assign_emit_fused_t",
        lambda ops: [i64(W, M), i32(M), i64(N_USERS), RING, N_USERS, i32(CAP, 4), i32(1), i32(1),
                     0],
        {"mask_t": 0, "payload_len": 1, "ring_wpos": 2, "pairs": 5, "drops": 6, "n_pairs": 7},
        {"n_users": (4, True)}),
    Row("assign_emit_blocks_t",
        lambda ops: [i64(W, M), i64(N_USERS), RING, N_USERS, i32(NB * W64), i32(NB * W64),
                     i32(W64), i32(W64), i64(W64), i32(CAP, 4), i32(1), i32(1), REC],
        {"mask_t": 0, "ring_wpos": 1, "bcount": 4, "pprefix": 5, "ubase": 6, "ufit": 7,
         "udst": 8, "pairs": 9, "drops": 10, "n_pairs": 11},
        {"n_users": (3, True)}),
    Row("direct_lookup", lambda ops: [i64(S), i32(S), i64(M)],
        {"table_keys": 0, "table_vals": 1, "query": 2}, free={"query"}),
    Row("emit_direct",
        lambda ops: [i32(M), i32(M), i64(M), i32(M), RING, i64(N_USERS), i32(1), i32(CAP, 4),
                     i32(1)],
        {"disc": 0, "owner": 1, "payload_off": 2, "payload_len": 3, "ring_wpos": 5,
         "n_pairs": 6, "pairs": 7, "drops": 8}, free={"ring_wpos"}),
    Row("emit_direct_peers",
        lambda ops: [i32(M), i32(M), i32(M), i64(M), i32(M), RING, N_USERS, 1, i64(N_USERS + 1),
                     i32(1), i32(CAP, 4), i32(1)],
        {"disc": 0, "owner": 1, "origin": 2, "payload_off": 3, "payload_len": 4, "ring_wpos": 8,
         "n_pairs": 9, "pairs": 10, "drops": 11},
        {"n_users": (6, True), "n_peers": (7, True)}),
    # wpos' own length is the ring count: a shorter one is a smaller, valid call
    Row("compact_rings", lambda ops: [_egress(), RING, i64(N_USERS), i64(N_USERS), u8(16), 1],
        {"egress": 0, "wpos": 2, "dst_off": 3, "staging": 4}, {"max_chunks": (5, True)},
        free={"wpos", "staging"}),
    Row("direct_apply", lambda ops: [i64(S), i32(S), i64(2), i32(2), i64(1), i32(1)],
        {"table_keys": 0, "table_vals": 1, "up_keys": 2, "up_owners": 3, "del_keys": 4,
         "n_failed": 5}, free={"del_keys"}),
    Row("tick_uniform_broadcast", _tick,
        {"buf": 0, "offsets": 1, "sub_bitmap": 3, "ring_wpos": 4, "pairs": 7, "drops": 8,
         "n_pairs": 9, "n_sparse": 10, "scratch64": 11, "scratch32": 12, "egress": 15},
        {"n_users": (6, True), "uniform_len": (13, True)}, short={"offsets": i64(0)}),
    Row("drain_cursors", lambda ops: [i64(N_USERS), i64(N_USERS), i64(N_USERS)],
        {"ring_wpos": 0, "staging": 1, "host": 2}, free={"ring_wpos"}),   # as wpos above
    Row("bls_verify_batch", _k1(), K1_T, free={"msgs"}),
    Row("bls_verify_batch2", _k1([lambda: u8(128 * 192)]), {**K1_T, "g2_lines": 4},
        free={"msgs"}),
    Row("bls_verify_batch_wave", _k1([lambda: u8(128 * 192), lambda: i64(N)]),
        {**K1_T, "g2_lines": 4, "rand_r": 5}, free={"msgs"}),
    Row("hash_to_g1_batch", lambda ops: [u8(8), i64(N + 1)], {"msgs": 0, "moff": 1},
        free={"msgs"}, short={"moff": i64(0)}),
    Row("precompute_g2_lines", lambda ops: [u8(1)], {"device_probe": 0},
        free={"device_probe"}),
]

BY_OP = pytest.mark.parametrize("row", ROWS, ids=[r.op for r in ROWS])


def _refusal(ops, row, args):
    with pytest.raises(RuntimeError) as exc:
        getattr(ops, row.op)(*args)
    return str(exc.value).splitlines()[0]


def _names(msg, *names):
    return all(re.search(rf"(?<![A-Za-z0-9_]){re.escape(n)}(?![A-Za-z0-9_])", msg)
               for n in names)


def test_table_covers_every_op(ops):
    exported = {n for n in dir(ops) if not n.startswith("_")} - {"uniform_tick_scratch_sizes"}
    assert {r.op for r in ROWS} == exported


@BY_OP
def test_valid_arguments_reach_the_device_check(ops, row):
    """Every other check passed, and the device check ran last."""
    first = next(iter(row.tensors))
    msg = _refusal(ops, row, row.build(ops))
    assert msg.startswith(f"{row.op}: {first} must be on a GPU, got cpu"), msg


def _wrong_dtype(t):
    return t.to(torch.int64 if t.dtype == torch.int32 else torch.int32)


def _strided(t):
    # same sizes, every other element of a twice-as-long buffer
    return t.repeat(2)[::2] if t.dim() == 1 else t.repeat(1, 2)[:, ::2]


@BY_OP
def test_each_bad_tensor_is_refused_by_name(ops, row):
    for arg, pos in row.tensors.items():
        valid = row.build(ops)[pos]
        mutations = {"dtype": _wrong_dtype(valid)}
        if valid.numel() > 1:       # a one-element view is contiguous whatever its stride
            mutations["strided"] = _strided(valid)
            assert not mutations["strided"].is_contiguous()
        if arg in row.short:
            mutations["short"] = row.short[arg]
        elif arg not in row.free:
            mutations["short"] = valid.flatten()[:-1]
        for kind, bad in mutations.items():
            args = row.build(ops)
            args[pos] = bad
            msg = _refusal(ops, row, args)
            assert _names(msg, row.op, arg), f"{row.op} {arg} {kind}: {msg}"
            assert "must be on a GPU" not in msg, f"{row.op} {arg} {kind}: {msg}"


@BY_OP
def test_each_scalar_out_of_range_is_refused_by_name(ops, row):
    for name, (pos, negative_invalid) in row.scalars.items():
        for bad in [2 ** 31] + ([-1] if negative_invalid else []):
            args = row.build(ops)
            args[pos] = bad
            msg = _refusal(ops, row, args)
            assert _names(msg, name), f"{row.op} {name}={bad}: {msg}"
            assert "must be on a GPU" not in msg, f"{row.op} {name}={bad}: {msg}"
