"""The native boundary of the framed-drain extension
(csrc/gpu_drain_bindings.cpp, module pushcdn_gpu_drain) refuses a bad argument
by name.

As in test_gpu_ctl_binding_args.py: the op is called with CPU tensors only;
the bindings check dtype, stated shape, contiguity and length first and the
device LAST, so on a machine without a GPU a valid argument list gets as far
as "must be on a GPU" and a single bad argument is refused before that, with
a message that names the op and the argument.  On a machine WITH a GPU a
missing check would launch a kernel on host or short memory, so the whole
file is skipped there."""

import re

import pytest
import torch

from pushcdn_amd.ops import get_gpu_drain_ops

pytestmark = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="a missing check would launch a kernel on host memory; CPU-only machines only")

R, RING, TOTAL = 5, 256, 1024     # five rings of 256 B, 1 KiB of staging


def z(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype)


@pytest.fixture(scope="module")
def ops():
    return get_gpu_drain_ops()


def valid():
    return [z(torch.uint8, R * RING), RING, z(torch.int64, R), z(torch.int64, R),
            z(torch.uint8, TOTAL), z(torch.int64, R), z(torch.int32, R),
            z(torch.int32, TOTAL // 16, 4)]


TENSORS = {"egress": 0, "wpos": 2, "dst_off": 3, "staging": 4, "frame_len": 5,
           "frame_cnt": 6, "index": 7}


def _refusal(ops, args):
    with pytest.raises(RuntimeError) as exc:
        ops.frame_rings(*args)
    return str(exc.value).splitlines()[0]


def _names(msg, *names):
    return all(re.search(rf"(?<![A-Za-z0-9_]){re.escape(n)}(?![A-Za-z0-9_])", msg)
               for n in names)


def test_the_module_exports_one_op(ops):
    assert {n for n in dir(ops) if callable(getattr(ops, n)) and not n.startswith("_")} \
        == {"frame_rings"}
    assert ops.FRAME_SORT_MAX >= 4096 and ops.CHUNK_BYTES % 16 == 0


def test_the_data_plane_module_does_not_export_it():
    from pushcdn_amd.ops import get_gpu_ops

    assert not hasattr(get_gpu_ops(), "frame_rings")


def test_valid_arguments_reach_the_device_check(ops):
    msg = _refusal(ops, valid())
    assert msg.startswith("frame_rings: egress must be on a GPU, got cpu"), msg
    msg = _refusal(ops, valid() + [1])               # max_chunks, positional
    assert "must be on a GPU" in msg, msg


def test_no_rings_is_still_checked(ops):
    args = valid()
    for i in (2, 3, 5, 6):
        args[i] = args[i][:0]
    assert "egress must be on a GPU" in _refusal(ops, args)


def _narrow(t):
    return t.to(torch.int32) if t.dtype != torch.int32 else t.to(torch.int64)


BAD = {
    "egress": {
        "dtype": lambda t: t.to(torch.int8),
        "strided": lambda t: t.repeat(2)[::2],
        "two dimensions": lambda t: t.reshape(R, RING),
        "one ring short": lambda t: t[:-1],
    },
    "wpos": {
        "dtype": _narrow,
        "strided": lambda t: t.repeat(2)[::2],
        "two dimensions": lambda t: t.reshape(R, 1),
    },
    "dst_off": {
        "dtype": _narrow,
        "strided": lambda t: t.repeat(2)[::2],
        "one short": lambda t: t[:-1],
        "one more": lambda t: z(torch.int64, R + 1),
    },
    "staging": {
        "dtype": lambda t: t.to(torch.int8),
        "strided": lambda t: t.repeat(2)[::2],
        "two dimensions": lambda t: t.reshape(2, -1),
    },
    "frame_len": {
        "dtype": _narrow,
        "strided": lambda t: t.repeat(2)[::2],
        "one short": lambda t: t[:-1],
        "one more": lambda t: z(torch.int64, R + 1),
    },
    "frame_cnt": {
        "dtype": _narrow,
        "strided": lambda t: t.repeat(2)[::2],
        "one short": lambda t: t[:-1],
        "one more": lambda t: z(torch.int32, R + 1),
    },
    "index": {
        "dtype": _narrow,
        "strided": lambda t: t.repeat(1, 2)[:, ::2],
        "three columns": lambda t: z(torch.int32, TOTAL // 16, 3),
        "flat": lambda t: t.reshape(-1),
        "one entry short": lambda t: t[:-1],
    },
}


@pytest.mark.parametrize("arg", BAD)
def test_each_bad_tensor_is_refused_by_name(ops, arg):
    assert set(BAD) == set(TENSORS)
    for kind, mutate in BAD[arg].items():
        args = valid()
        bad = mutate(args[TENSORS[arg]])
        if kind == "strided":
            assert not bad.is_contiguous()
        args[TENSORS[arg]] = bad
        msg = _refusal(ops, args)
        assert _names(msg, "frame_rings", arg), f"{arg} {kind}: {msg}"
        assert "must be on a GPU" not in msg, f"{arg} {kind}: {msg}"


@pytest.mark.parametrize("ring_bytes", [-16, 8, 250, 1 << 31])
def test_a_bad_ring_size_is_refused(ops, ring_bytes):
    args = valid()
    args[1] = ring_bytes
    msg = _refusal(ops, args)
    assert _names(msg, "frame_rings") and "ring_bytes" in msg, msg
    assert "must be on a GPU" not in msg


def test_a_bad_chunk_count_is_refused(ops):
    msg = _refusal(ops, valid() + [65536])
    assert _names(msg, "frame_rings", "max_chunks"), msg
