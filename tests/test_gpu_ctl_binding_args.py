"""The native boundary of the maintenance extension (csrc/gpu_ctl_bindings.cpp,
module pushcdn_gpu_ctl) refuses a bad argument by name.

As in test_gpu_binding_args.py: every op is called with CPU tensors only; the
bindings check dtype, stated shape, contiguity and length first and the
device LAST, so on a machine without a GPU a valid argument list gets as far
as "must be on a GPU" and a single bad argument is refused before that, with
a message that names the op and the argument.  On a machine WITH a GPU a
missing check would launch a kernel on host or short memory, so the whole
file is skipped there."""

import re

import pytest
import torch

from pushcdn_amd.ops import get_gpu_ctl_ops

pytestmark = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="a missing check would launch a kernel on host memory; CPU-only machines only")

W, R, N = 2, 70, 3     # 70 recipients in a two-word bitmap, three rows


def i64(*shape):
    return torch.zeros(*shape, dtype=torch.int64)


@pytest.fixture(scope="module")
def ops():
    return get_gpu_ctl_ops()


# op -> (valid argument list, {tensor argument: position}, first tensor first)
ROWS = {
    "membership_apply": (lambda: [i64(256, W), i64(R), i64(N, 10)],
                         {"sub_bitmap": 0, "ring_wpos": 1, "recs": 2}),
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


def test_the_data_plane_module_does_not_export_it():
    from pushcdn_amd.ops import get_gpu_ops

    assert not hasattr(get_gpu_ops(), "membership_apply")


@pytest.mark.parametrize("op", ROWS)
def test_valid_arguments_reach_the_device_check(ops, op):
    build, tensors = ROWS[op]
    msg = _refusal(ops, op, build())
    assert msg.startswith(f"{op}: {next(iter(tensors))} must be on a GPU, got cpu"), msg


def test_an_empty_batch_is_still_checked(ops):
    args = ROWS["membership_apply"][0]()
    args[2] = i64(0, 10)
    msg = _refusal(ops, "membership_apply", args)
    assert msg.startswith("membership_apply: sub_bitmap must be on a GPU"), msg


BAD = {
    "sub_bitmap": {
        "dtype": lambda t: t.to(torch.int32),
        "strided": lambda t: t.repeat(1, 2)[:, ::2],
        "rows": lambda t: i64(255, W),
        "one dimension": lambda t: i64(256 * W),
        "too few words for the cursors": lambda t: i64(256, 1),     # 64 bits < R = 70
    },
    "ring_wpos": {
        "dtype": lambda t: t.to(torch.int32),
        "strided": lambda t: t.repeat(2)[::2],
        "two dimensions": lambda t: i64(R, 1),
        "more cursors than bits": lambda t: i64(W * 64 + 1),
    },
    "recs": {
        "dtype": lambda t: t.to(torch.int32),
        "strided": lambda t: t.repeat(1, 2)[:, ::2],
        "nine words": lambda t: i64(N, 9),
        "eleven words": lambda t: i64(N, 11),
        "flat": lambda t: i64(N * 10),
    },
}


@pytest.mark.parametrize("arg", BAD)
def test_each_bad_tensor_is_refused_by_name(ops, arg):
    build, tensors = ROWS["membership_apply"]
    assert set(BAD) == set(tensors)
    for kind, mutate in BAD[arg].items():
        args = build()
        bad = mutate(args[tensors[arg]])
        if kind == "strided":
            assert not bad.is_contiguous()
        args[tensors[arg]] = bad
        msg = _refusal(ops, "membership_apply", args)
        # the bitmap's width is refused where the cursor count meets it
        named = "ring_wpos" if kind == "too few words for the cursors" else arg
        assert _names(msg, "membership_apply", named), f"{arg} {kind}: {msg}"
        assert "must be on a GPU" not in msg, f"{arg} {kind}: {msg}"


def test_the_largest_cursor_count_passes(ops):
    args = ROWS["membership_apply"][0]()
    args[1] = i64(W * 64)
    msg = _refusal(ops, "membership_apply", args)
    assert "must be on a GPU" in msg, msg
