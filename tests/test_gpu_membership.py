"""K8 k8_membership_apply (csrc/hip/membership.hip, module pushcdn_gpu_ctl) on
the GPU against its serial model ref.membership_apply, at the smallest shapes
that can break it; then the engine's membership log on cuda:0 against the
immediate API on the CPU engine.

Every case starts from a sentinel-filled bitmap (random words) and non-zero
cursors, and compares the WHOLE bitmap and EVERY cursor with the model, so a
stray write anywhere shows."""

import pytest
import torch

from pushcdn_amd.ops import reference as ref
from tests.test_membership_cpu import (assert_same_as_immediate, make_engine, pack_row,
                                       random_state)

pytestmark = pytest.mark.gpu

ALL = list(range(256))
EDGE_TOPICS = [0, 63, 64, 127, 128, 255]     # both ends of each wave's word


@pytest.fixture(scope="module")
def ctl():
    from pushcdn_amd.ops import get_gpu_ctl_ops

    return get_gpu_ctl_ops()


def check(ctl, R, W, rows, seed=1):
    """Apply `rows` on the device and through the model; compare everything.
    Returns the bitmap before and after; the cursors before and after are
    left in check.cursors_before / check.cursors_after."""
    bitmap, wpos = random_state(R, W, seed)
    recs = torch.tensor([pack_row(*row) for row in rows],
                        dtype=torch.int64).reshape(len(rows), 10)
    d_bitmap, d_wpos = bitmap.cuda(), wpos.cuda()
    ctl.membership_apply(d_bitmap, d_wpos, recs.cuda())
    torch.cuda.synchronize()
    before = bitmap.clone()
    check.cursors_before = wpos.clone()
    ref.membership_apply(bitmap, wpos, recs)
    assert torch.equal(d_bitmap.cpu(), bitmap)
    assert torch.equal(d_wpos.cpu(), wpos)
    check.cursors_after = d_wpos.cpu()
    return before, bitmap


def test_three_recipients_one_word(ctl):
    before, after = check(ctl, 3, 1, [
        (0, True, [1, 2, 3], [3, 4]),
        (2, False, ALL, []),
        (1, True, [], EDGE_TOPICS),
    ])
    assert not torch.equal(before, after)


def test_peer_slots_word_boundary_and_the_four_wave_split(ctl):
    # R = 70: users 0..65, peer slots 66..69; slot 63 is the sign bit of word
    # 0, slot 64 the first bit of word 1
    R, W = 70, 2
    rows = [
        (0, True, [], EDGE_TOPICS),
        (63, False, EDGE_TOPICS, [63, 64]),
        (64, True, ALL, [127, 128]),
        (69, False, [0, 255], [1, 254]),
        (66, True, EDGE_TOPICS, []),
    ]
    before, after = check(ctl, R, W, rows)
    assert not torch.equal(before, after)


def test_64_rows_contend_for_the_words_of_one_column(ctl):
    # every recipient of word 0, overlapping topics: 64 blocks hit the same
    # 64-bit word of each topic with atomics
    rows = [(r, r % 3 == 0, [t for t in range(0, 256, 1 + r % 5)],
             [t for t in range(r % 7, 256, 7)]) for r in range(64)]
    check(ctl, 70, 2, rows)
    check(ctl, 64, 1, list(reversed(rows)), seed=2)


def test_clear_all_with_a_few_set(ctl):
    before, after = check(ctl, 70, 2, [(65, True, ALL, [0, 64, 200])])
    col = after[:, 1].tolist()
    assert [t for t in range(256) if col[t] >> 1 & 1] == [0, 64, 200]


def test_out_of_range_rows_are_skipped(ctl):
    R = 70
    rows = [(-1, True, ALL, ALL), (R, True, ALL, ALL), (R + 57, True, ALL, []),
            (1 << 40, True, ALL, ALL), (-(1 << 62), True, [], ALL), (5, False, [5], [6])]
    before, after = check(ctl, R, 2, rows)
    # only recipient 5's two bits may differ
    diff = (before ^ after)
    assert int((diff != 0).sum()) <= 2 and int((diff[:, 1] != 0).sum()) == 0
    # nothing but skipped rows: nothing changes at all
    before, after = check(ctl, R, 2, rows[:-1], seed=3)
    assert torch.equal(before, after)


def test_reset_flags_on_some_rows_only(ctl):
    R, W = 70, 2
    rows = [(r, r % 2 == 1, [r], [r + 1]) for r in range(0, 70, 3)]
    check(ctl, R, W, rows)
    was, got = check.cursors_before, check.cursors_after
    reset = {r for r, flag, _c, _s in rows if flag}
    assert 0 < len(reset) < len(rows) and int(was.min()) > 0
    assert all(int(got[r]) == (0 if r in reset else int(was[r])) for r in range(R))


def test_more_rows_than_the_grid_cap(ctl):
    # n = cap + 6 rows on R = cap + 8 recipients: the grid-stride loop takes
    # the rows beyond the cap, the last word of the bitmap is partial
    cap = ctl._K8_MAX_BLOCKS
    n, R = cap + 6, cap + 8
    W = (R + 63) // 64
    rows = [(r, r % 4 == 0, [(r * 7) & 0xFF, (r + 1) & 0xFF, 255 - (r & 0xFF)],
             [(r * 3) & 0xFF, (r >> 3) & 0xFF]) for r in range(n)]
    before, after = check(ctl, R, W, rows)
    assert not torch.equal(before[:, W - 1], after[:, W - 1])    # rows past the cap ran


def test_no_rows_no_launch(ctl):
    before, after = check(ctl, 3, 1, [])
    assert torch.equal(before, after)


def test_engine_log_on_the_gpu_equals_the_immediate_api_on_the_cpu():
    eng = make_engine(device="cuda:0", pair_capacity=1 << 10)
    assert_same_as_immediate(eng)
    assert eng._ctl_ops is not None      # the flushes went through K8
