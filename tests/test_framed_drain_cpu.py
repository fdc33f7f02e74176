"""The framed drain without a GPU: the model (ops.reference.frame_rings)
against frames built from parse_ring_records on every hand-built case,
parse_frames, the CPU engine's drain_framed against a twin engine's
drain_compact, and the native pump's send_framed_batch over loopback
sockets."""

import socket
import time

import pytest
import torch

from tests import framed_drain_cases as fc
from pushcdn_amd.ops import reference as ref
from pushcdn_amd.ops.ring_format import FRAME_SORT_MAX, parse_frames

CASES = {c.name: c for c in fc.all_cases()}


@pytest.mark.parametrize("name", CASES)
def test_model_matches_parse_ring_records(name):
    case = CASES[name]
    egress, wpos, dst_off, staging, frame_len, frame_cnt = fc.build_inputs(case)
    before = wpos.clone()
    ref.frame_rings(egress, case.ring_bytes, wpos, dst_off, staging, frame_len, frame_cnt)
    fc.check_outputs(case, dst_off, staging, frame_len, frame_cnt)
    assert torch.equal(wpos, before)


def test_the_cases_cover_what_they_claim():
    align = CASES["alignment"]
    starts = set()
    for ring in align.rings:
        off = 0
        for f in fc.expected_frames(ring, align.ring_bytes):
            starts.add((off + 4) % 16)
            off += 4 + len(f)
    assert starts == set(range(16))        # every body alignment mod 16
    cap = CASES["cap"].rings
    assert [len(fc.expected_frames(r, 1 << 30)) for r in cap] \
        == [FRAME_SORT_MAX, FRAME_SORT_MAX + 1, FRAME_SORT_MAX + 1]
    assert [r.raw for r in cap] == [False, True, False]
    many = CASES["many"].rings
    assert len(many) == 70 and many[0].wpos == 0 and many[-1].wpos == 0


def test_parse_frames_is_strict():
    frames = [b"", b"a", b"hello world", b"\x00" * 300]
    buf = b"".join(len(f).to_bytes(4, "big") + f for f in frames)
    assert parse_frames(buf) == frames
    assert parse_frames(b"") == []
    assert parse_frames(memoryview(buf)) == frames
    for bad in (buf[:-1], buf + b"\x00", buf + b"\x00\x00\x00", buf + b"\x00\x00\x00\x05abcd",
                b"\xff\xff\xff\xff"):
        with pytest.raises(ValueError):
            parse_frames(bad)


def test_engine_reexports():
    from pushcdn_amd.broker import gpu_engine

    assert gpu_engine.parse_frames is parse_frames
    assert gpu_engine.FRAME_SORT_MAX == FRAME_SORT_MAX >= 4096


# ------------------------------- CPU engine -------------------------------

@pytest.mark.parametrize("kw", [
    {}, {"join": True}, {"burst": True},
    {"loss_accounting": True, "ring_bytes": 1024},
    {"loss_accounting": True, "ring_bytes": 1024, "join": True},
], ids=["plain", "join", "burst", "lossy", "lossy-join"])
def test_cpu_engine_drain_framed_equals_drain_compact(kw):
    eng, wpos, per, losses = fc.run_scenario("cpu", True, **kw)
    _twin, wpos2, per2, losses2 = fc.run_scenario("cpu", False, **kw)
    assert wpos == wpos2
    assert per == per2
    assert losses == losses2
    if kw.get("loss_accounting"):
        assert losses                       # the small rings did overflow
    # a user with Directs and Broadcasts in one tick, peers, and a non-subscriber
    assert len(per[2]) >= 9 and per[fc.NU] and per[fc.NU + 1] and not per[5]
    if kw.get("burst"):
        assert len(per[1]) >= 40
    # cursors are zero and a second drain is empty
    assert int(eng.ring_wpos.sum()) == 0
    w, offsets, frame_len, frame_cnt, staging = eng.drain_framed()
    assert int(w.sum()) == 0 and int(frame_len.sum()) == 0 and int(frame_cnt.sum()) == 0
    assert staging.numel() == 0 and offsets.tolist() == [0] * (fc.NU + fc.NP + 1)


def test_drain_framed_refuses_by_reference_engines():
    eng = fc.make_engine("cpu", ref_threshold=512)
    with pytest.raises(ValueError, match="by-reference"):
        eng.drain_framed()


# --------------------------------- the pump ---------------------------------

def _tcp_pair():
    srv = socket.socket()
    srv.bind(("127.0.0.1", 0))
    srv.listen(1)
    a = socket.create_connection(srv.getsockname())
    b, _ = srv.accept()
    srv.close()
    return a, b


def _recv_frames(pump, cid, n, timeout=10.0):
    got, deadline = [], time.monotonic() + timeout
    while len(got) < n and time.monotonic() < deadline:
        frames, closed = pump.recv_batch(cid, 1 << 16)
        got.extend(frames)
        if closed:
            break
        if len(got) < n:
            time.sleep(0.002)
    return got


def _framed(frames):
    return b"".join(len(f).to_bytes(4, "big") + f for f in frames)


@pytest.fixture()
def pump_pair():
    from pushcdn_amd.ops.build import build_core

    pump = build_core().Pump()
    a, b = _tcp_pair()
    tx, rx = pump.add(a.detach()), pump.add(b.detach())
    yield pump, tx, rx
    pump.stop()


def test_pump_sends_frames_verbatim(pump_pair):
    pump, tx, rx = pump_pair
    frames = [b"one", b"", fc.body(3, 70_000), b"four"]
    lead = b"\x77" * 13
    buf = lead + _framed(frames) + b"\x77" * 5
    flat = pump.send_framed_batch(buf, [tx], [len(lead)], [len(_framed(frames))], [len(frames)])
    assert list(flat) == [4, sum(len(f) for f in frames)]
    assert _recv_frames(pump, rx, 4) == frames
    # an empty range is fine and sends nothing
    assert list(pump.send_framed_batch(buf, [tx], [0], [0], [0])) == [0, 0]


def test_pump_reports_a_closed_connection(pump_pair):
    pump, tx, _rx = pump_pair
    buf = _framed([b"x"])
    pump.hard_close(tx)
    assert list(pump.send_framed_batch(buf, [tx, 12345], [0, 0], [len(buf)] * 2, [1, 1])) \
        == [-1, 0, -1, 0]


def test_pump_refuses_malformed_frames_and_sends_nothing(pump_pair):
    pump, tx, rx = pump_pair
    frames = [b"alpha", b"beta", b"gamma"]
    good = _framed(frames)
    corrupt = bytearray(good)
    corrupt[9 + 3] ^= 0x40                          # second prefix: a length past the end
    too_long = (0x7FFFFFFF).to_bytes(4, "big") + b"abc"
    for buf, cnt in (
        (bytes(corrupt), 3),
        (good, 2), (good, 4),                       # a wrong count
        (good[:-1], 3), (good + b"\x00\x00", 3),    # a trailing partial frame
        (good + b"\x00\x00\x00\x09abc", 4),
        (too_long, 1),
    ):
        assert list(pump.send_framed_batch(buf, [tx], [0], [len(buf)], [cnt])) == [-2, 0]
    # nothing of the above reached the peer: the next frame it sees is this one
    assert list(pump.send_framed_batch(good, [tx], [0], [len(good)], [3])) == [3, 14]
    assert _recv_frames(pump, rx, 3) == frames
    # a refused entry does not hold the others back
    flat = pump.send_framed_batch(good + good[:-1], [tx, tx], [0, len(good)],
                                  [len(good), len(good) - 1], [3, 3])
    assert list(flat) == [3, 14, -2, 0]
    assert _recv_frames(pump, rx, 3) == frames


def test_pump_checks_its_ranges(pump_pair):
    pump, tx, _rx = pump_pair
    buf = _framed([b"x"])
    for starts, lens, cnts in (([0], [len(buf) + 1], [1]), ([-1], [1], [1]),
                               ([len(buf) + 1], [0], [0]), ([0], [-1], [0]),
                               ([0], [len(buf)], [-2]), ([0, 0], [1], [1])):
        with pytest.raises(RuntimeError):
            pump.send_framed_batch(buf, [tx] * len(starts), starts, lens, cnts)


def test_pump_ring_mode_entry_delivers_what_send_rings_batch_delivers(pump_pair):
    pump, tx, rx = pump_pair
    ring = fc.order_rings()[5]                      # broadcasts then racing directs
    want = fc.expected_frames(ring, 1 << 20)
    a = pump.send_rings_batch(ring.data, [tx], [0], [ring.wpos])
    got_a = _recv_frames(pump, rx, len(want))
    b = pump.send_framed_batch(ring.data, [tx], [0], [ring.wpos], [-1])
    got_b = _recv_frames(pump, rx, len(want))
    assert list(a) == list(b) == [len(want), sum(len(f) for f in want)]
    assert got_a == got_b == want


def test_check_frames():
    from pushcdn_amd.ops.build import build_core

    check = build_core().Pump.check_frames
    good = _framed([b"", b"ab", b"c" * 1000])
    assert check(good, 3) and check(b"", 0)
    assert not check(good, 2) and not check(good, 4) and not check(good, -1)
    assert not check(good[:-1], 3) and not check(good + b"\x00", 3)
    assert not check(b"\x20\x00\x00\x00", 1)        # above the framing limit
