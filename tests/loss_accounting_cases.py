"""Engine scenarios for the loss accounting, shared by
test_loss_accounting_cpu.py (CPU engine) and test_gpu_loss_accounting.py
(GPU engine against CPU engine).  Not a test module.

Every case builds an engine with n_users = 6, n_peer_slots = 2 and
1024-byte rings, sends messages whose ring record is exactly 256 bytes (four
fill a ring) and returns what take_losses() reported.  EXPECTED holds the
same figures from plain arithmetic: lost = demanded - min-prefix that fits."""

from pushcdn_amd.broker.gpu_engine import GpuBrokerEngine, ring_rec
from pushcdn_amd.proto import message as m

N_USERS, N_PEERS, RING = 6, 2, 1024
REC = 256
T = 5            # the topic users 1 and 2 take
PEER_T = 7       # the topic peer slot 0 takes
KEY = b"direct-user-key"        # owned by user 2
REMOTE = b"remote-user-key"     # owned by peer slot 1


def make_engine(device, **kw):
    kw.setdefault("loss_accounting", True)
    return GpuBrokerEngine(device=device, n_users=N_USERS, n_peer_slots=N_PEERS,
                           ring_bytes=RING, direct_table_size=64, fanout_wire=True,
                           hash_seed=0xACC7, **kw)


def sized(make, rec):
    """make(payload) with the shortest payload whose wire form takes a ring
    record of exactly `rec` bytes."""
    for n in range(rec + 1):
        msg = make(b"x" * n)
        if ring_rec(len(m.serialize(msg))) == rec:
            return msg
    raise AssertionError(f"no payload gives a {rec}-byte record")


def bcast(topic=T, rec=REC):
    return sized(lambda p: m.Broadcast([topic], p), rec)


def direct(key=KEY, rec=REC):
    return sized(lambda p: m.Direct(key, p), rec)


def tick(eng, msgs, origin=None):
    batch, offsets = b"", [0]
    for msg in msgs:
        batch += m.serialize(msg)
        offsets.append(len(batch))
    if origin is None:
        buf, off = eng.ingest(batch, offsets)
    else:
        buf, off, origin = eng.ingest(batch, offsets, origin=origin)
    eng.tick(buf, off, host_batch=batch, host_offsets=offsets, origin=origin)
    return offsets


DRAINS = ("drain_cursors", "drain_compact", "drain_compact_ref")


def drain(eng, how="drain_compact"):
    """Run one drain; returns its cursors as a list."""
    out = getattr(eng, how)()
    wpos = out if how == "drain_cursors" else out[0]
    return [int(x) for x in wpos]


# --- the cases: each returns (losses, cursors of the drain) ---

def five_broadcasts(device, how="drain_compact"):
    eng = make_engine(device)
    eng.subscribe(1, [T])
    tick(eng, [bcast()] * 5)
    wpos = drain(eng, how)
    return eng.take_losses(), wpos


def four_broadcasts_fill_the_ring(device, how="drain_compact"):
    eng = make_engine(device)
    eng.subscribe(1, [T])
    tick(eng, [bcast()] * 4)
    wpos = drain(eng, how)
    return eng.take_losses(), wpos


def directs_only(device):
    eng = make_engine(device)
    eng.register_direct(KEY, 2)
    tick(eng, [direct()] * 6)
    wpos = drain(eng)
    return eng.take_losses(), wpos


def peer_rings(device):
    """Slot 0 overflows by Broadcasts, slot 1 by Directs; a remote-origin
    Broadcast and a remote-origin Direct to a peer demand nothing there."""
    eng = make_engine(device)
    eng.set_peer_topics(0, [PEER_T])
    eng.register_direct(REMOTE, -(1 + 2))
    msgs = [bcast(PEER_T)] * 5 + [direct(REMOTE)] * 5 + [bcast(PEER_T), direct(REMOTE)]
    tick(eng, msgs, origin=[0] * 10 + [1, 1])
    wpos = drain(eng)
    return eng.take_losses(), wpos


def two_ticks_one_drain(device):
    eng = make_engine(device)
    eng.subscribe(1, [T])
    tick(eng, [bcast()] * 3)
    tick(eng, [bcast()] * 3)
    wpos = drain(eng)
    return eng.take_losses(), wpos


BIG_REC = 2048   # a record twice the ring


def larger_than_the_ring(device):
    eng = make_engine(device)
    eng.subscribe(1, [T])
    tick(eng, [bcast(rec=BIG_REC)])
    wpos = drain(eng)
    return eng.take_losses(), wpos


def larger_than_the_ring_by_reference(device):
    eng = make_engine(device, ref_threshold=1000)
    eng.subscribe(1, [T])
    tick(eng, [bcast(rec=BIG_REC)])
    wpos = drain(eng, "drain_compact_ref")
    return eng.take_losses(), wpos


def slot_reclaimed_before_the_drain(device):
    """Users 1 and 2 both overflow; user 1 leaves and a new user joins the
    slot before any drain.  Only user 2 reports."""
    eng = make_engine(device)
    eng.subscribe(1, [T])
    eng.subscribe(2, [T])
    tick(eng, [bcast()] * 5)
    eng.queue_leave(1, None)
    eng.queue_join(1, b"the-new-occupant", [T])
    wpos = drain(eng)
    return eng.take_losses(), wpos


def peer_cleared_before_the_drain(device):
    eng = make_engine(device)
    eng.set_peer_topics(0, [PEER_T])
    eng.subscribe(2, [PEER_T])
    tick(eng, [bcast(PEER_T)] * 5, origin=[0] * 5)
    eng.clear_peer(0)
    wpos = drain(eng)
    return eng.take_losses(), wpos


def _wpos(**used):
    w = [0] * (N_USERS + N_PEERS)
    for r, n in used.items():
        w[int(r[1:])] = n
    return w


# case -> (losses, cursors), by arithmetic: a ring takes RING // REC = 4
# records of REC bytes; everything demanded beyond that is lost
EXPECTED = {
    five_broadcasts: ({1: 5 * REC - RING}, _wpos(r1=RING)),
    four_broadcasts_fill_the_ring: ({}, _wpos(r1=RING)),
    directs_only: ({2: 6 * REC - RING}, _wpos(r2=RING)),
    peer_rings: ({N_USERS: 5 * REC - RING, N_USERS + 1: 5 * REC - RING},
                 _wpos(r6=RING, r7=RING)),
    two_ticks_one_drain: ({1: 6 * REC - RING}, _wpos(r1=RING)),
    larger_than_the_ring: ({1: BIG_REC}, _wpos()),
    larger_than_the_ring_by_reference: ({}, _wpos(r1=16)),
    slot_reclaimed_before_the_drain: ({2: 5 * REC - RING}, _wpos(r2=RING)),
    peer_cleared_before_the_drain: ({2: 5 * REC - RING}, _wpos(r2=RING)),
}
