#!/usr/bin/env python3
"""What the framed drain buys between the ring and the socket: the same
service-shaped tick drained two ways on twin engines,

  ring:    drain_compact  (K7)  + Pump.send_rings_batch   (parse, sort, re-copy)
  framed:  drain_framed   (K11) + Pump.send_framed_batch  (check, one copy)

Two shapes: "mixed" is bench_loss_accounting.py's (`--users` users, user u on
topic u % `--topics`, `--messages` messages of 32 .. `--max-payload` payload
bytes, three Broadcasts to one Direct) and "bcast1k" is Broadcasts only with
1 KiB payloads.  Whole wire messages are fanned out, as the broker does.

Three figures per variant, each a median with min-max over `--reps` steps,
the variants alternating step by step in one process:

  device_ms    the drain kernel(s) alone, between two stream events, on the
               rings the step's tick left (K7 against K11's two launches)
  drain_ms     wall time of the engine call, cursor readback to staging in
               host memory
  dispatch_ms  wall time of the pump call on one thread, for every recipient

Recipients share `--conns` loopback connections of one pump; a second pump
holds the peer ends and discards what arrives, outside the timed regions.

Needs a GPU (--device cpu dry-runs the script on the serial models and
reports no device times).

  python scripts/bench_framed_drain.py --out profiles/framed_drain.json
"""

from __future__ import annotations

import argparse
import json
import random
import socket
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from pushcdn_amd.broker.gpu_engine import GpuBrokerEngine  # noqa: E402
from pushcdn_amd.proto import message as m  # noqa: E402


def key_of(u: int) -> bytes:
    return b"bench-user-%08d" % u


def make_batch(args, shape: str):
    rng = random.Random(7)
    batch, offsets = bytearray(), [0]
    for i in range(args.messages):
        if shape == "bcast1k":
            msg = m.Broadcast([rng.randrange(args.topics)], rng.randbytes(1024))
        elif i % 4 == 3:
            msg = m.Direct(key_of(rng.randrange(args.users)),
                           rng.randbytes(rng.randint(32, args.max_payload)))
        else:
            msg = m.Broadcast([rng.randrange(args.topics)],
                              rng.randbytes(rng.randint(32, args.max_payload)))
        batch += m.serialize(msg)
        offsets.append(len(batch))
    return bytes(batch), offsets


def make_engine(args) -> GpuBrokerEngine:
    table = 1 << (4 * args.users - 1).bit_length()
    eng = GpuBrokerEngine(device=args.device, n_users=args.users,
                          ring_bytes=args.ring_kb << 10, direct_table_size=table,
                          fanout_wire=True, pair_capacity=1 << 20)
    eng.subscribe_modulo(args.topics)
    eng.register_direct_bulk([(key_of(u), u) for u in range(args.users)])
    return eng


def device_ms(eng, framed: bool, reps: int = 5):
    """The drain kernels alone on the engine's current rings (cursors are
    only read): median milliseconds between two events."""
    wpos = eng.ring_wpos.to("cpu")
    total = int(wpos.sum())
    dst_off = (torch.cumsum(wpos, 0) - wpos).to(eng.device)
    if eng._staging_dev is None or eng._staging_dev.numel() < total:
        return None      # the first drain sizes the staging; measured from the next step
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        if framed:
            eng._frame_rings(eng.ring_wpos, dst_off, int(wpos.max()))
        else:
            chunks = (int(wpos.max()) + (64 << 10) - 1) // (64 << 10)
            eng._ops.compact_rings(eng.egress, eng.ring_bytes, eng.ring_wpos, dst_off,
                                   eng._staging_dev, chunks)
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    return statistics.median(out)


def run_shape(args, shape: str, pump_tx, pump_rx, tx_ids, rx_ids, cuda: bool):
    batch, offsets = make_batch(args, shape)
    engines = {"ring": make_engine(args), "framed": make_engine(args)}
    ids = [tx_ids[u % len(tx_ids)] for u in range(args.users)]
    times = {v: dict(device_ms=[], drain_ms=[], dispatch_ms=[]) for v in engines}
    sent = {}
    reps = args.reps if shape == "mixed" else max(3, args.reps // 3)
    for rep in range(args.warmup + reps):
        for variant, eng in engines.items():     # alternate the variants
            framed = variant == "framed"
            buf, off = eng.ingest(batch, offsets)
            eng.tick(buf, off, host_batch=batch, host_offsets=offsets)
            dev = device_ms(eng, framed) if cuda else None
            if cuda:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            if framed:
                wpos, offs, frame_len, frame_cnt, staging = eng.drain_framed()
            else:
                wpos, offs, staging = eng.drain_compact()
            t1 = time.perf_counter()
            view = staging.numpy()
            starts = offs[:-1].tolist()
            if framed:
                lens, cnts = frame_len.tolist(), frame_cnt.tolist()
                t2 = time.perf_counter()
                flat = pump_tx.send_framed_batch(view, ids, starts, lens, cnts)
            else:
                ends = offs[1:].tolist()
                t2 = time.perf_counter()
                flat = pump_tx.send_rings_batch(view, ids, starts, ends)
            t3 = time.perf_counter()
            counts, payload = flat[0::2], flat[1::2]
            assert min(counts) >= 0, "a pump connection went away or a range was refused"
            sent[variant] = (sum(counts), sum(payload), int(wpos.sum()))
            # the peers discard; wait until everything went through, so the
            # next step's staging flip finds its buffer free
            want, got = sum(payload) + 4 * sum(counts), 0
            deadline = time.monotonic() + 120
            while got < want and time.monotonic() < deadline:
                for rx in rx_ids:
                    n, nbytes, _last, _closed = pump_rx.recv_drain(rx)
                    got += nbytes + 4 * n
                if got < want:
                    time.sleep(0.001)
            assert got == want, (got, want)
            if rep >= args.warmup:
                t = times[variant]
                if dev is not None:
                    t["device_ms"].append(dev)
                t["drain_ms"].append((t1 - t0) * 1e3)
                t["dispatch_ms"].append((t3 - t2) * 1e3)
    assert sent["ring"] == sent["framed"] and sent["ring"][0] > 0, sent

    def summary(xs):
        if not xs:
            return None
        return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4),
                    max=round(max(xs), 4))

    records, payload_bytes, ring_bytes_used = sent["ring"]
    return dict(
        shape=shape, users=args.users, messages=args.messages, topics=args.topics,
        batch_bytes=len(batch), reps=reps, warmup=args.warmup,
        records_per_step=records, payload_bytes_per_step=payload_bytes,
        ring_bytes_per_step=ring_bytes_used,
        **{v: {k: summary(xs) for k, xs in t.items()} for v, t in times.items()})


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=10_000)
    ap.add_argument("--messages", type=int, default=1_000)
    ap.add_argument("--topics", type=int, default=32)
    ap.add_argument("--max-payload", type=int, default=512)
    ap.add_argument("--ring-kb", type=int, default=64)
    ap.add_argument("--conns", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--shapes", default="mixed,bcast1k")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cuda = args.device.startswith("cuda")
    if cuda and not torch.cuda.is_available():
        sys.exit("bench_framed_drain.py measures on the GPU; none found")

    from pushcdn_amd.ops.build import build_core

    core = build_core()
    pump_tx, pump_rx = core.Pump(), core.Pump()
    tx_ids, rx_ids = [], []
    for _ in range(args.conns):
        a, b = socket.socketpair()
        tx_ids.append(pump_tx.add(a.detach()))
        rx_ids.append(pump_rx.add(b.detach()))
    try:
        shapes = [run_shape(args, s, pump_tx, pump_rx, tx_ids, rx_ids, cuda)
                  for s in args.shapes.split(",")]
    finally:
        pump_tx.stop()
        pump_rx.stop()
    result = dict(bench="framed_drain", device=args.device, ring_kb=args.ring_kb,
                  conns=args.conns, shapes=shapes)
    print(json.dumps(result), flush=True)
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        # the file also holds the default-path A/B (bench.py on the parent
        # commit and on this one): keep whatever else is in it
        merged = json.loads(out.read_text()) if out.exists() else {}
        merged["feature"] = result
        out.write_text(json.dumps(merged, indent=1) + "\n")


if __name__ == "__main__":
    main()
