#!/usr/bin/env python3
"""What the engine's loss accounting costs: the same service-shaped tick on
two engines, one with loss_accounting off and one with it on.

The tick: `--users` users, user u on topic u % `--topics`; `--messages`
messages of non-uniform size (payloads of 32 .. `--max-payload` bytes), three
Broadcasts to one Direct; whole wire messages fanned out (fanout_wire), as
the broker service does.  A step is tick() + drain_compact(), timed from
before the tick to a device synchronise after the drain.  The rings are sized
so that nothing is lost: the accounting's regular cost is K9 per tick, and per
drain K10 plus a 4-byte count copy; the list is copied only on a loss.

The two engines alternate step by step inside one process; `--warmup`
untimed steps each, then `--reps` timed ones; median and min-max are
reported for each, and the difference of the medians.

Needs a GPU: there is no CPU fallback for a timing (--device cpu exists to
dry-run the script on the serial models).

  python scripts/bench_loss_accounting.py --out profiles/loss_accounting.json
"""

from __future__ import annotations

import argparse
import json
import random
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


def make_batch(args):
    rng = random.Random(7)
    batch, offsets = bytearray(), [0]
    for i in range(args.messages):
        payload = rng.randbytes(rng.randint(32, args.max_payload))
        if i % 4 == 3:
            msg = m.Direct(key_of(rng.randrange(args.users)), payload)
        else:
            msg = m.Broadcast([rng.randrange(args.topics)], payload)
        batch += m.serialize(msg)
        offsets.append(len(batch))
    return bytes(batch), offsets


def make_engine(args, accounting: bool) -> GpuBrokerEngine:
    table = 1 << (4 * args.users - 1).bit_length()
    eng = GpuBrokerEngine(device=args.device, n_users=args.users,
                          ring_bytes=args.ring_kb << 10, direct_table_size=table,
                          fanout_wire=True, pair_capacity=1 << 20,
                          loss_accounting=accounting)
    eng.subscribe_modulo(args.topics)
    eng.register_direct_bulk([(key_of(u), u) for u in range(args.users)])
    return eng


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=10_000)
    ap.add_argument("--messages", type=int, default=1_000)
    ap.add_argument("--topics", type=int, default=32)
    ap.add_argument("--max-payload", type=int, default=512)
    ap.add_argument("--ring-kb", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cuda = args.device.startswith("cuda")
    if cuda and not torch.cuda.is_available():
        sys.exit("bench_loss_accounting.py measures on the GPU; none found")

    def sync():
        if cuda:
            torch.cuda.synchronize()

    batch, offsets = make_batch(args)
    engines = {"off": make_engine(args, False), "on": make_engine(args, True)}
    times = {v: [] for v in engines}
    delivered = {}
    for rep in range(args.warmup + args.reps):
        for variant, eng in engines.items():     # alternate the variants
            buf, off = eng.ingest(batch, offsets)
            sync()
            t0 = time.perf_counter()
            eng.tick(buf, off, host_batch=batch, host_offsets=offsets)
            wpos, _offsets, _staging = eng.drain_compact()
            sync()
            dt = time.perf_counter() - t0
            delivered[variant] = int(wpos.sum())
            if rep >= args.warmup:
                times[variant].append(dt)
    # the same work on both, and nothing lost: the common path was measured
    assert delivered["off"] == delivered["on"] > 0, delivered
    assert engines["on"].take_losses() == {}, "a ring overflowed: raise --ring-kb"

    med = {v: statistics.median(ts) for v, ts in times.items()}
    result = dict(
        users=args.users, messages=args.messages, topics=args.topics,
        max_payload=args.max_payload, ring_kb=args.ring_kb, batch_bytes=len(batch),
        ring_bytes_delivered_per_step=delivered["on"],
        reps=args.reps, warmup=args.warmup, device=args.device,
        step_ms={v: dict(median=round(med[v] * 1e3, 4),
                         min=round(min(ts) * 1e3, 4), max=round(max(ts) * 1e3, 4))
                 for v, ts in times.items()},
        accounting_cost_ms=round((med["on"] - med["off"]) * 1e3, 4),
        accounting_cost_pct=round((med["on"] / med["off"] - 1) * 100, 2),
    )
    print(json.dumps(result), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
