#!/usr/bin/env python3
"""What by-reference delivery saves: engine tick + drain of Broadcasts to
every subscriber, with ref_threshold unset (every delivery copied into the
rings: the behaviour without the feature) and set to the message size (every
delivery a 16-byte record).

Per payload size and variant it prints one JSON line:
  tick_ms / drain_ms   median host clock around work that ends in a device
                       synchronise (the drain ends in its own D2H)
  d2h_bytes            bytes the drain copies to the host (sum of cursors)
  hbm_written_bytes    ring bytes stored by the fan-out plus the compacted
                       copy K7 stores, computed from the cursors
The two variants alternate inside one process so both see the same machine
state; every shape is warmed up before its timed window.  Needs a GPU: there
is no CPU fallback for a timing.

  python scripts/bench_byref.py --users 1000 --sizes 65536 --out result.json
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from pushcdn_amd.broker.gpu_engine import GpuBrokerEngine  # noqa: E402
from pushcdn_amd.proto import message as m  # noqa: E402


def make_batch(size: int, n_msgs: int):
    buf, offsets = b"", [0]
    for i in range(n_msgs):
        buf += m.serialize(m.Broadcast([1], bytes([i & 0xFF]) * size))
        offsets.append(len(buf))
    return buf, offsets


def one_tick(eng, dbuf, doff, batch, offsets):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.tick(dbuf, doff, host_batch=batch, host_offsets=offsets)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if eng.ref_threshold is None:
        wpos, _off, staging = eng.drain_compact()
        refbuf = b""
    else:
        wpos, _off, staging, refbuf = eng.drain_compact_ref()
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, int(wpos.sum()), staging.numel(), len(refbuf)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1000)
    ap.add_argument("--msgs", type=int, default=8, help="Broadcasts per tick")
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536],
                    help="payload sizes; the threshold of the 'on' variant is the wire size")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inline-variant", action="store_true",
                    help="also time a threshold just above the message size")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_byref.py measures on the GPU; none found")

    results = []
    for size in args.sizes:
        batch, offsets = make_batch(size, args.msgs)
        wire = offsets[1]
        ring_bytes = 1 << max(12, (args.msgs * (wire + 32)).bit_length())
        engines = {}
        variants = [("off", None), ("on", wire)]
        if args.inline_variant:
            # threshold set but above every message: all records inline,
            # through the by-reference kernel — the cost of turning it on
            variants.append(("inline", wire + 8))
        for name, thr in variants:
            eng = GpuBrokerEngine(device="cuda:0", n_users=args.users, ring_bytes=ring_bytes,
                                  fanout_wire=True, direct_enabled=False,
                                  pair_capacity=max(1 << 16, 2 * args.users * args.msgs),
                                  ref_threshold=thr)
            eng.subscribe_all([1])
            engines[name] = (eng,) + tuple(eng.ingest(batch, offsets))
        torch.cuda.synchronize()
        times = {name: ([], []) for name in engines}
        counts = {}
        for rep in range(args.warmup + args.reps):
            for name, (eng, dbuf, doff) in engines.items():   # alternate the variants
                tick_s, drain_s, ring_used, d2h, reflen = one_tick(eng, dbuf, doff, batch,
                                                                   offsets)
                if rep >= args.warmup:
                    times[name][0].append(tick_s)
                    times[name][1].append(drain_s)
                counts[name] = (ring_used, d2h, reflen)
        for name in engines:
            ring_used, d2h, reflen = counts[name]
            drops = int(engines[name][0]._drops.cpu()[0])
            row = dict(
                variant=name, users=args.users, msgs_per_tick=args.msgs, payload=size,
                wire_len=wire, ring_bytes=ring_bytes,
                ref_threshold=engines[name][0].ref_threshold,
                tick_ms=round(statistics.median(times[name][0]) * 1e3, 4),
                drain_ms=round(statistics.median(times[name][1]) * 1e3, 4),
                tick_ms_min=round(min(times[name][0]) * 1e3, 4),
                tick_ms_max=round(max(times[name][0]) * 1e3, 4),
                drain_ms_min=round(min(times[name][1]) * 1e3, 4),
                drain_ms_max=round(max(times[name][1]) * 1e3, 4),
                d2h_bytes=d2h, hbm_written_bytes=2 * ring_used, refbuf_bytes=reflen,
                deliveries=args.users * args.msgs, drops=drops, reps=args.reps,
            )
            results.append(row)
            print(json.dumps(row), flush=True)
        del engines
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
