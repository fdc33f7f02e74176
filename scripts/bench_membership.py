#!/usr/bin/env python3
"""What the engine's membership log saves: user joins, leaves and
subscription toggles applied through the immediate API (subscribe /
register_direct / unregister_direct / unsubscribe: the behaviour without
gpu_batched_membership) and through queue_* + flush_membership() (one K8
launch + one K6 launch per batch).

One engine per resident population P, 8 topics per user.  A cycle is
  join storm    n new users take n spare slots,
  toggle storm  each of those n users subscribes, then unsubscribes one topic,
  leave storm   the n users depart,
so the population is P again after every cycle and both variants see the same
state.  Every storm is timed from its first host call to a device
synchronise after its last.  The two variants alternate inside one process;
1 warm-up cycle, then `--reps` timed ones; median and min-max are reported
per storm and per change.

The immediate join and leave cost O(P) host work EACH (a DirectMap rebuild),
so only the first `--immediate-cap` changes of such a storm go through the
immediate API and are timed; the rest of the storm is applied through the
log, untimed, to reach the same state.  `changes_timed` says how many were
timed; `us_per_change` divides by that number.

direct_table_size is 4 * P, or the next power of two at or above
4 * (P + max n) where P + max n would pass half of that (the table's
half-full compaction rule would otherwise add rebuilds that neither path
asks for).

Needs a GPU: there is no CPU fallback for a timing (--device cpu exists to
dry-run the script on the serial models).

  python scripts/bench_membership.py --out profiles/membership_churn.json
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

TOPICS_PER_USER = 8


def topics_of(u: int):
    return [(u * 7 + i * 31) & 0xFF for i in range(TOPICS_PER_USER)]


def key_of(u: int) -> bytes:
    return b"bench-user-%08d" % u


class Bench:
    def __init__(self, device: str, P: int, n_max: int):
        S = 4 * P
        if P + n_max > S // 2:
            S = 1 << (4 * (P + n_max) - 1).bit_length()
        self.P, self.S = P, S
        self.cuda = device.startswith("cuda")
        self.eng = GpuBrokerEngine(device=device, n_users=P + n_max, ring_bytes=1 << 10,
                                   direct_table_size=S, fanout_wire=True,
                                   pair_capacity=1 << 16)
        for u in range(P):
            self.eng.queue_join(u, key_of(u), topics_of(u))
        self.eng.flush_membership()
        self.sync()
        # DirectMap rebuilds (O(P) host work), counted per storm
        self.rebuilds = 0
        real = self.eng.directs.rebuild

        def counted():
            self.rebuilds += 1
            real()
        self.eng.directs.rebuild = counted

    def sync(self):
        if self.cuda:
            torch.cuda.synchronize()

    def storm(self, kind: str, n: int, batched: bool, cap: int) -> tuple:
        """One storm over users P .. P+n-1.  Returns (seconds, changes timed,
        DirectMap rebuilds inside the timed part)."""
        eng, P = self.eng, self.P
        users = range(P, P + n)
        timed = n if batched or kind == "toggle" else min(n, cap)
        self.sync()
        rebuilds0 = self.rebuilds
        t0 = time.perf_counter()
        if batched:
            if kind == "join":
                for u in users:
                    eng.queue_join(u, key_of(u), topics_of(u))
            elif kind == "leave":
                for u in users:
                    eng.queue_leave(u, key_of(u))
            else:
                for u in users:
                    eng.queue_subscribe(u, [255])
                    eng.queue_unsubscribe(u, [255])
            eng.flush_membership()
        else:
            for u in list(users)[:timed]:
                if kind == "join":
                    eng.subscribe(u, topics_of(u))
                    eng.register_direct(key_of(u), u)
                elif kind == "leave":
                    eng.unregister_direct(key_of(u))
                    eng.unsubscribe(u, list(range(256)))
                else:
                    eng.subscribe(u, [255])
                    eng.unsubscribe(u, [255])
        self.sync()
        dt = time.perf_counter() - t0
        rebuilds = self.rebuilds - rebuilds0
        # the untimed rest of a capped immediate join / leave storm
        for u in list(users)[timed:]:
            if kind == "join":
                eng.queue_join(u, key_of(u), topics_of(u))
            elif kind == "leave":
                eng.queue_leave(u, key_of(u))
        eng.flush_membership()
        self.sync()
        return dt, timed, rebuilds

    def check(self, n_live: int) -> None:
        """The state both variants must leave: n_live registered users."""
        assert len(self.eng.directs.entries) == n_live, (len(self.eng.directs.entries), n_live)
        assert self.eng.pending_membership == 0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--populations", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--storms", type=int, nargs="+", default=[1, 64, 4096])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--immediate-cap", type=int, default=16,
                    help="changes of an immediate join/leave storm that are timed")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.device.startswith("cuda") and not torch.cuda.is_available():
        sys.exit("bench_membership.py measures on the GPU; none found")

    results = []
    for P in args.populations:
        bench = Bench(args.device, P, max(args.storms))
        for n in args.storms:
            times = {(v, k): [] for v in ("immediate", "batched")
                     for k in ("join", "toggle", "leave")}
            timed, rebuilds = {}, {}
            for rep in range(args.warmup + args.reps):
                for variant in ("immediate", "batched"):   # alternate the variants
                    for kind in ("join", "toggle", "leave"):
                        dt, cnt, reb = bench.storm(kind, n, variant == "batched",
                                                   args.immediate_cap)
                        rebuilds[(variant, kind)] = reb
                        bench.check(P + (0 if kind == "leave" else n))
                        timed[(variant, kind)] = cnt
                        if rep >= args.warmup:
                            times[(variant, kind)].append(dt)
            for (variant, kind), ts in times.items():
                cnt = timed[(variant, kind)]
                row = dict(
                    population=P, storm=kind, n=n, variant=variant, changes_timed=cnt,
                    direct_table_size=bench.S, topics_per_user=TOPICS_PER_USER,
                    storm_ms=round(statistics.median(ts) * 1e3, 4),
                    storm_ms_min=round(min(ts) * 1e3, 4),
                    storm_ms_max=round(max(ts) * 1e3, 4),
                    us_per_change=round(statistics.median(ts) * 1e6 / cnt, 3),
                    us_per_change_min=round(min(ts) * 1e6 / cnt, 3),
                    us_per_change_max=round(max(ts) * 1e6 / cnt, 3),
                    rebuilds_per_storm=rebuilds[(variant, kind)],
                    reps=args.reps, device=args.device,
                )
                results.append(row)
                print(json.dumps(row), flush=True)
        del bench
        if args.device.startswith("cuda"):
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
