#!/usr/bin/env python3
"""Extract a per-kernel stats table from rocprofv3 output (rocpd sqlite DB
or kernel_stats CSV) into the plain-text format committed under profiles/.

Usage: python scripts/prof_extract.py <dir-or-file> [out.txt] [--interval KERNEL]
Introspects the schema (rocprofv3's table/column names move between
versions) and prints: kernel, calls, total_us, avg_us, %, plus
vgpr/sgpr/scratch when the symbol table carries them.

From a rocpd DB (which has every dispatch's start and end) it adds a
timeline table: per kernel, the median duration and the median IDLE time
before it, i.e. from the end of the dispatch that finished last before it
to its own start.  With --interval KERNEL it also gives the median interval
from the end of one KERNEL dispatch to the start of the next, and how much
of that interval other kernels were running, KERNEL's own shortest, median
and longest dispatch, and the dispatches that stand between two KERNELs one
by one, in order, each with its median duration and idle time before it.
"""

import csv
import glob
import os
import sqlite3
import sys


# (start_ns, end_ns, kernel) of every dispatch seen in a DB
TIMELINE = []


def find_inputs(path):
    if os.path.isfile(path):
        return [path]
    return (sorted(glob.glob(os.path.join(path, "**", "*.db"), recursive=True))
            or sorted(glob.glob(os.path.join(path, "**", "*kernel_stats*.csv"),
                                recursive=True)))


def cols(con, table):
    return [r[1] for r in con.execute(f"PRAGMA table_info('{table}')")]


def pick(names, *subs):
    for s in subs:
        for n in names:
            if s in n.lower():
                return n
    return None


def extract_db(path):
    con = sqlite3.connect(path)
    tables = [r[0] for r in con.execute(
        "SELECT name FROM sqlite_master WHERE type='table'")]
    dispatch = pick(tables, "kernel_dispatch")
    symbol = pick(tables, "kernel_symbol", "kernel_info", "symbol")
    if not dispatch:
        print(f"## {path}: no kernel_dispatch table; tables = {tables}")
        return []
    dc = cols(con, dispatch)
    start = pick(dc, "start")
    end = pick(dc, "end")
    kid = pick(dc, "kernel_id", "symbol_id", "kernel")
    rows = {}
    names = {}
    res = {}
    if symbol:
        sc = cols(con, symbol)
        sid = pick(sc, "id")
        sname = pick(sc, "display_name", "kernel_name", "name")
        svgpr = pick(sc, "arch_vgpr", "vgpr")
        ssgpr = pick(sc, "sgpr")
        sscr = pick(sc, "private_segment", "scratch")
        sagpr = pick(sc, "accum_vgpr", "agpr")
        for r in con.execute(f"SELECT * FROM {symbol}"):
            d = dict(zip(sc, r))
            names[d[sid]] = d.get(sname, "?")
            res[d[sid]] = (d.get(svgpr), d.get(sagpr), d.get(ssgpr), d.get(sscr))
    for r in con.execute(f"SELECT {kid}, {start}, {end} FROM {dispatch}"):
        k, s, e = r
        dur = (e - s) / 1e3  # ns -> us
        c, t = rows.get(k, (0, 0.0))
        rows[k] = (c + 1, t + dur)
        TIMELINE.append((s, e, str(names.get(k, k))))
    out = []
    for k, (c, t) in rows.items():
        nm = str(names.get(k, k))
        v = res.get(k, (None,) * 4)
        out.append((nm, c, t, v))
    return out


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return 0.0 if not n else (xs[n // 2] if n % 2 else (xs[n // 2 - 1] + xs[n // 2]) / 2)


def timeline_text(interval_kernel):
    """Per-kernel median duration and idle-before; the interval summary."""
    tl = sorted(TIMELINE)
    dur, idle = {}, {}
    last_end = None
    for s, e, nm in tl:
        dur.setdefault(nm, []).append((e - s) / 1e3)
        if last_end is not None:
            idle.setdefault(nm, []).append(max(0, s - last_end) / 1e3)
        last_end = e if last_end is None else max(last_end, e)
    lines = ["", f"{'kernel (timeline)':<52} {'calls':>6} {'med_dur_us':>11} {'med_idle_before_us':>19}"]
    for nm in sorted(dur, key=lambda n: -sum(dur[n])):
        lines.append(f"{nm[:52]:<52} {len(dur[nm]):>6} {median(dur[nm]):>11.2f} "
                     f"{median(idle.get(nm, [])):>19.2f}")
    if interval_kernel:
        # a template instance's name starts with its return type
        marks = [i for i, (_s, _e, nm) in enumerate(tl)
                 if nm.removeprefix("void ").startswith(interval_kernel)]
        spans, busy = [], []
        for a, b in zip(marks, marks[1:]):
            spans.append((tl[b][0] - tl[a][1]) / 1e3)
            busy.append(sum(e - s for s, e, _nm in tl[a + 1:b]) / 1e3)
        # the steady state: the second half of the intervals (past the warm-up)
        spans, busy = spans[len(spans) // 2:], busy[len(busy) // 2:]
        lines += ["", f"end of {interval_kernel} -> start of the next, median of the last "
                      f"{len(spans)} intervals: {median(spans):.1f} us, "
                      f"kernel time inside it {median(busy):.1f} us, "
                      f"idle {median(spans) - median(busy):.1f} us"]
        if marks:
            lines += chain_lines(tl, marks, interval_kernel)
    return "\n".join(lines) + "\n"


def chain_lines(tl, marks, interval_kernel):
    """KERNEL's own durations, and the dispatches between one KERNEL and the
    next, position by position: a name shared by several launches of a step
    (the blit kernel of every copy) is told apart by where it stands."""
    durs = [(tl[i][1] - tl[i][0]) / 1e3 for i in marks]
    lines = ["", f"{interval_kernel}: {len(durs)} dispatches, duration min {min(durs):.2f} / "
                 f"median {median(durs):.2f} / max {max(durs):.2f} us, "
                 f"spread {max(durs) - min(durs):.2f} us"]
    pairs = list(zip(marks, marks[1:]))
    pairs = pairs[len(pairs) // 2:]  # the steady state, as above
    chains = {}
    for a, b in pairs:
        chains.setdefault(tuple(nm for _s, _e, nm in tl[a + 1:b]), []).append(a)
    if not chains:
        return lines
    names, starts = max(chains.items(), key=lambda kv: len(kv[1]))
    lines += ["", f"dispatches after {interval_kernel} up to the next one, in order "
                  f"({len(starts)} of the last {len(pairs)} intervals have this sequence):",
              f"{'#':>2} {'kernel':<52} {'med_dur_us':>11} {'med_idle_before_us':>19}"]
    for k, nm in enumerate(names):
        d = [(tl[a + 1 + k][1] - tl[a + 1 + k][0]) / 1e3 for a in starts]
        idle = [max(0, tl[a + 1 + k][0] - max(e for _s, e, _n in tl[:a + 1 + k])) / 1e3
                for a in starts]
        lines.append(f"{k + 1:>2} {nm[:52]:<52} {median(d):>11.2f} {median(idle):>19.2f}")
    return lines


def extract_csv(path):
    out = []
    with open(path) as f:
        for row in csv.DictReader(f):
            nm = row.get("Name") or row.get("KernelName") or "?"
            c = int(row.get("Calls") or row.get("TotalCalls") or 1)
            t = float(row.get("TotalDurationNs", 0)) / 1e3
            out.append((nm, c, t, (None,) * 4))
    return out


def main():
    interval_kernel = None
    if "--interval" in sys.argv:
        k = sys.argv.index("--interval")
        interval_kernel = sys.argv[k + 1]
        del sys.argv[k:k + 2]
    path = sys.argv[1]
    inputs = find_inputs(path)
    if not inputs:
        print(f"no rocprof outputs under {path}")
        sys.exit(1)
    rows = []
    for p in inputs:
        rows += extract_db(p) if p.endswith(".db") else extract_csv(p)
    agg = {}
    for nm, c, t, v in rows:
        c0, t0, v0 = agg.get(nm, (0, 0.0, v))
        agg[nm] = (c0 + c, t0 + t, v0 if v0[0] is not None else v)
    total = sum(t for _c, t, _v in agg.values()) or 1.0
    lines = [f"{'kernel':<52} {'calls':>6} {'total_us':>11} {'avg_us':>9} "
             f"{'%':>6} {'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'scratch_B':>9}"]
    for nm, (c, t, v) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        vg, ag, sg, scr = (x if x is not None else "-" for x in v)
        lines.append(f"{nm[:52]:<52} {c:>6} {t:>11.1f} {t / c:>9.2f} "
                     f"{t / total * 100:>5.1f}% {vg:>5} {ag:>5} {sg:>5} {scr:>9}")
    text = "\n".join(lines) + "\n"
    if TIMELINE:
        text += timeline_text(interval_kernel)
    print(text)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
