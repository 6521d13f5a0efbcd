#!/usr/bin/env python
"""Per-queue accounting of the steady-state forwards in a rocprofv3 --kernel-trace rocpd database: for every hardware queue
the sum of its kernels' durations per forward, the time per forward during which at least one of its kernels ran (busy span),
and its longest kernels -- next to the spacing of the forwards.  With in-order streams the throughput of pipelined forwards
is bounded by the busiest queue: this is the table that says which chain that is.

    python tools/stream_table.py <results.db> [--last N forwards, default 60] [--grep name]

A forward is counted at every lstm_prep_kernel / lstm_pack_kernel launch (one per forward); the window is the last N of them
but two (the timed replays of a plain bench.py run come last)."""
import sqlite3
import sys


def short(name):
    return name.split("(")[0].replace("(anonymous namespace)::", "").replace("void ", "")[:48]


def main():
    db = sys.argv[1]
    last = int(sys.argv[sys.argv.index("--last") + 1]) if "--last" in sys.argv else 60
    grep = sys.argv[sys.argv.index("--grep") + 1] if "--grep" in sys.argv else "label_gcn"
    cur = sqlite3.connect(db).cursor()
    tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
    disp = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
    sym = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
    rows = cur.execute("select d.start, d.end, d.queue_id, s.kernel_name from %s d join %s s on d.kernel_id = s.id order by d.start"
                       % (disp, sym)).fetchall()
    marks = [r[0] for r in rows if "lstm_prep_kernel" in r[3] or "lstm_pack_kernel(" in r[3]]
    if len(marks) < last + 3:
        last = len(marks) - 3
    t0, t1, n = marks[-last - 2], marks[-2], last
    win = [r for r in rows if t0 <= r[0] < t1]
    print("window: %d forwards, %.1f us per forward, %d dispatches per forward" % (n, (t1 - t0) / 1e3 / n, len(win) // n))
    print("| queue | kernels / fwd | kernel time / fwd us | busy span / fwd us | idle / fwd us | longest kernels (avg us x launches / fwd) |")
    print("|---|---|---|---|---|---|")
    for q in sorted({r[2] for r in win}):
        mine = [r for r in win if r[2] == q]
        ksum = sum(r[1] - r[0] for r in mine)
        busy, end = 0, 0
        for s, e, _, _ in mine:                         # union of the intervals (sorted by start)
            if e > end:
                busy += e - max(s, end)
                end = e
        by = {}
        for s, e, _, name in mine:
            by.setdefault(short(name), []).append(e - s)
        top = sorted(by.items(), key=lambda kv: -sum(kv[1]))[:4]
        print("| %d | %.1f | %.1f | %.1f | %.1f | %s |" % (
            q, len(mine) / n, ksum / 1e3 / n, busy / 1e3 / n, (t1 - t0 - busy) / 1e3 / n,
            "; ".join("%s %.1f x %.1f" % (k, sum(v) / len(v) / 1e3, len(v) / n) for k, v in top)))
    by = {}
    for s, e, _, name in win:
        if grep in name:
            by.setdefault(short(name), []).append(e - s)
    for k, v in sorted(by.items()):
        v.sort()
        h = len(v) // 2                                 # two launches per forward (object / place graph): the halves apart
        print("%s: %d launches (%.1f / fwd), avg %.2f us (shorter half %.2f, longer half %.2f), min %.2f, max %.2f" % (
            k, len(v), len(v) / n, sum(v) / len(v) / 1e3, sum(v[:h]) / max(h, 1) / 1e3, sum(v[h:]) / max(len(v) - h, 1) / 1e3,
            v[0] / 1e3, v[-1] / 1e3))


if __name__ == "__main__":
    main()
