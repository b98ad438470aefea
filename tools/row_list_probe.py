#!/usr/bin/env python3
"""What do the ordered row lists cost?  On one generated table (pie_gen_synthetic, the 1.25 x 10^7-row shard size of
tools/delete_users_probe.py by default), host wall time around each call, its waits and the copy of the list included:
  prune_before, retention_purge, retention_purge under a zone table, delete_user: `reps` calls each after one warm-up, every call
      on rows no earlier call tombstoned (ascending quantiles of the start column; fresh user ids)
  archive_queue: `reps` calls, the device time of the chain from pie_archive_stats (profiling on), the queue left on the device
  shard_table(0, 2): once, last (it consumes the table)
The library is PIE_HIP_LIB's or the tree's: one library per process, so two builds are compared in alternating processes.

usage: row_list_probe.py [--rows N] [--users U] [--reps R] [--out FILE]      -> one JSON line (and FILE)"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import sph_pie_amd as pie  # noqa: E402
from sph_pie_amd.binding import tz_table  # noqa: E402

SEED, D, DAY = 0x5EED5EED, 32, 86400000


def stats(ms):
    return {"median": float(np.median(ms)), "p90": float(np.percentile(ms, 90)), "n": len(ms)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=12_500_000)
    ap.add_argument("--users", type=int, default=10 ** 5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, reps = a.rows, a.reps
    out = {"lib": os.environ.get("PIE_HIP_LIB", "tree"), "rows": n, "users": a.users, "reps": reps}
    zone = tz_table("Europe/Berlin")
    with pie.PieScan(0) as ctx:
        ctx.gen_synthetic(SEED, n, 0, n, a.users, D, 0)
        start = np.sort(ctx.read_columns()[0])
        # 3 x (reps + 1) slices of half a percent of the rows each, oldest first: prune, then the two purges
        cut = [int(start[(i + 1) * n // 200]) for i in range(3 * (reps + 1))]
        calls = (("prune_before", lambda i: ctx.prune_before(cut[i])),
                 ("retention_purge", lambda i: ctx.retention_purge(cut[reps + 1 + i] + 62 * DAY, 2, 3600000)),
                 ("retention_purge_tz", lambda i: ctx.retention_purge(cut[2 * (reps + 1) + i] + 62 * DAY, 2, tz_table=zone)))
        for name, call in calls:
            ms, listed = [], 0
            for i in range(reps + 1):   # call 0 warms up
                t, rows = timed(lambda: call(i))
                assert rows.size > 0 and np.all(np.diff(rows) > 0)
                if i:
                    ms.append(t)
                    listed += rows.size
            out[name] = dict(stats(ms), wall_ms=ms, listed=listed)
        ids = np.random.default_rng(3).permutation(a.users)[: reps + 1]
        ms, listed = [], 0
        for i, u in enumerate(ids):
            t, rows = timed(lambda: ctx.delete_user(int(u)))
            if i:
                ms.append(t)
                listed += rows.size
        out["delete_user"] = dict(stats(ms), wall_ms=ms, listed=listed)
        ctx.set_profiling(1)
        now, ms, last = int(start[n // 2]) + 43200000, [], 0.0
        for i in range(reps + 1):
            q = ctx.archive_queue(now, fetch=False)
            total = ctx.archive_stats()[0]
            if i:
                ms.append(total - last)
            last = total
        out["archive_queue_device"] = dict(stats(ms), device_ms=ms, queued=int(q))
        ctx.set_profiling(0)
        ctx.synchronize()
        t, shape = timed(lambda: ctx.shard_table(0, 2))
        out["shard_table_0_of_2"] = {"wall_ms": t, "rows": shape[0], "users": shape[1]}
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
