"""What the search by global id costs: one of eight shards of cfg3 (10^8 rows / 10^5 users -> about 1.25 x 10^7 rows), bursts of
1 000 touches through pie_shard_set_end (global rows, a lower-bound search of the row map per element) against the same 1 000
touches through pie_set_end (local rows: the path that existed before), and bursts of 1 000 appended rows through
pie_shard_append_rows (global user ids, a search of the user map per row) against pie_append_rows (local ids).  Every burst
names only rows / users of this shard, so both paths do the same stores.  Each figure is the median (min, max) over --regions
timed regions of --reps bursts, microseconds per burst, wall clock with a synchronize on both sides of a region.  The plain
appends come last: they leave rows without a global row.  Prints one JSON record and writes it to profiles/.

    python tools/shard_mutate_probe.py [--regions 5] [--reps 20] [--rows 100000000] [--users 100000] [--world 8]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import sph_pie_amd  # noqa: E402

T0, SPAN, TTL = 1_700_000_000_000, 10_368_000_000, 43_200_000
SEED, BURST = 0x5EED5EED, 1000


def regions(ctx, burst, k, reps):
    burst()  # warm-up: staging areas, capacity
    ts = []
    for _ in range(k):
        ctx.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            burst()
        ctx.synchronize()
        ts.append((time.perf_counter() - t) * 1e6 / reps)
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts), "regions": k, "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--users", type=int, default=10 ** 5)
    ap.add_argument("--world", type=int, default=8)
    args = ap.parse_args()
    sph_pie_amd.build_hip()
    rng = np.random.default_rng(1)
    ctx = sph_pie_amd.PieScan(0)
    ctx.gen_synthetic(SEED, args.rows, 0, args.rows, args.users, 32, 0)
    n_local, u_local = ctx.shard_table(0, args.world)
    rows_g, users_g = ctx.shard_maps()
    users_g = users_g[:u_local]
    clock = [0]

    def rows_of(k):
        clock[0] += 1
        s = (T0 + SPAN + clock[0] * 100000 + np.arange(k)).astype(np.int64)
        lu = rng.integers(0, u_local, k).astype(np.int32)
        return s, s + TTL, lu, rng.integers(0, 32, k).astype(np.int32)

    # room for every timed append: the first one takes the growth path, the timed ones run in place
    s, e, lu, d = rows_of(BURST)
    ctx.shard_append_rows(s, e, users_g[lu], d, args.users)
    local = rng.choice(n_local, BURST, replace=False).astype(np.int32)
    glob = rows_g[local]
    vals = (T0 + SPAN + rng.integers(-TTL, TTL, BURST)).astype(np.int64)
    s, e, lu, d = rows_of(BURST)
    gu = users_g[lu]
    out = {"rows": args.rows, "users": args.users, "world": args.world, "shard_rows": n_local, "shard_users": u_local, "burst": BURST,
           "async_mutations": os.environ.get("PIE_ASYNC_MUTATIONS", "1")}
    out["shard_set_end"] = regions(ctx, lambda: ctx.shard_set_end(glob, vals), args.regions, args.reps)
    out["set_end"] = regions(ctx, lambda: ctx.set_end(local, vals), args.regions, args.reps)
    out["shard_append_rows"] = regions(ctx, lambda: ctx.shard_append_rows(s, e, gu, d, args.users), args.regions, args.reps)
    out["append_rows"] = regions(ctx, lambda: ctx.append_rows(s, e, lu, d, u_local), args.regions, args.reps)
    out["set_end_ratio"] = out["shard_set_end"]["median_us"] / out["set_end"]["median_us"]
    out["append_ratio"] = out["shard_append_rows"]["median_us"] / out["append_rows"]["median_us"]
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "shard_mutate_probe.json"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
