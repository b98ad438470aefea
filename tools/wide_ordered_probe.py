"""Wide batches on the ordered run (pie_set_wide_ordered): the 512 near-identical clocks of the headline batch (now - 977 ms q,
one cutoff, 16 of 32 disciplines) on the Zipf(1.1) corpus at cfg2 (10^7 rows / 10^4 users) and cfg3 (10^8 / 10^5), ordered run
always on (mode 2), three ways:
  (a) one wide batch with the switch off: every query reruns as a single scan (the behaviour before the switch existed)
  (b) eight ordinary 64-query batches on the run, up to three in flight
  (c) one wide batch with the switch on
Each figure is the median (min, max) over --regions timed regions of --reps passes each, ms per 512 queries, wall clock around
begin .. finish with a synchronize on both sides.  Prints one JSON record.

    python tools/wide_ordered_probe.py [--regions 5] [--reps 10] [--only cfg2]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import sph_pie_amd  # noqa: E402

T0 = 1_700_000_000_000
DAY, HOUR = 86400 * 1000, 3600 * 1000
SEED = 0x5EED5EED


def run(ctx, groups, wide, reps):
    """reps rounds of `groups` (lists of queries), as many in flight as the context takes -> ms per round, last M list"""
    begin = ctx.scan_wide_begin if wide else ctx.scan_batch_begin
    items = [g for _ in range(reps) for g in groups]
    ms = None
    ctx.synchronize()
    t = time.perf_counter()
    begun = done = 0
    while done < len(items):
        while begun < len(items) and ctx.batch_room() > 0:
            begin(items[begun])
            begun += 1
        ms = ctx.scan_wide_finish()
        done += 1
    ctx.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps, ms


def regions(ctx, groups, wide, reps, k):
    run(ctx, groups, wide, 1)   # warm-up: allocations, the run's batch arrays
    ts = [run(ctx, groups, wide, reps)[0] for _ in range(k)]
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "regions": k, "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    sph_pie_amd.build_hip()
    tables = {"cfg2": (10 ** 7, 10 ** 4), "cfg3": (10 ** 8, 10 ** 5)}
    q512 = [(T0 - 6 * HOUR - 977 * q, T0 - 61 * DAY, 0x55555555) for q in range(512)]
    eight = [q512[64 * i: 64 * (i + 1)] for i in range(8)]
    out = {"tool": "wide_ordered_probe", "corpus": "zipf(1.1)", "seed": hex(SEED), "results": []}
    for name, (n, U) in tables.items():
        if args.only and name != args.only:
            continue
        with sph_pie_amd.PieScan(0) as ctx:
            ctx.gen_synthetic_cdf(SEED, n, 0, n, U, 32, 0, sph_pie_amd.zipf_cdf(U))
            ctx.set_disciplines(0x55555555, 32)
            ctx.set_ordered_run(2)
            ctx.scan(*q512[0][:2])   # builds the run
            assert ctx.stats()["k1_variant"] & 0x2000
            ctx.set_wide_ordered(0)
            a = regions(ctx, [q512], True, 1, args.regions)
            assert ctx.batch_read_union_wide() is None
            b = regions(ctx, eight, False, args.reps, args.regions)
            assert ctx.stats()["k1_variant"] & 0x3000 == 0x3000
            ctx.set_wide_ordered(1)
            c = regions(ctx, [q512], True, args.reps, args.regions)
            st = ctx.stats()
            _, m_wide = run(ctx, [q512], True, 1)
            un = ctx.batch_union_wide_device_ptrs()
            rec = {"table": name, "rows": n, "users": U, "a_wide_switch_off": a, "b_eight_64_batches": b, "c_wide_switch_on": c,
                   "c_over_b": c["median_ms"] / b["median_ms"], "c_over_a": c["median_ms"] / a["median_ms"],
                   "k1_variant": hex(int(st["k1_variant"])), "candidates": int(st["candidates"]), "union_rows": int(un[4]),
                   "largest_union_bucket": int(st["max_bucket"]), "selected_512": int(sum(m_wide))}
            out["results"].append(rec)
            print(json.dumps(rec), file=sys.stderr)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
