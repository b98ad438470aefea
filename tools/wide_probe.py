"""Wide batches against ordinary ones over the same queries: eight 64-query batches vs one 512-query wide batch, and a
256-query wide batch, on cfg3 (10^8 rows / 10^5 users / 32 disciplines) and on a 1/8 shard (1.25 x 10^7 rows / 12 500 users),
with bench.py's near-identical clocks (now - 977 ms q) and a heterogeneous mix (several cutoffs and masks), pipelined up to
three batches per lane on 1 and 3 lanes.  Prints one JSON record: ms per pass, feeds/s, union rows, candidates, fallbacks.

    python tools/wide_probe.py [--reps 20] [--only shard]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import sph_pie_amd  # noqa: E402

T0 = 1_700_000_000_000
DAY, HOUR = 86400 * 1000, 3600 * 1000
ALL = 2 ** 64 - 1


def queries(mix, k):
    if mix == "bench":
        return [(T0 - 6 * HOUR - 977 * q, T0 - 61 * DAY, ALL) for q in range(k)]
    masks = [0x5555555555555555, 0xAAAAAAAAAAAAAAAA, ALL, 0x00000000FFFF0000, 0x1, 0x8000000000000001]
    return [(T0 - 6 * HOUR - 977 * i - (i % 3) * HOUR, T0 - (61 + i % 4) * DAY - 13 * i, masks[i % len(masks)]) for i in range(k)]


def run(ctx, groups, wide, reps):
    """reps rounds of `groups` (lists of queries), up to three per lane in flight -> ms per round, last round's M"""
    begin = ctx.scan_wide_begin if wide else ctx.scan_batch_begin
    finish = ctx.scan_wide_finish
    items = [g for _ in range(reps) for g in groups]
    ms = None
    ctx.synchronize()
    t = time.perf_counter()
    begun = done = 0
    while done < len(items):
        while begun < len(items) and ctx.batch_room() > 0:
            begin(items[begun])
            begun += 1
        ms = finish()
        done += 1
    ctx.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    sph_pie_amd.build_hip()
    tables = {"cfg3": (10 ** 8, 10 ** 5), "shard": (12_500_000, 12_500)}
    out = {"tool": "wide_probe", "reps": args.reps, "results": []}
    with sph_pie_amd.PieScan(0) as ctx:
        for name, (n, U) in tables.items():
            if args.only and name != args.only:
                continue
            ctx.gen_synthetic(0x5EED5EED, n, 0, n, U, 32, 0)
            ctx.set_disciplines(ALL, 32)
            for lanes in (1, 3):
                ctx.set_batch_lanes(lanes)
                for mix in ("bench", "mixed"):
                    q512 = queries(mix, 512)
                    run(ctx, [q512], True, 2)   # warm-up (allocations, bucket capacity)
                    eight = [q512[64 * i: 64 * (i + 1)] for i in range(8)]
                    run(ctx, eight, False, 2)
                    t_eight, _ = run(ctx, eight, False, args.reps)
                    t_wide, m_wide = run(ctx, [q512], True, args.reps)
                    st = ctx.stats()
                    un = ctx.batch_union_wide_device_ptrs() if ctx.batch_read_union_wide() is not None else None
                    t_256, _ = run(ctx, [q512[:256]], True, args.reps)
                    t_64, _ = run(ctx, [q512[:64]], False, args.reps)
                    out["results"].append({
                        "table": name, "rows": n, "users": U, "lanes": lanes, "mix": mix,
                        "ms_eight_64_batches": t_eight, "ms_one_512_wide": t_wide, "ms_one_256_wide": t_256, "ms_one_64_batch": t_64,
                        "wide512_over_batch64": t_wide / t_64, "feeds_per_s_eight_64": 512e3 / t_eight, "feeds_per_s_wide_512": 512e3 / t_wide,
                        "union_rows_512": un[4] if un else None, "candidates_512": int(st["candidates"]),
                        "selected_512": int(sum(m_wide)), "union_kept": un is not None,
                    })
                    print(json.dumps(out["results"][-1]), file=sys.stderr)
            ctx.set_batch_lanes(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
