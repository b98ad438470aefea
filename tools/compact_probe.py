#!/usr/bin/env python3
"""What does pie_compact_rows cost?  For the synthetic corpus at cfg2 (10^7 rows) and cfg3 (10^8 rows), in creation order
(PIE_GEN_TIME_ORDERED) and in random order, and for dropped fractions 0, 0.1, 0.5, 0.9 and 1.0: the device time of the two
passes (HIP events inside the library: count + prefix, write), the wall time of the whole call (key rebuild included), with and
without PIE_COMPACT_SHRINK (every figure the median of 5 calls after a warm-up call, each on a freshly generated table), and the achieved bytes per second against the algorithmic count 20 N + 44 K (reads 16 N + 16 K, writes
24 K + 4 N + 4 K; K = kept rows).  The dropped fraction is set through dead_before: the quantile of `end` over a sample of the
table, so nothing has to be tombstoned first; the fraction actually dropped is reported.

At cfg2 the only route to a smaller table without pie_compact_rows is timed in the same process: read_columns -> numpy filter ->
load_columns.  The one expectation checked here: the whole pie_compact_rows call is faster than that round trip.

usage: compact_probe.py [--quick]     (--quick: cfg2 only)      -> profiles/compact_probe.json"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import sph_pie_amd as pie  # noqa: E402

SEED, D = 0x5EED5EED, 32
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
FRACTIONS = (0.0, 0.1, 0.5, 0.9, 1.0)
CONFIGS = [("cfg2", 10 ** 7, 10 ** 4), ("cfg3", 10 ** 8, 10 ** 5)]
ORDERS = [("time_ordered", pie.PIE_GEN_TIME_ORDERED), ("random", 0)]


def pcie_link():
    """Generation / width of the first AMD display device's link, from sysfs (read only); None when it cannot be told."""
    base = "/sys/bus/pci/devices"
    try:
        for dev in sorted(os.listdir(base)):
            p = os.path.join(base, dev)
            with open(os.path.join(p, "vendor")) as f:
                if f.read().strip() != "0x1002":
                    continue
            with open(os.path.join(p, "class")) as f:
                if not f.read().strip().startswith(("0x03", "0x12")):
                    continue
            with open(os.path.join(p, "current_link_speed")) as f:
                speed = f.read().strip()
            with open(os.path.join(p, "current_link_width")) as f:
                width = f.read().strip()
            gen = {"2.5": 1, "5.0": 2, "8.0": 3, "16.0": 4, "32.0": 5, "64.0": 6}.get(speed.split()[0])
            return {"speed": speed, "width": width, "generation": gen}
    except OSError:
        pass
    return None


def dead_before_for(ctx, n, frac, rng):
    if frac <= 0.0:
        return INT64_MIN
    if frac >= 1.0:
        return INT64_MAX
    sample = np.sort(rng.integers(0, n, min(n, 1_000_000))).astype(np.int32)
    ends = ctx.fetch_rows(sample)[1]
    return int(np.quantile(ends, frac))


REPS = 5   # every case: one unrecorded warm-up call on a fresh table, then the median of REPS calls, each on a fresh table


def median(xs):
    return float(np.median(np.asarray(xs, float)))


def one(ctx, n, U, flags, frac, shrink, rng):
    ctx.gen_synthetic(SEED, n, 0, n, U, D, flags)
    dead_before = dead_before_for(ctx, n, frac, rng)
    count, write, wall = [], [], []
    for rep in range(REPS + 1):
        if rep:
            ctx.gen_synthetic(SEED, n, 0, n, U, D, flags)
        ctx.synchronize()
        t0 = time.perf_counter()
        kept = ctx.compact_rows(dead_before, shrink=shrink)
        w = (time.perf_counter() - t0) * 1e3
        info = ctx.table_info()
        if rep:
            count.append(info["compact_count_ms"])
            write.append(info["compact_write_ms"])
            wall.append(w)
    count_ms, write_ms = median(count), median(write)
    dev_ms = count_ms + write_ms
    alg = 20 * n + 44 * kept if kept < n else 8 * n + 8 * n   # nothing dropped: the count pass and the identity maps
    return {"fraction_asked": frac, "dropped": 1.0 - kept / n, "kept": kept, "shrink": shrink, "reps": REPS, "count_ms": count_ms,
            "count_ms_min_max": [min(count), max(count)], "write_ms": write_ms, "write_ms_min_max": [min(write), max(write)],
            "wall_ms": median(wall), "wall_ms_min_max": [min(wall), max(wall)], "alg_bytes": alg,
            "count_gbs": 8 * n / (count_ms * 1e-3) / 1e9 if count_ms > 0 else None,
            "write_gbs": (12 * n + 44 * kept) / (write_ms * 1e-3) / 1e9 if write_ms > 0 and kept < n else None,
            "device_gbs": alg / (dev_ms * 1e-3) / 1e9 if dev_ms > 0 else None,
            "write_ns_per_kept_row": write_ms * 1e6 / kept if kept and kept < n else None,
            "table_bytes": info["table_bytes"], "workspace_bytes": info["workspace_bytes"], "index_build_ms": info["index_build_ms"]}


def shard_against_compact(ctx, n, U, flags):
    """pie_shard_table(0, 2) keeps the rows of half the users with k_shard_row_count / k_shard_row_write and copies them into a
    right-sized table; pie_compact_rows with PIE_COMPACT_SHRINK at half the rows dropped does the same kind of work with the new
    kernels.  The library times no kernel of the shard path, so this compares WHOLE CALLS (wall time, key rebuild in both), per
    row kept: the shard call also flags and renumbers users and copies the columns a second time."""
    rng = np.random.default_rng(2)
    shard, comp = [], []
    for rep in range(REPS + 1):
        ctx.gen_synthetic(SEED, n, 0, n, U, D, flags)
        ctx.synchronize()
        t0 = time.perf_counter()
        kept_s, _ = ctx.shard_table(0, 2)
        w = (time.perf_counter() - t0) * 1e3
        if rep:
            shard.append(w)
    ctx.gen_synthetic(SEED, n, 0, n, U, D, flags)
    dead_before = dead_before_for(ctx, n, 0.5, rng)
    for rep in range(REPS + 1):
        ctx.gen_synthetic(SEED, n, 0, n, U, D, flags)
        ctx.synchronize()
        t0 = time.perf_counter()
        kept_c = ctx.compact_rows(dead_before, shrink=True)
        w = (time.perf_counter() - t0) * 1e3
        if rep:
            comp.append(w)
    return {"rows": n, "reps": REPS, "shard_call_ms": median(shard), "shard_kept": kept_s, "shard_ns_per_kept_row": median(shard) * 1e6 / kept_s,
            "compact_shrink_call_ms": median(comp), "compact_kept": kept_c, "compact_ns_per_kept_row": median(comp) * 1e6 / kept_c}


def round_trip(ctx, n, U, flags, frac, rng):
    """The route without pie_compact_rows: columns to the host, a numpy filter, columns back (keys and all rebuilt by the load).
    Warmed and repeated like the compaction: the median of REPS round trips after one that is not recorded."""
    ctx.gen_synthetic(SEED, n, 0, n, U, D, flags)
    dead_before = dead_before_for(ctx, n, frac, rng)
    wall = []
    for rep in range(REPS + 1):
        if rep:
            ctx.gen_synthetic(SEED, n, 0, n, U, D, flags)
        ctx.synchronize()
        t0 = time.perf_counter()
        s, e, u, d = ctx.read_columns()
        keep = e > dead_before
        ctx.load_columns(s[keep], e[keep], u[keep], d[keep], U)
        ctx.synchronize()
        if rep:
            wall.append((time.perf_counter() - t0) * 1e3)
    return {"fraction_asked": frac, "kept": int(np.count_nonzero(keep)), "reps": REPS, "wall_ms": median(wall), "wall_ms_min_max": [min(wall), max(wall)]}


def main():
    quick = "--quick" in sys.argv[1:]
    rng = np.random.default_rng(1)
    out = {"tool": "tools/compact_probe.py", "pcie": pcie_link(), "alg_bytes": "20 N + 44 K (K kept rows); 16 N when nothing is dropped", "runs": [], "round_trip_cfg2": []}
    with pie.PieScan(0) as ctx:
        for name, n, U in CONFIGS[:1] if quick else CONFIGS:
            for oname, flags in ORDERS:
                for frac in FRACTIONS:
                    for shrink in (False, True):
                        r = one(ctx, n, U, flags, frac, shrink, rng)
                        r.update(config=name, rows=n, order=oname)
                        out["runs"].append(r)
                        print("%s %-12s drop %.2f shrink %d: count %.3f ms (%.0f GB/s), write %.3f ms (%s GB/s), both %s GB/s, call %.2f ms [%.2f .. %.2f]" % (
                            name, oname, r["dropped"], shrink, r["count_ms"], r["count_gbs"] or 0, r["write_ms"],
                            "%.0f" % r["write_gbs"] if r["write_gbs"] else "-", "%.0f" % r["device_gbs"] if r["device_gbs"] else "-",
                            r["wall_ms"], r["wall_ms_min_max"][0], r["wall_ms_min_max"][1]), flush=True)
                if name == "cfg2":
                    for frac in FRACTIONS:
                        r = round_trip(ctx, n, U, flags, frac, rng)
                        r.update(order=oname)
                        out["round_trip_cfg2"].append(r)
                        print("cfg2 %-12s drop %.2f: read_columns -> filter -> load_columns %.1f ms" % (oname, frac, r["wall_ms"]), flush=True)
        if not quick:
            out["shard_table_against_compact_cfg3"] = shard_against_compact(ctx, 10 ** 8, 10 ** 5, 0)
            print("cfg3 random: pie_shard_table(0, 2) %.1f ms (%.3f ns per kept row), pie_compact_rows shrink at 0.5 dropped %.1f ms (%.3f ns per kept row)" % (
                out["shard_table_against_compact_cfg3"]["shard_call_ms"], out["shard_table_against_compact_cfg3"]["shard_ns_per_kept_row"],
                out["shard_table_against_compact_cfg3"]["compact_shrink_call_ms"], out["shard_table_against_compact_cfg3"]["compact_ns_per_kept_row"]), flush=True)
    # the one expectation: at cfg2 the whole call beats the round trip, case by case
    ratios = []
    for rt in out["round_trip_cfg2"]:
        for r in out["runs"]:
            if r["config"] == "cfg2" and r["order"] == rt["order"] and r["fraction_asked"] == rt["fraction_asked"]:
                ratios.append({"order": rt["order"], "fraction_asked": rt["fraction_asked"], "shrink": r["shrink"], "round_trip_over_compact": rt["wall_ms"] / r["wall_ms"]})
    out["cfg2_round_trip_over_compact"] = ratios
    out["cfg2_compact_faster_than_round_trip"] = bool(ratios) and all(x["round_trip_over_compact"] > 1.0 for x in ratios)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "compact_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("cfg2: pie_compact_rows faster than the round trip in every case: %s (smallest ratio %.1f)" % (
        out["cfg2_compact_faster_than_round_trip"], min(x["round_trip_over_compact"] for x in ratios)))
    if not out["cfg2_compact_faster_than_round_trip"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
