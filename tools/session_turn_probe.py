#!/usr/bin/env python3
"""What does a turn that logs in (pie_session_turn) cost, beside what a caller does today, and did the existing path get slower?

On the benchmark's table (cfg3: 10^8 generated rows, 10^5 users; every row gets a random key, as tools/token_turn_probe.py gives
them) the host wall time through the Python binding, median and 90th percentile over --reps calls, of

  session     ctx.session_turn(ops, user, disc): one upload, one kernel, one download, one wait
  three_calls the same ops the way a caller makes them today: pie_append_rows of the turn's creates, pie_token_append of their
              keys, then pie_token_turn of the other ops.  The split is done ahead of the clock: only the device calls are timed.

for turns of 1, 64 and 4 096 ops under two mixes (get / touch / delete / create): 95 / 0 / 0 / 5 % and 75 / 15 / 5 / 5 %.  The
creates of a turn are max(1, round(5 % of k)) ops at random places, so every timed turn logs somebody in (k = 1 is a login alone);
the other ops name distinct sessions that are live at the clock.  One create is made before anything is timed: the generated table
is exactly full, and the first append doubles its capacity once.

Then the two bars of the existing path, on create-free lists (80 % get, 15 % touch, 5 % delete on distinct keys):
  token_turn            ctx.token_turn(ops) of this library
  session_no_create     ctx.session_turn(ops) of this library on the same kind of list
  baseline_token_turn   ctx.token_turn(ops) of the library given with --baseline-lib (the parent commit's, built beside this one),
                        on a table of its own generated the same way
A bar holds when the median stays within the baseline's own 90th percentile.

usage: session_turn_probe.py [--rows N] [--reps R] [--baseline-lib FILE] [--out FILE]      -> profiles/session_turn_probe.json"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import sph_pie_amd as pie  # noqa: E402
from sph_pie_amd import binding, build  # noqa: E402

SEED, D = 0x5EED5EED, 32
TTL = 12 * 3600 * 1000
END_NONE = -(2 ** 63)
MIXES = {"95_0_0_5": (0.95, 0.0, 0.0), "75_15_5_5": (0.75, 0.15, 0.05)}
CREATE_SHARE = 0.05
PLAIN = (0.80, 0.15, 0.05)
SIZES = (1, 64, 4096)


def open_ctx(lib_path):
    """a context of the library at lib_path; an older library lacks the newest entry points, which are then left untyped"""
    have = ctypes.CDLL(lib_path)
    sigs = binding._SIGS
    binding._SIGS = [s for s in sigs if hasattr(have, s[0])]
    try:
        return pie.PieScan(0, lib_path=lib_path)
    finally:
        binding._SIGS = sigs


def load_table(ctx, rng, n, users, chunk):
    """the generated table with a random key per row -> (clock at which half the sessions are live, keys of live sessions)"""
    ctx.gen_synthetic(SEED, n, 0, n, users, D, 0)
    sample = []
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        keys = rng.integers(0, 2 ** 64, (hi - lo, 2), dtype=np.uint64)
        (ctx.token_set if lo == 0 else ctx.token_append)(keys)
        sample.append(keys[rng.integers(0, hi - lo, min(hi - lo, 1 + (1 << 21) * chunk // n))])
    ctx.synchronize()
    sample = np.concatenate(sample)
    got = ctx.token_lookup(sample, END_NONE)
    clock = int(np.median(got["end"]))
    return clock, sample[got["end"] > clock + 8]


def make_turn(rng, pool, k, mix, clock, n_create, users):
    ops = np.zeros(k, pie.TURN_OP)
    ops["tok"] = pool[rng.choice(pool.shape[0], k, replace=False)]
    ops["now"] = clock
    p = np.array(mix) / sum(mix)
    ops["kind"] = rng.choice([pie.TURN_GET, pie.TURN_TOUCH, pie.TURN_DELETE], k, p=p)
    if n_create:
        at = rng.choice(k, n_create, replace=False)
        ops["kind"][at] = pie.TURN_CREATE
        ops["tok"][at] = rng.integers(0, 2 ** 64, (n_create, 2), dtype=np.uint64)
    ops["new_end"] = np.where(np.isin(ops["kind"], (pie.TURN_TOUCH, pie.TURN_CREATE)), ops["now"] + TTL, 0)
    return ops, rng.integers(0, users, k).astype(np.int32), rng.integers(0, D, k).astype(np.int32)


def timed(reps, make, run):
    times = []
    for rep in range(reps + 3):                  # three warm-up calls
        args = make()
        t0 = time.perf_counter()
        run(*args)
        dt = time.perf_counter() - t0
        if rep >= 3:
            times.append(dt * 1e3)
    return float(np.median(times)), float(np.percentile(times, 90))


def plain_series(ctx, rng, pool, clock, users, reps, call):
    out = {}
    for k in SIZES:
        out[k] = timed(reps, lambda: (make_turn(rng, pool, k, PLAIN, clock, 0, users)[0],), call)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "session_turn_probe.json"))
    a = ap.parse_args()
    n, users = a.rows, max(1, a.rows // 1000)
    out = {"rows": n, "users": users, "reps": a.reps, "create_share": CREATE_SHARE, "series": [], "existing_path": []}
    baseline = None
    if a.baseline_lib:
        rng = np.random.default_rng(1)
        with open_ctx(a.baseline_lib) as ctx:
            clock, pool = load_table(ctx, rng, n, users, a.chunk)
            baseline = plain_series(ctx, rng, pool, clock, users, a.reps, ctx.token_turn)
        print("baseline library measured:", baseline, flush=True)
    rng = np.random.default_rng(1)
    with open_ctx(build.HIP_LIB) as ctx:
        clock, pool = load_table(ctx, rng, n, users, a.chunk)
        out["clock"], out["pool"] = clock, int(pool.shape[0])
        print("table and keys ready: %d live sessions to draw from" % pool.shape[0], flush=True)
        ours = plain_series(ctx, rng, pool, clock, users, a.reps, ctx.token_turn)
        no_create = plain_series(ctx, rng, pool, clock, users, a.reps, lambda ops: ctx.session_turn(ops))
        for k in SIZES:
            rec = {"k": k, "mix": "80_15_5_0", "token_turn_median_ms": ours[k][0], "token_turn_p90_ms": ours[k][1],
                   "session_no_create_median_ms": no_create[k][0], "session_no_create_p90_ms": no_create[k][1],
                   "session_no_create_within_token_turn_p90": no_create[k][0] <= ours[k][1]}
            if baseline:
                rec.update({"baseline_token_turn_median_ms": baseline[k][0], "baseline_token_turn_p90_ms": baseline[k][1],
                            "token_turn_within_baseline_p90": ours[k][0] <= baseline[k][1],
                            "session_no_create_within_baseline_p90": no_create[k][0] <= baseline[k][1]})
            out["existing_path"].append(rec)
            print(rec, flush=True)
        # the first create doubles the capacity of the exactly-full generated table: once, ahead of the clock
        t0 = time.perf_counter()
        ctx.session_turn(*make_turn(rng, pool, 1, MIXES["95_0_0_5"], clock, 1, users), users)
        out["first_create_ms"] = (time.perf_counter() - t0) * 1e3

        def three_calls(creates, keys, rest):
            ctx.append_rows(*creates, users)
            ctx.token_append(keys)
            if rest.shape[0]:
                ctx.token_turn(rest)

        def split(ops, user, disc):
            c = ops["kind"] == pie.TURN_CREATE
            cols = [np.ascontiguousarray(x) for x in (ops["now"][c], ops["new_end"][c], user[c], disc[c])]
            return cols, np.ascontiguousarray(ops["tok"][c]), np.ascontiguousarray(ops[~c])

        for k in SIZES:
            n_create = max(1, int(round(CREATE_SHARE * k)))
            for name, mix in MIXES.items():
                rec = {"k": k, "mix": name, "creates": n_create}
                rec["session_median_ms"], rec["session_p90_ms"] = timed(
                    a.reps, lambda: make_turn(rng, pool, k, mix, clock, n_create, users), lambda ops, u, d: ctx.session_turn(ops, u, d, users))
                rec["three_calls_median_ms"], rec["three_calls_p90_ms"] = timed(
                    a.reps, lambda: split(*make_turn(rng, pool, k, mix, clock, n_create, users)), three_calls)
                rec["three_calls_over_session"] = rec["three_calls_median_ms"] / rec["session_median_ms"]
                out["series"].append(rec)
                print(rec, flush=True)
        info = ctx.table_info()
        out["rows_after"], out["token_builds"] = int(info["rows"]), int(info["token_builds"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
