#!/usr/bin/env python3
"""What is keeping the ordered run through a login worth (pie_set_turn_ordered), what does it cost, and did the existing paths get
slower?  The Zipf(1.1) corpus of pie_gen_synthetic_cdf (cfg3: 10^8 rows, 10^5 users), a random token key per row, mode 2 of the
ordered run, host wall time through the Python binding, median and 90th percentile over --steps steps.

  mixed      one step = one session_turn of 64 ops (3 creates, the rest 80 / 15 / 5 % get / touch / delete on live sessions) and one
             16-query batch.  Switch on and switch off in alternation (two contexts of this library, one step each in turn); per
             leg the step time, ordered_builds and ordered_respreads at the end, and how many batches ran on the run.
  keep_cost  a create turn of 64 and of 4 096 ops (5 % creates) on a table with a valid run, switch on: the gather and the insert
             launches are inside; beside it the same turns on the same table with mode 0 (no run).
  existing   switch off, this library and — in a process of its own — the library given with --baseline-lib (the parent commit's):
             create turns of 1 / 64 / 4 096 ops, create-free token_turn at the same sizes, append_rows of 1 000 rows on a table with
             a run.  A bar holds when this library's median lies within the baseline's 90th percentile.

usage: session_turn_ordered_probe.py [--rows N] [--steps S] [--baseline-lib FILE] [--out FILE]
       -> profiles/session_turn_ordered_probe.json"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
import sph_pie_amd as pie  # noqa: E402
from sph_pie_amd import binding, build  # noqa: E402

SEED, D = 0x5EED5EED, 32
TTL = 12 * 3600 * 1000
END_NONE = -(2 ** 63)
HOUR, DAY = 3600 * 1000, 86400 * 1000
PLAIN = (0.80, 0.15, 0.05)
SIZES = (1, 64, 4096)


def zipf_cdf(n_users, exponent=1.1):
    w = 1.0 / np.arange(1, n_users + 1, dtype=np.float64) ** exponent
    c = np.cumsum(w) / w.sum()
    thr = np.minimum(np.floor(c * 2.0 ** 64), 2.0 ** 64 - 2048).astype(np.uint64)
    thr[-1] = np.uint64(2 ** 64 - 1)
    return np.maximum.accumulate(thr)


def open_ctx(lib_path):
    """a context of the library at lib_path; an older library lacks the newest entry points, which are then left untyped"""
    have = ctypes.CDLL(lib_path)
    sigs = binding._SIGS
    binding._SIGS = [s for s in sigs if hasattr(have, s[0])]
    try:
        return pie.PieScan(0, lib_path=lib_path)
    finally:
        binding._SIGS = sigs


def load_table(ctx, rng, n, users, chunk, mode):
    """the Zipf table with a random key per row and room for the logins -> (clock, keys of sessions live at it, the next start)"""
    ctx.set_ordered_run(mode)
    ctx.gen_synthetic_cdf(SEED, n, 0, n, users, D, 0, zipf_cdf(users))
    sample = []
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        keys = rng.integers(0, 2 ** 64, (hi - lo, 2), dtype=np.uint64)
        (ctx.token_set if lo == 0 else ctx.token_append)(keys)
        sample.append(keys[rng.integers(0, hi - lo, min(hi - lo, 1 + (1 << 21) * chunk // n))])
    sample = np.concatenate(sample)
    got = ctx.token_lookup(sample, END_NONE)
    clock = int(np.median(got["end"]))
    top = int(got["start"].max()) + DAY            # logins are stamped behind every start of the table: they arrive in time order
    # the generated table is exactly full: one login ahead of every clock doubles its capacity
    first = np.zeros(1, pie.TURN_OP)
    first["tok"], first["now"], first["new_end"], first["kind"] = rng.integers(0, 2 ** 64, (1, 2), dtype=np.uint64), top, top + TTL, pie.TURN_CREATE
    ctx.session_turn(first, np.zeros(1, np.int32), np.zeros(1, np.int32), users)
    ctx.synchronize()
    print("table of %d rows and its keys ready" % n, file=sys.stderr, flush=True)
    return clock, sample[got["end"] > clock + 8], top + 1


def make_turn(rng, pool, k, clock, n_create, users, start):
    ops = np.zeros(k, pie.TURN_OP)
    ops["tok"] = pool[rng.choice(pool.shape[0], k, replace=False)]
    ops["now"] = clock
    ops["kind"] = rng.choice([pie.TURN_GET, pie.TURN_TOUCH, pie.TURN_DELETE], k, p=PLAIN)
    if n_create:
        at = np.sort(rng.choice(k, n_create, replace=False))
        ops["kind"][at] = pie.TURN_CREATE
        ops["tok"][at] = rng.integers(0, 2 ** 64, (n_create, 2), dtype=np.uint64)
        ops["now"][at] = start + np.arange(n_create)
    ops["new_end"] = np.where(np.isin(ops["kind"], (pie.TURN_TOUCH, pie.TURN_CREATE)), ops["now"] + TTL, 0)
    return ops, rng.integers(0, users, k).astype(np.int32), rng.integers(0, D, k).astype(np.int32)


def stats_of(times):
    return {"median_ms": float(np.median(times)), "p90_ms": float(np.percentile(times, 90))}


class Clock:
    def __init__(self, start):
        self.start = start

    def take(self, k):
        at = self.start
        self.start += k + 1
        return at


def queries(clock):
    return [(clock - 977 * q - (q % 5) * HOUR, clock - (61 + q % 4) * DAY, (0x55555555, 0xAAAAAAAA, 0xFFFFFFFF)[q % 3]) for q in range(16)]


def timed_turns(ctx, rng, pool, clock, users, starts, k, n_create, steps, call=None):
    times = []
    for rep in range(steps + 3):
        ops, u, d = make_turn(rng, pool, k, clock, n_create, users, starts.take(n_create))
        t0 = time.perf_counter()
        (call or (lambda o, uu, dd: ctx.session_turn(o, uu, dd, users)))(ops, u, d)
        dt = time.perf_counter() - t0
        if rep >= 3:
            times.append(dt * 1e3)
    print("timed %d turns of %d ops, %d creates" % (steps, k, n_create), file=sys.stderr, flush=True)
    return stats_of(times)


def existing_leg(lib_path, n, users, chunk, steps):
    """the existing paths with the switch off, on a table with a run (mode 2, built by one scan)"""
    rng = np.random.default_rng(1)
    out = {}
    with open_ctx(lib_path) as ctx:
        clock, pool, start = load_table(ctx, rng, n, users, chunk, 2)
        starts = Clock(start)
        ctx.set_disciplines(0x55555555, D)
        for k in SIZES:
            out["token_turn_%d" % k] = timed_turns(ctx, rng, pool, clock, users, starts, k, 0, steps, lambda o, u, d: ctx.token_turn(o))
        for k in SIZES:
            out["create_turn_%d" % k] = timed_turns(ctx, rng, pool, clock, users, starts, k, max(1, round(0.05 * k)), steps)
        times = []
        for rep in range(steps + 3):
            ctx.scan(clock, clock - 61 * DAY)                 # mode 2: the run is valid before every timed append
            at = starts.take(1000)
            cols = (at + np.arange(1000), at + np.arange(1000) + TTL, rng.integers(0, users, 1000).astype(np.int32),
                    rng.integers(0, D, 1000).astype(np.int32))
            keys = rng.integers(0, 2 ** 64, (1000, 2), dtype=np.uint64)
            t0 = time.perf_counter()
            ctx.append_rows(*cols, users)
            dt = time.perf_counter() - t0
            ctx.token_append(keys)
            if rep >= 3:
                times.append(dt * 1e3)
        out["append_rows_1000_on_a_run"] = stats_of(times)
        out["ordered_rows_after"] = int(ctx.table_info()["ordered_rows"])
    return out


def mixed_legs(n, users, chunk, steps):
    legs = {}
    ctxs = {}
    try:
        for name, on in (("on", 1), ("off", 0)):
            rng = np.random.default_rng(1)
            ctx = open_ctx(build.HIP_LIB)
            ctx.set_turn_ordered(on)
            clock, pool, start = load_table(ctx, rng, n, users, chunk, 2)
            ctx.set_disciplines(0xFFFFFFFF, D)
            ctx.scan_batch(queries(clock))                    # builds the run
            ctxs[name] = (ctx, rng, clock, pool, Clock(start))
            legs[name] = {"times": [], "batches_on_run": 0, "ordered_builds_before": int(ctx.table_info()["ordered_builds"])}
        for step in range(steps + 3):
            for name in ("on", "off"):
                ctx, rng, clock, pool, starts = ctxs[name]
                ops, u, d = make_turn(rng, pool, 64, clock, 3, users, starts.take(3))
                qs = queries(clock)
                t0 = time.perf_counter()
                ctx.session_turn(ops, u, d, users)
                ctx.scan_batch(qs)
                dt = time.perf_counter() - t0
                if step >= 3:
                    legs[name]["times"].append(dt * 1e3)
                    legs[name]["batches_on_run"] += int(bool(ctx.stats()["k1_variant"] & 0x2000))
        for name in ("on", "off"):
            ti = ctxs[name][0].table_info()
            leg = legs[name]
            leg.update(stats_of(leg.pop("times")))
            leg.update({"ordered_builds": int(ti["ordered_builds"]), "ordered_respreads": int(ti["ordered_respreads"]),
                        "ordered_rows": int(ti["ordered_rows"]), "rows": int(ti["rows"]), "ordered_build_ms": float(ti["ordered_build_ms"])})
    finally:
        for ctx, *_ in ctxs.values():
            ctx.close()
    return legs


def keep_cost(n, users, chunk, steps):
    out = {}
    for name, mode in (("run_kept", 2), ("mode_0", 0)):
        rng = np.random.default_rng(1)
        with open_ctx(build.HIP_LIB) as ctx:
            ctx.set_turn_ordered(1)
            clock, pool, start = load_table(ctx, rng, n, users, chunk, mode)
            starts = Clock(start)
            ctx.set_disciplines(0x55555555, D)
            ctx.scan(clock, clock - 61 * DAY)
            for k in (64, 4096):
                rec = timed_turns(ctx, rng, pool, clock, users, starts, k, max(1, round(0.05 * k)), steps)
                ti = ctx.table_info()
                rec.update({"ordered_rows": int(ti["ordered_rows"]), "ordered_builds": int(ti["ordered_builds"]),
                            "ordered_respreads": int(ti["ordered_respreads"])})
                out["%s_%d" % (name, k)] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--existing-of", default=None, help="internal: measure the existing paths of this library file and print them")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "session_turn_ordered_probe.json"))
    a = ap.parse_args()
    n, users = a.rows, max(1, a.rows // 1000)
    if a.existing_of:
        print("EXISTING " + json.dumps(existing_leg(a.existing_of, n, users, a.chunk, a.steps)))
        return
    out = {"rows": n, "users": users, "steps": a.steps, "corpus": "Zipf(1.1)", "ordered_mode": 2}

    def save():                                   # after every section: a run that is cut short leaves what it had measured
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    def child(lib):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", str(n), "--chunk", str(a.chunk), "--steps", str(a.steps),
                              "--existing-of", lib], stdout=subprocess.PIPE, text=True, check=True)
        return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("EXISTING ")][-1][9:])

    out["existing"] = {"this": child(build.HIP_LIB)}
    print("existing, this library:", out["existing"]["this"], flush=True)
    save()
    if a.baseline_lib:
        base = child(a.baseline_lib)
        out["existing"]["baseline"] = base
        out["existing"]["within_baseline_p90"] = {k: out["existing"]["this"][k]["median_ms"] <= base[k]["p90_ms"]
                                                   for k in base if isinstance(base[k], dict)}
        print("existing, baseline:", base, flush=True)
        save()
    out["mixed"] = mixed_legs(n, users, a.chunk, a.steps)
    print("mixed:", out["mixed"], flush=True)
    save()
    out["keep_cost"] = keep_cost(n, users, a.chunk, a.steps)
    print("keep_cost:", out["keep_cost"], flush=True)
    save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
