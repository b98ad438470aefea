#!/usr/bin/env python3
"""What does the token index cost?  On a generated table (pie_gen_synthetic; default 10^8 rows) every row gets the key
token_key(str(row)), uploaded in chunks through token_set then token_append.  Reported: the device time of the last index build
and of a full rebuild (token_build_ms), token_bytes, and for k = 1, 64, 4 096 and 65 536 the host wall time of pie_token_lookup
for all-hit and all-miss batches (median of 20) beside pie_fetch_rows of the same k from the same run: the per-request device
round trip a host pays today once it knows the row.  Wall times include the one wait of the call; the device time of a lookup is
not separated from it here.

usage: token_probe.py [--rows N] [--chunk K]      -> profiles/token_probe.json
       token_probe.py --inflight [--rows N] [--reps R] [--out FILE]   -> profiles/token_inflight_probe.json (see inflight())"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import sph_pie_amd as pie  # noqa: E402

SEED, D = 0x5EED5EED, 32
NOW = 1700000000000


def keys_of_rows(lo, hi, salt=b""):
    """token_key(salt + str(row)) for rows [lo, hi) as a (hi - lo, 2) uint64 array (the rule of binding.token_key, in bulk)."""
    buf = bytearray(16 * (hi - lo))
    for i, row in enumerate(range(lo, hi)):
        buf[16 * i : 16 * i + 16] = hashlib.sha256(salt + str(row).encode()).digest()[:16]
    return np.frombuffer(bytes(buf), dtype="<u8").reshape(-1, 2).astype(np.uint64)


def median_ms(fn, reps=20):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def inflight(a):
    """--inflight: what a token lookup costs while the batch pipeline is full (pie_token_lookup_begin / _finish), at the
    benchmark's configuration (10^8 rows, 10^5 users, 64-query batches, lanes pinned to 3).  Keys are random words (the device
    never hashes).  Wall times, for k = 1, 64 and 4096 keys:
      (a) begin + finish with nothing in flight;
      (b) the same with nine batches in flight (before every timed lookup the oldest batch is finished and a new one begun,
          untimed, so the lanes stay busy);
      (c) the per-step cost of the batch loop (nine in flight, one finish and one begin per step) without and with one lookup
          per step;
      (d) the drained way, the only one without these calls: flush, finish all nine, pie_token_lookup, begin nine again.
    -> profiles/token_inflight_probe.json (--out)"""
    n, users = a.rows, max(1, a.rows // 1000)
    t0_ms, day = 1700000000000, 86400 * 1000
    now, cutoff, mask = t0_ms - 6 * 3600 * 1000, t0_ms - 61 * day, 0x55555555
    queries = [(now - 977 * q, cutoff, mask) for q in range(64)]
    out = {"rows": n, "users": users, "lanes": 3, "queries_per_batch": 64, "batches_in_flight": 9, "reps": a.reps, "lookups": []}
    rng = np.random.default_rng(1)
    with pie.PieScan(0) as ctx:
        ctx.set_batch_lanes(3)
        ctx.gen_synthetic(SEED, n, 0, n, users, D, 0)
        ctx.set_disciplines(mask, D)
        sample = []
        for lo in range(0, n, a.chunk):
            hi = min(n, lo + a.chunk)
            keys = rng.integers(0, 2 ** 64, (hi - lo, 2), dtype=np.uint64)
            (ctx.token_set if lo == 0 else ctx.token_append)(keys)
            sample.append(keys[rng.integers(0, hi - lo, min(hi - lo, 1 + 8192 * a.chunk // n))])
        ctx.synchronize()
        sample = np.concatenate(sample)
        ctx.scan_batch_pipelined(10, queries)

        def fill():
            while ctx.batch_room() > 0:
                ctx.scan_batch_begin(queries)

        def drain():
            ctx.scan_batch_flush()
            while ctx.batch_room() < 9:
                ctx.scan_batch_finish(want_m=False)

        def turn():
            ctx.scan_batch_finish(want_m=False)
            ctx.scan_batch_begin(queries)

        def samples(fn, before=None, reps=a.reps):
            times = []
            for _ in range(reps + 1):
                if before:
                    before()
                t0 = time.perf_counter()
                fn()
                times.append((time.perf_counter() - t0) * 1e3)
            return np.array(times[1:])

        def timed(fn, before=None, reps=a.reps):
            return float(np.median(samples(fn, before, reps)))

        if a.drained_only:   # form (d) alone: it uses no call of the in-flight pair, so a build without them can run it
            for k in (1, 64, 4096):
                hit = sample[rng.integers(0, sample.shape[0], k)]
                fill()

                def drained():
                    drain()
                    ctx.token_lookup(hit, t0_ms)
                    fill()

                out["lookups"].append({"k": k, "d_drain_lookup_refill_wall_ms": timed(drained, reps=max(a.reps // 2, 5))})
                drain()
                print(out["lookups"][-1], flush=True)
            out["drained_only"] = True

        for k in (() if a.drained_only else (1, 64, 4096)):
            hit = sample[rng.integers(0, sample.shape[0], k)]
            nows = np.full(k, t0_ms, np.int64)

            def lookup():
                ctx.token_lookup_begin(hit, nows)
                return ctx.token_lookup_finish()

            want = ctx.token_lookup(hit, t0_ms)
            assert np.all(want["row"] >= 0)
            idle = samples(lookup, reps=3 * a.reps)
            rec = {"k": k, "a_idle_wall_ms": float(np.median(idle)), "a_p90_wall_ms": float(np.percentile(idle, 90)), "a_max_wall_ms": float(idle.max())}
            fill()
            assert ctx.batch_room() == 0
            got = lookup()
            assert all(np.array_equal(got[c], want[c]) for c in want), "the in-flight lookup differs from the drained one"
            # the new batch of every third sample goes to lane 0, the context's stream, which the lookup is ordered behind:
            # the median hides those, so the upper tail is kept as well
            b = samples(lookup, before=turn, reps=3 * a.reps)
            rec["b_nine_in_flight_wall_ms"] = float(np.median(b))
            rec["b_p90_wall_ms"], rec["b_max_wall_ms"] = float(np.percentile(b, 90)), float(b.max())
            steps = 200
            for name, with_lookup in (("c_step_wall_ms", False), ("c_step_with_lookup_wall_ms", True)):
                turn()
                t0 = time.perf_counter()
                for _ in range(steps):
                    turn()
                    if with_lookup:
                        lookup()
                rec[name] = (time.perf_counter() - t0) * 1e3 / steps

            def drained():
                drain()
                ctx.token_lookup(hit, t0_ms)
                fill()

            rec["d_drain_lookup_refill_wall_ms"] = timed(drained, reps=max(a.reps // 2, 5))
            drain()
            out["lookups"].append(rec)
            print(rec, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--inflight", action="store_true", help="lookups beside a full batch pipeline -> profiles/token_inflight_probe.json")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--drained-only", action="store_true", help="--inflight: time form (d) alone (runs on a build without the in-flight calls)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "token_inflight_probe.json"), help="--inflight: where the result goes")
    a = ap.parse_args()
    if a.inflight:
        return inflight(a)
    n, users = a.rows, max(1, a.rows // 1000)
    out = {"rows": n, "users": users, "chunk": a.chunk, "lookups": []}
    with pie.PieScan(0) as ctx:
        ctx.gen_synthetic(SEED, n, 0, n, users, D, pie.PIE_GEN_TIME_ORDERED)
        assert np.array_equal(pie.token_key("12345"), keys_of_rows(12345, 12346)[0])
        t0 = time.perf_counter()
        rng = np.random.default_rng(1)
        sample_rows, sample_keys = [], []
        for lo in range(0, n, a.chunk):
            hi = min(n, lo + a.chunk)
            keys = keys_of_rows(lo, hi)
            (ctx.token_set if lo == 0 else ctx.token_append)(keys)
            pick = rng.integers(0, hi - lo, min(hi - lo, 1 + 70000 * a.chunk // n))
            sample_rows.append(pick + lo)
            sample_keys.append(keys[pick])
            print("keys for rows [%d, %d): %.0f s" % (lo, hi, time.perf_counter() - t0), flush=True)
        ctx.synchronize()
        out["upload_wall_s"] = time.perf_counter() - t0       # host hashing included
        info = ctx.table_info()
        out.update(token_rows=info["token_rows"], token_bytes=info["token_bytes"], token_builds=info["token_builds"],
                   last_growth_build_ms=info["token_build_ms"])
        out["slots"] = pie.token_slots_for(info["token_rows"])
        sample_rows, sample_keys = np.concatenate(sample_rows), np.concatenate(sample_keys)
        for k in (1, 64, 4096, 65536):
            sel = rng.integers(0, sample_rows.shape[0], k)
            hit, rows = sample_keys[sel], sample_rows[sel].astype(np.int32)
            miss = keys_of_rows(0, k, salt=b"absent-")
            got = ctx.token_lookup(hit, NOW)
            assert np.array_equal(got["row"], rows), "a key did not find its row"
            assert np.all(ctx.token_lookup(miss, NOW)["row"] == -1)
            out["lookups"].append({"k": k, "lookup_hit_wall_ms": median_ms(lambda: ctx.token_lookup(hit, NOW)),
                                   "lookup_miss_wall_ms": median_ms(lambda: ctx.token_lookup(miss, NOW)),
                                   "fetch_rows_wall_ms": median_ms(lambda: ctx.fetch_rows(rows))})
            print(out["lookups"][-1], flush=True)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "token_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
