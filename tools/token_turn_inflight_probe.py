#!/usr/bin/env python3
"""What does a token turn cost while the batch pipeline is full (pie_token_turn_begin / _finish)?  At the benchmark's
configuration (10^8 rows, 10^5 users, 64-query batches, lanes pinned to 3, nine batches in flight; keys are random words, the
device never hashes).  A turn of k ops is 80 % get / 15 % touch / 5 % delete on keys of the table; touches move a row's `end`
inside the cold range (clock below every end, new end 30 to 60 days before the queries' clocks), so the hot index the batches read
keeps its shape over the run.  Wall times, median and 90th percentile, for k = 1, 64 and 4 096:
  (a) begin -> finish with nothing in flight;
  (b) begin -> finish with nine batches in flight (before every timed turn the oldest batch is finished and a new one begun,
      untimed, so the lanes stay busy);
  (c) the drained way, the only one without these calls: flush, finish all nine, pie_token_turn, begin nine again;
  (d) the batch step (nine in flight, one finish and one begin per step) with no turns, and with one turn of k ops begun every
      8 steps and finished 4 steps later: the fence stalls the lanes for the length of the turn's kernel.
usage: token_turn_inflight_probe.py [--rows N] [--reps R] [--out FILE]   -> profiles/token_turn_inflight_probe.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import sph_pie_amd as pie  # noqa: E402
from sph_pie_amd.binding import turn_ops  # noqa: E402

SEED, D = 0x5EED5EED, 32
T0_MS, DAY = 1700000000000, 86400 * 1000
GET, TOUCH, DELETE = 0, 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "token_turn_inflight_probe.json"))
    a = ap.parse_args()
    n, users = a.rows, max(1, a.rows // 1000)
    now, cutoff, mask = T0_MS - 6 * 3600 * 1000, T0_MS - 61 * DAY, 0x55555555
    queries = [(now - 977 * q, cutoff, mask) for q in range(64)]
    out = {"rows": n, "users": users, "lanes": 3, "queries_per_batch": 64, "batches_in_flight": 9, "reps": a.reps, "steps": a.steps,
           "mix": {"get": 0.80, "touch": 0.15, "delete": 0.05}, "turns": []}
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
            sample.append(keys[rng.integers(0, hi - lo, min(hi - lo, 1 + 65536 * a.chunk // n))])
        ctx.synchronize()
        sample = np.concatenate(sample)
        ctx.scan_batch_pipelined(10, queries)
        out["hot_rows"] = int(ctx.table_info()["hot_rows"])

        def ops_of(k):
            kinds = rng.choice([GET, TOUCH, DELETE], k, p=[0.80, 0.15, 0.05]).astype(np.int32)
            keys = sample[rng.integers(0, sample.shape[0], k)]
            new_end = np.where(kinds == TOUCH, T0_MS - 30 * DAY - rng.integers(0, 30 * DAY, k), 0).astype(np.int64)
            clock = np.where(kinds == TOUCH, -(2 ** 62), T0_MS).astype(np.int64)
            return turn_ops(keys=keys, now=clock, new_end=new_end, kind=kinds)

        def fill():
            while ctx.batch_room() > 0:
                ctx.scan_batch_begin(queries)

        def drain():
            ctx.scan_batch_flush()
            while ctx.batch_room() < 9:
                ctx.scan_batch_finish(want_m=False)

        def step():
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

        def stat(rec, name, t):
            rec[name + "_median_ms"], rec[name + "_p90_ms"] = float(np.median(t)), float(np.percentile(t, 90))

        def step_loop(k):
            """per-step wall time of the batch loop; k > 0: one turn of k ops begun every 8 steps, finished 4 steps later"""
            step()
            times = []
            for i in range(a.steps):
                t0 = time.perf_counter()
                step()
                if k and i % 8 == 0:
                    ctx.token_turn_begin(ops_of_k[k])
                if k and i % 8 == 4:
                    ctx.token_turn_finish()
                times.append((time.perf_counter() - t0) * 1e3)
            while ctx.token_turn_room() < 4:
                ctx.token_turn_finish()
            return np.array(times)

        ops_of_k = {k: ops_of(k) for k in (1, 64, 4096)}
        fill()
        stat(out, "d_step_no_turns", step_loop(0))
        drain()
        for k in (1, 64, 4096):
            ops = ops_of_k[k]
            rec = {"k": k}

            def in_flight():
                ctx.token_turn_begin(ops)
                return ctx.token_turn_finish()

            stat(rec, "a_idle", samples(in_flight, reps=3 * a.reps))
            fill()
            assert ctx.batch_room() == 0
            stat(rec, "b_nine_in_flight", samples(in_flight, before=step, reps=3 * a.reps))

            def drained():
                drain()
                ctx.token_turn(ops)
                fill()

            stat(rec, "c_drain_turn_refill", samples(drained, reps=max(a.reps // 2, 5)))
            stat(rec, "d_step_turn_every_8", step_loop(k))
            drain()
            out["turns"].append(rec)
            print(rec, flush=True)
        out["hot_rows_after"] = int(ctx.table_info()["hot_rows"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
