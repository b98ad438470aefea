#!/usr/bin/env python3
"""What does the purge tick cost a process that keeps the batch pipeline full?  At the benchmark's configuration (10^8 rows, 10^5
users, 64-query batches, lanes pinned to 3, nine batches in flight) and a one-hour window, for every grid size tried
(PIE_EXPQ_BLOCKS_PER_CU, a context each):
  1. wall time of pie_expired_queue_begin -> _finish with nine batches in flight (before every timed tick the oldest batch is
     finished and a new one begun, untimed): median and 90th percentile over --ticks ticks; the same for the FIRST tick after a
     burst of --burst batch steps (the 200 MB key column has left the Infinity Cache by then); and what the drained way needs
     for the same answer: flush, finish all nine, pie_expired_queue, begin nine again (--drained-only times this alone: it uses
     none of the new calls);
  2. ms per step of the batch loop (one finish and one begin per step) with no tick begun, and with one tick begun every
     --every steps and finished right before the next one is begun: the ratio is what the pass costs the lanes;
  3. pie_table_info.expired_inflight_ms (device time of the pass, events on its own stream) on an idle chip, beside the wall
     time of the in-flight pair and of pie_expired_queue there.
-> profiles/expired_inflight_probe.json (--out)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import sph_pie_amd as pie  # noqa: E402

SEED, D = 0x5EED5EED, 32
T0_MS, DAY, HOUR = 1700000000000, 86400 * 1000, 3600 * 1000


def stats(times):
    t = np.asarray(times)
    return {"median_ms": float(np.median(t)), "p90_ms": float(np.percentile(t, 90)), "max_ms": float(t.max()), "n": int(t.size)}


def probe_grid(a, per_cu):
    n, users = a.rows, max(1, a.rows // 1000)
    now, cutoff, mask = T0_MS - 6 * HOUR, T0_MS - 61 * DAY, 0x55555555
    prev = now - HOUR
    queries = [(now - 977 * q, cutoff, mask) for q in range(64)]
    if per_cu is not None:
        os.environ["PIE_EXPQ_BLOCKS_PER_CU"] = str(per_cu)
    rec = {"blocks_per_cu": per_cu}
    with pie.PieScan(0) as ctx:
        ctx.set_batch_lanes(3)
        ctx.gen_synthetic(SEED, n, 0, n, users, D, 0)
        ctx.set_disciplines(mask, D)
        ctx.scan_batch_pipelined(10, queries)
        want = ctx.expired_queue(prev, now)
        cap = int(want.size) + 4096
        buf, q_len = np.empty(cap, np.int32), C.c_size_t(0)

        def synchronous():   # pie_expired_queue into a buffer of the same size as the in-flight pair's
            ctx._check(ctx._lib.pie_expired_queue(ctx._ctx, prev, now, buf.ctypes.data_as(C.c_void_p), cap, C.byref(q_len)))
        rec["queue_rows"] = int(want.size)

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

        def burst():
            for _ in range(a.burst):
                turn()

        def samples(fn, before, reps):
            times = []
            for _ in range(reps + 1):
                if before:
                    before()
                t0 = time.perf_counter()
                fn()
                times.append((time.perf_counter() - t0) * 1e3)
            return times[1:]

        def drained():
            drain()
            synchronous()
            fill()

        if a.drained_only:
            fill()
            rec["drain_queue_refill_wall"] = stats(samples(drained, None, max(a.ticks // 4, 10)))
            drain()
            return rec
        rec["geometry"] = dict(zip(("rows_per_wave_step", "rows_per_unit", "blocks"), ctx.expired_inflight_geometry(n)))

        def tick():
            ctx.expired_queue_begin(prev, now, cap)
            return ctx.expired_queue_finish()

        # 3. an idle chip
        assert np.array_equal(tick(), want), "the in-flight queue differs from pie_expired_queue"
        dev = []
        for _ in range(30):
            tick()
            dev.append(ctx.table_info()["expired_inflight_ms"])
        rec["idle_device_ms"] = stats(dev)
        rec["idle_pair_wall"] = stats(samples(tick, None, 30))
        rec["idle_synchronous_wall"] = stats(samples(synchronous, None, 30))
        # 1. nine batches in flight
        fill()
        assert ctx.batch_room() == 0
        assert np.array_equal(tick(), want), "the in-flight queue differs with nine batches in flight"
        rec["nine_in_flight_wall"] = stats(samples(tick, turn, a.ticks))
        rec["nine_in_flight_device_ms"] = float(ctx.table_info()["expired_inflight_ms"])
        rec["first_after_burst_wall"] = stats(samples(tick, burst, max(a.ticks // 10, 10)))
        rec["drain_queue_refill_wall"] = stats(samples(drained, None, max(a.ticks // 4, 10)))
        # 2. the batch loop, without and with ticks
        for name, every in (("step_ms", 0), ("step_with_ticks_ms", a.every)):
            runs = []
            for _ in range(5):
                turn()
                begun = False
                t0 = time.perf_counter()
                for i in range(a.steps):
                    turn()
                    if every and i % every == 0:
                        if begun:
                            ctx.expired_queue_finish()
                        ctx.expired_queue_begin(prev, now, cap)
                        begun = True
                runs.append((time.perf_counter() - t0) * 1e3 / a.steps)
                if begun:
                    ctx.expired_queue_finish()
            rec[name] = float(np.median(runs))
        rec["step_ratio"] = rec["step_with_ticks_ms"] / rec["step_ms"]
        drain()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--every", type=int, default=8, help="steps of the batch loop per tick begun")
    ap.add_argument("--burst", type=int, default=60, help="batch steps ahead of a first-tick sample")
    ap.add_argument("--grids", default="1,2,4,8", help="PIE_EXPQ_BLOCKS_PER_CU values to try")
    ap.add_argument("--drained-only", action="store_true", help="time the drained way alone (runs on a build without the in-flight calls)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "expired_inflight_probe.json"))
    a = ap.parse_args()
    out = {"rows": a.rows, "users": max(1, a.rows // 1000), "lanes": 3, "queries_per_batch": 64, "batches_in_flight": 9, "window_ms": HOUR,
           "ticks": a.ticks, "steps": a.steps, "steps_per_tick": a.every, "burst_steps": a.burst, "grids": []}
    for g in ([None] if a.drained_only else [int(x) for x in a.grids.split(",")]):
        rec = probe_grid(a, g)
        out["grids"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
