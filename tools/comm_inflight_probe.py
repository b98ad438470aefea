#!/usr/bin/env python3
"""What do getSession by token and the purge tick cost a SHARDED server that keeps its pipelined steps in flight?  cfg3 (10^8
sessions / 10^5 users / 32 disciplines) as a world-8 communicator on ONE GPU (the RCCL stand-in tests/stub_rccl.c: the eight shards
share one MI355X — nothing here ever ran across GPUs), batch lanes pinned to 3, nine 32-query ordinary steps begun and unfinished.
For lookups of 1 and 4 096 keys and for a one-hour expired window, in the same run:
  in_flight   wall time of pie_comm_token_lookup_begin -> _finish / pie_comm_expired_queue_begin -> _finish with the nine steps in
              flight (before every timed sample the oldest step is finished, the one before it collected and a new one begun,
              untimed): median and 90th percentile
  drained     the same answer with the calls the parent commit has: finish and collect every step, pie_comm_token_lookup /
              pie_comm_expired_queue, begin nine steps again
  steps       ms per step of the step loop (finish, collect, begin) with no tick, and with one expired-queue tick begun every
              --every steps and finished right before the next is begun
-> profiles/comm_inflight_probe.json (--out)"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
stub_dir = os.path.join(REPO, "tests", "_stub")
os.makedirs(stub_dir, exist_ok=True)
stub = os.path.join(stub_dir, "libstub_rccl_inflight_probe.so")
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                "-L/opt/rocm/lib", "-lamdhip64"], check=True)
os.environ["PIE_RCCL_LIB"] = stub

import numpy as np  # noqa: E402
import torch  # noqa: F401,E402  (before libpie_hip.so initialises HIP)
import sph_pie_amd as pie  # noqa: E402

SEED, D = 0x5EED5EED, 32
T0_MS, DAY, HOUR = 1700000000000, 86400 * 1000, 3600 * 1000
IN_FLIGHT, NQ = 9, 32


def stats(times):
    t = np.asarray(times)
    return {"median_ms": float(np.median(t)), "p90_ms": float(np.percentile(t, 90)), "min_ms": float(t.min()), "max_ms": float(t.max()),
            "n": int(t.size)}


def samples(fn, before, reps):
    times = []
    for _ in range(reps + 1):   # the first is a warm-up
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--users", type=int, default=10 ** 5)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--reps", type=int, default=100, help="timed in-flight samples per case")
    ap.add_argument("--drained-reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--every", type=int, default=8, help="steps of the step loop per tick begun")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "comm_inflight_probe.json"))
    a = ap.parse_args()
    n, users, world = a.rows, a.users, a.world
    now, cutoff, mask = T0_MS - 6 * HOUR, T0_MS - 61 * DAY, 0x55555555
    prev = now - HOUR
    queries = [(now - 977 * q, cutoff, mask) for q in range(NQ)]
    out = {"rows": n, "users": users, "disciplines": D, "world": world, "lanes": 3, "queries_per_step": NQ, "steps_in_flight": IN_FLIGHT,
           "window_ms": HOUR, "steps_per_tick": a.every,
           "setup": "one MI355X, %d shards on it, RCCL stand-in (never across GPUs); wall times through the Python binding" % world}
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 2 ** 64, (n, 2), dtype=np.uint64)
    comm = pie.PieComm([0] * world)
    comm.gen_synthetic_sharded(SEED, n, users, D, 0)
    for r in range(world):
        c = comm.ctx(r)
        c.set_batch_lanes(3)
        c.set_disciplines(mask, D)
    comm.token_set(keys)
    # the union capacity the steps need: one step with too little says it at its collect
    comm.step_reserve(NQ, 0, 1 << 16)
    comm.step_begin(queries)
    comm.step_finish()
    try:
        comm.step_collect()
    except pie.PieError as e:
        if e.code != pie.binding.PIE_E_CAPACITY:
            raise
        comm.step_reserve(NQ, 0, comm.needed_cap())
    out["union_cap"] = max(comm.needed_cap(), 1 << 16)
    state = {"begun": 0, "finished": 0, "collected": 0}

    def begin():
        comm.step_begin(queries)
        state["begun"] += 1

    def fill():
        while state["begun"] - state["finished"] < IN_FLIGHT:
            begin()

    def drain():
        while state["finished"] < state["begun"]:
            comm.step_finish()
            state["finished"] += 1
        while state["collected"] < state["finished"]:
            comm.step_collect()
            state["collected"] += 1

    def turn():   # finish the oldest, collect the one finished the turn before, begin a new one
        comm.step_finish()
        state["finished"] += 1
        if state["finished"] - state["collected"] > 1:
            comm.step_collect()
            state["collected"] += 1
        begin()

    want_q = comm.expired_queue(prev, now)
    cap = int(want_q.size) + 4096
    out["queue_rows"] = int(want_q.size)
    cases = []
    for k in (1, 4096):
        ask = keys[rng.integers(0, n, k)]
        want = comm.token_lookup(ask, now)

        def lookup(ask=ask):
            comm.token_lookup_begin(ask, now)
            return comm.token_lookup_finish()

        def lookup_drained(ask=ask):
            drain()
            comm.token_lookup(ask, now)
            fill()
        cases.append(("token_lookup_%d" % k, lookup, lookup_drained, lambda got, want=want: all(np.array_equal(got[c], want[c]) for c in want)))

    def tick():
        comm.expired_queue_begin(prev, now, cap)
        return comm.expired_queue_finish()

    def tick_drained():
        drain()
        comm.expired_queue(prev, now)
        fill()
    cases.append(("expired_queue_1h", tick, tick_drained, lambda got: np.array_equal(got[0], want_q)))

    fill()
    for name, fn, fn_drained, same in cases:
        assert same(fn()), name + ": the in-flight answer differs from the synchronous one"
        rec = {"in_flight": stats(samples(fn, turn, a.reps)), "drained": stats(samples(fn_drained, None, a.drained_reps))}
        rec["drained_over_in_flight"] = rec["drained"]["median_ms"] / rec["in_flight"]["median_ms"]
        out[name] = rec
        print(name, json.dumps(rec), flush=True)
    # the step loop without and with ticks
    steps = {}
    for name, every in (("step_ms", 0), ("step_with_ticks_ms", a.every)):
        runs = []
        for _ in range(3):
            turn()
            begun = False
            t0 = time.perf_counter()
            for i in range(a.steps):
                turn()
                if every and i % every == 0:
                    if begun:
                        comm.expired_queue_finish()
                    comm.expired_queue_begin(prev, now, cap)
                    begun = True
            runs.append((time.perf_counter() - t0) * 1e3 / a.steps)
            if begun:
                comm.expired_queue_finish()
        steps[name] = float(np.median(runs))
        steps[name + "_runs"] = runs
    steps["ratio"] = steps["step_with_ticks_ms"] / steps["step_ms"]
    out["steps"] = steps
    print("steps", json.dumps(steps), flush=True)
    drain()
    comm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
