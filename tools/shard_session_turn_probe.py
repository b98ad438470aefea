#!/usr/bin/env python3
"""What does a turn that logs in cost on a sharded table behind the communicator (pie_comm_session_turn), beside what a caller did
before it, and did the existing path get slower?

cfg3 (10^8 generated rows, 10^5 users; every row gets a random key) split into eight shards of one communicator on ONE GPU (the
RCCL stand-in tests/stub_rccl.c, as tools/shard_token_probe.py sets it up).  Host wall time through the Python binding, median and
90th percentile over --reps calls, of

  session      comm.session_turn(ops, user, disc, users): per shard one upload, one kernel, one download, one wait
  three_calls  the same ops the way a caller made them before: pie_comm_append_rows of the turn's creates, pie_comm_token_append of
               their keys, then pie_comm_token_turn of the other ops.  The split is done ahead of the clock.

for turns of 1, 64 and 4 096 ops of which max(1, round(5 % of k)) are creates at random places (k = 1 is a login alone); the other
ops are 80 % get, 15 % touch, 5 % delete on distinct live sessions.  Creates are made before anything is timed until every shard
has grown once: the generated shards are exactly full, and the first append a shard keeps doubles its capacity.

Then the bar of the existing path, on create-free lists of the same mix:
  token_turn            comm.token_turn(ops) of this library
  session_no_create     comm.session_turn(ops) of this library
  baseline_token_turn   comm.token_turn(ops) of the library given with --baseline-lib (the parent commit's, built beside this one):
                        a fresh child process of this tool, started before this process opens the GPU, loads it (PIE_HIP_LIB)
                        and measures on a table of its own generated the same way
The bar holds when each median stays within the baseline's own 90th percentile.  Two ways that are compared within one process
(session against three_calls, token_turn against session_no_create) are timed in alternation, call by call; each process makes
one whole create-free pass before the pass it records.

usage: shard_session_turn_probe.py [--rows N] [--world W] [--reps R] [--baseline-lib FILE] [--out FILE]
       -> profiles/shard_session_turn_probe.json"""
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
stub_dir = os.path.join(REPO, "tests", "_stub")
os.makedirs(stub_dir, exist_ok=True)
stub = os.path.join(stub_dir, "libstub_rccl_session_turn_probe.so")
if not os.environ.get("PIE_RCCL_LIB"):
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                    "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    os.environ["PIE_RCCL_LIB"] = stub

SEED, D = 0x5EED5EED, 32
TTL = 12 * 3600 * 1000
END_NONE = -(2 ** 63)
MIX = (0.80, 0.15, 0.05)
CREATE_SHARE = 0.05
SIZES = (1, 64, 4096)


def open_library():
    """the library PIE_HIP_LIB names (default: this tree's); an older one lacks the newest entry points, which are left untyped"""
    import torch  # noqa: F401  (before libpie_hip.so initialises HIP)
    import sph_pie_amd as pie
    from sph_pie_amd import binding, build
    have = ctypes.CDLL(os.environ.get("PIE_HIP_LIB") or build.HIP_LIB)
    binding._SIGS = [s for s in binding._SIGS if hasattr(have, s[0])]
    binding.load_library()
    return pie


def load_table(pie, rng, n, users, world, chunk):
    """the generated table in `world` shards with a random key per row -> (comm, clock at which half the sessions are live, keys of
    live sessions)"""
    comm = pie.PieComm([0] * world)
    comm.gen_synthetic_sharded(SEED, n, users, D, 0)
    sample = []
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        keys = rng.integers(0, 2 ** 64, (hi - lo, 2), dtype=np.uint64)
        (comm.token_set if lo == 0 else comm.token_append)(keys)
        sample.append(keys[rng.integers(0, hi - lo, min(hi - lo, 1 + (1 << 21) * chunk // n))])
    sample = np.concatenate(sample)
    got = comm.token_lookup(sample, END_NONE)
    assert np.all(got["row"] >= 0), "a key did not find its row"
    clock = int(np.median(got["end"]))
    return comm, clock, sample[got["end"] > clock + 8]


def make_turn(pie, rng, pool, k, clock, n_create, users):
    ops = np.zeros(k, pie.TURN_OP)
    ops["tok"] = pool[rng.choice(pool.shape[0], k, replace=False)]
    ops["now"] = clock
    ops["kind"] = rng.choice([pie.TURN_GET, pie.TURN_TOUCH, pie.TURN_DELETE], k, p=MIX)
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


def timed_pair(reps, make_a, run_a, make_b, run_b):
    """two ways measured in alternation, call by call, so that neither has the later (warmer) half of the run to itself"""
    ta, tb = [], []
    for rep in range(reps + 3):                  # three warm-up calls each
        for make, run, times in ((make_a, run_a, ta), (make_b, run_b, tb)):
            args = make()
            t0 = time.perf_counter()
            run(*args)
            dt = time.perf_counter() - t0
            if rep >= 3:
                times.append(dt * 1e3)
    return (float(np.median(ta)), float(np.percentile(ta, 90))), (float(np.median(tb)), float(np.percentile(tb, 90)))


def plain_series(pie, rng, pool, clock, users, reps, call, also=None):
    """create-free lists of every size through `call` (and, in alternation, through `also`).  One whole pass is made and thrown
    away first: the first few hundred turns of a process are slower than the rest (staging blocks grow, the table's pages are
    touched for the first time), and the baseline's process and this one must both be measured past that."""
    make = lambda k: (lambda: (make_turn(pie, rng, pool, k, clock, 0, users)[0],))
    for k in SIZES:
        timed(reps, make(k), call)
    if also is None:
        return {k: timed(reps, make(k), call) for k in SIZES}
    pairs = {k: timed_pair(reps, make(k), call, make(k), also) for k in SIZES}
    return {k: v[0] for k, v in pairs.items()}, {k: v[1] for k, v in pairs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--baseline-child", action="store_true", help="internal: measure comm.token_turn alone and print one JSON line")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shard_session_turn_probe.json"))
    a = ap.parse_args()
    n, users, world = a.rows, max(1, a.rows // 1000), a.world
    baseline = None
    if a.baseline_lib:                           # before this process opens the GPU: one process at a time holds the tables
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-child", "--rows", str(n), "--world", str(world),
                                "--chunk", str(a.chunk), "--reps", str(a.reps)], env=dict(os.environ, PIE_HIP_LIB=os.path.abspath(a.baseline_lib)),
                               stdout=subprocess.PIPE, text=True, check=True)
        baseline = {int(k): v for k, v in json.loads(child.stdout.strip().splitlines()[-1]).items()}
        print("baseline library measured:", baseline, flush=True)
    pie = open_library()
    rng = np.random.default_rng(1)
    comm, clock, pool = load_table(pie, rng, n, users, world, a.chunk)
    if a.baseline_child:
        print(json.dumps(plain_series(pie, rng, pool, clock, users, a.reps, comm.token_turn)), flush=True)
        comm.close()
        return
    out = {"rows": n, "users": users, "world": world, "reps": a.reps, "create_share": CREATE_SHARE, "mix_get_touch_delete": MIX,
           "setup": "one MI355X, %d shards on it, RCCL stand-in; wall times through the Python binding, ms" % world,
           "clock": clock, "pool": int(pool.shape[0]), "series": [], "existing_path": []}
    print("table and keys ready: %d live sessions to draw from" % pool.shape[0], flush=True)
    ours, no_create = plain_series(pie, rng, pool, clock, users, a.reps, comm.token_turn, lambda ops: comm.session_turn(ops, None, None, users))
    for k in SIZES:
        rec = {"k": k, "mix": "80_15_5_0", "token_turn_median_ms": ours[k][0], "token_turn_p90_ms": ours[k][1],
               "session_no_create_median_ms": no_create[k][0], "session_no_create_p90_ms": no_create[k][1]}
        if baseline:
            rec.update({"baseline_token_turn_median_ms": baseline[k][0], "baseline_token_turn_p90_ms": baseline[k][1],
                        "token_turn_within_baseline_p90": ours[k][0] <= baseline[k][1],
                        "session_no_create_within_baseline_p90": no_create[k][0] <= baseline[k][1]})
        out["existing_path"].append(rec)
        print(rec, flush=True)
    # every shard grows once, ahead of the clock: 64 creates at a time until each shard has kept one
    t0 = time.perf_counter()
    rows0 = [comm.ctx(r).table_info()["rows"] for r in range(world)]
    for _ in range(8):
        comm.session_turn(*make_turn(pie, rng, pool, 64, clock, 64, users), users)
        if all(comm.ctx(r).table_info()["rows"] > rows0[r] for r in range(world)):
            break
    out["first_creates_ms"] = (time.perf_counter() - t0) * 1e3

    def three_calls(creates, keys, rest):
        comm.append_rows(*creates, users)
        comm.token_append(keys)
        if rest.shape[0]:
            comm.token_turn(rest)

    def split(ops, user, disc):
        c = ops["kind"] == pie.TURN_CREATE
        cols = [np.ascontiguousarray(x) for x in (ops["now"][c], ops["new_end"][c], user[c], disc[c])]
        return cols, np.ascontiguousarray(ops["tok"][c]), np.ascontiguousarray(ops[~c])

    for k in SIZES:
        n_create = max(1, int(round(CREATE_SHARE * k)))
        rec = {"k": k, "mix": "76_14_5_5" if k > 1 else "a login alone", "creates": n_create}
        (rec["session_median_ms"], rec["session_p90_ms"]), (rec["three_calls_median_ms"], rec["three_calls_p90_ms"]) = timed_pair(
            a.reps, lambda: make_turn(pie, rng, pool, k, clock, n_create, users), lambda ops, u, d: comm.session_turn(ops, u, d, users),
            lambda: split(*make_turn(pie, rng, pool, k, clock, n_create, users)), three_calls)
        rec["three_calls_over_session"] = rec["three_calls_median_ms"] / rec["session_median_ms"]
        out["series"].append(rec)
        print(rec, flush=True)
    out["rows_after"] = comm.table_size()[0]
    out["token_builds"] = [int(comm.ctx(r).table_info()["token_builds"]) for r in range(world)]
    comm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
