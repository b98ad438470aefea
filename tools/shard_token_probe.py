#!/usr/bin/env python3
"""What does getSession by token cost on a sharded table?  cfg3 (10^8 sessions / 10^5 users / 32 disciplines) as a world-8
communicator on ONE GPU (the RCCL stand-in tests/stub_rccl.c: the eight shards share one MI355X), beside the unsharded table
with the plain token index in the same process.  Every row gets a random 128-bit key.  Recorded:
  lookups   host wall time (median of 20 after one warm-up) of comm.token_lookup (pie_comm_token_lookup: queued on all eight
            shards, then waited for, merged on the host) and of pie_token_lookup on the unsharded table, for k = 1, 64, 4 096 and
            65 536, all-hit and all-miss, and their ratio.  One launch-and-wait if the shards' queue phases overlap, eight if not.
  build     token_build_ms of every shard after comm.token_set (device time, HIP events around the fill and every chunk), the
            host wall time of the whole comm.token_set, and of pie_token_set on the unsharded table
  plain_lookup_regression   (--token-probe LABEL=FILE ...) results of tools/token_probe.py runs, copied in as they are: two runs
            of the parent build (its run-to-run spread) and one of this build
usage: shard_token_probe.py [--rows N] [--users U] [--world W] [--token-probe LABEL=FILE ...] [--out FILE]
       -> profiles/shard_token_probe.json"""
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
stub = os.path.join(stub_dir, "libstub_rccl_token_probe.so")
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                "-L/opt/rocm/lib", "-lamdhip64"], check=True)
os.environ["PIE_RCCL_LIB"] = stub

import numpy as np  # noqa: E402
import torch  # noqa: F401,E402  (before libpie_hip.so initialises HIP)
import sph_pie_amd as pie  # noqa: E402

SEED, D = 0x5EED5EED, 32
NOW = 1700000000000


def wall_ms(fn, reps=20):
    """(median, min, max) over `reps` calls after one warm-up"""
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--users", type=int, default=10 ** 5)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--token-probe", nargs="*", default=[], metavar="LABEL=FILE")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shard_token_probe.json"))
    a = ap.parse_args()
    n, users, world = a.rows, a.users, a.world
    out = {"rows": n, "users": users, "disciplines": D, "world": world, "reps": 20,
           "setup": "one MI355X, %d shards on it, RCCL stand-in; wall times through the Python binding" % world}
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 2 ** 64, (n, 2), dtype=np.uint64)   # 128 random bits per row: no two rows share a key
    comm = pie.PieComm([0] * world)
    comm.gen_synthetic_sharded(SEED, n, users, D, 0)
    shards = [comm.ctx(r) for r in range(world)]
    print("sharded table resident: %s rows per shard" % [c.n for c in shards], flush=True)
    t0 = time.perf_counter()
    comm.token_set(keys)
    build = {"comm_token_set_wall_ms": (time.perf_counter() - t0) * 1e3, "shards": []}
    for r, c in enumerate(shards):
        info = c.table_info()
        build["shards"].append({"rank": r, "rows": c.n, "token_rows": info["token_rows"], "token_bytes": info["token_bytes"],
                                "token_builds": info["token_builds"], "token_build_ms": info["token_build_ms"]})
        assert info["token_rows"] == c.n, "every local row is covered"
    print(json.dumps(build), flush=True)
    with pie.PieScan(0) as plain:
        plain.gen_synthetic(SEED, n, 0, n, users, D, 0)
        t0 = time.perf_counter()
        plain.token_set(keys)
        build["plain_token_set_wall_ms"] = (time.perf_counter() - t0) * 1e3
        build["plain_token_build_ms"] = plain.table_info()["token_build_ms"]
        out["build"] = build
        out["lookups"] = []
        for k in (1, 64, 4096, 65536):
            rows = rng.integers(0, n, k).astype(np.int32)
            hit = keys[rows]
            miss = rng.integers(0, 2 ** 64, (k, 2), dtype=np.uint64)
            got, want = comm.token_lookup(hit, NOW), plain.token_lookup(hit, NOW)
            assert np.array_equal(got["row"], rows) and np.array_equal(want["row"], rows), "a key did not find its row"
            for col in ("live", "user", "start", "end"):
                assert np.array_equal(got[col], want[col]), col
            assert np.all(comm.token_lookup(miss, NOW)["row"] == -1) and np.all(plain.token_lookup(miss, NOW)["row"] == -1)
            rec = {"k": k}
            for name, ask in (("hit", hit), ("miss", miss)):
                c_med, c_min, c_max = wall_ms(lambda: comm.token_lookup(ask, NOW))
                p_med, p_min, p_max = wall_ms(lambda: plain.token_lookup(ask, NOW))
                rec[name] = {"comm_token_lookup_wall_ms": c_med, "comm_min_ms": c_min, "comm_max_ms": c_max,
                             "pie_token_lookup_wall_ms": p_med, "plain_min_ms": p_min, "plain_max_ms": p_max, "ratio": c_med / p_med}
            out["lookups"].append(rec)
            print(json.dumps(rec), flush=True)
    comm.close()
    if a.token_probe:
        out["plain_lookup_regression"] = {"tool": "tools/token_probe.py, unchanged, one run each", "runs": {}}
        for item in a.token_probe:
            label, path = item.split("=", 1)
            with open(path) as f:
                out["plain_lookup_regression"]["runs"][label] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
