#!/usr/bin/env python3
"""What does it cost a SHARDED table to age?  cfg3 (10^8 sessions / 10^5 users / 32 disciplines) as a world-8 communicator on ONE
GPU (the RCCL stand-in tests/stub_rccl.c: eight shards on one MI355X, never across GPUs).  Three calls, each made ONCE on a
fresh table (they consume what they list), on two communicators that hold the same table:
  comm      wall time of pie_comm_prune_before (a cutoff that lists about 1 % of the rows), then pie_comm_retention_purge_tz
            (lists about 90 % of the rows), then pie_comm_compact_rows, with the device times of pie_comm_queue_timing (shard
            passes, staging copies, -, merge kernel)
  caller    what a caller must do without them, measured by the same tool in the same run: the plain call on each context of
            pie_comm_ctx, pie_shard_rows_to_global on each list, a host merge with numpy; pie_compact_rows per context
Both sides bring the list to the host through the Python binding.  -> profiles/comm_maint_probe.json (--out)"""
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
stub = os.path.join(stub_dir, "libstub_rccl_maint_probe.so")
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                "-L/opt/rocm/lib", "-lamdhip64"], check=True)
os.environ["PIE_RCCL_LIB"] = stub

import numpy as np  # noqa: E402
import torch  # noqa: F401,E402  (before libpie_hip.so initialises HIP)
import sph_pie_amd as pie  # noqa: E402

SEED, D = 0x5EED5EED, 32
T0_MS, SPAN_MS, DAY = 1700000000000, 10368000000, 86400 * 1000
ZONE = "America/New_York"


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def caller_list(comm, world, call):
    """the parent commit's way: per context the plain call, the translation, then one host merge"""
    t = {"plain_calls_ms": 0.0, "rows_to_global_ms": 0.0}
    lists = []
    for r in range(world):
        c = comm.ctx(r)
        rows, ms = timed(lambda: call(c))
        t["plain_calls_ms"] += ms
        rows, ms = timed(lambda: c.shard_rows_to_global(rows))
        t["rows_to_global_ms"] += ms
        lists.append(rows)
    merged, t["host_merge_ms"] = timed(lambda: np.sort(np.concatenate(lists), kind="stable"))
    t["total_ms"] = t["plain_calls_ms"] + t["rows_to_global_ms"] + t["host_merge_ms"]
    return merged, t


def comm_list(comm, call):
    rows, ms = timed(call)
    shard, stage, _, merge = comm.queue_timing()
    return rows, {"total_ms": ms, "device_shard_passes_ms": shard, "device_staging_ms": stage, "device_merge_kernel_ms": merge}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--users", type=int, default=10 ** 5)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "comm_maint_probe.json"))
    a = ap.parse_args()
    n, users, world = a.rows, a.users, a.world
    tz = pie.binding.tz_table(ZONE)
    cutoff = T0_MS - SPAN_MS + SPAN_MS // 100          # starts are uniform over [T0 - SPAN, T0]: about 1 % lie below
    now, months = T0_MS + 49 * DAY, 2                  # start + 2 months <= now for about 90 % of the rows
    out = {"rows": n, "users": users, "disciplines": D, "world": world, "zone": ZONE, "cutoff": cutoff, "now": now, "months": months,
           "setup": "one MI355X, %d shards on it, RCCL stand-in: eight shards on one GPU, never across GPUs; wall times through the "
                    "Python binding, every call made once on a fresh table; both sides end with the list on the host" % world}
    new, old = pie.PieComm([0] * world), pie.PieComm([0] * world)
    for c in (new, old):
        c.gen_synthetic_sharded(SEED, n, users, D, 0)
    # a first call of each kind on an empty result warms the code objects and the communicator's buffers on both sides
    new.prune_before(-(2 ** 62))
    caller_list(old, world, lambda c: c.prune_before(-(2 ** 62)))

    got, t_new = comm_list(new, lambda: new.prune_before(cutoff))
    want, t_old = caller_list(old, world, lambda c: c.prune_before(cutoff))
    assert np.array_equal(got, want)
    out["prune_before"] = {"listed": int(got.size), "comm": t_new, "caller": t_old}

    got, t_new = comm_list(new, lambda: new.retention_purge(now, months, tz_table=tz))
    want, t_old = caller_list(old, world, lambda c: c.retention_purge(now, months, tz_table=tz))
    assert np.array_equal(got, want)
    out["retention_purge_tz"] = {"listed": int(got.size), "comm": t_new, "caller": t_old}

    (kept, _), ms_new = timed(lambda: new.compact_rows())
    kept_old, ms_old = timed(lambda: sum(old.ctx(r).compact_rows() for r in range(world)))
    assert kept == kept_old
    out["compact_rows"] = {"kept": int(kept), "comm": {"total_ms": ms_new}, "caller": {"total_ms": ms_old}}
    assert new.table_size() == (n, users)
    new.close()
    old.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
