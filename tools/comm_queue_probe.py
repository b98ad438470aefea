#!/usr/bin/env python3
"""Cost of the cross-shard dispatch queues (pie_comm_expired_queue / pie_comm_archive_queue) at BASELINE config 5 size:
10^8 sessions / 10^5 users / 32 disciplines in a world-8 communicator on ONE GPU (the RCCL stand-in tests/stub_rccl.c: the eight
shards share one MI355X and the "exchange" is device-to-device copies on it, not xGMI).  Per queue kind it records
  local        per-shard queue (pie_expired_queue / pie_archive_queue, no host copy), host wall time per shard
  phases       the communicator's own events on rank 0's stream (pie_comm_queue_timing): local queues + header exchange, pack,
               payload exchange, merge
  call         host wall time of the whole call (queue left on the device: queue_out = NULL)
  merge bytes  algorithmic bytes of the merge on ONE rank: every queued row read once (global + local row, 8 B) and written once
               (global row, source rank, source row, 12 B); the binary-search probes are listed apart
and prints one JSON object.  Kernel times come from a separate run under rocprofv3:
  rocprofv3 --kernel-trace --stats -d OUT -o cq -- python tools/comm_queue_probe.py --reps 3 --trace-only
usage: comm_queue_probe.py [--reps K] [--trace-only] [--out FILE]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
stub_dir = os.path.join(REPO, "tests", "_stub")
os.makedirs(stub_dir, exist_ok=True)
stub = os.path.join(stub_dir, "libstub_rccl.so")
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                "-L/opt/rocm/lib", "-lamdhip64"], check=True)
os.environ["PIE_RCCL_LIB"] = stub

import torch  # noqa: F401,E402  (before libpie_hip.so initialises HIP)
import sph_pie_amd as pie  # noqa: E402

T0, HOUR, DAY, W = 1700000000000, 3600 * 1000, 86400 * 1000, 43200000
WORLD, N, U, D = 8, 10 ** 8, 10 ** 5, 32
KINDS = {
    # the webhook tick: sessions that expired in the last hour
    "expired": ("pie_comm_expired_queue", T0 - 7 * HOUR, T0 - 6 * HOUR),
    # the daily archive: a window that qualifies part of the users
    "archive": ("pie_comm_archive_queue", T0 - 118 * DAY, W),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    comm = pie.PieComm([0] * WORLD)
    comm.gen_synthetic_sharded(0x5EED5EED, N, U, D, 1)
    ctxs = [comm.ctx(r) for r in range(WORLD)]
    out = {"world": WORLD, "rows": N, "users": U, "disciplines": D, "reps": a.reps,
           "setup": "one MI355X, eight shards, RCCL stand-in (device-to-device copies)", "kinds": {}}
    for kind, (fn, x, y) in KINDS.items():
        q = C.c_size_t(0)

        def call():
            rc = getattr(comm._lib, fn)(comm._c, int(x), int(y), None, 0, C.byref(q))
            assert rc == 0, comm._lib.pie_comm_last_error(comm._c).decode()

        call()  # warm-up: buffers grown to this queue
        if a.trace_only:
            for _ in range(a.reps):
                call()
            continue
        local = []
        for r in range(WORLD):
            ts = []
            for _ in range(a.reps):
                t = time.perf_counter()
                if kind == "expired":
                    ctxs[r].expired_queue(x, y, fetch=False)
                else:
                    ctxs[r].archive_queue(x, y, fetch=False)
                ctxs[r].synchronize()
                ts.append((time.perf_counter() - t) * 1e3)
            local.append(statistics.median(ts))
        shard_rows = [ctxs[r].queue_info()[1] for r in range(WORLD)]
        shard_groups = [ctxs[r].queue_info()[2] for r in range(WORLD)]
        walls, phases = [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            call()
            walls.append((time.perf_counter() - t) * 1e3)
            phases.append(comm.queue_timing())
        total = q.value
        med = [statistics.median(p[i] for p in phases) for i in range(4)]
        cap_rows = max(shard_rows)
        probes = total * (WORLD - 1) * max(1, math.ceil(math.log2(max(cap_rows, 2)))) if kind == "expired" else \
            sum(shard_groups) * (WORLD - 1) * max(1, math.ceil(math.log2(max(max(shard_groups), 2)))) * 2
        msg_words = 2 + 2 * cap_rows + max(shard_groups) + 1
        out["kinds"][kind] = {
            "queued_rows": total, "shard_rows": shard_rows, "shard_groups": shard_groups,
            "local_queue_ms_per_shard": [round(v, 3) for v in local],
            "phase_ms_rank0": {"local_and_header": round(med[0], 3), "pack": round(med[1], 3), "exchange": round(med[2], 3),
                               "merge": round(med[3], 3)},
            "call_ms": round(statistics.median(walls), 3),
            "message_bytes_per_rank": msg_words * 4,
            "merge_alg_bytes_per_rank": total * 20,
            "merge_search_probes_per_rank": probes,
        }
    comm.close()
    if not a.trace_only:
        text = json.dumps(out, indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
    else:
        print("trace run done")


if __name__ == "__main__":
    main()
