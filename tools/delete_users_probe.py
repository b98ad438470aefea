#!/usr/bin/env python3
"""What does deleting the sessions of K users cost?  On generated tables (pie_gen_synthetic: cfg3, 10^8 rows and 10^5 users, and
the 1.25 x 10^7-row shard size) and for K = 1, 16, 256 and 4096 distinct users that no earlier repetition touched:
  (a) K calls of pie_delete_user, the path the library had before and keeps: the baseline
  (b) one pie_delete_users
both in this process, host wall time around the calls (their waits and the copy of the row list included), median of `reps`
repetitions after one warm-up on ids of its own.  Beside them the box's streaming-read ceiling (libpie_ubench.so, the best of
the one-stream forms of tools/read_ceiling.py) and what each path reads by its own arithmetic.  The kernels' device time is not
separated from the wall time here: neither path carries events.

usage: delete_users_probe.py [--rows N ...] [--users U] [--reps R]      -> profiles/delete_users_probe.json"""
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

SEED, D = 0x5EED5EED, 32
KS = (1, 16, 256, 4096)


def read_ceiling_gbs(nbytes=2_400_000_000, reps=5):
    ub = ctypes.CDLL(pie.build_ubench())
    ub.pie_ubench_read_bw.restype = ctypes.c_int
    ub.pie_ubench_read_bw.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    ms = (ctypes.c_double * 12)()
    if ub.pie_ubench_read_bw(0, nbytes, reps, ms):
        raise SystemExit("pie_ubench_read_bw failed")
    return max(nbytes / (m * 1e-3) / 1e9 for m in list(ms)[:8])


def probe_table(n, users, reps):
    out = {"rows": n, "users": users, "reps": reps, "k": []}
    need = sum(KS) * 2 * (reps + 1)
    if need > users:
        raise SystemExit("%d users are too few for %d fresh ids" % (users, need))
    ids = np.random.default_rng(3).permutation(users).astype(np.int32)
    at = 0

    def fresh(k):
        nonlocal at
        at += k
        return ids[at - k:at]

    with pie.PieScan(0) as ctx:
        ctx.gen_synthetic(SEED, n, 0, n, users, D, 0)
        ctx.synchronize()
        for k in KS:
            a_ms, b_ms, a_rows, b_rows = [], [], 0, 0
            for rep in range(reps + 1):   # rep 0 warms both paths up
                mine = fresh(k)
                t0 = time.perf_counter()
                got = sum(ctx.delete_user(int(u)).size for u in mine)
                ta = (time.perf_counter() - t0) * 1e3
                other = fresh(k)
                t0 = time.perf_counter()
                rows, per = ctx.delete_users(other)
                tb = (time.perf_counter() - t0) * 1e3
                assert rows.size == int(per.sum()) and np.all(np.diff(rows) > 0)
                if rep:
                    a_ms.append(ta)
                    b_ms.append(tb)
                    a_rows += got
                    b_rows += rows.size
            rec = {"k": k, "a_k_calls_delete_user_wall_ms": float(np.median(a_ms)), "b_one_delete_users_wall_ms": float(np.median(b_ms)),
                   "a_rows_per_rep": a_rows / reps, "b_rows_per_rep": b_rows / reps,
                   "a_bytes_read": 24.0 * n * k, "b_bytes_read": 8.0 * n + 16.0 * b_rows / reps}
            out["k"].append(rec)
            print(rec, flush=True)
    a1 = out["k"][0]["a_k_calls_delete_user_wall_ms"]
    b16 = out["k"][1]["b_one_delete_users_wall_ms"]
    out["condition"] = {"b_at_16_ms": b16, "twice_a_at_1_ms": 2 * a1, "met": bool(b16 < 2 * a1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[10 ** 8, 12_500_000])
    ap.add_argument("--users", type=int, default=10 ** 5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    out = {"tables": [probe_table(n, a.users, a.reps) for n in a.rows]}
    out["read_ceiling_gbs"] = read_ceiling_gbs()
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "delete_users_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
