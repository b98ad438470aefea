#!/usr/bin/env python3
"""What does the token index cost?  On a generated table (pie_gen_synthetic; default 10^8 rows) every row gets the key
token_key(str(row)), uploaded in chunks through token_set then token_append.  Reported: the device time of the last index build
and of a full rebuild (token_build_ms), token_bytes, and for k = 1, 64, 4 096 and 65 536 the host wall time of pie_token_lookup
for all-hit and all-miss batches (median of 20) beside pie_fetch_rows of the same k from the same run: the per-request device
round trip a host pays today once it knows the row.  Wall times include the one wait of the call; the device time of a lookup is
not separated from it here.

usage: token_probe.py [--rows N] [--chunk K]      -> profiles/token_probe.json"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    a = ap.parse_args()
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
