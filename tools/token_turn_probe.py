#!/usr/bin/env python3
"""What does a whole turn in one launch (pie_token_turn) cost, beside what a caller without it has to do?

On the benchmark's table (cfg3: 10^8 generated rows, 10^5 users; every row gets a random key, as tools/token_probe.py --inflight
gives them) the host wall time through the Python binding, median and 90th percentile over 200 calls, of

  turn       ctx.token_turn(ops): one upload, one kernel, one download, one wait
  composed   the same ops through the calls that exist without it: the turn is cut wherever the clock changes and wherever a key
             comes a second time; every piece is one pie_token_lookup (its gets), one pie_token_set_end under the piece's clock
             (its touches) and one under PIE_END_NONE (its deletes), in that order — the pieces hold distinct keys, so the three do
             not interact.  The cutting itself is done ahead of the clock: only the device calls are timed.

for turns of 1, 64 and 4 096 ops under three mixes: all get; 80 % get, 15 % touch, 5 % del on distinct keys; the same with 10 % of
the ops repeating a key used earlier in the turn.  A turn of k ops carries 1, 2 and 4 distinct clocks for k = 1, 64, 4 096 (the
calls of a turn are stamped with Date.now() as they arrive: a turn that long spans a few milliseconds).  Every call of a series gets
ops of its own, drawn from sessions that are live at the clock, so deletes and touches do real work in every call.

usage: token_turn_probe.py [--rows N] [--reps R] [--out FILE]      -> profiles/token_turn_probe.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import sph_pie_amd as pie  # noqa: E402

SEED, D = 0x5EED5EED, 32
TTL = 12 * 3600 * 1000
END_NONE = -(2 ** 63)
MIXES = {"all_get": (1.0, 0.0, 0.0, 0.0), "mixed_distinct": (0.80, 0.15, 0.05, 0.0), "mixed_repeats": (0.80, 0.15, 0.05, 0.10)}
CLOCKS = {1: 1, 64: 2, 4096: 4}


def make_turn(rng, pool, k, mix, clock):
    """k ops on distinct keys of `pool`, then a share of them re-pointed at a key used earlier in the turn"""
    p_get, p_touch, p_del, p_repeat = mix
    ops = np.zeros(k, pie.TURN_OP)
    ops["tok"] = pool[rng.choice(pool.shape[0], k, replace=False)]
    if p_repeat and k > 1:
        again = np.nonzero(rng.random(k) < p_repeat)[0]
        again = again[again > 0]
        ops["tok"][again] = ops["tok"][(rng.random(again.size) * again).astype(np.int64)]
    ops["now"] = clock + np.sort(rng.integers(0, CLOCKS[k], k))
    ops["kind"] = rng.choice([pie.TURN_GET, pie.TURN_TOUCH, pie.TURN_DELETE], k, p=[p_get, p_touch, p_del])
    ops["new_end"] = np.where(ops["kind"] == pie.TURN_TOUCH, ops["now"] + TTL, 0)
    return ops


def compose(ops):
    """-> the pieces of the turn: (clock, get keys, touch keys, their new ends, delete keys), cut at every change of clock and at
    every key that comes a second time within a piece"""
    pieces, lo, seen = [], 0, set()
    for i in range(ops.shape[0] + 1):
        key = (int(ops["tok"][i][0]), int(ops["tok"][i][1])) if i < ops.shape[0] else None
        if i == ops.shape[0] or (i > lo and (ops["now"][i] != ops["now"][lo] or key in seen)):
            part = ops[lo:i]
            g, t, d = part["kind"] == pie.TURN_GET, part["kind"] == pie.TURN_TOUCH, part["kind"] == pie.TURN_DELETE
            pieces.append((int(part["now"][0]), np.ascontiguousarray(part["tok"][g]), np.ascontiguousarray(part["tok"][t]),
                           np.ascontiguousarray(part["new_end"][t]), np.ascontiguousarray(part["tok"][d])))
            lo, seen = i, set()
        if key is not None:
            seen.add(key)
    return pieces


def run_composed(ctx, pieces):
    calls = 0
    for clock, gets, touches, ends, dels in pieces:
        if gets.shape[0]:
            ctx.token_lookup(gets, clock)
            calls += 1
        if touches.shape[0]:
            ctx.token_set_end(touches, ends, clock)
            calls += 1
        if dels.shape[0]:
            ctx.token_set_end(dels, np.full(dels.shape[0], END_NONE, np.int64), END_NONE)
            calls += 1
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "token_turn_probe.json"))
    a = ap.parse_args()
    n, users = a.rows, max(1, a.rows // 1000)
    out = {"rows": n, "users": users, "reps": a.reps, "clocks_per_turn": CLOCKS, "series": []}
    rng = np.random.default_rng(1)
    with pie.PieScan(0) as ctx:
        ctx.gen_synthetic(SEED, n, 0, n, users, D, 0)
        sample = []
        for lo in range(0, n, a.chunk):
            hi = min(n, lo + a.chunk)
            keys = rng.integers(0, 2 ** 64, (hi - lo, 2), dtype=np.uint64)
            (ctx.token_set if lo == 0 else ctx.token_append)(keys)
            sample.append(keys[rng.integers(0, hi - lo, min(hi - lo, 1 + (1 << 21) * a.chunk // n))])
        ctx.synchronize()
        sample = np.concatenate(sample)
        got = ctx.token_lookup(sample, END_NONE)
        clock = int(np.median(got["end"]))                     # half of the sessions are live at it
        pool = sample[got["end"] > clock + 8]                  # sessions live at every clock a turn carries
        out["clock"], out["pool"] = clock, int(pool.shape[0])
        print("table and keys ready: %d live sessions to draw from" % pool.shape[0], flush=True)
        for k in (1, 64, 4096):
            for name, mix in MIXES.items():
                if k == 1 and name == "mixed_repeats":
                    continue                                   # one op repeats nothing
                rec = {"k": k, "mix": name}
                for way in ("turn", "composed"):
                    times, calls, pieces_n = [], 0, 0
                    for rep in range(a.reps + 3):              # three warm-up calls
                        ops = make_turn(rng, pool, k, mix, clock)
                        if way == "turn":
                            t0 = time.perf_counter()
                            ctx.token_turn(ops)
                            dt = time.perf_counter() - t0
                        else:
                            pieces = compose(ops)
                            t0 = time.perf_counter()
                            calls = run_composed(ctx, pieces)
                            dt = time.perf_counter() - t0
                            pieces_n = len(pieces)
                        if rep >= 3:
                            times.append(dt * 1e3)
                    rec[way + "_median_ms"], rec[way + "_p90_ms"] = float(np.median(times)), float(np.percentile(times, 90))
                    if way == "composed":
                        rec["composed_pieces_last"], rec["composed_calls_last"] = pieces_n, calls
                rec["composed_over_turn"] = rec["composed_median_ms"] / rec["turn_median_ms"]
                out["series"].append(rec)
                print(rec, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
