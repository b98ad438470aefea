"""GPU: the end-ordered hot index (pie_kernels.h HotRec) — the batched 1-byte pass reading the index's suffix and delta instead
of the key column.  Every batch is compared with the oracle and with a context that never builds the index (PIE_HOT_INDEX=0):
bench's 64-query batch and a heterogeneous one, queries on and below the index's range, touches across bins, revivals,
deletes, prune and retention purge, time-ordered and late appends, the delta outgrowing its capacity, batches pipelined on
1-4 lanes between mutations, a sharded table and the full cfg3 table."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT64_MIN = -(2 ** 63)
ALL = 2 ** 64 - 1
DAY = 86400 * 1000
HOUR = 3600 * 1000
SEED = 0x5EED5EED
SPEC_MASK = 0x5555555555555555


def ctx_with(pie, hot):
    old = os.environ.get("PIE_HOT_INDEX")
    os.environ["PIE_HOT_INDEX"] = "1" if hot else "0"
    try:
        return pie.PieScan(0)
    finally:
        if old is None:
            os.environ.pop("PIE_HOT_INDEX")
        else:
            os.environ["PIE_HOT_INDEX"] = old


def bench_queries(oracle, D):
    lim = ALL if D >= 64 else (1 << D) - 1
    return [(oracle.T0_MS - 6 * HOUR - 977 * q, oracle.T0_MS - 61 * DAY, SPEC_MASK & lim) for q in range(64)]


def mixed_queries(oracle, k):
    t0 = oracle.T0_MS
    masks = [0x5555555555555555, 0xAAAAAAAAAAAAAAAA, ALL, 0x00000000FFFF0000, 0x1, 0x8000000000000001]
    return [(t0 - 6 * HOUR - 977 * i - (i % 5) * HOUR, t0 - (61 + i % 4) * DAY - 13 * i, masks[i % len(masks)]) for i in range(k)]


def same(got, want, tag):
    for name, a, b in zip(("counts", "offsets", "idx"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), (tag, name)


class Pair:
    """The same table in a context with the index and one without; the oracle's columns kept in step on the host."""

    def __init__(self, pie, cols, U, D):
        self.on, self.off = ctx_with(pie, True), ctx_with(pie, False)
        self.s, self.e, self.u, self.d = [c.copy() for c in cols]
        self.U, self.D = U, D
        for c in (self.on, self.off):
            c.load_columns(self.s, self.e, self.u, self.d, U)
            c.set_disciplines(ALL, D)

    def close(self):
        self.on.close()
        self.off.close()

    def each(self, fn):
        return [fn(c) for c in (self.on, self.off)]

    def check(self, oracle, queries, tag, n_oracle=None):
        lim = ALL if self.D >= 64 else (1 << self.D) - 1
        got_on, got_off = self.each(lambda c: c.scan_batch(queries))
        pick = range(len(queries)) if n_oracle is None else sorted({0, len(queries) - 1} | set(range(0, len(queries), max(1, len(queries) // n_oracle))))
        for q in range(len(queries)):
            same(got_on[q], got_off[q], "%s: query %d, index on vs off" % (tag, q))
        for q in pick:
            now, cutoff, mask = queries[q]
            same(got_on[q], oracle.scan(self.s, self.e, self.u, self.d, self.U, now, cutoff, mask & lim), "%s: query %d vs oracle" % (tag, q))
        return got_on

    def info(self):
        return self.on.table_info()


def test_hot_index_batches_match(pie, oracle):
    n, U, D = 3_000_017, 20011, 32
    p = Pair(pie, oracle.gen(SEED, n, 0, n, U, D, 0), U, D)
    try:
        p.check(oracle, bench_queries(oracle, D), "bench batch", n_oracle=8)
        info = p.info()
        assert info["hot_builds"] == 1 and 0 < info["hot_rows"] < n // 5 and info["hot_bytes"] > 32 * info["hot_rows"]
        assert p.off.table_info()["hot_builds"] == 0
        p.check(oracle, mixed_queries(oracle, 64), "mixed batch", n_oracle=8)
        # candidates: the records the pass evaluated, on an unchanged table the keyed pass's count
        c_on, c_off = p.each(lambda c: c.stats()["candidates"])
        assert c_on == c_off > 0
        # queries on `end` values (a row's `end` equal to a query's `now` is not live), and below the index's range
        t0 = oracle.T0_MS
        top = np.sort(p.e[p.e > t0 - 12 * HOUR])
        edge = [(int(top[i]), t0 - 61 * DAY, ALL) for i in range(0, top.size, max(1, top.size // 20))]
        edge += [(int(top[i]) - 1, t0 - 61 * DAY, SPEC_MASK) for i in range(0, top.size, max(1, top.size // 20))]
        p.check(oracle, edge[:64], "on end values")
        p.check(oracle, [(t0 - 30 * DAY, t0 - 61 * DAY, ALL), (t0 - 6 * HOUR, t0 - 61 * DAY, ALL)], "below the index")
        assert p.info()["hot_builds"] == 1
    finally:
        p.close()


def test_hot_index_under_mutation(pie, oracle):
    n, U, D = 1_000_003, 5003, 32
    p = Pair(pie, oracle.gen(SEED + 1, n, 0, n, U, D, 0), U, D)
    rng = np.random.default_rng(7)
    t0 = oracle.T0_MS
    queries = mixed_queries(oracle, 24) + bench_queries(oracle, D)[:8]
    try:
        p.check(oracle, queries, "built")
        assert p.info()["hot_builds"] == 1

        def set_end(rows, ne):
            p.each(lambda c: c.set_end(rows, ne))
            p.e[rows] = ne

        # touches: rows from below the index into its top bins, held rows up a bin or down, rows lowered out of it
        live = np.nonzero(p.e > t0 - 12 * HOUR)[0]
        dead = np.nonzero(p.e < t0 - 30 * DAY)[0]
        rows = np.concatenate([rng.choice(dead, 3000, replace=False), rng.choice(live, 3000, replace=False)]).astype(np.int32)
        ne = np.concatenate([t0 + rng.integers(0, 12 * HOUR, 3000), t0 - rng.integers(0, 20 * DAY, 3000)]).astype(np.int64)
        set_end(rows, ne)
        p.check(oracle, queries, "touched")
        # the same rows again (entries now in the delta), some of them up again
        set_end(rows[:2000], (ne[:2000] + HOUR).astype(np.int64))
        p.check(oracle, queries, "touched twice")
        # deletes, prune and retention purge tombstone rows in place
        for uu in rng.choice(U, 40, replace=False):
            gone = p.each(lambda c: c.delete_user(int(uu)))
            assert np.array_equal(gone[0], gone[1])
            p.e[gone[0]] = INT64_MIN
        gone = p.each(lambda c: c.prune_before(t0 - 60 * DAY))
        assert np.array_equal(gone[0], gone[1])
        p.e[gone[0]] = INT64_MIN
        gone = p.each(lambda c: c.retention_purge(t0 - 3 * HOUR, 2, 0))
        assert np.array_equal(gone[0], gone[1])
        p.e[gone[0]] = INT64_MIN
        p.check(oracle, queries, "tombstoned")
        # revived tombstones
        tomb = np.nonzero(p.e == INT64_MIN)[0]
        rv = rng.choice(tomb, min(tomb.size, 1500), replace=False).astype(np.int32)
        set_end(rv, (t0 + rng.integers(-HOUR, 6 * HOUR, rv.size)).astype(np.int64))
        p.check(oracle, queries, "revived")
        assert p.info()["hot_builds"] == 1   # every change so far was mirrored, none rebuilt the index
        # appends: created now in time order, and late ones out of order (the first outgrows the loaded table's capacity: the
        # columns are re-allocated and the keys rebuilt, and with them the index; the second lands in place and is mirrored)
        builds = []
        for late in (False, True):
            k = 4000
            s2 = (int(p.s.max()) + np.sort(rng.integers(0, 4000, k))) if not late else (t0 - rng.integers(0, 20 * HOUR, k))
            s2 = s2.astype(np.int64)
            e2 = (s2 + rng.integers(-2 * DAY, DAY, k)).astype(np.int64)
            u2, d2 = rng.integers(0, U, k).astype(np.int32), rng.integers(0, D, k).astype(np.int32)
            p.each(lambda c: c.append_rows(s2, e2, u2, d2, U))
            p.s, p.e, p.u, p.d = np.concatenate([p.s, s2]), np.concatenate([p.e, e2]), np.concatenate([p.u, u2]), np.concatenate([p.d, d2])
            p.check(oracle, queries, "appended (late %s)" % late)
            builds.append(p.info()["hot_builds"])
        assert builds[0] == builds[1] and p.info()["hot_rows"] > 0
    finally:
        p.close()


def test_hot_index_delta_overflow_rebuilds(pie, oracle):
    n, U, D = 700_001, 3001, 32
    p = Pair(pie, oracle.gen(SEED + 2, n, 0, n, U, D, 0), U, D)
    rng = np.random.default_rng(11)
    t0 = oracle.T0_MS
    queries = mixed_queries(oracle, 16)
    try:
        p.check(oracle, queries, "built")
        builds = p.info()["hot_builds"]
        dropped = False
        for step in range(8):   # 30000 rows a call: the host's bound passes the delta's 65536 entries on the third
            rows = rng.choice(n, 30000, replace=False).astype(np.int32)
            ne = (t0 + rng.integers(-6 * HOUR, 12 * HOUR, rows.size)).astype(np.int64)
            p.each(lambda c: c.set_end(rows, ne))
            p.e[rows] = ne
            dropped = dropped or p.info()["hot_rows"] == 0
            p.check(oracle, queries, "touch %d" % step)
        assert dropped and p.info()["hot_builds"] > builds and p.info()["hot_rows"] > 0
    finally:
        p.close()


@pytest.mark.parametrize("lanes", [1, 2, 3, 4])
def test_hot_index_pipelined_lanes_between_mutations(pie, oracle, lanes):
    n, U, D = 2_000_003, 10007, 32
    p = Pair(pie, oracle.gen(SEED + 3, n, 0, n, U, D, 4), U, D)   # rows in order of creation
    rng = np.random.default_rng(lanes)
    t0 = oracle.T0_MS
    lim = (1 << D) - 1
    try:
        p.each(lambda c: c.set_batch_lanes(lanes))
        for rnd in range(3):
            batches = [mixed_queries(oracle, 64)[j::3] + bench_queries(oracle, D)[j:j + 40] for j in range(3 * lanes)]
            res = []
            for c in (p.on, p.off):   # every batch of the round in flight at once, finished in order
                for qs in batches:
                    c.scan_batch_begin(qs)
                out = []
                for qs in batches:
                    c.scan_batch_finish()
                    out.append([c.batch_read_results(q) for q in range(len(qs))])
                res.append(out)
            for b, qs in enumerate(batches):
                for q in range(len(qs)):
                    same(res[0][b][q], res[1][b][q], "round %d batch %d query %d" % (rnd, b, q))
                for q in (0, len(qs) - 1):
                    now, cutoff, mask = qs[q]
                    same(res[0][b][q], oracle.scan(p.s, p.e, p.u, p.d, U, now, cutoff, mask & lim), "round %d batch %d query %d vs oracle" % (rnd, b, q))
            rows = rng.choice(p.s.size, 2000, replace=False).astype(np.int32)
            ne = (t0 + rng.integers(-12 * HOUR, 12 * HOUR, rows.size)).astype(np.int64)
            p.each(lambda c: c.set_end(rows, ne))
            p.e[rows] = ne
            k = 1500
            s2 = (int(p.s.max()) + np.sort(rng.integers(0, 3000, k))).astype(np.int64)
            e2, u2, d2 = s2 + 12 * HOUR, rng.integers(0, U, k).astype(np.int32), rng.integers(0, D, k).astype(np.int32)
            p.each(lambda c: c.append_rows(s2, e2, u2, d2, U))
            p.s, p.e, p.u, p.d = np.concatenate([p.s, s2]), np.concatenate([p.e, e2]), np.concatenate([p.u, u2]), np.concatenate([p.d, d2])
        assert p.info()["hot_rows"] > 0
    finally:
        p.close()


def test_hot_index_on_a_shard(pie, oracle):
    n, U, D = 2_000_003, 10007, 32
    on, off = ctx_with(pie, True), ctx_with(pie, False)
    try:
        shapes = []
        for c in (on, off):
            c.gen_synthetic(SEED, n, 0, n, U, D, 0)
            c.set_disciplines(ALL, D)
            c.scan_batch(bench_queries(oracle, D)[:4])   # an index of the whole table first: sharding must drop it
            shapes.append(c.shard_table(1, 4))
        assert shapes[0] == shapes[1]
        assert on.table_info()["hot_rows"] == 0
        queries = mixed_queries(oracle, 32)
        got_on, got_off = on.scan_batch(queries), off.scan_batch(queries)
        for q in range(len(queries)):
            same(got_on[q], got_off[q], "shard query %d" % q)
        assert on.table_info()["hot_builds"] == 2
        # against the oracle on the shard's own columns
        s, e, u, d = on.read_columns()
        for q in (0, 31):
            now, cutoff, mask = queries[q]
            same(got_on[q], oracle.scan(s, e, u, d, on.n_users, now, cutoff, mask & ((1 << D) - 1)), "shard query %d vs oracle" % q)
    finally:
        on.close()
        off.close()


def test_hot_index_cfg3(pie, oracle):
    """The benchmark's table (10^8 rows, 10^5 users, 32 disciplines): bench's batch and a heterogeneous one, three lanes,
    nine batches in flight.  It compares index on against index off: both sides share the union tail, so this is no check of
    the tail at this user count; tests/test_gpu_user_axis.py checks batches at 100 003 users against the oracle."""
    N, U, D = 10 ** 8, 10 ** 5, 32
    on, off = ctx_with(pie, True), ctx_with(pie, False)
    try:
        for c in (on, off):
            c.gen_synthetic(SEED, N, 0, N, U, D, 0)
            c.set_disciplines(SPEC_MASK & ((1 << D) - 1), D)
            c.set_batch_lanes(3)
        batches = [bench_queries(oracle, D) if b % 2 == 0 else mixed_queries(oracle, 64) for b in range(9)]
        res = []
        for c in (on, off):
            for qs in batches:
                c.scan_batch_begin(qs)
            out = []
            for qs in batches:
                c.scan_batch_finish()
                out.append([c.batch_read_results(q) for q in (0, 17, 63)] + [c.stats()["candidates"]])
            res.append(out)
        for b in range(9):
            for k in range(3):
                same(res[0][b][k], res[1][b][k], "cfg3 batch %d result %d" % (b, k))
            assert res[0][b][3] == res[1][b][3], "candidates of batch %d" % b
        info = on.table_info()
        assert info["hot_builds"] == 1 and 0 < info["hot_rows"] < N // 5
    finally:
        on.close()
        off.close()
