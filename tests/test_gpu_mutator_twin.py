"""GPU: the plain mutators and the mutators by global id are the same code.  Two contexts hold the same table, one plain, one
sharded as the only shard of a world of one (its maps are the identity); the same chain of appends and touches goes through
append_rows / set_end on the first and shard_append_rows / shard_set_end on the second.  After every step the two must agree
exactly on the columns, the sizes, the hot index as the device holds it (hot_canon: all of it but the order in which an atomic
counter hands out delta slots, in which two contexts that run the very same kernel differ too) and on a single scan, a 16-query
batch and a 70-query wide batch; the single scan is also held against the oracle on a numpy copy of the table."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, N0, U0, D = 20261, 2000, 40, 32
INT64_MIN = -(2 ** 63)


def same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


def hot_state(pie, ctx):
    """hot_layout(), or None while the context has no hot index"""
    try:
        return ctx.hot_layout()
    except pie.PieError as e:
        assert e.code == -6
        return None


def hot_canon(h):
    """A hot index with the one thing left out that the code does not decide: which slot of the delta a row that moved there
    took.  The slots are handed out by an atomic counter in whatever order the waves of a touch reach it, so two runs of ONE
    kernel may differ there.  Kept: the bin offsets, the main records, every row's place in the main part or outside the
    index, which rows sit in the delta, and the set of slots they hold."""
    pos, m = h["pos"], h["n_main"]
    return (np.array([m]), h["off"], h["user"], h["row"], h["bin"], np.where(pos >= m, m, pos), np.sort(pos[pos >= m]))


class Twin:
    def __init__(self, pie, oracle, ordered):
        self.pie, self.o = pie, oracle
        self.plain, self.shard = pie.PieScan(0), pie.PieScan(0)
        for c in (self.plain, self.shard):
            if ordered:
                c.set_ordered_run(2)
            c.gen_synthetic(SEED, N0, 0, N0, U0, D, 0)
        assert self.shard.shard_table(0, 1) == (N0, U0)
        self.s, self.e, self.u, self.d = (a.copy() for a in oracle.gen(SEED, N0, 0, N0, U0, D, 0))
        self.U, self.t = U0, 0
        self.rng = np.random.default_rng(81)
        self.hot_seen = 0

    def close(self):
        self.plain.close()
        self.shard.close()

    def append(self, k, new_users=0):
        o, rng = self.o, self.rng
        n_users = self.U + new_users
        self.t += 1
        s = (o.T0_MS + o.SPAN_MS + self.t * 100000 + np.arange(k)).astype(np.int64)  # in creation order, as a session store appends
        e = s + rng.integers(o.TTL_MS // 4, o.TTL_MS, k)
        u = rng.integers(0, n_users, k).astype(np.int32)
        u[: min(new_users, k)] = np.arange(self.U, self.U + min(new_users, k))  # the new ids do appear
        d = rng.integers(0, D, k).astype(np.int32)
        self.plain.append_rows(s, e, u, d, n_users)
        assert self.shard.shard_append_rows(s, e, u, d, n_users) == (self.s.shape[0], k)
        self.s, self.e = np.concatenate([self.s, s]), np.concatenate([self.e, e])
        self.u, self.d = np.concatenate([self.u, u]), np.concatenate([self.d, d])
        self.U = n_users

    def touch(self, k, recent):
        o, rng, n = self.o, self.rng, self.s.shape[0]
        rows = rng.integers(0, n, k).astype(np.int32)
        rows[: min(recent, k)] = np.arange(n - min(recent, k), n)  # rows the step just before appended; no wait in between
        if k >= 4:
            rows[k // 2] = rows[0]  # repeats: the last value wins
            rows[k - 1] = rows[1]
        vals = (o.T0_MS + o.SPAN_MS + rng.integers(-o.TTL_MS, o.TTL_MS, k)).astype(np.int64)
        vals[rng.random(k) < 0.2] = INT64_MIN  # tombstones among them
        if k == 1:
            vals[0] = INT64_MIN
        self.plain.set_end(rows, vals)
        self.shard.shard_set_end(rows, vals)
        for r, v in zip(rows.tolist(), vals.tolist()):  # array order
            self.e[r] = v

    def check(self, what):
        o, rng, a, b = self.o, self.rng, self.plain, self.shard
        n = self.s.shape[0]
        assert a.n == b.n == n and a.n_users == b.n_users == self.U, what
        ca, cb = a.read_columns(), b.read_columns()
        assert same(ca, cb) and same(ca, (self.s, self.e, self.u, self.d)), "%s: columns" % what
        ha, hb = hot_state(self.pie, a), hot_state(self.pie, b)
        assert (ha is None) == (hb is None), "%s: one context has a hot index, the other none" % what
        if ha is not None:
            self.hot_seen += 1
            assert same(hot_canon(ha), hot_canon(hb)), "%s: hot index" % what
        top = o.T0_MS + o.SPAN_MS
        now, cutoff = int(top - o.TTL_MS // 3), int(top - 3 * o.TTL_MS)
        one = a.scan(now, cutoff)
        assert same(one, b.scan(now, cutoff)), "%s: single scan" % what
        assert same(one, o.scan(self.s, self.e, self.u, self.d, self.U, now, cutoff, 2 ** 64 - 1)), "%s: single scan against the oracle" % what

        def query():
            return (int(top + rng.integers(-o.TTL_MS, o.TTL_MS // 2)), int(top - rng.integers(0, 4 * o.TTL_MS)),
                    int(rng.integers(1, 2 ** 32)) | (1 << int(rng.integers(0, D))))

        q16, q70 = [query() for _ in range(16)], [query() for _ in range(70)]
        for ga, gb in zip(a.scan_batch(q16), b.scan_batch(q16)):
            assert same(ga, gb), "%s: batch" % what
        for ga, gb in zip(a.scan_wide(q70), b.scan_wide(q70)):
            assert same(ga, gb), "%s: wide batch" % what


@pytest.mark.parametrize("ordered", (False, True), ids=("plain_table", "ordered_run"))
@pytest.mark.parametrize("async_mutations", ("0", "1"))
def test_twin_chain(pie, oracle, async_mutations, ordered, monkeypatch):
    monkeypatch.setenv("PIE_ASYNC_MUTATIONS", async_mutations)  # read when a context is created
    tw = Twin(pie, oracle, ordered)
    try:
        tw.check("start")  # the first batch builds the hot index where there is one: the mutators below keep it in step
        # the wave and 256-thread block edges of both append kernels, each followed by touches of 1, 64 or 257 elements that
        # reach into the rows just appended; the first append and the first new users outgrow the capacity, the second new
        # users fit it, and the last append is larger than all the room the table has
        steps = [("append", 1, 0), ("touch", 1, 1), ("append", 63, 0), ("touch", 64, 63), ("append", 64, 0), ("touch", 257, 64),
                 ("append", 65, 7), ("touch", 64, 65), ("append", 255, 0), ("touch", 257, 255), ("append", 256, 5), ("touch", 1, 1),
                 ("append", 257, 0), ("touch", 257, 257), ("append", None, 0), ("touch", 64, 64), ("append", 64, 0), ("touch", 257, 64)]
        for i, (op, k, arg) in enumerate(steps):
            if op == "append":
                if k is None:
                    k = tw.plain.table_info()["table_bytes"] // 24
                    assert k == tw.shard.table_info()["table_bytes"] // 24 and k > 0
                tw.append(k, new_users=arg)
            else:
                tw.touch(k, recent=arg)
            tw.check("step %d (%s %d)" % (i, op, k))
        if not ordered:
            assert tw.hot_seen > 0, "the chain never ran with a hot index"
    finally:
        tw.close()
