"""GPU: wide batches on the ordered run (pie_set_wide_ordered; sph-pie_amd/csrc/pie_ordered.h "wide batches on the run") against
the CPU oracle: per-query sizes and lists, the wide union word for word (no 64-row bound per user), feeds and request fetches
read from it, both key streams, ambiguous keys, a dense query, a union that outgrows the result arrays, the exchange message,
pipelining with ordinary batches, table changes between batches, and the switch itself.  Every test has a context of its own:
the shared one is never left with the switch on."""
import numpy as np
import pytest

from test_gpu_ordered import skewed_table

pytestmark = pytest.mark.gpu

INT64_MIN = -(2 ** 63)
ALL = 2 ** 64 - 1
DAY = 86400 * 1000
HOUR = 3600 * 1000
E_INVAL, E_STATE = -1, -6
MASKS = [0x5555555555555555, ALL, 0xAAAAAAAAAAAAAAAA, 0x00000000FFFF0000 | 3, 0x1]
GUARD, GUARD_WORD = 64, -1234567


def assert_same(got, want, tag=""):
    for name, a, b in zip(("counts", "offsets", "idx"), got, want):
        assert a.dtype == b.dtype, (tag, name)
        assert np.array_equal(a, b), (tag, name)


def base_queries(oracle, k):
    t0 = oracle.T0_MS
    return [(t0 - 6 * HOUR - 977 * i - (i % 3) * HOUR, t0 - (61 + i % 4) * DAY - 13 * i, MASKS[i % len(MASKS)]) for i in range(k)]


def answers(oracle, cols, U, D, queries):
    s, e, u, d = cols
    lim = ALL if D >= 64 else (1 << D) - 1
    return [oracle.scan(s, e, u, d, U, now, cutoff, mask & lim) for now, cutoff, mask in queries]


def union_from(cols, U, ans):
    """the wide union restated in numpy from the oracle's answers: per user the rows any query selects in (start, row) order,
    ceil(Q / 64) mask words per row, bit q set iff query q selects the row"""
    words = (len(ans) + 63) // 64
    allr = np.concatenate([a[2] for a in ans]).astype(np.int64)
    qs = np.concatenate([np.full(a[2].size, q, np.int64) for q, a in enumerate(ans)])
    rows, inv = np.unique(allr, return_inverse=True)
    s, user = cols[0], cols[2]
    order = np.lexsort((rows, s[rows], user[rows]))
    rank = np.empty(rows.size, np.int64)
    rank[order] = np.arange(rows.size)
    masks = np.zeros((rows.size, words), np.uint64)
    np.bitwise_or.at(masks, (rank[inv.reshape(-1)], qs // 64), np.uint64(1) << (qs % 64).astype(np.uint64))
    rows = rows[order]
    uoff = np.zeros(U + 1, np.int64)
    np.add.at(uoff, user[rows].astype(np.int64) + 1, 1)
    return np.cumsum(uoff), rows.astype(np.int32), masks


def union_cap(n, U):
    """the union result arrays hold at least this many rows (batch_ucap with the table at its own size)"""
    return max(16 * U, n // 16 + 4096)


def open_run(pie, oracle, cols, U, D, switch=1):
    """a context whose batches take the ordered run (mode 2, one scan builds it), with the switch as asked"""
    ctx = pie.PieScan(0)
    ctx.load_columns(*cols, U)
    ctx.set_disciplines(ALL, D)
    ctx.set_ordered_run(2)
    ctx.scan(oracle.T0_MS - 6 * HOUR, oracle.T0_MS - 61 * DAY)
    assert ctx.table_info()["ordered_builds"] == 1
    if switch:
        ctx.set_wide_ordered(switch)
    return ctx


def check_union(ctx, cols, U, want, tag):
    un = ctx.batch_read_union_wide()
    assert un is not None, tag
    uoff, rows, masks = un
    w_uoff, w_rows, w_masks = union_from(cols, U, want)
    assert np.array_equal(uoff, w_uoff), tag
    assert np.array_equal(rows, w_rows), tag
    assert masks.shape == w_masks.shape and np.array_equal(masks, w_masks), tag
    nq = len(want)
    assert masks.shape[1] == (nq + 63) // 64
    if nq % 64 and masks.shape[0]:
        assert not np.any(masks[:, -1] >> np.uint64(nq % 64)), "mask bits at or above n_q"
    return un


def check_feeds(ctx, cols, want, q, users, tag):
    s, e, u, d = cols
    offs, idx, st, en, di = ctx.batch_fetch_requests([q] * len(users), users)
    for i, user in enumerate(users):
        c, off, ix = want[q]
        feed = ix[off[user]: off[user + 1]]
        assert np.array_equal(ctx.batch_read_user_feed(q, user), feed), (tag, q, user)
        got = idx[offs[i]: offs[i + 1]]
        assert np.array_equal(got, feed), (tag, q, user)
        assert np.array_equal(st[offs[i]: offs[i + 1]], s[feed]) and np.array_equal(en[offs[i]: offs[i + 1]], e[feed]), (tag, q, user)


_tables = {}


def table(oracle, n, U, D):
    """the skewed table of a shape and the oracle's answers to its 512 base queries, computed once"""
    key = (n, U, D)
    if key not in _tables:
        cols = skewed_table(oracle, n, U, D, 0x5EED + n)
        _tables[key] = (cols, answers(oracle, cols, U, D, base_queries(oracle, 512)))
    return _tables[key]


@pytest.mark.parametrize("n,U,D,nqs", [(70001, 333, 7, (65, 300, 512)), (400000, 2000, 16, (65, 300, 512)), (700, 3, 2, (65,))])
def test_wide_on_the_run_equals_the_oracle(pie, oracle, n, U, D, nqs):
    cols, want_all = table(oracle, n, U, D)
    head = 7 % U
    with open_run(pie, oracle, cols, U, D) as ctx:
        for nq in nqs:
            queries, want = base_queries(oracle, nq), want_all[:nq]
            mu = int(np.unique(np.concatenate([w[2] for w in want])).size)
            assert mu <= union_cap(n, U), "the inputs keep the union inside the result arrays"
            ctx.scan_wide_begin(queries)
            ms = ctx.scan_wide_finish()
            assert ms == [int(w[2].size) for w in want], nq
            assert ctx.stats()["k1_variant"] & 0x3000 == 0x3000, hex(ctx.stats()["k1_variant"])
            check_union(ctx, cols, U, want, "n=%d nq=%d" % (n, nq))
            for q in sorted({0, 1, 63, 64, nq // 2, nq - 1}):
                assert_same(ctx.batch_read_results(q), want[q], "nq=%d query %d" % (nq, q))
            for q in (0, 64, nq - 1):
                check_feeds(ctx, cols, want, q, [head, 0, U - 1], "nq=%d" % nq)


def test_wide_on_the_run_key_streams_and_edges(pie, oracle):
    """the 2-byte and the 1-byte key stream; `now` equal to a row's end, one below, one above (the ambiguous-key compare); a
    query that selects nothing; 64 disciplines with rows whose discipline lies outside the table"""
    n, U, D = 70001, 333, 64
    t0 = oracle.T0_MS
    s, e, u, d = skewed_table(oracle, n, U, D, 0x5EED + n)
    d = d.copy()
    d[5::997] = 64
    d[6::997] = 100
    d[7::997] = -1
    cols = (s, e, u, d)
    ends = np.sort(e[(e > t0 - 5 * HOUR) & (e < t0 - 4 * HOUR)])
    assert ends.size >= 3
    edge = []
    for ev in (int(ends[0]), int(ends[ends.size // 2]), int(ends[-1])):
        edge += [(ev, t0 - 61 * DAY, ALL), (ev - 1, t0 - 61 * DAY, ALL), (ev + 1, t0 - 62 * DAY, MASKS[0])]
    base = base_queries(oracle, 130)
    fine = base[:100] + edge + [(2 ** 62, INT64_MIN, ALL)] + base[100:]
    coarse = list(fine)
    # The 1-byte key covers the top tenth of the `end` values, so a `now` below its base has more than a tenth of the rows keyed
    # above it: with a fresh key histogram the library calls such a query dense and takes it out of the batch.  A touch (here
    # of one row, to the value it has) makes the histogram stale; no query is called dense then, and the batch takes the 2-byte
    # stream for this one.
    coarse[3] = (t0 - 20 * DAY, t0 - 61 * DAY, 0xFF)
    assert np.count_nonzero(e > coarse[3][0]) > n // 10
    with open_run(pie, oracle, cols, U, D) as ctx:
        for queries, variant in ((fine, 0x3C00), (coarse, 0x3400)):
            if variant == 0x3400:
                ctx.set_end(np.array([11], np.int32), e[11:12])
            want = answers(oracle, cols, U, D, queries)
            assert want[109][2].size == 0 and len(np.unique(np.concatenate([w[2] for w in want]))) <= union_cap(n, U)
            ctx.scan_wide_begin(queries)
            assert ctx.scan_wide_finish() == [int(w[2].size) for w in want], hex(variant)
            assert ctx.stats()["k1_variant"] == variant, hex(ctx.stats()["k1_variant"])
            check_union(ctx, cols, U, want, hex(variant))
            for q in (3, 100, 101, 102, 108, 109, len(queries) - 1):
                assert_same(ctx.batch_read_results(q), want[q], "%x query %d" % (variant, q))


class HostMsg:
    """mapped host memory for one message plus guard words behind it"""

    def __init__(self, ctx, n_words):
        self.ctx, self.n = ctx, n_words
        self.h, self.d, self.addr = ctx.host_alloc(n_words + GUARD)
        self.h[:] = GUARD_WORD

    def free(self):
        self.ctx.host_free(self.addr)


def msg_words(u_pad, cap, words):
    return u_pad + 2 + cap * (1 + 2 * words)


def expected_message(U, u_pad, cap, words, union):
    uoff, rows, masks = union
    mu = int(rows.size)
    k = min(mu, cap)
    msg = np.zeros(msg_words(u_pad, cap, words), np.int32)
    written = np.zeros(msg.size, bool)
    msg[: U + 1] = uoff.astype(np.int32)
    msg[U + 1: u_pad + 2] = mu
    written[: u_pad + 2] = True
    msg[u_pad + 2: u_pad + 2 + k] = rows[:k]
    written[u_pad + 2: u_pad + 2 + k] = True
    base = u_pad + 2 + cap
    msg[base: base + k * 2 * words] = np.ascontiguousarray(masks[:k]).reshape(-1).view(np.int32)
    written[base: base + k * 2 * words] = True
    return msg, written


def test_wide_on_the_run_dense_query_falls_back(pie, oracle):
    """a dense query leaves the batch and runs on the general path: every query exact, no union, ready = 0"""
    n, U, D = 70001, 333, 7
    cols, want_all = table(oracle, n, U, D)
    queries = base_queries(oracle, 100)
    queries[40] = (oracle.T0_MS - 100 * DAY, oracle.T0_MS - 61 * DAY, ALL)
    want = list(want_all[:100])
    want[40] = answers(oracle, cols, U, D, [queries[40]])[0]
    assert want[40][2].size * 10 > n, "the query is dense"
    with open_run(pie, oracle, cols, U, D) as ctx:
        words, u_pad, cap = 2, U, 2048
        a = HostMsg(ctx, msg_words(u_pad, cap, words))
        try:
            ctx.scan_wide_begin_union(queries, a.d, u_pad, cap)
            ms, ready = ctx.scan_wide_finish_packed()
            assert ready is False and ms == [int(w[2].size) for w in want]
            assert ctx.batch_read_union_wide() is None
            for q in (0, 39, 40, 41, 99):
                assert_same(ctx.batch_read_results(q), want[q], "query %d" % q)
            ctx.synchronize()
            assert np.all(a.h[: u_pad + 2] == -1) and np.all(a.h[a.n:] == GUARD_WORD)
        finally:
            a.free()


def overflow_queries(oracle):
    """240 queries, `now` 12 h apart across the corpus's 120 days, no cutoff, every discipline: together nearly every row"""
    return [(oracle.T0_MS - 12 * HOUR * i, INT64_MIN, ALL) for i in range(240)]


def test_wide_on_the_run_union_outgrows_the_arrays(pie, oracle):
    """240 queries that together select nearly every row: far more than the result arrays hold.  With a fresh key histogram
    most of them are called dense and leave the batch before the pass; a touch of one row (to the value it has) makes the
    histogram stale, so here ALL of them take the pass and its union really outgrows the pool and the result arrays.  The pass
    ran on the run (variant 0x3400), every query is rerun and exact, there is no union; the sticky flag then sends the
    context's next wide batches to the per-query path (variant 0, no union), exact too."""
    n, U, D = 70001, 333, 7
    cols, want_all = table(oracle, n, U, D)
    queries = overflow_queries(oracle)
    want = answers(oracle, cols, U, D, queries)
    assert np.unique(np.concatenate([w[2] for w in want])).size > 2 * union_cap(n, U)
    with open_run(pie, oracle, cols, U, D) as ctx:
        ctx.set_end(np.array([11], np.int32), cols[1][11:12])
        ctx.scan_wide_begin(queries)
        assert ctx.scan_wide_finish() == [int(w[2].size) for w in want]
        assert ctx.stats()["k1_variant"] == 0x3400, hex(ctx.stats()["k1_variant"])
        assert ctx.batch_read_union_wide() is None
        for q in (0, 1, 64, 120, 239):
            assert_same(ctx.batch_read_results(q), want[q], "query %d" % q)
        small, want_small = base_queries(oracle, 70), want_all[:70]
        for _ in range(2):
            ctx.scan_wide_begin(small)
            assert ctx.scan_wide_finish() == [int(w[2].size) for w in want_small]
            assert ctx.stats()["k1_variant"] == 0 and ctx.batch_read_union_wide() is None, "the sticky flag"
            for q in (0, 64, 69):
                assert_same(ctx.batch_read_results(q), want_small[q], "after the overflow, query %d" % q)
        # a table loaded anew clears the flag
        ctx.load_columns(*cols, U)
        ctx.scan(oracle.T0_MS - 6 * HOUR, oracle.T0_MS - 61 * DAY)
        ctx.scan_wide_begin(small)
        assert ctx.scan_wide_finish() == [int(w[2].size) for w in want_small]
        assert ctx.stats()["k1_variant"] & 0x3000 == 0x3000
        check_union(ctx, cols, U, want_small, "after a new load")


def test_wide_on_the_run_overflow_with_fresh_histogram(pie, oracle):
    """the same 240 queries with the key histogram fresh: whichever of them are called dense fall back before the pass; every
    query is exact, there is no union, and the next small wide batch is exact with or without one"""
    n, U, D = 70001, 333, 7
    cols, want_all = table(oracle, n, U, D)
    queries = overflow_queries(oracle)
    want = answers(oracle, cols, U, D, queries)
    with open_run(pie, oracle, cols, U, D) as ctx:
        ctx.scan_wide_begin(queries)
        assert ctx.scan_wide_finish() == [int(w[2].size) for w in want]
        assert ctx.batch_read_union_wide() is None
        for q in (0, 120, 239):
            assert_same(ctx.batch_read_results(q), want[q], "query %d" % q)
        small, want_small = base_queries(oracle, 70), want_all[:70]
        ctx.scan_wide_begin(small)
        assert ctx.scan_wide_finish() == [int(w[2].size) for w in want_small]
        un = ctx.batch_read_union_wide()
        if un is not None:
            assert all(np.array_equal(a, b) for a, b in zip(un, union_from(cols, U, want_small)))


def test_wide_on_the_run_overflow_with_a_message(pie, oracle):
    """pie_scan_wide_begin_union whose union outgrows the arrays (stale histogram, as above): the message pack runs on the
    clipped union before finish says ready = 0 and writes the "no union" header; nothing is written past the message"""
    n, U, D = 70001, 333, 7
    cols, _ = table(oracle, n, U, D)
    queries = overflow_queries(oracle)
    want = answers(oracle, cols, U, D, queries)
    words, u_pad = 4, U + 3
    with open_run(pie, oracle, cols, U, D) as ctx:
        ctx.set_end(np.array([11], np.int32), cols[1][11:12])
        for cap in (2 * n, 1000):   # above what the arrays hold, and below it
            a = HostMsg(ctx, msg_words(u_pad, cap, words))
            try:
                ctx.set_wide_ordered(1)
                if cap != 2 * n:    # the first overflow set the sticky flag: a new load clears it
                    ctx.load_columns(*cols, U)
                    ctx.scan(oracle.T0_MS - 6 * HOUR, oracle.T0_MS - 61 * DAY)
                    ctx.set_end(np.array([11], np.int32), cols[1][11:12])
                ctx.scan_wide_begin_union(queries, a.d, u_pad, cap)
                ms, ready = ctx.scan_wide_finish_packed()
                assert ready is False and ms == [int(w[2].size) for w in want]
                assert ctx.stats()["k1_variant"] == 0x3400, hex(ctx.stats()["k1_variant"])
                assert ctx.batch_read_union_wide() is None
                ctx.synchronize()
                assert np.all(a.h[: u_pad + 2] == -1), cap
                assert np.all(a.h[a.n:] == GUARD_WORD), cap
            finally:
                a.free()


def test_wide_on_the_run_writes_its_message(pie, oracle):
    """pie_scan_wide_begin_union on the run: ready = 1 at finish and the message, read without a synchronize call, equals the
    oracle's union word for word; a cap below Mu cuts rows while Mu stays the full count; the guard words are intact"""
    n, U, D = 70001, 333, 7
    cols, want_all = table(oracle, n, U, D)
    with open_run(pie, oracle, cols, U, D) as ctx:
        for nq in (65, 300):
            queries, want = base_queries(oracle, nq), want_all[:nq]
            union = union_from(cols, U, want)
            mu, words, u_pad = int(union[1].size), (nq + 63) // 64, U + 5
            assert 3 < mu <= union_cap(n, U)
            for cap in (mu + 9, mu, mu // 3):
                L = msg_words(u_pad, cap, words)
                a = HostMsg(ctx, L)
                try:
                    ctx.scan_wide_begin_union(queries, a.d, u_pad, cap)
                    ms, ready = ctx.scan_wide_finish_packed()
                    assert ready is True, (nq, cap)
                    got = a.h.copy()
                    assert ms == [int(w[2].size) for w in want]
                    exp, written = expected_message(U, u_pad, cap, words, union)
                    assert np.array_equal(got[:L][written], exp[written]), (nq, cap)
                    assert np.all(got[:L][~written] == GUARD_WORD), "words of cut rows were written"
                    assert np.all(got[L:] == GUARD_WORD), "written past the message"
                    assert np.all(got[U: u_pad + 2] == mu), "padding words / Mu word"
                finally:
                    a.free()


def test_wide_on_the_run_pipelined_and_after_table_changes(pie, oracle):
    """two wide batches in flight; a wide, an ordinary and a wide batch in flight, finished in begin order; then a touch, a
    delete and an in-order append between batches: the next batch sees the changed columns"""
    n, U, D = 70001, 333, 7
    cols, want_all = table(oracle, n, U, D)
    s, e, u, d = [c.copy() for c in cols]
    t0 = oracle.T0_MS
    head = 7 % U
    qa, qb, qo = base_queries(oracle, 300), base_queries(oracle, 512)[200:330], base_queries(oracle, 512)[400:416]
    wa, wb, wo = want_all[:300], want_all[200:330], want_all[400:416]
    with open_run(pie, oracle, cols, U, D) as ctx:
        ctx.scan_wide_begin(qa)
        ctx.scan_wide_begin(qb)
        assert ctx.scan_wide_finish() == [int(w[2].size) for w in wa]
        check_union(ctx, cols, U, wa, "first of two")
        assert ctx.scan_wide_finish() == [int(w[2].size) for w in wb]
        check_union(ctx, cols, U, wb, "second of two")
        ctx.scan_wide_begin(qb)
        ctx.scan_batch_begin(qo)
        ctx.scan_wide_begin(qa)
        ms, ready = ctx.scan_wide_finish_packed()
        assert ms == [int(w[2].size) for w in wb]
        check_union(ctx, cols, U, wb, "wide, then ordinary")
        ms, ready = ctx.scan_wide_finish_packed()
        assert ms == [int(w[2].size) for w in wo]
        for q in (0, 15):
            assert_same(ctx.batch_read_results(q), wo[q], "ordinary batch between wide ones, query %d" % q)
        ms, ready = ctx.scan_wide_finish_packed()
        assert ms == [int(w[2].size) for w in wa]
        check_union(ctx, cols, U, wa, "wide behind an ordinary batch")
        # the first append outgrows the loaded table's capacity: the table is re-allocated and the run goes with it; the next
        # scan builds it again (mode 2), and from then on in-order appends go into the run in place
        g_s, g_e = np.array([s.max() + 1], np.int64), np.array([t0 + HOUR], np.int64)
        ctx.append_rows(g_s, g_e, np.array([head], np.int32), np.array([0], np.int32), U)
        s, e, u, d = np.concatenate([s, g_s]), np.concatenate([e, g_e]), np.append(u, head).astype(np.int32), np.append(d, 0).astype(np.int32)
        n += 1
        ctx.scan(t0 - 6 * HOUR, t0 - 61 * DAY)
        assert ctx.table_info()["ordered_builds"] == 2
        want = answers(oracle, (s, e, u, d), U, D, qa)
        ctx.scan_wide_begin(qa)
        assert ctx.scan_wide_finish() == [int(w[2].size) for w in want]
        assert ctx.stats()["k1_variant"] & 0x3000 == 0x3000, hex(ctx.stats()["k1_variant"])
        check_union(ctx, (s, e, u, d), U, want, "after the table grew")
        wa = want
        # a touch and a delete of rows of the head user that the batch selects, then an in-order append
        sel_head = np.unique(np.concatenate([w[2] for w in wa]))
        sel_head = sel_head[u[sel_head] == head]
        assert sel_head.size >= 8
        touched, deleted = sel_head[:4].astype(np.int32), sel_head[4:8].astype(np.int32)
        e[touched] = t0 + DAY
        e[deleted] = INT64_MIN
        ctx.set_end(np.concatenate([touched, deleted]), np.concatenate([e[touched], e[deleted]]))
        k = 50
        a_s = np.int64(s.max()) + 1 + np.arange(k, dtype=np.int64)
        a_e = np.full(k, t0 + HOUR, np.int64)
        a_u = np.where(np.arange(k) % 2 == 0, head, np.arange(k) % U).astype(np.int32)
        a_d = (np.arange(k) % D).astype(np.int32)
        ctx.append_rows(a_s, a_e, a_u, a_d, U)
        s, e, u, d = np.concatenate([s, a_s]), np.concatenate([e, a_e]), np.concatenate([u, a_u]), np.concatenate([d, a_d])
        changed = (s, e, u, d)
        want = answers(oracle, changed, U, D, qa)
        assert any(np.isin(np.arange(n, n + k), w[2]).any() for w in want), "the appended rows are selected"
        ctx.scan_wide_begin(qa)
        assert ctx.scan_wide_finish() == [int(w[2].size) for w in want]
        assert ctx.stats()["k1_variant"] & 0x3000 == 0x3000, hex(ctx.stats()["k1_variant"])
        check_union(ctx, changed, U, want, "after touch, delete and append")
        for q in (0, 64, 299):
            assert_same(ctx.batch_read_results(q), want[q], "after the changes, query %d" % q)
        check_feeds(ctx, changed, want, 1, [head, 0, U - 1], "after the changes")


def test_wide_ordered_switch(pie, oracle):
    """off is the default (no union on the run, as before); PIE_E_STATE with a batch in flight; PIE_E_INVAL for other values; a
    table that does not take the ordered run is not affected"""
    n, U, D = 70001, 333, 7
    cols, want_all = table(oracle, n, U, D)
    queries, want = base_queries(oracle, 100), want_all[:100]
    with open_run(pie, oracle, cols, U, D, switch=0) as ctx:
        ctx.scan_wide_begin(queries)
        assert ctx.scan_wide_finish() == [int(w[2].size) for w in want]
        assert ctx.batch_read_union_wide() is None and ctx.stats()["k1_variant"] == 0
        ctx.scan_wide_begin(queries)
        with pytest.raises(pie.PieError) as ei:
            ctx.set_wide_ordered(1)
        assert ei.value.code == E_STATE
        ctx.scan_wide_finish()
        for bad in (2, -1):
            with pytest.raises(pie.PieError) as ei:
                ctx.set_wide_ordered(bad)
            assert ei.value.code == E_INVAL
        ctx.set_wide_ordered(1)
        ctx.scan_wide_begin(queries)
        assert ctx.scan_wide_finish() == [int(w[2].size) for w in want]
        check_union(ctx, cols, U, want, "switched on")
        ctx.set_wide_ordered(0)
        ctx.scan_wide_begin(queries)
        ctx.scan_wide_finish()
        assert ctx.batch_read_union_wide() is None
    # evenly spread users, default mode: the general wide pass, whatever the switch says
    n, U, D = 100003, 4999, 32
    cols = oracle.gen(0x5EED5EED, n, 0, n, U, D, 0)
    want = answers(oracle, cols, U, D, queries)
    with pie.PieScan(0) as ctx:
        ctx.load_columns(*cols, U)
        ctx.set_disciplines(ALL, D)
        ctx.scan_wide_begin(base_queries(oracle, 512))   # grows the union slot capacity
        ctx.scan_wide_finish()
        unions = []
        for on in (0, 1):
            ctx.set_wide_ordered(on)
            ctx.scan_wide_begin(queries)
            assert ctx.scan_wide_finish() == [int(w[2].size) for w in want]
            assert ctx.stats()["k1_variant"] & 0x3000 == 0x1000
            unions.append(check_union(ctx, cols, U, want, "general pass, switch %d" % on))
        assert all(np.array_equal(a, b) for a, b in zip(*unions))
