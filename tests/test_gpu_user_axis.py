"""GPU: batches, wide batches, single-scan buckets and user-table growth on LARGE user tables, against the oracle.

Every batched path has a stage shaped by the number of users: the transposed histogram, the 256-user tiles of the union tail
and their look-back (256 threads gather a tile's predecessors: tile 256, the last of 65 537 users, still has 256 of them;
tile 257, which 65 793 users bring, is the first to make a second trip), the per-query totals folded into 64 slots by tile & 63,
and the capacity rules that choose between routes (524 288 users: the last batched size; 1 048 576: the last fused single-scan
size; two rules of 2 GiB on the bucket slots).  The tables here are small in rows (300 007) and large in users; hand-made
buckets of exactly 1, 2, 8, 9, 16, 17, 33 and 64 selected union rows (table_model.plant_user_buckets) sit in tile 0, tiles 255,
256 and 257, the last full tile, the last tile (user U - 1) and in tiles congruent mod 64.  The queries come in stages
(table_model.user_axis_queries): stage k selects at most 16, 17, 33, 64, 65 rows of a bucket, so the tests decide when the
union buckets outgrow their slots.  tests/test_table_model.py checks those properties of the tables without a GPU.

Every expected value comes from oracle_py.scan on the same columns or from TableModel; every context is created here and
closed again (these tables would resize the shared context's user arrays for every test after them)."""
import numpy as np
import pytest

import table_model as T
from table_model import ALL, DAY, HOUR, INT64_MIN

pytestmark = pytest.mark.gpu

N, D = 300007, 32
LIM = (1 << D) - 1
SIZES = [65536, 65537, 65793, 100003, 262145, 524288, 524289]
GUARD, GUARD_WORD = 64, -1234567


class Book:
    """The tables of this module and the oracle's answers on them, kept for the module's tests only (fixture `book`)."""

    def __init__(self, oracle):
        self.oracle, self.T0_MS = oracle, oracle.T0_MS
        self.tables, self.idx = {}, {}

    def table(self, U):
        if U not in self.tables:
            self.tables[U] = T.plant_user_buckets(self.oracle.gen(11, N, 0, N, U, D, 0), U, D, self.T0_MS)
        return self.tables[U]

    def put(self, U, cols, planted):
        self.tables[U] = (cols, planted)

    def drop(self, U):
        self.tables.pop(U, None)
        for key in [k for k in self.idx if k[0] == U]:
            del self.idx[key]

    def answer(self, U, q):
        """oracle.scan of one query on table(U).  Only idx is kept (counts and offsets of half a million users for hundreds
        of queries would be gigabytes); they are checked against idx when the answer is computed and rebuilt from it on
        demand."""
        cols, _ = self.table(U)
        if (U, q) not in self.idx:
            c, off, idx = self.oracle.scan(*cols, U, q[0], q[1], q[2] & LIM)
            assert np.array_equal(c, np.bincount(cols[2][idx], minlength=U)) and np.array_equal(off[1:], np.cumsum(c)) and off[0] == 0
            self.idx[(U, q)] = idx
        idx = self.idx[(U, q)]
        c = np.bincount(cols[2][idx], minlength=U).astype(np.int32)
        off = np.zeros(U + 1, np.int64)
        np.cumsum(c, out=off[1:])
        return c, off, idx


@pytest.fixture(scope="module")
def book(oracle):
    b = Book(oracle)
    yield b
    b.tables.clear()
    b.idx.clear()


class Answers:
    """the answers of a query list, built one at a time when asked for"""

    def __init__(self, book, U, qs):
        self.book, self.U, self.qs = book, U, qs

    def __len__(self):
        return len(self.qs)

    def __getitem__(self, k):
        return self.book.answer(self.U, self.qs[k])

    def __iter__(self):
        return (self[k] for k in range(len(self.qs)))

    def m(self):
        return [int(self[k][2].size) for k in range(len(self.qs))]

    def union(self):
        cols, _ = self.book.table(self.U)
        light = [(None, None, self.book.answer(self.U, q)[2]) for q in self.qs]
        return T.union_from_answers(cols[0], cols[2], self.U, light)


def open_ctx(pie, cols, U, hot, lanes=1):
    ctx = T.ctx_with_env(pie, hot, 1)
    try:
        ctx.set_ordered_run(0)        # the batched pass and its tail are under test, not the ordered run
        ctx.set_batch_lanes(lanes)
        ctx.load_columns(*cols, U)
        ctx.set_disciplines(ALL, D)
    except BaseException:
        ctx.close()
        raise
    return ctx


class HostMsg:
    def __init__(self, ctx, n_words):
        self.ctx = ctx
        self.h, self.d, self.addr = ctx.host_alloc(n_words + GUARD)
        self.h[:] = GUARD_WORD

    def free(self):
        self.ctx.host_free(self.addr)


def special_users(U, planted):
    return sorted(planted) + [0, 1, U - 1, U // 2]


def check_readers(ctx, tag, cols, U, planted, qs, wants, which):
    """per-query lists of `which`, the planted users' feeds and a handful of (query, user) requests in one call"""
    for qi in which:
        T.same(ctx.batch_read_results(qi), wants[qi], (tag, "query", qi))
    users = special_users(U, planted)
    last = len(qs) - 1
    for u in users:
        w = wants[last]
        assert np.array_equal(ctx.batch_read_user_feed(last, u), w[2][w[1][u]:w[1][u + 1]]), (tag, "feed", last, u)
    big = [u for u in sorted(planted) if planted[u] >= 33][:6] + [U - 1, 0, -1, U]
    qis = np.array([(7 * k) % len(qs) for k in range(len(big))], np.int32)
    off, idx, st, en, di = ctx.batch_fetch_requests(qis, np.array(big, np.int32))
    assert off[0] == 0 and off[-1] == idx.size
    for k, (qi, u) in enumerate(zip(qis.tolist(), big)):
        w = wants[qi]
        want = w[2][w[1][u]:w[1][u + 1]] if 0 <= u < U else np.zeros(0, np.int32)
        assert np.array_equal(idx[off[k]:off[k + 1]], want), (tag, "request", qi, u)
    assert np.array_equal(st, cols[0][idx]) and np.array_equal(en, cols[1][idx]) and np.array_equal(di, cols[3][idx])


def check_narrow_union(ctx, tag, U, qs, wants, msg, u_pad, cap, ready):
    """the union word for word, check_union, and the message the tail wrote against the pack kernel's and numpy's"""
    un = ctx.batch_read_union()
    assert un is not None, (tag, "the batch kept no union")
    want = wants.union()
    assert np.array_equal(un[0], want[0]) and np.array_equal(un[1], want[1]) and np.array_equal(un[2], want[2][:, 0]), (tag, "union")
    T.check_union(tag, un, wants, False)
    if msg is None:
        return
    assert ready is True, (tag, "the tail did not write the message")
    exp, written = T.union_message(U, u_pad, cap, want, len(qs), False)
    got = msg.h.copy()
    L = exp.size
    assert np.array_equal(got[:L][written], exp[written]), (tag, "message of the tail")
    assert np.all(got[:L][~written] == GUARD_WORD) and np.all(got[L:] == GUARD_WORD), (tag, "words written outside the message")
    ref = HostMsg(ctx, L)
    try:
        ctx.batch_pack_union_device(ref.d, u_pad, cap)
        ctx.synchronize()
        assert np.array_equal(ref.h[:L][written], exp[written]) and np.all(ref.h[L:] == GUARD_WORD), (tag, "message of the pack kernel")
    finally:
        ref.free()


def batch_path(ctx, hot_rows):
    v = ctx.stats()["k1_variant"]
    if v == 0:
        return "fallback"
    return ("hot_index" if hot_rows else "keyed_1byte" if v & 0x800 else "keyed_2byte") + ("" if ctx.batch_read_union() is not None else "+rerun")


def one_batch(ctx, book, tag, U, planted, stage, nq, expect, hot, which=None):
    """one batch of stage `stage`, checked in full.  expect: "union" (the batched pass answered and kept its union), "rerun" (it
    ran, a bucket outgrew its slots, every query was rerun) or "fallback" (no batched pass at all)."""
    qs = T.user_axis_queries(book.T0_MS, nq, stage)
    wants = Answers(book, U, qs)
    cols = book.table(U)[0]
    ctx.scan_batch_begin(qs)
    hot_rows = ctx.table_info()["hot_rows"]
    ms = ctx.scan_batch_finish()
    assert list(ms) == wants.m(), (tag, "M per query")
    path = batch_path(ctx, hot_rows)
    if expect == "fallback":
        assert path == "fallback" and ctx.batch_read_union() is None, (tag, path)
    elif expect == "rerun":
        assert path.endswith("+rerun"), (tag, path)
    else:
        assert path == ("hot_index" if hot else "keyed_1byte"), (tag, path)
        check_narrow_union(ctx, tag, U, qs, wants, None, 0, 0, False)
    check_readers(ctx, tag, cols, U, planted, qs, wants, range(nq) if which is None else which)
    return path


# ------------------------------------------------------------------------------------------------ 1. the batched pass
@pytest.mark.parametrize("hot", [1, 0])
@pytest.mark.parametrize("U", SIZES)
def test_batches_by_user_count(pie, oracle, book, U, hot):
    """Batches of 1, 16 and 64 heterogeneous queries, three in flight on one lane and spread over three, each writing its union
    message (u_pad = U and u_pad > U).  Up to 524 288 users the batched pass answers (over the hot index with the index on, the
    keyed 1-byte pass over the table with it off) and keeps its union once two warm-up batches, whose buckets of 17 and of 33
    rows outgrow 16 and 32 slots, have grown the buckets to 64 slots; at 524 289 every query falls back, with the same results."""
    cols, planted = book.table(U)
    supported = T.batch_supported_users(U)
    seen = []
    for lanes in (1, 3):
        ctx = open_ctx(pie, cols, U, hot, lanes)
        try:
            for stage in (1, 2):
                seen.append(one_batch(ctx, book, ("warm-up", U, hot, lanes, stage), U, planted, stage, 1, "rerun" if supported else "fallback", hot))
            sets = [T.user_axis_queries(oracle.T0_MS, nq, 3) for nq in (1, 16, 64)]
            sized = Answers(book, U, sets[2]).union()
            assert int(np.diff(sized[0]).max()) == 64 and sorted(set(np.diff(sized[0])[sorted(planted)])) == list(T.PLANT_SIZES)
            cap = int(sized[1].size) + 5
            pads = [U, U + 5, U + 64]
            msgs = [HostMsg(ctx, p + 2 + 3 * cap) for p in pads]
            try:
                hot_rows = []
                for qs, msg, u_pad in zip(sets, msgs, pads):
                    ctx.scan_batch_begin_union(qs, msg.d, u_pad, cap)
                    hot_rows.append(ctx.table_info()["hot_rows"])
                for qs, msg, u_pad, hr in zip(sets, msgs, pads, hot_rows):
                    tag = ("batch", U, "hot", hot, "lanes", lanes, "queries", len(qs))
                    wants = Answers(book, U, qs)
                    ms, ready = ctx.scan_batch_finish(packed=True)
                    assert list(ms) == wants.m(), (tag, "M per query")
                    path = batch_path(ctx, hr)
                    seen.append(path)
                    if supported:
                        assert path == ("hot_index" if hot else "keyed_1byte"), (tag, path)
                        assert (hr > 0) == bool(hot), (tag, "hot_rows at begin", hr)
                        assert ready is True, (tag, "a batch that kept its union did not write its message itself")
                        check_narrow_union(ctx, tag, U, qs, wants, msg, u_pad, cap, ready)
                    else:
                        assert path == "fallback" and ctx.batch_read_union() is None and not ready, (tag, path)
                    check_readers(ctx, tag, cols, U, planted, qs, wants, range(len(qs)))
                info = ctx.table_info()
                assert info["hot_builds"] == (1 if hot and supported else 0), ("hot_builds", U, hot, info["hot_builds"])
            finally:
                ctx.synchronize()
                for m in msgs:
                    m.free()
        finally:
            ctx.close()
    print("\nuser-axis batches: U %d tiles %d hot %d -> %s" % (U, (U + 255) // 256, hot, sorted(set(seen))))


@pytest.mark.parametrize("U", [100003, 524288])
def test_union_buckets_grow_with_large_user_tables(pie, oracle, book, U):
    """A batch in which a user's union holds 17 rows outgrows the 16 slots: it is rerun, every batch array is replaced, and the
    next batches are exact at 32 slots per user; the same from 33 rows to 64 slots.  65 rows do not fit 64 slots: from then on
    batches run as single scans, still exact."""
    cols, planted = book.table(U)
    ctx = open_ctx(pie, cols, U, 1)
    try:
        steps = [(0, 16, "union"), (1, 16, "rerun"), (1, 16, "union"), (0, 64, "union"), (2, 16, "rerun"), (2, 16, "union"),
                 (3, 64, "union"), (1, 1, "union"), (4, 16, "rerun"), (3, 16, "fallback"), (0, 64, "fallback")]
        for k, (stage, nq, expect) in enumerate(steps):
            one_batch(ctx, book, ("growth", U, "step", k, "stage", stage), U, planted, stage, nq, expect, 1, which=sorted({0, min(1, nq - 1), nq // 2, nq - 1}))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 2. wide batches
def one_wide(ctx, book, tag, U, planted, stage, nq, expect_union, with_msg=False, u_pad=0):
    from sph_pie_amd.binding import split_wide_message
    qs = T.user_axis_queries(book.T0_MS, nq, stage)
    wants = Answers(book, U, qs)
    cols = book.table(U)[0]
    words = (nq + 63) // 64
    msg = None
    try:
        if with_msg:
            want_un = wants.union()
            cap = int(want_un[1].size) + 3
            msg = HostMsg(ctx, u_pad + 2 + cap * (1 + 2 * words))
            ctx.scan_wide_begin_union(qs, msg.d, u_pad, cap)
            ms, ready = ctx.scan_wide_finish_packed()
        else:
            ctx.scan_wide_begin(qs)
            ms, ready = ctx.scan_wide_finish(), None
        assert ms == wants.m(), (tag, "M per query")
        un = ctx.batch_read_union_wide()
        if expect_union is not None:
            assert (un is not None) == expect_union, (tag, "a union" if un is not None else "no union")
        if un is not None:
            want_un = wants.union()
            assert np.array_equal(un[0], want_un[0]) and np.array_equal(un[1], want_un[1]) and np.array_equal(un[2], want_un[2]), (tag, "wide union")
            T.check_union(tag, (un[0], un[1], un[2].reshape(-1)), wants, True)
        if with_msg and un is not None:
            assert ready is True, (tag, "the tail did not write the message")
            exp, written = T.union_message(U, u_pad, cap, want_un, nq, True)
            got, L = msg.h.copy(), exp.size
            assert np.array_equal(got[:L][written], exp[written]), (tag, "message of the tail")
            assert np.all(got[:L][~written] == GUARD_WORD) and np.all(got[L:] == GUARD_WORD), (tag, "words written outside the message")
            s_uoff, s_mu, s_rows, s_masks = split_wide_message(got[:L], u_pad, cap, words)
            assert s_mu == want_un[1].size and np.array_equal(s_rows, want_un[1]) and np.array_equal(s_masks, want_un[2])
            ref = HostMsg(ctx, L)
            try:
                ctx.batch_pack_union_wide_device(ref.d, u_pad, cap)
                ctx.synchronize()
                assert np.array_equal(ref.h[:L][written], exp[written]) and np.all(ref.h[L:] == GUARD_WORD), (tag, "message of the pack kernel")
            finally:
                ref.free()
        check_readers(ctx, tag, cols, U, planted, qs, wants, sorted({0, min(63, nq - 1), min(64, nq - 1), nq // 2, nq - 1}))
        return un is not None
    finally:
        if msg is not None:
            ctx.synchronize()
            msg.free()


@pytest.mark.parametrize("U", SIZES)
def test_wide_batches_by_user_count(pie, oracle, book, U):
    """65, 300 and 512 queries in one pass: M per query, the wide union in all its mask words, lists of queries 0, 63, 64 and
    the last, and the message of the tail against the pack kernel's and numpy's.  Up to 524 288 users a wide pass answers (after
    the two warm-up batches that grow the buckets to 64 slots); at 524 289 the fallback does."""
    cols, planted = book.table(U)
    supported = T.batch_supported_users(U)
    ctx = open_ctx(pie, cols, U, 1)
    seen = []
    try:
        for stage in (1, 2):
            seen.append(one_wide(ctx, book, ("wide warm-up", U, stage), U, planted, stage, 65, False))
        for nq, u_pad in ((65, U), (300, U + 7), (512, U + 7)):
            seen.append(one_wide(ctx, book, ("wide", U, nq), U, planted, 3, nq, supported, True, u_pad))
    finally:
        ctx.close()
    print("\nuser-axis wide batches: U %d -> %s" % (U, ["wide_pass" if s else "fallback" for s in seen]))


def test_wide_capacity_rule_after_user_growth(pie, oracle, book):
    """A wide batch keeps a 64-byte mask record per union bucket slot, (cap_users << shift) * 64 bytes with 16 << (shift - 4)
    slots per user, and gives up its union beyond 2 GiB: cap_users << shift > 33 554 432.  The ordinary batch is bound by
    (cap_users << shift) * 16 bytes <= 2 GiB and by 2048 tiles of users.  300 000 users loaded give cap_users = 300 000, and
    300 000 << 6 = 19 200 000 stays below.  One appended row of a NEW user doubles the user arrays: cap_users = 600 000, and
    600 000 << 4 = 9 600 000, << 5 = 19 200 000 (wide batches keep their union), << 6 = 38 400 000 (they do not), while
    38 400 000 * 16 B = 586 MiB and 1172 tiles leave the ordinary batch supported.  So: the wide batch before the growth and
    the ones at 16 and 32 slots keep their union; once a 33-row bucket has brought 64 slots, wide batches fall back, exactly,
    and a 64-query batch on the same table still returns its union."""
    U0 = 300000
    cols0, planted = T.plant_user_buckets(oracle.gen(11, N, 0, N, U0, D, 0), U0, D, oracle.T0_MS)
    U = U0 + 1
    extra = (np.array([oracle.T0_MS - 62 * DAY], np.int64), np.array([oracle.T0_MS + HOUR], np.int64), np.array([U0], np.int32), np.array([3], np.int32))
    try:
        book.put(U0, cols0, planted)
        book.put(U, tuple(np.concatenate([a, b]) for a, b in zip(cols0, extra)), planted)
        ctx = open_ctx(pie, cols0, U0, 1)
        try:
            assert one_wide(ctx, book, "wide before the growth", U0, planted, 0, 65, True)
            ctx.append_rows(*extra, U)
            for name, got, want in zip(("start", "end", "user", "disc"), ctx.read_columns(), book.table(U)[0]):
                assert np.array_equal(got, want), name
            assert one_wide(ctx, book, "wide at 16 slots", U, planted, 0, 65, True)
            one_batch(ctx, book, "17 rows", U, planted, 1, 16, "rerun", 1, which=[0, 15])
            assert one_wide(ctx, book, "wide at 32 slots", U, planted, 1, 300, True, True, U + 3)
            one_batch(ctx, book, "33 rows", U, planted, 2, 16, "rerun", 1, which=[0, 15])
            one_batch(ctx, book, "64 slots", U, planted, 3, 64, "union", 1, which=[0, 31, 32, 63])
            assert not one_wide(ctx, book, "wide at 64 slots", U, planted, 3, 300, False, True, U + 3)
            assert ctx.stats()["k1_variant"] == 0
            assert not one_wide(ctx, book, "wide at 64 slots, few rows", U, planted, 0, 65, False)
            one_batch(ctx, book, "batch after the wide fallback", U, planted, 3, 64, "union", 1, which=[0, 63])
        finally:
            ctx.close()
    finally:
        book.drop(U0)
        book.drop(U)


# ------------------------------------------------------------------------------------------------ 3. single scans
@pytest.mark.parametrize("U", [1048577, 3000000])
def test_single_scan_buckets_on_large_user_tables(pie, oracle, U):
    """Direct bucket slots with separate kernels (beyond 1 048 576 users), one user with 40 selected rows and one with 100.
    The scan is repeated: the capacity the first one asked for (128 slots, clamped so that the slots stay within 2 GiB: 64 at
    1 048 577 users, 32 at 3 000 000) is applied at the next begin, and the buckets that still do not fit keep taking the
    staged route.  Every repeat equals the oracle."""
    t0 = oracle.T0_MS
    s, e, u, d = [np.array(c) for c in oracle.gen(13, N, 0, N, U, D, 0)]
    rows = np.random.default_rng(5).permutation(N)[:140]
    for user, part in ((U - 1, rows[:40]), (70001, rows[40:])):
        u[part], e[part], d[part] = user, t0 + HOUR, np.arange(part.size) % D
        s[part] = t0 - 63 * DAY + (np.arange(part.size) % 4) * DAY
    now = t0 - 2 * HOUR
    want = oracle.scan(s, e, u, d, U, now, INT64_MIN, LIM)
    assert want[0][U - 1] == 40 and want[0][70001] == 100 and int(want[0].max()) == 100
    ctx = open_ctx(pie, (s, e, u, d), U, 1)
    try:
        work = []
        for rep in range(3):
            T.same(ctx.scan(now, INT64_MIN), want, ("single scan", U, "repeat", rep))
            st, info = ctx.stats(), ctx.table_info()
            assert st["max_bucket"] == 100 and st["users"] == U and st["selected"] == want[2].size, (U, rep, st)
            work.append(info["workspace_bytes"])
            for user in (U - 1, 70001, 0):
                assert np.array_equal(ctx.read_user_feed(user), want[2][want[1][user]:want[1][user + 1]]), (U, rep, user)
        # The slots grew once, at the second begin, and then stayed.  A bucket of 100 rows asks for 128 slots per user; 2 GiB hold
        # 64 per user at 1 048 577 users and 32 at 3 000 000 (table_model.union_slots_fit).  Every result slot's array grew from 16
        # slots to that, so the growth is a whole number of (users << shift) - 16 * users records, and no multiple of what one
        # shift more would have taken.
        shift = 6 if U == 1048577 else 5
        assert T.union_slots_fit(U, shift) and not T.union_slots_fit(U, shift + 1)
        assert work[0] < work[1] == work[2], work
        grown = work[1] - work[0]
        assert grown % (((U << shift) - 16 * U) * T.BUCKET_REC_BYTES) == 0, (work, "not the clamped capacity")
        assert grown % (((U << (shift + 1)) - 16 * U) * T.BUCKET_REC_BYTES) != 0, (work, "one shift too many")
        assert grown // (((U << shift) - 16 * U) * T.BUCKET_REC_BYTES) <= 4, work
        print("\nuser-axis single scans: U %d workspace MiB %s" % (U, [w >> 20 for w in work]))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 4. growth of the user table
class Growing:
    """524 200 users with a hot index in a context and in TableModel; appends and the readers that follow each of them.  The
    queries are those of stage 0 (at most 16 rows per bucket), so the union buckets stay at 16 slots and a wide batch keeps its
    union on the doubled user arrays: (2 * 524 200) << 4 slots * 64 B is half of 2 GiB."""
    U0 = 524200

    def __init__(self, pie, oracle):
        self.t0 = t0 = oracle.T0_MS
        cols, self.planted = T.plant_user_buckets(oracle.gen(17, N, 0, N, self.U0, D, 0), self.U0, D, t0)
        self.m = T.TableModel(oracle)
        self.m.load(*cols, self.U0, D)
        self.q16, self.q64, self.q200 = (T.user_axis_queries(t0, k, 0) for k in (16, 64, 200))
        self.ctx = open_ctx(pie, cols, self.U0, 1)

    def builds(self):
        return self.ctx.table_info()["hot_builds"]

    def columns(self, tag):
        ctx, m = self.ctx, self.m
        assert ctx.n == m.n and ctx.n_users == m.U, (tag, "shape")
        for name, got, want in zip(("start", "end", "user", "disc"), ctx.read_columns(), m.columns()):
            assert got.dtype == want.dtype and np.array_equal(got, want), (tag, "column " + name)

    def readers(self, tag):
        """a 16-query batch, a 64-query batch, a 200-query wide batch and a single scan against the model; which path answered"""
        ctx, m = self.ctx, self.m
        supported = T.batch_supported_users(m.U)
        paths = []
        # a condition the table meets, stated before the GPU is asked: no union bucket outgrows the 16 slots
        assert int(T.union_sizes(m.columns(), m.U, D, self.q200).max()) <= 16, tag
        for qs in (self.q16, self.q64):
            wants = m.scan_many(qs)
            ctx.scan_batch_begin(qs)
            hot_rows = ctx.table_info()["hot_rows"]
            ms = ctx.scan_batch_finish()
            assert list(ms) == [int(w[2].size) for w in wants], (tag, len(qs), "M per query")
            un = ctx.batch_read_union()
            assert (un is not None) == supported, (tag, len(qs), "union" if un is not None else "no union")
            assert (ctx.stats()["k1_variant"] != 0) == supported and (hot_rows > 0 or not supported), (tag, len(qs), hot_rows)
            if un is not None:
                T.check_union(tag, un, wants, False)
            for qi in (0, len(qs) // 2, len(qs) - 1):
                T.same(ctx.batch_read_results(qi), wants[qi], (tag, len(qs), "query", qi))
            for u in (m.U - 1, 0, self.U0 - 1):
                w = wants[0]
                assert np.array_equal(ctx.batch_read_user_feed(0, u), w[2][w[1][u]:w[1][u + 1]]), (tag, "batch feed", u)
            paths.append("batched" if supported else "fallback")
        wants = m.scan_many(self.q200)
        ctx.scan_wide_begin(self.q200)
        assert ctx.scan_wide_finish() == [int(w[2].size) for w in wants], (tag, "wide M per query")
        un = ctx.batch_read_union_wide()
        assert (un is not None) == supported, (tag, "wide union" if un is not None else "no wide union")
        if un is not None:
            T.check_union(tag, (un[0], un[1], un[2].reshape(-1)), wants, True)
        for qi in (0, 63, 64, 199):
            T.same(ctx.batch_read_results(qi), wants[qi], (tag, "wide query", qi))
        paths.append("wide_pass" if supported else "wide_fallback")
        q = self.q16[0]
        ctx.set_disciplines(q[2], D)
        want = m.scan(*q)
        T.same(ctx.scan(q[0], q[1]), want, (tag, "single scan"))
        for u in (m.U - 1, 0):
            assert np.array_equal(ctx.read_user_feed(u), want[2][want[1][u]:want[1][u + 1]]), (tag, "feed", u)
        ctx.set_disciplines(ALL, D)
        print("user-axis growth: %-28s U %7d -> %s, hot_builds %d" % (tag, m.U, paths, self.builds()))

    def append(self, tag, users, U):
        """one live row per user of `users` (starts tied in pairs), the table's user count raised to U"""
        k, t0 = len(users), self.t0
        s2 = (t0 - 62 * DAY + (np.arange(k) // 2) * HOUR).astype(np.int64)
        e2 = np.full(k, t0 + HOUR, np.int64)
        u2, d2 = np.array(users, np.int32), (np.arange(k) % D).astype(np.int32)
        self.ctx.append_rows(s2, e2, u2, d2, U)
        self.m.append_rows(s2, e2, u2, d2, U)
        self.columns(tag)


def test_user_table_grows_across_the_batch_boundary(pie, oracle):
    """A hand-written sequence against TableModel: 524 200 users with a hot index; appends bring 524 287, exactly 524 288,
    524 289 and then 2 096 801 users (one past twice the capacity of 1 048 400 that the first append left), with appends for
    existing users in between.  After every append the columns are compared bit for bit, a 16-query batch, a 64-query batch
    and a 200-query wide batch are compared with the model, and so are the feeds of the newest user and of user 0.  The
    batched pass and the wide pass answer up to 524 288 users and the fallback from 524 289 on.  The index is rebuilt by the
    batch after the append that reallocated; appends in place, also those that add a user within the arrays' capacity, are
    mirrored into the live index and rebuild nothing; from 524 289 users on no batched pass runs, so nothing is built either,
    whatever the append did."""
    g = Growing(pie, oracle)
    try:
        print()
        g.readers("loaded")
        builds = g.builds()
        assert builds >= 1 and g.ctx.table_info()["hot_rows"] > 0
        some = [u for u in sorted(g.planted) if g.planted[u] <= 9][:5] + [0, 12345]   # their buckets stay within 16 rows
        for tag, users, U, rebuilt in (
                ("new users, to 524 287", list(range(g.U0, 524287)), 524287, True),
                ("existing users, in place", some, 524287, False),
                ("a new user, to 524 288", [524287, 0], 524288, False),
                ("existing users, in place", some, 524288, False),
                ("a new user, to 524 289", [524288], 524289, False),
                ("existing users", some + [524288], 524289, False),
                ("a jump to 2 096 801", [2096800, 524289, 1048400, 0], 2096801, False)):
            g.append(tag, users, U)
            g.readers(tag)
            if rebuilt:
                assert g.builds() > builds, (tag, "the index was not rebuilt after the user table was reallocated")
            else:
                assert g.builds() == builds, (tag, "the index was rebuilt")
            builds = g.builds()
    finally:
        g.ctx.close()


def test_touches_and_delete_at_the_last_batched_size(pie, oracle):
    """The end of the sequence on a table grown to exactly 524 288 users (the user arrays reallocated, the index rebuilt): a
    set_end that tombstones rows of the hand-made users, one that revives half of them, and delete_user of the user with 64
    rows in the last tile; columns and readers against the model after each, the batched pass over the live index answering."""
    g = Growing(pie, oracle)
    try:
        print()
        g.readers("loaded")
        g.append("new users, to 524 288", list(range(g.U0, 524288)), 524288)
        g.readers("new users, to 524 288")
        builds, t0, m = g.builds(), g.t0, g.m
        hand = np.nonzero(np.isin(m.user, np.array(sorted(g.planted), np.int32)) & (m.end > t0))[0].astype(np.int32)
        for tag, rows, ne in (("tombstones", hand[::3], np.full(hand[::3].size, INT64_MIN)),
                              ("revived", hand[::6], np.full(hand[::6].size, t0 + 2 * HOUR))):
            g.ctx.set_end(rows, ne.astype(np.int64))
            m.set_end(rows, ne)
            g.columns(tag)
            g.readers(tag)
        victim = max(u for u in g.planted if g.planted[u] == 64)
        got, want = g.ctx.delete_user(victim), m.delete_user(victim)
        assert want.size and got.dtype == want.dtype and np.array_equal(got, want)
        g.columns("delete_user")
        g.readers("delete_user")
        assert g.builds() == builds and g.ctx.table_info()["hot_rows"] > 0, "touches of a few hundred rows rebuilt or dropped the index"
    finally:
        g.ctx.close()


# ------------------------------------------------------------------------------------------------ 5. the cross-feature chain
# Seeded chains of table_model.Chain (mutators and readers mixed, every reader against the model) with the user count
# overridden to the headline's and to the last batched size, on 300 007 rows, cut to seven steps so that a chain takes a few
# seconds.  One configuration each of (hot index on, no ordered run), (index off, no ordered run) and (ordered run always, one
# heavy user).  Seeds chosen on the MI355X so that together they reach the paths CHAIN_PATHS names.
CHAIN_CONFIGS = {"hot": {"hot": 1, "ordered": 0, "heavy": False}, "cold": {"hot": 0, "ordered": 0, "heavy": False},
                 "ordered": {"ordered": 2, "heavy": True}}
CHAINS = [("hot", 100003, 1), ("hot", 524288, 2), ("hot", 524288, 1), ("cold", 100003, 4), ("cold", 524288, 2), ("cold", 524288, 1),
          ("ordered", 100003, 1), ("ordered", 100003, 4), ("ordered", 524288, 1), ("ordered", 524288, 7)]
CHAIN_PATHS = ("hot_clean", "hot_delta", "keyed_1byte", "wide_pass", "ordered_batch")
CHAIN_REACHED = {}


@pytest.mark.parametrize("config,U,seed", CHAINS)
def test_chain_at_large_user_counts(pie, oracle, config, U, seed):
    ch = T.run_chain(pie, oracle, seed, dict(CHAIN_CONFIGS[config], n=N, U=U, steps=7))
    CHAIN_REACHED[(config, U, seed)] = dict(ch.paths)
    print("\nuser-axis chain: %-7s U %6d seed %d -> %s" % (config, U, seed, sorted(ch.paths)))


def test_chains_at_large_user_counts_reached_their_paths():
    missing = [c for c in CHAINS if c not in CHAIN_REACHED]
    assert not missing, "chains %s failed or were deselected: their path records are missing, run the whole file" % missing
    seen = {}
    for paths in CHAIN_REACHED.values():
        for p, k in paths.items():
            seen[p] = seen.get(p, 0) + k
    print("paths reached:", seen)
    assert not [p for p in CHAIN_PATHS if not seen.get(p)], "no checked call was answered by %s" % [p for p in CHAIN_PATHS if not seen.get(p)]
    for U in (100003, 524288):   # both sizes ran batches over the index and over the table, and a wide pass
        at = {p for c, paths in CHAIN_REACHED.items() if c[1] == U for p in paths}
        assert {"hot_clean", "keyed_1byte", "wide_pass"} <= at, (U, sorted(at))
