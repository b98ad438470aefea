"""GPU: pie_delete_users (deleteSessionsForUser for a set of users in one table pass) is K calls of pie_delete_user in array
order: two contexts with one table, one deleted id by id, one in one call, must agree on everything derived from the table and
both must answer like the numpy model; then the edges of the row axis and of the user axis, the contract of the call, and the
sharded form.  The inputs are tests/delete_users_cases.py; test_delete_users_cpu.py proves on the model that none is vacuous."""
import ctypes as C

import numpy as np
import pytest

import delete_users_cases as cases
from compact_model import CompactModel
from table_model import ALL, DAY, HOUR, INT64_MIN, ctx_with_env, same, shard_view

pytestmark = pytest.mark.gpu

PIE_E_CAPACITY, PIE_E_STATE = -5, -6


@pytest.fixture(scope="module")
def twin_tables(oracle):
    return {c[0]: c for c in cases.twin_cases(oracle)}


def hot_state(pie, ctx):
    try:
        return ctx.hot_layout()
    except pie.PieError as e:
        assert e.code == PIE_E_STATE
        return None


def hot_canon(h):
    """hot_layout without the one thing the code does not decide: which delta slot a moved row took (an atomic cursor)."""
    pos, m = h["pos"], h["n_main"]
    return (np.array([m]), h["off"], h["user"], h["row"], h["bin"], np.where(pos >= m, m, pos), np.sort(pos[pos >= m]))


def queries_for(m, rng, k):
    live = np.sort(m.end[m.end != INT64_MIN])
    out = []
    for _ in range(k):
        now = int(live[int(rng.integers(0, live.size))]) + int(rng.integers(-2, 3))
        cutoff = INT64_MIN if rng.random() < 0.5 else int(np.median(m.start))
        out.append((now, cutoff, int(rng.integers(1, 2 ** 32)) | (1 << int(rng.integers(0, min(m.D, 32))))))
    return out


def check_against_model(tag, ctx, m, keys, key_rows, rng):
    """single scan, 16- and 64-query batches, a wide batch, both queues and a token lookup, all against the model"""
    q1, q16, q64, q70 = (queries_for(m, rng, k) for k in (1, 16, 64, 70))
    now, cutoff, mask = q1[0]
    ctx.set_disciplines(mask, m.D)
    same(ctx.scan(now, cutoff), m.scan(now, cutoff, mask), (tag, "single scan"))
    ctx.set_disciplines(ALL, m.D)
    for qs, call in ((q16, ctx.scan_batch), (q64, ctx.scan_batch), (q70, ctx.scan_wide)):
        for qi, (got, want) in enumerate(zip(call(qs), m.scan_many(qs))):
            same(got, want, (tag, "batch of", len(qs), "query", qi))
    live = np.sort(m.end[m.end != INT64_MIN])
    lo, hi = int(live[live.size // 3]), int(live[(4 * live.size) // 5])
    assert np.array_equal(ctx.expired_queue(lo, hi), m.expired_queue(lo, hi)), (tag, "expired queue")
    a_now = int(np.median(m.start)) + 12 * HOUR
    assert np.array_equal(ctx.archive_queue(a_now), m.archive_queue(a_now, 12 * HOUR)), (tag, "archive queue")
    got = ctx.token_lookup(keys, hi)
    assert np.array_equal(got["row"], key_rows), (tag, "token rows")
    assert np.array_equal(got["live"], (m.end[key_rows] > hi).astype(np.uint8)), (tag, "token liveness")
    assert np.array_equal(got["end"], m.end[key_rows]), (tag, "token end")


@pytest.mark.parametrize("hot,ordered,wide_ordered", ((0, 0, 0), (1, 0, 0), (0, 2, 0), (1, 2, 0), (1, 2, 1)),
                         ids=("plain", "hot", "ordered", "hot_ordered", "hot_ordered_wide"))
@pytest.mark.parametrize("table", ("lattice", "tie", "seeded"))
def test_twin(pie, oracle, twin_tables, table, hot, ordered, wide_ordered):
    case = twin_tables[table]
    name, s, e, u, d, U, D, ids = case
    cases.check_case(oracle, case)
    rng = np.random.default_rng(5)
    tok = rng.integers(1, 2 ** 63, (s.size, 2)).astype(np.uint64)
    m = cases.model_of(oracle, case)
    ctxs = [ctx_with_env(pie, hot, 1) for _ in range(2)]
    try:
        for c in ctxs:
            c.set_ordered_run(ordered)
            c.set_wide_ordered(wide_ordered)
            c.load_columns(s, e, u, d, U)
            c.set_disciplines(ALL, D)
            c.token_set(tok)
            live = np.sort(m.end[m.end != INT64_MIN])   # a top-of-range batch: builds the hot index / the ordered run where there is one
            c.scan_batch([(int(live[live.size - 1 - 3 * q]) - 1, INT64_MIN, 0xFFFFFFFF) for q in range(16)])
        one, many = ctxs
        singles, union, per = cases.expected(m, ids)
        got_singles = [one.delete_user(int(x)) for x in ids]
        rows, got_per = many.delete_users(ids)
        for x, (g, w) in zip(ids, zip(got_singles, singles)):
            assert np.array_equal(g, w), (name, "single list of", x)
        assert rows.dtype == np.int32 and np.array_equal(rows, union), (name, "list")
        assert np.array_equal(got_per, per), (name, "per-user counts")
        ca, cb = one.read_columns(), many.read_columns()
        for a, b, w in zip(ca, cb, m.columns()):
            assert np.array_equal(a, b) and np.array_equal(a, w), (name, "columns")
        ha, hb = hot_state(pie, one), hot_state(pie, many)
        assert (ha is None) == (hb is None), (name, "one context has a hot index, the other none")
        assert (ha is not None) == bool(hot), (name, "the top-of-range batch builds the hot index wherever it is enabled")
        if ha is not None:
            for a, b in zip(hot_canon(ha), hot_canon(hb)):
                assert np.array_equal(a, b), (name, "hot index")
        keep = np.nonzero(m.end != INT64_MIN)[0]
        key_rows = np.concatenate([union[:: max(1, union.size // 40)], keep[:: max(1, keep.size // 40)]]).astype(np.int32)
        for which, c in zip(("singles", "one call"), ctxs):
            check_against_model((name, which), c, m, tok[key_rows], key_rows, np.random.default_rng(7))
    finally:
        for c in ctxs:
            c.close()


def run_case(pie, oracle, case, kind="mixed"):
    name, s, e, u, d, U, D, ids = case
    cases.check_case(oracle, case, kind)
    m = cases.model_of(oracle, case)
    _, union, per = cases.expected(m, ids)
    with pie.PieScan(0) as ctx:
        ctx.load_columns(s, e, u, d, U)
        rows, got_per = ctx.delete_users(ids)
        assert np.array_equal(rows, union), (name, "list")
        assert np.array_equal(got_per, per) and int(got_per.sum()) == rows.size, (name, "per-user counts")
        for a, w in zip(ctx.read_columns(), m.columns()):
            assert np.array_equal(a, w), (name, "columns")
        ctx.set_disciplines(ALL, D)
        same(ctx.scan(oracle.T0_MS, INT64_MIN), m.scan(oracle.T0_MS, INT64_MIN, ALL), (name, "scan"))
        again, per2 = ctx.delete_users(ids)
        assert again.size == 0 and not per2.any(), (name, "a second call found rows")


def test_row_axis(pie, oracle):
    for case, kind in cases.row_axis_cases(oracle):
        run_case(pie, oracle, case, kind)


def test_row_axis_empty_list(pie, oracle):
    (case, _), = [c for c in cases.row_axis_cases(oracle) if c[0][0] == "rows_1025"]
    _, s, e, u, d, U, D, _ = case
    with pie.PieScan(0) as ctx:
        ctx.load_columns(s, e, u, d, U)
        rows, per = ctx.delete_users(np.zeros(0, np.int32))
        assert rows.size == 0 and per.size == 0
        assert np.array_equal(ctx.read_columns()[1], e)


def test_user_axis(pie, oracle):
    for case in cases.user_axis_cases(oracle):
        run_case(pie, oracle, case)


# ------------------------------------------------------------------------------------------------ the contract
def raw_delete_users(pie, ctx, ids, cap):
    ids = np.ascontiguousarray(ids, np.int32)
    rows, per, k = np.full(max(cap, 1), -7, np.int32), np.full(ids.size, -7, np.int32), C.c_size_t(99)
    rc = pie.load_library().pie_delete_users(ctx._ctx, ids.ctypes.data_as(C.c_void_p), ids.size, rows.ctypes.data_as(C.c_void_p), cap,
                                             C.byref(k), per.ctypes.data_as(C.c_void_p))
    return rc, rows, int(k.value), per


def test_capacity_too_small(pie, oracle, twin_tables):
    case = twin_tables["seeded"]
    _, s, e, u, d, U, D, ids = case
    m = cases.model_of(oracle, case)
    _, union, per = cases.expected(m, ids)
    with pie.PieScan(0) as ctx:
        ctx.load_columns(s, e, u, d, U)
        rc, rows, k, got_per = raw_delete_users(pie, ctx, ids, union.size - 1)
        assert rc == PIE_E_CAPACITY and k == union.size and np.array_equal(got_per, per)
        assert np.array_equal(ctx.read_columns()[1], m.end), "the rows were not tombstoned"
        rc, rows, k, got_per = raw_delete_users(pie, ctx, ids, union.size)
        assert rc == 0 and k == 0 and not got_per.any()
        lib = pie.load_library()
        assert lib.pie_delete_users(ctx._ctx, None, 3, None, 0, None, None) == -1
        assert lib.pie_delete_users(ctx._ctx, None, 0, None, 0, None, None) == 0


def test_scan_in_flight_is_refused(pie, oracle, twin_tables):
    _, s, e, u, d, U, D, ids = twin_tables["seeded"]
    with pie.PieScan(0) as ctx:
        ctx.load_columns(s, e, u, d, U)
        ctx.set_disciplines(ALL, D)
        ctx.scan_begin(oracle.T0_MS, INT64_MIN)
        with pytest.raises(pie.PieError) as ei:
            ctx.delete_users(ids)
        assert ei.value.code == PIE_E_STATE
        ctx.scan_finish()
        assert np.array_equal(ctx.read_columns()[1], e), "a refused call changed the table"


def test_queued_append_then_delete_growth_and_compaction(pie, oracle, twin_tables):
    case = twin_tables["seeded"]
    _, s, e, u, d, U, D, ids = case
    m = CompactModel(oracle)
    m.load(s, e, u, d, U, D)
    ctx = ctx_with_env(pie, 1, 1)
    try:
        ctx.load_columns(s, e, u, d, U)
        top = int(s.max())

        def rows_of(users, t):
            k = len(users)
            st = (top + t * 1000 + np.arange(k)).astype(np.int64)
            return st, st + 5 * HOUR, np.asarray(users, np.int32), np.arange(k, dtype=np.int32) % D

        first = rows_of([1, 2, 3], 1)          # outgrows the capacity: waited for, makes room
        ctx.append_rows(*first, U)
        m.append_rows(*first, U)
        second = rows_of([5, 6, 96, 5], 2)     # in place: queued, not waited for
        ctx.append_rows(*second, U)
        m.append_rows(*second, U)
        n_before = m.n
        _, union, per = cases.expected(m, ids)
        rows, got_per = ctx.delete_users(ids)
        assert {n_before - 4, n_before - 2, n_before - 1} <= set(rows.tolist()), "the rows just appended stayed"
        assert np.array_equal(rows, union) and np.array_equal(got_per, per)
        # the user table grows: the new highest id is deletable
        grown = rows_of([U + 2, 4, U + 2], 3)
        ctx.append_rows(*grown, U + 3)
        m.append_rows(*grown, U + 3)
        want = m.delete_user(U + 2)
        rows, got_per = ctx.delete_users([U + 3, U + 2])
        assert want.size == 2 and np.array_equal(rows, want) and got_per.tolist() == [0, 2]
        for a, w in zip(ctx.read_columns(), m.columns()):
            assert np.array_equal(a, w)
        m.compact_rows()
        assert ctx.compact_rows() == m.n
        for a, w in zip(ctx.read_columns(), m.columns()):
            assert np.array_equal(a, w), "compaction after delete_users"
        ctx.set_disciplines(ALL, D)
        same(ctx.scan(top, INT64_MIN), m.scan(top, INT64_MIN, ALL), "scan after compaction")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ sharded
@pytest.mark.parametrize("world", (1, 2, 3, 5))
def test_sharded(pie, oracle, twin_tables, world):
    case = twin_tables["seeded"]
    _, s, e, u, d, U, D, ids = case
    m = cases.model_of(oracle, case)
    owner = np.array([oracle.shard_of(x, world) for x in range(U)], np.int32)
    _, union, per = cases.expected(m, ids)
    got_rows, got_per = [], np.zeros(len(ids), np.int32)
    for rank in range(world):
        with pie.PieScan(0) as ctx:
            ctx.load_columns(s, e, u, d, U)
            ctx.shard_table(rank, world)
            rows, p = ctx.shard_delete_users(ids)
            view, held, _ = shard_view(m, rank, owner)
            assert np.all(np.diff(rows) > 0) and np.all(np.isin(rows, held)), (rank, "rows of another shard")
            for i, x in enumerate(ids):
                if not (0 <= x < U and owner[x] == rank):
                    assert p[i] == 0, (rank, "an id of another shard counted", x)
            for a, w in zip(ctx.read_columns(), view.columns()):
                assert np.array_equal(a, w), (rank, "columns")
            got_rows.append(rows)
            got_per += p
    assert np.array_equal(np.sort(np.concatenate(got_rows)), union)
    assert np.array_equal(got_per, per)


def test_unsharded_context_is_refused(pie, oracle, twin_tables):
    _, s, e, u, d, U, D, ids = twin_tables["seeded"]
    with pie.PieScan(0) as ctx:
        ctx.load_columns(s, e, u, d, U)
        with pytest.raises(pie.PieError) as ei:
            ctx.shard_delete_users(ids)
        assert ei.value.code == PIE_E_STATE
        with pytest.raises(pie.PieError):
            ctx.shard_delete_user(3)
