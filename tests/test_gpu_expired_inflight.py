"""GPU: the expired queue while scans and batches are in flight (pie_expired_queue_begin / _finish / _room and the shard pair)
against the oracle's expired queue (oracle/oracle_py.py), with pie_expired_queue on the idle context as a second witness.  Row
counts come from pie_expired_inflight_geometry: around a wave, a wave step and a unit, and several units with a ragged tail.
Every test has a context of its own (lanes, the ordered run and the pass's slot are context state)."""
import ctypes as C
import os

import numpy as np
import pytest

from table_model import same
from token_model import TokenModel

pytestmark = pytest.mark.gpu

U, D = 50, 8
MASK = (1 << D) - 1
NOW = 1700000000000
HOUR = 3600000
PREV = NOW - HOUR
END_NONE = -(2 ** 63)
PIE_E_INVAL, PIE_E_CAPACITY, PIE_E_STATE = -1, -5, -6
PATTERNS = ("none", "every", "last", "first", "alternating", "random")


def ctx_with_env(pie, **env):
    """A context created under the given environment; the environment is restored before returning."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pie.PieScan(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def new_ctx(pie, column="key", **env):
    """column = "key": the derived key columns are in step and the pass reads the 2-byte key; "end": a context that never takes
    the keyed forms (PIE_K1_KEYED=0), so the pass reads the end column."""
    if column == "end":
        env["PIE_K1_KEYED"] = "0"
    return ctx_with_env(pie, **env)


def row_counts(ctx):
    step, unit, _ = ctx.expired_inflight_geometry(1)
    assert step == 1024 and unit % step == 0 and unit >= step
    return [1, 63, 64, 65, step - 1, step + 1, unit - 1, unit + 1, 3 * unit + 777], unit


def ends(n, pattern, seed):
    """end[n] for the window (PREV, NOW]: rows outside it lie in the future, in the past, exactly at PREV (out), one past NOW (out,
    but on NOW's key) or are tombstones; the rows of `pattern` lie inside it, some exactly at NOW and at PREV + 1."""
    rng = np.random.default_rng(seed)
    e = NOW + 1 + rng.integers(0, 10 ** 9, n)
    for value, share in ((PREV, 16), (NOW + 1, 16), (END_NONE, 16), (None, 8)):
        at = rng.integers(0, n, max(n // share, 1))
        e[at] = PREV - rng.integers(0, 10 ** 9, at.size) if value is None else value
    hit = np.zeros(n, bool)
    if pattern == "every":
        hit[:] = True
    elif pattern == "last":
        hit[n - 1] = True
    elif pattern == "first":
        hit[0] = True
    elif pattern == "alternating":
        hit[::2] = True
    elif pattern == "random":
        hit = rng.random(n) < 0.03
    k = int(hit.sum())
    inside = rng.integers(PREV + 1, NOW + 1, k)
    inside[::3] = NOW
    inside[1::3] = PREV + 1
    e[hit] = inside
    return e.astype(np.int64)


def columns(e, seed=0):
    n = e.size
    rng = np.random.default_rng(seed + 1)
    start = (NOW - rng.integers(1, 10 ** 9, n)).astype(np.int64)
    return start, e, (np.arange(n) % U).astype(np.int32), rng.integers(0, D, n).astype(np.int32)


def load(ctx, e, seed=0):
    cols = columns(e, seed)
    ctx.load_columns(*cols, U)
    ctx.set_disciplines(MASK, D)
    return cols


def in_flight(ctx, oracle, e, prev=PREV, now=NOW, tag=""):
    want = oracle.expired_queue(e, prev, now)
    ctx.expired_queue_begin(prev, now)
    got = ctx.expired_queue_finish()
    assert got.dtype == np.int32 and np.array_equal(got, want), (tag, got.size, want.size)
    return got


def queries(seed, n_q):
    """clocks near the top of the tables' end range: a few per cent of the rows are live, so the batches take the batched pass
    (a query with a tenth of the table live is answered by a scan of its own)"""
    rng = np.random.default_rng(seed)
    return [(int(NOW + 93 * 10 ** 7 + rng.integers(0, 6 * 10 ** 7)), int(rng.choice([END_NONE, NOW - 5 * 10 ** 8])),
             MASK if q % 3 == 0 else int(rng.integers(1, MASK + 1))) for q in range(n_q)]


def queue_state(pie, ctx):
    try:
        return ctx.queue_info()
    except pie.PieError as err:
        return ("error", err.code)


@pytest.mark.parametrize("column", ["key", "end"])
def test_hit_patterns_at_every_row_count(pie, oracle, column):
    with new_ctx(pie, column) as ctx:
        sizes, _ = row_counts(ctx)
        if column == "key":
            load(ctx, ends(100, "random", 1))
            assert ctx.table_info()["has_keys"] == 1
        total = 0
        for n in sizes:
            for j, pattern in enumerate(PATTERNS):
                e = ends(n, pattern, 100 * n + j)
                load(ctx, e)
                got = in_flight(ctx, oracle, e, tag=(column, n, pattern))
                total += got.size
                assert np.array_equal(ctx.expired_queue(PREV, NOW), got), ("the idle witness", n, pattern)
                if pattern == "every":
                    assert got.size == n
                if pattern == "none":
                    assert got.size == 0
                if pattern == "last":
                    assert list(got) == [n - 1]
            # windows at exact end values, inside one key bucket, empty and inverted, and the widest there is
            k = int(e[n // 2]) if e[n // 2] != END_NONE else NOW
            for prev, now in ((k - 1, k), (k, k + 1), (k, k), (k - 1000, k + 1000), (5, 4), (NOW, PREV), (END_NONE, 2 ** 62), (END_NONE, k),
                              (k, 2 ** 63 - 1)):
                in_flight(ctx, oracle, e, prev, now, (column, n, "window", prev, now))
        assert total > 0


@pytest.mark.parametrize("column", ["key", "end"])
def test_waves_that_take_several_units(pie, oracle, column):
    """a grid of one block on a table of seven units: every wave walks two units, grid-stride"""
    with new_ctx(pie, column, PIE_EXPQ_MAX_BLOCKS="1") as ctx:
        _, unit = row_counts(ctx)
        n = 6 * unit + 333
        assert ctx.expired_inflight_geometry(n) == (1024, unit, 1)
        for pattern in ("alternating", "random", "last"):
            e = ends(n, pattern, 7)
            load(ctx, e)
            in_flight(ctx, oracle, e, tag=(column, pattern))


def test_capacity(pie, oracle):
    with new_ctx(pie) as ctx:
        sizes, unit = row_counts(ctx)
        n = sizes[-1]
        e = ends(n, "random", 3)
        load(ctx, e)
        want = oracle.expired_queue(e, PREV, NOW)
        q = want.size
        assert q > 100
        lib, h = ctx._lib, ctx._ctx
        out = np.full(q + 1, -7, np.int32)
        got_q = C.c_size_t(0)
        # exactly enough
        assert lib.pie_expired_queue_begin(h, PREV, NOW, q) == 0
        assert lib.pie_expired_queue_finish(h, out.ctypes.data_as(C.c_void_p), q, C.byref(got_q)) == 0
        assert got_q.value == q and np.array_equal(out[:q], want) and out[q] == -7
        # one too few: a true prefix, the length, and nothing behind the host copy
        out[:] = -7
        assert lib.pie_expired_queue_begin(h, PREV, NOW, q - 1) == 0
        assert lib.pie_expired_queue_finish(h, out.ctypes.data_as(C.c_void_p), q - 2, C.byref(got_q)) == PIE_E_INVAL
        assert ctx.expired_queue_room() == 0 and np.all(out == -7), "too little room consumes nothing"
        assert lib.pie_expired_queue_finish(h, out.ctypes.data_as(C.c_void_p), q - 1, C.byref(got_q)) == PIE_E_CAPACITY
        assert got_q.value == q and np.array_equal(out[: q - 1], want[: q - 1]) and out[q - 1] == -7 and out[q] == -7
        assert ctx.expired_queue_room() == 1, "the pass is consumed"
        ctx.expired_queue_begin(PREV, NOW, q - 1)
        with pytest.raises(pie.PieError) as ei:
            ctx.expired_queue_finish()
        assert ei.value.code == PIE_E_CAPACITY and ei.value.length == q and np.array_equal(ei.value.prefix, want[: q - 1])
        # a tiny buffer on a long queue: the kernel stores nothing past it (the rows behind it in the pass's buffer are the last pass's)
        ctx.expired_queue_begin(PREV, NOW, 3)
        with pytest.raises(pie.PieError) as ei:
            ctx.expired_queue_finish()
        assert ei.value.length == q and np.array_equal(ei.value.prefix, want[:3])
        # counting only
        ctx.expired_queue_begin(PREV, NOW, 0)
        assert ctx.expired_queue_finish() == q
        assert lib.pie_expired_queue_begin(h, PREV, NOW, 0) == 0
        assert lib.pie_expired_queue_finish(h, None, 0, C.byref(got_q)) == 0 and got_q.value == q
        # the whole queue again, and the pass's memory and time in pie_table_info
        assert np.array_equal(in_flight(ctx, oracle, e), want)
        ti = ctx.table_info()
        assert ti["expired_inflight_bytes"] >= 4 * n and ti["expired_inflight_ms"] > 0
        assert lib.pie_expired_queue_begin(h, PREV, NOW, 1 << 31) == PIE_E_INVAL and ctx.expired_queue_room() == 1


@pytest.mark.parametrize("kind", ["scan", "six", "wide", "ordered", "token"])
def test_begun_with_work_in_flight(pie, oracle, kind):
    with new_ctx(pie) as ctx:
        if kind == "ordered":
            ctx.set_ordered_run(2)
        ctx.set_batch_lanes(2 if kind == "six" else 3)
        sizes, unit = row_counts(ctx)
        n = sizes[-1]
        e = ends(n, "random", 11)
        s, e, u, d = load(ctx, e, 11)
        want_scan = oracle.scan(s, e, u, d, U, NOW, 0, MASK)
        same(ctx.scan(NOW, 0), want_scan, "the scan finished before the begin")   # (it also builds the ordered run)
        if kind == "token":
            keys = np.random.default_rng(5).integers(0, 2 ** 64, (n, 2), dtype=np.uint64)
            ctx.token_set(keys)
        batches = {"scan": [], "six": [queries(40 + b, 8) for b in range(6)], "wide": [queries(50, 70)], "ordered": [queries(60, 16)], "token": []}[kind]
        wants = [[oracle.scan(s, e, u, d, U, *q) for q in qs] for qs in batches]
        if kind == "scan":
            ctx.scan_begin(NOW - 1000, 0)
        for qs in batches:
            (ctx.scan_wide_begin if kind == "wide" else ctx.scan_batch_begin)(qs)
        if kind == "six":
            assert ctx.batch_room() == 0, "three batches on each of two lanes are in flight"
        if kind == "token":
            ctx.token_lookup_begin(keys[:300], NOW)
        before = queue_state(pie, ctx)
        if kind != "token":
            with pytest.raises(pie.PieError) as ei:      # the synchronous call keeps its rule
                ctx.expired_queue(PREV, NOW)
            assert ei.value.code == PIE_E_STATE
            before = queue_state(pie, ctx)
        assert ctx.expired_queue_room() == 1
        in_flight(ctx, oracle, e, tag=kind)
        in_flight(ctx, oracle, e, PREV - 5 * HOUR, NOW + 10 ** 8, (kind, "a wide window"))
        ctx.expired_queue_begin(PREV, NOW, 0)
        assert ctx.expired_queue_finish() == oracle.expired_queue(e, PREV, NOW).size
        assert queue_state(pie, ctx) == before, "the queue pie_queue_info knows is as it was"
        if kind == "token":
            same(ctx.read_results(), want_scan, "the finished result that stood before the begin")
            got = ctx.token_lookup_finish()
            assert np.array_equal(got["row"], np.arange(300)) and np.array_equal(got["live"], (e[:300] > NOW).astype(np.uint8))
            # a queue the synchronous call left on the device stands through a pass
            standing = ctx.expired_queue(PREV - 5 * HOUR, NOW, fetch=False)
            ctx.token_lookup_begin(keys[:10], NOW)
            assert queue_state(pie, ctx) == (1, standing, 0) and standing > 0
            in_flight(ctx, oracle, e, tag="beside a standing queue")
            assert queue_state(pie, ctx) == (1, standing, 0)
            ctx.token_lookup_finish()
        if kind == "scan":
            want = oracle.scan(s, e, u, d, U, NOW - 1000, 0, MASK)
            assert ctx.scan_finish() == want[2].shape[0]
            same(ctx.read_results(), want, "the scan that was in flight")
        for b, want in enumerate(wants):
            ms = ctx.scan_wide_finish() if kind == "wide" else list(ctx.scan_batch_finish())
            assert [int(x) for x in ms] == [int(w[2].size) for w in want], (kind, "batch", b)
            for qi, w in enumerate(want):
                same(ctx.batch_read_results(qi), w, (kind, "batch", b, "query", qi))
        if kind == "ordered":
            assert ctx.stats()["k1_variant"] & 0x2000, "the batch did not run on the ordered run"
        if kind in ("six", "wide"):
            assert ctx.stats()["k1_variant"] & 0x1000, "the batches did not take the batched pass"
        in_flight(ctx, oracle, e, tag=(kind, "with nothing in flight"))


def test_ordering_against_mutators(pie, oracle):
    with new_ctx(pie, PIE_ASYNC_MUTATIONS="1") as ctx:
        sizes, unit = row_counts(ctx)
        n = unit + 1
        e = ends(n, "random", 21)
        s, e, u, d = load(ctx, e, 21)
        # a touch and an append queued right before the begin, with no wait: both are seen
        moved = np.nonzero(e > NOW + 1)[0][:40].astype(np.int32)
        ctx.set_end(moved, np.full(moved.size, NOW, np.int64))
        e[moved] = NOW
        more = ends(500, "alternating", 22)
        ms, me, mu, md = columns(more, 22)
        ctx.append_rows(ms, me, mu, md, U)
        e = np.concatenate([e, me])
        got = in_flight(ctx, oracle, e, tag="queued mutations")
        assert np.isin(moved, got).all() and (got >= n).sum() == 250
        # a touch issued between begin and finish is not seen by this queue, and is seen by the next
        want = oracle.expired_queue(e, PREV, NOW)
        ctx.expired_queue_begin(PREV, NOW)
        gone = want[:25].astype(np.int32)
        ctx.set_end(gone, np.full(gone.size, END_NONE, np.int64))
        assert np.array_equal(ctx.expired_queue_finish(), want)
        e[gone] = END_NONE
        got = in_flight(ctx, oracle, e, tag="after the touch")
        assert not np.isin(gone, got).any()
        # a new table between begin and finish: the old table's queue
        want = oracle.expired_queue(e, PREV, NOW)
        ctx.expired_queue_begin(PREV, NOW)
        e2 = ends(777, "every", 23)
        load(ctx, e2)
        assert np.array_equal(ctx.expired_queue_finish(), want)
        in_flight(ctx, oracle, e2, tag="the new table")
        # growth of the capacity in an append between begin and finish
        want = oracle.expired_queue(e2, PREV, NOW)
        ctx.expired_queue_begin(PREV, NOW)
        big = ends(4000, "alternating", 24)
        ctx.append_rows(*columns(big, 24), U)
        assert np.array_equal(ctx.expired_queue_finish(), want)
        in_flight(ctx, oracle, np.concatenate([e2, big]), tag="after the growth")


@pytest.mark.parametrize("change", ["load", "append", "compact"])
def test_both_side_passes_begun_under_a_table_change(pie, oracle, change):
    """an expired queue and two token lookups are begun, then the table is replaced, outgrown or renumbered under all three: each
    finish gives the old table's answer (the oracle's queue, the dict model's rows), and a fresh begin / finish of each sees
    the new table"""
    def lookup_is(got, want, tag):
        assert np.array_equal(got["row"], want["row"]) and np.array_equal(got["live"], want["live"]), tag
        f = want["found"]
        for col in ("user", "start", "end"):
            assert np.array_equal(got[col][f], want[col][f]), (tag, col)

    with new_ctx(pie) as ctx:
        _, unit = row_counts(ctx)
        n = unit + 1
        e = ends(n, "random", 51)
        cols = load(ctx, e, 51)
        model = TokenModel(*cols)
        keys = np.random.default_rng(52).integers(0, 2 ** 64, (n + 600, 2), dtype=np.uint64)
        ctx.token_set(keys[:n])
        model.token_set(keys[:n])
        asks = (keys[:n:37], np.concatenate([keys[n - 300:n], keys[n:n + 40]]))     # the second: the last rows and keys no row has
        clocks = (NOW, PREV)
        want_queue = oracle.expired_queue(e, PREV, NOW)
        want_rows = [{k: np.array(v) for k, v in model.lookup(a, t).items()} for a, t in zip(asks, clocks)]
        assert want_queue.size > 100 and all(w["found"].any() and w["live"].any() for w in want_rows) and not want_rows[1]["found"].all()
        ctx.expired_queue_begin(PREV, NOW)
        for a, t in zip(asks, clocks):
            ctx.token_lookup_begin(a, t)
        assert ctx.expired_queue_room() == 0 and ctx.token_lookup_room() == 2
        if change == "load":
            e = ends(777, "every", 53)
            cols = load(ctx, e, 53)
            model = TokenModel(*cols)
        elif change == "append":
            more = ends(500, "alternating", 54)
            grow = columns(more, 54)
            ctx.append_rows(*grow, U)
            model.append_rows(*grow)
            e = np.concatenate([e, more])
        else:
            assert (e == END_NONE).sum() > 100
            assert ctx.compact_rows() == (e != END_NONE).sum()
            new_of_old = model.compact()
            e = e[e != END_NONE]
        assert np.array_equal(ctx.expired_queue_finish(), want_queue), (change, "the old table's queue")
        for i, want in enumerate(want_rows):
            lookup_is(ctx.token_lookup_finish(), want, (change, "the old table's rows, lookup", i))
        assert ctx.expired_queue_room() == 1 and ctx.token_lookup_room() == 4
        # afterwards: the new table
        if change == "load":
            keys = np.random.default_rng(55).integers(0, 2 ** 64, (777, 2), dtype=np.uint64)
            ctx.token_set(keys)
            model.token_set(keys)
            asks = (keys[::5], keys[700:])
        elif change == "append":
            ctx.token_append(keys[n:n + 500])
            model.token_append(keys[n:n + 500])
        assert np.array_equal(model.end, e)
        in_flight(ctx, oracle, e, tag=(change, "the new table's queue"))
        for i, (a, t) in enumerate(zip(asks, clocks)):
            ctx.token_lookup_begin(a, t)
            got = ctx.token_lookup_finish()
            lookup_is(got, model.lookup(a, t), (change, "the new table's rows, lookup", i))
            if change == "append" and i == 1:
                assert np.array_equal(got["row"][300:], np.arange(n, n + 40)), "the keys no row had name the appended rows"
            if change == "compact" and i == 0:
                assert np.array_equal(got["row"], new_of_old[::37]) and not np.array_equal(got["row"], want_rows[0]["row"])


def test_state_rules(pie, oracle):
    with new_ctx(pie) as ctx:
        lib, h = ctx._lib, ctx._ctx
        q = C.c_size_t(9)
        assert lib.pie_expired_queue_begin(h, PREV, NOW, 4) == PIE_E_STATE, "no table"
        assert ctx.expired_queue_room() == 1
        e = ends(300, "alternating", 31)
        load(ctx, e)
        assert lib.pie_expired_queue_finish(h, None, 0, C.byref(q)) == PIE_E_STATE, "none begun"
        assert lib.pie_shard_expired_queue_begin(h, PREV, NOW, 4) == PIE_E_STATE, "the shard form on a plain context"
        assert ctx.expired_queue_room() == 1
        ctx.expired_queue_begin(PREV, NOW)
        assert ctx.expired_queue_room() == 0
        assert lib.pie_expired_queue_begin(h, PREV, NOW, 4) == PIE_E_STATE, "a second begin"
        assert lib.pie_shard_expired_queue_finish(h, None, 0, C.byref(q)) == PIE_E_STATE, "the other form's finish"
        assert ctx.expired_queue_room() == 0
        assert np.array_equal(ctx.expired_queue_finish(), oracle.expired_queue(e, PREV, NOW))
        assert ctx.expired_queue_room() == 1
        # an empty table: an empty queue
        ctx.load_columns(*(c[:0] for c in columns(e)), 1)
        ctx.expired_queue_begin(PREV, NOW, 8)
        assert ctx.expired_queue_room() == 0
        assert ctx.expired_queue_finish().size == 0 and ctx.expired_queue_room() == 1


@pytest.mark.parametrize("world", [2, 3])
def test_shard_form(pie, oracle, world):
    sizes = None
    ctxs = []
    try:
        for r in range(world):
            ctxs.append(new_ctx(pie))
        sizes, unit = row_counts(ctxs[0])
        n = 2 * unit + 55
        e = ends(n, "random", 41 + world)
        s, e, u, d = columns(e, 41)

        def whole(tag):
            parts = []
            for c in ctxs:
                c.shard_expired_queue_begin(PREV, NOW)
                with pytest.raises(pie.PieError) as ei:
                    c.expired_queue_finish()
                assert ei.value.code == PIE_E_STATE
                parts.append(c.shard_expired_queue_finish())
            got = np.sort(np.concatenate(parts))
            assert np.array_equal(got, oracle.expired_queue(e, PREV, NOW)), tag
            assert sum(p.size for p in parts) == got.size and all(p.size for p in parts)

        for r, c in enumerate(ctxs):
            c.set_batch_lanes(3)
            c.load_columns(s, e, u, d, U)
            c.shard_table(r, world)
            c.set_disciplines(MASK, D)
            c.scan_batch_begin(queries(70 + r, 4))
        whole("with a batch in flight on every shard")
        for c in ctxs:
            c.scan_batch_finish()
        more = ends(900, "alternating", 45)
        ms, me, mu, md = columns(more, 45)
        for c in ctxs:
            c.shard_append_rows(ms, me, mu, md, U)
        e = np.concatenate([e, me])
        whole("after shard_append_rows")
        dead = np.nonzero(e == END_NONE)[0]
        assert dead.size > 0
        for c in ctxs:
            before = c.n
            c.compact_rows()
            assert c.n < before
        whole("after a compaction that dropped the tombstones")
    finally:
        for c in ctxs:
            c.close()
