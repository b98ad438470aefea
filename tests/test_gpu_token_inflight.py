"""GPU: token lookups while scans and batches are in flight (pie_token_lookup_begin / _finish / _room) against the dict model of
tests/token_model.py, with the per-key clock applied on top of it as end > now[i]; the scans and batches that were in flight are
held against the oracle afterwards.  Tables are a few thousand rows, batch lanes are pinned to 3, every test has a context of
its own (lanes, the ordered run and the lookup slots are context state)."""
import ctypes as C

import numpy as np
import pytest

from table_model import check_union, same
from token_model import END_NONE, TokenModel

pytestmark = pytest.mark.gpu

N, U, D = 3000, 50, 8
NOW = 1700000000000
MASK = (1 << D) - 1
PIE_E_INVAL, PIE_E_CAPACITY, PIE_E_STATE = -1, -5, -6
KS = (1, 255, 256, 257, 1000)          # around the blocks of a 256-thread launch


def columns(seed, n=N):
    rng = np.random.default_rng(seed)
    start = NOW - rng.integers(1, 10 ** 9, n)
    end = NOW + rng.integers(-5 * 10 ** 8, 5 * 10 ** 8, n)
    end[rng.integers(0, n, 8)] = NOW
    return start.astype(np.int64), end.astype(np.int64), rng.integers(0, U, n).astype(np.int32), rng.integers(0, D, n).astype(np.int32)


def random_keys(seed, n):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (n, 2), dtype=np.uint64)


def new_ctx(pie, seed, ordered=None):
    """-> (context with 3 lanes, the table of `seed` and keys for every row; its model; the keys)"""
    ctx = pie.PieScan(0)
    if ordered is not None:
        ctx.set_ordered_run(ordered)
    ctx.set_batch_lanes(3)
    cols = columns(seed)
    ctx.load_columns(*cols, U)
    ctx.set_disciplines(MASK, D)
    model = TokenModel(*cols)
    keys = random_keys(seed + 1000, N)
    ctx.token_set(keys)
    model.token_set(keys)
    return ctx, model, keys


def snapshot(model, keys, now):
    """the model's answer, per-key clock included, as arrays that later changes of the model leave alone"""
    now = np.broadcast_to(np.asarray(now, np.int64), (np.asarray(keys).reshape(-1, 2).shape[0],))
    return {k: np.array(v) for k, v in model.lookup(keys, now).items()}


def check_answer(got, want, tag=""):
    assert got["row"].shape == want["row"].shape, tag
    assert np.array_equal(got["row"], want["row"]), (tag, "row")
    assert np.array_equal(got["live"], want["live"]), (tag, "live")
    f = want["found"]
    for col in ("user", "start", "end"):
        assert np.array_equal(got[col][f], want[col][f]), (tag, col)


def in_flight(ctx, model, keys, now, tag=""):
    want = snapshot(model, keys, now)
    ctx.token_lookup_begin(keys, now)
    got = ctx.token_lookup_finish()
    check_answer(got, want, tag)
    return got


def tombstone(ctx, model, rows):
    ctx.set_end(rows, np.full(len(rows), END_NONE))
    model.end[rows] = END_NONE


def mixed(model, keys, k, seed):
    """k keys and clocks: present, absent, one key repeated, keys of tombstoned rows, and clocks at end - 1, end, end + 1"""
    rng = np.random.default_rng(seed)
    alive = np.nonzero(model.end != END_NONE)[0]
    tomb = np.nonzero(model.end == END_NONE)[0]
    assert tomb.size > 0
    ask = np.empty((k, 2), np.uint64)
    now = np.full(k, NOW, np.int64)
    absent = random_keys(seed + 1, k)
    rep = keys[alive[0]]
    for i in range(k):
        kind = i % 8 if k > 1 else 5
        r = int(rng.choice(alive))
        if kind == 1:
            ask[i] = absent[i]
        elif kind == 2:
            ask[i] = rep
        elif kind == 3:
            ask[i] = keys[int(rng.choice(tomb))]
        elif kind in (4, 5, 6):
            ask[i] = keys[r]
            now[i] = model.end[r] + (kind - 5)
        else:
            ask[i] = keys[r]
            if kind == 7:
                now[i] = NOW + int(rng.integers(-5 * 10 ** 8, 5 * 10 ** 8))
    return ask, now


def queries(seed, n_q):
    rng = np.random.default_rng(seed)
    return [(int(NOW + rng.integers(-10 ** 8, 10 ** 8)), int(rng.choice([-(2 ** 63), NOW - 5 * 10 ** 8])),
             MASK if q % 3 == 0 else int(rng.integers(1, MASK + 1))) for q in range(n_q)]


def oracle_answers(oracle, model, qs):
    return [oracle.scan(model.start, model.end, model.user, model.disc, U, now, cutoff, mask) for now, cutoff, mask in qs]


def check_finished_batch(ctx, ms, wants, wide, tag):
    assert [int(x) for x in ms] == [int(w[2].size) for w in wants], (tag, "M per query")
    un = ctx.batch_read_union_wide() if wide else ctx.batch_read_union()
    if un is not None:
        check_union(tag, un, wants, wide)
    for qi, w in enumerate(wants):
        same(ctx.batch_read_results(qi), w, (tag, "query", qi))


def lookups_of_every_size(ctx, model, keys, seed):
    live_seen = 0
    for j, k in enumerate(KS):
        ask, now = mixed(model, keys, k, seed + 10 * j)
        got = in_flight(ctx, model, ask, now, ("k", k))
        live_seen += int(got["live"].sum())
        if k >= 8:   # the clock is the key's own: end - 1 is live, end and end + 1 are not
            assert list(got["live"][4:7]) == [1, 0, 0] and np.all(got["row"][1::8] == -1) and np.all(got["live"][3::8] == 0)
            assert np.all(got["row"][2::8] == got["row"][2])
    assert live_seen > 0
    # several begun before any is finished, scalar clock
    asks = [mixed(model, keys, k, seed + 100 + k)[0] for k in (3, 257, 64)]
    wants = [snapshot(model, a, NOW + 7) for a in asks]
    for a in asks:
        ctx.token_lookup_begin(a, NOW + 7)
    for w in wants:
        check_answer(ctx.token_lookup_finish(), w, "three begun together")


def test_single_scan_in_flight(pie, oracle):
    ctx, model, keys = new_ctx(pie, 31)
    with ctx:
        tombstone(ctx, model, np.arange(5, N, 97))
        ctx.scan_begin(NOW, 0)
        ask, now = mixed(model, keys, 300, 32)
        got = in_flight(ctx, model, ask, now)
        assert 0 < got["live"].sum() < 300
        with pytest.raises(pie.PieError) as ei:          # the synchronous call keeps its rule
            ctx.token_lookup(ask, NOW)
        assert ei.value.code == PIE_E_STATE
        m = ctx.scan_finish()
        want = oracle.scan(model.start, model.end, model.user, model.disc, U, NOW, 0, MASK)
        assert m == want[2].shape[0]
        same(ctx.read_results(), want, "the scan that was in flight")


@pytest.mark.parametrize("kind", ["nine", "wide", "ordered"])
def test_batches_in_flight(pie, oracle, kind):
    ctx, model, keys = new_ctx(pie, 33, ordered=2 if kind == "ordered" else None)
    with ctx:
        tombstone(ctx, model, np.arange(3, N, 61))
        if kind == "nine":
            batches = [queries(40 + b, 8) for b in range(9)]
        elif kind == "wide":
            batches = [queries(50, 70)]
        else:
            batches = [queries(60, 16)]
        wants = [oracle_answers(oracle, model, qs) for qs in batches]
        if kind == "ordered":   # a finished scan builds the run the batch then takes
            same(ctx.scan(NOW, 0), oracle.scan(model.start, model.end, model.user, model.disc, U, NOW, 0, MASK), "the scan that builds the run")
        for qs in batches:
            (ctx.scan_wide_begin if kind == "wide" else ctx.scan_batch_begin)(qs)
        if kind == "nine":
            assert ctx.batch_room() == 0, "nine batches on three lanes are in flight"
        lookups_of_every_size(ctx, model, keys, 70)
        for b, (qs, want) in enumerate(zip(batches, wants)):
            ms = ctx.scan_wide_finish() if kind == "wide" else list(ctx.scan_batch_finish())
            check_finished_batch(ctx, ms, want, kind == "wide", (kind, "batch", b))
        if kind == "ordered":
            assert ctx.stats()["k1_variant"] & 0x2000, "the batch did not run on the ordered run"
        in_flight(ctx, model, keys[:100], NOW, "with nothing in flight")


def test_slot_rules(pie):
    ctx, model, keys = new_ctx(pie, 35)
    with ctx:
        lib, h = ctx._lib, ctx._ctx
        ks = (5, 0, 300, 1)
        ctx.scan_batch_begin(queries(36, 4))
        assert ctx.token_lookup_room() == 4
        wants = []
        for i, k in enumerate(ks):
            ask = keys[100 * i: 100 * i + k]
            wants.append(snapshot(model, ask, NOW))
            ctx.token_lookup_begin(ask, NOW)
            assert ctx.token_lookup_room() == 3 - i
        with pytest.raises(pie.PieError) as ei:
            ctx.token_lookup_begin(keys[:1], NOW)
        assert ei.value.code == PIE_E_STATE and ctx.token_lookup_room() == 0
        # the oldest has 5 keys: too little room leaves it finishable
        k_out = C.c_size_t(99)
        row = np.full(5, -7, np.int32)
        assert lib.pie_token_lookup_finish(h, row.ctypes.data_as(C.c_void_p), None, None, None, None, 4, C.byref(k_out)) == PIE_E_CAPACITY
        assert k_out.value == 5 and ctx.token_lookup_room() == 0 and np.all(row == -7)
        assert lib.pie_token_lookup_finish(h, row.ctypes.data_as(C.c_void_p), None, None, None, None, 5, C.byref(k_out)) == 0
        assert k_out.value == 5 and np.array_equal(row, wants[0]["row"]) and ctx.token_lookup_room() == 1
        for k, want in zip(ks[1:], wants[1:]):          # in begin order; the second one is the lookup of no keys
            got = ctx.token_lookup_finish()
            assert got["row"].shape == (k,)
            check_answer(got, want, ("k", k))
        assert ctx.token_lookup_room() == 4
        assert lib.pie_token_lookup_finish(h, None, None, None, None, None, 0, None) == PIE_E_STATE
        with pytest.raises(pie.PieError) as ei:
            ctx.token_lookup_finish()
        assert ei.value.code == PIE_E_STATE
        # every output pointer may be NULL; k = 0 takes and returns a slot, NULL pointers and all
        assert lib.pie_token_lookup_begin(h, None, None, 0) == 0 and ctx.token_lookup_room() == 3
        assert lib.pie_token_lookup_finish(h, None, None, None, None, None, 0, C.byref(k_out)) == 0 and k_out.value == 0
        assert ctx.token_lookup_room() == 4
        nows = np.full(3, NOW, np.int64)
        kp, np_ = keys[:3].ctypes.data_as(C.c_void_p), nows.ctypes.data_as(C.c_void_p)
        assert lib.pie_token_lookup_begin(h, None, np_, 3) == PIE_E_INVAL
        assert lib.pie_token_lookup_begin(h, kp, None, 3) == PIE_E_INVAL
        assert lib.pie_token_lookup_begin(h, kp, np_, 1 << 31) == PIE_E_INVAL
        assert ctx.token_lookup_room() == 4
        assert lib.pie_token_lookup_begin(h, kp, np_, 3) == 0
        assert lib.pie_token_lookup_finish(h, None, None, None, None, None, 3, None) == 0
        # the shard form on a context that is not sharded
        with pytest.raises(pie.PieError) as ei:
            ctx.shard_token_lookup_begin(keys[:2], NOW)
        assert ei.value.code == PIE_E_STATE
        ctx.scan_batch_finish()
    with pie.PieScan(0) as bare:                       # no table; a table without a column
        with pytest.raises(pie.PieError) as ei:
            bare.token_lookup_begin(keys[:2], NOW)
        assert ei.value.code == PIE_E_STATE
        bare.load_columns(*columns(37), U)
        with pytest.raises(pie.PieError) as ei:
            bare.token_lookup_begin(keys[:2], NOW)
        assert ei.value.code == PIE_E_STATE and bare.token_lookup_room() == 4


def test_order_against_mutations(pie):
    ctx, model, keys = new_ctx(pie, 38)
    with ctx:
        more_keys = random_keys(39, 300)
        grow = columns(40, 200)                       # the growing append: from here on appends are in place
        ctx.append_rows(*grow, U)
        ctx.token_append(more_keys[:200])
        model.append_rows(*grow)
        model.token_append(more_keys[:200])
        in_flight(ctx, model, more_keys[:200], NOW, "after the growing append")
        # append + token_append + set_end, then at once the lookup: it sees all three
        new = columns(41, 10)
        touched = np.array([7, 1200, N + 3, N + 205], np.int32)
        vals = np.array([NOW + 12345, END_NONE, NOW - 1, NOW + 99], np.int64)
        ctx.append_rows(*new, U)
        ctx.token_append(more_keys[200:210])
        ctx.set_end(touched, vals)
        ask = np.concatenate([more_keys[195:210], keys[[7, 1200, 8]]])
        ctx.token_lookup_begin(ask, NOW)
        model.append_rows(*new)
        model.token_append(more_keys[200:210])
        model.end[touched] = vals
        got = ctx.token_lookup_finish()
        check_answer(got, snapshot(model, ask, NOW), "behind three queued mutations")
        assert np.array_equal(got["row"][:15], np.arange(N + 195, N + 210)) and got["end"][15] == NOW + 12345 and got["end"][16] == END_NONE
        # a lookup, then a touch and a delete of what it looks up, then its finish: the answer from before them
        victim = int(model.user[50])
        rows_u = np.nonzero((model.user == victim) & (model.end != END_NONE))[0]
        ask = keys[np.concatenate([[50, 51, 52], rows_u[:20]])]
        before = snapshot(model, ask, NOW - 10 ** 9)
        ctx.token_lookup_begin(ask, NOW - 10 ** 9)
        ctx.set_end([51, 52], [NOW + 777, END_NONE])
        deleted = ctx.delete_user(victim)
        model.end[[51, 52]] = [NOW + 777, END_NONE]
        rows_u = np.nonzero((model.user == victim) & (model.end != END_NONE))[0]
        assert np.array_equal(deleted, rows_u)
        model.end[rows_u] = END_NONE
        check_answer(ctx.token_lookup_finish(), before, "mutated behind its begin")
        assert before["live"][0] == 1 and before["end"][1] != NOW + 777
        after = in_flight(ctx, model, ask, NOW - 10 ** 9, "the lookup after them")
        assert after["live"][0] == 0 and after["end"][1] == NOW + 777 and after["end"][2] == END_NONE


def test_replacement_under_an_unfinished_lookup(pie):
    ctx, model, keys = new_ctx(pie, 42)
    with ctx:
        # compaction that drops rows: the answer in the old row ids, with the old values
        tombstone(ctx, model, np.arange(0, N, 3))
        ask = keys[::7]
        before = snapshot(model, ask, NOW)
        ctx.token_lookup_begin(ask, NOW)
        kept = ctx.compact_rows()
        new_of_old = model.compact()
        assert kept == model.start.shape[0] < N
        check_answer(ctx.token_lookup_finish(), before, "compacted under it")
        fresh = in_flight(ctx, model, ask, NOW, "after the compaction")
        assert np.array_equal(fresh["row"], new_of_old[::7]) and not np.array_equal(fresh["row"], before["row"])
        # an index rebuild inside token_append
        ctx.token_set(keys[:400])
        model.token_set(keys[:400])
        assert ctx.token_layout()[1] == 1024
        ask = keys[300:700]
        before = snapshot(model, ask, NOW)
        ctx.token_lookup_begin(ask, NOW)
        ctx.token_append(keys[400:600])                # covered passes half of 1024 slots
        model.token_append(keys[400:600])
        check_answer(ctx.token_lookup_finish(), before, "the index rebuilt under it")
        assert np.all(before["row"][100:] == -1)
        fresh = in_flight(ctx, model, ask, NOW, "after the rebuild")
        assert np.all(fresh["row"][:300] >= 0) and ctx.token_layout()[1] == 2048
        # a new table
        ask = keys[:600]
        before = snapshot(model, ask, NOW)
        ctx.token_lookup_begin(ask, NOW)
        cols = columns(43, 2000)
        ctx.load_columns(*cols, U)
        check_answer(ctx.token_lookup_finish(), before, "a new table loaded under it")
        with pytest.raises(pie.PieError) as ei:          # the load dropped the column
            ctx.token_lookup_begin(ask, NOW)
        assert ei.value.code == PIE_E_STATE
        model = TokenModel(*cols)
        keys2 = random_keys(44, 2000)
        ctx.token_set(keys2)
        model.token_set(keys2)
        in_flight(ctx, model, np.concatenate([keys2[::5], keys[:50]]), NOW, "the new table")


def test_staging_growth(pie):
    ctx, model, keys = new_ctx(pie, 45)
    with ctx:
        ctx.scan_batch_begin(queries(46, 8))
        small = keys[10:40]
        big = keys[np.random.default_rng(47).integers(0, N, 1 << 17)]
        big[::5] = random_keys(48, big[::5].shape[0])
        now_big = NOW + np.random.default_rng(49).integers(-5 * 10 ** 8, 5 * 10 ** 8, 1 << 17)
        want_small, want_big = snapshot(model, small, NOW), snapshot(model, big, now_big)
        ctx.token_lookup_begin(small, NOW)
        ctx.token_lookup_begin(big, now_big)           # outgrows its slot's staging while the small one is unfinished
        check_answer(ctx.token_lookup_finish(), want_small, "the small lookup")
        check_answer(ctx.token_lookup_finish(), want_big, "2^17 keys")
        ctx.scan_batch_finish()


def test_synchronous_calls_are_undisturbed(pie):
    ctx, model, keys = new_ctx(pie, 50)
    with ctx:
        ctx.scan_batch_begin(queries(51, 8))
        in_flight(ctx, model, np.concatenate([keys[:500], random_keys(52, 200)]), NOW)
        ctx.scan_batch_finish()
        got, want = ctx.token_lookup(keys, NOW), model.lookup(keys, NOW)
        check_answer(got, {k: np.asarray(v) for k, v in want.items()}, "token_lookup")
        new_end = np.full(40, NOW + 4242, np.int64)
        rows = ctx.token_set_end(keys[:40], new_end, NOW)
        assert np.array_equal(rows, model.token_set_end(keys[:40], new_end, NOW))
        assert np.array_equal(ctx.read_columns()[1], model.end)
        cov, slots, slot_row, back = ctx.token_layout()
        assert cov == N and slots == pie.token_slots_for(N) and np.array_equal(back, keys)
        assert np.array_equal(np.sort(slot_row[slot_row >= 0]), np.arange(N))
        in_flight(ctx, model, keys[:64], NOW, "and again")
