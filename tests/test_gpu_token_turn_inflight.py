"""GPU: token turns while scans and batches are in flight (pie_token_turn_begin / _finish / _room and the shard forms) against
tests/turn_model.py, the executable form of pie_token_turn's rules, and the oracle: what was begun before a turn answers for the
table before it, what was begun after it for the table behind it, whenever the turn is finished.  Tables have 20 000 rows and 300
users (the size at which tests/test_gpu_token_turn.py gets a hot index), batch lanes are pinned to 3, and every test has a context
of its own (lanes, the hot index and the turn slots are context state)."""
import ctypes as C

import numpy as np
import pytest

from table_model import check_union, ctx_with_env, same
from token_model import END_NONE
from turn_model import DELETE, GET, TOUCH, TurnModel, make_ops, same_turn

pytestmark = pytest.mark.gpu

N, U, D = 20_000, 300, 32
SEED = 0x5EED5EED
LIM = (1 << D) - 1
HOUR, DAY = 3600 * 1000, 86400 * 1000
PIE_E_INVAL, PIE_E_CAPACITY, PIE_E_STATE = -1, -5, -6


def random_keys(seed, n):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (n, 2), dtype=np.uint64)


def queries(oracle, first, n_q):
    """n_q sparse queries around T0 - 6 h, as bench.py's: the rows with the largest `end` are the ones they find live"""
    t0 = oracle.T0_MS
    return [(t0 - 6 * HOUR - 977 * q - (q % 5) * HOUR, t0 - (61 + q % 4) * DAY, (0x55555555, 0xAAAAAAAA, LIM)[q % 3])
            for q in range(first, first + n_q)]


def new_ctx(pie, oracle, seed, hot=True, n=N, users=U):
    """-> (context with 3 lanes, a generated table, a key per row, warmed so that batches keep their unions; model; keys)"""
    ctx = ctx_with_env(pie, hot, 1)
    ctx.set_batch_lanes(3)
    cols = oracle.gen(SEED + seed, n, 0, n, users, D, 0)
    ctx.load_columns(*cols, users)
    ctx.set_disciplines(LIM, D)
    model = TurnModel(*cols)
    keys = random_keys(seed + 1000, n)
    ctx.token_set(keys)
    model.token_set(keys)
    for _ in range(2):                       # the union buckets and the wide slots grow to what these queries need
        ctx.scan_batch(queries(oracle, 0, 16))
        ctx.scan_wide(queries(oracle, 0, 100))
    return ctx, model, keys


def answers(oracle, model, qs, users=U):
    return [oracle.scan(model.start, model.end, model.user, model.disc, users, now, cutoff, mask) for now, cutoff, mask in qs]


def check_finished_batch(ctx, ms, wants, wide, tag):
    assert [int(x) for x in ms] == [int(w[2].size) for w in wants], (tag, "M per query")
    un = ctx.batch_read_union_wide() if wide else ctx.batch_read_union()
    if un is not None:
        check_union(tag, un, wants, wide)
    for qi, w in enumerate(wants):
        same(ctx.batch_read_results(qi), w, (tag, "query", qi))


def moving_turn(oracle, model, keys, seed):
    """A turn of touches and deletes on rows the queries select: 60 live rows touched out of every query's reach, 60 deleted, 60
    expired rows deleted (no effect on a feed), 60 rows touched up inside the live range.  -> (ops, rows out, rows deleted)"""
    t0 = oracle.T0_MS
    rng = np.random.default_rng(seed)
    top = rng.permutation(np.argsort(model.end, kind="stable")[-240:])
    low = rng.permutation(np.nonzero((model.end < t0 - 30 * DAY) & (model.end != END_NONE))[0])[:60]
    out, gone, up = top[:60], top[60:120], top[120:180]
    ops = np.concatenate([
        make_ops(keys[out], model.end[out] - 1, TOUCH, t0 - rng.integers(1, 20, 60) * DAY),
        make_ops(keys[gone], t0, DELETE),
        make_ops(keys[low], t0, DELETE),
        make_ops(keys[up], model.end[up] - 1, TOUCH, t0 + rng.integers(1, 6 * HOUR, 60)),
        make_ops(keys[out[:10]], t0, GET),
    ])
    return ops, out, gone


def membership_changes(wants_before, wants_after, out, gone):
    """the CPU model itself says the turn matters: a touched row and a deleted row leave some query's list"""
    sel_before = np.unique(np.concatenate([w[2] for w in wants_before]))
    sel_after = np.unique(np.concatenate([w[2] for w in wants_after]))
    assert np.intersect1d(sel_before, out).size > 0 and np.intersect1d(sel_after, out).size == 0, "no touched row changes membership"
    assert np.intersect1d(sel_before, gone).size > 0 and np.intersect1d(sel_after, gone).size == 0, "no deleted row leaves"
    assert any(not np.array_equal(b[2], a[2]) for b, a in zip(wants_before, wants_after))


def columns_match(ctx, model):
    assert np.array_equal(ctx.read_columns()[1], model.end), "end"


def test_nothing_in_flight_equals_the_synchronous_turn(pie, oracle):
    ctx, model, keys = new_ctx(pie, oracle, 1)
    twin, _, _ = new_ctx(pie, oracle, 1)
    with ctx, twin:
        assert ctx.table_info()["hot_rows"] > 0, "the table has no hot index"
        for rep in range(2):
            ops, _, _ = moving_turn(oracle, model, keys, 10 + rep)
            ctx.token_turn_begin(ops)
            got, sync, want = ctx.token_turn_finish(), twin.token_turn(ops), model.turn(ops)
            same_turn(got, want, ("in flight", rep))
            for col in ("row", "live", "user", "start", "end"):
                assert np.array_equal(got[col], sync[col]), (rep, col)
            assert np.array_equal(ctx.read_columns()[1], twin.read_columns()[1])
            columns_match(ctx, model)
            a, b = ctx.hot_layout(), twin.hot_layout()
            assert a["n_main"] == b["n_main"] and all(np.array_equal(a[k], b[k]) for k in ("off", "user", "row", "bin", "pos"))
        assert ctx.table_info()["hot_builds"] == twin.table_info()["hot_builds"] == 1


def test_six_batches_over_three_lanes(pie, oracle):
    ctx, model, keys = new_ctx(pie, oracle, 2)
    with ctx:
        assert ctx.table_info()["hot_rows"] > 0
        batches = [queries(oracle, 8 * b, 8) for b in range(12)]
        before = [answers(oracle, model, qs) for qs in batches[:6]]
        for qs in batches[:6]:                       # two per lane, no flush: the second of each lane has its tail riding
            ctx.scan_batch_begin(qs)
        ops, out, gone = moving_turn(oracle, model, keys, 20)
        assert ctx.token_turn_room() == 4
        ctx.token_turn_begin(ops)
        assert ctx.token_turn_room() == 3
        want_turn = model.turn(ops)
        after = [answers(oracle, model, qs) for qs in batches[6:]]
        membership_changes(before[0] + before[5], answers(oracle, model, batches[0] + batches[5]), out, gone)
        begun = 6
        for b in range(12):                          # nine at most in flight: the last six are begun as room appears
            while begun < 12 and ctx.batch_room() > 0:
                ctx.scan_batch_begin(batches[begun])
                begun += 1
            ms = list(ctx.scan_batch_finish())
            check_finished_batch(ctx, ms, before[b] if b < 6 else after[b - 6], False, ("batch", b, "before" if b < 6 else "after"))
        same_turn(ctx.token_turn_finish(), want_turn, "finished last")
        assert ctx.token_turn_room() == 4
        columns_match(ctx, model)
        assert ctx.table_info()["hot_builds"] == 1, "the turn was mirrored into the index"


def test_wide_batch_in_flight(pie, oracle):
    ctx, model, keys = new_ctx(pie, oracle, 3)
    with ctx:
        wide_qs, qs = queries(oracle, 0, 100), queries(oracle, 3, 16)
        before = [answers(oracle, model, wide_qs), answers(oracle, model, qs)]
        ctx.scan_wide_begin(wide_qs)
        ctx.scan_batch_begin(qs)
        ops, out, gone = moving_turn(oracle, model, keys, 30)
        ctx.token_turn_begin(ops)
        want_turn = model.turn(ops)
        ctx.scan_batch_begin(qs)
        ctx.scan_wide_begin(wide_qs)
        after = [answers(oracle, model, qs), answers(oracle, model, wide_qs)]
        membership_changes(before[0], after[1], out, gone)
        same_turn(ctx.token_turn_finish(), want_turn, "finished first")
        for tag, wants, wide in (("wide before", before[0], True), ("batch before", before[1], False), ("batch after", after[0], False),
                                 ("wide after", after[1], True)):
            check_finished_batch(ctx, ctx.scan_wide_finish(), wants, wide, tag)
        columns_match(ctx, model)


def test_single_scans_in_flight(pie, oracle):
    ctx, model, keys = new_ctx(pie, oracle, 4)
    with ctx:
        now, cutoff, mask = queries(oracle, 0, 1)[0]
        ctx.set_disciplines(mask, D)
        before = answers(oracle, model, [(now, cutoff, mask)])
        ctx.scan_begin(now, cutoff)
        ops, out, gone = moving_turn(oracle, model, keys, 40)
        ctx.token_turn_begin(ops)
        want_turn = model.turn(ops)
        ctx.scan_begin(now, cutoff)
        after = answers(oracle, model, [(now, cutoff, mask)])
        membership_changes(before, after, out, gone)
        assert ctx.scan_finish() == before[0][2].size
        same(ctx.read_results(), before[0], "the scan begun before the turn")
        assert ctx.scan_finish() == after[0][2].size
        same(ctx.read_results(), after[0], "the scan begun after the turn")
        same_turn(ctx.token_turn_finish(), want_turn)
        columns_match(ctx, model)


def test_four_turns_back_to_back(pie, oracle):
    ctx, model, keys = new_ctx(pie, oracle, 5)
    with ctx:
        t0 = oracle.T0_MS
        live = np.nonzero(model.end > t0)[0][:40]
        share = keys[live]
        turns = [
            np.concatenate([make_ops(share, t0, TOUCH, t0 + 5 * HOUR), make_ops(share[:3], t0, TOUCH, t0 + 7 * HOUR)]),   # repeats tokens
            make_ops(share, t0 + 6 * HOUR, GET),                    # sees turn 1: the first three live, the rest expired
            make_ops(share[::2], t0, DELETE),
            make_ops(share, t0, TOUCH, t0 + 9 * HOUR),              # a no-op on what turn 3 deleted
        ]
        ctx.scan_batch_begin(queries(oracle, 0, 8))
        for i, ops in enumerate(turns):
            assert ctx.token_turn_room() == 4 - i
            ctx.token_turn_begin(ops)
        assert ctx.token_turn_room() == 0
        with pytest.raises(pie.PieError) as ei:
            ctx.token_turn_begin(turns[0])
        assert ei.value.code == PIE_E_STATE and ctx.token_turn_room() == 0
        wants = [model.turn(ops) for ops in turns]            # the model's sequential replay
        assert wants[1]["live"][:3].all() and not wants[1]["live"][3:].any()
        assert not wants[3]["live"][::2].any() and wants[3]["live"][1::2].all()
        for i, want in enumerate(wants):                      # strictly in begin order: the sizes alone tell them apart
            got = ctx.token_turn_finish()
            assert got["row"].shape[0] == turns[i].shape[0]
            same_turn(got, want, ("turn", i))
            assert ctx.token_turn_room() == i + 1
        ctx.scan_batch_finish()
        columns_match(ctx, model)


def mixed_turn(model, keys, seed, k):
    """k get / touch / delete ops, each with a clock of its own on both sides of the rows' ends: about 20 % name keys the table does
    not hold, about 10 % name the token of an earlier op of the turn (chains form)"""
    rng = np.random.default_rng(seed)
    tok = keys[rng.choice(keys.shape[0], k, replace=False)]
    unknown = rng.random(k) < 0.2
    tok[unknown] = random_keys(seed + 500, int(unknown.sum()))
    for i in np.nonzero(rng.random(k) < 0.1)[0][1:]:
        tok[i] = tok[rng.integers(0, i)]
    clock = int(np.median(model.end[model.end != END_NONE]))
    now = clock + rng.integers(-40 * DAY, 40 * DAY, k)
    kind = rng.choice([GET, TOUCH, DELETE], k, p=[0.5, 0.3, 0.2])
    return make_ops(tok, now, kind, np.where(kind == TOUCH, now + rng.integers(1, 40 * DAY, k), 0))


def test_turn_staging_growth(pie, oracle):
    ctx, model, keys = new_ctx(pie, oracle, 8)
    with ctx:
        for i in range(4):                           # every slot has been used: each owns a first block (256 KiB, about 3 700 ops)
            ctx.token_turn_begin(make_ops(keys[i:i + 1], oracle.T0_MS, GET))
            ctx.token_turn_finish()
        bytes_before = ctx.table_info()["token_bytes"]
        qs = queries(oracle, 0, 8)
        before = answers(oracle, model, qs)
        ctx.scan_batch_begin(qs)
        small, big = mixed_turn(model, keys, 80, 30), mixed_turn(model, keys, 81, 8192)
        names = np.unique(big["tok"], axis=0).shape[0]
        assert 0.05 * 8192 < 8192 - names < 0.15 * 8192, "about a tenth of the ops repeat a token"
        ctx.token_turn_begin(small)
        ctx.token_turn_begin(big)                    # outgrows its slot's block while the small turn is unfinished
        want_small, want_big = model.turn(small), model.turn(big)
        assert 0.15 * 8192 < np.count_nonzero(~want_big["found"]) < 0.25 * 8192 and 0 < want_big["live"].sum() < names
        assert all(np.any((big["kind"] == kind) & (want_big["row"] >= 0)) for kind in (GET, TOUCH, DELETE))
        same_turn(ctx.token_turn_finish(), want_small, "the small turn")
        same_turn(ctx.token_turn_finish(), want_big, "8 192 ops")
        check_finished_batch(ctx, list(ctx.scan_batch_finish()), before, False, "the batch begun before the turns")
        columns_match(ctx, model)
        assert ctx.table_info()["token_bytes"] > bytes_before, "no slot grew"


def test_order_against_the_side_passes(pie, oracle):
    ctx, model, keys = new_ctx(pie, oracle, 6)
    with ctx:
        t0 = oracle.T0_MS
        rows = np.nonzero(model.end > t0)[0][:50]
        ask = keys[rows]

        def lookup_answer():
            return {k: np.array(v) for k, v in model.lookup(ask, np.full(50, t0, np.int64)).items()}

        window = (t0 + 20 * DAY, t0 + 21 * DAY)               # nothing ends here until the turn touches rows into it
        assert np.count_nonzero((model.end > window[0]) & (model.end <= window[1])) == 0
        ctx.scan_batch_begin(queries(oracle, 0, 8))
        lk_before = lookup_answer()
        ctx.token_lookup_begin(ask, t0)
        ctx.expired_queue_begin(*window)
        ops = np.concatenate([make_ops(ask[:25], t0, TOUCH, window[0] + 1 + np.arange(25)), make_ops(ask[25:], t0, DELETE)])
        ctx.token_turn_begin(ops)
        want_turn = model.turn(ops)
        ctx.token_lookup_begin(ask, t0)
        lk_after = lookup_answer()
        got = ctx.token_lookup_finish()
        assert np.array_equal(got["end"], lk_before["end"]) and got["live"].all(), "the lookup begun before the turn"
        got = ctx.token_lookup_finish()
        assert np.array_equal(got["end"], lk_after["end"]) and np.array_equal(got["live"], lk_after["live"]), "the lookup begun after it"
        assert got["live"][:25].all() and not got["live"][25:].any()
        assert ctx.expired_queue_finish().size == 0, "the queue begun before the turn"
        ctx.expired_queue_begin(*window)
        assert np.array_equal(ctx.expired_queue_finish(), np.sort(rows[:25])), "the queue begun after it"
        same_turn(ctx.token_turn_finish(), want_turn)
        ctx.scan_batch_finish()
        columns_match(ctx, model)


def test_refusals_change_nothing(pie, oracle):
    ctx, model, keys = new_ctx(pie, oracle, 7, hot=False)
    with ctx:
        lib, h = ctx._lib, ctx._ctx
        t0 = oracle.T0_MS
        layout = ctx.token_layout()

        def unchanged():
            columns_match(ctx, model)
            now = ctx.token_layout()
            assert now[:2] == layout[:2] and np.array_equal(now[2], layout[2]) and np.array_equal(now[3], layout[3])

        def code(fn, *a):
            with pytest.raises(pie.PieError) as ei:
                fn(*a)
            return ei.value.code

        live = np.nonzero(model.end > t0)[0][:8]
        ops = make_ops(keys[live], t0, TOUCH, t0 + 3 * HOUR)
        bad = ops.copy()
        bad["kind"][5] = 3
        ctx.scan_batch_begin(queries(oracle, 0, 8))
        assert code(ctx.token_turn_begin, bad) == PIE_E_INVAL
        bad["kind"][5], bad["reserved"][2] = TOUCH, 1
        assert code(ctx.token_turn_begin, bad) == PIE_E_INVAL
        assert lib.pie_token_turn_begin(h, None, 4) == PIE_E_INVAL and ctx.token_turn_room() == 4
        assert code(ctx.shard_token_turn_begin, ops) == PIE_E_STATE, "the shard form on a context that is not sharded"
        assert code(ctx.token_turn_finish) == PIE_E_STATE, "finish with none begun"
        ctx.scan_batch_finish()
        unchanged()
        # a turn begun: the synchronous mutators are refused, cap < k leaves it finishable
        ctx.token_turn_begin(ops)
        want = model.turn(ops)
        assert code(ctx.token_turn, ops) == PIE_E_STATE
        assert code(ctx.set_end, live[:2].astype(np.int32), np.full(2, END_NONE)) == PIE_E_STATE
        assert code(ctx.token_set_end, keys[live], np.full(8, t0), t0) == PIE_E_STATE
        k_out = C.c_size_t(99)
        row = np.full(8, -7, np.int32)
        assert lib.pie_token_turn_finish(h, row.ctypes.data_as(C.c_void_p), None, None, None, None, 7, C.byref(k_out)) == PIE_E_CAPACITY
        assert k_out.value == 8 and np.all(row == -7) and ctx.token_turn_room() == 3
        same_turn(ctx.token_turn_finish(), want, "after cap < k")
        assert ctx.token_turn_room() == 4
        layout = ctx.token_layout()
        unchanged()
        # every output pointer may be NULL; k = 0 takes and returns a slot
        assert lib.pie_token_turn_begin(h, None, 0) == 0 and ctx.token_turn_room() == 3
        assert lib.pie_token_turn_finish(h, None, None, None, None, None, 0, C.byref(k_out)) == 0 and k_out.value == 0
        unchanged()
        # an ordered run that is valid
        ctx.set_ordered_run(2)
        ctx.scan(t0 - 6 * HOUR, t0 - 61 * DAY)
        assert ctx.table_info()["ordered_rows"] > 0
        assert code(ctx.token_turn_begin, ops) == PIE_E_STATE and ctx.token_turn_room() == 4
        unchanged()
        same_turn(ctx.token_turn(ops), model.turn(ops), "the synchronous turn serves such a table")
    with pie.PieScan(0) as bare:                       # no table; a table without a column
        assert code(bare.token_turn_begin, ops) == PIE_E_STATE
        bare.load_columns(model.start, model.end, model.user, model.disc, U)
        assert code(bare.token_turn_begin, ops) == PIE_E_STATE and bare.token_turn_room() == 4


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_contexts(pie, oracle, world):
    """every shard is given the same turn with two batches in flight: it answers the ops whose key it holds as the unsharded
    model does, in GLOBAL ids, and the others -1 / live 0 / PIE_END_NONE (the unsharded TurnModel with the owner of every user:
    the model of tests/shard_token_model.py with the turn's rules on top)"""
    n, users = 8_000, 120
    cols = oracle.gen(SEED + 8, n, 0, n, users, D, 0)
    owner = np.array([oracle.shard_of(u, world) for u in range(users)], np.int32)
    keys = random_keys(8, n)
    t0 = oracle.T0_MS
    ctxs = []
    try:
        for r in range(world):
            c = pie.PieScan(0)
            ctxs.append(c)
            c.set_batch_lanes(3)
            c.load_columns(*cols, users)
            c.shard_table(r, world)
            c.set_disciplines(LIM, D)
            c.shard_token_set(keys)
            c.scan_batch(queries(oracle, 0, 8))
            c.scan_batch(queries(oracle, 0, 8))
        model = TurnModel(*cols)
        model.token_set(keys)
        ops, out, gone = moving_turn(oracle, model, keys, 80)
        ops = np.concatenate([ops, make_ops(random_keys(81, 5), t0, GET)])
        qs = [queries(oracle, 0, 8), queries(oracle, 8, 8)]
        pre = TurnModel(model.start, model.end.copy(), model.user, model.disc)
        want = model.turn(ops)
        holder = np.where(want["found"], owner[np.where(want["found"], want["user"], 0)], -1)
        for r, c in enumerate(ctxs):
            rows_g, users_g = c.shard_maps()
            local_user = np.full(users, -1, np.int32)
            local_user[users_g[:c.n_users]] = np.arange(c.n_users)

            def shard_answers(m, q):
                return [oracle.scan(m.start[rows_g], m.end[rows_g], local_user[m.user[rows_g]], m.disc[rows_g], c.n_users, *x) for x in q]

            c.scan_batch_begin(qs[0])
            c.scan_batch_begin(qs[1])
            c.shard_token_turn_begin(ops)
            c.scan_batch_begin(qs[0])
            for tag, w in (("before", shard_answers(pre, qs[0])), ("before", shard_answers(pre, qs[1])), ("after", shard_answers(model, qs[0]))):
                check_finished_batch(c, list(c.scan_batch_finish()), w, False, ("rank", r, tag))
            with pytest.raises(pie.PieError) as ei:      # the plain finish of a turn the shard form began
                c.token_turn_finish()
            assert ei.value.code == PIE_E_STATE
            got = c.shard_token_turn_finish()
            mine = holder == r
            for col in ("row", "live", "end", "user", "start"):
                assert np.array_equal(got[col][mine], want[col][mine]), (r, col)
            assert np.all(got["row"][~mine] == -1) and not got["live"][~mine].any() and np.all(got["end"][~mine] == END_NONE), (r, "not held")
            assert np.array_equal(c.read_columns()[1], model.end[rows_g]), r
        assert np.all(holder[:-5] >= 0) and np.all(holder[-5:] == -1)
    finally:
        for c in ctxs:
            c.close()


def test_no_leak_over_fifty_pairs(pie, oracle):
    ctx, model, keys = new_ctx(pie, oracle, 9)
    with ctx:
        t0 = oracle.T0_MS
        rows = np.nonzero(model.end > t0)[0][:64]

        def pair(i):
            ops = make_ops(keys[rows], t0, TOUCH, t0 + HOUR + i)
            ctx.token_turn_begin(ops)
            same_turn(ctx.token_turn_finish(), model.turn(ops), i)

        ctx.scan_batch_begin(queries(oracle, 0, 8))
        for i in range(4):                          # every slot has had its staging
            pair(i)
        info = ctx.table_info()
        for i in range(4, 54):
            pair(i)
        now = ctx.table_info()
        assert now["workspace_bytes"] == info["workspace_bytes"] and now["token_bytes"] == info["token_bytes"]
        ctx.scan_batch_finish()
        columns_match(ctx, model)
