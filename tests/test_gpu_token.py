"""GPU: the token column and its index (pie_token_*, sph-pie_amd/csrc/pie_token.h) against the dict model of tests/token_model.py:
batched getSession, touch and delete by token, appends with no host wait, compaction, and the state rules."""
import numpy as np
import pytest

from token_model import END_NONE, TokenModel, check_layout

pytestmark = pytest.mark.gpu

N, U, D = 3000, 50, 8
NOW = 1700000000000
PIE_E_INVAL, PIE_E_STATE = -1, -6


def columns(seed, n=N):
    """Seeded columns with `end` on both sides of NOW (and a few exactly at it: not live)."""
    rng = np.random.default_rng(seed)
    start = NOW - rng.integers(1, 10 ** 9, n)
    end = NOW + rng.integers(-5 * 10 ** 8, 5 * 10 ** 8, n)
    end[rng.integers(0, n, 8)] = NOW
    return start.astype(np.int64), end.astype(np.int64), rng.integers(0, U, n).astype(np.int32), rng.integers(0, D, n).astype(np.int32)


def random_keys(seed, n):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (n, 2), dtype=np.uint64)


def load(ctx, seed):
    cols = columns(seed)
    ctx.load_columns(*cols, U)
    return TokenModel(*cols)


def check_lookup(ctx, model, keys, now=NOW):
    got, want = ctx.token_lookup(keys, now), model.lookup(keys, now)
    assert np.array_equal(got["row"], want["row"])
    assert np.array_equal(got["live"], want["live"])
    f = want["found"]
    for col in ("user", "start", "end"):
        assert np.array_equal(got[col][f], want[col][f]), col
    return got


def check_index(pie, ctx, covered):
    cov, slots, slot_row, keys = ctx.token_layout()
    assert cov == covered and slots == pie.token_slots_for(covered)
    slot_of = check_layout(cov, slots, slot_row, keys, pie.token_homes(keys, slots.bit_length() - 1))
    return slots, slot_of, keys


def test_round_trip(pie, gpu_ctx):
    ctx = gpu_ctx
    model = load(ctx, 1)
    keys = random_keys(2, N)
    ctx.token_set(keys)
    model.token_set(keys)
    order = np.random.default_rng(3).permutation(N)
    at = 0
    for k in (1, 63, 64, 65, 256, 257, 3000):
        ask = keys[order[np.arange(at, at + k) % N]]
        at += k
        got = check_lookup(ctx, model, ask)
        assert np.all(got["row"] >= 0)
    got = check_lookup(ctx, model, keys)
    assert np.array_equal(got["row"], np.arange(N)) and 0 < got["live"].sum() < N
    absent = ctx.token_lookup(random_keys(4, 500), NOW)
    assert np.all(absent["row"] == -1) and not absent["live"].any()
    assert ctx.token_lookup(np.zeros((0, 2), np.uint64), NOW)["row"].shape == (0,)
    slots, _, back = check_index(pie, ctx, N)
    assert slots == pie.token_slots_for(3000) == 8192 and np.array_equal(back, keys)
    info = ctx.table_info()
    assert info["token_rows"] == N and info["token_bytes"] >= N * 16 + slots * 4 and info["token_builds"] >= 1 and info["token_build_ms"] > 0


def test_chains_that_wrap(pie, gpu_ctx):
    ctx = gpu_ctx
    model = load(ctx, 5)
    log2_slots = 13
    assert pie.token_slots_for(N) == 1 << log2_slots
    pool = random_keys(6, 10 ** 6)
    homes = pie.token_homes(pool, log2_slots)
    tail, head = pool[homes >= (1 << log2_slots) - 4], pool[homes == 0]
    assert tail.shape[0] >= 80 and head.shape[0] >= 80
    keys = random_keys(7, N)
    keys[:40], keys[40:80] = tail[:40], head[:40]
    ctx.token_set(keys)
    model.token_set(keys)
    _, slot_of, _ = check_index(pie, ctx, N)
    assert np.any(slot_of[:40] < pie.token_homes(keys[:40], log2_slots)), "forty keys on the last four slots: the chain crosses the end"
    got = check_lookup(ctx, model, keys[:80])
    assert np.array_equal(got["row"], np.arange(80))
    same_homes = np.concatenate([tail[40:80], head[40:80]])          # other keys, the same homes
    assert np.all(ctx.token_lookup(same_homes, NOW)["row"] == -1)
    check_lookup(ctx, model, keys)


def test_half_equal_keys(gpu_ctx):
    ctx = gpu_ctx
    model = load(ctx, 8)
    ones = 2 ** 64 - 1
    keys = random_keys(9, N)
    quads = [(0, 0, ones, ones), (0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x0123456789ABCDEE, 0x7EDCBA9876543210)]
    present, absent = [], []
    for a, b, a2, b2 in quads:                    # (a, b), (a, b'), (a', b) present; (a', b') absent
        present += [(a, b), (a, b2), (a2, b)]
        absent += [(a2, b2)]
    rows = np.array([17 + 311 * i for i in range(len(present))])
    keys[rows] = np.array(present, np.uint64)
    ctx.token_set(keys)
    model.token_set(keys)
    got = check_lookup(ctx, model, np.array(present, np.uint64))
    assert np.array_equal(got["row"], rows)
    assert np.all(ctx.token_lookup(np.array(absent, np.uint64), NOW)["row"] == -1)
    swapped = np.array([(b, a) for a, b in present if a != b and (b, a) not in present], np.uint64)   # the words are not interchangeable
    assert swapped.shape[0] > 0 and np.all(ctx.token_lookup(swapped, NOW)["row"] == -1)


def test_duplicates_latest_row_wins(gpu_ctx):
    ctx = gpu_ctx
    model = load(ctx, 10)
    keys = random_keys(11, N)
    keys[900] = keys[2500] = keys[10]
    ctx.token_set(keys)
    model.token_set(keys)
    assert ctx.token_lookup(keys[10:11], NOW)["row"][0] == 2500
    check_lookup(ctx, model, keys)
    ctx.set_end([2500], [END_NONE])
    model.end[2500] = END_NONE
    got = ctx.token_lookup(keys[10:11], NOW)
    assert got["row"][0] == 2500 and got["live"][0] == 0, "a tombstone stays findable"
    kept = ctx.compact_rows()
    new_of_old, _ = ctx.compact_maps()
    assert np.array_equal(model.compact(), new_of_old) and kept == model.start.shape[0]
    assert ctx.token_lookup(keys[10:11], NOW)["row"][0] == new_of_old[900] == 900
    check_lookup(ctx, model, keys)


def test_prefix_and_appends_without_a_host_wait(pie, gpu_ctx):
    ctx = gpu_ctx
    model = load(ctx, 12)
    n_all = N + 200
    keys = random_keys(13, n_all)
    ctx.token_set(keys[:400])
    model.token_set(keys[:400])
    assert ctx.token_layout()[1] == 1024
    got = check_lookup(ctx, model, keys[:N])
    assert np.all(got["row"][:400] >= 0) and np.all(got["row"][400:] == -1)
    # appended rows, keys for 113 more rows and a lookup, back to back
    new = columns(14, 200)
    ctx.append_rows(*new, U)
    ctx.token_append(keys[400:513])
    got = ctx.token_lookup(keys, NOW)
    model.append_rows(*new)
    model.token_append(keys[400:513])
    want = model.lookup(keys, NOW)
    assert np.array_equal(got["row"], want["row"]) and np.array_equal(got["row"][:513], np.arange(513)) and np.all(got["row"][513:] == -1)
    cov, slots, _, _ = ctx.token_layout()
    assert cov == 513 and slots == 2048, "the growth rebuild"
    builds = ctx.table_info()["token_builds"]
    # keys up to 87 rows short of the table's end: the appended rows answer with their own columns, again with no wait
    ctx.token_append(keys[513 : n_all - 87])
    got = ctx.token_lookup(keys, NOW)
    model.token_append(keys[513 : n_all - 87])
    want = model.lookup(keys, NOW)
    assert np.array_equal(got["row"][: n_all - 87], np.arange(n_all - 87)) and np.all(got["row"][n_all - 87 :] == -1)
    for col in ("live", "user", "start", "end"):
        assert np.array_equal(got[col][: n_all - 87], want[col][: n_all - 87]), col
    assert np.array_equal(got["start"][N : n_all - 87], new[0][:113]) and np.array_equal(got["user"][N : n_all - 87], new[2][:113])
    check_index(pie, ctx, n_all - 87)
    assert ctx.table_info()["token_builds"] == builds + 1
    # an in-place append (the capacity doubled above), its keys and a lookup: the queued path of both
    more = columns(15, 10)
    more_keys = random_keys(16, 10)
    ctx.append_rows(*more, U)
    ctx.token_append(np.concatenate([keys[n_all - 87 :], more_keys]))
    got = ctx.token_lookup(more_keys, NOW)
    assert np.array_equal(got["row"], np.arange(n_all, n_all + 10)) and np.array_equal(got["end"], more[1])
    assert np.array_equal(got["live"], (more[1] > NOW).astype(np.uint8))
    # beyond the table
    with pytest.raises(pie.PieError) as ei:
        ctx.token_append(random_keys(17, 1))
    assert ei.value.code == PIE_E_INVAL
    assert ctx.token_layout()[0] == n_all + 10 and ctx.table_info()["token_rows"] == n_all + 10


def test_touch_and_delete_by_token(pie, oracle, gpu_ctx):
    ctx = gpu_ctx
    model = load(ctx, 18)
    keys = random_keys(19, N)
    ctx.token_set(keys)
    model.token_set(keys)
    live = np.nonzero(model.end > NOW)[0]
    dead = np.nonzero(model.end <= NOW)[0]
    tomb = live[:30]
    ctx.set_end(tomb, np.full(30, END_NONE))
    model.end[tomb] = END_NONE
    twice = live[40]
    rows = np.concatenate([live[30:200], dead[:100], tomb[:10], [twice]])
    ask = np.concatenate([keys[rows], random_keys(20, 25)])
    order = np.random.default_rng(21).permutation(ask.shape[0])
    ask = ask[order]
    new_end = NOW + np.random.default_rng(22).integers(1, 10 ** 8, ask.shape[0])
    new_end[::7] = END_NONE                                      # deletes among the touches
    before = model.end.copy()
    rows_out = ctx.token_set_end(ask, new_end, NOW)
    want_rows = model.token_set_end(ask, new_end, NOW)
    assert np.array_equal(rows_out, want_rows)
    assert np.count_nonzero(rows_out == twice) == 2
    assert set(rows_out[rows_out >= 0]) == set(live[30:200]), "live sessions only: no expired, tombstoned or unknown key"
    last = np.nonzero(rows_out == twice)[0][-1]
    assert model.end[twice] == new_end[last]
    got_end = ctx.read_columns()[1]
    assert np.array_equal(got_end, model.end)
    changed = np.nonzero(got_end != before)[0]
    assert set(changed) <= set(live[30:200])
    mask = (1 << D) - 1
    ctx.set_disciplines(mask, D)
    for a, b in zip(ctx.scan(NOW, 0), oracle.scan(model.start, model.end, model.user, model.disc, U, NOW, 0, mask)):
        assert np.array_equal(a, b), "the derived keys fell out of step"
    # deleteSession of an expired session: now = PIE_END_NONE takes every found row that is not a tombstone
    victim = dead[0]
    assert model.end[victim] != END_NONE
    both = np.stack([keys[victim], keys[tomb[0]]])
    rows_out = ctx.token_set_end(both, [END_NONE, NOW + 5], END_NONE)
    assert np.array_equal(rows_out, model.token_set_end(both, [END_NONE, NOW + 5], END_NONE)) and list(rows_out) == [victim, -1]
    got = check_lookup(ctx, model, both)
    assert list(got["row"]) == [victim, tomb[0]] and not got["live"].any() and got["end"][0] == END_NONE
    assert np.array_equal(ctx.read_columns()[1], model.end)
    assert ctx.token_set_end(np.zeros((0, 2), np.uint64), [], NOW).shape == (0,)


@pytest.mark.parametrize("shrink", [False, True])
def test_compaction(pie, gpu_ctx, shrink):
    ctx = gpu_ctx
    model = load(ctx, 23)
    keys = random_keys(24, N)
    ctx.token_set(keys[: N - 100])                 # the last 100 rows never had a key
    model.token_set(keys[: N - 100])
    builds = ctx.table_info()["token_builds"]
    assert ctx.compact_rows(shrink=False) == N and ctx.table_info()["token_builds"] == builds, "nothing dropped: the index stays"
    check_lookup(ctx, model, keys)
    dropped = np.arange(0, N, 3)
    ctx.set_end(dropped, np.full(dropped.shape[0], END_NONE))
    model.end[dropped] = END_NONE
    kept = ctx.compact_rows(END_NONE, shrink=shrink)
    new_of_old, old_of_new = ctx.compact_maps()
    assert np.array_equal(model.compact(), new_of_old) and kept == N - dropped.shape[0]
    covered = int(np.count_nonzero(old_of_new < N - 100))
    assert model.covered == covered
    got = check_lookup(ctx, model, keys)
    want_row = np.where(np.arange(N) < N - 100, new_of_old, -1)
    assert np.array_equal(got["row"], want_row), "kept keys at their new rows; dropped and never-covered keys absent"
    check_index(pie, ctx, covered)
    info = ctx.table_info()
    assert info["token_rows"] == covered and info["token_builds"] == builds + 1
    # the table goes on: the rows behind the prefix can still be given keys
    ctx.token_append(keys[N - 100 :][new_of_old[N - 100 :] >= 0])
    model.token_append(keys[N - 100 :][new_of_old[N - 100 :] >= 0])
    got = check_lookup(ctx, model, keys)
    assert np.array_equal(got["row"], new_of_old)


def test_state_rules(pie, oracle, gpu_ctx):
    ctx = gpu_ctx
    keys = random_keys(25, N)

    def refused(fn, *a):
        with pytest.raises(pie.PieError) as ei:
            fn(*a)
        return ei.value.code == PIE_E_STATE

    def no_column():
        assert refused(ctx.token_lookup, keys[:4], NOW) and refused(ctx.token_append, keys[:4])
        assert refused(ctx.token_set_end, keys[:4], np.zeros(4, np.int64), NOW) and refused(ctx.token_layout)
        assert ctx.table_info()["token_rows"] == 0

    model = load(ctx, 26)
    no_column()                                       # before token_set
    ctx.token_set(keys)
    assert ctx.table_info()["token_rows"] == N
    load(ctx, 26)
    no_column()                                       # a load drops the column
    ctx.token_set(keys)
    ctx.gen_synthetic(0x5EED, 2000, 0, 2000, U, D, 0)
    no_column()                                       # and so does a generated table
    model = load(ctx, 26)
    ctx.token_set(keys)
    model.token_set(keys)
    # between begin and finish of a scan
    mask = (1 << D) - 1
    ctx.set_disciplines(mask, D)
    ctx.scan_begin(NOW, 0)
    assert refused(ctx.token_lookup, keys[:4], NOW) and refused(ctx.token_set_end, keys[:4], np.zeros(4, np.int64), NOW)
    assert refused(ctx.token_set, keys) and refused(ctx.token_layout)
    m = ctx.scan_finish()
    want = oracle.scan(model.start, model.end, model.user, model.disc, U, NOW, 0, mask)
    assert m == want[2].shape[0]
    for a, b in zip(ctx.read_results(), want):
        assert np.array_equal(a, b)
    check_lookup(ctx, model, keys[:100])
    # the struct as callers built before this change know it
    import ctypes as C
    from sph_pie_amd.binding import PieTableInfo
    old = PieTableInfo()
    old.struct_size = PieTableInfo.token_rows.offset
    old.token_rows = 12345
    assert ctx._lib.pie_table_info_get(ctx._ctx, C.byref(old)) == 0
    assert old.rows == N and old.token_rows == 12345, "the library wrote past the size the caller gave"
    # NULL keys
    assert ctx._lib.pie_token_lookup(ctx._ctx, None, 3, NOW, None, None, None, None, None) == PIE_E_INVAL
    assert ctx._lib.pie_token_lookup(ctx._ctx, None, 0, NOW, None, None, None, None, None) == 0
    # a sharded context of its own
    with pie.PieScan(0) as sh:
        sh.load_columns(model.start, model.end, model.user, model.disc, U)
        sh.token_set(keys)
        n_local, _ = sh.shard_table(0, 2)[:2]
        assert sh.table_info()["token_rows"] == 0
        with pytest.raises(pie.PieError) as ei:
            sh.token_set(keys[:n_local])
        assert ei.value.code == PIE_E_STATE
    with pie.PieScan(0) as fresh:                    # no table at all
        with pytest.raises(pie.PieError) as ei:
            fresh.token_set(keys[:1])
        assert ei.value.code == PIE_E_STATE
