"""GPU: pie_compact_rows against tests/compact_model.py (numpy) and the oracles, bit for bit.

The invariant behind every check: compaction keeps the rows with end > dead_before in table order, so the table afterwards
IS the model's filtered table (read_columns), the maps are the model's, every reader answers what the oracle answers on the
new table, and — for queries whose `now` is at or above dead_before, which select no dropped row — every answer is the one
given before with its rows pushed through new_of_old."""
import numpy as np
import pytest

import compact_model as CM
import table_model as T
from table_model import ALL, DAY, HOUR, INT64_MAX, INT64_MIN

pytestmark = pytest.mark.gpu

PIE_E_STATE = -6


# ------------------------------------------------------------------------------------------------ helpers
def same(got, want, tag):
    for name, a, b in zip(("counts", "offsets", "idx"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), (tag, name)


def columns_match(ctx, m, tag):
    assert ctx.n == m.n and int(ctx.stats()["rows"]) == m.n and int(ctx.stats()["users"]) == m.U, (tag, "shape")
    for name, got, want in zip(("start", "end", "user", "disc"), ctx.read_columns(), m.columns()):
        assert got.dtype == want.dtype and np.array_equal(got, want), (tag, "column " + name)


def load(ctx, m, mask=ALL):
    ctx.load_columns(*m.columns(), m.U)
    ctx.set_disciplines(mask, m.D)


def make_model(oracle, seed, n, U, D, flags=0):
    m = CM.CompactModel(oracle)
    m.load(*[a.copy() for a in oracle.gen(seed, n, 0, n, U, D, flags)], U, D)
    return m


def kill_rows(ctx, m, rng, frac, prune=True):
    """Tombstone roughly `frac` of the rows through the public mutators, the same on the context and the model: whole
    users, the oldest starts, and rows picked at random (a fifth of those merely expire, at various ends)."""
    t0 = m.oracle.T0_MS
    for u in rng.choice(m.U, min(24, max(1, int(m.U * frac * 0.4))), replace=False).tolist():
        assert np.array_equal(ctx.delete_user(int(u)), m.delete_user(int(u)))
    if prune:
        cutoff = int(np.quantile(m.start, frac * 0.3))
        assert np.array_equal(ctx.prune_before(cutoff), m.prune_before(cutoff))
    rows = rng.choice(m.n, max(1, int(m.n * frac)), replace=False).astype(np.int32)
    ne = np.full(rows.size, INT64_MIN, np.int64)
    ne[::5] = t0 - rng.integers(1, 30 * DAY, ne[::5].size)
    ctx.set_end(rows, ne)
    m.set_end(rows, ne)


def queries_at_or_above(m, rng, k, floor):
    """k queries with now >= floor: sparse ones at the top of the range, one on the floor itself, one above everything."""
    t0 = m.oracle.T0_MS
    e = m.end[(m.end > floor) & (m.end < t0 + 365 * DAY)]
    top = int(e.max()) if e.size else floor
    lo = max(floor, int(np.quantile(e, 0.97))) if e.size else floor
    qs = []
    for i in range(k):
        now = int(rng.integers(lo, top + 1)) if top > lo else lo
        if i == 1 and k <= 16 and floor > INT64_MIN:      # on the floor itself: every kept row that is live there
            now = floor
        if i == 2:
            now = top
        cutoff = int(rng.choice([INT64_MIN, t0 - 61 * DAY]))
        mask = ALL if i % 3 == 0 else int(rng.integers(1, 2 ** 63))
        qs.append((now, cutoff, mask))
    return qs


def read_everything(ctx, m, qs16, qs64, qsw, single):
    """-> dict of every reader's answer: the single scan, a 16- and a 64-query batch (M, union, lists), one wide batch."""
    out = {"single": ctx.scan(single[0], single[1])}
    for name, qs in (("b16", qs16), ("b64", qs64)):
        ctx.scan_batch_begin(qs)
        out[name + "_m"] = list(ctx.scan_batch_finish())
        out[name + "_union"] = ctx.batch_read_union()
        out[name] = [ctx.batch_read_results(q) for q in range(len(qs))]
    ctx.scan_wide_begin(qsw)
    out["wide_m"] = ctx.scan_wide_finish()
    out["wide"] = {q: ctx.batch_read_results(q) for q in (0, 1, 2, len(qsw) // 2, len(qsw) - 1)}
    return out


UNIONS_CHECKED = []   # (tag, batch) of every union compared with the model: the large tables must get there


def check_against_model(tag, got, m, qs16, qs64, qsw, single, mask):
    same(got["single"], m.scan(single[0], single[1], mask), (tag, "single"))
    for name, qs in (("b16", qs16), ("b64", qs64)):
        wants = m.scan_many(qs)
        assert got[name + "_m"] == [int(w[2].size) for w in wants], (tag, name, "M")
        for q, w in enumerate(wants):
            same(got[name][q], w, (tag, name, q))
        un = got[name + "_union"]
        if un is not None:
            uoff, rows, masks = un
            for q, w in enumerate(wants):
                sel = ((masks >> np.uint64(q)) & np.uint64(1)) == 1
                csum = np.concatenate([[0], np.cumsum(sel)])
                assert np.array_equal(rows[sel], w[2]) and np.array_equal(csum[uoff], w[1]), (tag, name, "union", q)
            UNIONS_CHECKED.append((tag, name, m.n))
    wants = m.scan_many([qsw[q] for q in sorted(got["wide"])])
    for q, w in zip(sorted(got["wide"]), wants):
        same(got["wide"][q], w, (tag, "wide", q))


def check_pushed(tag, before, after, new_of_old):
    same(after["single"], CM.push_result(before["single"], new_of_old), (tag, "single pushed"))
    for name in ("b16", "b64"):
        assert after[name + "_m"] == before[name + "_m"], (tag, name, "a kept selected row was lost")
        for q, (a, b) in enumerate(zip(after[name], before[name])):
            same(a, CM.push_result(b, new_of_old), (tag, name, "pushed", q))
    assert after["wide_m"] == before["wide_m"], (tag, "wide", "a kept selected row was lost")
    for q in before["wide"]:
        same(after["wide"][q], CM.push_result(before["wide"][q], new_of_old), (tag, "wide pushed", q))


def compact_both(ctx, m, dead_before=INT64_MIN, shrink=False, tag=""):
    n_old = m.n
    want_new, want_old = m.compact_rows(dead_before)
    kept = ctx.compact_rows(dead_before, shrink=shrink)
    assert kept == m.n == ctx.n, (tag, "kept", kept, m.n)
    got_new, got_old = ctx.compact_maps()
    assert got_new.dtype == np.int32 and got_old.dtype == np.int32
    assert got_new.size == n_old and np.array_equal(got_new, want_new), (tag, "new_of_old")
    assert np.array_equal(got_old, want_old), (tag, "old_of_new")
    columns_match(ctx, m, (tag, "after compaction"))
    return want_new, want_old


# ------------------------------------------------------------------------------------------------ 1. the renumbering invariant
@pytest.mark.parametrize("seed,n,U,frac,flags", [(1, 3_000_000, 40009, 0.5, 4), (2, 700_001, 997, 0.9, 0), (3, 300_007, 5003, 0.2, 5),
                                                  (4, 65_537, 3, 0.6, 2)])
def test_renumbering_invariant(gpu_ctx, oracle, seed, n, U, frac, flags):
    rng = np.random.default_rng([seed, 0xC0AC])
    ctx, D = gpu_ctx, 32
    m = make_model(oracle, seed, n, U, D, flags)
    mask = ALL if seed % 2 else 0x5555555555555555
    load(ctx, m, mask)
    kill_rows(ctx, m, rng, frac)
    dead_frac = 1.0 - np.count_nonzero(m.end != INT64_MIN) / m.n
    print("seed %d: %d rows, %.0f %% tombstoned" % (seed, n, 100 * dead_frac))
    # half the tables also drop what expired a while ago
    dead_before = INT64_MIN if seed % 2 else oracle.T0_MS - 10 * DAY
    qs16, qs64 = queries_at_or_above(m, rng, 16, dead_before), queries_at_or_above(m, rng, 64, dead_before)
    qsw = queries_at_or_above(m, rng, 130, dead_before)
    single = (qs16[0][0], qs16[0][1])
    before = read_everything(ctx, m, qs16, qs64, qsw, single)
    check_against_model("before", before, m, qs16, qs64, qsw, single, mask)
    new_of_old, _ = compact_both(ctx, m, dead_before, tag=("seed", seed))
    assert m.n < n
    ctx.set_disciplines(mask, D)
    after = read_everything(ctx, m, qs16, qs64, qsw, single)
    check_against_model("after", after, m, qs16, qs64, qsw, single, mask)
    check_pushed(("seed", seed), before, after, new_of_old)
    if seed == 1:
        # without a dense query (dead_before is the tombstone here, so no query sits on the floor) the batches of this table keep
        # their union: the union / mask comparison above really ran, before and after the compaction
        seen = {(t, b) for t, b, _ in UNIONS_CHECKED if _ in (n, m.n)}
        assert {("before", "b16"), ("before", "b64"), ("after", "b16"), ("after", "b64")} <= seen, seen


# ------------------------------------------------------------------------------------------------ 2. edges
def test_nothing_dropped_is_the_identity(gpu_ctx, oracle):
    ctx = gpu_ctx
    m = make_model(oracle, 11, 100_003, 211, 16)
    load(ctx, m)
    q = (oracle.T0_MS - 6 * HOUR, INT64_MIN)
    before = ctx.scan(*q)
    compactions = ctx.table_info()["compactions"]
    new_of_old, old_of_new = compact_both(ctx, m, INT64_MIN, tag="identity")
    assert np.array_equal(new_of_old, np.arange(m.n)) and np.array_equal(old_of_new, np.arange(m.n))
    info = ctx.table_info()
    assert info["compactions"] == compactions + 1 and info["compact_bytes"] == 8 * m.n
    same(ctx.scan(*q), before, "identity")
    same(ctx.scan(*q), m.scan(q[0], q[1], ALL), "identity vs model")


def test_everything_dropped_leaves_an_empty_table(gpu_ctx, oracle):
    ctx = gpu_ctx
    m = make_model(oracle, 12, 20_011, 97, 8)
    load(ctx, m)
    new_of_old, old_of_new = compact_both(ctx, m, INT64_MAX, tag="all dropped")
    assert m.n == 0 and old_of_new.size == 0 and np.all(new_of_old == -1)
    info = ctx.table_info()
    assert info["rows"] == 0 and info["table_bytes"] >= 24
    same(ctx.scan(INT64_MIN, INT64_MIN), m.scan(INT64_MIN, INT64_MIN, ALL), "empty scan")
    for res, want in zip(ctx.scan_batch([(INT64_MIN, INT64_MIN, ALL)] * 3), m.scan_many([(INT64_MIN, INT64_MIN, ALL)] * 3)):
        same(res, want, "empty batch")
    assert ctx.expired_queue(INT64_MIN, INT64_MAX).size == 0
    t0 = oracle.T0_MS
    s2 = np.array([t0, t0 + 1, t0 + 1], np.int64)
    e2 = np.array([t0 + DAY, INT64_MIN, t0 + 2 * DAY], np.int64)
    u2, d2 = np.array([5, 5, 96], np.int32), np.array([0, 1, 7], np.int32)
    ctx.append_rows(s2, e2, u2, d2, m.U)
    m.append_rows(s2, e2, u2, d2, m.U)
    columns_match(ctx, m, "append to the empty table")
    same(ctx.scan(t0, INT64_MIN), m.scan(t0, INT64_MIN, ALL), "scan after the append")
    compact_both(ctx, m, INT64_MIN, shrink=True, tag="empty, then three rows, shrunk")
    same(ctx.scan(t0, INT64_MIN), m.scan(t0, INT64_MIN, ALL), "scan after the second compaction")


def test_a_single_row(gpu_ctx, oracle):
    ctx, t0 = gpu_ctx, oracle.T0_MS
    for end, dead_before, kept in ((t0, INT64_MIN, 1), (INT64_MIN, INT64_MIN, 0), (t0, t0, 0), (t0, t0 - 1, 1)):
        m = CM.CompactModel(oracle)
        m.load([t0 - DAY], [end], [0], [0], 1, 1)
        load(ctx, m)
        compact_both(ctx, m, dead_before, tag=("single row", end, dead_before))
        assert m.n == kept
        same(ctx.scan(INT64_MIN, INT64_MIN), m.scan(INT64_MIN, INT64_MIN, ALL), "single row scan")


def test_dead_before_edges(gpu_ctx, oracle):
    ctx, t0 = gpu_ctx, oracle.T0_MS
    rng = np.random.default_rng(77)
    base = make_model(oracle, 13, 50_021, 307, 32)
    base.end[rng.choice(base.n, 9000, replace=False)] = INT64_MIN           # tombstones together with every dead_before
    base.end[rng.choice(base.n, 50, replace=False)] = INT64_MAX
    base.end[rng.choice(base.n, 50, replace=False)] = INT64_MAX - 1
    value = int(base.end[base.end != INT64_MIN][1234])
    for dead_before in (INT64_MIN, INT64_MAX - 1, value, value - 1, INT64_MIN + 1, t0):
        m = CM.CompactModel(oracle)
        m.load(*base.columns(), base.U, base.D)
        load(ctx, m)
        compact_both(ctx, m, dead_before, tag=("dead_before", dead_before))
        assert np.all(m.end > dead_before)
        q = (max(dead_before, t0 - 3 * HOUR), INT64_MIN)
        same(ctx.scan(*q), m.scan(q[0], q[1], ALL), ("dead_before", dead_before, "scan"))
    assert np.count_nonzero(base.end > INT64_MAX - 1) == 50


def test_sizes_around_every_kernel_boundary(gpu_ctx, oracle):
    """Row counts of 1 below, on and 1 above a wave step, a block step, a wave's whole unit and a block's four units, for the
    geometry the library reports; live and dead rows alternate in runs of coprime lengths so that every store shape
    (ragged head, aligned middle, ragged tail) occurs at every boundary."""
    ctx, t0 = gpu_ctx, oracle.T0_MS
    big = 3_000_000        # large enough that a unit holds several steps
    geo = ctx.compact_geometry(big)
    wave, block, unit = geo["rows_per_wave_step"], geo["rows_per_block_step"], geo["rows_per_unit"]
    assert wave >= 64 and block == 4 * wave and unit % wave == 0 and unit > wave
    sizes = {1, 2, 3}
    for edge in (wave, block, 2 * block, unit, 4 * unit, 5 * unit):
        sizes |= {edge - 1, edge, edge + 1}
    # sizes at which the library's own plan puts the boundary at the table's end
    for n in (big - 1, big, big + 1):
        g = ctx.compact_geometry(n)
        sizes |= {n} | {g["rows_per_unit"] * 4 * (g["blocks"] - 1) + d for d in (-1, 0, 1)}
    for n in sorted(s for s in sizes if s > 0):
        i = np.arange(n, dtype=np.int64)
        m = CM.CompactModel(oracle)
        end = np.where((i % 7 < 3) | (i % 11 == 0), t0 + i % 1000 + 1, INT64_MIN).astype(np.int64)
        m.load(t0 - DAY + i % 5, end, (i * 13 % 29).astype(np.int32), (i % 4).astype(np.int32), 29, 4)
        load(ctx, m)
        compact_both(ctx, m, INT64_MIN if n % 2 else t0 + 500, tag=("size", n))
        if n < 1_000_000:
            same(ctx.scan(t0, INT64_MIN), m.scan(t0, INT64_MIN, ALL), ("size", n, "scan"))


# ------------------------------------------------------------------------------------------------ 3. every derived structure alive
@pytest.mark.parametrize("form", [0xC85, 0x485, 0x01])
def test_pinned_key_forms_survive(pie, oracle, form):
    t0 = oracle.T0_MS
    rng = np.random.default_rng(form)
    with pie.PieScan(0) as ctx:
        m = make_model(oracle, 21, 400_009, 1009, 32, 4)
        load(ctx, m)
        ctx.set_scan_form(form)
        q = (t0 - 2 * HOUR, INT64_MIN)
        same(ctx.scan(*q), m.scan(q[0], q[1], ALL), ("form", form, "before"))
        has_keys = ctx.table_info()["has_keys"]
        kill_rows(ctx, m, rng, 0.5)
        compact_both(ctx, m, t0 - 20 * DAY, tag=("form", form))
        assert ctx.table_info()["has_keys"] == has_keys == 1
        for _ in range(3):
            same(ctx.scan(*q), m.scan(q[0], q[1], ALL), ("form", form, "after"))
        v = ctx.stats()["k1_variant"]
        print("form 0x%x pinned: the scans after the compaction ran as 0x%x" % (form, v))
        assert v & 0xC00 == form & 0xC00, "the pinned form's key (0x400 2-byte, 0x800 1-byte, neither: every byte) was not the one read"


def test_hot_index_and_ordered_run_are_rebuilt(pie, oracle):
    t0 = oracle.T0_MS
    rng = np.random.default_rng(5)
    ctx = T.ctx_with_env(pie, 1, 1)
    try:
        m = make_model(oracle, 22, 3_000_017, 20011, 32, 0)
        load(ctx, m)
        qs = [(t0 - 6 * HOUR - 977 * q, t0 - 61 * DAY, ALL if q % 2 else 0x5555555555555555) for q in range(16)]
        for res, want in zip(ctx.scan_batch(qs), m.scan_many(qs)):
            same(res, want, "hot before")
        for res, want in zip(ctx.scan_batch(qs), m.scan_many(qs)):
            same(res, want, "hot before, again")
        info = ctx.table_info()
        assert info["hot_rows"] > 0 and info["hot_builds"] >= 1, "the table is large enough for the hot index"
        kill_rows(ctx, m, rng, 0.4, prune=False)    # spread evenly over the range of `end`: the fine key's range stays where it was
        builds = ctx.table_info()["hot_builds"]
        new_of_old, _ = compact_both(ctx, m, INT64_MIN, tag="hot")
        info = ctx.table_info()
        assert info["hot_rows"] == 0 and info["has_keys"] == 1, "dropped with the rows it named, as after a load"
        for _ in range(2):
            for res, want in zip(ctx.scan_batch(qs), m.scan_many(qs)):
                same(res, want, "hot after")
        info = ctx.table_info()
        assert info["hot_builds"] > builds and info["hot_rows"] > 0, "the next batch rebuilt the index"
        # ordered run, mode 2: built by the next scan, again after the compaction
        ctx.set_ordered_run(2)
        q = (t0 - 2 * HOUR, INT64_MIN)
        same(ctx.scan(*q), m.scan(q[0], q[1], ALL), "ordered before")
        info = ctx.table_info()
        assert info["ordered_rows"] > 0 and ctx.stats()["k1_variant"] & 0x2000
        ord_builds = info["ordered_builds"]
        rows = rng.choice(m.n, m.n // 3, replace=False).astype(np.int32)
        ctx.set_end(rows, np.full(rows.size, INT64_MIN, np.int64))
        m.set_end(rows, np.full(rows.size, INT64_MIN, np.int64))
        compact_both(ctx, m, INT64_MIN, tag="ordered")
        assert ctx.table_info()["ordered_rows"] == 0, "the run is invalid after a compaction"
        same(ctx.scan(*q), m.scan(q[0], q[1], ALL), "ordered after")
        info = ctx.table_info()
        assert info["ordered_builds"] > ord_builds and info["ordered_rows"] > 0 and ctx.stats()["k1_variant"] & 0x2000
        for res, want in zip(ctx.scan_batch(qs), m.scan_many(qs)):
            same(res, want, "ordered batch after")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 4. mutations after compaction
def test_mutations_after_compaction_and_composition(gpu_ctx, oracle):
    ctx, t0 = gpu_ctx, oracle.T0_MS
    rng = np.random.default_rng(31)
    m = make_model(oracle, 31, 200_003, 499, 32, 4)
    ends0 = m.end.copy()
    load(ctx, m)
    kill_rows(ctx, m, rng, 0.5)
    ends1 = m.end.copy()
    n1, o1 = compact_both(ctx, m, INT64_MIN, tag="first")
    q = (t0 - HOUR, INT64_MIN)

    def check(tag):
        columns_match(ctx, m, tag)
        same(ctx.scan(*q), m.scan(q[0], q[1], ALL), (tag, "scan"))
        for res, want in zip(ctx.scan_batch([(q[0] + k, q[1], ALL) for k in range(5)]), m.scan_many([(q[0] + k, q[1], ALL) for k in range(5)])):
            same(res, want, (tag, "batch"))

    # append in place (capacity is the old one), touch, revive a dead user's slot, delete a user
    k = 1000
    s2 = (int(m.start.max()) + np.sort(rng.integers(0, 4000, k))).astype(np.int64)
    e2 = (t0 + rng.integers(-HOUR, 6 * HOUR, k)).astype(np.int64)
    u2, d2 = rng.integers(0, m.U, k).astype(np.int32), rng.integers(0, m.D, k).astype(np.int32)
    cap_before = ctx.table_info()["table_bytes"]
    ctx.append_rows(s2, e2, u2, d2, m.U)
    m.append_rows(s2, e2, u2, d2, m.U)
    assert ctx.table_info()["table_bytes"] == cap_before, "the append fits the capacity the compaction left"
    check("append in place")
    rows = rng.choice(m.n, 5000, replace=False).astype(np.int32)
    ne = (t0 + rng.integers(-3 * DAY, DAY, rows.size)).astype(np.int64)
    ne[::7] = INT64_MIN
    ctx.set_end(rows, ne)
    m.set_end(rows, ne)
    check("touch")
    dead = np.nonzero(m.end == INT64_MIN)[0][:50].astype(np.int32)
    ctx.set_end(dead, np.full(dead.size, t0 + 2 * HOUR, np.int64))
    m.set_end(dead, np.full(dead.size, t0 + 2 * HOUR, np.int64))
    check("revive")
    u = int(np.bincount(m.user, minlength=m.U).argmax())
    assert np.array_equal(ctx.delete_user(u), m.delete_user(u))
    check("delete_user")
    assert np.array_equal(ctx.expired_queue(t0 - DAY, t0), m.expired_queue(t0 - DAY, t0))
    assert ctx.queue_info()[0] == 1
    assert np.array_equal(ctx.archive_queue(t0, 30 * DAY), m.archive_queue(t0, 30 * DAY))
    now = int(T.add_months(np.array([int(m.start.min())], np.int64), 2)[0]) + 2 * DAY
    assert np.array_equal(ctx.retention_purge(now, 2, 0), m.retention_purge(now, 2, 0))
    check("retention_purge")
    # a shrinking compaction, then an append that has to grow the table
    ends2 = m.end.copy()
    n2, o2 = compact_both(ctx, m, t0 - 2 * DAY, shrink=True, tag="second")
    check("second compaction")
    k = m.n + 10
    s3 = (int(m.start.max()) + np.sort(rng.integers(0, 4000, k))).astype(np.int64)
    e3 = (t0 + rng.integers(-HOUR, 6 * HOUR, k)).astype(np.int64)
    u3, d3 = rng.integers(0, m.U, k).astype(np.int32), rng.integers(0, m.D, k).astype(np.int32)
    ctx.append_rows(s3, e3, u3, d3, m.U)
    m.append_rows(s3, e3, u3, d3, m.U)
    check("append that grows")
    assert np.array_equal(ctx.compact_maps()[0], n2), "the maps outlive appends: they renumber nothing"
    # composition: old_of_new of the second compaction, restricted to rows the first table already held, chained through
    # the first one's, names the rows of the ORIGINAL table that survived both — computed here from the history of `end`
    held = o2[o2 < o1.size]
    survived_first = np.nonzero(ends1 > INT64_MIN)[0]
    survived_both = survived_first[ends2[:o1.size] > t0 - 2 * DAY]
    assert np.array_equal(o1[held], survived_both) and ends0.size == n1.size
    assert np.array_equal(CM.translate(n2, n1[survived_both]), np.arange(held.size)), "new_of_old chains the same way"


# ------------------------------------------------------------------------------------------------ 5. state rules
def test_state_rules(pie, oracle):
    t0 = oracle.T0_MS
    with pie.PieScan(0) as fresh:
        with pytest.raises(pie.PieError) as ei:
            fresh.compact_rows()
        assert ei.value.code == PIE_E_STATE, "no table"
        with pytest.raises(pie.PieError) as ei:
            fresh.compact_maps()
        assert ei.value.code == PIE_E_STATE, "no maps"
    ctx = T.ctx_with_env(pie, 1, 1)     # asynchronous mutations on
    try:
        m = make_model(oracle, 41, 150_001, 301, 16, 4)
        load(ctx, m)
        ctx.scan_begin(t0, INT64_MIN)
        with pytest.raises(pie.PieError) as ei:
            ctx.compact_rows()
        assert ei.value.code == PIE_E_STATE and ctx.n == m.n, "a scan begun and unfinished"
        ctx.scan_finish()
        ctx.scan_batch_begin([(t0, INT64_MIN, ALL)] * 4)
        with pytest.raises(pie.PieError) as ei:
            ctx.compact_rows()
        assert ei.value.code == PIE_E_STATE and ctx.n == m.n, "a batch in flight"
        ctx.scan_batch_finish()
        # a queue on the device, then queued asynchronous appends and touches: the compaction sees them all
        assert ctx.expired_queue(t0 - DAY, t0, fetch=False) == m.expired_queue(t0 - DAY, t0).size
        assert ctx.queue_info()[0] == 1
        rows = np.arange(0, m.n, 3, dtype=np.int32)
        ctx.set_end(rows, np.full(rows.size, INT64_MIN, np.int64))
        m.set_end(rows, np.full(rows.size, INT64_MIN, np.int64))
        for burst in range(3):      # in place: the table has room only after a first growing append
            k = 200 if burst else m.n // 2
            s2 = (int(m.start.max()) + np.arange(k)).astype(np.int64)
            e2 = np.where(np.arange(k) % 4 == 0, INT64_MIN, t0 + HOUR + np.arange(k)).astype(np.int64)
            u2, d2 = (np.arange(k) % m.U).astype(np.int32), (np.arange(k) % m.D).astype(np.int32)
            ctx.append_rows(s2, e2, u2, d2, m.U)
            m.append_rows(s2, e2, u2, d2, m.U)
        compact_both(ctx, m, INT64_MIN, tag="queued appends")
        with pytest.raises(pie.PieError) as ei:
            ctx.queue_info()
        assert ei.value.code == PIE_E_STATE, "the queue is forgotten"
        kind = pie.binding.C.c_int32(7)
        ctx._lib.pie_queue_info(ctx._ctx, pie.binding.C.byref(kind), None, None)
        assert kind.value == 0
        with pytest.raises(pie.PieError) as ei:
            ctx.read_results()
        assert ei.value.code == PIE_E_STATE, "the last scan's results are forgotten"
        same(ctx.scan(t0, INT64_MIN), m.scan(t0, INT64_MIN, ALL), "scan after")
        # a load renumbers the rows: the maps go
        load(ctx, m)
        with pytest.raises(pie.PieError) as ei:
            ctx.compact_maps()
        assert ei.value.code == PIE_E_STATE and ctx.table_info()["compact_bytes"] == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 6. PIE_COMPACT_SHRINK
def test_shrink_resizes_table_and_workspace(pie, oracle):
    t0 = oracle.T0_MS
    rng = np.random.default_rng(6)
    with pie.PieScan(0) as ctx, pie.PieScan(0) as ref:
        m = make_model(oracle, 51, 500_009, 2003, 32, 4)
        load(ctx, m)
        kill_rows(ctx, m, rng, 0.7)
        ctx.scan(t0, INT64_MIN)
        before = ctx.table_info()
        compact_both(ctx, m, INT64_MIN, tag="no shrink")
        kept = ctx.table_info()
        assert kept["table_bytes"] == before["table_bytes"] and kept["workspace_bytes"] == before["workspace_bytes"]
        assert kept["rows"] == m.n < 500_009
        # the same history with the flag: sizes of a fresh load of the kept rows
        ctx.load_columns(*m.columns(), m.U)
        rows = np.arange(0, m.n, 2, dtype=np.int32)
        ctx.set_end(rows, np.full(rows.size, INT64_MIN, np.int64))
        m.set_end(rows, np.full(rows.size, INT64_MIN, np.int64))
        wide = ctx.table_info()
        compact_both(ctx, m, INT64_MIN, shrink=True, tag="shrink")
        ref.load_columns(*m.columns(), m.U)
        got, want = ctx.table_info(), ref.table_info()
        assert got["table_bytes"] == want["table_bytes"] == 24 * m.n < wide["table_bytes"]
        assert got["workspace_bytes"] == want["workspace_bytes"] < wide["workspace_bytes"]
        assert got["derived_bytes"] == want["derived_bytes"]
        same(ctx.scan(t0, INT64_MIN), m.scan(t0, INT64_MIN, ALL), "scan after the shrink")


# ------------------------------------------------------------------------------------------------ 7. compact_translate
def test_compact_translate(gpu_ctx, oracle):
    ctx = gpu_ctx
    rng = np.random.default_rng(7)
    m = make_model(oracle, 61, 1_200_011, 997, 8)
    load(ctx, m)
    rows = rng.choice(m.n, m.n // 2, replace=False).astype(np.int32)
    ctx.set_end(rows, np.full(rows.size, INT64_MIN, np.int64))
    m.set_end(rows, np.full(rows.size, INT64_MIN, np.int64))
    n_old = m.n
    new_of_old, old_of_new = compact_both(ctx, m, INT64_MIN, tag="translate")
    assert ctx.compact_translate([]).size == 0
    assert np.array_equal(ctx.compact_translate(old_of_new[:1000]), np.arange(1000))                       # kept
    assert np.all(ctx.compact_translate(np.sort(rows)[:1000]) == -1)                                       # dropped
    odd = np.array([-1, n_old, n_old + 1, 2 ** 31 - 1, -(2 ** 31), 0, n_old - 1], np.int32)                # out of range
    assert np.array_equal(ctx.compact_translate(odd), CM.translate(new_of_old, odd))
    many = rng.integers(-5, n_old + 5, 1_000_000).astype(np.int32)
    got = ctx.compact_translate(many)
    assert got.dtype == np.int32 and np.array_equal(got, CM.translate(new_of_old, many))
    assert many.min() < 0, "the caller's array is not written"


# ------------------------------------------------------------------------------------------------ 8. sharded context
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_context_keeps_global_rows(pie, oracle, world):
    import torch
    t0 = oracle.T0_MS
    rng = np.random.default_rng(world)
    rank = world - 1
    with pie.PieScan(0) as ctx:
        m = make_model(oracle, 71, 300_011, 1201, 16)
        load(ctx, m)
        assert ctx.shard_table(rank, world) == m.shard_table(rank, world)
        ctx.set_disciplines(ALL, m.D)
        assert np.array_equal(ctx.shard_maps()[0], m.global_rows)
        users_before = ctx.shard_maps()[1].copy()
        kill_rows(ctx, m, rng, 0.5)
        compact_both(ctx, m, t0 - 15 * DAY, tag=("sharded", world))
        rows_global, users_global = ctx.shard_maps()
        assert np.array_equal(rows_global, m.global_rows), "local row -> ORIGINAL global row of the kept rows"
        assert np.array_equal(users_global, users_before), "the user map is untouched"
        want = m.expired_queue(t0 - 10 * DAY, t0)
        assert np.array_equal(ctx.expired_queue(t0 - 10 * DAY, t0), want) and want.size > 0
        cap = int(want.size) + 8
        msg = torch.full((2 + 2 * cap + 1,), -7, dtype=torch.int32, device="cuda:0")
        ctx.queue_pack_device(msg.data_ptr(), cap, 0)
        ctx.synchronize()
        torch.cuda.synchronize()
        host = msg.cpu().numpy()
        assert host[0] == want.size and host[1] == 0
        assert np.array_equal(host[2:2 + want.size], m.global_rows[want]), "the packed queue carries the original global rows"
        assert np.array_equal(host[2 + cap:2 + cap + want.size], want)
        same(ctx.scan(t0, INT64_MIN), m.scan(t0, INT64_MIN, ALL), "sharded scan after")
        # a second compaction composes on the map
        rows = np.arange(0, m.n, 2, dtype=np.int32)
        ctx.set_end(rows, np.full(rows.size, INT64_MIN, np.int64))
        m.set_end(rows, np.full(rows.size, INT64_MIN, np.int64))
        compact_both(ctx, m, INT64_MIN, shrink=True, tag=("sharded again", world))
        assert np.array_equal(ctx.shard_maps()[0], m.global_rows)
        # rows appended behind the shard have no global row: the map covers the kept rows in front of them, the tail stays a tail
        k = 500
        s2 = (int(m.start.max()) + np.arange(k)).astype(np.int64)
        e2 = np.where(np.arange(k) % 3 == 0, INT64_MIN, t0 + HOUR).astype(np.int64)
        u2, d2 = (np.arange(k) % m.U).astype(np.int32), (np.arange(k) % m.D).astype(np.int32)
        ctx.append_rows(s2, e2, u2, d2, m.U)
        m.append_rows(s2, e2, u2, d2, m.U)
        rows = np.arange(1, m.n - k, 3, dtype=np.int32)
        ctx.set_end(rows, np.full(rows.size, INT64_MIN, np.int64))
        m.set_end(rows, np.full(rows.size, INT64_MIN, np.int64))
        covered = m.global_rows.size
        compact_both(ctx, m, INT64_MIN, tag=("sharded with a tail", world))
        assert m.global_rows.size == covered - rows.size and m.n == m.global_rows.size + k - (k + 2) // 3
        assert np.array_equal(ctx.shard_maps()[0][:m.global_rows.size], m.global_rows)
        with pytest.raises(pie.PieError) as ei:      # the tail still has no global row: as before the compaction
            ctx.expired_queue(t0 - DAY, t0, fetch=False)
            ctx.queue_info()
        assert ei.value.code == PIE_E_STATE
