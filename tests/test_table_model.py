"""CPU self-checks of tests/table_model.py: the model's scans and mutators against the C oracle on chains of mutations, and the
lattice table's values against the bin edges of the documented key definition."""
import numpy as np
import pytest

import table_model as T
from table_model import ALL, DAY, HOUR, INT64_MIN


def test_model_imports_without_a_gpu():
    assert len(T.PATHS) == 9 and T.chain_config(3) == T.chain_config(3) and T.chain_config(3) != T.chain_config(4)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_scans_match_the_c_oracle_over_mutations(oracle, seed):
    rng = np.random.default_rng(seed)
    n, U, D = 60011, (3, 211, 997)[seed - 1], (7, 32, 64)[seed - 1]
    t0 = oracle.T0_MS
    m = T.TableModel(oracle)
    m.load(*oracle.gen(seed, n, 0, n, U, D, seed), U, D)

    def check(tag):
        qs = [(t0 - 6 * HOUR, t0 - 61 * DAY, ALL), (t0 - 30 * DAY, INT64_MIN, 0x5555555555555555), (INT64_MIN, INT64_MIN, 1 << 63 | 1),
              (int(m.end.max()), INT64_MIN, ALL), (int(m.end[m.end != INT64_MIN][7]) - 1, int(m.start[9]), ALL)]
        for q, got in zip(qs, m.scan_many(qs)):
            T.same(got, oracle.scan(*m.columns(), m.U, q[0], q[1], q[2] & m.lim()), (tag, q))
        assert np.array_equal(m.expired_queue(t0 - DAY, t0), oracle.expired_queue(m.end, t0 - DAY, t0))
        for now, win in ((t0, 12 * HOUR), (t0 - 100 * DAY, 0), (2 ** 62, 30 * DAY)):
            assert np.array_equal(m.archive_queue(now, win), oracle.archive_queue(m.start, m.end, m.user, m.U, now, win)), (tag, now, win)

    check("loaded")
    rows = rng.choice(n, 4000, replace=False).astype(np.int32)
    ne = (t0 + rng.integers(-40 * DAY, DAY, rows.size)).astype(np.int64)
    ne[:100], ne[100:200] = INT64_MIN, 2 ** 63 - 1
    m.set_end(rows, ne)
    check("set_end")
    gone = m.delete_user(1)
    assert gone.size and np.all(m.end[gone] == INT64_MIN) and m.delete_user(1).size == 0 and m.delete_user(U).size == 0
    for months, tz in ((3, -5 * HOUR), (2, 0), (1, 330 * 60000)):   # each purges what the one before left
        now = t0 - 20 * DAY
        want = oracle.retention_queue(m.start, m.end, now, months, tz)
        assert np.array_equal(m.retention_purge(now, months, tz), want) and want.size
    cutoff = int(np.quantile(m.start, 0.05))
    want = np.nonzero((m.start < cutoff) & (m.end != INT64_MIN))[0]
    assert np.array_equal(m.prune_before(cutoff), want)
    check("tombstoned")
    k = 900
    s2 = (t0 + rng.integers(-DAY, DAY, k)).astype(np.int64)
    m.append_rows(s2, s2 + 12 * HOUR, rng.integers(0, U + 4, k).astype(np.int32), rng.integers(0, D, k).astype(np.int32), U + 4)
    check("appended")
    if U >= 3:
        from sph_pie_amd.shard import partition_by_user_hash
        sh = partition_by_user_hash(*m.columns(), m.U, 3)[1]
        assert m.shard_table(1, 3) == (sh["rows"].size, sh["n_users"])
        for got, name in zip(m.columns(), ("start", "end", "user", "disc")):
            assert np.array_equal(got, sh[name]), name
        check("sharded")


def test_add_months_matches_the_oracle(oracle):
    rng = np.random.default_rng(9)
    ts = np.concatenate([oracle.T0_MS + rng.integers(-900 * DAY, 900 * DAY, 3000), [1706659200000, 1703980800000 + 5, 1709164800000]]).astype(np.int64)
    for months in (1, 2, 3, 14, -2):
        for tz in (0, 330 * 60000, -5 * HOUR):
            got = T.add_months(ts, months, tz)
            assert [int(x) for x in got] == [oracle.add_months(int(t), months, tz) for t in ts], (months, tz)


def test_lattice_values_are_bin_edges(oracle):
    """Under the key definition the table derives from its own `end` column, every lattice value is the lower edge of a bin of
    the 15-bit key, the fine key's base is an occupied lattice value, and every lattice value at or above it (below the fine
    clamp) is the lower edge of a fine bin."""
    s, e, u, d, U, D, values = T.lattice_table(oracle)
    pitch = 1 << T.LATTICE_SHIFT
    base, shift, fbase, fshift = T.key_params(e)
    assert 2000 < e.size < 5000 and np.array_equal(np.unique(e), values)
    assert base == int(values[0]) and np.all((values - base) % pitch == 0)
    assert shift == T.LATTICE_SHIFT, "the pitch is the bin width of the 15-bit key"
    assert fshift <= shift and fbase in set(values.tolist()) and (fbase - base) % pitch == 0
    frac_below = np.count_nonzero(e < fbase) / e.size
    assert 0.85 < frac_below <= 0.9, "the fine key's base sits just below the 90th percentile"
    for v in values.tolist():
        assert T.key_of(v, base, shift) == T.key_of(v - 1, base, shift) + 1 == (v - base) // pitch + 1
        assert T.key_of(v, base, shift) < T.KEY_MAX
        if v >= fbase:
            fk = T.key_of(v, fbase, fshift, T.FINE_KEY_MAX)
            assert fk == T.key_of(v - 1, fbase, fshift, T.FINE_KEY_MAX) + 1 and fk < T.FINE_KEY_MAX
    # several rows on every value, with different users and disciplines
    for v in values[[0, 5, -200, -1]].tolist():
        at = np.nonzero(e == v)[0]
        assert at.size >= 4 and np.unique(u[at]).size >= 3 and np.unique(d[at]).size >= 2
    # the tie table: a run of equal starts longer than a wave and than the 16-record direct bucket, for one user
    s, e, u, d, U, D = T.tie_table(oracle)
    assert np.unique(s[u == 0]).size == 1 and np.count_nonzero(u == 0) > 64 and np.any(d >= 64) and np.any(d < 0) and np.any(d == 63)


def test_set_end_with_repeated_rows_keeps_the_last_value(oracle):
    """TableModel.set_end against a plain loop over the elements in array order: repeats next to each other, far apart, with
    equal and with different values, tombstones among them; rows the call does not name stay as they were."""
    rng = np.random.default_rng(12)
    n = 500
    for k, distinct in ((1, 1), (2, 1), (300, 40), (16384, 40), (16384, n), (400, 400)):
        m = T.TableModel(oracle)
        m.load(*oracle.gen(5, n, 0, n, 7, 4, 0), 7, 4)
        before = m.end.copy()
        pool = rng.choice(n, min(distinct, n), replace=False)
        rows = rng.choice(pool, k).astype(np.int32) if distinct < k else rng.permutation(n)[:k].astype(np.int32)
        ne = rng.choice(np.array([INT64_MIN, 2 ** 63 - 1, oracle.T0_MS, oracle.T0_MS + 1], np.int64), k) + 0
        ne[::3] = rng.integers(-2 ** 62, 2 ** 62, ne[::3].size)
        want = [int(v) for v in before]
        for r, v in zip(rows.tolist(), ne.tolist()):
            want[r] = v
        m.set_end(rows, ne)
        assert m.end.dtype == np.int64 and [int(v) for v in m.end] == want, (k, distinct)
        untouched = np.setdiff1d(np.arange(n), rows)
        assert np.array_equal(m.end[untouched], before[untouched])


# ------------------------------------------------------------------------------------------------ the user axis
USER_AXIS_N, USER_AXIS_D = 300007, 32
USER_AXIS_SIZES = [65536, 65537, 65793, 100003, 262145, 524288, 524289]


@pytest.mark.parametrize("U", USER_AXIS_SIZES)
def test_planted_buckets_have_the_stated_sizes(oracle, U):
    """What tests/test_gpu_user_axis.py relies on: under the queries of stage k every planted user's union holds exactly
    min(size, PLANT_STAGE_ROWS[k]) rows for 1, 16, 64 and 512 queries alike, nobody else's exceeds 16, no bucket exceeds 64
    before stage 4, the places cover tiles 0, 255, 256, 257 where they exist, the last full tile, user U - 1 and two tiles that
    are congruent mod 64, and the queries' masks differ on the planted rows.  The numpy union equals the C oracle's answers."""
    n, D, t0 = USER_AXIS_N, USER_AXIS_D, oracle.T0_MS
    cols, planted = T.plant_user_buckets(oracle.gen(11, n, 0, n, U, D, 0), U, D, t0)
    tiles = sorted({u // T.USER_TILE for u in planted} - {T.PLANT_GROW_USER // T.USER_TILE})
    n_tiles = (U + T.USER_TILE - 1) // T.USER_TILE
    assert 0 in tiles and U // T.USER_TILE - 1 in tiles and n_tiles - 1 in tiles and planted[U - 1] == 64
    assert [t for t in (255, 256, 257) if t < n_tiles] == [t for t in (255, 256, 257) if t in tiles]
    assert any(a != b and a % T.MQ_SLOTS == b % T.MQ_SLOTS for a in tiles for b in tiles)
    for t in tiles:
        if min(T.USER_TILE, U - t * T.USER_TILE) == T.USER_TILE:
            assert sorted(planted[u] for u in planted if u // T.USER_TILE == t and u != T.PLANT_GROW_USER) == list(T.PLANT_SIZES)
    assert planted[T.PLANT_GROW_USER] == 65 and np.all(np.bincount(cols[2], minlength=U)[list(planted)] >= 1)
    users = np.array(sorted(planted))
    sizes = np.array([planted[int(u)] for u in users])
    for stage, top in enumerate(T.PLANT_STAGE_ROWS):
        for k in (1, 16, 64, 512):
            got = T.union_sizes(cols, U, D, T.user_axis_queries(t0, k, stage))
            assert np.array_equal(got[users], np.minimum(sizes, top)), (stage, k)
            assert int(got.max()) == top, (stage, k, "the largest bucket of the table is not the stage's")
            got[users] = 0
            assert got.max() <= 16, (stage, k, "a bucket that is not planted")
    # one stage against the C oracle: the union, its sizes, and masks that differ inside the planted buckets
    qs = T.user_axis_queries(t0, 16, 3)
    answers = [oracle.scan(*cols, U, now, cutoff, mask & ((1 << D) - 1)) for now, cutoff, mask in qs]
    uoff, rows, masks = T.union_from_answers(cols[0], cols[2], U, answers)
    assert np.array_equal(np.diff(uoff), T.union_sizes(cols, U, D, qs))
    T.check_union("planted", (uoff, rows, masks.reshape(-1)), answers, False)
    big = int(users[sizes == 64][0])
    in_big = slice(int(uoff[big]), int(uoff[big + 1]))
    assert np.unique(masks[in_big]).size >= 8, "the queries' masks do not differ on the planted rows"
    assert np.unique(cols[0][rows[in_big]]).size <= 5, "no equal starts inside the bucket"
    for q, (c, off, idx) in enumerate(answers):
        assert np.array_equal(c, np.diff(off)) and idx.size == off[-1]
    msg, written = T.union_message(U, U + 3, rows.size + 2, (uoff, rows, masks), 16, False)
    assert msg[U + 1] == msg[U + 4] == rows.size and not written[U + 5 + rows.size] and written[U + 5 + rows.size + 2]


def test_user_axis_boundaries():
    """The capacity arithmetic the GPU tests state in their docstrings."""
    assert T.batch_supported_users(524288) and not T.batch_supported_users(524289) and T.BATCH_MAX_USERS == 524288
    assert T.FUSED_SCAN_MAX_USERS == 1048576
    # the wide rule: 300 000 users loaded, one more appended: the user arrays double to 600 000
    cap = 2 * 300000
    assert T.batch_supported_users(300001)
    assert T.wide_union_fits(cap, 4) and T.wide_union_fits(cap, 5) and not T.wide_union_fits(cap, 6)
    assert T.union_slots_fit(cap, T.UNION_SHIFT_MAX)
    assert T.wide_union_fits(300000, 6), "without the doubling the rule is not reached"
    # growth across 524 288: 524 200 users loaded, then more: 1 048 400; wide batches keep their union while buckets hold 16 slots
    assert T.wide_union_fits(2 * 524200, 4) and T.wide_union_fits(2 * 524200, 5) and not T.wide_union_fits(2 * 524200, 6)
    # single scans: a bucket of 100 rows asks for 128 slots; 2 GiB hold 64 per user at 1 048 577 users and 32 at 3 000 000
    assert T.union_slots_fit(1048577, 6) and not T.union_slots_fit(1048577, 7)
    assert T.union_slots_fit(3000000, 5) and not T.union_slots_fit(3000000, 6)
