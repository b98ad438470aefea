"""GPU: the ordered run (sph-pie_amd/csrc/pie_ordered.h: the table a second time in (user, start, row) order; a query is a
filter over positions) against the oracle — bit-exact counts / offsets / idx — in both of its forms (dense, keyed on the 2- and
the 1-byte key), on ragged / empty / skewed tables, after every writer of `end`, after the changes that invalidate it, and under
the adaptive rule that builds it.  Through the C ABI (ctypes).  The boundaries of its kernels (cross-chunk carries, unit and group
boundaries, insert edges) are driven by designed tables in test_gpu_ordered_paths.py / ordered_cases.py / test_ordered_cases_cpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT64_MIN = -(2 ** 63)
ALL = 2 ** 64 - 1
DAY = 86400 * 1000
HOUR = 3600 * 1000
SEED = 0x0D0E0D


def assert_same(got, want, tag=""):
    for name, a, b in zip(("counts", "offsets", "idx"), got, want):
        assert a.dtype == b.dtype, (tag, name)
        assert np.array_equal(a, b), (tag, name)


def queries(oracle, cols):
    """sparse (keyed form, fine key), mid (keyed on the 2-byte key), dense (dense form), everything, nothing, a cutoff taken from
    the data, a `now` below every key base (key(now) == 0: every row is a candidate)"""
    t0 = oracle.T0_MS
    s = cols[0]
    some_start = int(s[s.size // 3]) if s.size else t0
    return [(t0 - 6 * HOUR, t0 - 61 * DAY, 0x5555555555555555),
            (t0 - 10 * DAY, t0 - 61 * DAY, ALL),
            (t0 - 100 * DAY, t0 - 61 * DAY, 0xAAAAAAAAAAAAAAAA),
            (INT64_MIN, INT64_MIN, ALL),
            (2 ** 62, INT64_MIN, ALL),
            (t0 - 3 * DAY, some_start, 0x00000000FFFF0000 | 1),
            (t0 - 4000 * DAY, INT64_MIN, ALL)]


def check(ctx, oracle, cols, U, D, q, tag, want_ordered=True):
    s, e, u, d = cols
    now, cutoff, mask = q
    lim = ALL if D >= 64 else (1 << D) - 1
    ctx.set_disciplines(mask, D)
    got = ctx.scan(now, cutoff)
    assert_same(got, oracle.scan(s, e, u, d, U, now, cutoff, mask & lim), tag)
    if want_ordered:
        assert ctx.stats()["k1_variant"] & 0x2000, (tag, hex(ctx.stats()["k1_variant"]))


@pytest.mark.parametrize("n,U,D,flags", [
    (1, 1, 1, 0), (7, 3, 2, 1), (300, 50, 7, 0), (4097, 9, 7, 3), (70001, 333, 32, 0), (70001, 40000, 64, 2),
    (1 << 20, 5000, 32, 3), (1 << 20, 600000, 32, 4), (1000003, 10, 5, 1), (262144, 1000, 32, 7),
])
def test_ordered_run_equals_the_oracle(pie, oracle, n, U, D, flags):
    cols = oracle.gen(SEED + n, n, 0, n, U, D, flags)
    with pie.PieScan(0) as ctx:
        ctx.load_columns(*cols, U)
        ctx.set_ordered_run(2)
        forms = set()
        for k, q in enumerate(queries(oracle, cols)):
            check(ctx, oracle, cols, U, D, q, f"n={n} U={U} flags={flags} q{k}")
            forms.add(ctx.stats()["k1_variant"])
        if n >= 70001:
            assert 0x2003 in forms and (0x2400 in forms or 0x2C00 in forms), [hex(f) for f in forms]
        info = ctx.table_info()
        assert info["ordered_builds"] == 1 and info["ordered_rows"] <= n <= info["ordered_positions"] and info["ordered_bytes"] > 0


def test_ordered_run_empty_and_unselectable_tables(pie, oracle):
    """no rows; only tombstones; only disciplines outside the table: the run holds nothing and every answer is empty"""
    t0 = oracle.T0_MS
    with pie.PieScan(0) as ctx:
        ctx.set_ordered_run(2)
        z = np.zeros(0, np.int64)
        ctx.load_columns(z, z, np.zeros(0, np.int32), np.zeros(0, np.int32), 4)
        got = ctx.scan(t0, INT64_MIN)
        assert got[2].size == 0 and got[0].tolist() == [0, 0, 0, 0]
        n = 5000
        s = np.full(n, t0, np.int64)
        u = (np.arange(n) % 7).astype(np.int32)
        ctx.load_columns(s, np.full(n, INT64_MIN, np.int64), u, np.zeros(n, np.int32), 7)
        assert ctx.scan(INT64_MIN, INT64_MIN)[2].size == 0
        assert ctx.table_info()["ordered_rows"] == 0
        ctx.load_columns(s, s + HOUR, u, np.full(n, 64, np.int32), 7)
        assert ctx.scan(INT64_MIN, INT64_MIN)[2].size == 0


def test_ordered_run_skewed_users_and_equal_keys(pie, oracle):
    """a head user owning half the rows, starts and ends on whole hours (many equal sort keys, ties broken by row)"""
    n, U, D = 400000, 2000, 16
    s, e, u, d = [c.copy() for c in oracle.gen(SEED, n, 0, n, U, D, 0)]
    rng = np.random.default_rng(5)
    u = np.where(rng.random(n) < 0.5, 17, u).astype(np.int32)
    s = (s // HOUR) * HOUR
    e = (e // HOUR) * HOUR
    cols = (s, e, u, d)
    with pie.PieScan(0) as ctx:
        ctx.load_columns(*cols, U)
        ctx.set_ordered_run(2)
        for k, q in enumerate(queries(oracle, cols)):
            check(ctx, oracle, cols, U, D, q, f"skew q{k}")


def test_ordered_run_follows_every_writer_of_end(pie, oracle):
    """touch (set_end), delete (set_end to the tombstone), delete_user, prune_before, retention purge: the run's copies of
    `end` and of both keys stay in step; a tombstoned row that comes back to life is not in the run — the run is dropped and
    rebuilt; an append invalidates it."""
    n, U, D = 200000, 700, 8
    t0 = oracle.T0_MS
    s, e, u, d = [c.copy() for c in oracle.gen(SEED + 1, n, 0, n, U, D, 0)]
    rng = np.random.default_rng(11)
    dead = rng.choice(n, 500, replace=False).astype(np.int32)
    e[dead] = INT64_MIN                                      # tombstoned before the run is built: not in the run
    qs = [(t0 - 6 * HOUR, t0 - 61 * DAY, ALL), (t0 - 100 * DAY, t0 - 61 * DAY, 0x55), (t0 - 30 * DAY, INT64_MIN, ALL)]

    def all_queries(ctx, tag, want_ordered=True):
        for k, q in enumerate(qs):
            check(ctx, oracle, (s, e, u, d), U, D, q, f"{tag} q{k}", want_ordered)

    with pie.PieScan(0) as ctx:
        ctx.load_columns(s, e, u, d, U)
        ctx.set_ordered_run(2)
        all_queries(ctx, "fresh")
        assert ctx.table_info()["ordered_rows"] == n - 500
        # touches: live again / further out / into the past, incl. values beyond the key range
        rows = rng.choice(np.setdiff1d(np.arange(n), dead), 3000, replace=False).astype(np.int32)
        new_end = np.where(rng.random(3000) < 0.5, t0 + rng.integers(0, 40 * DAY, 3000), t0 - rng.integers(0, 200 * DAY, 3000)).astype(np.int64)
        ctx.set_end(rows, new_end)
        e[rows] = new_end
        all_queries(ctx, "touched")
        # deletes
        gone = rows[:700]
        ctx.set_end(gone, np.full(700, INT64_MIN, np.int64))
        e[gone] = INT64_MIN
        all_queries(ctx, "deleted")
        # delete_user / prune_before tombstone on the device
        del_rows = ctx.delete_user(5)
        assert np.array_equal(np.sort(del_rows), np.nonzero((u == 5) & (e != INT64_MIN))[0].astype(np.int32))
        e[u == 5] = INT64_MIN
        all_queries(ctx, "user deleted")
        pruned = ctx.prune_before(int(t0 - 90 * DAY))
        e[pruned] = INT64_MIN
        all_queries(ctx, "pruned")
        assert ctx.table_info()["ordered_builds"] == 1       # all of the above were mirrored, none rebuilt the run
        # rows of the run brought back to life are still its rows
        ctx.set_end(gone[:100], np.full(100, t0 + DAY, np.int64))
        e[gone[:100]] = t0 + DAY
        all_queries(ctx, "revived inside the run")
        assert ctx.table_info()["ordered_builds"] == 1
        # a row that was a tombstone when the run was built is not in it: reviving it drops the run, the next scan rebuilds
        ctx.set_end(dead[:3], np.full(3, t0 + DAY, np.int64))
        e[dead[:3]] = t0 + DAY
        assert ctx.table_info()["ordered_rows"] == 0
        all_queries(ctx, "revived outside the run")
        assert ctx.table_info()["ordered_builds"] == 2
        # a back-fill (starts anywhere in the last 120 days: rows that belong hundreds of rows back): the run is dropped
        k = 1000
        a = [c.copy() for c in oracle.gen(SEED + 2, k, 0, k, U, D, 0)]
        ctx.append_rows(*a, U)
        s, e, u, d = [np.concatenate([x, y]) for x, y in zip((s, e, u, d), a)]
        assert ctx.table_info()["ordered_rows"] == 0
        all_queries(ctx, "appended")
        assert ctx.table_info()["ordered_builds"] == 3


def test_ordered_run_takes_appends_in_time_order(pie, oracle):
    """createSession: rows whose start is not below their user's last start go into the spare slots of the user's segment — the
    run stays valid (no rebuild), answers stay exact, touches of the new rows are mirrored; users that did not exist when the
    run was built have segments too; when a segment fills up the run is re-spread (a linear move into fresh segments, no rebuild)
    and the rows left over take their places; rows a little out of time order are inserted at their places; a back-fill (a row that
    belongs hundreds of rows back) drops the run."""
    n, U, D = 200000, 300, 8                                                      # ~666 rows per user: ~45 spare slots each
    t0 = oracle.T0_MS
    s, e, u, d = [c.copy() for c in oracle.gen(SEED + 7, n, 0, n, U, D, 0)]
    qs = [(t0 + 6 * HOUR, t0 - 61 * DAY, ALL), (t0 - 100 * DAY, t0 - 61 * DAY, 0x55), (t0 + 2 * DAY, INT64_MIN, ALL), (INT64_MIN, INT64_MIN, ALL)]
    rng = np.random.default_rng(3)
    with pie.PieScan(0) as ctx:
        ctx.load_columns(s, e, u, d, U)
        ctx.set_ordered_run(2)

        def all_queries(tag, n_users):
            for k, q in enumerate(qs):
                check(ctx, oracle, (s, e, u, d), n_users, D, q, f"{tag} q{k}")
        all_queries("fresh", U)
        now = t0 + HOUR
        # the first append (of a new user) outgrows the loaded table's row and user capacity: the table is re-allocated (twice
        # the size, room for as many users again) and the run goes with it
        n_users = U + 1
        ctx.append_rows(np.array([now], np.int64), np.array([now + HOUR], np.int64), np.array([U], np.int32), np.array([0], np.int32), n_users)
        s, e, u, d = np.append(s, now), np.append(e, now + HOUR), np.append(u, U).astype(np.int32), np.append(d, 0).astype(np.int32)
        assert ctx.table_info()["ordered_rows"] == 0
        all_queries("grown", n_users)
        assert ctx.table_info()["ordered_builds"] == 2
        for step in range(12):
            k = int(rng.integers(1, 200))
            now += int(rng.integers(0, 5000))
            s2 = np.sort(now + rng.integers(0, 3, k)).astype(np.int64)            # equal and ascending starts inside one batch
            e2 = s2 + 12 * HOUR
            if step == 5:
                n_users = U + 8                                                   # users the run has only empty segments for
            u2 = rng.integers(0, n_users, k).astype(np.int32)
            if step % 3 == 0:
                u2[: min(k, 5)] = 11                                              # the same user several times in one batch
            d2 = rng.integers(0, D, k).astype(np.int32)
            ctx.append_rows(s2, e2, u2, d2, n_users)
            s, e, u, d = np.concatenate([s, s2]), np.concatenate([e, e2]), np.concatenate([u, u2]), np.concatenate([d, d2])
            now = int(s2[-1])
            if step % 4 == 1:                                                     # touch some of the rows just appended
                rows = np.arange(s.size - k, s.size, 3, dtype=np.int32)
                ne = (e[rows] + rng.integers(-20 * HOUR, 20 * HOUR, rows.size)).astype(np.int64)
                ctx.set_end(rows, ne)
                e[rows] = ne
            info = ctx.table_info()
            assert info["ordered_builds"] == 2 and info["ordered_rows"] == s.size, (step, info)
            all_queries(f"step {step}", n_users)
        # one user's segment fills up many times over in ONE append: a re-spread makes room for all of it
        k = 4000
        s2 = np.full(k, now + 10, np.int64)
        before = ctx.table_info()["ordered_respreads"]
        ctx.append_rows(s2, s2 + HOUR, np.full(k, 11, np.int32), np.zeros(k, np.int32), n_users)
        s, e, u, d = np.concatenate([s, s2]), np.concatenate([e, s2 + HOUR]), np.concatenate([u, np.full(k, 11, np.int32)]), np.concatenate([d, np.zeros(k, np.int32)])
        info = ctx.table_info()
        assert info["ordered_rows"] == s.size and info["ordered_respreads"] == before + 1 and info["ordered_builds"] == 2
        all_queries("segment overflow", n_users)
        now += 10
        # a batch out of time order inside itself, and rows a little late (before the rows just appended): inserted at their
        # places, the few rows behind them shift
        s2 = np.array([now + 100, now + 50, now - 3, now + 70, now - 40000], np.int64)
        u2 = np.array([3, 3, 12, 3, 12], np.int32)
        ctx.append_rows(s2, s2 + HOUR, u2, np.zeros(5, np.int32), n_users)
        s, e, u, d = np.concatenate([s, s2]), np.concatenate([e, s2 + HOUR]), np.concatenate([u, u2]).astype(np.int32), np.concatenate([d, np.zeros(5, np.int32)]).astype(np.int32)
        info = ctx.table_info()
        assert info["ordered_rows"] == s.size and info["ordered_builds"] == 2
        all_queries("a little out of order", n_users)
        # a back-fill: a row that belongs hundreds of rows back in its user's segment drops the run
        s2 = np.array([t0 - 100 * DAY], np.int64)
        ctx.append_rows(s2, s2 + HOUR, np.array([11], np.int32), np.zeros(1, np.int32), n_users)
        s, e, u, d = np.concatenate([s, s2]), np.concatenate([e, s2 + HOUR]), np.concatenate([u, [11]]).astype(np.int32), np.concatenate([d, [0]]).astype(np.int32)
        assert ctx.table_info()["ordered_rows"] == 0
        all_queries("back-fill", n_users)

def test_ordered_run_rejected_append_and_chains_of_one_user(pie, oracle):
    """an append that carries a user id outside the table is rejected as a whole: the table is unchanged, the run (some of the
    rows may already sit in its spare slots) is dropped and rebuilt by the next scan; batches with 2, 3, 4 and 5+ rows of one user
    with equal starts (the chain of a user's rows is put in batch order: in registers up to four, off the batch beyond) keep
    (start, row) order"""
    n, U, D = 100000, 400, 8
    t0 = oracle.T0_MS
    s, e, u, d = [c.copy() for c in oracle.gen(SEED + 21, n, 0, n, U, D, 0)]
    qs = [(t0 + HOUR, t0 - 61 * DAY, ALL), (INT64_MIN, INT64_MIN, ALL)]
    with pie.PieScan(0) as ctx:
        ctx.load_columns(s, e, u, d, U)
        ctx.set_ordered_run(2)
        now = t0 + HOUR
        ctx.append_rows(np.array([now], np.int64), np.array([now + HOUR], np.int64), np.array([0], np.int32), np.array([0], np.int32), U)  # capacity growth
        s, e, u, d = np.append(s, now), np.append(e, now + HOUR), np.append(u, 0).astype(np.int32), np.append(d, 0).astype(np.int32)
        for k, q in enumerate(qs):
            check(ctx, oracle, (s, e, u, d), U, D, q, f"grown q{k}")
        builds = ctx.table_info()["ordered_builds"]
        bad_u = np.array([3, 3, U + 5, 9], np.int32)
        with pytest.raises(Exception):
            ctx.append_rows(np.full(4, now + 1, np.int64), np.full(4, now + HOUR, np.int64), bad_u, np.zeros(4, np.int32), U)
        assert ctx.table_info()["ordered_rows"] == 0
        for k, q in enumerate(qs):
            check(ctx, oracle, (s, e, u, d), U, D, q, f"after the rejected append q{k}")
        assert ctx.table_info()["ordered_builds"] == builds + 1
        respreads = ctx.table_info()["ordered_respreads"]
        for step, users in enumerate(([5, 5], [6, 1, 6, 6], [7, 7, 2, 7, 7], [8] * 5 + [1], [9, 3] * 6, list(range(20)) + [4] * 7)):
            u2 = np.array(users, np.int32)
            k = u2.size
            s2 = np.full(k, now + 10 * (step + 1), np.int64)                      # equal starts: order is by row
            if step % 2:
                s2[::2] += 1                                                      # and not in time order inside the batch
            e2 = s2 + HOUR + np.arange(k)
            d2 = (np.arange(k) % D).astype(np.int32)
            ctx.append_rows(s2, e2, u2, d2, U)
            s, e, u, d = np.concatenate([s, s2]), np.concatenate([e, e2]), np.concatenate([u, u2]).astype(np.int32), np.concatenate([d, d2]).astype(np.int32)
            info = ctx.table_info()
            assert info["ordered_rows"] == s.size and info["ordered_builds"] == builds + 1 and info["ordered_respreads"] == respreads, (step, info)
            for k2, q in enumerate(qs):
                check(ctx, oracle, (s, e, u, d), U, D, (q[0] if q[0] == INT64_MIN else now + 20 * HOUR, q[1], q[2]), f"chains step {step} q{k2}")


def test_ordered_run_is_built_when_the_general_path_is_weak(pie, oracle):
    """mode 1 (the default): sparse queries on evenly spread users never build it; the second dense query in a row does,
    and from then on dense queries use it while sparse ones stay on the keyed general path; skewed users call for it too."""
    n, U, D = 1 << 20, 3000, 32
    t0 = oracle.T0_MS
    cols = oracle.gen(SEED + 3, n, 0, n, U, D, 0)
    sparse = (t0 - 6 * HOUR, t0 - 61 * DAY, 0x5555555555555555)
    dense = (t0 - 100 * DAY, t0 - 61 * DAY, ALL)
    with pie.PieScan(0) as ctx:
        ctx.load_columns(*cols, U)
        for k in range(4):
            check(ctx, oracle, cols, U, D, sparse, f"sparse {k}", want_ordered=False)
            assert not ctx.stats()["k1_variant"] & 0x2000
        assert ctx.table_info()["ordered_builds"] == 0
        check(ctx, oracle, cols, U, D, dense, "dense 0", want_ordered=False)      # nothing known yet
        check(ctx, oracle, cols, U, D, dense, "dense 1", want_ordered=False)      # wanted once
        check(ctx, oracle, cols, U, D, dense, "dense 2", want_ordered=False)      # wanted twice: built, used
        assert ctx.stats()["k1_variant"] == 0x2003
        assert ctx.table_info()["ordered_builds"] == 1
        check(ctx, oracle, cols, U, D, dense, "dense 3")
        check(ctx, oracle, cols, U, D, sparse, "sparse after dense")              # the last scan was dense: the run, keyed form
        check(ctx, oracle, cols, U, D, sparse, "sparse again", want_ordered=False)
        assert not ctx.stats()["k1_variant"] & 0x2000
    # skew
    s, e, u, d = [c.copy() for c in cols]
    u = np.where(np.random.default_rng(2).random(n) < 0.3, 9, u).astype(np.int32)
    with pie.PieScan(0) as ctx:
        ctx.load_columns(s, e, u, d, U)
        sparse_all = (sparse[0], sparse[1], ALL)
        for k in range(4):
            check(ctx, oracle, (s, e, u, d), U, D, sparse_all, f"skewed {k}", want_ordered=False)
        assert ctx.stats()["k1_variant"] & 0x2000 and ctx.table_info()["ordered_builds"] == 1


def test_ordered_run_two_scans_in_flight_and_batches(pie, oracle):
    """pipelined begin / begin / finish / finish on the run; a batch whose queries fall back (dense) is served by it"""
    n, U, D = 300000, 900, 16
    t0 = oracle.T0_MS
    cols = oracle.gen(SEED + 4, n, 0, n, U, D, 1)
    s, e, u, d = cols
    qs = [(t0 - 6 * HOUR - 1000 * k, t0 - (61 + k) * DAY) for k in range(6)] + [(t0 - 100 * DAY, t0 - 61 * DAY)]
    with pie.PieScan(0) as ctx:
        ctx.load_columns(*cols, U)
        ctx.set_disciplines(ALL, D)
        ctx.set_ordered_run(2)
        ctx.scan_begin(*qs[0])
        for k in range(len(qs)):
            if k + 1 < len(qs):
                ctx.scan_begin(*qs[k + 1])
            ctx.scan_finish()
            assert_same(ctx.read_results(), oracle.scan(s, e, u, d, U, qs[k][0], qs[k][1], (1 << D) - 1), f"pipelined {k}")
        batch = [(t0 - 100 * DAY, t0 - 61 * DAY, 0xFF), (t0 - 6 * HOUR, t0 - 61 * DAY, ALL), (t0 - 50 * DAY, INT64_MIN, 0xF0F0)]
        ctx.scan_batch(batch)
        for qi, (now, cutoff, mask) in enumerate(batch):
            assert_same(ctx.batch_read_results(qi), oracle.scan(s, e, u, d, U, now, cutoff, mask & ((1 << D) - 1)), f"batch q{qi}")


def test_ordered_run_is_built_under_a_pipelined_caller(pie, oracle):
    """two scans in flight at every begin (bench.py's loop): the build takes the free slot while the caller's scan stays in
    flight, and every answer before, at and after the build is exact"""
    n, U, D = 1 << 20, 3000, 32
    t0 = oracle.T0_MS
    cols = oracle.gen(SEED + 5, n, 0, n, U, D, 0)
    s, e, u, d = cols
    qs = [(t0 - 100 * DAY - 1000 * k, t0 - 61 * DAY - 7 * k) for k in range(8)]
    with pie.PieScan(0) as ctx:
        ctx.load_columns(*cols, U)
        ctx.set_disciplines(ALL, D)
        ctx.scan_begin(*qs[0])
        forms = []
        for k in range(len(qs)):
            if k + 1 < len(qs):
                ctx.scan_begin(*qs[k + 1])
            ctx.scan_finish()
            forms.append(ctx.stats()["k1_variant"])
            assert_same(ctx.read_results(), oracle.scan(s, e, u, d, U, qs[k][0], qs[k][1], ALL), f"pipelined {k}")
        assert ctx.table_info()["ordered_builds"] == 1
        assert not forms[0] & 0x2000 and forms[-1] == 0x2003, [hex(f) for f in forms]


def test_ordered_run_result_messages(pie, oracle):
    """the packed exchange message (offsets | M | rows) of a scan served by the ordered run equals the one packed from
    the oracle's answer"""
    import torch
    n, U, D = 200000, 500, 16
    t0 = oracle.T0_MS
    cols = oracle.gen(SEED + 6, n, 0, n, U, D, 0)
    s, e, u, d = cols
    u_pad = 512
    cap = n
    with pie.PieScan(0) as ctx:
        ctx.load_columns(*cols, U)
        ctx.set_disciplines(ALL, D)
        ctx.set_ordered_run(2)
        msg = torch.zeros(u_pad + 2 + cap, dtype=torch.int32, device="cuda:0")
        for now, cutoff in [(t0 - 100 * DAY, t0 - 61 * DAY), (t0 - 6 * HOUR, t0 - 61 * DAY)]:
            ctx.scan_begin_packed(now, cutoff, msg.data_ptr(), u_pad, cap)
            m, _ready = ctx.scan_finish_packed()
            ctx.synchronize()
            assert ctx.stats()["k1_variant"] & 0x2000
            w = oracle.scan(s, e, u, d, U, now, cutoff, (1 << D) - 1)
            got = msg.cpu().numpy()
            assert m == w[2].size
            assert np.array_equal(got[: U + 1], w[1].astype(np.int32)) and np.all(got[U + 1: u_pad + 2] == m)
            assert np.array_equal(got[u_pad + 2: u_pad + 2 + m], w[2])


def skewed_table(oracle, n, U, D, seed, head_share=0.4):
    s, e, u, d = [c.copy() for c in oracle.gen(seed, n, 0, n, U, D, 0)]
    rng = np.random.default_rng(seed)
    u = np.where(rng.random(n) < head_share, 7 % U, u).astype(np.int32)
    return s, e, u, d


@pytest.mark.parametrize("n,U,D", [(400000, 2000, 16), (70001, 333, 7), (1 << 20, 50000, 64)])
@pytest.mark.parametrize("nq", [1, 5, 16])
def test_ordered_batch_equals_separate_scans(pie, oracle, n, U, D, nq):
    """Q queries in ONE pass over the run's key column (the batched form a skewed table's batches take): every query's
    counts / offsets / idx equal the oracle's, with mixed now / cutoff / mask, a dense query that is taken out of the batch,
    a query that selects nothing, 1-byte and 2-byte key streams."""
    t0 = oracle.T0_MS
    cols = skewed_table(oracle, n, U, D, SEED + n + nq)
    s, e, u, d = cols
    lim = ALL if D >= 64 else (1 << D) - 1
    masks = [0x5555555555555555, ALL, 0xAAAAAAAAAAAAAAAA, 0x00000000FFFF0000 | 3, 0x1]
    base = [(t0 - 6 * HOUR - 977 * i - (i % 3) * HOUR, t0 - (61 + i % 4) * DAY - 13 * i, masks[i % len(masks)]) for i in range(nq)]
    with pie.PieScan(0) as ctx:
        ctx.load_columns(*cols, U)
        ctx.set_disciplines(ALL, D)
        ctx.set_ordered_run(2)
        ctx.scan(t0 - 6 * HOUR, t0 - 61 * DAY)                                   # builds the run
        assert ctx.table_info()["ordered_builds"] == 1
        variants = [base]
        if nq >= 5:
            mid = list(base)
            mid[1] = (t0 - 100 * DAY, t0 - 61 * DAY, ALL)                          # dense: leaves the batch, runs as a single scan
            mid[2] = (2 ** 62, INT64_MIN, ALL)                                     # nothing is live
            mid[3] = (t0 - 9 * DAY, INT64_MIN, 0xFF)                               # below the 1-byte key's base: the 2-byte stream
            variants.append(mid)
        for vi, qs in enumerate(variants):
            ctx.scan_batch_begin(qs)
            ms = ctx.scan_batch_finish()
            assert ctx.stats()["k1_variant"] & 0x3000 == 0x3000            # a batch, on the ordered run
            for qi, (now, cutoff, mask) in enumerate(qs):
                w = oracle.scan(s, e, u, d, U, now, cutoff, mask & lim)
                assert ms[qi] == w[2].size, (vi, qi)
                assert_same(ctx.batch_read_results(qi), w, f"variant {vi} q{qi}")
                for uu in (0, 7 % U, U - 1):
                    assert np.array_equal(ctx.batch_read_user_feed(qi, uu), w[2][w[1][uu]:w[1][uu + 1]])


def test_ordered_batch_pipelined_with_messages_and_changes(pie, oracle):
    """two batches in flight; per-query messages packed from the ordered batch; touches and in-order appends between batches"""
    import torch
    n, U, D = 300000, 900, 16
    t0 = oracle.T0_MS
    s, e, u, d = skewed_table(oracle, n, U, D, SEED + 99)
    lim = (1 << D) - 1
    u_pad, cap = U + 5, 60000
    stride = u_pad + 2 + cap
    rng = np.random.default_rng(8)
    with pie.PieScan(0) as ctx:
        ctx.load_columns(s, e, u, d, U)
        ctx.set_disciplines(ALL, D)
        ctx.set_ordered_run(2)
        ctx.scan(t0 - 6 * HOUR, t0 - 61 * DAY)
        batches = [[(t0 - 6 * HOUR - 1000 * (3 * b + i), t0 - (61 + i) * DAY, ALL if i % 2 else 0x0F0F) for i in range(4 + b)] for b in range(4)]
        ctx.scan_batch_begin(batches[0])
        for k in range(len(batches)):
            if k + 1 < len(batches):
                ctx.scan_batch_begin(batches[k + 1])
            ms = ctx.scan_batch_finish()
            for qi, (now, cutoff, mask) in enumerate(batches[k]):
                w = oracle.scan(s, e, u, d, U, now, cutoff, mask & lim)
                assert ms[qi] == w[2].size
                assert_same(ctx.batch_read_results(qi), w, f"pipelined batch {k} q{qi}")
        # messages
        msg = torch.full((4 * stride,), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        qs = batches[1][:4]
        ctx.scan_batch_begin_packed(qs, msg.data_ptr(), stride, u_pad, cap)
        ms, _ready = ctx.scan_batch_finish(packed=True)
        ctx.synchronize()
        got = msg.cpu().numpy()
        for qi, (now, cutoff, mask) in enumerate(qs):
            w = oracle.scan(s, e, u, d, U, now, cutoff, mask & lim)
            m = w[2].size
            a = got[qi * stride:(qi + 1) * stride]
            assert ms[qi] == m and np.array_equal(a[: U + 1], w[1].astype(np.int32)) and np.all(a[U + 1: u_pad + 2] == m)
            assert np.array_equal(a[u_pad + 2: u_pad + 2 + m], w[2])
        # the table changes between batches: touches, deletes, in-order appends (the first append re-allocates: one rebuild)
        now = t0 + HOUR
        for step in range(4):
            rows = rng.choice(s.size, 500, replace=False).astype(np.int32)
            ne = np.where(rng.random(500) < 0.2, INT64_MIN, now + rng.integers(0, 12 * HOUR, 500)).astype(np.int64)
            ctx.set_end(rows, ne)
            e[rows] = ne
            k = 300
            s2 = np.sort(now + rng.integers(0, 2000, k)).astype(np.int64)
            u2 = np.where(rng.random(k) < 0.4, 7, rng.integers(0, U, k)).astype(np.int32)
            d2 = rng.integers(0, D, k).astype(np.int32)
            ctx.append_rows(s2, s2 + 12 * HOUR, u2, d2, U)
            s, e, u, d = np.concatenate([s, s2]), np.concatenate([e, s2 + 12 * HOUR]), np.concatenate([u, u2]), np.concatenate([d, d2])
            now = int(s2[-1]) + 1
            qs = [(now + 1000 * i, t0 - (61 + i) * DAY, ALL) for i in range(6)]
            got = ctx.scan_batch(qs)
            for qi, (nw, ct, mk) in enumerate(qs):
                assert_same(got[qi], oracle.scan(s, e, u, d, U, nw, ct, mk & lim), f"changed step {step} q{qi}")


def test_ordered_run_spare_slots_are_never_live(pie, oracle):
    """a table whose `end` values are all <= 0 puts the key base below zero; the run's spare slots (a sixteenth of
    the positions + a few per user) must still read as dead — they carry PIE_END_NONE, not 0 — so the live rows a scan reports
    are exactly the table's, before and after a key refit, and the answers equal the oracle's."""
    n, U, D = 200000, 700, 8
    s, e, u, d = oracle.gen(SEED + 99, n, 0, n, U, D, 1)
    shift = int(e.max()) + 5 * DAY
    s, e = s - shift, e - shift           # every end below zero
    assert e.max() < 0
    cols = (s, e, u, d)
    with pie.PieScan(0) as ctx:
        ctx.load_columns(*cols, U)
        ctx.set_ordered_run(2)
        ctx.set_disciplines(ALL, D)
        now = int(np.sort(e)[int(n * 0.97)])
        for rnd in range(3):
            got = ctx.scan(now, INT64_MIN)
            assert_same(got, oracle.scan(s, e, u, d, U, now, INT64_MIN, (1 << D) - 1))
            st = ctx.stats()
            assert st["k1_variant"] & 0x2000
            assert st["live"] == int(np.count_nonzero(e > now)), (rnd, st["live"])
            if rnd == 0:   # re-end some rows far below everything: the key column is refitted from the run's own `end`
                rows = np.arange(0, n, 97, dtype=np.int32)
                e = e.copy()
                e[rows] = e[rows] - 400 * DAY
                ctx.set_end(rows, e[rows])
        # a `now` below every end: every position is a candidate, spare slots included; still only the table's rows are live
        got = ctx.scan(int(e.min()) - 1, INT64_MIN)
        assert_same(got, oracle.scan(s, e, u, d, U, int(e.min()) - 1, INT64_MIN, (1 << D) - 1))
        assert ctx.stats()["live"] == n
