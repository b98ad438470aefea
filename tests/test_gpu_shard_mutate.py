"""GPU, context level, no communicator: appends, touches and deletes by GLOBAL id on `world` sharded contexts of one GPU
(pie_shard_append_rows / pie_shard_set_end / pie_shard_delete_user / pie_shard_rows_to_*), against the UNSHARDED columns of
the oracle's generator mutated in numpy.  After every step every shard must be in step with that table: ascending maps that
cover every local row, the four columns equal at rows_global, users equal through users_global."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, D = 20260, 32
INT64_MIN = -(2 ** 63)
SHAPES = {1: (20000, 300), 2: (20000, 300), 3: (20000, 300), 5: (20000, 7)}  # world 5: one rank has no user and no rows


class Model:
    """The unsharded table and, per rank, the rows that rank's own compactions dropped."""

    def __init__(self, oracle, world, n0, u0):
        self.oracle, self.world = oracle, world
        self.s, self.e, self.u, self.d = (a.copy() for a in oracle.gen(SEED, n0, 0, n0, u0, D, 0))
        self.U = u0
        self.owner = np.array([oracle.shard_of(k, world) for k in range(u0)], np.int32)
        self.dropped = [np.zeros(n0, bool) for _ in range(world)]

    @property
    def N(self):
        return self.s.shape[0]

    def grow_users(self, n_users):
        more = [self.oracle.shard_of(k, self.world) for k in range(self.U, n_users)]
        self.owner = np.concatenate([self.owner, np.array(more, np.int32)])
        self.U = n_users

    def append(self, s, e, u, d, n_users):
        self.grow_users(n_users)
        self.s, self.e = np.concatenate([self.s, s]), np.concatenate([self.e, e])
        self.u, self.d = np.concatenate([self.u, u]), np.concatenate([self.d, d])
        self.dropped = [np.concatenate([x, np.zeros(s.shape[0], bool)]) for x in self.dropped]

    def set_end(self, rows, vals):
        for r, v in zip(rows.tolist(), vals.tolist()):  # array order: the last element on a row wins
            self.e[r] = v

    def held(self, rank):
        return np.nonzero((self.owner[self.u] == rank) & ~self.dropped[rank])[0].astype(np.int32)

    def users_of(self, rank):
        return np.nonzero(self.owner == rank)[0].astype(np.int32)

    def shard(self, rank):
        rows, users = self.held(rank), self.users_of(rank)
        return rows, users, self.s[rows], self.e[rows], np.searchsorted(users, self.u[rows]).astype(np.int32), self.d[rows]


def make(pie, world, n0, u0, ordered=None):
    ctxs = []
    for r in range(world):
        c = pie.PieScan(0)
        ctxs.append(c)
        if ordered is not None:
            c.set_ordered_run(ordered)
        c.gen_synthetic(SEED, n0, 0, n0, u0, D, 0)
        c.shard_table(r, world)
    return ctxs


def check(ctxs, m):
    for r, c in enumerate(ctxs):
        rows, users, s, e, u, d = m.shard(r)
        info = c.shard_info()
        assert (info["rank"], info["world"], info["rows_global"], info["users_global"]) == (r, m.world, m.N, m.U)
        assert c.n == rows.size and c.n_users == max(users.size, 1)
        assert int(c.stats()["rows"]) == rows.size and int(c.stats()["users"]) == max(users.size, 1)
        got_rows, got_users = c.shard_maps()
        assert np.array_equal(got_rows, rows), "rank %d: row map" % r
        assert np.array_equal(got_users[: users.size], users), "rank %d: user map" % r
        gs, ge, gu, gd = c.read_columns()
        assert np.array_equal(gs, s) and np.array_equal(gd, d), "rank %d: start / disc" % r
        assert np.array_equal(gu, u), "rank %d: user" % r
        assert np.array_equal(ge, e), "rank %d: end" % r
        assert info["map_bytes"] >= 4 * (rows.size + users.size)


def same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


def check_scans(ctxs, m, rng):
    o = m.oracle
    top = o.T0_MS + o.SPAN_MS
    full = 2 ** 64 - 1

    def query():
        return (int(top + rng.integers(-o.TTL_MS, o.TTL_MS // 2)), int(top - rng.integers(0, 4 * o.TTL_MS)),
                int(rng.integers(1, 2 ** 32)) | (1 << int(rng.integers(0, D))))

    q16, q70 = [query() for _ in range(16)], [query() for _ in range(70)]
    now, cutoff = int(top - o.TTL_MS // 3), int(top - 3 * o.TTL_MS)
    for r, c in enumerate(ctxs):
        _, users, s, e, u, d = m.shard(r)
        nu = max(users.size, 1)
        assert same(c.scan(now, cutoff), o.scan(s, e, u, d, nu, now, cutoff, full)), "rank %d: single scan" % r
        for q, got in zip(q16, c.scan_batch(q16)):
            assert same(got, o.scan(s, e, u, d, nu, *q)), "rank %d: batch" % r
        for q, got in zip(q70, c.scan_wide(q70)):
            assert same(got, o.scan(s, e, u, d, nu, *q)), "rank %d: wide batch" % r


class Chain:
    def __init__(self, ctxs, m, rng):
        self.ctxs, self.m, self.rng, self.t = ctxs, m, rng, 0

    def rows(self, k, users):
        o, rng = self.m.oracle, self.rng
        self.t += 1
        s = (o.T0_MS + o.SPAN_MS + self.t * 100000 + np.arange(k)).astype(np.int64)  # in creation order, as a session store appends
        e = s + rng.integers(o.TTL_MS // 4, o.TTL_MS, k)
        return s, e, np.asarray(users, np.int32), rng.integers(0, D, k).astype(np.int32)

    def append(self, k, new_users=0, users=None):
        m = self.m
        n_users = m.U + new_users
        if users is None:
            users = self.rng.integers(0, n_users, k)
            users[: min(new_users, k)] = np.arange(m.U, m.U + min(new_users, k))  # the new ids do appear
        s, e, u, d = self.rows(k, users)
        first, kept = m.N, []
        for c in self.ctxs:
            got_first, n_kept = c.shard_append_rows(s, e, u, d, n_users)
            assert got_first == first
            kept.append(n_kept)
        m.append(s, e, u, d, n_users)
        assert kept == [int((m.owner[u] == r).sum()) for r in range(m.world)]
        return kept

    def touch(self, k, recent=0):
        m, rng, o = self.m, self.rng, self.m.oracle
        rows = rng.integers(0, m.N, k).astype(np.int32)
        if recent:  # rows the step just before appended; no wait in between
            rows[: min(recent, k)] = np.arange(m.N - min(recent, k), m.N)
        if k >= 4:
            rows[k // 2] = rows[0]  # repeats: the last value wins
            rows[k - 1] = rows[1]
        vals = (o.T0_MS + o.SPAN_MS + rng.integers(-o.TTL_MS, o.TTL_MS, k)).astype(np.int64)
        vals[rng.random(k) < 0.2] = INT64_MIN  # tombstones among them
        for c in self.ctxs:
            c.shard_set_end(rows, vals)
        m.set_end(rows, vals)

    def delete(self, user):
        m = self.m
        want = np.nonzero((m.u == user) & (m.e != INT64_MIN))[0].astype(np.int32) if 0 <= user < m.U else np.zeros(0, np.int32)
        for r, c in enumerate(self.ctxs):
            got = c.shard_delete_user(user)
            mine = 0 <= user < m.U and m.owner[user] == r
            assert np.array_equal(got, want[~m.dropped[r][want]] if mine else np.zeros(0, np.int32)), "rank %d: delete of user %d" % (r, user)
        m.e[want] = INT64_MIN


def run_chain(pie, oracle, world, ordered=None):
    n0, u0 = SHAPES[world]
    m = Model(oracle, world, n0, u0)
    ctxs = make(pie, world, n0, u0, ordered)
    rng = np.random.default_rng(7000 + world)
    ch = Chain(ctxs, m, rng)
    one_rank = [k for k in range(u0) if m.owner[k] == m.owner[0]]
    steps = [
        lambda: ch.append(1), lambda: ch.touch(1, recent=1), lambda: ch.append(63, new_users=1), lambda: ch.append(64),
        lambda: ch.touch(257, recent=64), lambda: ch.append(65, new_users=37), lambda: ch.delete(3),
        lambda: ch.append(255), lambda: ch.append(256), lambda: ch.append(257), lambda: ch.touch(3000, recent=257),
        lambda: ch.append(50, users=rng.choice(one_rank, 50)),  # one rank keeps all of it: everybody's N_g still advances
        lambda: ch.append(4096), lambda: ch.touch(3000, recent=500), lambda: ch.append(40000, new_users=1),  # outgrows the capacity
        lambda: ch.touch(3000, recent=3000), lambda: ch.delete(-5), lambda: ch.delete(m.U), lambda: ch.delete(m.U + 1000),
        lambda: ch.append(64), lambda: ch.touch(257, recent=64),
        lambda: ch.append(0, new_users=5), lambda: ch.append(3, new_users=3), lambda: ch.touch(64, recent=3),  # users and no row
    ]
    steps += [(lambda r=r: ch.delete(int(m.users_of(r)[-1]))) for r in range(world) if m.users_of(r).size]
    try:
        check(ctxs, m)
        for i, step in enumerate(steps):
            step()
            check(ctxs, m)
            if i % 3 == 2:
                check_scans(ctxs, m, rng)
        check_scans(ctxs, m, rng)
        if world == 5:  # the rank that started with no user: its first user is local id 0, n_users still 1
            empty = [r for r in range(world) if not np.any(m.owner[:u0] == r)]
            assert empty and all(m.users_of(r).size >= 1 and int(m.users_of(r)[0]) >= u0 for r in empty)
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("world", (1, 2, 3, 5))
def test_chain_default(pie, oracle, world):
    run_chain(pie, oracle, world)


@pytest.mark.parametrize("world", (1, 2, 3, 5))
def test_chain_ordered_run(pie, oracle, world):
    run_chain(pie, oracle, world, ordered=2)


@pytest.mark.parametrize("async_mutations", ("0", "1"))
@pytest.mark.parametrize("world", (1, 2, 3, 5))
def test_chain_async_setting(pie, oracle, world, async_mutations, monkeypatch):
    monkeypatch.setenv("PIE_ASYNC_MUTATIONS", async_mutations)  # read when a context is created
    run_chain(pie, oracle, world)


def test_translation(pie, oracle):
    world = 3
    n0, u0 = SHAPES[world]
    m = Model(oracle, world, n0, u0)
    ctxs = make(pie, world, n0, u0)
    try:
        ch = Chain(ctxs, m, np.random.default_rng(5))
        ch.append(300, new_users=5)
        probe = np.concatenate([np.arange(0, m.N, 7), [m.N - 1, m.N, m.N + 5, -1, -(2 ** 31), 2 ** 31 - 1]]).astype(np.int32)
        for r, c in enumerate(ctxs):
            held = m.held(r)
            local = c.shard_rows_to_local(probe)
            is_held = np.isin(probe, held)
            assert np.array_equal(local[is_held], np.searchsorted(held, probe[is_held])) and np.all(local[~is_held] == -1)
            back = c.shard_rows_to_global(local)
            assert np.array_equal(back[is_held], probe[is_held]) and np.all(back[~is_held] == -1)
            edge = c.shard_rows_to_global(np.array([0, held.size - 1, held.size, -1, 2 ** 31 - 1], np.int32))
            assert edge.tolist() == [int(held[0]), int(held[-1]), -1, -1, -1]
    finally:
        for c in ctxs:
            c.close()


def test_compaction(pie, oracle):
    world = 2
    n0, u0 = SHAPES[world]
    m = Model(oracle, world, n0, u0)
    ctxs = make(pie, world, n0, u0)
    try:
        rng = np.random.default_rng(11)
        ch = Chain(ctxs, m, rng)
        ch.append(500, new_users=3)
        dead = rng.choice(m.N, 4000, replace=False).astype(np.int32)
        tomb = np.full(dead.size, INT64_MIN, np.int64)
        for c in ctxs:
            c.shard_set_end(dead, tomb)
        m.set_end(dead, tomb)
        check(ctxs, m)
        before = m.held(0)
        kept = ctxs[0].compact_rows()  # one shard only
        m.dropped[0] |= (m.e == INT64_MIN) & (m.owner[m.u] == 0)
        assert kept == m.held(0).size < before.size
        check(ctxs, m)
        gone = before[m.dropped[0][before]]
        assert np.all(ctxs[0].shard_rows_to_local(gone) == -1)
        # touches that name dropped global rows change nothing on the shard that dropped them
        alive = np.full(gone.size, oracle.T0_MS + oracle.SPAN_MS + 12345, np.int64)
        ctxs[0].shard_set_end(gone, alive)
        ctxs[1].shard_set_end(gone, alive)
        check(ctxs, m)
        # appends continue from N_g, the maps stay ascending and cover every row
        ch.append(700, new_users=2)
        ch.touch(300, recent=200)
        check(ctxs, m)
        check_scans(ctxs, m, rng)
        # the packed queue reports the ORIGINAL global rows
        rows, _, _, e, _, _ = m.shard(0)
        lo, hi = int(np.median(e[e != INT64_MIN])) - 10 ** 7, int(np.median(e[e != INT64_MIN])) + 10 ** 7
        want = np.nonzero((e > lo) & (e <= hi))[0]
        assert want.size > 0
        q = ctxs[0].expired_queue(lo, hi)
        assert np.array_equal(q, want)
        assert ctxs[0].queue_info()[:2] == (1, want.size)
        cap = want.size + 3
        msg, dev, host = ctxs[0].host_alloc(2 + 2 * cap + 1)
        try:
            ctxs[0].queue_pack_device(dev, cap, 0)
            ctxs[0].synchronize()
            assert msg[0] == want.size and np.array_equal(msg[2:2 + want.size], rows[want])
            assert np.array_equal(msg[2 + cap:2 + cap + want.size], want)
        finally:
            ctxs[0].host_free(host)
    finally:
        for c in ctxs:
            c.close()


def test_refusals_change_nothing(pie, oracle):
    world = 2
    n0, u0 = SHAPES[world]
    m = Model(oracle, world, n0, u0)
    ctxs = make(pie, world, n0, u0)
    plain = pie.PieScan(0)
    try:
        ch = Chain(ctxs, m, np.random.default_rng(3))
        ch.append(100)  # the table has room from here on: the in-place path is the one that must refuse cleanly
        s, e, u, d = ch.rows(8, np.arange(8))

        def refused(code, fn):
            with pytest.raises(pie.PieError) as ei:
                fn()
            assert ei.value.code == code
            check(ctxs, m)

        for c in ctxs:
            refused(-1, lambda: c.shard_append_rows(s, e, u, d, m.U - 1))                       # n_users_global < U_g
            bad = u.copy()
            bad[5] = m.U + 4
            refused(-1, lambda: c.shard_append_rows(s, e, bad, d, m.U + 4))                     # a user id outside [0, n_users_global)
            bad[5] = -1
            refused(-1, lambda: c.shard_append_rows(s, e, bad, d, m.U))
            for row in (-1, m.N, 2 ** 31 - 1):                                                  # a row outside [0, N_g)
                refused(-1, lambda: c.shard_set_end(np.array([0, row], np.int32), np.array([5, 5], np.int64)))
            huge = 2 ** 31 - 1 - m.N                                                            # N_g + k >= 2^31 - 1: refused before a row is read
            p = [a.ctypes.data_as(C.c_void_p) for a in (s, e, u, d)]
            assert c._lib.pie_shard_append_rows(c._ctx, p[0], p[1], p[2], p[3], huge, m.U, None, None) == -1
            check(ctxs, m)
            c.scan_begin(oracle.T0_MS, 0)                                                       # a scan in flight
            refused(-6, lambda: c.shard_append_rows(s, e, u, d, m.U))
            refused(-6, lambda: c.shard_set_end(np.array([0], np.int32), np.array([5], np.int64)))
            c.scan_finish()
            c.scan_batch_begin([(oracle.T0_MS, 0, 1), (oracle.T0_MS + 5, 0, 3)])                # a batch in flight
            refused(-6, lambda: c.shard_append_rows(s, e, u, d, m.U))
            refused(-6, lambda: c.shard_set_end(np.array([0], np.int32), np.array([5], np.int64)))
            refused(-6, lambda: c.shard_delete_user(3))
            c.scan_batch_finish()
            assert c.shard_append_rows(s[:0], e[:0], u[:0], d[:0], m.U) == (m.N, 0)             # k = 0 is fine ...
            c.shard_set_end(np.zeros(0, np.int32), np.zeros(0, np.int64))
        for c in ctxs:
            c.shard_append_rows(s[:0], e[:0], u[:0], d[:0], m.U + 2)                            # ... and still raises U_g
        m.grow_users(m.U + 2)
        check(ctxs, m)
        # a context that was never sharded
        plain.gen_synthetic(SEED, 1000, 0, 1000, 20, D, 0)
        for fn in (plain.shard_info, lambda: plain.shard_append_rows(s, e, u, d, 20), lambda: plain.shard_delete_user(1),
                   lambda: plain.shard_set_end(np.array([0], np.int32), np.array([5], np.int64)), lambda: plain.shard_rows_to_local([0])):
            with pytest.raises(pie.PieError) as ei:
                fn()
            assert ei.value.code == -6
        # plain pie_append_rows on a sharded context leaves rows with no global row
        c = ctxs[0]
        c.append_rows(s, e, np.zeros(8, np.int32), d, c.n_users)
        for fn in (lambda: c.shard_append_rows(s, e, u, d, m.U), lambda: c.shard_set_end(np.array([0], np.int32), np.array([5], np.int64)),
                   lambda: c.shard_delete_user(int(m.users_of(0)[0]))):
            with pytest.raises(pie.PieError) as ei:
                fn()
            assert ei.value.code == -6 and "no global row" in str(ei.value)
        # a table generated or loaded anew forgets the sharded state; pie_shard_table starts it over from the table it finds
        cols = oracle.gen(SEED, 1000, 0, 1000, 20, D, 0)
        for renew in (lambda: c.gen_synthetic(SEED, 1000, 0, 1000, 20, D, 0), lambda: c.load_columns(*cols, 20)):
            renew()
            for fn in (c.shard_info, lambda: c.shard_append_rows(s, e, u, d, 20)):
                with pytest.raises(pie.PieError) as ei:
                    fn()
                assert ei.value.code == -6
            c.shard_table(1, 2)
            info = c.shard_info()
            assert (info["rank"], info["world"], info["rows_global"], info["users_global"]) == (1, 2, 1000, 20)
            assert c.shard_append_rows(s, e, u, d, 20)[0] == 1000
            assert c.shard_info()["rows_global"] == 1008
    finally:
        plain.close()
        for c in ctxs:
            c.close()
