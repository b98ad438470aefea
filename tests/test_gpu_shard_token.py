"""GPU, context level, no communicator: the token column of `world` sharded contexts of one GPU (pie_shard_token_*, the kernels
k_shard_token_place / k_shard_token_lookup of sph-pie_amd/csrc/pie_token.h) against tests/shard_token_model.py: the unsharded
TokenModel, the owner of every user and, per rank, the rows its compactions dropped.  Shapes as tests/test_gpu_shard_mutate.py:
20 000 rows / 300 users, world 5 with 7 users so that one rank holds no user and no row."""
import numpy as np
import pytest

from shard_token_model import ShardTokenModel
from token_model import END_NONE, check_layout

pytestmark = pytest.mark.gpu

SEED, D = 20260, 32
SHAPES = {1: (20000, 300), 2: (20000, 300), 3: (20000, 300), 5: (20000, 7)}
PIE_E_INVAL, PIE_E_STATE = -1, -6
WORLDS = (1, 2, 3, 5)


def random_keys(seed, n):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (n, 2), dtype=np.uint64)


class Shards:
    """`world` sharded contexts on GPU 0 and the model, kept in step."""

    def __init__(self, pie, oracle, world, n0=None, u0=None, ordered=None):
        n0, u0 = (n0, u0) if n0 else SHAPES[world]
        self.pie, self.oracle, self.world = pie, oracle, world
        self.ctxs = []
        for r in range(world):
            c = pie.PieScan(0)
            self.ctxs.append(c)
            if ordered is not None:
                c.set_ordered_run(ordered)
            c.gen_synthetic(SEED, n0, 0, n0, u0, D, 0)
            c.shard_table(r, world)
        cols = oracle.gen(SEED, n0, 0, n0, u0, D, 0)
        self.U = u0
        self.m = ShardTokenModel(*cols, [oracle.shard_of(u, world) for u in range(u0)], world)
        self.top = oracle.T0_MS + oracle.SPAN_MS
        self.t = 0

    def close(self):
        for c in self.ctxs:
            c.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def token_set(self, keys):
        for c in self.ctxs:
            c.shard_token_set(keys)
        self.m.token_set(keys)

    def token_append(self, keys):
        for c in self.ctxs:
            c.shard_token_append(keys)
        self.m.token_append(keys)

    def new_rows(self, k, new_users, rng):
        o = self.oracle
        self.t += 1
        n_users = self.U + new_users
        s = (self.top + self.t * 100000 + np.arange(k)).astype(np.int64)
        e = s + rng.integers(o.TTL_MS // 4, o.TTL_MS, k)
        u = rng.integers(0, n_users, k).astype(np.int32)
        u[: min(new_users, k)] = np.arange(self.U, self.U + min(new_users, k))
        return s, e, u, rng.integers(0, D, k).astype(np.int32), n_users

    def append_rows(self, k, new_users, rng):
        s, e, u, d, n_users = self.new_rows(k, new_users, rng)
        for c in self.ctxs:
            assert c.shard_append_rows(s, e, u, d, n_users)[0] == self.m.N
        self.m.append_rows(s, e, u, d, [self.oracle.shard_of(g, self.world) for g in range(self.U, n_users)])
        self.U = n_users
        return s, e, u, d

    def check_lookup(self, keys, nows):
        for r, c in enumerate(self.ctxs):
            for now in nows:
                got, want = c.shard_token_lookup(keys, now), self.m.shard_lookup(r, keys, now)
                assert np.array_equal(got["row"], want["row"]), "rank %d: global row" % r
                assert np.array_equal(got["live"], want["live"]), "rank %d: live" % r
                f = want["found"]
                for col in ("user", "start", "end"):
                    assert np.array_equal(got[col][f], want[col][f]), "rank %d: %s" % (r, col)

    def check_layout(self):
        pie = self.pie
        for r, c in enumerate(self.ctxs):
            cg, cl, slots, slot_row, keys = c.shard_token_layout()
            assert cg == self.m.covered_g and cl == self.m.covered_l(r), "rank %d: coverage" % r
            assert slots >= pie.token_slots_for(c.n) and slots & (slots - 1) == 0
            check_layout(cl, slots, slot_row, keys, pie.token_homes(keys, slots.bit_length() - 1))
            assert np.array_equal(keys, self.m.shard_keys(r)), "rank %d: the keys of its covered rows, in local order" % r
            assert c.table_info()["token_rows"] == cl

    def check_columns(self):
        tm = self.m.tm
        for r, c in enumerate(self.ctxs):
            rows = self.m.held(r)
            got_rows, got_users = c.shard_maps()
            assert np.array_equal(got_rows, rows), "rank %d: row map" % r
            s, e, u, d = c.read_columns()
            assert np.array_equal(s, tm.start[rows]) and np.array_equal(e, tm.end[rows]) and np.array_equal(d, tm.disc[rows]), "rank %d" % r
            assert np.array_equal(got_users[u] if rows.size else u, tm.user[rows]), "rank %d: user" % r


@pytest.mark.parametrize("world", WORLDS)
def test_set_lookup_layout(pie, oracle, world):
    with Shards(pie, oracle, world) as t:
        N = t.m.N
        keys = random_keys(1, N)
        t.token_set(keys)
        ask = np.concatenate([keys, random_keys(2, 500)])
        t.check_lookup(ask, (t.top - oracle.TTL_MS // 3, t.top - 20 * oracle.TTL_MS))
        t.check_layout()
        found = np.zeros(N, int)
        for r, c in enumerate(t.ctxs):
            got = c.shard_token_lookup(ask, t.top)
            assert np.all(got["row"][N:] == -1) and not got["live"][N:].any()
            found += got["row"][:N] >= 0
            assert c.shard_token_lookup(np.zeros((0, 2), np.uint64), t.top)["row"].shape == (0,)
            info = c.table_info()
            assert info["token_builds"] >= 1 and info["token_bytes"] >= 16 * c.n
        assert np.all(found == 1), "every key is held by exactly one shard"
        if world == 5:
            empty = [r for r in range(world) if t.m.held(r).size == 0]
            assert empty
            for r in empty:
                got = t.ctxs[r].shard_token_lookup(ask, t.top)
                assert np.all(got["row"] == -1) and not got["live"].any()
                assert t.ctxs[r].shard_token_layout()[:3] == (N, 0, 1024)


@pytest.mark.parametrize("world", WORLDS)
def test_partial_coverage(pie, oracle, world):
    with Shards(pie, oracle, world) as t:
        N = t.m.N
        keys = random_keys(3, N)
        now = (t.top - oracle.TTL_MS // 3,)
        t.token_set(keys[: N - 100])
        t.check_lookup(keys, now)
        t.check_layout()
        at = N - 100
        for k in (1, 37, 62):
            t.token_append(keys[at: at + k])
            at += k
            t.check_lookup(keys, now)
        assert at == N
        t.check_layout()
        for c in t.ctxs:                                  # past N_g: refused, nothing changes
            with pytest.raises(pie.PieError) as ei:
                c.shard_token_append(random_keys(4, 1))
            assert ei.value.code == PIE_E_INVAL
            with pytest.raises(pie.PieError) as ei:
                c.shard_token_set(random_keys(4, N + 1))
            assert ei.value.code == PIE_E_INVAL
        t.check_layout()
        t.check_lookup(keys, now)
        t.token_set(keys[:5])                             # a set replaces the column
        t.check_lookup(keys[:300], now)
        t.check_layout()


@pytest.mark.parametrize("world", WORLDS)
def test_chained_without_a_host_wait(pie, oracle, world):
    with Shards(pie, oracle, world) as t:
        N = t.m.N
        rng = np.random.default_rng(50 + world)
        keys = random_keys(5, N + 113)
        t.token_set(keys[:N])
        sizes = [(c.n, c.n_users) for c in t.ctxs]
        s, e, u, d, n_users = t.new_rows(113, 9, rng)
        owner_new = [oracle.shard_of(g, world) for g in range(t.U, n_users)]
        owner = np.concatenate([t.m.owner, np.array(owner_new, np.int32)])
        got = []
        for r, c in enumerate(t.ctxs):                    # append, keys, lookup: back to back on every shard
            kept = int((owner[u] == r).sum())
            users = int((owner == r).sum())
            c.shard_append_rows(s, e, u, d, n_users, local_size=(sizes[r][0] + kept, max(users, 1)))
            c.shard_token_append(keys[N:])
            got.append(c.shard_token_lookup(keys[N:], t.top))
        t.m.append_rows(s, e, u, d, owner_new)
        t.m.token_append(keys[N:])
        t.U = n_users
        for r in range(world):
            want = t.m.shard_lookup(r, keys[N:], t.top)
            mine = owner[u] == r
            assert np.array_equal(got[r]["row"], np.where(mine, np.arange(N, N + 113), -1)), "exactly the owning shard finds a key"
            assert np.array_equal(got[r]["row"], want["row"]) and np.array_equal(got[r]["live"], want["live"])
            assert np.array_equal(got[r]["user"][mine], u[mine]) and np.array_equal(got[r]["end"][mine], e[mine])
            assert np.array_equal(got[r]["start"][mine], s[mine])
        t.check_layout()
        t.check_columns()


def test_growth(pie, oracle):
    world, u0 = 2, 40
    owner = np.array([oracle.shard_of(g, world) for g in range(u0)])
    # the largest of these tables whose shards both start at 1024 slots (at most 512 rows each)
    n0 = next(n for n in (900, 800, 700, 600) if np.bincount(owner[oracle.gen(SEED, n, 0, n, u0, D, 0)[2]], minlength=2).max() <= 512)
    with Shards(pie, oracle, world, n0, u0) as t:
        rng = np.random.default_rng(6)
        keys = random_keys(7, n0)
        t.token_set(keys)
        assert [c.shard_token_layout()[2] for c in t.ctxs] == [1024, 1024] and all(c.n <= 512 for c in t.ctxs)
        all_keys = keys
        builds = [c.table_info()["token_builds"] for c in t.ctxs]
        # rows of rank 0's users only, until rank 0 holds more than 512 rows; rank 1 never passes half its slots
        mine = [g for g in range(t.U) if t.m.owner[g] == 0]
        grew = False
        for step in range(8):
            k = 120
            s, e, _, d, n_users = t.new_rows(k, 0, rng)
            u = rng.choice(mine, k).astype(np.int32)
            for c in t.ctxs:
                c.shard_append_rows(s, e, u, d, n_users)
            t.m.append_rows(s, e, u, d)
            more = random_keys(100 + step, k)
            passed = t.ctxs[0].n > 512 and not grew
            t.token_append(more)
            all_keys = np.concatenate([all_keys, more])
            now_builds = [c.table_info()["token_builds"] for c in t.ctxs]
            if passed:
                assert now_builds == [builds[0] + 1, builds[1]], "the rebuild, on the shard that grew only"
                assert [c.shard_token_layout()[2] for c in t.ctxs] == [2048, 1024]
                grew, builds = True, now_builds
            else:
                assert now_builds == builds
            if t.ctxs[0].n > 700:
                break
        assert grew and t.ctxs[1].n <= 512
        t.check_lookup(all_keys, (t.top,))
        t.check_layout()
        got = t.ctxs[0].shard_token_lookup(all_keys, t.top)["row"]
        assert np.array_equal(np.nonzero(got >= 0)[0], t.m.held(0)), "every earlier key is still found"


@pytest.mark.parametrize("world", (2, 3))
def test_duplicates(pie, oracle, world):
    with Shards(pie, oracle, world) as t:
        N = t.m.N
        user, owner = t.m.tm.user, t.m.owner
        keys = random_keys(8, N)
        # one key on two rows of one user: the larger global row answers
        u0 = int(user[100])
        rows_u0 = np.nonzero(user == u0)[0]
        a, b = int(rows_u0[1]), int(rows_u0[-1])
        keys[b] = keys[a]
        # one key on rows of users of two shards: each shard answers its own
        r0 = np.nonzero(owner[user] == 0)[0]
        r1 = np.nonzero(owner[user] == 1)[0]
        x, y = int(r0[50]), int(r1[60])
        keys[y] = keys[x]
        t.token_set(keys)
        ask = np.stack([keys[a], keys[x]])
        got0, got1 = t.ctxs[0].shard_token_lookup(ask, t.top), t.ctxs[1].shard_token_lookup(ask, t.top)
        ra = int(owner[u0])
        assert t.ctxs[ra].shard_token_lookup(ask, t.top)["row"][0] == b
        assert got0["row"][1] == x and got1["row"][1] == y and got0["user"][1] == user[x] and got1["user"][1] == user[y]
        t.check_lookup(keys, (t.top - oracle.TTL_MS // 3,))


@pytest.mark.parametrize("world,ordered", [(1, None), (2, None), (3, None), (5, None), (3, 2)])  # once with the ordered run in mode 2
def test_touch_and_delete_by_token(pie, oracle, world, ordered):
    with Shards(pie, oracle, world, ordered=ordered) as t:
        N, tm = t.m.N, t.m.tm
        rng = np.random.default_rng(9 + world)
        keys = random_keys(10, N)
        t.token_set(keys)
        now = int(np.median(tm.end))
        live, dead = np.nonzero(tm.end > now)[0], np.nonzero((tm.end <= now) & (tm.end != END_NONE))[0]
        assert live.size > 2000 and dead.size > 2000
        rows = np.concatenate([live[:600], dead[:200], [live[7], live[7], live[9]]])
        ask = np.concatenate([keys[rows], random_keys(11, 25)])
        ask = ask[rng.permutation(ask.shape[0])]
        new_end = (t.top + rng.integers(-oracle.TTL_MS, oracle.TTL_MS, ask.shape[0])).astype(np.int64)
        new_end[::7] = END_NONE                            # deletes among the touches
        got = [c.shard_token_set_end(ask, new_end, now) for c in t.ctxs]
        want = t.m.shard_set_end(ask, new_end, now)
        for r in range(world):
            assert np.array_equal(got[r], want[r]), "rank %d: rows_global_out" % r
        written = np.max(np.stack(got), axis=0)
        assert set(written[written >= 0]) == set(live[:600]), "live sessions only"
        assert np.count_nonzero(written == live[7]) == 3
        t.check_columns()
        # now = PIE_END_NONE: every found row that is not a tombstone
        tomb = np.nonzero(tm.end == END_NONE)[0]
        both = np.concatenate([keys[dead[200:230]], keys[tomb[:5]]])
        vals = np.full(35, t.top + 5, np.int64)
        got = [c.shard_token_set_end(both, vals, END_NONE) for c in t.ctxs]
        want = t.m.shard_set_end(both, vals, END_NONE)
        for r in range(world):
            assert np.array_equal(got[r], want[r])
        written = np.max(np.stack(got), axis=0)
        assert np.array_equal(written[:30], dead[200:230]) and np.all(written[30:] == -1)
        t.check_columns()
        t.check_lookup(keys[::3], (now, END_NONE))
        for c in t.ctxs:
            assert c.shard_token_set_end(np.zeros((0, 2), np.uint64), [], now).shape == (0,)
        # the derived keys, the hot index and the ordered run stayed in step: a scan and a 16-query batch against the oracle
        full = 2 ** 64 - 1
        q16 = [(int(t.top + rng.integers(-oracle.TTL_MS, oracle.TTL_MS // 2)), int(t.top - rng.integers(0, 4 * oracle.TTL_MS)),
                int(rng.integers(1, 2 ** 32)) | (1 << int(rng.integers(0, D)))) for _ in range(16)]
        s_now, s_cut = int(t.top - oracle.TTL_MS // 3), int(t.top - 3 * oracle.TTL_MS)
        for r, c in enumerate(t.ctxs):
            rows_r = t.m.held(r)
            users_r = np.nonzero(t.m.owner == r)[0]
            nu = max(users_r.size, 1)
            cols = (tm.start[rows_r], tm.end[rows_r], np.searchsorted(users_r, tm.user[rows_r]).astype(np.int32), tm.disc[rows_r])
            for a, b in zip(c.scan(s_now, s_cut), oracle.scan(*cols, nu, s_now, s_cut, full)):
                assert np.array_equal(a, b), "rank %d: scan" % r
            for q, res in zip(q16, c.scan_batch(q16)):
                for a, b in zip(res, oracle.scan(*cols, nu, *q)):
                    assert np.array_equal(a, b), "rank %d: batch" % r


def test_compaction(pie, oracle):
    world = 2
    with Shards(pie, oracle, world) as t:
        N, tm = t.m.N, t.m.tm
        rng = np.random.default_rng(12)
        keys = random_keys(13, N + 300)
        t.token_set(keys[: N - 100])                        # the last 100 rows have no key yet
        builds = [c.table_info()["token_builds"] for c in t.ctxs]
        # touches by token, then compact rank 0 only
        T = int(np.median(tm.end))
        ask = keys[rng.integers(0, N - 100, 3000)]
        vals = np.where(rng.random(3000) < 0.5, END_NONE, t.top + 77).astype(np.int64)
        got = [c.shard_token_set_end(ask, vals, END_NONE) for c in t.ctxs]
        want = t.m.shard_set_end(ask, vals, END_NONE)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        before = t.m.held(0)
        kept = t.ctxs[0].compact_rows(T)
        held = t.m.compact(0, T)
        assert kept == held.size < before.size
        t.check_columns()                                   # the row map holds the ORIGINAL global ids
        t.check_lookup(keys[:N], (t.top, END_NONE))
        t.check_layout()
        now_builds = [c.table_info()["token_builds"] for c in t.ctxs]
        assert now_builds == [builds[0] + 1, builds[1]]
        assert t.ctxs[0].compact_rows(T) == kept and t.ctxs[0].table_info()["token_builds"] == now_builds[0], \
            "a compaction that drops nothing leaves the index alone"
        t.check_lookup(keys[:N:5], (t.top,))
        gone = before[~np.isin(before, held)]
        got = t.ctxs[0].shard_token_lookup(keys[gone[gone < N - 100]], t.top)
        assert np.all(got["row"] == -1), "the keys of dropped rows are gone from the shard that dropped them"
        # the keys of the uncovered tail, then rows appended afterwards: both still land
        t.token_append(keys[N - 100: N])
        t.append_rows(300, 4, rng)
        t.token_append(keys[N:])
        t.check_lookup(keys, (t.top,))
        t.check_layout()
        t.check_columns()


def test_chunk_boundary(pie, oracle):
    world, U = 2, 1000
    N = 2 ** 20 + 777
    ctxs = []
    try:
        for r in range(world):
            c = pie.PieScan(0)
            ctxs.append(c)
            c.gen_synthetic(SEED, N, 0, N, U, D, 0)
            c.shard_table(r, world)
        s, e, u, _ = oracle.gen(SEED, N, 0, N, U, D, 0)
        owner = np.array([oracle.shard_of(g, world) for g in range(U)], np.int32)
        keys = random_keys(14, N)                          # 128 random bits per row: no two rows share a key
        rng = np.random.default_rng(15)
        rows = np.concatenate([rng.integers(0, N, 4096), np.arange(N - 777, N), [2 ** 20 - 1, 2 ** 20]])
        now = int(np.median(e))
        for r, c in enumerate(ctxs):
            c.shard_token_set(keys)                        # two chunks: 2^20 keys and 777
            cg, cl, slots = c.shard_token_layout()[:3]
            assert cg == N and cl == c.n == int((owner[u] == r).sum()) and slots >= pie.token_slots_for(c.n)
            got = c.shard_token_lookup(keys[rows], now)
            mine = owner[u[rows]] == r
            assert np.array_equal(got["row"], np.where(mine, rows, -1))
            assert np.array_equal(got["live"], (mine & (e[rows] > now)).astype(np.uint8))
            assert np.array_equal(got["user"][mine], u[rows][mine]) and np.array_equal(got["start"][mine], s[rows][mine])
            assert np.array_equal(got["end"][mine], e[rows][mine])
    finally:
        for c in ctxs:
            c.close()


def test_state_rules(pie, oracle):
    keys = random_keys(16, 20000)
    now = oracle.T0_MS

    def refused(fn, *a):
        with pytest.raises(pie.PieError) as ei:
            fn(*a)
        return ei.value.code == PIE_E_STATE

    def all_refused(c, with_set):
        ok = refused(c.shard_token_append, keys[:4]) and refused(c.shard_token_lookup, keys[:4], now)
        ok = ok and refused(c.shard_token_set_end, keys[:4], np.zeros(4, np.int64), now) and refused(c.shard_token_layout)
        return ok and (not with_set or refused(c.shard_token_set, keys[:4]))

    with pie.PieScan(0) as fresh:                          # no table
        assert all_refused(fresh, True)
    with pie.PieScan(0) as plain:                          # a context that is not sharded, with a plain column of its own
        plain.gen_synthetic(SEED, 1000, 0, 1000, 20, D, 0)
        assert all_refused(plain, True)
        plain.token_set(keys[:1000])
        assert all_refused(plain, True)
        assert plain.token_lookup(keys[:3], now)["row"].tolist() == [0, 1, 2]
    with Shards(pie, oracle, 2) as t:
        c = t.ctxs[0]
        N = t.m.N
        assert all_refused(c, False), "no column yet: all but the set"
        assert c.table_info()["token_rows"] == 0
        with pytest.raises(pie.PieError) as ei:            # pie_token_set stays refused on a sharded context
            c.token_set(keys[: c.n])
        assert ei.value.code == PIE_E_STATE
        t.token_set(keys[: N - 10])
        with pytest.raises(pie.PieError) as ei:
            c.token_set(keys[: c.n])
        assert ei.value.code == PIE_E_STATE
        assert refused(c.token_append, keys[:1]), "pie_token_append would break covered_g"
        # the plain calls run unchanged, in LOCAL ids
        held = t.m.held(0)
        covered_l = t.m.covered_l(0)
        got = c.token_lookup(keys[held[:50]], now)
        assert np.array_equal(got["row"], np.arange(50))
        cov, slots, slot_row, back = c.token_layout()
        assert cov == covered_l and np.array_equal(back, keys[held[:covered_l]])
        check_layout(cov, slots, slot_row, back, pie.token_homes(back, slots.bit_length() - 1))
        assert list(c.token_set_end(keys[held[:2]], [END_NONE, END_NONE], END_NONE)) == [0, 1]
        t.m.tm.end[held[:2]] = END_NONE
        t.check_columns()
        # NULL keys, k = 0
        lib = c._lib
        assert lib.pie_shard_token_lookup(c._ctx, None, 3, now, None, None, None, None, None) == PIE_E_INVAL
        assert lib.pie_shard_token_lookup(c._ctx, None, 0, now, None, None, None, None, None) == 0
        assert lib.pie_shard_token_append(c._ctx, None, 3) == PIE_E_INVAL and lib.pie_shard_token_append(c._ctx, None, 0) == 0
        assert lib.pie_shard_token_set_end(c._ctx, None, None, 3, now, None) == PIE_E_INVAL
        assert lib.pie_shard_token_set_end(c._ctx, None, None, 0, now, None) == 0
        assert lib.pie_shard_token_set(c._ctx, None, 3) == PIE_E_INVAL
        assert lib.pie_shard_token_lookup(c._ctx, keys.ctypes.data, 5, now, None, None, None, None, None) == 0, "every output may be NULL"
        assert c.shard_token_layout()[0] == N - 10
        # a scan, then a batch, in flight
        c.scan_begin(now, 0)
        assert all_refused(c, True)
        c.scan_finish()
        c.scan_batch_begin([(now, 0, 1), (now + 5, 0, 3)])
        assert all_refused(c, True)
        c.scan_batch_finish()
        t.check_lookup(keys[:500], (now,))
        # a row the map does not cover
        o = oracle
        c.append_rows([o.T0_MS], [o.T0_MS + 5], [0], [1], c.n_users)
        assert all_refused(c, True)
        # what renumbers or replaces the table drops the column
        c1 = t.ctxs[1]
        c1.shard_table(0, 2)
        assert all_refused(c1, False) and c1.table_info()["token_rows"] == 0
        c1.shard_token_set(keys[:5])
        c1.gen_synthetic(SEED, 1000, 0, 1000, 20, D, 0)
        assert all_refused(c1, True)
