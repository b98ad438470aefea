"""The token column behind the C-ABI communicator (pie_comm_token_set / _append / _lookup / _set_end), in a fresh process whose
"RCCL" is tests/stub_rccl.c (PIE_RCCL_LIB): several shards of one table on GPU 0.  The model is the UNSHARDED TokenModel of
tests/token_model.py: the communicator's answers must equal it element for element.
usage: comm_token_worker.py CASE
  worlds   worlds 1, 2, 3, 5: token_set, append_rows + token_append, token_lookup (owner included), cross-shard duplicates,
           token_set_end with repeats and expired tokens; the merged expired queues and gathered feeds equal the oracle afterwards
  errors   refusal while a pipelined step is uncollected; a call one shard refuses changes no shard"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
CASE = sys.argv[1]
stub_dir = os.path.join(REPO, "tests", "_stub")
os.makedirs(stub_dir, exist_ok=True)
stub = os.path.join(stub_dir, "libstub_rccl_token.so")
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                "-L/opt/rocm/lib", "-lamdhip64"], check=True)
os.environ["PIE_RCCL_LIB"] = stub

import numpy as np
import torch  # noqa: F401  (before libpie_hip.so initialises HIP)
import oracle_py
import sph_pie_amd as pie
from sph_pie_amd.binding import PieError
from token_model import END_NONE, TokenModel

T0, SPAN, TTL, SEED, D = oracle_py.T0_MS, oracle_py.SPAN_MS, oracle_py.TTL_MS, 0x5EED5EED, 32
TOP = T0 + SPAN
PIE_E_INVAL, PIE_E_STATE = -1, -6


def random_keys(seed, n):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (n, 2), dtype=np.uint64)


class Live:
    """A communicator over one synthetic table and the unsharded TokenModel, kept in step."""

    def __init__(self, world, n, U):
        self.world, self.U = world, U
        self.comm = pie.PieComm([0] * world)
        self.comm.gen_synthetic_sharded(SEED, n, U, D, 0)
        self.tm = TokenModel(*oracle_py.gen(SEED, n, 0, n, U, D, 0))
        self.rng = np.random.default_rng(world)
        self.t = 0

    @property
    def N(self):
        return self.tm.start.shape[0]

    def owner_of_rows(self, rows):
        return np.array([pie.shard_of(int(u), self.world) for u in self.tm.user[rows]], np.int32)

    def append(self, k, new_users, keys):
        rng = self.rng
        self.t += 1
        n_users = self.U + new_users
        s = (TOP + self.t * 100000 + np.arange(k)).astype(np.int64)
        e = s + rng.integers(TTL // 4, TTL, k)
        u = rng.integers(0, n_users, k).astype(np.int32)
        u[:new_users] = np.arange(self.U, n_users)
        d = rng.integers(0, D, k).astype(np.int32)
        assert self.comm.append_rows(s, e, u, d, n_users) == self.N
        self.comm.token_append(keys)                       # no wait in between
        self.tm.append_rows(s, e, u, d)
        self.tm.token_append(keys)
        self.U = n_users

    def check_lookup(self, keys, now):
        got, want = self.comm.token_lookup(keys, now), self.tm.lookup(keys, now)
        assert np.array_equal(got["row"], want["row"]), "row"
        assert np.array_equal(got["live"], want["live"]), "live"
        f = want["found"]
        for col in ("user", "start", "end"):
            assert np.array_equal(got[col][f], want[col][f]), col
        assert np.array_equal(got["owner"][f], self.owner_of_rows(want["row"][f])) and np.all(got["owner"][~f] == -1), "owner"
        return got

    def check_columns(self):
        total = 0
        for r in range(self.world):
            c = self.comm.ctx(r)
            rows_g, users_g = c.shard_maps()
            s, e, u, d = c.read_columns()
            total += rows_g.size
            assert np.array_equal(s, self.tm.start[rows_g]) and np.array_equal(e, self.tm.end[rows_g]), r
            assert np.array_equal(users_g[u] if rows_g.size else u, self.tm.user[rows_g]), r
        assert total == self.N

    def check_queues_and_feeds(self):
        tm = self.tm
        checks = 0
        for prev, now in ((END_NONE, 2 ** 62), (TOP - TTL, TOP), (TOP, TOP + TTL)):
            assert np.array_equal(self.comm.expired_queue(prev, now), oracle_py.expired_queue(tm.end, prev, now)), (prev, now)
            checks += 1
        maps = []
        for r in range(self.world):
            c = self.comm.ctx(r)
            c.set_disciplines(0xFFFFFFFF, D)
            rows_g, users_g = c.shard_maps()
            maps.append((rows_g, users_g[: c.n_users] if users_g[0] >= 0 else np.zeros(0, np.int32)))
        qs = [(TOP - TTL // 3 - 977 * q, TOP - (2 + q % 2) * TTL, (0x55555555, 0xAAAAAAAA, 0xFFFFFFFF)[q % 3]) for q in range(3)]
        want = [oracle_py.scan(tm.start, tm.end, tm.user, tm.disc, self.U, *q) for q in qs]
        self.comm.scan_batch_gather(qs)
        for q in range(len(qs)):
            _, wo, wi = want[q]
            total = 0
            for r in range(self.world):
                off, idx = self.comm.read_gathered(0, r, q)
                total += idx.size
                rows_r, users_r = maps[r]
                for lu in range(users_r.size):
                    gu = int(users_r[lu])
                    assert np.array_equal(rows_r[idx[off[lu]:off[lu + 1]]], wi[wo[gu]:wo[gu + 1]]), (q, r, gu)
            assert total == wi.size
            checks += 1
        return checks


def case_worlds():
    checks = 0
    for world, n, U in [(1, 20000, 300), (2, 20000, 300), (3, 20000, 300), (5, 20000, 7)]:
        t = Live(world, n, U)
        rng = t.rng
        keys = random_keys(10 + world, n + 65 + 4096)
        # planted duplicates: one key on rows of users of different shards (where there are several), and on two rows of one user
        owner = t.owner_of_rows(np.arange(n))
        pairs, used = [], set(range(100, 140))
        for a in range(100, 140):
            other = np.nonzero((owner != owner[a]) & (np.arange(n) > a))[0] if world > 1 else np.arange(a + 1, n)
            b = next(int(x) for x in other[a:] if int(x) not in used)   # no row takes part in two pairs
            used.add(b)
            keys[b] = keys[a]
            pairs.append((a, b))
        t.comm.token_set(keys[: n - 50])
        t.tm.token_set(keys[: n - 50])
        now = int(np.median(t.tm.end))
        ask = np.concatenate([keys[:n], random_keys(3, 500)])
        got = t.check_lookup(ask, now)
        t.check_lookup(ask[::7], END_NONE)
        assert all(got["row"][a] == b and got["row"][b] == b for a, b in pairs), "of two rows under one key the largest global row answers, across shards"
        assert np.all(got["row"][n - 50: n] == -1)
        t.comm.token_append(keys[n - 50: n])
        t.tm.token_append(keys[n - 50: n])
        t.append(65, 3, keys[n: n + 65])
        t.append(4096, 37, keys[n + 65:])
        t.check_lookup(np.concatenate([keys, random_keys(4, 100)]), now)
        assert t.comm.token_lookup(np.zeros((0, 2), np.uint64), now)["row"].shape == (0,)
        for r in range(world):
            assert t.comm.ctx(r).shard_token_layout()[0] == t.N
        # touches and deletes by token: repeats, expired and unknown tokens, duplicates
        live, dead = np.nonzero(t.tm.end > now)[0], np.nonzero(t.tm.end <= now)[0]
        rows = np.concatenate([live[:800], dead[:300], [live[3], live[3], live[5]], [a for a, _ in pairs]])
        ask = np.concatenate([keys[rows], random_keys(5, 30)])
        ask = ask[rng.permutation(ask.shape[0])]
        new_end = (TOP + rng.integers(-TTL, TTL, ask.shape[0])).astype(np.int64)
        new_end[::7] = END_NONE
        got_rows = t.comm.token_set_end(ask, new_end, now)
        assert np.array_equal(got_rows, t.tm.token_set_end(ask, new_end, now))
        assert np.count_nonzero(got_rows == live[3]) == 3 and np.count_nonzero(got_rows >= 0) > 700
        t.check_columns()
        both = keys[np.concatenate([dead[300:330], np.nonzero(t.tm.end == END_NONE)[0][:5]])]
        vals = np.full(35, TOP + 5, np.int64)
        got_rows = t.comm.token_set_end(both, vals, END_NONE)
        assert np.array_equal(got_rows, t.tm.token_set_end(both, vals, END_NONE)) and np.all(got_rows[30:] == -1)
        assert t.comm.token_set_end(np.zeros((0, 2), np.uint64), [], now).shape == (0,)
        t.check_columns()
        t.check_lookup(keys[::5], now)
        checks += t.check_queues_and_feeds()
        t.comm.close()
    print("worlds ok: %d checks" % checks)


def case_errors():
    t = Live(3, 20000, 300)
    n = t.N
    keys = random_keys(1, n + 10)
    t.comm.token_set(keys[: n - 10])
    t.tm.token_set(keys[: n - 10])

    def state():
        return [(t.comm.ctx(r).shard_token_layout()[0], t.comm.ctx(r).table_info()["token_builds"]) for r in range(3)]

    before = state()
    assert [s[0] for s in before] == [n - 10] * 3
    s = np.zeros(2, np.int64)

    def refused(code, fn, text=None):
        try:
            fn()
            raise AssertionError("the call went through")
        except PieError as e:
            assert e.code == code and (text is None or text in str(e)), e

    calls = (lambda: t.comm.token_set(keys[:5]), lambda: t.comm.token_append(keys[n - 10: n - 8]), lambda: t.comm.token_lookup(keys[:2], TOP),
             lambda: t.comm.token_set_end(keys[:2], s, TOP))
    # a pipelined step begun and not collected, then finished and not collected
    for r in range(3):
        t.comm.ctx(r).set_disciplines(0xFFFFFFFF, D)
    t.comm.step_reserve(1, 0, 1 << 16)
    t.comm.step_begin([(TOP - TTL // 3, TOP - 3 * TTL, 0x55555555)])
    for fn in calls:
        refused(PIE_E_STATE, fn)
    t.comm.step_finish()
    for fn in calls:
        refused(PIE_E_STATE, fn)
    t.comm.step_collect()
    assert state() == before
    # past the table's end, on every shard alike
    refused(PIE_E_INVAL, lambda: t.comm.token_append(keys[: 11]))
    refused(PIE_E_INVAL, lambda: t.comm.token_set(random_keys(2, n + 1)))
    assert state() == before
    t.check_lookup(keys[:500], TOP)
    # one shard holds a row its map does not cover: the whole call is refused and no shard changes
    c1 = t.comm.ctx(1)
    c1.append_rows([TOP], [TOP + TTL], [0], [1], c1.n_users)
    for fn in calls:
        refused(PIE_E_STATE, fn, "rank 1")
    for r in (0, 2):
        c = t.comm.ctx(r)
        assert (c.shard_token_layout()[0], c.table_info()["token_builds"]) == before[r]
        got = c.shard_token_lookup(keys[:200], TOP)
        assert np.count_nonzero(got["row"] >= 0) > 0
    t.comm.close()
    print("errors ok")


if __name__ == "__main__":
    {"worlds": case_worlds, "errors": case_errors}[CASE]()
