"""A live sharded table through the C-ABI communicator (pie_comm_append_rows / pie_comm_set_end / pie_comm_delete_user), in a
fresh process whose "RCCL" is tests/stub_rccl.c (PIE_RCCL_LIB): several shards of one table on GPU 0.  The model is the
UNSHARDED table of the oracle's generator, mutated in numpy.
usage: comm_mutate_worker.py CASE
  worlds   worlds 1, 2, 3, 5 (one with a rank that starts without a user): appends with new users, touches, a delete; then the
           merged expired and archive queues equal the oracle's queues of the mutated table, sources included, and every
           gathered feed of a batch with u_pad = 0 equals the oracle's
  errors   refusal while a pipelined step is uncollected; a refused call changes no shard"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
CASE = sys.argv[1]
stub_dir = os.path.join(REPO, "tests", "_stub")
os.makedirs(stub_dir, exist_ok=True)
stub = os.path.join(stub_dir, "libstub_rccl.so")
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                "-L/opt/rocm/lib", "-lamdhip64"], check=True)
os.environ["PIE_RCCL_LIB"] = stub

import numpy as np
import torch  # noqa: F401  (before libpie_hip.so initialises HIP)
import oracle_py
import sph_pie_amd as pie
from sph_pie_amd.binding import PieError

T0, SPAN, TTL, SEED, D, W = oracle_py.T0_MS, oracle_py.SPAN_MS, oracle_py.TTL_MS, 0x5EED5EED, 32, 43200000
TOP = T0 + SPAN
INT64_MIN = -(2 ** 63)
PIE_E_INVAL, PIE_E_STATE = -1, -6


class Live:
    """A communicator over one synthetic table and the host columns of the unsharded table, kept in step."""

    def __init__(self, world, n, U):
        self.world, self.U = world, U
        self.comm = pie.PieComm([0] * world)
        self.comm.gen_synthetic_sharded(SEED, n, U, D, 0)
        self.s, self.e, self.u, self.d = (a.copy() for a in oracle_py.gen(SEED, n, 0, n, U, D, 0))
        self.rng = np.random.default_rng(world)
        self.t = 0

    @property
    def N(self):
        return self.s.shape[0]

    def append(self, k, new_users):
        rng = self.rng
        self.t += 1
        n_users = self.U + new_users
        s = (TOP + self.t * 100000 + np.arange(k)).astype(np.int64)
        e = s + rng.integers(TTL // 4, TTL, k)
        u = rng.integers(0, n_users, k).astype(np.int32)
        u[:new_users] = np.arange(self.U, n_users)
        d = rng.integers(0, D, k).astype(np.int32)
        assert self.comm.append_rows(s, e, u, d, n_users) == self.N
        self.s, self.e = np.concatenate([self.s, s]), np.concatenate([self.e, e])
        self.u, self.d = np.concatenate([self.u, u]), np.concatenate([self.d, d])
        self.U = n_users
        assert self.comm.table_size() == (self.N, self.U)

    def touch(self, k, recent):
        rng = self.rng
        rows = rng.integers(0, self.N, k).astype(np.int32)
        rows[:recent] = np.arange(self.N - recent, self.N)
        rows[k - 1] = rows[0]  # a repeat: the last value wins
        vals = (TOP + rng.integers(-TTL, TTL, k)).astype(np.int64)
        vals[rng.random(k) < 0.2] = INT64_MIN
        self.comm.set_end(rows, vals)
        for r, v in zip(rows.tolist(), vals.tolist()):
            self.e[r] = v

    def delete(self, user):
        want = np.nonzero((self.u == user) & (self.e != INT64_MIN))[0] if 0 <= user < self.U else np.zeros(0, np.int64)
        rows, owner = self.comm.delete_user(user)
        assert owner == (pie.shard_of(user, self.world) if 0 <= user < self.U else -1)
        assert np.array_equal(rows, want), (user, rows.size, want.size)
        self.e[want] = INT64_MIN

    def maps(self):
        out = []
        for r in range(self.world):
            c = self.comm.ctx(r)
            rows_g, users_g = c.shard_maps()
            out.append((rows_g.astype(np.int64), users_g[: c.n_users].astype(np.int64) if users_g[0] >= 0 else np.zeros(0, np.int64)))
        return out

    def check_columns(self):
        maps = self.maps()
        assert sum(m[0].size for m in maps) == self.N
        for r in range(self.world):
            rows_g, users_g = maps[r]
            s, e, u, d = self.comm.ctx(r).read_columns()
            assert np.array_equal(s, self.s[rows_g]) and np.array_equal(e, self.e[rows_g]) and np.array_equal(d, self.d[rows_g]), r
            assert np.array_equal(users_g[u] if rows_g.size else u, self.u[rows_g]), r
        return maps

    def check_queues(self):
        maps = self.maps()
        checks = 0
        for prev, now in ((INT64_MIN, 2 ** 62), (TOP - TTL, TOP), (TOP, TOP + TTL), (TOP - 5, TOP - 5)):
            want = oracle_py.expired_queue(self.e, prev, now)
            rows, src_rank, src_row = self.comm.expired_queue(prev, now, sources=True)
            assert np.array_equal(rows, want), (self.world, prev, now, rows.size, want.size)
            self.check_sources(maps, rows, src_rank, src_row)
            checks += 1
        for now in (TOP - 100 * 86400000, TOP - SPAN // 2, TOP + TTL):
            want = oracle_py.archive_queue(self.s, self.e, self.u, self.U, now, W)
            rows, src_rank, src_row = self.comm.archive_queue(now, W, sources=True)
            assert np.array_equal(rows, want), (self.world, now, rows.size, want.size)
            self.check_sources(maps, rows, src_rank, src_row)
            checks += 1
        return checks

    def check_sources(self, maps, rows, src_rank, src_row):
        owner = np.array([pie.shard_of(int(g), self.world) for g in range(self.U)], np.int32)
        assert np.array_equal(src_rank, owner[self.u[rows]])
        for r in range(self.world):
            sel = src_rank == r
            assert np.array_equal(maps[r][0][src_row[sel]], rows[sel])

    def check_gather(self):
        maps = self.maps()
        for r in range(self.world):
            self.comm.ctx(r).set_disciplines(0xFFFFFFFF, D)
        qs = [(TOP - TTL // 3 - 977 * q, TOP - (2 + q % 2) * TTL, (0x55555555, 0xAAAAAAAA, 0xFFFFFFFF)[q % 3]) for q in range(5)]
        want = [oracle_py.scan(self.s, self.e, self.u, self.d, self.U, *q) for q in qs]
        ms = self.comm.scan_batch_gather(qs)  # u_pad = 0: the largest shard's user count, which the appends may have raised
        for at in range(self.world):
            for q in range(len(qs)):
                _, wo, wi = want[q]
                total = 0
                for r in range(self.world):
                    off, idx = self.comm.read_gathered(at, r, q)
                    assert ms[r][q] == idx.size
                    total += idx.size
                    rows_r, users_r = maps[r]
                    for lu in range(users_r.size):
                        gu = int(users_r[lu])
                        assert np.array_equal(rows_r[idx[off[lu]:off[lu + 1]]], wi[wo[gu]:wo[gu + 1]]), (at, q, r, gu)
                assert total == wi.size
        return len(qs)


def case_worlds():
    checks = 0
    for world, n, U in [(1, 20000, 300), (2, 20000, 300), (3, 20000, 300), (5, 20000, 7)]:
        t = Live(world, n, U)
        t.append(65, 3)
        t.touch(257, 65)
        t.append(1, 0)
        t.append(4096, 37)
        t.touch(3000, 500)
        t.delete(int(t.u[n // 3]))
        t.delete(t.U - 1)
        t.delete(t.U)
        t.delete(-1)
        t.check_columns()
        checks += t.check_queues()
        checks += t.check_gather()
        t.append(40000, 1)  # outgrows every shard's capacity
        t.touch(3000, 3000)
        t.check_columns()
        checks += t.check_queues()
        checks += t.check_gather()
        t.comm.close()
    print("worlds ok: %d checks" % checks)


def case_errors():
    t = Live(3, 20000, 300)
    t.append(100, 2)
    before = t.check_columns()
    size = t.comm.table_size()
    s = np.array([TOP, TOP + 1], np.int64)
    u = np.array([0, 1], np.int32)

    def refused(code, fn):
        try:
            fn()
            raise AssertionError("the call went through")
        except PieError as e:
            assert e.code == code, e
        assert t.comm.table_size() == size
        after = t.check_columns()
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(before, after))

    # a pipelined step begun and not collected
    for r in range(3):
        t.comm.ctx(r).set_disciplines(0xFFFFFFFF, D)
    t.comm.step_reserve(1, 0, 1 << 16)
    t.comm.step_begin([(TOP - TTL // 3, TOP - 3 * TTL, 0x55555555)])
    try:
        t.comm.append_rows(s, s + TTL, u, u, t.U)
        raise AssertionError("append while a step is in flight")
    except PieError as e:
        assert e.code == PIE_E_STATE
    for fn in (lambda: t.comm.set_end(u, s), lambda: t.comm.delete_user(0)):
        try:
            fn()
            raise AssertionError("mutation while a step is in flight")
        except PieError as e:
            assert e.code == PIE_E_STATE
    t.comm.step_finish()
    for fn in (lambda: t.comm.append_rows(s, s + TTL, u, u, t.U), lambda: t.comm.set_end(u, s), lambda: t.comm.delete_user(0)):
        try:
            fn()
            raise AssertionError("mutation while a step is finished and not collected")
        except PieError as e:
            assert e.code == PIE_E_STATE
    t.comm.step_collect()
    # ... and a WIDE step begun and not collected
    t.comm.wide_step_reserve(70, 0, 1 << 16)
    t.comm.wide_step_begin([(TOP - TTL // 3 - q, TOP - 3 * TTL, 0x55555555) for q in range(70)])
    for fn in (lambda: t.comm.append_rows(s, s + TTL, u, u, t.U), lambda: t.comm.set_end(u, s), lambda: t.comm.delete_user(0)):
        try:
            fn()
            raise AssertionError("mutation while a wide step is in flight")
        except PieError as e:
            assert e.code == PIE_E_STATE and "wide" in str(e), e
    t.comm.wide_step_finish()
    try:
        t.comm.wide_step_collect()
    except PieError as e:  # the first wide batch on a table may keep no union (Mu = -1): collected all the same
        assert e.code == -5, e
    assert t.comm.table_size() == size
    refused(PIE_E_INVAL, lambda: t.comm.append_rows(s, s + TTL, u, u, t.U - 1))
    refused(PIE_E_INVAL, lambda: t.comm.append_rows(s, s + TTL, np.array([0, t.U + 3], np.int32), u, t.U + 3))
    refused(PIE_E_INVAL, lambda: t.comm.set_end(np.array([0, t.N], np.int32), s))
    refused(PIE_E_INVAL, lambda: t.comm.set_end(np.array([-1, 0], np.int32), s))
    # one shard holds a row its map does not cover: the whole call is refused and the others stay as they were
    c1 = t.comm.ctx(1)
    c1.append_rows(s[:1], s[:1] + TTL, np.array([0], np.int32), np.array([1], np.int32), c1.n_users)
    cols = [t.comm.ctx(r).read_columns() for r in (0, 2)]
    for fn in (lambda: t.comm.append_rows(s, s + TTL, u, u, t.U), lambda: t.comm.set_end(u, s)):
        try:
            fn()
            raise AssertionError("the uncovered row went unnoticed")
        except PieError as e:
            assert e.code == PIE_E_STATE and "rank 1" in str(e), e
    # a delete touches the owning shard only: the shard with the uncovered row refuses its own users, the others work on
    mine = [g for g in range(t.U) if pie.shard_of(g, 3) == 1]
    try:
        t.comm.delete_user(mine[0])
        raise AssertionError("the uncovered row went unnoticed")
    except PieError as e:
        assert e.code == PIE_E_STATE and "rank 1" in str(e), e
    assert t.comm.table_size() == size
    for r, want in zip((0, 2), cols):
        assert all(np.array_equal(a, b) for a, b in zip(t.comm.ctx(r).read_columns(), want))
    t.comm.close()
    print("errors ok")


if __name__ == "__main__":
    {"worlds": case_worlds, "errors": case_errors}[CASE]()
