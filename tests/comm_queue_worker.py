"""Cross-shard dispatch queues through the C-ABI communicator (pie_comm_expired_queue / pie_comm_archive_queue), in a fresh
process whose "RCCL" is tests/stub_rccl.c (PIE_RCCL_LIB): several shards of one table on GPU 0.  Every merged queue is checked
element for element against the oracle's queue of the UNSHARDED table.
usage: comm_queue_worker.py CASE
  worlds   worlds 1, 2, 3, 5 (one with a rank that holds no rows): expired windows (empty, inverted, most of the table, after
           touches and tombstones applied to the shards), archive windows (no group, some, all, now - window below int64),
           sources, every local rank's copy, the capacity error and its repeat
  errors   refusal while a pipelined step is uncollected; a shard with rows its map does not cover fails every rank alike
  edges    worlds 3 and 5 (a rank without rows), 20 000 rows: expired windows whose merged queue holds exactly 0, 1, 255, 256, 257
           and 4 097 rows, and one whose rows all sit on one shard; rows, sources, and the in-flight form on the same communicator
  cfg5     world 8, 10^8 rows, 10^5 users: one expired and one archive queue
  real     world 1 through the real RCCL (prints "skip: ..." when it does not load)"""
import ctypes as C
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
CASE = sys.argv[1]
if CASE != "real":
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
from sph_pie_amd.binding import PieError, _ptr

T0, DAY, SEED, W = oracle_py.T0_MS, 86400 * 1000, 0x5EED5EED, 43200000
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
PIE_E_CAPACITY, PIE_E_STATE = -5, -6


class Sharded:
    """A communicator over one synthetic table and the host columns of the unsharded table, kept in step."""

    def __init__(self, world, n, U, flags=1):
        self.world, self.n, self.U = world, n, U
        self.comm = pie.PieComm([0] * world)
        self.comm.gen_synthetic_sharded(SEED, n, U, 32, flags)
        self.ctxs = [self.comm.ctx(r) for r in range(world)]
        self.rows_g, self.users_g = [], []
        for r in range(world):
            rg, ug = self.ctxs[r].shard_maps()
            self.rows_g.append(rg.astype(np.int64))
            self.users_g.append(ug[: self.ctxs[r].n_users].astype(np.int64) if rg.size else np.zeros(0, np.int64))
        assert sum(m.size for m in self.rows_g) == n
        self.start, self.end, self.user, _ = oracle_py.gen(SEED, n, 0, n, U, 32, flags)
        self.end = self.end.copy()
        self.rank_of_row = np.empty(n, np.int32)
        self.local_of_row = np.empty(n, np.int32)
        for r in range(world):
            assert np.all(np.diff(self.rows_g[r]) > 0), "shard maps are ascending"
            self.rank_of_row[self.rows_g[r]] = r
            self.local_of_row[self.rows_g[r]] = np.arange(self.rows_g[r].size, dtype=np.int32)

    def set_end(self, rows, new_end):
        rows, new_end = np.asarray(rows, np.int64), np.asarray(new_end, np.int64)
        for r in range(self.world):
            sel = self.rank_of_row[rows] == r
            if sel.any():
                self.ctxs[r].set_end(self.local_of_row[rows[sel]], new_end[sel])
        self.end[rows] = new_end

    def delete_user(self, g):
        r = pie.shard_of(g, self.world)
        lu = int(np.searchsorted(self.users_g[r], g))
        assert self.users_g[r][lu] == g
        gone = self.rows_g[r][self.ctxs[r].delete_user(lu)]
        assert np.array_equal(gone, np.nonzero((self.user == g) & (self.end != INT64_MIN))[0])
        self.end[gone] = INT64_MIN

    def check_sources(self, rows, src_rank, src_row):
        assert np.array_equal(src_rank, self.rank_of_row[rows])
        for r in range(self.world):
            sel = src_rank == r
            assert np.array_equal(self.rows_g[r][src_row[sel]], rows[sel])

    def check_every_rank(self, rows):
        for at in range(self.world):
            assert np.array_equal(self.comm.queue_read(at), rows), at

    def expired(self, prev, now, full=True):
        want = oracle_py.expired_queue(self.end, prev, now)
        rows, src_rank, src_row = self.comm.expired_queue(prev, now, sources=True)
        assert np.array_equal(rows, want), (self.world, prev, now, rows.size, want.size)
        if full:
            self.check_sources(rows, src_rank, src_row)
            self.check_every_rank(rows)
            assert np.array_equal(self.comm.expired_queue(prev, now), want)
        return rows.size

    def archive(self, now, full=True, oracle_fn=oracle_py.archive_queue):
        want = oracle_fn(self.start, self.end, self.user, self.U, now, W)
        rows, src_rank, src_row = self.comm.archive_queue(now, W, sources=True)
        assert np.array_equal(rows, want), (self.world, now, rows.size, want.size)
        if full:
            self.check_sources(rows, src_rank, src_row)
            self.check_every_rank(rows)
        return rows.size


def raw_queue(comm, fn, a, b, cap):
    out = np.full(max(cap, 1), -7, np.int32)
    q = C.c_size_t(12345)
    rc = getattr(comm._lib, fn)(comm._c, int(a), int(b), _ptr(out), int(cap), C.byref(q))
    return rc, q.value, out[:cap]


def case_worlds():
    checks = 0
    for world, n, U in [(1, 200_003, 1000), (2, 400_000, 3001), (3, 1_000_000, 10_007), (5, 200_000, 7)]:
        t = Sharded(world, n, U)
        if U == 7:
            assert min(m.size for m in t.rows_g) == 0, "7 users over 5 ranks leave one rank without rows"
        k = int(t.end[n // 2])
        windows = [(k, k), (5, 4), (INT64_MIN, 2 ** 62), (T0 - 6 * 3600 * 1000 - 60000, T0 - 6 * 3600 * 1000), (k - 1000, k + 1000),
                   (T0 - 50 * DAY, T0 - 20 * DAY)]
        sizes = [t.expired(p, q) for p, q in windows]
        assert sizes[0] == 0 and sizes[1] == 0 and sizes[2] > n // 2 and 0 < sizes[5] < n, sizes
        # no group, some (a user count of a thousand or more leaves some too young at -118 days), every group, and a window
        # that takes now - window below int64 (no group)
        arch_now = [T0 - 200 * DAY, T0 - 119 * DAY - 20 * 3600 * 1000, T0 - 118 * DAY, T0, INT64_MIN + 5]
        asz = [t.archive(now) for now in arch_now]
        live = int(np.count_nonzero(t.end != INT64_MIN))
        assert asz[0] == 0 and asz[-1] == 0 and asz[3] == live, asz
        assert U < 1000 or 0 < asz[2] < live, asz
        # the capacity error reports the total; a repeat with room fills the queue
        want = oracle_py.expired_queue(t.end, INT64_MIN, 2 ** 62)
        rc, q, _ = raw_queue(t.comm, "pie_comm_expired_queue", INT64_MIN, 2 ** 62, want.size - 1)
        assert rc == PIE_E_CAPACITY and q == want.size, (rc, q)
        rc, q, out = raw_queue(t.comm, "pie_comm_expired_queue", INT64_MIN, 2 ** 62, want.size)
        assert rc == 0 and q == want.size and np.array_equal(out, want)
        want = oracle_py.archive_queue(t.start, t.end, t.user, U, T0 - 118 * DAY, W)
        if want.size:
            rc, q, _ = raw_queue(t.comm, "pie_comm_archive_queue", T0 - 118 * DAY, W, want.size // 2)
            assert rc == PIE_E_CAPACITY and q == want.size, (rc, q)
        rc, q, out = raw_queue(t.comm, "pie_comm_archive_queue", T0 - 118 * DAY, W, want.size)
        assert rc == 0 and q == want.size and np.array_equal(out, want)
        # touches and tombstones applied to the shards at global rows
        rng = np.random.default_rng(world)
        rows = rng.choice(n, min(500, n // 4), replace=False)
        new_end = rng.integers(T0 - 200 * DAY, T0 + 200 * DAY, rows.size).astype(np.int64)
        new_end[:20] = INT64_MIN
        t.set_end(rows, new_end)
        t.delete_user(int(t.user[n // 3]))
        for p, q in windows:
            t.expired(p, q)
        for now in arch_now:
            t.archive(now)
        checks += len(windows) * 2 + len(arch_now) * 2 + 4
        t.comm.close()
    print("worlds ok: %d checks" % checks)


def case_errors():
    # a pipelined step begun and not collected: every queue call is refused; after the collect it works
    t = Sharded(3, 300_000, 2000)
    for c in t.ctxs:
        c.set_disciplines(0xFFFFFFFF, 32)
    qs = [(T0 - 6 * 3600 * 1000, T0 - 61 * DAY, 0x55555555)]
    t.comm.step_reserve(1, 0, 1 << 16)
    t.comm.step_begin(qs)
    for fn, a, b in (("pie_comm_expired_queue", INT64_MIN, T0), ("pie_comm_archive_queue", T0, W)):
        rc, q, _ = raw_queue(t.comm, fn, a, b, t.n)
        assert rc == PIE_E_STATE and q == 0, (fn, rc, q)
    t.comm.step_finish()
    t.comm.step_collect()
    t.expired(INT64_MIN, T0)
    t.archive(T0)
    t.comm.close()
    # a shard that holds a row its map does not cover (appended after the sharding): every rank returns PIE_E_STATE
    t = Sharded(3, 300_000, 2000)
    c1 = t.ctxs[1]
    c1.append_rows(np.array([T0], np.int64), np.array([T0 + DAY], np.int64), np.array([0], np.int32), np.array([1], np.int32), c1.n_users)
    for call in (lambda: t.comm.expired_queue(INT64_MIN, 2 ** 62), lambda: t.comm.archive_queue(T0, W)):
        try:
            call()
            raise AssertionError("the uncovered row went unnoticed")
        except PieError as e:
            assert e.code == PIE_E_STATE and "rank 1" in str(e), e
    try:
        t.comm.queue_read(0)
        raise AssertionError("a failed call left a queue behind")
    except PieError as e:
        assert e.code == PIE_E_STATE
    t.comm.close()
    print("errors ok")


EDGE_TOTALS = (0, 1, 255, 256, 257, 4097)   # around one block of the merge (256 lanes) and past sixteen of them


def edge_windows(end, rank_of_row):
    """Windows (prev, now, total) cut from the sorted end column: one per EDGE_TOTALS whose queue holds exactly that many rows,
    then the longest one (total None) whose rows all sit on one shard.  A window is the sorted positions [a, b) with a new end
    value beginning at a and at b, so prev = the end before a, now = the end at b - 1."""
    order = np.argsort(end, kind="stable")
    se, rs = end[order], rank_of_row[order]
    cuts = np.flatnonzero(np.diff(se) > 0) + 1
    is_cut = np.zeros(se.size + 1, bool)
    is_cut[cuts] = True
    is_cut[se.size] = True
    mid = int(se[se.size // 2])
    out = [(mid, mid, 0)]
    for total in EDGE_TOTALS[1:]:
        a = next(int(a) for a in cuts[cuts.size // 3:] if a + total <= se.size and is_cut[a + total])
        out.append((int(se[a - 1]), int(se[a + total - 1]), total))
    # maximal runs of one rank in end order, shrunk to the cuts inside them
    edges = np.concatenate(([0], np.flatnonzero(np.diff(rs) != 0) + 1, [se.size]))
    best = (0, 0)
    for p, q in zip(edges[:-1], edges[1:]):
        inner = cuts[(cuts >= p) & (cuts <= q)]
        if inner.size >= 2 and inner[-1] - inner[0] > best[1] - best[0]:
            best = (int(inner[0]), int(inner[-1]))
    assert best[1] - best[0] >= 2, "no run of two rows on one shard"
    out.append((int(se[best[0] - 1]), int(se[best[1] - 1]), None))
    return out


def case_edges():
    """The synchronous expired queue at the merge's block boundaries, and the in-flight form beside it on the same communicator."""
    checks = 0
    for world, n, U in [(3, 20_000, 1000), (5, 20_000, 7)]:
        # the windows are designed and checked on the host, with the oracle alone, before anything runs on the GPU
        _, end, user, _ = oracle_py.gen(SEED, n, 0, n, U, 32, 1)
        owner = np.array([pie.shard_of(int(u), world) for u in user], np.int32)
        windows = edge_windows(end, owner)
        wants = [oracle_py.expired_queue(end, p, q) for p, q, _ in windows]
        assert [w.size for w in wants[:-1]] == list(EDGE_TOTALS), [w.size for w in wants]
        assert wants[-1].size >= 2 and np.unique(owner[wants[-1]]).size == 1
        t = Sharded(world, n, U)
        assert np.array_equal(t.rank_of_row, owner)
        if U == 7:
            assert min(m.size for m in t.rows_g) == 0, "7 users over 5 ranks leave one rank without rows"
        for (p, q, _), want in zip(windows, wants):
            rows, src_rank, src_row = t.comm.expired_queue(p, q, sources=True)
            assert np.array_equal(rows, want), (world, p, q, rows.size, want.size)
            t.check_sources(rows, src_rank, src_row)
            t.comm.expired_queue_begin(p, q, cap_rows=want.size)     # (0 rows: the begin counts only)
            res = t.comm.expired_queue_finish()
            rows2, owner2 = res if want.size else (np.zeros(0, np.int32), np.zeros(0, np.int32))
            assert (want.size or res == 0) and np.array_equal(rows2, want) and np.array_equal(owner2, src_rank), (world, p, q)
            checks += 1
        t.comm.close()
    print("edges ok: %d windows" % checks)


def case_cfg5():
    t = Sharded(8, 10 ** 8, 10 ** 5)
    e = t.expired(T0 - 6 * 3600 * 1000 - 3600 * 1000, T0 - 6 * 3600 * 1000, full=False)
    # the oracle's numpy restatement of the archive chain: the C oracle's per-row loop takes many minutes at 10^8 rows
    a = t.archive(T0 - 118 * DAY, full=False, oracle_fn=oracle_py.archive_queue_numpy)
    assert e > 0 and a > 0
    print("cfg5 ok: expired %d archive %d" % (e, a))


def case_real():
    try:
        comm = pie.PieComm([0])
    except PieError as e:
        print("skip: %s" % e)
        return
    comm.gen_synthetic_sharded(SEED, 200_003, 1000, 32, 1)
    s, e, u, _ = oracle_py.gen(SEED, 200_003, 0, 200_003, 1000, 32, 1)
    assert np.array_equal(comm.expired_queue(INT64_MIN, T0), oracle_py.expired_queue(e, INT64_MIN, T0))
    assert np.array_equal(comm.archive_queue(T0 - 118 * DAY, W), oracle_py.archive_queue(s, e, u, 1000, T0 - 118 * DAY, W))
    comm.close()
    print("real ok")


if __name__ == "__main__":
    {"worlds": case_worlds, "errors": case_errors, "edges": case_edges, "cfg5": case_cfg5, "real": case_real}[CASE]()
