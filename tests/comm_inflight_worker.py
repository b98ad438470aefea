"""Token lookups and the expired queue behind the communicator WHILE STEPS ARE IN FLIGHT (pie_comm_token_lookup_begin / _finish /
_room, pie_comm_expired_queue_begin / _finish / _room), in a fresh process whose "RCCL" is tests/stub_rccl.c (PIE_RCCL_LIB):
several shards of one table on GPU 0.  The models are the UNSHARDED TokenModel of tests/token_model.py and the oracle on the
unsharded table.  The table: 40 000 rows, 300 users, 7 disciplines.
usage: comm_inflight_worker.py CASE [WORLD]
  lookup W   three ordinary steps in flight; lookups of 0, 1, 64, 65 and 4096 keys (present, absent, expired under their own clock,
             tombstoned, duplicated, carried by rows of two shards), four begun before any finish; the steps' feeds afterwards
  wide W     the same lookups once with two wide steps in flight
  expired W  windows (empty, one shard only, the whole range, totals of 256 and 257) x cap_rows (0, the total, the total - 1) with
             three ordinary steps in flight, against pie_comm_expired_queue once drained and the oracle
  errors     finish with nothing begun, a second queue, a slot taken on a shard directly, cap < k, destroy with work begun"""
import ctypes as C
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
CASE = sys.argv[1]
WORLD = int(sys.argv[2]) if len(sys.argv) > 2 else 3
stub_dir = os.path.join(REPO, "tests", "_stub")
os.makedirs(stub_dir, exist_ok=True)
stub = os.path.join(stub_dir, "libstub_rccl_inflight_%d.so" % os.getpid())
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                "-L/opt/rocm/lib", "-lamdhip64"], check=True)
os.environ["PIE_RCCL_LIB"] = stub

import numpy as np
import torch  # noqa: F401  (before libpie_hip.so initialises HIP)
import oracle_py
import sph_pie_amd as pie
from sph_pie_amd.binding import PieError
from token_model import END_NONE, TokenModel

T0, SPAN, TTL, SEED = oracle_py.T0_MS, oracle_py.SPAN_MS, oracle_py.TTL_MS, 0x5EED5EED
N, U, D = 40000, 300, 7
TOP = T0 + SPAN
PIE_E_INVAL, PIE_E_CAPACITY, PIE_E_STATE = -1, -5, -6
DAY = 86400 * 1000
QUERIES = [(T0 - TTL // 3 - 977 * q, T0 - (61 + q % 2) * DAY, (0x55, 0x2A, 0x7F)[q % 3]) for q in range(3)]   # 100 .. 200 rows each


def random_keys(seed, n):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (n, 2), dtype=np.uint64)


def refused(code, fn, text=None):
    try:
        fn()
    except PieError as e:
        assert e.code == code and (text is None or text in str(e)), e
        return e
    raise AssertionError("the call went through")


class Table:
    """A communicator over one synthetic table and the unsharded model, kept in step."""

    def __init__(self, world):
        self.world = world
        self.comm = pie.PieComm([0] * world)
        self.comm.gen_synthetic_sharded(SEED, N, U, D, 0)
        self.tm = TokenModel(*oracle_py.gen(SEED, N, 0, N, U, D, 0))
        self.owner = np.array([pie.shard_of(int(u), world) for u in self.tm.user], np.int32)   # of every row
        self.maps = []
        for r in range(world):
            c = self.comm.ctx(r)
            c.set_disciplines(0x7F, D)
            rows_g, users_g = c.shard_maps()
            self.maps.append((rows_g.astype(np.int64), users_g[: c.n_users].astype(np.int64)))
        assert sum(m[0].size for m in self.maps) == N

    def set_end(self, rows, new_end):
        rows, new_end = np.asarray(rows, np.int32), np.asarray(new_end, np.int64)
        self.comm.set_end(rows, new_end)
        self.tm.end[rows] = new_end

    def want_feeds(self):
        tm = self.tm
        return [oracle_py.scan(tm.start, tm.end, tm.user, tm.disc, U, *q) for q in QUERIES]

    def check_ordinary(self, step, want):
        """every user's feed of every query from the gathered union messages, as rank 0 holds them"""
        got = [self.comm.step_read_gathered(0, r, step) for r in range(self.world)]
        for q in range(len(QUERIES)):
            _, wo, wi = want[q]
            total = 0
            for r in range(self.world):
                uoff, rows, masks = got[r]
                rows_r, users_r = self.maps[r]
                sel = ((masks >> np.uint64(q)) & np.uint64(1)) == 1
                total += int(sel.sum())
                for lu in range(users_r.size):
                    gu, a, b = int(users_r[lu]), int(uoff[lu]), int(uoff[lu + 1])
                    assert np.array_equal(rows_r[rows[a:b][sel[a:b]]], wi[wo[gu]:wo[gu + 1]]), (step, q, r, gu)
            assert total == wi.size, (step, q)

    def check_wide(self, step, want):
        per_rank = []
        for r in range(self.world):
            uoff, rows, masks, mu = self.comm.wide_step_read_gathered(0, r, step)
            rows_r, users_r = self.maps[r]
            per_rank.append((rows_r[rows], np.repeat(users_r, np.diff(uoff[: users_r.size + 1])), masks))
        for q in range(len(QUERIES)):
            wc, _, wi = want[q]
            bits = [((m[:, 0] >> np.uint64(q)) & np.uint64(1)).astype(bool) for _, _, m in per_rank]
            g_rows = np.concatenate([p[0][b] for p, b in zip(per_rank, bits)])
            g_users = np.concatenate([p[1][b] for p, b in zip(per_rank, bits)])
            assert np.array_equal(g_rows[np.argsort(g_users, kind="stable")], wi), (step, q)
            assert np.array_equal(np.bincount(g_users, minlength=U), wc), (step, q)


def token_table(world):
    """-> (table, keys, asks): a token column with about 50 keys carried by rows of users on different shards, some rows uncovered
    and some tombstoned; asks[k] = (keys, per-key now) for k in 0, 1, 64, 65, 4096"""
    t = Table(world)
    rng = np.random.default_rng(100 + world)
    keys = random_keys(10 + world, N)
    pairs, used = [], set(range(100, 150))
    for a in range(100, 150):
        other = np.nonzero((t.owner != t.owner[a]) & (np.arange(N) > a))[0] if world > 1 else np.arange(a + 1, N)
        b = next(int(x) for x in other[a:] if int(x) not in used)
        used.add(b)
        keys[b] = keys[a]
        pairs.append((a, b))
    t.comm.token_set(keys[: N - 50])
    t.tm.token_set(keys[: N - 50])
    tomb = rng.choice(N - 50, 40, replace=False)
    t.set_end(tomb, np.full(40, END_NONE, np.int64))
    ends = t.tm.end[t.tm.end != END_NONE]
    lo, hi = int(ends.min()), int(ends.max())
    asks = {}
    for k in (0, 1, 64, 65, 4096):
        rows = rng.integers(0, N - 50, k)
        ask = keys[rows].copy()
        now = rng.integers(lo - 5, hi + 5, k).astype(np.int64)       # expired or live under its OWN clock
        if k >= 64:
            ask[0:8] = keys[[a for a, _ in pairs[:8]]]                # carried by rows of two shards
            ask[8:16] = keys[tomb[:8]]                                # tombstoned
            ask[16:24] = random_keys(k, 8)                            # absent
            ask[24:28] = keys[N - 50: N - 46]                         # rows the column does not cover
            ask[28:32] = ask[0:4]                                     # duplicated in the call, under another clock
            now[32:36] = END_NONE                                     # every found row that is not a tombstone is live
        asks[k] = (ask, now)
    return t, keys, pairs, asks


def check_lookup(t, got, ask, now):
    want = t.tm.lookup(ask, now)
    k = ask.shape[0]
    assert all(got[c].shape == (k,) for c in ("row", "live", "user", "start", "end", "owner"))
    assert np.array_equal(got["row"], want["row"]), "row"
    assert np.array_equal(got["live"], want["live"]), "live"
    f = want["found"]
    for col in ("user", "start", "end"):
        assert np.array_equal(got[col][f], want[col][f]), col
    assert np.array_equal(got["owner"][f], t.owner[want["row"][f]]) and np.all(got["owner"][~f] == -1), "owner"
    return want


def lookups_in_flight(t, keys, pairs, asks):
    """four begun before any finish, a fifth refused, finished in begin order; then the fifth size"""
    comm = t.comm
    assert comm.token_lookup_room() == 4
    first = (4096, 0, 65, 1)
    for i, k in enumerate(first):
        comm.token_lookup_begin(*asks[k])
        assert comm.token_lookup_room() == 3 - i
        assert [comm.ctx(r).token_lookup_room() for r in range(t.world)] == [3 - i] * t.world
    refused(PIE_E_STATE, lambda: comm.token_lookup_begin(*asks[64]))
    refused(PIE_E_STATE, lambda: comm.token_lookup(keys[:2], TOP))      # the synchronous form keeps its rule
    assert comm.token_lookup_room() == 0
    for i, k in enumerate(first):
        want = check_lookup(t, comm.token_lookup_finish(), *asks[k])
        assert comm.token_lookup_room() == i + 1
        if k >= 64:
            assert list(want["row"][:8]) == [b for _, b in pairs[:8]], "of two rows under one key the largest global row answers"
            assert np.all(want["live"][8:16] == 0) and np.all(want["row"][8:16] >= 0) and np.all(want["row"][16:28] == -1)
    comm.token_lookup_begin(*asks[64])
    comm.token_lookup_begin(asks[65][0], TOP)                            # one clock for every key
    check_lookup(t, comm.token_lookup_finish(), *asks[64])
    check_lookup(t, comm.token_lookup_finish(), asks[65][0], np.full(65, TOP, np.int64))
    assert comm.token_lookup_room() == 4
    refused(PIE_E_STATE, comm.token_lookup_finish)


def case_lookup():
    t, keys, pairs, asks = token_table(WORLD)
    comm = t.comm
    want = t.want_feeds()
    comm.step_reserve(len(QUERIES), 0, 1 << 16)
    for _ in range(3):
        comm.step_begin(QUERIES)
    lookups_in_flight(t, keys, pairs, asks)
    for _ in range(3):
        ms = comm.step_finish()
        assert [sum(ms[r][q] for r in range(WORLD)) for q in range(len(QUERIES))] == [int(w[2].size) for w in want]
    lookups_in_flight(t, keys, pairs, asks)                             # finished and uncollected: in flight all the same
    steps = [comm.step_collect() for _ in range(3)]
    assert steps == [0, 1, 2]
    for s in steps:
        t.check_ordinary(s, want)
    comm.close()
    print("lookup ok: world %d" % WORLD)


def case_wide():
    t, keys, pairs, asks = token_table(WORLD)
    comm = t.comm
    want = t.want_feeds()
    comm.wide_step_reserve(len(QUERIES), 0, 1 << 16)
    step = 0
    while True:   # a shard's first wide batches may keep no union while its union slots grow (Mu = -1): repeated, as the header says
        assert step < 4
        comm.wide_step_begin(QUERIES)
        comm.wide_step_finish()
        step += 1
        try:
            comm.wide_step_collect()
            break
        except PieError as e:
            assert e.code == PIE_E_CAPACITY and np.any(comm.wide_step_status(step - 1) < 0), e
    comm.wide_step_begin(QUERIES)
    comm.wide_step_begin(QUERIES)
    lookups_in_flight(t, keys, pairs, asks)
    for _ in range(2):
        comm.wide_step_finish()
    for s in (step, step + 1):
        assert comm.wide_step_collect() == s
        t.check_wide(s, want)
    comm.close()
    print("wide ok: world %d" % WORLD)


def case_expired():
    t = Table(WORLD)
    comm, tm = t.comm, t.tm
    rng = np.random.default_rng(200 + WORLD)
    # rows touched first: 256 ends at X + 1 and one more at X + 2 (the merge's block edge), and five rows of ONE shard at Y + 1
    X, Y = TOP + 10 * TTL, TOP + 20 * TTL
    edge = rng.choice(N, 257, replace=False)
    rest = np.setdiff1d(np.arange(N), edge)
    one = rest[t.owner[rest] == t.owner[rest[0]]][:5]
    t.set_end(edge, np.concatenate([np.full(256, X + 1), [X + 2]]).astype(np.int64))
    t.set_end(one, np.full(5, Y + 1, np.int64))
    t.set_end(rest[1000:1020], np.full(20, END_NONE, np.int64))
    windows = [(TOP, TOP), (TOP, TOP - 1), (Y, Y + 1), (END_NONE, 2 ** 62), (X, X + 1), (X, X + 2), (T0 - TTL, T0)]
    want = {w: oracle_py.expired_queue(tm.end, *w) for w in windows}
    assert [want[w].size for w in windows[:3]] == [0, 0, 5] and [want[w].size for w in windows[4:6]] == [256, 257]
    assert want[windows[3]].size == int((tm.end != END_NONE).sum()) > N // 2 and want[windows[6]].size > 100
    feeds = t.want_feeds()
    comm.step_reserve(len(QUERIES), 0, 1 << 16)
    for _ in range(3):
        comm.step_begin(QUERIES)
    got = {}
    for w in windows:
        total = want[w].size
        assert comm.expired_queue_room() == 1
        comm.expired_queue_begin(*w, cap_rows=0)
        assert comm.expired_queue_room() == 0
        refused(PIE_E_STATE, lambda: comm.expired_queue_begin(*w))                  # a second queue
        refused(PIE_E_STATE, lambda: comm.expired_queue(*w))                        # the synchronous form keeps its rule
        assert comm.expired_queue_finish() == total, w                               # counts only
        assert comm.inflight_queue_device_ptrs()[2:] == (0, total)
        comm.expired_queue_begin(*w, cap_rows=total)                                # the exact total (0 for an empty window: counts)
        res = comm.expired_queue_finish()
        rows, owner = res if total else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        assert np.array_equal(rows, want[w]), w
        assert np.array_equal(owner, t.owner[rows]), w
        assert comm.inflight_queue_device_ptrs()[2:] == (total, total)
        got[w] = rows
        if total > 1:
            comm.expired_queue_begin(*w, cap_rows=total - 1)
            e = refused(PIE_E_CAPACITY, comm.expired_queue_finish)
            assert e.length == total and np.array_equal(e.prefix, want[w][: total - 1]), w   # the true ascending prefix
            assert np.array_equal(e.prefix_owner, t.owner[e.prefix]), w
            assert comm.expired_queue_room() == 1                                   # consumed
        comm.expired_queue_begin(*w)                                                # room for the whole table
        rows, owner = comm.expired_queue_finish()
        assert np.array_equal(rows, want[w]) and np.array_equal(owner, t.owner[rows]), w
    assert np.unique(t.owner[got[windows[2]]]).size == 1
    for _ in range(3):
        comm.step_finish()
    steps = [comm.step_collect() for _ in range(3)]
    for s in steps:
        t.check_ordinary(s, feeds)
    for w in windows:   # the same table once drained
        assert np.array_equal(comm.expired_queue(*w), got[w]), w
    comm.close()
    print("expired ok: world %d" % WORLD)


def case_errors():
    t, keys, pairs, asks = token_table(3)
    comm, lib = t.comm, pie.load_library()
    refused(PIE_E_STATE, comm.token_lookup_finish)
    comm._expq_cap = 0
    refused(PIE_E_STATE, comm.expired_queue_finish)
    comm.step_reserve(len(QUERIES), 0, 1 << 16)
    comm.step_begin(QUERIES)
    # a slot taken on a shard directly: the communicator's begin is refused and no shard's room moves
    c1 = comm.ctx(1)
    c1.shard_token_lookup_begin(keys[:3], TOP)
    rooms = [comm.ctx(r).token_lookup_room() for r in range(3)]
    assert rooms == [4, 3, 4] and comm.token_lookup_room() == 3
    refused(PIE_E_STATE, lambda: comm.token_lookup_begin(*asks[64]), "rank 1")
    assert [comm.ctx(r).token_lookup_room() for r in range(3)] == rooms
    assert np.array_equal(c1.shard_token_lookup_finish()["row"] >= 0, t.owner[:3] == 1)
    c1.shard_expired_queue_begin(T0 - TTL, T0, 0)
    refused(PIE_E_STATE, lambda: comm.expired_queue_begin(T0 - TTL, T0), "rank 1")
    assert [comm.ctx(r).expired_queue_room() for r in range(3)] == [1, 0, 1]
    c1.shard_expired_queue_finish()
    # cap < k: the size comes back and the lookup stays finishable
    comm.token_lookup_begin(*asks[65])
    got = C.c_size_t(0)
    row = np.empty(65, np.int32)
    assert lib.pie_comm_token_lookup_finish(comm._c, row.ctypes.data_as(C.c_void_p), None, None, None, None, None, 64, C.byref(got)) == PIE_E_CAPACITY
    assert got.value == 65 and comm.token_lookup_room() == 3
    check_lookup(t, comm.token_lookup_finish(), *asks[65])
    assert comm.token_lookup_room() == 4
    # room below the begin's cap_rows: PIE_E_INVAL, nothing consumed
    want = oracle_py.expired_queue(t.tm.end, T0 - TTL, T0)
    comm.expired_queue_begin(T0 - TTL, T0, cap_rows=want.size)
    comm._expq_cap = want.size - 1
    refused(PIE_E_INVAL, comm.expired_queue_finish)
    assert comm.expired_queue_room() == 0
    refused(PIE_E_STATE, lambda: comm.expired_queue_begin(T0 - TTL, T0))
    comm._expq_cap = want.size
    rows, owner = comm.expired_queue_finish()
    assert np.array_equal(rows, want) and np.array_equal(owner, t.owner[rows])
    # bad arguments take nothing
    assert lib.pie_comm_token_lookup_begin(comm._c, None, None, 3) == PIE_E_INVAL and comm.token_lookup_room() == 4
    comm.step_finish()
    assert comm.step_collect() == 0
    # destroy with a lookup and a queue begun: it returns
    comm.token_lookup_begin(*asks[4096])
    comm.expired_queue_begin(END_NONE, 2 ** 62)
    comm.close()
    print("errors ok")


if __name__ == "__main__":
    try:
        {"lookup": case_lookup, "wide": case_wide, "expired": case_expired, "errors": case_errors}[CASE]()
    finally:
        try:
            os.unlink(stub)
        except OSError:
            pass
