"""GPU: the ordered row lists at the edges of their skeleton.  Every call that walks the table once and writes the rows of a
predicate in table order (per-block counts, a prefix, a block-ordered write) is run on tables whose sizes sit on the edges of a
256-row step and of a block, with hits placed on those edges; the tombstones are checked through everything derived from `end`.
Expectations are numpy's and the oracle's, never the library's.

  list modes     prune_before, delete_user, retention_purge, retention_purge under a two-transition zone, and the two-pass
                 expired queue (PIE_EXPIRED_TWO_PASS), plain and with the hot index and the ordered run on
  capacity       a list one, 4096 and 4097 entries too long: PIE_E_CAPACITY, the count reported, the rows tombstoned
  delete_users   the same tables through the wave-owned pass (the tombstone's second caller)
  shard_table    blocks of 16 384 rows, worlds 2 and 3, a rank that keeps no row
  archive queue  512 rows per step, two rows per lane
  mapped lists   a shard's global rows, and the communicator's global and local rows (run as a worker process: the
                 communicator needs the one-GPU stand-in for RCCL loaded before anything else)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT64_MIN = -(2 ** 63)
ALL = 2 ** 64 - 1
HOUR = 3600 * 1000
DAY = 24 * HOUR
PIE_E_CAPACITY = -5
U, D = 37, 32
STEP, BLOCK = 256, 4096          # rows of one step of the block-ordered write; rows of a block of the streaming plan at these sizes
SIZES = (1, 255, 256, 257, 4095, 4096, 4097, 8193)
PATTERNS = ("none", "all", "row_0", "row_last", "last_of_every_step", "first_of_every_block_but_the_first", "mix")
MODES = ("prune", "delete_user", "retention", "retention_tz", "expired_two_pass")
CONFIGS = {"plain": (0, 0), "hot_ordered": (1, 2)}


def hits(pattern, n, block=BLOCK):
    h = np.zeros(n, bool)
    if pattern == "all":
        h[:] = True
    elif pattern == "row_0":
        h[0] = True
    elif pattern == "row_last":
        h[n - 1] = True
    elif pattern == "last_of_every_step":
        h[STEP - 1::STEP] = True
    elif pattern == "first_of_every_block_but_the_first":
        h[block::block] = True
    elif pattern == "mix":
        h = np.random.default_rng(n).random(n) < 0.5
    return h


def base_table(oracle, n):
    """n live rows, every `end` in the top of the range (where the liveness keys decide without reading `end`), users below U - 3"""
    t0, top = oracle.T0_MS, oracle.T0_MS + oracle.SPAN_MS
    rng = np.random.default_rng(1000 + n)
    i = np.arange(n, dtype=np.int64)
    return [t0 + i * 1000, top + HOUR + i * 997, rng.integers(0, U - 3, n).astype(np.int32), rng.integers(0, D, n).astype(np.int32)]


def mode_case(oracle, mode, cols, h):
    """Bend the column the mode's predicate reads so that exactly the rows of h match -> (call(ctx) -> list, the expected list)"""
    s, e, u, d = cols
    t0, top = oracle.T0_MS, oracle.T0_MS + oracle.SPAN_MS
    idx = np.nonzero(h)[0]
    if mode == "prune":
        s[idx] = t0 - 1 - idx
        want = np.nonzero((s < t0) & (e != INT64_MIN))[0]
        call = lambda c: c.prune_before(t0)
    elif mode == "delete_user":
        u[idx] = U - 1
        want = np.nonzero((u == U - 1) & (e != INT64_MIN))[0]
        call = lambda c: c.delete_user(U - 1)
    elif mode == "retention":
        now, tz = t0 + 30 * DAY, 3 * HOUR
        s[idx] = now - 400 * DAY - idx
        want = oracle.retention_queue(s, e, now, 2, tz)
        call = lambda c: c.retention_purge(now, 2, tz)
    elif mode == "retention_tz":
        now = t0 + 30 * DAY
        zone = (np.array([t0 - 200 * DAY, t0 + 10 * DAY], np.int64), np.array([0, HOUR, 0], np.int64))
        s[idx] = now - 400 * DAY - idx
        want = oracle.retention_queue_tz(s, e, now, 2, *zone)
        call = lambda c: c.retention_purge(now, 2, tz_table=zone)
    else:
        e[idx] = top - idx % 1000
        want = oracle.expired_queue(e, top - HOUR, top)

        def call(c):
            os.environ["PIE_EXPIRED_TWO_PASS"] = "1"   # read by every call
            try:
                return c.expired_queue(top - HOUR, top)
            finally:
                del os.environ["PIE_EXPIRED_TWO_PASS"]
    assert np.array_equal(want, idx), "the pattern is not what the reference selects"
    return call, want.astype(np.int32)


def top_queries(e):
    live = np.sort(e[e != INT64_MIN])
    if live.size == 0:
        return [(0, INT64_MIN, 0xFFFFFFFF)] * 16
    return [(int(live[live.size - 1 - (q * live.size) // 17]) - 1, INT64_MIN, 0xFFFFFFFF) for q in range(16)]


def new_ctx(pie, config):
    from table_model import ctx_with_env
    hot, ordered = CONFIGS[config]
    ctx = ctx_with_env(pie, hot, 1)
    ctx.set_ordered_run(ordered)
    return ctx


def load(ctx, cols):
    ctx.load_columns(*cols, U)
    ctx.set_disciplines(ALL, D)
    ctx.scan_batch(top_queries(cols[1]))   # builds the hot index / the ordered run where there is one


def check_derived(oracle, ctx, cols, tag):
    """`end` itself, then everything kept in step with it: a full scan (the 2-byte key), top-of-range batches (the 1-byte key, or
    the hot index, or the ordered run)"""
    s, e, u, d = cols
    assert np.array_equal(ctx.read_columns()[1], e), (tag, "end column")
    ctx.set_disciplines(ALL, D)
    for now in (oracle.T0_MS, INT64_MIN):
        for name, a, b in zip(("counts", "offsets", "idx"), ctx.scan(now, INT64_MIN), oracle.scan(s, e, u, d, U, now, INT64_MIN, ALL)):
            assert np.array_equal(a, b), (tag, "scan", now, name)
    qs = top_queries(e)
    for qi, (q, got) in enumerate(zip(qs, ctx.scan_batch(qs))):
        for name, a, b in zip(("counts", "offsets", "idx"), got, oracle.scan(s, e, u, d, U, *q)):
            assert np.array_equal(a, b), (tag, "batch query", qi, name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("config", tuple(CONFIGS))
def test_list_modes(pie, oracle, config, n, mode):
    ctx = new_ctx(pie, config)
    try:
        for pattern in PATTERNS:
            tag = (config, n, mode, pattern)
            cols = base_table(oracle, n)
            call, want = mode_case(oracle, mode, cols, hits(pattern, n))
            load(ctx, cols)
            got = call(ctx)
            assert got.dtype == np.int32 and np.array_equal(got, want), (tag, "list")
            if mode == "expired_two_pass":
                assert np.array_equal(call(ctx), want), (tag, "the queue changed the table")
            else:
                cols[1][want] = INT64_MIN
                assert call(ctx).size == 0, (tag, "a second call found rows")
            check_derived(oracle, ctx, cols, tag)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ capacity
def raw_list(pie, ctx, mode, cap, n):
    lib, t0 = pie.load_library(), 1700000000000
    rows, k = np.full(max(cap, 1), -7, np.int32), C.c_size_t(99)
    out = rows.ctypes.data_as(C.c_void_p)
    if mode == "prune":
        rc = lib.pie_prune_before(ctx._ctx, C.c_int64(t0), out, C.c_size_t(cap), C.byref(k))
    elif mode == "delete_user":
        rc = lib.pie_delete_user(ctx._ctx, C.c_int32(U - 1), out, C.c_size_t(cap), C.byref(k))
    elif mode == "retention":
        rc = lib.pie_retention_purge(ctx._ctx, C.c_int64(t0 + 30 * DAY), C.c_int32(2), C.c_int64(3 * HOUR), out, C.c_size_t(cap), C.byref(k))
    else:
        ids, per = np.array([U - 1], np.int32), np.zeros(1, np.int32)
        rc = lib.pie_delete_users(ctx._ctx, ids.ctypes.data_as(C.c_void_p), C.c_size_t(1), out, C.c_size_t(cap), C.byref(k),
                                  per.ctypes.data_as(C.c_void_p))
        assert per[0] == n
    return rc, int(k.value)


@pytest.mark.parametrize("cap", (0, 1, 4096))
@pytest.mark.parametrize("mode", ("prune", "delete_user", "retention", "delete_users"))
def test_capacity(pie, oracle, mode, cap):
    n = 4097
    assert oracle.T0_MS == 1700000000000
    cols = base_table(oracle, n)
    mode_case(oracle, "delete_user" if mode == "delete_users" else mode, cols, hits("all", n))
    ctx = new_ctx(pie, "plain")
    try:
        load(ctx, cols)
        rc, k = raw_list(pie, ctx, mode, cap, n)
        assert rc == PIE_E_CAPACITY and k == n, "a list above cap: PIE_E_CAPACITY and the count"
        cols[1][:] = INT64_MIN
        check_derived(oracle, ctx, cols, (mode, cap, "the rows were not tombstoned"))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ delete_users
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("config", tuple(CONFIGS))
def test_delete_users(pie, oracle, config, n):
    ids = np.array([U - 1, U - 3, 9999, U - 2, U - 1, -4], np.int32)   # an unknown id, a repeat, a negative id
    ctx = new_ctx(pie, config)
    try:
        for pattern in PATTERNS:
            tag = (config, n, pattern)
            cols = base_table(oracle, n)
            want = np.nonzero(hits(pattern, n))[0].astype(np.int32)
            cols[2][want] = U - 1 - want % 3
            per = np.array([np.count_nonzero(cols[2] == x) for x in ids], np.int32)
            per[4] = 0   # the repeat: the first occurrence has the count
            load(ctx, cols)
            rows, got_per = ctx.delete_users(ids)
            assert rows.dtype == np.int32 and np.array_equal(rows, want), (tag, "list")
            assert np.array_equal(got_per, per), (tag, "per-user counts")
            cols[1][want] = INT64_MIN
            again, per2 = ctx.delete_users(ids)
            assert again.size == 0 and not per2.any(), (tag, "a second call found rows")
            check_derived(oracle, ctx, cols, tag)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ shard_table
@pytest.mark.parametrize("empty_rank", (False, True), ids=("every_rank_holds_rows", "last_rank_holds_none"))
@pytest.mark.parametrize("world", (2, 3))
@pytest.mark.parametrize("n", (1, 16383, 16384, 16385, 32769))
def test_shard_table(pie, oracle, n, world, empty_rank):
    users = 41
    owner = np.array([oracle.shard_of(g, world) for g in range(users)], np.int32)
    pool = np.nonzero(owner != world - 1)[0] if empty_rank else np.arange(users)
    rng = np.random.default_rng(n + world)
    s, e, _, d = base_table(oracle, n)
    e[3::11] = INT64_MIN
    u = pool[rng.integers(0, pool.size, n)].astype(np.int32)
    some_empty = False
    for rank in range(world):
        held = np.nonzero(owner[u] == rank)[0]
        mine = np.nonzero(owner == rank)[0]
        local = np.full(users, -1, np.int32)
        local[mine] = np.arange(mine.size, dtype=np.int32)
        with pie.PieScan(0) as ctx:
            ctx.load_columns(s, e, u, d, users)
            nr, nu = ctx.shard_table(rank, world)
            assert nr == held.size and nu == max(mine.size, 1), (rank, "rows, users")
            rows_g, users_g = ctx.shard_maps()
            assert np.array_equal(rows_g, held), (rank, "row map")
            assert np.array_equal(users_g[: mine.size], mine), (rank, "user map")
            if nr:
                for name, a, w in zip(("start", "end", "user", "disc"), ctx.read_columns(), (s[held], e[held], local[u[held]], d[held])):
                    assert np.array_equal(a, w), (rank, name)
            some_empty |= nr == 0
    assert some_empty == (empty_rank or n == 1), "a rank that keeps no row was not among the cases"


# ------------------------------------------------------------------------------------------------ archive selection
@pytest.mark.parametrize("users", (1, 37))
@pytest.mark.parametrize("n", (1, 2, 511, 512, 513, 4097))
def test_archive_selection(pie, oracle, n, users):
    rng = np.random.default_rng(7 * n + users)
    s, e, _, d = base_table(oracle, n)
    u = rng.integers(0, users, n).astype(np.int32)
    e[10::11] = INT64_MIN
    with pie.PieScan(0) as ctx:
        ctx.load_columns(s, e, u, d, users)
        for now in (int(s[n // 2]) + 12 * HOUR, int(s[0]) + 12 * HOUR - 1, int(s[n - 1]) + 13 * HOUR):   # some groups, none, all
            want = oracle.archive_queue(s, e, u, users, now, 12 * HOUR)
            got = ctx.archive_queue(now, 12 * HOUR)
            assert got.dtype == np.int32 and np.array_equal(got, want), (now - int(s[0]), got.size, want.size)


# ------------------------------------------------------------------------------------------------ mapped lists
def mapped_table(oracle, n):
    cols = base_table(oracle, n)
    h = hits("mix", n)
    h[[0, n - 1]] = True
    h[STEP - 1::STEP] = True
    h[BLOCK::BLOCK] = True
    cols[0][h] = oracle.T0_MS - 1 - np.nonzero(h)[0]
    return cols, np.nonzero(h)[0].astype(np.int32)


@pytest.mark.parametrize("n", (4097, 8193))
def test_mapped_list_of_a_shard(pie, oracle, n):
    cols, want = mapped_table(oracle, n)
    owner = np.array([oracle.shard_of(g, 2) for g in range(U)], np.int32)
    for rank in range(2):
        with pie.PieScan(0) as ctx:
            ctx.load_columns(*cols, U)
            ctx.shard_table(rank, 2)
            got = ctx.shard_prune_before(oracle.T0_MS)
            mine = want[owner[cols[2][want]] == rank]
            assert got.dtype == np.int32 and np.array_equal(got, mine), (rank, "global rows")
            assert ctx.shard_prune_before(oracle.T0_MS).size == 0, (rank, "a second call found rows")
            held = np.nonzero(owner[cols[2]] == rank)[0]
            e = cols[1][held].copy()
            e[np.isin(held, mine)] = INT64_MIN
            assert np.array_equal(ctx.read_columns()[1], e), (rank, "end column")


def test_mapped_list_of_the_communicator(pie, oracle):
    """pie_comm_prune_before with the source rows wanted, on two shards of 4097 and of 8193 global rows"""
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "comm"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=300, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert res.returncode == 0 and "comm ok" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


def comm_worker():
    from comm_mutate_worker import oracle_py, pie   # loads the stand-in for RCCL first
    for n in (4097, 8193):
        cols, want = mapped_table(oracle_py, n)
        owner = np.array([oracle_py.shard_of(g, 2) for g in range(U)], np.int32)
        comm = pie.PieComm([0, 0])
        try:
            for r in range(2):
                comm.ctx(r).load_columns(*cols, U)
                comm.ctx(r).shard_table(r, 2)
            rows, src_rank, src_row = comm.prune_before(oracle_py.T0_MS, sources=True)
            assert np.array_equal(rows, want), (n, "global rows")
            assert np.array_equal(src_rank, owner[cols[2][want]]), (n, "source ranks")
            local = np.zeros(n, np.int64)   # a global row's place among the rows of its shard
            for r in range(2):
                held = np.nonzero(owner[cols[2]] == r)[0]
                local[held] = np.arange(held.size)
            assert np.array_equal(src_row, local[want]), (n, "local rows")
            assert comm.prune_before(oracle_py.T0_MS).size == 0, (n, "a second call found rows")
        finally:
            comm.close()
    print("comm ok")


if __name__ == "__main__":
    comm_worker()
