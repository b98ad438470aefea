"""GPU: the archive queue on the designed tables of archive_cases.py (test_archive_cases_cpu.py shows what each one plants).

  every case     PieScan.archive_queue on a fresh context against the C oracle (oracle.archive_queue), then a plain scan
  pack message   pie_queue_info / pie_queue_pack_device for the cases of group_sizes, order, n_qual and tombstones: header, global
                 and local rows, group offsets, the words that must stay unwritten, the capacity errors; plain and after
                 pie_shard_table (worlds 2 and 3)
  state          the capacity error of pie_archive_queue and its repeat; the queue after appends that take n_users across a multiple
                 of 64 and across 393 216, after tombstones, delete_user and a compaction; with the hot index and the ordered run on
  forgetting     pie_set_end and pie_append_rows (growing and in place) forget the held queue

Every expectation is the oracle's on the model columns; none comes from the library."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import archive_cases as AC
from table_model import ctx_with_env

pytestmark = pytest.mark.gpu

INT64_MIN = -(2 ** 63)
ALL = 2 ** 64 - 1
D = 32
SENT = -7
PIE_E_CAPACITY, PIE_E_STATE = -5, -6


@functools.lru_cache(maxsize=None)
def n_cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=None)
def case(name):
    return AC.build(name, n_cus())


_want = {}


def wanted(oracle, name, k):
    """the oracle's queue of query k of a case: computed once, shared, never changed"""
    if (name, k) not in _want:
        start, end, user, _, U, queries, _ = case(name)
        _want[name, k] = oracle.archive_queue(start, end, user, U, *queries[k])
        _want[name, k].setflags(write=False)
    return _want[name, k]


def same_scan(oracle, ctx, cols, U, tag):
    ctx.set_disciplines(ALL, D)
    for what, a, b in zip(("counts", "offsets", "idx"), ctx.scan(AC.T0, INT64_MIN), oracle.scan(*cols, U, AC.T0, INT64_MIN, ALL)):
        assert np.array_equal(a, b), (tag, "scan", what)


def archive(oracle, ctx, cols, U, now=AC.T0, window=AC.W, tag=""):
    want = oracle.archive_queue(cols[0], cols[1], cols[2], U, now, window)
    got = ctx.archive_queue(now, window)
    assert got.dtype == np.int32 and np.array_equal(got, want), (tag, got.size, want.size)
    return want


# ------------------------------------------------------------------------------------------------ the pack message
def pack(ctx, cap_rows, cap_groups):
    words = 2 + 2 * cap_rows + cap_groups + 1
    buf = torch.full((words + 8,), SENT, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.queue_pack_device(buf.data_ptr(), cap_rows, cap_groups)
    ctx.synchronize()
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def check_message(host, cap_rows, cap_groups, rows_global, rows_local, goff, tag):
    q, g = rows_local.size, goff.size - 1
    assert host[0] == q and host[1] == g, (tag, "header", host[:2])
    rg, rl = host[2:2 + cap_rows], host[2 + cap_rows:2 + 2 * cap_rows]
    off, tail = host[2 + 2 * cap_rows:2 + 2 * cap_rows + cap_groups + 1], host[2 + 2 * cap_rows + cap_groups + 1:]
    assert np.array_equal(rg[:q], rows_global), (tag, "global rows")
    assert np.array_equal(rl[:q], rows_local), (tag, "local rows")
    assert np.array_equal(off[:g + 1], goff) and goff[-1] == q, (tag, "group offsets, closed by q")
    assert np.all(rg[q:] == SENT) and np.all(rl[q:] == SENT) and np.all(off[g + 1:] == SENT) and np.all(tail == SENT), (tag, "padding written")


def offsets_of(user, queue):
    sizes = AC.queue_groups(user, queue)[1]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def check_pack(pie, ctx, user, want, rows_global, tag, grow=(0, 1, 257)):
    """the queue `want` (local rows) is the one the context holds"""
    goff = offsets_of(user, want)
    q, g = want.size, goff.size - 1
    assert ctx.queue_info() == (2, q, g), (tag, "pie_queue_info")
    for more in grow:
        check_message(pack(ctx, q + more, g + more), q + more, g + more, rows_global, want, goff, (tag, more))
    for cap_rows, cap_groups in ((q - 1, g), (q, g - 1)):
        if min(cap_rows, cap_groups) < 0:
            continue
        buf = torch.full((2 + 2 * q + g + 1,), SENT, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(pie.PieError) as ei:
            ctx.queue_pack_device(buf.data_ptr(), cap_rows, cap_groups)
        ctx.synchronize()
        assert ei.value.code == PIE_E_CAPACITY and bool(torch.all(buf == SENT)), (tag, cap_rows, cap_groups)
    assert ctx.queue_info() == (2, q, g), (tag, "a refused pack keeps the queue")


@functools.lru_cache(maxsize=None)
def owners(oracle, U, world):
    return np.array([oracle.shard_of(g, world) for g in range(U)], np.int32)


def check_sharded_pack(pie, oracle, name):
    start, end, user, disc, U, queries, _ = case(name)
    for world in (2, 3):
        owner = owners(oracle, U, world)
        for rank in range(world):
            held = np.nonzero(owner[user] == rank)[0]
            want = oracle.archive_queue(start[held], end[held], user[held], U, *queries[0])
            with pie.PieScan(0) as ctx:
                ctx.load_columns(start, end, user, disc, U)
                ctx.shard_table(rank, world)
                assert np.array_equal(ctx.shard_maps()[0], held), (name, world, rank, "row map")
                assert ctx.archive_queue(*queries[0], fetch=False) == want.size
                check_pack(pie, ctx, user[held], want, held[want], (name, world, rank), grow=(0, 1))


# ------------------------------------------------------------------------------------------------ every case
@pytest.mark.parametrize("name", AC.names())
def test_case(pie, oracle, name):
    start, end, user, disc, U, queries, props = case(name)
    packed = props["family"] in AC.PACK_FAMILIES
    with pie.PieScan(0) as ctx:
        ctx.load_columns(start, end, user, disc, U)
        for k, (now, window) in enumerate(queries):
            want = wanted(oracle, name, k)
            got = ctx.archive_queue(now, window)
            assert got.dtype == np.int32 and np.array_equal(got, want), (name, k, got.size, want.size)
            if packed:
                check_pack(pie, ctx, user, want, want, (name, k))
        same_scan(oracle, ctx, (start, end, user, disc), U, name)
    if packed:
        check_sharded_pack(pie, oracle, name)


# ------------------------------------------------------------------------------------------------ state around the chain
def raw_archive(ctx, now, window, cap):
    out, q = np.full(max(cap, 1), SENT, np.int32), C.c_size_t(12345)
    rc = ctx._lib.pie_archive_queue(ctx._ctx, int(now), int(window), out.ctypes.data_as(C.c_void_p), int(cap), C.byref(q))
    return rc, q.value, out[:cap]


def info_code(pie, ctx):
    kind = C.c_int32(7)
    rc = ctx._lib.pie_queue_info(ctx._ctx, C.byref(kind), None, None)
    return rc, kind.value


def test_capacity_and_repeat(pie, oracle):
    start, end, user, disc, U, queries, _ = case("group_sizes")
    want = wanted(oracle, "group_sizes", 0)
    with pie.PieScan(0) as ctx:
        ctx.load_columns(start, end, user, disc, U)
        for cap in (want.size - 1, 0):
            rc, q, out = raw_archive(ctx, *queries[0], cap)
            assert rc == PIE_E_CAPACITY and q == want.size and np.all(out == SENT), (cap, rc, q)
            assert info_code(pie, ctx) == (PIE_E_STATE, 0), "a refused queue is not held"
        rc, q, out = raw_archive(ctx, *queries[0], want.size)
        assert rc == 0 and q == want.size and np.array_equal(out, want)
        assert ctx.queue_info() == (2, want.size, len(AC.GROUP_SIZES))


def grown(cols, more):
    return tuple(np.concatenate([a, np.asarray(b, a.dtype)]) for a, b in zip(cols, more))


@pytest.mark.parametrize("u0,u1", ((60, 70), (64, 65), (AC.LDS_USERS, AC.LDS_USERS + 1)))
def test_after_appends_that_add_users(pie, oracle, u0, u1):
    """n_users crosses a multiple of 64 (the per-group scratch is carved in units of 64) and the LDS limit of the bitmap; the new
    last user qualifies, and so does user u0 - 1"""
    n = 5001
    user = (np.arange(n) % 50).astype(np.int32)
    user[7::100] = u0 - 1
    old = np.isin(user, (3, u0 - 1))
    cols = AC.make("state", "append", user, u0, [{3, u0 - 1}], old=old)[:4]
    with pie.PieScan(0) as ctx:
        ctx.load_columns(*cols, u0)
        archive(oracle, ctx, cols, u0, tag="before")
        k = 11
        more = (np.full(k, AC.LIMIT - 1), np.full(k, AC.T0 + AC.DAY), np.where(np.arange(k) % 2 == 0, u1 - 1, 4), np.zeros(k))
        ctx.append_rows(*grown(tuple(np.zeros(0, a.dtype) for a in cols), more), u1)
        cols = grown(cols, more)
        want = archive(oracle, ctx, cols, u1, tag="after the append")
        assert {3, 4, u0 - 1, u1 - 1} == set(cols[2][want].tolist())
        more = (np.full(3, AC.LIMIT + 5), np.full(3, AC.T0 + AC.DAY), np.full(3, 5), np.zeros(3))   # fits the grown table
        ctx.append_rows(*grown(tuple(np.zeros(0, a.dtype) for a in cols), more), u1)
        cols = grown(cols, more)
        archive(oracle, ctx, cols, u1, tag="after a second append")
        same_scan(oracle, ctx, cols, u1, "appends")


def test_after_tombstones_delete_user_and_compaction(pie, oracle):
    start, end, user, disc, U, queries, props = case("group_sizes")
    end = end.copy()
    with pie.PieScan(0) as ctx:
        ctx.load_columns(start, end, user, disc, U)
        archive(oracle, ctx, (start, end, user), U, tag="loaded")
        # the only old row of groups 1 and 4 becomes a tombstone: they leave the queue; group 2 loses its first row
        rows = np.array([np.nonzero(user == 1)[0][-1], np.nonzero(user == 4)[0][-1], np.nonzero(user == 2)[0][0]], np.int32)
        ctx.set_end(rows, np.full(3, INT64_MIN, np.int64))
        end[rows] = INT64_MIN
        want = archive(oracle, ctx, (start, end, user), U, tag="tombstones")
        assert set(user[want].tolist()) == {0, 2, 3, 5, 6, 7}
        gone = ctx.delete_user(7)
        assert np.array_equal(gone, np.nonzero(user == 7)[0])
        end[gone] = INT64_MIN
        want = archive(oracle, ctx, (start, end, user), U, tag="delete_user")
        assert set(user[want].tolist()) == {0, 2, 3, 5, 6}
        keep = end != INT64_MIN
        assert ctx.compact_rows() == np.count_nonzero(keep)
        cols = (start[keep], end[keep], user[keep], disc[keep])
        archive(oracle, ctx, cols, U, tag="compacted")
        same_scan(oracle, ctx, cols, U, "compacted")


@pytest.mark.parametrize("name", ("group_sizes", "order-late", "tombstones-mixed", "placement-4097-tail_decides"))
def test_with_hot_index_and_ordered_run(pie, oracle, name):
    start, end, user, disc, U, queries, _ = case(name)
    ctx = ctx_with_env(pie, 1, 1)
    try:
        ctx.set_ordered_run(2)
        ctx.load_columns(start, end, user, disc, U)
        ctx.set_disciplines(ALL, D)
        ctx.scan_batch([(AC.T0 + q, INT64_MIN, 0xFFFFFFFF) for q in range(16)])   # builds the hot index / the ordered run
        for k, (now, window) in enumerate(queries):
            got = ctx.archive_queue(now, window)
            assert got.dtype == np.int32 and np.array_equal(got, wanted(oracle, name, k)), (name, k)
        same_scan(oracle, ctx, (start, end, user, disc), U, name)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ what forgets the queue
def test_table_changes_forget_the_queue(pie, oracle):
    """include/pie_scan.h: a table change since the queue call forgets the queue.  pie_set_end and pie_append_rows (whether the
    table had to grow or the rows went in place) are such changes: pie_queue_info answers PIE_E_STATE and kind 0 after each, and
    pie_queue_pack_device writes nothing."""
    start, end, user, disc, U, queries, _ = case("order-late")
    cols = (start, end.copy(), user, disc)
    one = (np.array([AC.LIMIT - 3], np.int64), np.array([AC.T0 + AC.DAY], np.int64), np.array([0], np.int32), np.array([1], np.int32))
    with pie.PieScan(0) as ctx:
        ctx.load_columns(*cols, U)

        def held():
            want = archive(oracle, ctx, cols, U, tag="held")
            assert ctx.queue_info()[:2] == (2, want.size)

        def forgotten(tag):
            assert info_code(pie, ctx) == (PIE_E_STATE, 0), tag
            buf = torch.full((64,), SENT, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            with pytest.raises(pie.PieError) as ei:
                ctx.queue_pack_device(buf.data_ptr(), 10 ** 6, 10 ** 6)
            ctx.synchronize()
            assert ei.value.code == PIE_E_STATE and bool(torch.all(buf == SENT)), tag

        held()
        ctx.set_end(np.array([700], np.int32), np.array([INT64_MIN], np.int64))   # group 2's only old row
        cols[1][700] = INT64_MIN
        forgotten("pie_set_end")
        held()
        for tag in ("an append that grows the table", "an append in place", "another append in place"):
            ctx.append_rows(*one, U)
            cols = grown(cols, one)
            forgotten(tag)
            held()
        ctx.load_columns(*cols, U)   # a load into the capacity the table already has
        forgotten("pie_load_columns")
        held()
