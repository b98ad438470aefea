"""GPU, one context: a wide batch that writes its own exchange message (pie_scan_wide_begin_union /
pie_scan_wide_finish_packed).  The message sits in mapped host memory and is read WITHOUT a synchronize call once finish said
ready = 1: it equals the numpy union built from the oracle's per-query scans, what pie_batch_pack_union_wide_device writes,
and its padding words equal Mu.  Also: a cap below Mu (rows cut, nothing written past the message), batches that keep no
union (ready = 0, Mu = -1, per-query results exact), and wide-union / ordinary batches interleaved on 1 and 3 lanes."""
import numpy as np
import pytest

from test_gpu_wide import ALL, SEED, assert_same, mixed_queries, oracle_answers, wide_union_from

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_WORD = -1234567


def msg_words(u_pad, cap, words):
    return u_pad + 2 + cap * (1 + 2 * words)


def expected_message(U, u_pad, cap, words, union):
    """the message the union (uoff int64[U + 1], rows, masks[Mu, words]) makes; positions the kernel leaves alone are None-masked
    by the caller through `written`"""
    uoff, rows, masks = union
    mu = int(rows.size)
    k = min(mu, cap)
    msg = np.zeros(msg_words(u_pad, cap, words), np.int32)
    written = np.zeros(msg.size, bool)
    msg[: U + 1] = uoff.astype(np.int32)
    msg[U + 1: u_pad + 2] = mu
    written[: u_pad + 2] = True
    msg[u_pad + 2: u_pad + 2 + k] = rows[:k]
    written[u_pad + 2: u_pad + 2 + k] = True
    base = u_pad + 2 + cap
    msg[base: base + k * 2 * words] = np.ascontiguousarray(masks[:k]).reshape(-1).view(np.int32)
    written[base: base + k * 2 * words] = True
    return msg, written


class HostMsg:
    """mapped host memory for one message plus guard words behind it"""

    def __init__(self, ctx, n_words):
        self.ctx, self.n = ctx, n_words
        self.h, self.d, self.addr = ctx.host_alloc(n_words + GUARD)
        self.h[:] = GUARD_WORD

    def free(self):
        self.ctx.host_free(self.addr)


@pytest.mark.parametrize("n,U,D", [(100003, 4999, 32), (1 << 20, 10 ** 4, 32)])
def test_wide_message_written_by_the_tail(gpu_ctx, oracle, n, U, D):
    from sph_pie_amd.binding import split_wide_message
    cols = oracle.gen(SEED, n, 0, n, U, D, 0)
    gpu_ctx.load_columns(*cols, U)
    gpu_ctx.set_disciplines(ALL, D)
    gpu_ctx.scan_wide_begin(mixed_queries(oracle, 512))   # warm-up: grows the union slot capacity
    gpu_ctx.scan_wide_finish()
    for nq in (65, 300, 512):
        queries = mixed_queries(oracle, nq)
        want = oracle_answers(oracle, cols, (n, U, D, 0), U, D, queries)
        words = (nq + 63) // 64
        union = wide_union_from(cols, U, want)
        mu = int(union[1].size)
        # a condition the inputs meet, stated before the GPU is asked: no user's union exceeds 64 rows, so the batch keeps its union
        assert int(np.diff(union[0]).max()) <= 64
        u_pad = U + 5
        for cap in (mu + 9, mu, max(mu // 3, 1)):
            L = msg_words(u_pad, cap, words)
            a, b = HostMsg(gpu_ctx, L), HostMsg(gpu_ctx, L)
            try:
                gpu_ctx.scan_wide_begin_union(queries, a.d, u_pad, cap)
                ms, ready = gpu_ctx.scan_wide_finish_packed()
                assert ready is True, (nq, cap)
                got = a.h.copy()                          # no synchronize: the message is complete when finish returns
                assert ms == [int(w[2].size) for w in want]
                exp, written = expected_message(U, u_pad, cap, words, union)
                assert np.array_equal(got[:L][written], exp[written]), (nq, cap)
                assert np.all(got[:L][~written] == GUARD_WORD), "words of cut rows were written"
                assert np.all(got[L:] == GUARD_WORD), "written past u_pad + 2 + cap * (1 + 2 * words)"
                assert np.all(got[U: u_pad + 2] == mu), "padding words / Mu word"
                # what the separate pack launch writes into a second buffer
                gpu_ctx.batch_pack_union_wide_device(b.d, u_pad, cap)
                gpu_ctx.synchronize()
                assert np.array_equal(b.h[:L][written], got[:L][written]), (nq, cap)
                assert np.all(b.h[L:] == GUARD_WORD)
                # and through the helper
                s_uoff, s_mu, s_rows, s_masks = split_wide_message(got[:L], u_pad, cap, words)
                k = min(mu, cap)
                assert s_mu == mu and np.array_equal(s_rows, union[1][:k]) and np.array_equal(s_masks, union[2][:k])
                assert np.array_equal(s_uoff[: U + 1], union[0].astype(np.int32))
                # the batch's other readers are as after pie_scan_wide_begin
                assert_same(gpu_ctx.batch_read_results(nq - 1), want[nq - 1], "nq=%d" % nq)
            finally:
                a.free()
                b.free()


def test_wide_message_without_a_union(gpu_ctx, oracle):
    """the 7-user table whose buckets outgrow the union slots, and a table on the ordered run: ready = 0, and once the context's
    stream has passed the header says Mu = -1, uoff all -1; the per-query results are exact"""
    D = 32
    n, U = 300000, 7
    cols = oracle.gen(SEED, n, 0, n, U, D, 0)
    gpu_ctx.load_columns(*cols, U)
    gpu_ctx.set_disciplines(ALL, D)
    queries = mixed_queries(oracle, 300)
    want = oracle_answers(oracle, cols, ("fb", n, U), U, D, queries)
    assert max(int(w[0].max()) for w in want) > 64
    words, u_pad, cap = 5, U + 2, 1000
    L = msg_words(u_pad, cap, words)
    a = HostMsg(gpu_ctx, L)
    try:
        for _ in range(2):
            gpu_ctx.scan_wide_begin_union(queries, a.d, u_pad, cap)
            ms, ready = gpu_ctx.scan_wide_finish_packed()
            assert ready is False
            assert ms == [int(w[2].size) for w in want]
            gpu_ctx.synchronize()
            assert np.all(a.h[: u_pad + 2] == -1)
            assert np.all(a.h[L:] == GUARD_WORD)
            for q in (0, 1, 100, 299):
                assert_same(gpu_ctx.batch_read_results(q), want[q], "few users, query %d" % q)
            assert gpu_ctx.batch_read_union_wide() is None
    finally:
        a.free()
    # the ordered run
    n, U = 1 << 20, 5000
    cols = oracle.gen(SEED, n, 0, n, U, D, 0)
    gpu_ctx.load_columns(*cols, U)
    gpu_ctx.set_ordered_run(2)
    words, u_pad, cap = 2, U, 4096
    L = msg_words(u_pad, cap, words)
    a = HostMsg(gpu_ctx, L)
    try:
        queries = mixed_queries(oracle, 100)
        gpu_ctx.set_disciplines(queries[0][2], D)
        gpu_ctx.scan(queries[0][0], queries[0][1])          # builds the run: the table's batches now take it
        assert gpu_ctx.stats()["k1_variant"] & 0x2000
        gpu_ctx.set_disciplines(ALL, D)
        want = oracle_answers(oracle, cols, ("ord", n, U), U, D, queries)
        gpu_ctx.scan_wide_begin_union(queries, a.d, u_pad, cap)
        ms, ready = gpu_ctx.scan_wide_finish_packed()
        assert ready is False and ms == [int(w[2].size) for w in want]
        gpu_ctx.synchronize()
        assert np.all(a.h[: u_pad + 2] == -1) and np.all(a.h[L:] == GUARD_WORD)
        for q in (0, 50, 99):
            assert_same(gpu_ctx.batch_read_results(q), want[q], "ordered run, query %d" % q)
    finally:
        gpu_ctx.set_ordered_run(1)
        a.free()


def test_wide_finish_also_finishes_a_union_batch(gpu_ctx, oracle):
    """pie_scan_wide_finish on a batch begun with pie_scan_wide_begin_union: the message is in order on the context's stream"""
    n, U, D = 100003, 4999, 32
    cols = oracle.gen(SEED, n, 0, n, U, D, 0)
    gpu_ctx.load_columns(*cols, U)
    gpu_ctx.set_disciplines(ALL, D)
    gpu_ctx.scan_wide_begin(mixed_queries(oracle, 512))
    gpu_ctx.scan_wide_finish()
    queries = mixed_queries(oracle, 130)
    want = oracle_answers(oracle, cols, (n, U, D, 0), U, D, queries)
    union = wide_union_from(cols, U, want)
    words, u_pad, cap = 3, U, int(union[1].size) + 1
    L = msg_words(u_pad, cap, words)
    a = HostMsg(gpu_ctx, L)
    try:
        gpu_ctx.scan_wide_begin_union(queries, a.d, u_pad, cap)
        assert gpu_ctx.scan_wide_finish() == [int(w[2].size) for w in want]
        gpu_ctx.synchronize()
        exp, written = expected_message(U, u_pad, cap, words, union)
        assert np.array_equal(a.h[:L][written], exp[written]) and np.all(a.h[L:] == GUARD_WORD)
    finally:
        a.free()


@pytest.mark.parametrize("lanes", [1, 3])
def test_wide_union_and_ordinary_batches_interleaved(gpu_ctx, oracle, lanes):
    """wide-union and ordinary batches, three in flight per lane: finish order is begin order and every message is exact"""
    n, U, D = 1 << 20, 10 ** 4, 32
    cols = oracle.gen(SEED, n, 0, n, U, D, 0)
    gpu_ctx.load_columns(*cols, U)
    gpu_ctx.set_disciplines(ALL, D)
    gpu_ctx.set_batch_lanes(lanes)
    bufs = []
    try:
        all_q = mixed_queries(oracle, 512)
        want = oracle_answers(oracle, cols, (n, U, D, 0), U, D, all_q)
        gpu_ctx.scan_wide_begin(all_q)                      # warm-up
        gpu_ctx.scan_wide_finish()
        plan = []   # (wide, first query, n_q)
        for i in range(3 * lanes + 3):
            plan.append((True, (37 * i) % 200, 200 + 13 * i) if i % 2 == 0 else (False, (11 * i) % 300, 16 + i))
        unions = {}
        for i, (wide, q0, nq) in enumerate(plan):
            if wide:
                un = wide_union_from(cols, U, want[q0:q0 + nq])
                assert int(np.diff(un[0]).max()) <= 64
                cap = int(un[1].size) + 3
                unions[i] = (un, cap, HostMsg(gpu_ctx, msg_words(U + 1, cap, (nq + 63) // 64)))
                bufs.append(unions[i][2])
        begun = done = 0
        while done < len(plan):
            while begun < len(plan) and gpu_ctx.batch_room() > 0 and begun - done < 3 * lanes:
                wide, q0, nq = plan[begun]
                if wide:
                    un, cap, hm = unions[begun]
                    gpu_ctx.scan_wide_begin_union(all_q[q0:q0 + nq], hm.d, U + 1, cap)
                else:
                    gpu_ctx.scan_batch_begin(all_q[q0:q0 + nq])
                begun += 1
            assert begun - done == min(3 * lanes, len(plan) - done) or gpu_ctx.batch_room() == 0
            wide, q0, nq = plan[done]
            ms, ready = gpu_ctx.scan_wide_finish_packed()
            assert ms == [int(w[2].size) for w in want[q0:q0 + nq]], done      # begin order
            assert ready is True, done
            if wide:
                un, cap, hm = unions[done]
                words = (nq + 63) // 64
                L = msg_words(U + 1, cap, words)
                got = hm.h.copy()
                exp, written = expected_message(U, U + 1, cap, words, un)
                assert np.array_equal(got[:L][written], exp[written]), done
                assert np.all(got[:L][~written] == GUARD_WORD) and np.all(got[L:] == GUARD_WORD), done
            done += 1
    finally:
        gpu_ctx.set_batch_lanes(0)
        gpu_ctx.synchronize()
        for hm in bufs:
            hm.free()


def test_wide_begin_union_arguments(gpu_ctx, oracle):
    from sph_pie_amd import PieError
    n, U, D = 100003, 97, 32
    cols = oracle.gen(SEED, n, 0, n, U, D, 0)
    gpu_ctx.load_columns(*cols, U)
    gpu_ctx.set_disciplines(ALL, D)
    a = HostMsg(gpu_ctx, msg_words(U, 16, 1))
    try:
        for args in ((mixed_queries(oracle, 4), None, U, 16), (mixed_queries(oracle, 4), a.d, U - 1, 16), (mixed_queries(oracle, 513), a.d, U, 16)):
            with pytest.raises(PieError) as ei:
                gpu_ctx.scan_wide_begin_union(*args)
            assert ei.value.code == -1
        assert np.all(a.h == GUARD_WORD)
    finally:
        a.free()
