"""GPU: wide batches (pie_scan_wide_*: up to 512 queries, one table pass) against the CPU oracle — every query's
(counts, offsets, idx), the wide union word for word, its exchange message, the queries that fall back, the ordered run,
pipelining with ordinary batches on 1..4 lanes, and the argument / state errors.  Through the C ABI (ctypes)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT64_MIN = -(2 ** 63)
ALL = 2 ** 64 - 1
DAY = 86400 * 1000
HOUR = 3600 * 1000
SEED = 0x5EED5EED
E_INVAL, E_CAPACITY, E_STATE = -1, -5, -6


def assert_same(got, want, tag=""):
    for name, a, b in zip(("counts", "offsets", "idx"), got, want):
        assert a.dtype == b.dtype, (tag, name)
        assert np.array_equal(a, b), (tag, name)


def mixed_queries(oracle, k):
    """as tests/test_gpu_batch.py: distinct now / cutoff / mask per request"""
    t0 = oracle.T0_MS
    masks = [0x5555555555555555, 0xAAAAAAAAAAAAAAAA, ALL, 0x00000000FFFF0000, 0x1, 0x8000000000000001]
    return [(t0 - 6 * HOUR - 977 * i - (i % 3) * HOUR, t0 - (61 + i % 4) * DAY - 13 * i, masks[i % len(masks)]) for i in range(k)]


_answers = {}


def oracle_answers(oracle, cols, key, U, D, queries):
    """oracle answers, cached per table (the queries of a smaller batch are a prefix of the larger one's)"""
    s, e, u, d = cols
    lim = ALL if D >= 64 else (1 << D) - 1
    have = _answers.setdefault(key, {})
    out = []
    for q in queries:
        if q not in have:
            now, cutoff, mask = q
            have[q] = oracle.scan(s, e, u, d, U, now, cutoff, mask & lim)
        out.append(have[q])
    return out


def wide_union_from(cols, U, answers):
    """numpy restatement of the wide union: per user the rows any query selects, in (start, row) order, ceil(Q / 64) mask words"""
    words = (len(answers) + 63) // 64
    sel = {}
    for q, (_, _, idx) in enumerate(answers):
        for r in idx:
            sel[int(r)] = sel.get(int(r), 0) | (1 << q)
    s, user = cols[0], cols[2]
    rows = np.array(sorted(sel, key=lambda r: (int(user[r]), int(s[r]), r)), np.int64)
    uoff = np.zeros(U + 1, np.int64)
    if rows.size:
        np.add.at(uoff, user[rows].astype(np.int64) + 1, 1)
    masks = np.array([[(sel[int(r)] >> (64 * w)) & ALL for w in range(words)] for r in rows], np.uint64).reshape(rows.size, words)
    return np.cumsum(uoff), rows.astype(np.int32), masks


SHAPES = [
    (1, 1, 1, 0), (65, 3, 2, 0), (4097, 9, 7, 1), (100003, 97, 32, 0), (1 << 20, 10 ** 4, 32, 0), (3000017, 20011, 64, 1),
    (1 << 20, 10 ** 4, 32, 4), (3000017, 20011, 64, 5),
]


@pytest.mark.parametrize("n,U,D,flags", SHAPES)
def test_wide_equals_separate_scans(gpu_ctx, oracle, n, U, D, flags):
    cols = oracle.gen(SEED, n, 0, n, U, D, flags)
    gpu_ctx.load_columns(*cols, U)
    gpu_ctx.set_disciplines(ALL, D)
    key = (n, U, D, flags)
    for nq in (1, 63, 64, 65, 200, 511, 512):
        queries = mixed_queries(oracle, nq)
        want = oracle_answers(oracle, cols, key, U, D, queries)
        gpu_ctx.scan_wide_begin(queries)
        ms = gpu_ctx.scan_wide_finish()
        assert ms == [int(w[2].size) for w in want], nq
        # every query's lists for the small batches, a spread of them (the high mask words included) for the large ones
        qs = range(nq) if nq <= 65 else sorted({0, 63, 64, 65, 127, 128, nq // 2, nq - 2, nq - 1} | set(range(0, nq, 37)))
        for q in qs:
            assert_same(gpu_ctx.batch_read_results(q), want[q], "nq=%d query %d" % (nq, q))


@pytest.mark.parametrize("n,U,D,flags", [(65, 3, 2, 0), (100003, 4999, 32, 0), (1 << 20, 10 ** 4, 32, 0), (3000017, 20011, 64, 5)])
def test_wide_union(gpu_ctx, oracle, n, U, D, flags):
    """the wide union against its numpy restatement; Feed(q, u) from it for every q; the exchange message agrees with it.
    On these tables no user's union outgrows 64 slots: after a warm-up batch (which grows the slot capacity) every batch keeps
    its union."""
    cols = oracle.gen(SEED, n, 0, n, U, D, flags)
    gpu_ctx.load_columns(*cols, U)
    gpu_ctx.set_disciplines(ALL, D)
    gpu_ctx.scan_wide_begin(mixed_queries(oracle, 512))
    gpu_ctx.scan_wide_finish()
    for nq in (65, 300, 512):
        queries = mixed_queries(oracle, nq)
        want = oracle_answers(oracle, cols, (n, U, D, flags), U, D, queries)
        gpu_ctx.scan_wide_begin(queries)
        gpu_ctx.scan_wide_finish()
        un = gpu_ctx.batch_read_union_wide()
        assert un is not None, nq
        uoff, rows, masks = un
        w_uoff, w_rows, w_masks = wide_union_from(cols, U, want)
        assert np.array_equal(uoff, w_uoff) and np.array_equal(rows, w_rows) and np.array_equal(masks, w_masks), nq
        words = masks.shape[1]
        assert words == (nq + 63) // 64
        if nq % 64:
            assert not np.any(masks[:, -1] >> np.uint64(nq % 64)), "mask bits above n_q"
        # Feed(q, u) rebuilt from the union equals the oracle's, for every q
        row_user = np.repeat(np.arange(U), np.diff(uoff))
        for q in range(nq):
            bit = ((masks[:, q // 64] >> np.uint64(q % 64)) & np.uint64(1)).astype(bool)
            c, off, idx = want[q]
            assert np.array_equal(rows[bit], idx), q
            assert np.array_equal(np.bincount(row_user[bit], minlength=U), c), q
        rng = np.random.default_rng(nq)
        for u in [0, U - 1] + [int(x) for x in rng.integers(0, U, 4)]:
            for q in (0, nq - 1, nq // 2):
                c, off, idx = want[q]
                assert np.array_equal(gpu_ctx.batch_read_user_feed(q, u), idx[off[u]:off[u + 1]]), (q, u)
        # the message
        mu = rows.size
        cap = mu + 5
        u_pad = U + 3
        msg_h, msg_d, msg_addr = gpu_ctx.host_alloc(u_pad + 2 + cap * (1 + 2 * words))
        try:
            gpu_ctx.batch_pack_union_wide_device(msg_d, u_pad, cap)
            gpu_ctx.synchronize()
            assert np.array_equal(msg_h[: U + 1], uoff.astype(np.int32))
            assert np.all(msg_h[U + 1: u_pad + 2] == mu)
            assert np.array_equal(msg_h[u_pad + 2: u_pad + 2 + mu], rows)
            got_masks = msg_h[u_pad + 2 + cap: u_pad + 2 + cap + mu * 2 * words].copy().view(np.uint64).reshape(mu, words)
            assert np.array_equal(got_masks, masks)
        finally:
            gpu_ctx.host_free(msg_addr)


def want_x_size(oracle, cols, U, D, x):
    return int(oracle.scan(*cols, U, *x)[2].size)


def test_wide_fallbacks(gpu_ctx, oracle):
    """a 300-query batch holding dense, everything and nothing queries; a few-users table whose buckets overflow; a table whose
    batches take the ordered run: every query exact, the union readers PIE_E_STATE"""
    from sph_pie_amd import PieError
    n, U, D = 1 << 20, 5000, 32
    cols = oracle.gen(SEED, n, 0, n, U, D, 0)
    gpu_ctx.load_columns(*cols, U)
    gpu_ctx.set_disciplines(ALL, D)
    t0 = oracle.T0_MS
    queries = mixed_queries(oracle, 300)
    queries[7] = (t0 - 100 * DAY, t0 - 61 * DAY, 0xAAAAAAAAAAAAAAAA)   # dense
    queries[150] = (INT64_MIN, INT64_MIN, ALL)                        # everything
    queries[299] = (2 ** 62, INT64_MIN, ALL)                          # nothing
    want = oracle_answers(oracle, cols, ("fb", n, U), U, D, queries)
    gpu_ctx.scan_wide_begin(queries)
    assert gpu_ctx.scan_wide_finish() == [int(w[2].size) for w in want]
    for q in (0, 7, 64, 150, 200, 299):
        assert_same(gpu_ctx.batch_read_results(q), want[q], "query %d" % q)
    assert gpu_ctx.batch_read_union_wide() is None
    with pytest.raises(PieError) as ei:
        gpu_ctx.batch_union_wide_device_ptrs()
    assert ei.value.code == E_STATE
    for q, u in ((0, 3), (7, 11), (150, 0), (299, 5)):
        c, off, idx = want[q]
        assert np.array_equal(gpu_ctx.batch_read_user_feed(q, u), idx[off[u]:off[u + 1]]), (q, u)
    # the lists of the fallback queries were built at finish: reading them while the caller has a single scan of its own in
    # flight neither takes that scan's result nor leaves a scan of its own behind
    gpu_ctx.scan_wide_begin(queries)
    gpu_ctx.scan_wide_finish()
    x = (t0 - 5 * HOUR, t0 - 30 * DAY, ALL)
    gpu_ctx.scan_begin(x[0], x[1])
    for q in (7, 150, 299, 3):
        assert_same(gpu_ctx.batch_read_results(q), want[q], "interleaved, query %d" % q)
    assert gpu_ctx.scan_finish() == want_x_size(oracle, cols, U, D, x)
    assert_same(gpu_ctx.read_results(), oracle.scan(*cols, U, *x), "the caller's own scan")
    with pytest.raises(PieError) as ei:
        gpu_ctx.scan_finish()
    assert ei.value.code == E_STATE                                     # nothing else was left in flight
    # few users: buckets outgrow the union slots -> every query reruns on the general path
    n, U = 300000, 7
    cols = oracle.gen(SEED, n, 0, n, U, D, 0)
    gpu_ctx.load_columns(*cols, U)
    queries = mixed_queries(oracle, 300)
    want = oracle_answers(oracle, cols, ("fb", n, U), U, D, queries)
    assert max(int(w[0].max()) for w in want) > 64
    gpu_ctx.scan_wide_begin(queries)
    assert gpu_ctx.scan_wide_finish() == [int(w[2].size) for w in want]
    for q in (0, 1, 100, 299):
        assert_same(gpu_ctx.batch_read_results(q), want[q], "few users, query %d" % q)
    assert gpu_ctx.batch_read_union_wide() is None
    # the ordered run
    n, U = 1 << 20, 5000
    cols = oracle.gen(SEED, n, 0, n, U, D, 0)
    gpu_ctx.load_columns(*cols, U)
    gpu_ctx.set_ordered_run(2)
    try:
        queries = mixed_queries(oracle, 100)
        gpu_ctx.set_disciplines(queries[0][2], D)
        gpu_ctx.scan(queries[0][0], queries[0][1])          # builds the run: the table's batches now take it
        assert gpu_ctx.stats()["k1_variant"] & 0x2000
        gpu_ctx.set_disciplines(ALL, D)
        want = oracle_answers(oracle, cols, ("ord", n, U), U, D, queries)
        gpu_ctx.scan_wide_begin(queries)
        assert gpu_ctx.scan_wide_finish() == [int(w[2].size) for w in want]
        for q in (0, 50, 99):
            assert_same(gpu_ctx.batch_read_results(q), want[q], "ordered run, query %d" % q)
        assert gpu_ctx.batch_read_union_wide() is None
    finally:
        gpu_ctx.set_ordered_run(1)


@pytest.mark.parametrize("lanes", [1, 2, 3, 4])
def test_wide_and_ordinary_batches_pipelined(gpu_ctx, oracle, lanes):
    """wide and ordinary batches interleaved, up to three per lane in flight: finish returns begin order; pie_scan_batch_finish
    on a wide oldest batch is PIE_E_STATE and leaves it in flight"""
    from sph_pie_amd import PieError
    n, U, D = 1 << 20, 10 ** 4, 32
    cols = oracle.gen(SEED, n, 0, n, U, D, 0)
    gpu_ctx.load_columns(*cols, U)
    gpu_ctx.set_disciplines(ALL, D)
    gpu_ctx.set_batch_lanes(lanes)
    try:
        all_q = mixed_queries(oracle, 512)
        want = oracle_answers(oracle, cols, (n, U, D, 0), U, D, all_q)
        plan = []   # (wide, first query, n_q)
        for i in range(3 * lanes + 2):
            plan.append((True, (37 * i) % 200, 200 + 13 * i) if i % 2 == 0 else (False, (11 * i) % 300, 16 + i))
        begun = done = 0
        while done < len(plan):
            while begun < len(plan) and gpu_ctx.batch_room() > 0:
                wide, q0, nq = plan[begun]
                qs = all_q[q0:q0 + nq]
                (gpu_ctx.scan_wide_begin if wide else gpu_ctx.scan_batch_begin)(qs)
                begun += 1
            wide, q0, nq = plan[done]
            if wide:
                with pytest.raises(PieError) as ei:
                    gpu_ctx.scan_batch_finish()
                assert ei.value.code == E_STATE
            ms = gpu_ctx.scan_wide_finish()
            assert ms == [int(w[2].size) for w in want[q0:q0 + nq]], done
            assert_same(gpu_ctx.batch_read_results(nq - 1), want[q0 + nq - 1], "batch %d" % done)
            done += 1
    finally:
        gpu_ctx.set_batch_lanes(0)


def test_wide_limits(pie, oracle):
    from sph_pie_amd import PieError
    n, U, D = 100003, 97, 32
    cols = oracle.gen(SEED, n, 0, n, U, D, 0)
    with pie.PieScan(0) as ctx:
        ctx.load_columns(*cols, U)
        ctx.set_disciplines(ALL, D)
        queries = mixed_queries(oracle, 100)
        ctx.scan_batch(queries[:16])
        ws = ctx.table_info()["workspace_bytes"]
        for bad in ([], mixed_queries(oracle, 513)):
            with pytest.raises(PieError) as ei:
                ctx.scan_wide_begin(bad)
            assert ei.value.code == E_INVAL
        assert ctx.table_info()["workspace_bytes"] == ws
        ctx.scan_wide_begin(queries)
        assert ctx.table_info()["workspace_bytes"] > ws                  # the wide state, reported from its first batch on
        lib = ctx._lib
        m = (C.c_size_t * 512)()
        nq = C.c_int(0)
        assert lib.pie_scan_wide_finish(ctx._ctx, m, 99, C.byref(nq)) == E_CAPACITY and nq.value == 100
        assert lib.pie_scan_batch_finish(ctx._ctx, m) == E_STATE     # the wide batch stays the oldest
        assert lib.pie_scan_wide_finish(ctx._ctx, m, 512, C.byref(nq)) == 0 and nq.value == 100
        ctx._batches.pop(0)
        want = oracle_answers(oracle, cols, (n, U, D, 0), U, D, queries)
        assert list(m[:100]) == [int(w[2].size) for w in want]
        # the 32/64-bit union readers refuse a wide batch
        p = C.c_void_p()
        sz = C.c_size_t(0)
        assert lib.pie_batch_union_device_ptrs(ctx._ctx, C.byref(p), C.byref(p), C.byref(p), C.byref(p), C.byref(sz)) == E_STATE
        buf = np.zeros(U + 1, np.int64)
        assert lib.pie_batch_read_union(ctx._ctx, buf.ctypes.data, None, None, 0, C.byref(sz)) == E_STATE
        msg_h, msg_d, msg_addr = ctx.host_alloc(4096)
        try:
            assert lib.pie_batch_pack_union_device(ctx._ctx, msg_d, U + 1, 100) == E_STATE
        finally:
            ctx.host_free(msg_addr)
        # an ordinary batch after it reads as before
        got = ctx.scan_batch(queries[:3])
        for g, w in zip(got, want[:3]):
            assert_same(g, w)
        ctx.batch_read_union()


def test_wide_cfg3_heterogeneous_on_three_lanes(pie, oracle):
    """cfg3 (10^8 rows / 10^5 users / 32 disciplines), one heterogeneous 512-query wide batch on three lanes: every query's M
    against the oracle, 16 sampled queries' full lists against oracle.scan_mt, the union against the union of those lists"""
    n, U, D = 10 ** 8, 10 ** 5, 32
    cols = oracle.gen(SEED, n, 0, n, U, D, 0)
    queries = mixed_queries(oracle, 512)
    with pie.PieScan(0) as ctx:
        ctx.gen_synthetic(SEED, n, 0, n, U, D, 0)
        ctx.set_disciplines(ALL, D)
        ctx.set_batch_lanes(3)
        ctx.scan_wide_begin(queries)         # warm-up: grows the union slot capacity where the first pass outgrows it
        ctx.scan_wide_finish()
        ctx.scan_batch_begin(queries[:64])   # an ordinary batch in flight beside it, on another lane
        ctx.scan_wide_begin(queries)
        ctx.scan_batch_finish()
        ms = ctx.scan_wide_finish()
        out = (np.empty(U, np.int32), np.empty(U + 1, np.int64), np.empty(n, np.int32))
        threads = min(16, os.cpu_count() or 1)
        for q, (now, cutoff, mask) in enumerate(queries):
            assert ms[q] == oracle.scan_mt(*cols, U, now, cutoff, mask & 0xFFFFFFFF, threads, out)[2].size, q
        un = ctx.batch_read_union_wide()
        assert un is not None
        uoff, rows, masks = un
        samples = sorted({0, 1, 63, 64, 65, 127, 128, 255, 256, 300, 383, 384, 447, 448, 510, 511})
        lists = []
        for q in samples:
            now, cutoff, mask = queries[q]
            want = tuple(a.copy() for a in oracle.scan_mt(*cols, U, now, cutoff, mask & 0xFFFFFFFF, threads, out))
            assert_same(ctx.batch_read_results(q), want, "cfg3 query %d" % q)
            lists.append(want[2])
        hit = np.zeros(rows.size, bool)
        for q in samples:
            hit |= ((masks[:, q // 64] >> np.uint64(q % 64)) & np.uint64(1)).astype(bool)
        sel = np.unique(np.concatenate(lists))
        order = np.lexsort((sel, cols[0][sel], cols[2][sel]))
        assert np.array_equal(rows[hit], sel[order].astype(np.int32))


def test_node_feed_service_wide_turn(pie):
    """Node end to end: 300 distinct request groups of one turn through sessionStore + feedService({wide: true}) run in ONE
    device pass, every body byte-identical to the default service's (sph-pie_amd/host/test/gpu_wide_test.js)"""
    import shutil
    import subprocess
    from conftest import REPO
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this machine")
    assert pie.build_napi() is not None, "node headers (node_api.h) not found"
    res = subprocess.run([node, os.path.join(REPO, "sph-pie_amd", "host", "test", "gpu_wide_test.js")], cwd=REPO,
                         env=dict(os.environ, TZ="UTC"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout
    assert "gpu_wide_test ok" in res.stdout
