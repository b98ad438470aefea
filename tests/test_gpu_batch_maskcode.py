"""GPU: the 20-bit mask code of the batched pass.  A selected row's bucket slot holds r | w << 7 | d << 14 (r: queries whose `now`
lies below the row's end, w: queries whose cutoff is <= its start, d: its discipline) and the union tail expands it through the
batch's own tables, which the pass publishes to memory of the batch slot.  Every union here — rows and 64-bit masks, word for
word — is compared with the union put together from SINGLE-query scans of the same queries on a second context: the edges of the
code (r, w in {0, 1, n_q}, ties, disciplines 0 / 31 / 32 / 63) for 1 .. 64 queries with the hot index on and off, batches with
different tables in flight on one lane and on three, queries that fall back, and the tail's three bucket paths.
Tables of 10^6 rows / 5003 users; about 800 single-query reference scans in all."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT64_MIN = -(2 ** 63)
ALL = 2 ** 64 - 1
DAY = 86400 * 1000
HOUR = 3600 * 1000
SEED = 0x5EED5EED
N, U, D = 1_000_003, 5003, 64


def ctx_with(pie, hot):
    old = os.environ.get("PIE_HOT_INDEX")
    os.environ["PIE_HOT_INDEX"] = "1" if hot else "0"
    try:
        return pie.PieScan(0)
    finally:
        if old is None:
            os.environ.pop("PIE_HOT_INDEX")
        else:
            os.environ["PIE_HOT_INDEX"] = old


def queries_of(oracle, k, shift=0, flip=False):
    """k sparse queries, all different in now / cutoff / role mask; the masks of queries 32.. differ from those of 0..31 and
    several differ only in disciplines >= 32.  `shift` (ms) and `flip` give a batch other tables than its neighbours'."""
    t0 = oracle.T0_MS
    masks = [0x5555555555555555, 0xAAAAAAAAAAAAAAAA, ALL, 0x00000000FFFF0000, 0x1, 0x8000000000000001,
             0xFFFFFFFF00000000, 0x0000000180000000, 0x8000000000000000, 0x00000000FFFFFFFF]
    qs = [(t0 - 6 * HOUR - 977 * i - (i % 5) * HOUR - shift, t0 - (61 + i % 4) * DAY - 13 * i - 7 * shift,
           masks[(i + (3 if i >= 32 else 0)) % len(masks)]) for i in range(64)]
    if flip:
        qs = [(qs[i][0], qs[63 - i][1], qs[(i * 7 + 5) % 64][2]) for i in range(64)]
    return qs[:k]


def edge_table(oracle):
    """The seeded corpus with its recent rows moved onto the edges of the 64 queries above: ends just above / on each query's
    `now` (a row live for exactly one query of every prefix of the list, ties), above all of them (r = n_q) and on the smallest
    (r = 0); starts below every cutoff (w = 0), on each cutoff (ties) and above all (w = n_q); disciplines 0, 31, 32, 63."""
    s, e, u, d = [c.copy() for c in oracle.gen(SEED, N, 0, N, U, D, 0)]
    qs = queries_of(oracle, 64)
    nows, cuts = np.array([q[0] for q in qs], np.int64), np.array([q[1] for q in qs], np.int64)
    rng = np.random.default_rng(20)
    rows = np.nonzero(e > oracle.T0_MS - 12 * HOUR)[0]
    rows = rows[rng.random(rows.size) < 0.8]
    k = rows.size
    ends = np.concatenate([nows + 1, nows, [nows.max() + 1, nows.max() + HOUR, nows.min(), nows.min() + 1]])
    starts = np.concatenate([cuts, cuts + 1, cuts - 1, [cuts.min() - 1, cuts.min() - DAY, cuts.max() + 5, oracle.T0_MS - 20 * DAY]])
    e[rows] = ends[rng.integers(0, ends.size, k)]
    s[rows] = starts[rng.integers(0, starts.size, k)]
    d[rows] = np.array([0, 31, 32, 63, 1, 33], np.int32)[rng.integers(0, 6, k)]
    return s, e, u, d


def union_of_singles(ref, cols, queries):
    """The union result from single-query scans on `ref`: (uoff[U+1], rows, masks uint64), rows per user in (start, row) order."""
    mask = np.zeros(cols[0].size, np.uint64)
    for q, (now, cutoff, m) in enumerate(queries):
        ref.set_disciplines(m, D)
        mask[ref.scan(now, cutoff)[2]] |= np.uint64(1 << q)
    rows = np.nonzero(mask)[0]
    rows = rows[np.lexsort((rows, cols[0][rows], cols[2][rows]))]
    uoff = np.zeros(U + 1, np.int64)
    np.add.at(uoff, cols[2][rows].astype(np.int64) + 1, 1)
    return np.cumsum(uoff), rows.astype(np.int32), mask[rows]


def same_union(got, want, tag):
    assert got is not None, (tag, "the batch left no union")
    for name, a, b in zip(("uoff", "rows", "masks"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), (tag, name)


def loaded(pie, cols, hot):
    c = ctx_with(pie, hot)
    c.load_columns(*cols, U)
    c.set_disciplines(ALL, D)
    return c


@pytest.mark.parametrize("hot", [True, False])
def test_code_edges(pie, oracle, hot):
    cols = edge_table(oracle)
    ctx, ref = loaded(pie, cols, hot), loaded(pie, cols, False)
    try:
        for nq in (1, 2, 31, 32, 33, 63, 64):
            qs = queries_of(oracle, nq)
            want = union_of_singles(ref, cols, qs)
            ctx.scan_batch_begin(qs)
            ms = ctx.scan_batch_finish()
            same_union(ctx.batch_read_union(), want, "n_q %d" % nq)
            assert ms == [int(((want[2] >> np.uint64(q)) & np.uint64(1)).sum()) for q in range(nq)]
            # the edges are in the union: rows one query selects and rows many select, bits on both sides of 32, the disciplines
            pop = np.array([bin(int(m)).count("1") for m in want[2]])
            assert (pop == 1).any()
            if nq >= 31:
                assert pop.max() > 8 and set(np.unique(cols[3][want[1]])) >= {0, 31, 32, 63}
            if nq > 32:
                assert (want[2] >> np.uint64(32)).any() and (want[2] & np.uint64(0xFFFFFFFF)).any()
        builds = ctx.table_info()["hot_builds"]
        assert builds >= 1 if hot else builds == 0
    finally:
        ctx.close()
        ref.close()


@pytest.mark.parametrize("hot", [True, False])
def test_batches_with_different_tables_in_flight(pie, oracle, hot):
    """The riding tail of a batch runs in the launch of the next batch's pass on its lane: each must expand its codes with its
    own tables."""
    cols = edge_table(oracle)
    ctx, ref = loaded(pie, cols, hot), loaded(pie, cols, False)
    try:
        for lanes, n_batches in ((1, 2), (3, 9)):
            ctx.set_batch_lanes(lanes)
            batches = [queries_of(oracle, (64, 40, 33, 17)[b % 4], shift=b * 1800 * 1000, flip=b % 2 == 1) for b in range(n_batches)]
            wants = [union_of_singles(ref, cols, qs) for qs in batches]
            assert all(not np.array_equal(wants[0][2], w[2]) for w in wants[1:])
            for qs in batches:
                ctx.scan_batch_begin(qs)
            for b in range(n_batches):
                ctx.scan_batch_finish()
                same_union(ctx.batch_read_union(), wants[b], "%d lanes, batch %d of %d" % (lanes, b, n_batches))
    finally:
        ctx.close()
        ref.close()


def test_dense_queries_keep_the_other_bits_in_place(pie, oracle):
    """Dense queries fall back and are not in the tables; the bits of the others stay at their query indices."""
    cols = edge_table(oracle)
    ctx, ref = loaded(pie, cols, True), loaded(pie, cols, False)
    try:
        t0 = oracle.T0_MS
        qs = queries_of(oracle, 40)
        dense = {3: (t0 - 100 * DAY, t0 - 110 * DAY, 0xAAAAAAAAAAAAAAAA), 35: (t0 - 90 * DAY, INT64_MIN, ALL)}
        for k, q in dense.items():
            qs[k] = q
        got = ctx.scan_batch(qs)
        for q, (now, cutoff, m) in enumerate(qs):
            ref.set_disciplines(m, D)
            for name, a, b in zip(("counts", "offsets", "idx"), got[q], ref.scan(now, cutoff)):
                assert a.dtype == b.dtype and np.array_equal(a, b), (q, name)
        assert ctx.batch_read_union() is None   # (queries fell back: the union does not hold the whole batch)
    finally:
        ctx.close()
        ref.close()


@pytest.mark.parametrize("nq", [64, 20])
def test_all_three_bucket_paths_expand_the_code(pie, oracle, nq):
    """A few heavy users: union buckets of 1..8 rows (ordered in registers), 9..16 (rows of 16 lanes) and 17..64 (the whole wave)
    once the slot capacity has grown."""
    s, e, u, d = edge_table(oracle)
    rng = np.random.default_rng(3)
    recent = np.nonzero(e > oracle.T0_MS - 12 * HOUR)[0]
    sizes = list(range(1, 56, 2))   # users 0..27 get 1, 3, .. 55 rows every query selects, some with equal starts
    take = recent[: sum(sizes)]
    assert take.size == sum(sizes)
    u[take] = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    e[take] = oracle.T0_MS
    s[take] = oracle.T0_MS - DAY + rng.integers(0, 40, take.size)
    d[take] = rng.integers(0, 64, take.size)
    cols = (s, e, u, d)
    ctx, ref = loaded(pie, cols, True), loaded(pie, cols, False)
    try:
        qs = queries_of(oracle, nq)
        want = union_of_singles(ref, cols, qs)
        per_user = np.diff(want[0])
        assert ((per_user >= 1) & (per_user <= 8)).any() and ((per_user >= 9) & (per_user <= 16)).any()
        assert (per_user >= 17).sum() >= 10 and per_user.max() <= 64
        got = None
        for _ in range(4):   # buckets that outgrow their slots: the batch's queries are rerun, the capacity grows for the next
            ctx.scan_batch_begin(qs)
            ms = ctx.scan_batch_finish()
            assert ms == [int(((want[2] >> np.uint64(q)) & np.uint64(1)).sum()) for q in range(nq)]
            got = ctx.batch_read_union()
            if got is not None:
                break
        same_union(got, want, "grown slots")
    finally:
        ctx.close()
        ref.close()
