"""GPU: the paths of the batched union tail (union_tail_body), each at the smallest shape at which it can go wrong.  The tail
publishes a tile's granule from the counts alone, loads the small buckets and the first four 9..16-row buckets of every wave up
front, and counts the rows each query selected by a bit-matrix transpose across the wave; these tests pin all of that bit for
bit against the numpy table model (tests/table_model.py): the union uoff / rows / masks and the per-query M that
scan_batch_finish reports.

Every table is a few thousand rows: `designed` rows whose union bucket sizes are chosen per user (query 0 selects every one
of them, so a user's union bucket is exactly its designed rows), with only two distinct `start` values per user so that the
(start, row) tie-break decides most of the order, shuffled among ten times as many rows that ended long ago (the queries stay
sparse and take the batched pass).  The 64 queries differ pairwise in `now`, cutoff and discipline mask."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_model  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = 2 ** 64 - 1
DAY = 86400 * 1000
HOUR = 3600 * 1000
D = 64
NOBODY = 1 << 63   # the discipline no row has
# seeds at which the 64 per-query totals of the table differ pairwise (the tests assert that they do)
TABLE_SEED = {"sizes": 14, "grown": 1, "over": 16, "mids": 19, "mids_big": 24}


def queries(t0, k=64):
    """Query 0 selects every designed row; query i > 0 has a later `now`, a later cutoff and a mask of its own."""
    rng = np.random.default_rng(77)
    qs = [(t0, t0 - 60 * DAY, ALL ^ NOBODY)]
    seen = {qs[0][2]}
    for i in range(1, 64):   # every discipline but three (and the one nobody has): no two masks alike
        while True:
            m = ALL ^ NOBODY
            for d in rng.choice(63, 3, replace=False):
                m ^= 1 << int(d)
            if m not in seen:
                break
        seen.add(m)
        qs.append((t0 + 1000 * i, t0 - 60 * DAY + 7 * i, m))
    return qs[:k]


def make_table(t0, sizes, seed):
    """Columns (start, end, user, disc) with sizes[u] designed rows for user u (see the module docstring)."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    U = sizes.size
    live = int(sizes.sum())
    n_dead = max(2000, 11 * live)
    user = np.concatenate([np.repeat(np.arange(U, dtype=np.int32), sizes), rng.integers(0, U, n_dead).astype(np.int32)])
    # designed: end just above the `now` of query j (live for queries 0..j), start one of two values of the user, both at or
    # above a cutoff of some query (in the window of a prefix of the queries)
    j_end = rng.integers(0, 64, live)
    end = np.concatenate([t0 + 1000 * j_end + 1, t0 - 30 * DAY - rng.integers(0, 270 * DAY, n_dead)])
    two = t0 - 60 * DAY + 7 * rng.integers(0, 64, (U, 2))
    start = np.concatenate([two[user[:live], rng.integers(0, 2, live)], t0 - 40 * DAY - rng.integers(0, 300 * DAY, n_dead)])
    disc = rng.integers(0, 63, live + n_dead).astype(np.int32)
    perm = rng.permutation(live + n_dead)
    return start[perm].astype(np.int64), end[perm].astype(np.int64), user[perm], disc[perm]


def union_of(model, qs):
    """(uoff[U+1], rows, masks uint64, M per query, per-query results) from the table model."""
    res = model.scan_many(qs)
    mask = np.zeros(model.n, np.uint64)
    for q, (_, _, idx) in enumerate(res):
        mask[idx] |= np.uint64(1 << q)
    rows = np.nonzero(mask)[0]
    rows = rows[np.lexsort((rows, model.start[rows], model.user[rows]))]
    uoff = np.zeros(model.U + 1, np.int64)
    np.add.at(uoff, model.user[rows].astype(np.int64) + 1, 1)
    return np.cumsum(uoff), rows.astype(np.int32), mask[rows], [int(r[2].size) for r in res], res


def ctx_env(pie, **env):
    """A context created under the given environment (read once, when the context is made)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return pie.PieScan(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v


def loaded(pie, cols, U, **env):
    c = ctx_env(pie, **env) if env else pie.PieScan(0)
    c.load_columns(*cols, U)
    c.set_disciplines(ALL, D)
    return c


def same_union(got, want, tag):
    assert got is not None, (tag, "the batch left no union")
    for name, a, b in zip(("uoff", "rows", "masks"), got, want[:3]):
        assert a.dtype == b.dtype and np.array_equal(a, b), (tag, name)


def sizes_small(U, seed, mids=0):
    """Bucket sizes 0 .. 8 for U users, the sizes 0, 1, 7, 8 present where U allows; `mids` users get 9 .. 16 rows."""
    rng = np.random.default_rng(seed)
    s = rng.choice([0, 0, 0, 1, 1, 1, 2, 3, 7, 8], U)
    if mids:
        s[rng.choice(U, min(mids, U), replace=False)] = rng.integers(9, 17, min(mids, U))
    return s


@functools.lru_cache(maxsize=None)
def case(oracle_t0, kind, arg=0):
    """(cols, U, sizes) of a named table: built once, shared, never changed."""
    t0 = oracle_t0
    if kind == "users":
        U = arg
        sizes = sizes_small(U, 100 + U, mids=max(1, U // 40))
        if U == 1:
            sizes[:] = 5
    elif kind == "sizes":      # every bucket size at which the tail takes another path, up to the first capacity
        sizes = sizes_small(300, 5)
        sizes[[0, 1, 2, 3, 64, 65, 130, 255, 256, 299]] = [0, 1, 7, 8, 9, 15, 16, 16, 9, 8]
    elif kind == "grown":      # ... and beyond it: the slot capacity has to grow twice (16 -> 32 -> 64)
        sizes = sizes_small(300, 6)
        sizes[[0, 1, 2, 3, 64, 65, 130, 200, 256, 257, 299]] = [0, 1, 8, 9, 16, 17, 32, 33, 64, 17, 64]
    elif kind == "over":       # one bucket no capacity holds, next to ordinary ones
        sizes = sizes_small(300, 7, mids=6)
        sizes[70] = 70
    elif kind in ("mids", "mids_big"):
        # one tile; wave w (users 64 w ..) holds exactly 1, 4, 5 and 9 buckets of 9 .. 16 rows: the group loaded up front
        # alone, full, with a second round behind it, and with two more.  Some owners sit in lanes 0 .. 15 of their row (they
        # hold a record of the first group and own a bucket), and the lanes around them own full 8-row buckets (a lane that
        # adds eight masks of its own and the record it holds: nine inputs).
        rng = np.random.default_rng(8)
        sizes = rng.choice([0, 1, 2, 3, 8, 8], 256)
        for w, k in enumerate((1, 4, 5, 9)):
            lanes = np.concatenate([[3], rng.choice(np.arange(4, 64), k - 1, replace=False)]) if k > 1 else np.array([17])
            sizes[64 * w + lanes] = np.concatenate([[9, 16], rng.integers(9, 17, k)])[:k]
        assert [int(((sizes[64 * w: 64 * w + 64] >= 9)).sum()) for w in range(4)] == [1, 4, 5, 9]
        if kind == "mids_big":  # the same with a 17 .. 64 bucket in every wave
            for w, (lane, n) in enumerate(((0, 17), (63, 64), (20, 40), (33, 33))):
                assert sizes[64 * w + lane] <= 8
                sizes[64 * w + lane] = n
    else:
        raise KeyError(kind)
    sizes = np.asarray(sizes, np.int64)
    return make_table(t0, sizes, TABLE_SEED.get(kind, 1000 + int(arg))), int(sizes.size), sizes


@functools.lru_cache(maxsize=None)
def wanted(oracle_t0, kind, arg, nq, nothing_at=-1):
    import oracle_py
    cols, U, sizes = case(oracle_t0, kind, arg)
    model = table_model.TableModel(oracle_py)
    model.load(*cols, U, D)
    qs = queries(oracle_t0, nq)
    if nothing_at >= 0:
        qs[nothing_at] = (qs[nothing_at][0], qs[nothing_at][1], NOBODY)
    want = union_of(model, qs)
    if nothing_at < 0:   # the table is what it was designed to be: query 0 selects all designed rows and no others
        assert np.array_equal(np.diff(want[0]), sizes)
    return qs, want


def run_batch(ctx, qs, want, tag, tries=1):
    """One batch, begun and finished alone; with tries > 1 repeated while its union buckets outgrow their slots (the batch
    then answers through the general path — M and the per-query lists are right every time — and the capacity grows)."""
    got = None
    for i in range(tries):
        ctx.scan_batch_begin(qs)
        ms = ctx.scan_batch_finish()
        assert ms == want[3], (tag, "M per query", i)
        got = ctx.batch_read_union()
        if got is not None:
            break
        for q in sorted({0, len(qs) // 2, len(qs) - 1}):
            for name, a, b in zip(("counts", "offsets", "idx"), ctx.batch_read_results(q), want[4][q]):
                assert a.dtype == b.dtype and np.array_equal(a, b), (tag, "overflowed batch", q, name)
    return got, i


@pytest.mark.parametrize("U", [1, 63, 64, 255, 256, 257, 600])
def test_partial_waves_and_tiles(pie, oracle, U):
    """Partial waves, partial tiles and three tiles (the look-back has real predecessors)."""
    cols, _, _ = case(oracle.T0_MS, "users", U)
    qs, want = wanted(oracle.T0_MS, "users", U, 64)
    assert len(set(want[3])) > 1
    ctx = loaded(pie, cols, U)
    try:
        got, _ = run_batch(ctx, qs, want, "U %d" % U)
        same_union(got, want, "U %d" % U)
    finally:
        ctx.close()


@pytest.mark.parametrize("nq", [1, 2, 31, 32, 33, 63, 64])
def test_bucket_sizes_for_every_query_count(pie, oracle, nq):
    """Buckets of 0, 1, 7, 8, 9, 15, 16 rows in one table, 1 .. 64 queries: every per-query total differs from the others."""
    cols, U, _ = case(oracle.T0_MS, "sizes")
    qs, want = wanted(oracle.T0_MS, "sizes", 0, nq)
    assert len(set(want[3])) == nq, "the per-query totals must differ pairwise: a transposition error must not cancel"
    ctx = loaded(pie, cols, U)
    try:
        got, _ = run_batch(ctx, qs, want, "n_q %d" % nq)
        same_union(got, want, "n_q %d" % nq)
    finally:
        ctx.close()


@pytest.mark.parametrize("nq", [64, 20])
def test_buckets_beyond_the_first_capacity(pie, oracle, nq):
    """17, 32, 33 and 64 rows: the first batch reports the overflow and still answers; then the capacity has grown."""
    cols, U, _ = case(oracle.T0_MS, "grown")
    qs, want = wanted(oracle.T0_MS, "grown", 0, nq)
    assert len(set(want[3])) == nq
    ctx = loaded(pie, cols, U)
    try:
        got, rounds = run_batch(ctx, qs, want, "grown", tries=4)
        assert rounds >= 1, "the first batch cannot have held 64-row buckets in 16 slots"
        same_union(got, want, "grown")
    finally:
        ctx.close()


def test_bucket_above_every_capacity(pie, oracle):
    """A user with 70 union rows next to ordinary ones: the batched pass never holds that bucket (the first batches report the
    overflow), every batch answers correctly, and a union that some other path then leaves is the right one."""
    cols, U, _ = case(oracle.T0_MS, "over")
    qs, want = wanted(oracle.T0_MS, "over", 0, 40)
    ctx = loaded(pie, cols, U)
    try:
        got, rounds = run_batch(ctx, qs, want, "over", tries=4)
        assert rounds >= 1
        if got is not None:
            same_union(got, want, "over")
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["mids", "mids_big"])
@pytest.mark.parametrize("nq", [64, 32])
def test_groups_of_mid_buckets_in_one_wave(pie, oracle, kind, nq):
    """Exactly 1, 4, 5 and 9 buckets of 9 .. 16 rows in the four waves of one tile; then the same with a 17 .. 64 bucket in
    each wave."""
    cols, U, _ = case(oracle.T0_MS, kind)
    qs, want = wanted(oracle.T0_MS, kind, 0, nq)
    assert len(set(want[3])) == nq
    ctx = loaded(pie, cols, U)
    try:
        got, _ = run_batch(ctx, qs, want, kind, tries=4 if kind == "mids_big" else 1)
        same_union(got, want, kind)
    finally:
        ctx.close()


def test_query_that_selects_nothing(pie, oracle):
    cols, U, _ = case(oracle.T0_MS, "sizes")
    for nq, at in ((20, 7), (64, 40), (1, 0)):
        qs, want = wanted(oracle.T0_MS, "sizes", 0, nq, at)
        assert want[3][at] == 0 and (nq == 1 or sum(want[3]) > 0)
        ctx = loaded(pie, cols, U)
        try:
            got, _ = run_batch(ctx, qs, want, "nothing at %d of %d" % (at, nq))
            same_union(got, want, "nothing at %d of %d" % (at, nq))
        finally:
            ctx.close()


@pytest.mark.parametrize("ride", [1, 0])
@pytest.mark.parametrize("lanes", [1, 3])
def test_riding_and_stand_alone_tails_in_flight(pie, oracle, ride, lanes):
    """Several batches in flight on one lane and on three, the tail riding in the next pass's launch (and flushed for the last
    ones) or launched by itself: batches of different query counts, each with its own result."""
    cols, U, _ = case(oracle.T0_MS, "users", 600)
    sets = [wanted(oracle.T0_MS, "users", 600, k) for k in (64, 33, 20, 64, 1, 40, 32, 64, 2)]
    ctx = loaded(pie, cols, U, PIE_K2_RIDE=ride)
    try:
        ctx.set_batch_lanes(lanes)
        cap = 3 * lanes
        begun = done = 0
        while done < len(sets):
            while begun < len(sets) and begun - done < cap:
                ctx.scan_batch_begin(sets[begun][0])
                begun += 1
                if begun == len(sets):
                    ctx.scan_batch_flush()
            assert ctx.scan_batch_finish() == sets[done][1][3], (done, "M per query")
            same_union(ctx.batch_read_union(), sets[done][1], "ride %d, %d lanes, batch %d" % (ride, lanes, done))
            done += 1
    finally:
        ctx.close()


@pytest.mark.parametrize("nq", [64, 20])
def test_union_message_smaller_than_the_union(pie, oracle, nq):
    """scan_batch_begin_union with room for fewer rows than Mu: offsets and Mu complete, rows and masks cut at the capacity —
    from the small buckets, the 9 .. 16 groups and the 17 .. 64 path alike."""
    cols, U, _ = case(oracle.T0_MS, "mids_big")
    qs, want = wanted(oracle.T0_MS, "mids_big", 0, nq)
    w_uoff, w_rows, w_masks = want[:3]
    mu = int(w_rows.size)
    ctx = loaded(pie, cols, U)
    try:
        got, _ = run_batch(ctx, qs, want, "grow first", tries=4)   # (the capacity grows to 64 slots before the message batches)
        same_union(got, want, "grow first")
        planes = 3 if nq > 32 else 2
        for cap in (mu + 3, mu // 2, 5):
            u_pad = U + 3
            h, dev, addr = ctx.host_alloc(u_pad + 2 + planes * cap)
            try:
                h[:] = -7
                ctx.scan_batch_begin_union(qs, dev, u_pad, cap)
                ms, ready = ctx.scan_batch_finish(packed=True)
                assert ready and ms == want[3]
                k = min(cap, mu)
                assert np.array_equal(h[: U + 1], w_uoff.astype(np.int32)) and np.all(h[U + 1: u_pad + 2] == mu)
                assert np.array_equal(h[u_pad + 2: u_pad + 2 + k], w_rows[:k])
                lo = h[u_pad + 2 + cap: u_pad + 2 + cap + k].astype(np.uint32).astype(np.uint64)
                hi = h[u_pad + 2 + 2 * cap: u_pad + 2 + 2 * cap + k].astype(np.uint32).astype(np.uint64) if nq > 32 else np.uint64(0)
                assert np.array_equal(lo | (hi << np.uint64(32)), w_masks[:k])
                if cap > mu:
                    assert np.all(h[u_pad + 2 + mu: u_pad + 2 + cap] == -7)
                same_union(ctx.batch_read_union(), want, "message cap %d" % cap)
            finally:
                ctx.host_free(addr)
    finally:
        ctx.close()
