"""GPU: pie_set_end calls that name a row more than once.  The header's rule: the call behaves as its elements applied in array
order, so the last occurrence's value is the row's `end`, and both liveness keys, the hot index and the ordered run agree with it.

The table is T.lattice_table (3 010 rows, every `end` on a bin edge of both keys), so a derived structure that kept an earlier
element's value, one bin away, changes an answer.  A call has 16 384 elements — 64 blocks of 256 threads, all resident at once — and
is built from groups: one row named 2 to 4 times, the occurrences 1 element, less than a wave, less than a block, one to two blocks
or at least 8 192 elements apart, the (earlier, last) values drawn from every ordered pair of nine classes of value (below the
index's range, on fkey_base - 1 and fkey_base, a lower and a higher fine bin, above the fine key's top bin, ten years ahead,
INT64_MAX, the tombstone).  The table has fewer rows than a call has elements, so the elements the groups leave free cannot all
be rows named once: they go to the remaining rows, each named several times WITH ONE VALUE (the repeat the seeded chains have
always sent), at whatever positions are free.

The model (tests/table_model.py) is the only source of expected values; no context is compared with another."""
import time

import numpy as np
import pytest

import table_model as T
from table_model import ALL, INT64_MAX, INT64_MIN, YEAR, Edge, around, liveness_queries

pytestmark = pytest.mark.gpu

K = 16384
CLASSES = ("below", "fbase-1", "fbase", "lower bin", "higher bin", "above fine top", "ten years", "int64 max", "tombstone")
PAIRS = [(a, b) for a in range(len(CLASSES)) for b in range(len(CLASSES)) if a != b]
GAPS = ((1, 1), (2, 63), (64, 255), (256, 511), (8192, 12000))   # distance between the last two occurrences of a group
FORMS = (0x485, 0xC85, 0x01)                                     # 2-byte key, 1-byte key, every byte


class Lattice:
    """The lattice table in a context and in the model, the key parameters it derives, and the nine classes of value."""

    def __init__(self, pie, oracle, hot, ordered, async_mut, seed):
        s, e, u, d, U, D, values = T.lattice_table(oracle)
        self.oracle, self.rng = oracle, np.random.default_rng(seed)
        self.pitch = pitch = 1 << T.LATTICE_SHIFT
        self.base, self.shift, self.fbase, self.fshift = T.key_params(e)
        fbase, e_max = self.fbase, int(e.max())
        fine_top = fbase + ((T.FINE_KEY_MAX - 1) << self.fshift)
        assert fbase + 8 * pitch < e_max - 8 * pitch < e_max < fine_top
        self.pools = [
            [fbase - (1001 + j) * pitch for j in range(0, 2000, 97)],
            [fbase - 1], [fbase],
            [fbase + j * pitch for j in range(1, 9)],
            [e_max - j * pitch for j in range(0, 9)],
            [fine_top, fine_top + pitch, fine_top + 3 * pitch],
            [oracle.T0_MS + 10 * YEAR], [INT64_MAX], [INT64_MIN],
        ]
        assert min(self.pools[0]) > self.base and len(self.pools) == len(CLASSES)
        self.used = sorted({v for p in self.pools for v in p})
        # rows below the fine key's base tombstoned before anything is built: with an ordered run, rows it will not hold.  Moving
        # rows from below the 90th percentile to key 0 leaves the percentile's bin, the smallest and the largest end where they were.
        self.ed = Edge(pie, oracle, (s, e, u, d), U, D, hot, ordered, async_mut)
        pre = self.rng.choice(np.nonzero((e < fbase) & (e > e.min()))[0], 300, replace=False)
        self.ed.set_end("tombstones before the build", pre, np.full(pre.size, INT64_MIN))
        assert T.key_params(self.ed.m.end) == (self.base, self.shift, fbase, self.fshift)
        self.queries = liveness_queries(oracle, [int(e.min()) - 1, e_max + 1] + around(self.used + values[-(values.size // 4):].tolist()))
        v = self.used
        self.windows = [(a + da, b + db) for a, b in zip(v[:-1], v[1:]) for da, db in ((0, 0), (-1, 0), (0, -1), (1, 1))]
        self.windows += [(INT64_MIN, fbase), (INT64_MIN + 1, INT64_MAX), (fbase - 1, INT64_MAX - 1), (v[1], v[-2])]
        self.windows = [w for w in self.windows if INT64_MIN <= min(w) and max(w) <= INT64_MAX]
        self.singles = [fbase - 1, fbase, fbase + pitch, fbase + 4 * pitch - 1, e_max - 3 * pitch, e_max, fine_top - 1, fine_top,
                        oracle.T0_MS + 10 * YEAR - 1, INT64_MAX - 1, min(self.pools[0]), INT64_MIN]

    def value(self, cls):
        p = self.pools[cls]
        return int(p[int(self.rng.integers(len(p)))])

    # ---- one call of K elements
    def build_call(self, group_rows, pair_of, filler_rows, filler_value, k=K):
        """group_rows[g] is named 2 to 4 times, its last two occurrences GAPS[g % 5] apart, the earlier values of class
        pair_of(g)[0] and the last of class pair_of(g)[1]; the elements left free name filler_rows, one value per row.
        -> (rows, new_end, how many groups were placed)"""
        rng = self.rng
        rows, ne = np.full(k, -1, np.int64), np.zeros(k, np.int64)
        free = np.ones(k, bool)
        order = sorted(range(len(group_rows)), key=lambda g: -GAPS[g % 5][1])   # the far groups first, while there is room
        placed = 0
        for g in order:
            lo, hi = GAPS[g % 5]
            m = int(rng.integers(2, 5))
            for _ in range(200):
                gaps = [int(rng.integers(1, 512)) for _ in range(m - 2)] + [int(rng.integers(lo, hi + 1))]
                span = sum(gaps)
                if span >= k:
                    continue
                at = int(rng.integers(0, k - span)) + np.concatenate([[0], np.cumsum(gaps)])
                if np.all(free[at]):
                    break
            else:
                continue
            a, b = pair_of(g)
            free[at] = False
            rows[at] = group_rows[g]
            ne[at] = [self.value(a) for _ in range(m - 1)] + [self.value(b)]
            placed += 1
        at = np.nonzero(free)[0]
        assert len(filler_rows) > 0 and at.size >= len(filler_rows)
        who = np.concatenate([np.arange(len(filler_rows)), rng.integers(0, len(filler_rows), at.size - len(filler_rows))])
        who = who[rng.permutation(who.size)]
        rows[at] = np.asarray(filler_rows)[who]
        ne[at] = np.asarray([filler_value(r) for r in filler_rows], np.int64)[who]
        assert rows.min() >= 0
        return rows.astype(np.int32), ne, placed

    # ---- everything that reads `end` or a structure derived from it, against the model
    def check(self, tag, ordered):
        ed, ctx, m = self.ed, self.ed.ctx, self.ed.m
        ed.columns_match(tag)
        ed.sweep(tag, self.queries, single_every=len(self.queries) + 1)
        for form in FORMS + ((-1,) if ordered == 2 else ()):
            ctx.set_scan_form(form)
            for now in self.singles:
                T.same(ctx.scan(now, INT64_MIN), m.scan(now, INT64_MIN, ALL), (tag, "single scan, form", form, now))
                if form < 0:
                    assert ctx.stats()["k1_variant"] & 0x2000, (tag, "an unpinned scan did not run on the ordered run", now)
        ctx.set_scan_form(-1)
        for prev, now in self.windows:
            assert np.array_equal(ctx.expired_queue(prev, now), m.expired_queue(prev, now)), (tag, "expired", prev, now)

    def compact_and_check(self, tag):
        ed, m = self.ed, self.ed.m
        keep = m.end != INT64_MIN
        assert 0 < int(keep.sum()) < m.n
        assert ed.ctx.compact_rows(INT64_MIN) == int(keep.sum()), (tag, "rows kept")
        m.load(m.start[keep], m.end[keep], m.user[keep], m.disc[keep], m.U, m.D)
        ed.columns_match(tag)
        ed.sweep(tag, self.queries, single_every=17)


@pytest.mark.parametrize("async_mut", [1, 0])
@pytest.mark.parametrize("ordered", [0, 2])
@pytest.mark.parametrize("hot", [1, 0])
def test_repeated_rows_last_value_wins(pie, oracle, hot, ordered, async_mut):
    """Three calls of 16 384 elements on one context, everything checked after each.  The calls differ in what they do to rows
    that were tombstones when the ordered run was built (rows the run does not hold):
      1 leaves them alone: the run must survive (ordered_builds unchanged);
      2 names them in groups that go live and end on the tombstone: the run may be dropped or not, nothing is asserted;
      3 revives them: the run is dropped and rebuilt exactly once, by the next scan.
    With the hot index and no ordered run, every call is mirrored into the index (hot_builds unchanged across it, hot_rows > 0).
    The time of every parametrisation is printed (the model's side of it is about 1 s)."""
    t_begin = time.time()
    L = Lattice(pie, oracle, hot, ordered, async_mut, seed=100 + 4 * hot + ordered + async_mut)
    ed, ctx, m, rng = L.ed, L.ed.ctx, L.ed.m, L.rng
    tomb = len(CLASSES) - 1
    seen_pairs, seen_gaps = set(), set()
    try:
        L.check("built", ordered)
        info = ctx.table_info()
        if ordered == 2:
            assert info["ordered_rows"] > 0 and info["ordered_builds"] == 1
        elif hot:
            assert info["hot_builds"] >= 1 and info["hot_rows"] > 0
        in_run = m.end != INT64_MIN          # rows the run holds: those alive when it was (re)built
        for call in (1, 2, 3):
            tag = "call %d" % call
            held = m.end >= L.fbase
            inside = [rng.permutation(np.nonzero(in_run & ~held)[0]).tolist(), rng.permutation(np.nonzero(in_run & held)[0]).tolist()]
            outside = rng.permutation(np.nonzero(~in_run)[0]).tolist()
            was_tomb = m.end == INT64_MIN
            assert len(inside[0]) > 500 and len(inside[1]) > 100 and len(outside) > 100, (tag, [len(x) for x in inside], len(outside))
            n_out = 0 if call == 1 else min(len(outside) // 2, 72 * 3)
            group_rows, pairs, kinds = [], [], []
            for g in range(2000):
                if g < n_out:        # call 2: live, then the tombstone; call 3: every pair that ends alive
                    pair = [p for p in PAIRS if (p[1] == tomb if call == 2 else p[1] != tomb)][g % (8 if call == 2 else 64)]
                    row, kind = outside.pop(), 2
                else:
                    pair, kind = PAIRS[g % 72], (g // 72) % 2
                    if not inside[kind]:
                        kind = 1 - kind
                    if not inside[kind]:
                        break
                    row = inside[kind].pop()
                group_rows.append(row)
                pairs.append(pair)
                kinds.append(kind)
            filler = inside[0] + inside[1] + (outside if call > 1 else [])
            outside_set = set(outside)
            # call 2 may not revive a row outside the run by a filler either
            rows, ne, placed = L.build_call(group_rows, lambda g: pairs[g], filler,
                                            lambda r: INT64_MIN if call == 2 and r in outside_set else L.value(int(rng.integers(len(CLASSES)))))
            assert rows.size == K and placed > 1900, (tag, placed)
            for g in range(len(group_rows)):
                seen_pairs.add((pairs[g], kinds[g] if kinds[g] < 2 else 2 + int(was_tomb[group_rows[g]])))
                seen_gaps.add(g % 5)
            before = ctx.table_info()
            ctx.set_end(rows, ne)
            m.set_end(rows, ne)
            after = ctx.table_info()
            if hot and not ordered:
                assert after["hot_builds"] == before["hot_builds"] and after["hot_rows"] > 0, (tag, "the index was not mirrored", before, after)
            L.check(tag, ordered)
            if ordered == 2:
                builds = ctx.table_info()["ordered_builds"]
                if call == 1:
                    assert after["ordered_rows"] > 0 and builds == before["ordered_builds"], (tag, "the run did not survive a call on rows it holds")
                elif call == 3:
                    assert builds == before["ordered_builds"] + 1, (tag, "ordered_builds", before["ordered_builds"], builds)
                if builds != before["ordered_builds"]:
                    in_run = m.end != INT64_MIN
        # what the three calls covered: every ordered pair on rows the index held and on rows it did not, every distance; outside
        # the run, live -> tombstone and * -> live on rows that were tombstones at the call
        for kind in (0, 1):
            assert {p for p, k in seen_pairs if k == kind} == set(PAIRS), ("pairs on kind", kind)
        assert {p[1] == tomb for p, k in seen_pairs if k == 3} == {True, False} and seen_gaps == set(range(5))
        L.compact_and_check("compacted")
    finally:
        ctx.close()
    print("hot %d ordered %d async %d: %.2f s" % (hot, ordered, async_mut, time.time() - t_begin))


def test_repeats_equal_the_calls_made_one_by_one(pie, oracle):
    """300 (row, value) pairs over 40 rows: one call on one context, 300 one-element calls on another, each against the model."""
    t_begin = time.time()
    for one_by_one in (False, True):
        L = Lattice(pie, oracle, 1, 1, 1, seed=7)      # the same seed: the same pairs
        ed, rng = L.ed, L.rng
        try:
            ed.sweep("built", L.queries, single_every=23)
            held = ed.m.end >= L.fbase
            pool = np.concatenate([rng.choice(np.nonzero(held)[0], 15, replace=False), rng.choice(np.nonzero(~held & (ed.m.end != INT64_MIN))[0], 15, replace=False),
                                   rng.choice(np.nonzero(ed.m.end == INT64_MIN)[0], 10, replace=False)])
            rows, ne = np.zeros(300, np.int32), np.zeros(300, np.int64)
            for i in range(300):         # a row's consecutive values walk through the ordered pairs of classes
                r = i if i < 40 else int(rng.integers(40))
                a, b = PAIRS[(i * 7 + r) % 72]
                rows[i], ne[i] = pool[r], L.value(b if i % 2 else a)
            assert np.unique(rows).size == 40
            if one_by_one:
                for i in range(300):
                    ed.ctx.set_end(rows[i:i + 1], ne[i:i + 1])
                    ed.m.set_end(rows[i:i + 1], ne[i:i + 1])
                ed.columns_match("one by one")
            else:
                ed.set_end("one call", rows, ne)
            ed.sweep("one by one" if one_by_one else "one call", L.queries, single_every=23)
        finally:
            ed.ctx.close()
    print("one call and 300 calls: %.2f s" % (time.time() - t_begin))


def test_repeats_with_equal_values_and_single_rows(pie, oracle):
    """k = 1; one row named 16 384 times with the last value unlike all the others; repeats that all carry one value."""
    t_begin = time.time()
    L = Lattice(pie, oracle, 1, 1, 1, seed=8)
    ed, rng = L.ed, L.rng
    try:
        ed.sweep("built", L.queries, single_every=23)
        held = np.nonzero(ed.m.end >= L.fbase)[0]
        low = np.nonzero((ed.m.end < L.fbase - 1000 * L.pitch) & (ed.m.end != INT64_MIN))[0]
        ed.set_end("k = 1", [int(low[0])], [L.fbase])
        ed.set_end("k = 1, tombstone", [int(held[0])], [INT64_MIN])
        ed.sweep("k = 1", L.queries, single_every=23)
        # one row, K times: every earlier value lies in the index's range, the last one is the tombstone; then the other way round
        for row, earlier, last in ((int(held[1]), L.pools[3] + L.pools[4], INT64_MIN), (int(low[1]), [INT64_MIN] + L.pools[0], L.pools[4][0])):
            ne = rng.choice(np.array(earlier, np.int64), K)
            ne[-1] = last
            assert last not in earlier
            ed.set_end("one row %d times" % K, np.full(K, row, np.int32), ne)
            assert int(ed.m.end[row]) == last
            ed.sweep("one row %d times" % K, L.queries, single_every=23)
        # repeats with one value per row: 3 000 rows, each named about five times
        n = ed.m.n
        value = np.array([L.value(int(c)) for c in rng.integers(0, len(CLASSES), n)], np.int64)
        rows = np.concatenate([rng.permutation(n), rng.integers(0, n, K - n)])[rng.permutation(K)].astype(np.int32)
        ed.set_end("equal values", rows, value[rows])
        assert np.array_equal(ed.m.end, value)
        ed.sweep("equal values", L.queries, single_every=23)
    finally:
        ed.ctx.close()
    print("single rows and equal values: %.2f s" % (time.time() - t_begin))
