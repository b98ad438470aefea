"""GPU: the slot-ordered hot index (PIE_HOT_ORDER=slot, pie_kernels.h k_hot_keys / k_hot_gather).  Inside a bin the records
stand by histogram slot of their user, rows ascending among equal keys; nothing but the locality of the pass's atomics may
depend on it.  Layout through pie_hot_layout, against the row-order build of the same table; results of batches of 1, 33 and 64
queries with the order on `slot`, on `row` (the fallback build, forced by the switch) and with no index at all, against each
other and against single-query scans, before and after every kind of mutation, on one and on three lanes.

Tables.  The fine key's base is the lower edge of the coarse-key bin that holds the 90th percentile of `end` (tombstones count
as the smallest key), and a query with a tenth of the table live above it is not batched at all.  So:
  spread    89 % of the rows end far below, 11 % uniformly over a day on top: the index holds the top rows from the 90th
            percentile's coarse bin up (all but the lowest tenth of that day), and every
            bin the fine key's shift can reach is populated (the shift leaves the largest `end` between key 63 and key 126, so
            the populated bins are 1 .. at least 63, not always all 127); the queries look at the upper five eighths of that day
  one-bin   92 % tombstones: the base falls to the smallest live `end` and every live row is in the index.  One row a day
            below and one a day above pin the range; all others end within one second, far inside one bin
  few       4 050 of 4 096 rows are tombstones, the 46 live ones spread over a day
  none      every row is a tombstone: an index with no main record
Rows per table and user are few enough that a user's selected rows fit the union's 64 slots (else the batches of that table
would turn into single scans and leave the index unused)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL = 2 ** 64 - 1
DAY = 86400 * 1000
HOUR = 3600 * 1000
T0 = 1_700_000_000_000
D = 32
MASKS = [0x55555555, 0xAAAAAAAA, 0xFFFFFFFF, 0x0000FFFF, 0x1, 0x80000001]


def ctx_with(pie, order):
    """order: 'slot', 'row', or None for a context that never builds the index."""
    keep = {k: os.environ.get(k) for k in ("PIE_HOT_INDEX", "PIE_HOT_ORDER")}
    os.environ["PIE_HOT_INDEX"] = "0" if order is None else "1"
    os.environ["PIE_HOT_ORDER"] = order or "slot"
    try:
        return pie.PieScan(0)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v


def make_table(pie, kind, n, U, seed):
    rng = np.random.default_rng(seed)
    start = (T0 - rng.integers(0, 60 * DAY, n)).astype(np.int64)
    user = rng.integers(0, U, n).astype(np.int32)
    disc = rng.integers(0, D, n).astype(np.int32)
    n_top = n - int(n * 0.89)
    end = (T0 - 200 * DAY + rng.integers(0, 10 * DAY, n)).astype(np.int64)
    top = rng.choice(n, n_top, replace=False)
    if kind == "one-bin":
        end[:] = pie.PIE_END_NONE
        live = rng.choice(n, int(n * 0.08), replace=False)
        end[live] = T0 + rng.integers(0, 1000, live.size)
        end[live[0]], end[live[1]] = T0 - DAY, T0 + DAY
    elif kind == "spread":
        end[top] = T0 - 12 * HOUR + rng.integers(0, 24 * HOUR, n_top)
    elif kind == "few":
        end[:] = pie.PIE_END_NONE
        live = rng.choice(n, 46, replace=False)
        end[live] = T0 - 12 * HOUR + rng.integers(0, 24 * HOUR, 46)
    elif kind == "none":
        end[:] = pie.PIE_END_NONE
    return start, end, user, disc


def queries_for(kind, k):
    if kind == "one-bin":   # the last 64 ms of the second the rows end in: `now` values that are `end` values of some rows
        nows = [T0 + 999 - i for i in range(k)]
    else:                   # the upper five eighths of the top day: under a tenth of the table is live, all of it in the index
        nows = [T0 - 3 * HOUR + (14 * HOUR * i) // max(k, 1) - 977 * i for i in range(k)]
    return [(nows[i], T0 - (61 - (i % 5) * 9) * DAY - 13 * i, MASKS[i % len(MASKS)]) for i in range(k)]


TABLES = {  # name: (kind, rows, users)
    "one-bin-u1": ("one-bin", 4096, 1),
    "spread-u33": ("spread", 8192, 33),
    "spread-u101": ("spread", 30000, 101),
    "spread-u1000": ("spread", 200000, 1000),
    "few-u101": ("few", 4096, 101),
    "none-u33": ("none", 4096, 33),
    "users-over-hot-rows": ("spread", 8192, 50000),
}


class Trio:
    """One table in three contexts: index in slot order, index in row order (the fallback build), no index."""

    def __init__(self, pie, kind, n, U, seed=5):
        self.pie, self.kind, self.U = pie, kind, U
        self.cols = make_table(pie, kind, n, U, seed)
        self.ctx = {"slot": ctx_with(pie, "slot"), "row": ctx_with(pie, "row"), "off": ctx_with(pie, None)}
        for c in self.ctx.values():
            c.load_columns(*self.cols, U)
            c.set_disciplines(ALL, D)

    def close(self):
        for c in self.ctx.values():
            c.close()

    def each(self, fn):
        return {k: fn(c) for k, c in self.ctx.items()}

    def lanes(self, n_lanes):
        self.each(lambda c: c.set_batch_lanes(n_lanes))

    def run(self, c, batches):
        """Every batch begun before the first is finished (they share the lanes); -> per batch (union, per-query results)."""
        for qs in batches:
            c.scan_batch_begin(qs)
        out = []
        for qs in batches:
            c.scan_batch_finish()
            out.append((c.batch_read_union(), [c.batch_read_results(q) for q in range(len(qs))]))
        return out

    def check(self, tag, in_flight=1):
        batches = [queries_for(self.kind, k) for k in (1, 33, 64)]
        got = {}
        for name, c in self.ctx.items():
            got[name] = []
            for i in range(0, len(batches), in_flight):
                got[name] += self.run(c, batches[i:i + in_flight])
        for b, qs in enumerate(batches):
            ref_union, ref_res = got["off"][b]
            for name in ("slot", "row"):
                union, res = got[name][b]
                assert (union is None) == (ref_union is None), (tag, name, b)
                if union is not None:
                    for what, x, y in zip(("uoff", "rows", "masks"), union, ref_union):
                        assert x.dtype == y.dtype and np.array_equal(x, y), (tag, name, "batch of %d" % len(qs), "union " + what)
                for q in range(len(qs)):
                    for what, x, y in zip(("counts", "offsets", "idx"), res[q], ref_res[q]):
                        assert x.dtype == y.dtype and np.array_equal(x, y), (tag, name, "batch of %d" % len(qs), "query %d" % q, what)
        # single-query scans, on the context without an index: first, middle and last query of every batch
        single = self.ctx["off"]
        for b, qs in enumerate(batches):
            for q in sorted({0, len(qs) // 2, len(qs) - 1}):
                now, cutoff, mask = qs[q]
                single.set_disciplines(mask, D)
                want = single.scan(now, cutoff)
                for what, x, y in zip(("counts", "offsets", "idx"), got["slot"][b][1][q], want):
                    assert np.array_equal(x, y), (tag, "batch of %d" % len(qs), "query %d vs a single scan" % q, what)
        single.set_disciplines(ALL, D)
        return got

    def check_layout(self, tag, expect_order=1):
        """The slot context's layout against the table and against the row-order build of the same table."""
        slot, row = self.ctx["slot"], self.ctx["row"]
        info = slot.table_info()
        assert info["hot_builds"] >= 1 and row.table_info()["hot_builds"] >= 1, (tag, "the batches did not use the index")
        assert info["hot_order"] == expect_order and row.table_info()["hot_order"] == 0, tag
        L, R = slot.hot_layout(), row.hot_layout()
        n, m, U = slot.n, L["n_main"], slot.n_users
        _, end, user, _ = slot.read_columns()
        assert info["hot_rows"] == m == L["off"][128] == R["n_main"], tag
        assert np.array_equal(L["off"], R["off"]) and L["off"][0] == 0 and L["off"][1] == 0 and np.all(np.diff(L["off"]) >= 0), tag
        pos = L["pos"]
        held = np.nonzero(pos >= 0)[0]
        # every row with fine key >= 1 exactly once: the held rows are the rows at or above one threshold of `end` ...
        assert held.size == m and np.unique(L["row"]).size == m, tag
        if 0 < m < n:
            assert end[held].min() > np.delete(end, held).max(), tag
        # ... the same rows, in the same bins, as the row-order build holds
        assert np.array_equal(np.sort(L["row"]), np.sort(R["row"])), tag
        bin_of = np.zeros(n, np.int32)
        bin_of[R["row"]] = R["bin"]
        assert np.array_equal(bin_of[L["row"]], L["bin"]), tag
        # pos[] agrees with the records, the records with the table and with the bin offsets
        assert np.array_equal(pos[L["row"]], np.arange(m)), tag
        assert np.array_equal(user[L["row"]], L["user"]), tag
        assert np.array_equal(L["bin"], np.searchsorted(L["off"][1:], np.arange(m), side="right").astype(np.int32)), tag
        assert m == 0 or (L["bin"].min() >= 1 and L["bin"].max() <= 127), tag
        # the row-order build: rows ascend inside every bin
        same_bin = R["bin"][1:] == R["bin"][:-1]
        assert np.all(R["row"][1:][same_bin] > R["row"][:-1][same_bin]), tag
        # the slot build: keys never fall (the bin is the key's high part), rows ascend among equal keys
        bits = self.pie.hot_slot_bits(U)
        assert bits == info["hot_slot_bits"], tag
        t = (U + 31) // 32
        u64 = L["user"].astype(np.int64)
        key = (L["bin"].astype(np.int64) << bits) | ((u64 & 31) * t + (u64 >> 5))
        for i in range(0, m, max(1, m // 16)):
            assert key[i] == self.pie.hot_order_key(int(L["bin"][i]), int(L["user"][i]), U), tag
        if expect_order == 1:
            assert np.all(np.diff(key) >= 0), (tag, "keys fall inside a bin")
            tie = key[1:] == key[:-1]
            assert np.all(L["row"][1:][tie] > L["row"][:-1][tie]), (tag, "rows do not ascend among equal keys")
        return L


@pytest.mark.parametrize("name", list(TABLES))
def test_layout_and_results(pie, name):
    kind, n, U = TABLES[name]
    t = Trio(pie, kind, n, U)
    try:
        t.check(name)
        L = t.check_layout(name)
        filled = np.count_nonzero(np.diff(L["off"][1:]))
        if kind == "one-bin":
            assert L["n_main"] == int(n * 0.08) and np.diff(L["off"]).max() == L["n_main"] - 2 and filled == 3
        elif kind == "spread":
            assert L["n_main"] >= n // 11 and filled >= 63 and np.all(np.diff(L["off"][1:1 + filled + 1]) > 0)
        elif kind == "few":
            assert 0 < L["n_main"] < 64
        else:
            assert L["n_main"] == 0
        if name == "users-over-hot-rows":
            assert U > L["n_main"]
        assert t.ctx["off"].table_info()["hot_builds"] == 0
    finally:
        t.close()


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("name", ["spread-u33", "users-over-hot-rows"])
def test_results_after_mutation(pie, name, lanes):
    kind, n, U = TABLES[name]
    t = Trio(pie, kind, n, U, seed=9)
    rng = np.random.default_rng(lanes)
    try:
        t.lanes(lanes)
        t.check(name + ": built", in_flight=lanes)
        t.check_layout(name + ": built")
        s, e, u, d = [c.copy() for c in t.cols]
        hot = np.nonzero(e > T0 - 13 * HOUR)[0]
        cold = np.nonzero(e < T0 - 100 * DAY)[0]

        def set_end(rows, ne):
            rows, ne = rows.astype(np.int32), ne.astype(np.int64)
            t.each(lambda c: c.set_end(rows, ne))
            e[rows] = ne

        # set_end: the same value and a slightly lower one (the entry stays where it is), far lower (out of the range), and
        # up: top rows to the top of the range and rows from below into it (both move to the delta)
        k = 40   # few enough that the 90th percentile of `end`, and with it the rebuilt index's base, stays below the queries
        pick = rng.choice(hot, 4 * k, replace=False)
        set_end(pick[:k], e[pick[:k]])
        set_end(pick[k:2 * k], e[pick[k:2 * k]] - 1000)
        set_end(pick[2 * k:3 * k], np.full(k, T0 - 150 * DAY))
        set_end(pick[3 * k:], np.full(k, T0 + 12 * HOUR - 1) - rng.integers(0, 1000, k))
        set_end(rng.choice(cold, k, replace=False), T0 + rng.integers(-6 * HOUR, 11 * HOUR, k))
        t.check(name + ": set_end", in_flight=lanes)

        # appends with new user ids: n_users grows under the index and its order goes stale.  The first outgrows the loaded
        # table's capacity (the keys and the index are rebuilt), the second lands in place.
        for step in range(2):
            ka, U2 = 60, t.ctx["slot"].n_users + 5
            s2 = (T0 - rng.integers(0, 20 * HOUR, ka)).astype(np.int64)
            e2 = (T0 + rng.integers(-10 * HOUR, 11 * HOUR, ka)).astype(np.int64)
            u2 = np.concatenate([np.arange(U2 - 5, U2), rng.integers(0, U2, ka - 5)]).astype(np.int32)
            d2 = rng.integers(0, D, ka).astype(np.int32)
            t.each(lambda c: c.append_rows(s2, e2, u2, d2, U2))
            s, e, u, d = np.concatenate([s, s2]), np.concatenate([e, e2]), np.concatenate([u, u2]), np.concatenate([d, d2])
            t.check(name + ": appended %d" % step, in_flight=lanes)
        assert t.ctx["slot"].n_users == U + 10
        assert t.ctx["slot"].table_info()["hot_rows"] > 0

        # deletes
        for uu in rng.choice(min(U, 33), 5, replace=False):
            gone = t.each(lambda c: c.delete_user(int(uu)))
            assert np.array_equal(gone["slot"], gone["off"]) and np.array_equal(gone["row"], gone["off"])
            e[gone["off"]] = pie.PIE_END_NONE
        t.check(name + ": deleted", in_flight=lanes)

        # compaction drops the tombstones and renumbers the rows; the next batch rebuilds the index, in slot order again
        kept = t.each(lambda c: c.compact_rows())
        assert kept["slot"] == kept["row"] == kept["off"] == int(np.count_nonzero(e != pie.PIE_END_NONE))
        before = t.ctx["slot"].table_info()["hot_builds"]
        t.check(name + ": compacted", in_flight=lanes)
        assert t.ctx["slot"].table_info()["hot_builds"] == before + 1
        t.check_layout(name + ": compacted and rebuilt")
    finally:
        t.close()


def test_switch_is_reported(pie):
    """pie_table_info tells the order before any index exists (what the next build will try) and after."""
    for order, code in (("slot", 1), ("row", 0)):
        c = ctx_with(pie, order)
        try:
            assert c.table_info()["hot_order"] == code and c.table_info()["hot_build_ms"] == 0.0
            c.load_columns(*make_table(pie, "spread", 20000, 33, 1), 33)
            c.set_disciplines(ALL, D)
            c.scan_batch(queries_for("spread", 4))
            info = c.table_info()
            assert info["hot_builds"] == 1 and info["hot_order"] == code and info["hot_build_ms"] > 0.0
        finally:
            c.close()
