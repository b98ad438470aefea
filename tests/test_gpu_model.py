"""GPU: the table behind the C ABI against a numpy model (tests/table_model.py), with the ordered run, wide batches and the
hot index alive together.

test_model_sequences: seeded chains of 30 to 60 mutators and readers on one table and one context configuration each; after
every mutator the columns are read back and compared bit for bit, every reader is compared with the model, and the path that
answered each call is recorded.  test_model_sequences_reached_every_path then requires that the seed list reached every path.
test_liveness_edges_on_a_lattice / test_cutoff_and_tie_edges: hand-made tables whose values sit on the bin edges of both
liveness keys, on `start == cutoff` and on long runs of equal starts, swept value by value.

These chains carry no token column: the session-store half of the ABI (tokens, turns, in-flight forms, pie_delete_users,
compaction with keys) has a chain of its own, tests/test_gpu_store_chain.py over tests/store_chain.py.

No expected value comes from another GPU context: the model is the only source (index on against off is compared in
test_gpu_hot_index.py)."""
import numpy as np
import pytest

import table_model as T
from table_model import ALL, DAY, HOUR, INT64_MAX, INT64_MIN, YEAR, Edge, around, liveness_queries

pytestmark = pytest.mark.gpu

# Chosen on the MI355X so that together they reach every path of T.PATHS, hold an ordered run and a hot index across a
# set_end, and see the index dropped and rebuilt (test_model_sequences_reached_every_path).
SEEDS = [35, 16, 25, 2, 14, 18, 9, 17, 28, 4, 30, 21, 23]

REACHED = {}   # seed -> what its chain recorded; filled by test_model_sequences, read by the test after it


@pytest.mark.parametrize("seed", SEEDS)
def test_model_sequences(pie, oracle, seed):
    ch = T.run_chain(pie, oracle, seed)
    REACHED[seed] = {"paths": dict(ch.paths), "both": ch.both_valid_at_set_end, "rebuilt": ch.rebuilt_after_drop}


def test_model_sequences_reached_every_path():
    missing = [s for s in SEEDS if s not in REACHED]
    assert not missing, "chains %s failed or were deselected: their path records are missing, run the whole file" % missing
    seen = {}
    for r in REACHED.values():
        for p, k in r["paths"].items():
            seen[p] = seen.get(p, 0) + k
    print("paths reached:", seen)
    assert not [p for p in T.PATHS if not seen.get(p)], "no checked call was answered by %s" % [p for p in T.PATHS if not seen.get(p)]
    assert any(r["both"] for r in REACHED.values()), "no chain held an ordered run and a hot index at the same set_end"
    assert any(r["rebuilt"] for r in REACHED.values()), "no chain saw the hot index dropped and rebuilt"


# ------------------------------------------------------------------------------------------------ key-edge sweeps
# (the Edge helper, around() and liveness_queries() live in table_model.py: test_gpu_set_end_repeats.py uses them too)
@pytest.mark.parametrize("ordered", [0, 2])
@pytest.mark.parametrize("hot", [1, 0])
def test_liveness_edges_on_a_lattice(pie, oracle, hot, ordered):
    s, e, u, d, U, D, values = T.lattice_table(oracle)
    pitch = 1 << T.LATTICE_SHIFT
    base, shift, fbase, fshift = T.key_params(e)
    ed = Edge(pie, oracle, (s, e, u, d), U, D, hot, ordered)
    rng = np.random.default_rng(3)
    try:
        extremes = [int(e.min()) - 1, int(e.max()), int(e.max()) + 1, INT64_MAX - 1, INT64_MIN]
        # every lattice value, one below and one above; in ascending order, so the last batches lie wholly above the fine key's base
        ed.sweep("built", liveness_queries(oracle, extremes + around(values)))
        info = ed.ctx.table_info()
        if not ordered:
            assert (info["hot_builds"] >= 1 and info["hot_rows"] > 0) if hot else info["hot_builds"] == 0
        # a batch whose smallest `now` sits exactly on the fine key's base, and one that straddles it
        ed.sweep("on fkey_base", liveness_queries(oracle, [fbase + k * pitch for k in range(40)]), single_every=5)
        ed.sweep("across fkey_base", liveness_queries(oracle, [fbase - 1] + [fbase + k * pitch for k in range(40)]), single_every=50)
        # rows moved exactly onto v and v - 1 around the fine key's base: from below the index's range and from inside it
        low = np.nonzero(ed.m.end < fbase - 1000 * pitch)[0]
        held = np.nonzero(ed.m.end >= fbase)[0]
        near = [fbase + k * pitch for k in (-2, -1, 0, 1, 2)]
        targets = np.array([v - k for v in near for k in (0, 1)], np.int64)
        rows = np.concatenate([rng.choice(low, 3 * targets.size, replace=False), rng.choice(held, 3 * targets.size, replace=False)])
        ed.set_end("onto fkey_base", rows, np.tile(targets, 6))
        top_quarter = values[-(values.size // 4):]
        ed.sweep("around fkey_base", liveness_queries(oracle, around(np.concatenate([top_quarter, targets]))))
        # late appends put new rows on the same values.  The first outgrows the loaded table's capacity: the columns are
        # re-allocated, the keys refitted to much the same range, and the sweep rebuilds the index.  The second lands in place
        # and is mirrored into that index, which the sweep after it reads.
        on_edges = np.concatenate([top_quarter, targets])
        for k, in_place in ((300, False), (200, True)):
            builds = ed.ctx.table_info()["hot_builds"]
            s2 = (oracle.T0_MS - rng.integers(0, 30 * DAY, k)).astype(np.int64)
            e2 = rng.choice(on_edges, k).astype(np.int64)
            u2, d2 = rng.integers(0, U, k).astype(np.int32), rng.integers(0, D, k).astype(np.int32)
            ed.ctx.append_rows(s2, e2, u2, d2, U)
            ed.m.append_rows(s2, e2, u2, d2, U)
            ed.columns_match("late appends")
            if in_place and hot and not ordered:
                info = ed.ctx.table_info()
                assert info["hot_builds"] == builds and info["hot_rows"] > 0, "the second append was not mirrored into a live index"
            ed.sweep("late appends (in place %s)" % in_place, liveness_queries(oracle, around(on_edges)), single_every=13)
        # above the range the keys were fitted for: the fine key's last bins and its clamp, the 15-bit key's clamp, far beyond
        fine_top = fbase + ((T.FINE_KEY_MAX - 1) << fshift)
        far = np.array([int(e.max()) + pitch, fine_top - pitch, fine_top - 1, fine_top, fine_top + pitch,
                        base + ((T.KEY_MAX - 2) << shift) - 1, base + ((T.KEY_MAX - 2) << shift), base + ((T.KEY_MAX - 1) << shift),
                        oracle.T0_MS + 10 * YEAR, INT64_MAX], np.int64)
        rows = np.concatenate([rng.choice(low, 2 * far.size, replace=False), rng.choice(held, 2 * far.size, replace=False)])
        ed.set_end("above the range", rows, np.tile(far, 4))
        ed.sweep("above the range", liveness_queries(oracle, around(np.concatenate([top_quarter, far]))))
        # tombstones and revivals on the same values
        ed.set_end("tombstones", held[::7], np.full(held[::7].size, INT64_MIN))
        ed.set_end("revived", held[::14], rng.choice(np.concatenate([targets, top_quarter]), held[::14].size))
        ed.sweep("revived", liveness_queries(oracle, around(np.concatenate([top_quarter, targets]))), single_every=17)
        # and late appends once more, onto every value used so far, the far ones included
        k = 300
        s2 = (oracle.T0_MS - rng.integers(0, 30 * DAY, k)).astype(np.int64)
        e2 = rng.choice(np.concatenate([top_quarter, targets, far]), k).astype(np.int64)
        u2, d2 = rng.integers(0, U, k).astype(np.int32), rng.integers(0, D, k).astype(np.int32)
        ed.ctx.append_rows(s2, e2, u2, d2, U)
        ed.m.append_rows(s2, e2, u2, d2, U)
        ed.columns_match("late appends")
        ed.sweep("late appends", liveness_queries(oracle, around(np.concatenate([top_quarter, targets, far]))))
    finally:
        ed.ctx.close()


def test_cutoff_and_tie_edges(pie, oracle):
    s, e, u, d, U, D = T.tie_table(oracle)
    ed = Edge(pie, oracle, (s, e, u, d), U, D)
    t0 = oracle.T0_MS
    masks = [1, 1 << 63, ALL, (1 << 63) | 1, 0x5555555555555555, 0xFFFFFFFF00000000]
    try:
        cutoffs = around(np.unique(s)) + [INT64_MIN, INT64_MAX]
        for tag, now in (("most rows live", t0 - 3 * HOUR), ("top of the range", t0 + 9 * HOUR + HOUR // 2), ("no end excluded", INT64_MIN)):
            queries = [(now, c, masks[i % len(masks)]) for i, c in enumerate(cutoffs)]
            ed.sweep(tag, queries, single_every=4)
        # the same cutoffs after a touch has brought the long tie runs back to life
        ed.set_end("ties revived", np.nonzero(u < 2)[0], np.full(int(np.count_nonzero(u < 2)), t0 + 11 * HOUR))
        queries = [(t0 + 10 * HOUR, c, masks[(i + 1) % len(masks)]) for i, c in enumerate(cutoffs)]
        ed.sweep("ties revived", queries, single_every=4)
    finally:
        ed.ctx.close()
