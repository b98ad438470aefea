"""GPU: the ordered run (sph-pie_amd/csrc/pie_ordered.h, host side in pie_scan.hip) on designed tables, bit for bit against the
oracle, through the C ABI.  tests/ordered_cases.py designs the tables and restates the layout (run_layout, respread_layout,
RunModel); test_ordered_cases_cpu.py shows what each table plants.  Here the model is pinned to the device first
(pie_table_info's ordered_positions / ordered_rows / ordered_builds / ordered_respreads), then every query of every table is
compared with oracle.scan — counts, offsets and idx, dtypes included — and the form that was meant to run is asserted through
pie_stats (k1_variant 0x2003 dense, 0x2400 keyed on the 2-byte key, 0x2C00 keyed on the 1-byte key, 0x3000 set for batches; live,
selected and candidates are the model's).

Routes.  With a key histogram that describes the table, ordered_keyed_form takes the keyed form only for a `now` whose histogram
bin holds under 8 % of the rows at or above it, and the fine key's base is the lower edge of the bin of the 90th percentile
(build_keys): such a `now` is never below fkey_base, so launch_ordered's `fine` is true and a fresh context never runs the 2-byte
keyed single scan.  It is reached here the two ways the library offers: a context created under PIE_K1_KEYED=0x485 (the keyed
form without the fine key), and, once a touch has marked the histogram stale (key_dirty), a `now` below fkey_base right after a
sparse scan (ordered_keyed_form then goes by the last scan's live fraction).  The second way with `now` below every `end` is the
keyed form with key(now) == 0: padding and spare positions become candidates and are dropped by a_pos < n_ord
(test_alternating_forms_share_the_unit_counts).

Every batch designed to stay on the run must hand out its union; only the batch whose union is one row above batch_ucap
(union-cap) is designed to rerun, and there the union must be absent.  The keyed emit's in_lds == false needs 5.4e8 positions."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ordered_cases as oc  # noqa: E402
import table_model as tm  # noqa: E402
from table_model import ctx_with_env  # noqa: E402

pytestmark = pytest.mark.gpu

DENSE, KEYED2, KEYED1 = 0x2003, 0x2400, 0x2C00
INT64_MIN = oc.INT64_MIN


_WANTED = {}


def wanted(oracle, tab, q):
    """The oracle's answer of one query of one designed table: computed once, shared, never changed."""
    key = (tab.name, tab.n_ord) + tuple(q)
    if key not in _WANTED:
        res = oracle.scan(*tab.cols, tab.U, *q)
        for a in res:
            a.setflags(write=False)
        _WANTED[key] = res
    return _WANTED[key]


def same(got, want, tag):
    for name, a, b in zip(("counts", "offsets", "idx"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), (tag, name)


def loaded(ctx, tab):
    ctx.load_columns(*tab.cols, tab.U)
    ctx.set_ordered_run(2)
    return ctx


def pin_layout(ctx, tab, tag):
    info = ctx.table_info()
    assert info["ordered_positions"] == tab.n_ord and info["ordered_rows"] == tab.cols[0].size and info["ordered_builds"] == 1, (tag, info)


def scan_one(ctx, oracle, tab, q, form, tag):
    ctx.set_disciplines(q[2], oc.D)
    got = ctx.scan(q[0], q[1])
    same(got, wanted(oracle, tab, q), tag)
    st = ctx.stats()
    assert st["k1_variant"] == form, (tag, hex(st["k1_variant"]))
    assert st["selected"] == oc.selected_positions(tab, q).size and st["live"] == oc.live_positions(tab, q).size, (tag, st)
    if form != DENSE and q[0] >= oc.T_MIDNOW:
        assert st["candidates"] == oc.candidate_positions(tab, q).size, (tag, st)
    return st


def batch_on(ctx, oracle, cols, U, qs, tag, wide=False, rerun=False, wants=None):
    """one batch: per-query lists against the oracle; the union against the union of the oracle's answers — it must exist unless the
    batch is designed to rerun its queries (rerun), where it must not"""
    ctx.set_disciplines(oc.ALL, oc.D)
    got = ctx.scan_wide(qs) if wide else ctx.scan_batch(qs)
    if not rerun:
        assert ctx.stats()["k1_variant"] & 0x3000 == 0x3000, (tag, hex(ctx.stats()["k1_variant"]))
    wants = [oracle.scan(*cols, U, *q) for q in qs] if wants is None else wants
    for qi, w in enumerate(wants):
        same(got[qi], w, (tag, qi))
    un = ctx.batch_read_union_wide() if wide else ctx.batch_read_union()
    if rerun:
        assert un is None, (tag, "a rerun batch has no union")
        return
    assert un is not None, (tag, "the batch lost its union")
    uoff, rows, masks = tm.union_from_answers(cols[0], cols[2], U, wants)
    assert np.array_equal(un[0], uoff) and np.array_equal(un[1], rows), (tag, "union")
    assert np.array_equal(np.asarray(un[2]).reshape(masks.shape), masks), (tag, "union masks")


def batch(ctx, oracle, tab, qs, tag, wide=False, rerun=False):
    batch_on(ctx, oracle, tab.cols, tab.U, qs, tag, wide, rerun, [wanted(oracle, tab, q) for q in qs])


def small(name):
    if name == "uoff-edges":
        masks = oc.uoff_edges_queries()
        return oc.uoff_edges(), {f"sparse {k}": oc.sparse(m) for k, m in masks.items()}, {f"old {k}": oc.old(m) for k, m in masks.items()}
    if name == "chunk-counts":
        ms = {"all": oc.bit(oc.G_A, oc.G_B), "alternating": oc.bit(oc.G_A), "none": oc.bit(oc.G_NONE)}
        return oc.chunk_counts(), {k: oc.sparse(m) for k, m in ms.items()}, {f"old {k}": oc.old(m) for k, m in ms.items()}
    if name == "tile-slices":
        m = oc.bit(oc.G_DENSE, oc.G_AMB)
        return oc.tile_slices(), {"sparse": oc.sparse(oc.ALL)}, {"mid": oc.mid(m), "old": oc.old(m), "mid dense only": oc.mid(oc.bit(oc.G_DENSE))}
    tab = oc.alternating()
    return tab, {f"sparse {g}": oc.sparse(oc.bit(g)) for g in oc.G_ALT}, {f"old {g}": oc.old(oc.bit(g)) for g in oc.G_ALT}


@pytest.mark.parametrize("name", ["uoff-edges", "chunk-counts", "tile-slices", "alternating"])
def test_small_tables(pie, oracle, name):
    """every query of a small table: keyed on the 1-byte key and dense in a default context, keyed on the 2-byte key in a
    context without the fine key, then batches of 16 and of 33 queries (the HI template) of the sparse queries"""
    tab, keyed, dense = small(name)
    with loaded(pie.PieScan(0), tab) as ctx:
        first = True
        for k, q in list(keyed.items()) + list(dense.items()):
            scan_one(ctx, oracle, tab, q, KEYED1 if k in keyed else DENSE, (name, k))
            if first:
                pin_layout(ctx, tab, name)
                first = False
        qs = list(keyed.values())
        for nq in (16, 33):
            batch(ctx, oracle, tab, [qs[i % len(qs)] for i in range(nq)], (name, "batch", nq))
        assert ctx.table_info()["ordered_builds"] == 1
    with loaded(ctx_with_env(pie, PIE_K1_KEYED="0x485"), tab) as ctx:
        for k, q in keyed.items():
            scan_one(ctx, oracle, tab, q, KEYED2, (name, "2-byte", k))
        batch(ctx, oracle, tab, [qs[i % len(qs)] for i in range(16)], (name, "2-byte batch"))


def test_alternating_forms_share_the_unit_counts(pie, oracle):
    """A B C A over the forms on ONE run: each scan's unit-count buffer was zeroed by the scan before it, and the forms use it with
    different unit sizes.  keyed 1-byte, dense, a 16-query batch, [a touch that rewrites a row's own `end`: the key histogram is
    stale from here and the form goes by the live fraction of the single scan before], dense on the sparse query, keyed 1-byte,
    keyed 2-byte with key(now) == 0 (every position is a candidate), a wide batch, dense, dense."""
    tab = oc.alternating()
    a, b, c = (oc.bit(g) for g in oc.G_ALT)
    with loaded(pie.PieScan(0), tab) as ctx:
        ctx.set_wide_ordered(1)
        scan_one(ctx, oracle, tab, oc.sparse(a), KEYED1, "A keyed 1-byte")
        pin_layout(ctx, tab, "alternating")
        scan_one(ctx, oracle, tab, oc.old(b), DENSE, "B dense")
        batch(ctx, oracle, tab, [oc.sparse(m) for m in (c, a, b, a | b)] * 4, "C batch")
        row = np.array([int(tab.pos_row[oc.selected_positions(tab, oc.sparse(a))[0]])], np.int32)
        ctx.set_end(row, tab.cols[1][row])
        scan_one(ctx, oracle, tab, oc.sparse(c), DENSE, "C dense on the sparse query (the last scan found every row live)")
        scan_one(ctx, oracle, tab, oc.sparse(a), KEYED1, "A keyed 1-byte again")
        st = scan_one(ctx, oracle, tab, oc.old(b), KEYED2, "B keyed 2-byte, key(now) == 0")
        assert st["candidates"] == tab.n_ord                                      # spare slots too; the padding beyond n_ord is dropped
        batch(ctx, oracle, tab, [oc.sparse(m) for m in (c, b, a)] * 23, "C wide batch", wide=True)
        scan_one(ctx, oracle, tab, oc.old(a), DENSE, "A dense")
        scan_one(ctx, oracle, tab, oc.mid(c), DENSE, "C dense")
        assert ctx.table_info()["ordered_builds"] == 1


@pytest.mark.parametrize("nq", [16, 33])
def test_union_chunks(pie, oracle, nq):
    """chunks of 8 and 9 staged records (the per-lane against the whole-wave copy of k_ord_union_emit), 64, 65, 512, heavy beside
    light, queries with no row: ordinary batch on both keys, and the wide pass"""
    tab = oc.union_chunks()
    qs = oc.union_chunks_queries(nq)
    with loaded(pie.PieScan(0), tab) as ctx:
        scan_one(ctx, oracle, tab, qs[0], KEYED1, "builds the run")
        batch(ctx, oracle, tab, qs, ("union-chunks", nq))
        ctx.set_wide_ordered(1)
        batch(ctx, oracle, tab, qs * 3, ("union-chunks wide", nq), wide=True)
    with loaded(ctx_with_env(pie, PIE_K1_KEYED="0x485"), tab) as ctx:
        scan_one(ctx, oracle, tab, qs[0], KEYED2, "builds the run")
        batch(ctx, oracle, tab, qs, ("union-chunks 2-byte", nq))


def test_union_of_exactly_batch_ucap_rows_and_one_more(pie, oracle):
    tab = oc.union_cap()
    m = [oc.bit(oc.G_U1), oc.bit(oc.G_U2), oc.bit(oc.G_U1, oc.G_U2), oc.bit(oc.G_NONE)]
    fits = [oc.sparse(m[i % 4]) for i in range(16)]
    with loaded(pie.PieScan(0), tab) as ctx:
        ctx.set_disciplines(oc.ALL, oc.D)
        same(ctx.scan(oc.T_NOW, INT64_MIN), wanted(oracle, tab, oc.sparse(oc.ALL)), "builds the run")
        pin_layout(ctx, tab, "union-cap")
        batch(ctx, oracle, tab, fits, "exactly batch_ucap rows")
        batch(ctx, oracle, tab, fits + [oc.sparse(oc.bit(oc.G_U3))], "one row more: n_over, rerun per query", rerun=True)
        batch(ctx, oracle, tab, fits, "after the overflow: single scans from now on", rerun=True)


# ------------------------------------------------------------------------------------------------ the large table
@functools.lru_cache(maxsize=None)
def large_table():
    import torch
    return oc.large(int(torch.cuda.get_device_properties(0).multi_processor_count))


def large_queries(f=oc.sparse):
    return {k: f(m) for k, m in oc.LARGE_QUERIES.items()}


def test_large_keyed_2byte_waves_own_two_chunks(pie, oracle):
    tab = large_table()
    with loaded(ctx_with_env(pie, PIE_K1_KEYED="0x485"), tab) as ctx:
        for k, q in large_queries().items():
            scan_one(ctx, oracle, tab, q, KEYED2, ("large 2-byte", k))
            pin_layout(ctx, tab, "large")
        qs = list(large_queries().values())
        batch(ctx, oracle, tab, [qs[i % len(qs)] for i in range(16)], "large 2-byte batch")       # grid n_cus * 6: two chunks a wave
        ctx.set_wide_ordered(1)
        batch(ctx, oracle, tab, [qs[i % len(qs)] for i in range(66)], "large 2-byte wide", wide=True)   # n_cus * 3: three


def test_large_keyed_1byte_grid_1(pie, oracle):
    """PIE_ORD_GRID=1: the 1-byte single scan and batch deal eight or nine chunks to every wave"""
    tab = large_table()
    with loaded(ctx_with_env(pie, PIE_ORD_GRID="1"), tab) as ctx:
        for k, q in large_queries().items():
            scan_one(ctx, oracle, tab, q, KEYED1, ("large 1-byte", k))
        qs = list(large_queries().values())
        batch(ctx, oracle, tab, [qs[i % len(qs)] for i in range(33)], "large 1-byte batch")
        ctx.set_wide_ordered(1)
        batch(ctx, oracle, tab, [qs[i % len(qs)] for i in range(66)], "large 1-byte wide", wide=True)   # n_cus * 4: three chunks a wave
        pin_layout(ctx, tab, "large")


def test_large_dense_two_prefix_groups(pie, oracle):
    tab = large_table()
    assert (tab.n_ord + oc.TILE - 1) // oc.TILE > oc.GROUP
    with loaded(pie.PieScan(0), tab) as ctx:
        for k in ("bounds", "waves", "all"):
            scan_one(ctx, oracle, tab, oc.old(oc.LARGE_QUERIES[k]), DENSE, ("large dense", k))
        scan_one(ctx, oracle, tab, oc.mid(oc.LARGE_QUERIES["all"] | oc.bit(oc.FILL)), DENSE, "large dense mid")
        pin_layout(ctx, tab, "large")


# ------------------------------------------------------------------------------------------------ appends
def check_info(ctx, m, tag):
    info = ctx.table_info()
    for k, v in m.info().items():
        assert info[k] == v, (tag, k, info[k], v)


def after_append(ctx, oracle, m, tag):
    """One query of each form and one 16-query batch against the oracle over the concatenated columns; the first scan rebuilds a
    dropped run.  The forms: with a key histogram that describes the table (after a load or a growth: m.dirty false) the sparse
    query is keyed on the 1-byte key and the mid and old ones dense; after an in-place append or a touch the histogram is stale and
    the form goes by the live fraction of the scan before: while the sparse query finds under 8 % live, keyed 1-byte, then the mid
    query keyed on the 2-byte key (it lies below the fine key's base), then dense twice."""
    s, e, u, d = m.cols
    m.scan()
    qs = (oc.sparse(oc.ALL), oc.sparse(oc.ALL & ~oc.bit(oc.FILL)), oc.mid(oc.ALL), oc.old(oc.ALL & ~oc.bit(oc.FILL)), oc.sparse(oc.bit(1)))
    if m.dirty:   # ordered_keyed_form: keyed where the scan before found under 8 % of the rows live; the 1-byte key from its base up
        frac = [np.count_nonzero(e > q[0]) / e.size for q in qs]
        forms = [None] + [DENSE if frac[k - 1] >= 0.08 else KEYED1 if qs[k][0] == oc.T_NOW else KEYED2 for k in range(1, 5)]
    else:
        forms = (KEYED1, KEYED1, DENSE, DENSE, KEYED1)
    for k, (q, form) in enumerate(zip(qs, forms)):
        ctx.set_disciplines(q[2], oc.D)
        want = oracle.scan(s, e, u, d, m.n_users, *q)
        same(ctx.scan(q[0], q[1]), want, (tag, k))
        st = ctx.stats()
        assert st["k1_variant"] & 0x2000 and (form is None or st["k1_variant"] == form), (tag, k, hex(st["k1_variant"]), m.dirty)
        assert st["selected"] == want[2].size and st["live"] == np.count_nonzero(e > q[0]), (tag, k, st)
        check_info(ctx, m, (tag, k))
    qs = [(oc.T_NOW + 1000 * i, INT64_MIN, oc.ALL if i % 2 else oc.bit(1)) for i in range(16)]
    batch_on(ctx, oracle, m.cols, m.n_users, qs, (tag, "batch"))
    ctx.set_disciplines(oc.ALL, oc.D)
    same(ctx.scan(oc.T_NOW, INT64_MIN), oracle.scan(s, e, u, d, m.n_users, *oc.sparse(oc.ALL)), (tag, "closing sparse scan"))


@pytest.mark.parametrize("name", oc.APPEND_CASES)
def test_append_cases(pie, oracle, name):
    tab = oc.append_table()
    m = oc.RunModel(tab.cols, oc.APPEND_U)
    with loaded(pie.PieScan(0), tab) as ctx:
        after_append(ctx, oracle, m, (name, "fresh"))
        for i, (s, e, u, d, n_users, want) in enumerate(oc.fresh_model()[1] + oc.append_case(name)):
            ctx.append_rows(s, e, u, d, n_users)
            assert m.append(s, e, u, d, n_users) == want, (name, i)
            check_info(ctx, m, (name, i, want))
            after_append(ctx, oracle, m, (name, i, want))
        if name == "mirror":   # the 200 rows the insert shifted and the inserted row: touch, tombstone, revive — mirrored through pos[]
            seg = m.segs[oc.A_BIG]
            rows = np.array([r for _, r in seg[-201:]], np.int32)
            assert m.shifted == 200 and int(rows[0]) == m.n - 1
            builds = m.builds
            for k, ne in (("touch", oc.T0 + 5 * oc.HOUR), ("tombstone", INT64_MIN), ("revive", oc.T0 + oc.DAY)):
                ctx.set_end(rows, np.full(rows.size, ne, np.int64))
                m.cols[1][rows] = ne
                m.dirty = True
                after_append(ctx, oracle, m, (name, k))
                assert ctx.table_info()["ordered_builds"] == builds == m.builds


@pytest.mark.parametrize("name", ["shift", "fill", "long-chain"])
def test_append_cases_through_a_create_turn(pie, oracle, name):
    """the same steps as creates of one pie_session_turn with pie_set_turn_ordered on: k_ord_stage_rows, then k_ord_append.  The
    context first holds a table of the capacity the append cases have after their growing append (twice the rows, 16 users), so the
    model starts where oc.fresh_model() leaves it, one build earlier."""
    from turn_model import make_ops
    from session_turn_model import CREATE
    tab = oc.append_table()
    cols = [np.concatenate([a, b]) for a, b in zip(tab.cols, oc.fresh_model()[1][0][:4])]
    n = cols[0].size
    m = oc.RunModel(cols, oc.APPEND_U + 1)
    m.cap_rows, m.cap_users = 2 * (n - 1), 2 * oc.APPEND_U
    rng = np.random.default_rng(5)
    with pie.PieScan(0) as ctx:
        ctx.set_ordered_run(2)
        ctx.set_turn_ordered(1)
        z = np.zeros(m.cap_rows, np.int64)
        ctx.load_columns(z, z, z.astype(np.int32), z.astype(np.int32), m.cap_users)
        ctx.load_columns(*cols, oc.APPEND_U + 1)
        ctx.token_set(rng.integers(0, 2 ** 64, (n, 2), dtype=np.uint64))
        after_append(ctx, oracle, m, (name, "fresh"))
        ref, _ = oc.fresh_model()
        assert m.n_ord == ref.n_ord and np.array_equal(m.uoff, ref.uoff)
        for i, (s, e, u, d, n_users, want) in enumerate(oc.append_case(name)):
            if n_users > m.cap_users:
                break                                                   # the growth step is pie_append_rows' own
            ops = make_ops(rng.integers(0, 2 ** 64, (s.size, 2), dtype=np.uint64), s, CREATE, e)
            out = ctx.session_turn(ops, u, d, n_users)
            assert np.array_equal(out["row"], m.n + np.arange(s.size)), (name, i)
            assert m.append(s, e, u, d, n_users) == want, (name, i)
            check_info(ctx, m, (name, i, want))
            after_append(ctx, oracle, m, (name, i, want))
