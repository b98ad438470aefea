"""GPU: the single scan's general path (fused / unfused K2, k_scatter, k_copy_direct, k_sort_tiny, k_sort_small, k_sort_segments,
k_merge_pass and the host's slot growth and hot-set refresh), every route at the bucket sizes where it branches, bit for bit
against the oracle.  The tables are designed (tests/scan_order_cases.py; test_scan_order_cases_cpu.py shows what they plant): one
user per bucket size on both sides of every size class, wave groups of 9 .. 16-row buckets, exactly 32 and 40 users above the
hot threshold, rows clustered by user, and six start patterns with INT64_MIN / INT64_MAX rows.  Stages of one table let a user
pass through several size classes in successive scans of one context, so the same bucket meets the capacity, the hot set and the
launch configuration an earlier, larger query left behind.

Expected values come from the oracle only.  The route counters of pie_stats (n_small, n_over, n_hot, direct_shift, n_segments,
n_big) are compared with the host's decisions restated in scan_order_cases.Routes, and the last test of the file fails unless
the cases together saw every route condition.  The ordered run is switched off: the general path is the subject."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_order_cases as soc  # noqa: E402

pytestmark = pytest.mark.gpu

# (a): the three full scans are the point (every bucket above 16 rows overflows 16 slots; the slots have grown; hot candidates are
# known), then the reduced stages run with the capacity and the hot set a larger query left
STAGES_A = ("full", "full", "full", "16", "4", "17", "512", "513", "4096", "65536", "full")
SEEN = set()   # the route conditions the cases of this file reached (test_cases_reached_every_route)


@functools.lru_cache(maxsize=None)
def wanted(t0, name, pattern, stage):
    """The oracle's answer of one stage of one table: computed once, shared, never changed."""
    import oracle_py
    tab = soc.table(t0, name, pattern)
    res = oracle_py.scan(*tab.cols, tab.U, *soc.query(t0, soc.STAGE[stage]))
    for a in res:
        a.setflags(write=False)
    return res


def loaded(pie, tab):
    ctx = pie.PieScan(0)
    ctx.load_columns(*tab.cols, tab.U)
    ctx.set_disciplines(soc.ALL, soc.D)
    ctx.set_ordered_run(0)
    return ctx


def same_result(got, want, tag):
    for name, a, b in zip(("counts", "offsets", "idx"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), (tag, name)


def segments_of(counts):
    c = np.asarray(counts, np.int64)
    return int(np.count_nonzero((c > soc.SMALL_MAX) & (c <= soc.SEG_MAX)) + ((c[c > soc.SEG_MAX] + soc.SEG_MAX - 1) // soc.SEG_MAX).sum())


def check(ctx, got, want, tag, routes=None, stage="full", pinned=None):
    """The result bit for bit, the statistics every scan must report, and (routes given) the counters of the route it took."""
    same_result(got, want, tag)
    st = ctx.stats()
    counts = want[0]
    assert st["selected"] == want[2].size and st["max_bucket"] == int(counts.max(initial=0)), (tag, st)
    assert st["n_big"] == int(np.count_nonzero(counts > soc.SEG_MAX)) and st["n_segments"] == segments_of(counts), (tag, st)
    if pinned is not None:
        assert st["k1_variant"] == pinned, (tag, hex(st["k1_variant"]))
    if routes is None:
        return st
    exp = routes.scan(counts, st["k1_variant"])
    for key in ("direct_shift", "n_hot", "n_over", "n_small"):
        if key in exp:
            assert st[key] == exp[key], (tag, key, st, exp)
    SEEN.add(("direct_shift", st["direct_shift"]))
    if st["direct_shift"] == 9 and st["n_over"] > 0:
        SEEN.add("staged records beside grown slots")
    if st["n_hot"] == soc.HOT_MAX:
        SEEN.add("n_hot 32")
    if stage != "full" and exp["hot_in_force"] != 0 and st["n_over"] > 0 and int(counts.max(initial=0)) <= soc.TINY_MAX:
        SEEN.add("tiny buckets of hot users")
    if stage != "full" and exp["hot_in_force"] != 0:
        SEEN.add("reduced stage under a hot set")
    return st


def run_stages(pie, tab, t0, stages, tag, pinned=None, direct=True):
    ctx = loaded(pie, tab)
    routes = soc.Routes(direct=direct)
    out = []
    try:
        for i, stage in enumerate(stages):
            now, cutoff, _ = soc.query(t0, soc.STAGE[stage])
            got = ctx.scan(now, cutoff)
            out.append(check(ctx, got, wanted(t0, tab.name, tab.pattern, stage), (tag, i, stage), routes, stage, pinned))
    finally:
        ctx.close()
    return out


def assert_three_full_scans(tab, stats):
    """Part 4 of the design: what the first three full scans of a table with buckets above 512 rows must report."""
    one, two, three = stats[:3]
    sizes = tab.sizes
    assert one["direct_shift"] == 4 and three["direct_shift"] == 9
    assert one["n_over"] == int(np.count_nonzero(sizes > 16)) > 0
    assert three["n_small"] == int(np.count_nonzero((sizes > 16) & (sizes <= 512)))
    assert three["n_hot"] > 0
    if not (three["k1_variant"] & 0x40):   # no hot set in force: only the buckets no slot capacity holds have staged records
        assert three["n_over"] == int(np.count_nonzero(sizes > 512))


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("pattern", soc.PATTERNS)
@pytest.mark.parametrize("name", ["sizes", "hot", "hot40"])
def test_default_configuration(pie, oracle, name, pattern):
    tab = soc.table(oracle.T0_MS, name, pattern)
    stats = run_stages(pie, tab, oracle.T0_MS, STAGES_A, "default %s %s" % (name, pattern))
    assert_three_full_scans(tab, stats)
    if name != "sizes":
        assert stats[2]["n_hot"] == 32   # 32 candidates, and 40 clipped at kHotMax
        # regression: a hot user whose bucket the query leaves 1 .. 16 rows (or none) is read from the staged records
        assert stats[3]["n_over"] == stats[3]["n_small"] and stats[3]["n_over"] in ((31,) if name == "hot" else (31, 32))


@pytest.mark.parametrize("pattern", ["two", "rand5"])
@pytest.mark.parametrize("name", ["mids", "clustered", "clustered_desc"])
def test_default_configuration_other_tables(pie, oracle, name, pattern):
    tab = soc.table(oracle.T0_MS, name, pattern)
    stats = run_stages(pie, tab, oracle.T0_MS, STAGES_A, "default %s %s" % (name, pattern))
    if name == "mids":
        assert all(s["n_small"] == s["n_over"] == s["n_segments"] == 0 and s["direct_shift"] == 4 for s in stats)
        SEEN.add("mids: 6 and 7 buckets of 9..16 rows in one wave")
    else:
        assert_three_full_scans(tab, stats)


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("pattern", ["two", "rand5"])
@pytest.mark.parametrize("env", [{"PIE_ORDER_BLOCK": "512"}, {"PIE_ORDER_BLOCK": "1024"}, {"PIE_FUSED_ORDER": "0"}])
@pytest.mark.parametrize("name", ["sizes", "mids"])
def test_k2_configurations(pie, oracle, monkeypatch, name, env, pattern):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tab = soc.table(oracle.T0_MS, name, pattern)
    stats = run_stages(pie, tab, oracle.T0_MS, STAGES_A, "%s %s %s" % (env, name, pattern))
    if name == "sizes":
        assert_three_full_scans(tab, stats)


# ---------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("pattern", ["two", "rand5"])
@pytest.mark.parametrize("form", [0x03, 0x43, 0x85, 0xC5, 0x485, 0x4C5, 0xC85, 0xCC5])
def test_pinned_k1_forms(pie, oracle, monkeypatch, form, pattern):
    """Every K1 form that produces the ranks K2 .. K4 consume; the aggregated ones (0xC5, 0x4C5, 0xCC5) stage the hot users' rows
    with block-relative ranks, so the reduced stages find a hot set with tiny buckets."""
    monkeypatch.setenv("PIE_K1_VARIANT", hex(form))
    tab = soc.table(oracle.T0_MS, "sizes", pattern)
    stats = run_stages(pie, tab, oracle.T0_MS, STAGES_A, "form %#x %s" % (form, pattern), pinned=form)
    assert_three_full_scans(tab, stats)
    if (form & 0x44) == 0x44:
        hot = int(np.count_nonzero(tab.sizes > int(tab.sizes.sum()) // 256))
        assert stats[2]["n_over"] == int(np.count_nonzero(tab.sizes > 512)) and hot == 13   # (the hot users are among them)
        assert stats[3]["n_over"] == stats[3]["n_small"] == hot and stats[3]["max_bucket"] == 16


# ---------------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("pattern", ["two", "rand5"])
@pytest.mark.parametrize("name", ["sizes", "hot"])
def test_two_scans_in_flight(pie, oracle, name, pattern):
    """begin, begin, finish, read, finish, read over consecutive pairs of the stage list: K2 of the first rides in the second's
    launch, and the second begins before the first has chosen the capacity and the hot set."""
    t0 = oracle.T0_MS
    tab = soc.table(t0, name, pattern)
    ctx = loaded(pie, tab)
    try:
        for i in range(len(STAGES_A) - 1):
            pair = STAGES_A[i: i + 2]
            for stage in pair:
                ctx.scan_begin(*soc.query(t0, soc.STAGE[stage])[:2])
            for stage in pair:
                m = ctx.scan_finish()
                want = wanted(t0, name, pattern, stage)
                assert m == want[2].size
                check(ctx, ctx.read_results(), want, ("in flight", name, pattern, i, stage))
    finally:
        ctx.close()


@pytest.mark.parametrize("name,pair", [("sizes", ("full", "16")), ("sizes", ("16", "full")), ("mids", ("full", "4")), ("hot", ("16", "513"))])
def test_two_packed_scans_in_flight(pie, oracle, name, pair):
    """The same through scan_begin_packed: the message words equal the message packed from the oracle's answer; a scan with a
    bucket above 16 rows is not ready on return (a pack kernel follows), one without is."""
    t0 = oracle.T0_MS
    tab = soc.table(t0, name, "rand5")
    wants = [wanted(t0, name, "rand5", s) for s in pair]
    u_pad = tab.U + 3
    ctx = loaded(pie, tab)
    bufs = []
    try:
        for w in wants:
            bufs.append(ctx.host_alloc(u_pad + 2 + w[2].size + 5))
            bufs[-1][0][:] = -7
        for rounds in range(2):   # the second round runs with the capacity the first one asked for
            for stage, w, (h, dev, _) in zip(pair, wants, bufs):
                ctx.scan_begin_packed(*soc.query(t0, soc.STAGE[stage])[:2], dev, u_pad, w[2].size + 5)
            for stage, w in zip(pair, wants):
                m, ready = ctx.scan_finish_packed()
                assert m == w[2].size
                assert ready == (int(w[0].max()) <= soc.TINY_MAX), (name, stage, rounds, "ready")
                if not ready:
                    SEEN.add("message packed behind the sorts")
            ctx.synchronize()
            for stage, w, (h, _, _) in zip(pair, wants, bufs):
                m = w[2].size
                assert np.array_equal(h[: tab.U + 1], w[1].astype(np.int32)) and np.all(h[tab.U + 1: u_pad + 2] == m), (name, stage, rounds)
                assert np.array_equal(h[u_pad + 2: u_pad + 2 + m], w[2]), (name, stage, rounds, "rows")
                assert np.all(h[u_pad + 2 + m:] == -7)
                h[:] = -7
    finally:
        for _, _, addr in bufs:
            ctx.host_free(addr)
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- (e)
def test_staged_route_without_direct_slots(pie, oracle):
    """8 388 609 users: one more than direct slots are carried for, so every record is staged and k_sort_tiny orders the tiny
    buckets from bkt; the last user holds a 17-row bucket."""
    tab = soc.table(oracle.T0_MS, "staged", "two")
    stats = run_stages(pie, tab, oracle.T0_MS, ("full", "full", "16", "full"), "staged", direct=False)
    assert all(s["direct_shift"] == 0 for s in stats)
    assert stats[0]["n_over"] == int(np.count_nonzero(tab.sizes > 16)) and stats[2]["n_over"] == 0
    SEEN.add("staged route")


# ---------------------------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("pattern", soc.PATTERNS)
@pytest.mark.parametrize("name", ["hot", "hot40"])
def test_hot_set_with_tiny_buckets(pie, oracle, name, pattern):
    """full, full, reduced, reduced, full: the second full scan reports the candidates (exactly 32, or 40 clipped at 32), the
    first reduced scan runs with them as its hot set (their 0 .. 16 rows are staged and listed), the second without."""
    tab = soc.table(oracle.T0_MS, name, pattern)
    stats = run_stages(pie, tab, oracle.T0_MS, ("full", "full", "16", "16", "full"), "hot %s %s" % (name, pattern))
    assert stats[0]["n_hot"] == 0 and stats[1]["n_hot"] == 32
    assert (stats[1]["k1_variant"] & 0x44) == 0x44 and (stats[2]["k1_variant"] & 0x44) == 0x44, [hex(s["k1_variant"]) for s in stats]
    # regression: a hot user's small bucket is read from the staged records, not from its slots
    assert stats[2]["n_over"] == stats[2]["n_small"] and stats[2]["n_over"] in ((31,) if name == "hot" else (31, 32))
    assert stats[3]["n_over"] == 0 and stats[3]["n_small"] == 0


# ---------------------------------------------------------------------------------------------------------------- (g)
@pytest.mark.parametrize("pattern", ["two", "rand5"])
@pytest.mark.parametrize("form", [None, 0x43])
@pytest.mark.parametrize("name", ["clustered", "clustered_desc"])
def test_rows_clustered_by_user(pie, oracle, monkeypatch, name, form, pattern):
    if form is not None:
        monkeypatch.setenv("PIE_K1_VARIANT", hex(form))
    tab = soc.table(oracle.T0_MS, name, pattern)
    stats = run_stages(pie, tab, oracle.T0_MS, ("full", "full", "full", "16", "513", "full"), "%s %s %s" % (name, form, pattern), pinned=form)
    if form is None:   # one dense scan that finds the rows clustered, and the streaming form aggregates from the next one on
        assert stats[0]["k1_variant"] == 0x03 and stats[1]["k1_variant"] == 0x43, [hex(s["k1_variant"]) for s in stats]
        SEEN.add("0x43 chosen")


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_stats_struct_size_is_append_only(pie, oracle):
    """A caller built against pie_stats without the route counters gets the fields it knows and nothing behind them."""
    import ctypes as C
    from sph_pie_amd import binding
    old = binding.PieStats.n_small.offset
    assert C.sizeof(binding.PieStats) == old + 16 == 112
    tab = soc.table(oracle.T0_MS, "mids", "two")
    ctx = loaded(pie, tab)
    try:
        ctx.scan(*soc.query(oracle.T0_MS, soc.STAGE["full"])[:2])
        new = ctx.stats()
        buf = (C.c_uint8 * C.sizeof(binding.PieStats))()
        C.memset(buf, 0xAB, len(buf))
        st = C.cast(buf, C.POINTER(binding.PieStats))
        st.contents.struct_size = old
        assert ctx._lib.pie_stats_get(ctx._ctx, st) == 0
        assert st.contents.struct_size == old and st.contents.selected == new["selected"] and st.contents.max_bucket == new["max_bucket"]
        assert bytes(buf[old:]) == b"\xab" * 16
        st.contents.struct_size = old + 8
        assert ctx._lib.pie_stats_get(ctx._ctx, st) == -1
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_cases_reached_every_route():
    """Fails unless the cases above saw every route condition (a change that stops reaching one must not pass unnoticed)."""
    need = {("direct_shift", 4), ("direct_shift", 9), ("direct_shift", 0), "staged records beside grown slots", "n_hot 32",
            "reduced stage under a hot set", "tiny buckets of hot users", "mids: 6 and 7 buckets of 9..16 rows in one wave",
            "message packed behind the sorts", "staged route", "0x43 chosen"}
    assert need <= SEEN, sorted(map(str, need - SEEN))
