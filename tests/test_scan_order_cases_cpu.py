"""CPU: the designed tables of tests/scan_order_cases.py plant what they claim, shown with the oracle alone, so that a pass of
tests/test_gpu_scan_order_paths.py means something.  The expected order is also computed a second way (np.lexsort((row, start))
per user) and compared with oracle.scan: the reference itself is cross-checked here and not on the GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_order_cases as soc  # noqa: E402

NAMES = ("sizes", "clustered", "clustered_desc", "mids", "hot", "hot40")


def stage_answers(oracle, tab):
    return [oracle.scan(*tab.cols, tab.U, *soc.query(oracle.T0_MS, k)) for k in range(len(soc.STAGE_ROWS))]


@pytest.mark.parametrize("name", NAMES)
def test_stages_select_the_designed_prefixes(oracle, name):
    """Every stage: every user's count is clip(STAGE_ROWS[k] - skip, 0, size), the selected rows are designed rows (never filler),
    they are the FIRST rows of the bucket in row order, and the last stage selects every designed row."""
    tab = soc.table(oracle.T0_MS, name, "two")
    start, end, user, disc = tab.cols
    assert start.size < 10 ** 6
    assert np.array_equal(np.bincount(user[tab.designed], minlength=tab.U), tab.sizes)
    for k, (counts, offsets, idx) in enumerate(stage_answers(oracle, tab)):
        assert np.array_equal(counts, soc.expected_counts(tab, k)), (name, k)
        assert np.all(tab.designed[idx]), (name, k, "a filler row was selected")
        sel = np.zeros(start.size, bool)
        sel[idx] = True
        for u in np.nonzero(tab.sizes)[0].tolist():
            mine = np.nonzero(tab.designed & (user == u))[0]
            assert np.array_equal(np.nonzero(sel[mine])[0], np.arange(counts[u])), (name, k, u)
    assert idx.size == int(tab.sizes.sum())
    if name == "sizes":
        assert int(tab.sizes[1::3][: len(soc.SIZES)].sum()) == soc.SIZES_DESIGNED
        assert tab.sizes[1::3][: len(soc.SIZES)].tolist() == list(soc.SIZES) and tab.U % 64 != 0


def test_stage_list_holds_the_sizes_the_routes_branch_at():
    assert {4, 16, 17, 512, 513, 4096, soc.ALL_ROWS} <= set(soc.STAGE_ROWS) and soc.STAGE_ROWS[-1] == soc.ALL_ROWS
    assert list(soc.STAGE_ROWS) == sorted(soc.STAGE_ROWS)
    # the merge boundary: one pass up to 16 tiles of the largest bucket, two from 16 tiles and a row on
    assert 16 * soc.SEG_MAX in soc.SIZES and 16 * soc.SEG_MAX + 1 in soc.SIZES and 16 * soc.SEG_MAX in soc.STAGE_ROWS


def test_mids_wave_groups(oracle):
    tab = soc.table(oracle.T0_MS, "mids", "two")
    mid = (tab.sizes > 8) & (tab.sizes <= 16)
    per_group = np.bincount(np.nonzero(mid)[0] // 64, minlength=6).tolist()
    assert per_group == [6, 7, 64, 0, 0, 1], per_group
    assert mid[tab.U - 1] and tab.U % 64 != 0 and all(tab.U % b for b in (256, 512, 1024))
    assert int(tab.sizes.max()) <= 16
    assert {9, 16} <= set(tab.sizes[:64].tolist()) and {9, 16} <= set(tab.sizes[128:192].tolist())


@pytest.mark.parametrize("name,n_above", [("hot", 32), ("hot40", 40)])
def test_hot_tables(oracle, name, n_above):
    tab = soc.table(oracle.T0_MS, name, "two")
    full = oracle.scan(*tab.cols, tab.U, *soc.query(oracle.T0_MS, soc.STAGE["full"]))
    m = int(full[2].size)
    assert m >= 65536 and m < 0.1 * tab.cols[0].size   # (under a tenth of the table: the adaptive choice is a liveness-first form)
    above = np.nonzero(full[0] > m // 256)[0]
    assert above.size == n_above and (n_above == 32 or n_above >= 33)
    assert above[-1] == tab.U - 1, "a user above the threshold is the last of the table"
    assert int(full[0].max()) * 64 > m
    reduced = oracle.scan(*tab.cols, tab.U, *soc.query(oracle.T0_MS, soc.STAGE["16"]))[0]
    assert int(reduced[above].max()) == 16 and int(np.count_nonzero(reduced[above] == 0)) == 1
    assert set(reduced[above].tolist()) == set(range(17))
    # far from the threshold on both sides: which users are candidates does not hang on one row
    assert int(full[0][above].min()) >= 2 * (m // 256) and int(np.delete(full[0], above).max()) * 4 <= m // 256 * 3


# (the clustered tables are the sizes table in another row order, and the GPU test scans them under two patterns only)
@pytest.mark.parametrize("name,pattern", [(n, p) for n in NAMES for p in soc.PATTERNS if not n.startswith("clustered") or p in ("two", "rand5")])
def test_patterns_exercise_the_sort_and_hold_the_extremes(oracle, name, pattern):
    """Full stage: every bucket of two rows or more holds a pair of equal starts or an inversion relative to row order; every
    bucket of 17 rows or more holds selected INT64_MAX and INT64_MIN rows.  Reduced stages: the same for every bucket of 17
    designed rows or more of which the stage selects four or more (rows 1 .. 3 carry the extremes)."""
    tab = soc.table(oracle.T0_MS, name, pattern)
    start = tab.cols[0]
    for k in (soc.STAGE["full"], soc.STAGE["16"], soc.STAGE["4"]):
        counts, offsets, idx = oracle.scan(*tab.cols, tab.U, *soc.query(oracle.T0_MS, k))
        for u in np.nonzero(counts >= 2)[0].tolist():
            if k != soc.STAGE["full"] and (tab.sizes[u] <= 16 or counts[u] < 4):
                continue
            s = start[np.sort(idx[offsets[u]: offsets[u + 1]])]   # the bucket in row order
            assert np.any(s[1:] <= s[:-1]), (name, pattern, k, u, "already in order, all keys distinct")
            if tab.sizes[u] > 16 and counts[u] >= 4:
                assert np.count_nonzero(s == soc.INT64_MAX) >= 2 and np.count_nonzero(s == soc.INT64_MIN) >= 1, (name, pattern, k, u)
            if k == soc.STAGE["full"] and tab.sizes[u] > 16:
                assert s[-1] == soc.INT64_MAX and s[-2] == soc.INT64_MIN


@pytest.mark.parametrize("name,pattern", [("sizes", "rand5"), ("sizes", "equal"), ("clustered_desc", "two"), ("mids", "rand5"),
                                          ("hot40", "organ"), ("hot", "desc"), ("sizes", "asc")])
def test_oracle_equals_lexsort_per_user(oracle, name, pattern):
    tab = soc.table(oracle.T0_MS, name, pattern)
    for k in range(len(soc.STAGE_ROWS)):
        want = oracle.scan(*tab.cols, tab.U, *soc.query(oracle.T0_MS, k))
        got = soc.numpy_answer(oracle.T0_MS, tab, k)
        for a, b, what in zip(got, want, ("counts", "offsets", "idx")):
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, pattern, k, what)


def test_staged_table_keeps_the_users_and_adds_the_last(oracle):
    tab = soc.table(oracle.T0_MS, "staged", "two")
    base = soc.table(oracle.T0_MS, "sizes", "two")
    assert tab.U == soc.STAGED_USERS == 8388608 + 1
    assert np.array_equal(tab.sizes[: base.U], base.sizes) and tab.sizes[tab.U - 1] == 17 and int(tab.sizes[base.U: tab.U - 1].sum()) == 0
    for k in (soc.STAGE["full"], soc.STAGE["16"]):
        counts, _, idx = oracle.scan(*tab.cols, tab.U, *soc.query(oracle.T0_MS, k))
        assert np.array_equal(counts, soc.expected_counts(tab, k)) and np.all(tab.designed[idx])


def test_route_model_on_the_sizes_table():
    """The restated host logic (soc.Routes) gives the route conditions the GPU test asks of the first three full scans."""
    sizes = soc.sizes_layout()
    r = soc.Routes()
    one, two, three = (r.scan(sizes, 0x03) for _ in range(3))
    assert one["direct_shift"] == 4 and one["n_over"] == int(np.count_nonzero(sizes > 16)) and one["n_hot"] == 0
    assert two["direct_shift"] == 9 and three["direct_shift"] == 9
    assert three["n_over"] == int(np.count_nonzero(sizes > 512)) and three["n_hot"] == int(np.count_nonzero(sizes > int(sizes.sum()) // 256)) == 13
    assert three["n_small"] == int(np.count_nonzero((sizes > 16) & (sizes <= 512)))
    assert three["n_big"] == 5 and three["n_segments"] == int(np.count_nonzero((sizes > 512) & (sizes <= 4096))) + 2 + 2 + 3 + 16 + 17
