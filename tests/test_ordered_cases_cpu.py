"""CPU: the designed tables of tests/ordered_cases.py plant what they claim — shown with the oracle and the layout model alone.
For every table and query the oracle's answer equals the answer the claimed positions give through the model (layout, shuffle
and claim at once); then each table's own promises are checked on the positions.  The large table's oracle answers are left to
the GPU file (4 M rows per query); here its claims are checked with numpy on the positions."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ordered_cases as oc  # noqa: E402
import table_model as tm  # noqa: E402


def small_cases():
    return [(oc.uoff_edges(), {k: f(m) for k, m in oc.uoff_edges_queries().items() for f in (oc.sparse, oc.old)}),
            (oc.chunk_counts(), {"all": oc.sparse(oc.bit(oc.G_A, oc.G_B)), "alternating": oc.sparse(oc.bit(oc.G_A)),
                                 "none": oc.sparse(oc.bit(oc.G_NONE)), "dense": oc.old(oc.bit(oc.G_A))}),
            (oc.tile_slices(), {"mid": oc.mid(oc.bit(oc.G_DENSE, oc.G_AMB)), "old": oc.old(oc.bit(oc.G_DENSE))}),
            (oc.alternating(), {f"{f.__name__} {g}": f(oc.bit(g)) for g in oc.G_ALT for f in (oc.sparse, oc.old)})]


def keyed_share(tab, now):
    """the share ordered_keyed_form compares with 8 %: rows whose 15-bit key lies in the histogram bin of key(now) or above"""
    end = tab.cols[1]
    base, shift, fbase, fshift = tm.key_params(end)
    vals, cnt = np.unique(end, return_counts=True)
    keys = np.array([tm.key_of(v, base, shift) for v in vals])
    return cnt[(keys >> 3) >= (tm.key_of(now, base, shift) >> 3)].sum() / end.size, (base, shift, fbase, fshift)


def far_below(tab, now):
    """every row ending before `now` has a smaller key than key(now), on both keys: the candidates are the rows ending at or after"""
    end = tab.cols[1]
    base, shift, fbase, fshift = tm.key_params(end)
    below = end[end < now]
    if below.size == 0:
        return True
    top = int(below.max())
    return tm.key_of(top, base, shift) < tm.key_of(now, base, shift) and \
        (now < fbase or tm.key_of(top, fbase, fshift, tm.FINE_KEY_MAX) < tm.key_of(now, fbase, fshift, tm.FINE_KEY_MAX))


@pytest.mark.parametrize("case", range(4), ids=["uoff-edges", "chunk-counts", "tile-slices", "alternating"])
def test_small_tables_plant_their_claims(oracle, case):
    tab, queries = small_cases()[case]
    s, e, u, d = tab.cols
    assert np.array_equal(tab.uoff, oc.run_layout(np.bincount(u, minlength=tab.U), s.size, tab.U)[0])
    assert np.any(np.diff(tab.row_pos) < 0)                                         # row id order is not position order
    share, (_, _, fbase, _) = keyed_share(tab, oc.T_NOW)
    assert np.count_nonzero(e >= oc.T_NOW) <= 0.05 * s.size and share < 0.08 and oc.T_NOW >= fbase and far_below(tab, oc.T_NOW)
    assert keyed_share(tab, oc.T_OLDNOW)[0] == 1.0 and keyed_share(tab, oc.T_MIDNOW)[0] >= 0.08
    for name, q in queries.items():
        want = oracle.scan(s, e, u, d, tab.U, *q)
        got = oc.answer_from_positions(tab, oc.selected_positions(tab, q))
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b), (tab.name, name)


def test_uoff_edges_claims():
    tab = oc.uoff_edges()
    n = tab.notes
    assert [n[b]["uoff"] for b in oc.UOFF_BOUNDS] == [64, 512, 4096, tab.n_ord - tab.spare]
    assert np.all(tab.counts[:4] == 0) and np.all(tab.counts[5:7] == 0) and np.all(tab.counts[-3:] == 0)
    assert any(int(x) & 63 == 63 for x in tab.uoff[: tab.U]) and any(int(x) & 63 == 0 for x in tab.uoff[1: tab.U])
    assert np.all(tab.pos_disc[tab.uoff[1: tab.U + 1] - 1] == -1)                    # uoff[u] - 1 is always a spare slot
    for bi, b in enumerate(oc.UOFF_BOUNDS):
        q = n[b]["uoff"]
        for unit in (oc.CHUNK, oc.TILE):
            lo, hi = q // unit * unit, q // unit * unit + unit
            sel = {v: oc.selected_positions(tab, oc.sparse(oc.bit(oc.uoff_group(bi, vi)))) for vi, v in enumerate(oc.UOFF_VARIANTS)}
            inside = {v: p[(p >= lo) & (p < hi)] for v, p in sel.items()}
            assert inside["none"].size == 0 and sel["none"].size == 1
            assert np.all(inside["before"] < q) and np.all(inside["after"] >= q)
            if n[b]["before"] >= 4:
                assert sel["before"].size == 2 and np.any(sel["both"] < q)
            if n[b]["after"] >= 4:
                assert sel["after"].size == 2 and np.any(sel["both"] >= q)
            if n[b]["row_at"]:
                assert q in sel["at"]
    assert n[64]["row_at"] and n[4096]["row_at"] and n["last"]["before_in_chunk"] >= 4 and n[512]["before"] >= 4


def test_chunk_counts_claims():
    tab = oc.chunk_counts()
    cand = oc.per_unit(oc.candidate_positions(tab, oc.sparse(0)), oc.CHUNK, tab.n_ord)
    want = np.zeros_like(cand)
    for ch, k in tab.notes["chunks"].items():
        want[ch] = k
    assert np.array_equal(cand, want) and set(oc.CHUNK_COUNTS) <= set(cand.tolist())
    every = oc.selected_positions(tab, oc.sparse(oc.bit(oc.G_A, oc.G_B)))
    half = oc.selected_positions(tab, oc.sparse(oc.bit(oc.G_A)))
    assert oc.selected_positions(tab, oc.sparse(oc.bit(oc.G_NONE))).size == 0
    assert every.size == cand.sum() - 1                                              # all but the candidate that ends at `now`
    a, b = tab.notes["amb"]
    assert tab.pos_end[a] == oc.T_NOW and tab.pos_end[b] == oc.T_NOW + 1 and a not in every and b in every
    c = oc.candidate_positions(tab, oc.sparse(0))
    assert np.array_equal(np.sort(np.concatenate([half, [a] if tab.pos_disc[a] == oc.G_A else []])).astype(np.int64), c[tab.pos_disc[c] == oc.G_A])
    in40 = c[c // oc.CHUNK == tab.notes["last64"]]
    assert in40.size == 64 and in40[-1] == 41 * oc.CHUNK - 1                         # the 64th candidate is the chunk's last position
    last = (tab.n_ord - 1) // oc.CHUNK
    assert tab.n_ord % oc.CHUNK and cand[last] == 3


def test_tile_slices_claims():
    tab = oc.tile_slices()
    q = oc.mid(oc.bit(oc.G_DENSE, oc.G_AMB))
    sel, live = oc.selected_positions(tab, q), oc.live_positions(tab, q)
    per_tile = oc.per_unit(sel, oc.TILE, tab.n_ord)
    assert per_tile[1] == oc.TILE
    quarter = oc.per_unit(sel, 1024, tab.n_ord)[8:12]
    may = oc.per_unit(oc.candidate_positions(tab, q), 64, tab.n_ord)
    assert quarter[0] == 1024 and quarter[1] == 0 and np.all(may[2 * 64 + 16: 2 * 64 + 32] == 0)
    s2 = oc.per_unit(sel, 64, tab.n_ord)[2 * 64 + 32: 2 * 64 + 48]
    assert np.all(s2[0::2] == 22) and np.all(s2[1::2] == 0) and np.all(may[2 * 64 + 32: 2 * 64 + 48][1::2] == 0)
    a, b = tab.notes["amb"]
    assert may[a // 64] == 1 and may[b // 64] == 1 and b & 63 == 63 and a not in live and b in sel and quarter[3] == 1
    assert np.all(tab.notes["last_rows"] >= tab.n_ord // 64 * 64) and np.all(np.isin(tab.notes["last_rows"], sel)) and tab.n_ord % 64


def test_alternating_claims():
    tab = oc.alternating()
    chunks = [set((oc.selected_positions(tab, oc.sparse(oc.bit(g))) // oc.CHUNK).tolist()) for g in oc.G_ALT]
    for k, c in enumerate(chunks):
        assert c and all(x % 3 == k for x in c)
    per = oc.per_unit(oc.selected_positions(tab, oc.sparse(oc.bit(*oc.G_ALT))), oc.CHUNK, tab.n_ord)
    assert per[9] == 64 and per[16] == 65


def test_union_tables_claims(oracle):
    tab = oc.union_chunks()
    s, e, u, d = tab.cols
    assert np.count_nonzero(e >= oc.T_NOW) <= 0.05 * s.size and far_below(tab, oc.T_NOW)
    for nq in (16, 33):
        qs = oc.union_chunks_queries(nq)
        union = np.unique(np.concatenate([oc.selected_positions(tab, q) for q in qs]))
        staged = oc.per_unit(union, oc.CHUNK, tab.n_ord)                               # records a chunk stages: rows any query selects
        want = np.zeros_like(staged)
        for ch, k in oc.UNION_CHUNKS.items():
            want[ch] = k
        assert np.array_equal(staged, want) and {8, 9, 64, 65, 512} <= set(staged.tolist())
        assert any(oc.selected_positions(tab, q).size == 0 for q in qs)
    for q in oc.union_chunks_queries(4):
        got = oc.answer_from_positions(tab, oc.selected_positions(tab, q))
        for a, b in zip(got, oracle.scan(s, e, u, d, tab.U, *q)):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    cap = oc.union_cap()
    ucap = oc.batch_ucap(cap.cols[0].size, cap.U)
    assert oc.selected_positions(cap, oc.sparse(oc.bit(oc.G_U1, oc.G_U2))).size == ucap == 12288
    assert oc.selected_positions(cap, oc.sparse(oc.bit(oc.G_U1, oc.G_U2, oc.G_U3))).size == ucap + 1
    assert keyed_share(cap, oc.T_NOW)[0] < 0.10 and far_below(cap, oc.T_NOW)           # classify_queries keeps the queries in the batch


@pytest.fixture(scope="module")
def large():
    return oc.large(256)


def test_large_table_claims(large):
    tab, n = large, large.notes
    W, n_chunks = n["W"], n["n_chunks"]
    assert W == 8192 and n_chunks == W + 300 and n_chunks == (tab.n_ord + 511) // 512 and tab.n_ord < oc.MAX_LARGE_POSITIONS
    assert np.array_equal(tab.uoff, oc.run_layout(np.bincount(tab.cols[2], minlength=tab.U), tab.cols[0].size, tab.U)[0])
    assert np.count_nonzero(tab.cols[1] >= oc.T_NOW) <= 0.05 * tab.cols[0].size and 1000 < tab.U < 4000
    assert (n_chunks + 1023) // 1024 == 9 and (tab.n_ord + 4095) // 4096 > 1024      # nine keyed groups, two dense ones
    # which wave owns which chunks: grid = min((n_chunks + 3) // 4, n_cus * m) blocks of four waves, chunks dealt round robin
    for m, most in ((8, 2), (6, 2), (4, 3), (3, 3)):
        waves = 4 * min((n_chunks + 3) // 4, 256 * m)
        assert -(-n_chunks // waves) == most
    assert -(-n_chunks // (4 * 256 * 1)) == 9 and n_chunks // (4 * 256) == 8          # PIE_ORD_GRID=1: eight or nine chunks a wave
    cand = oc.per_unit(oc.candidate_positions(tab, oc.sparse(0)), oc.CHUNK, tab.n_ord)
    sel = oc.per_unit(oc.selected_positions(tab, oc.sparse(oc.LARGE_QUERIES["waves"])), oc.CHUNK, tab.n_ord)
    for w, ((s1, c1), (s2, c2)) in oc.WAVE_PLANTS.items():
        assert w + W < n_chunks and (sel[w], cand[w] - sel[w], sel[w + W], cand[w + W] - sel[w + W]) == (s1, c1, s2, c2)
    p = oc.candidate_positions(tab, oc.sparse(0))
    p = p[p // oc.CHUNK == 50 + W]
    assert np.all(tab.pos_disc[p[:58]] == oc.G_WAVE_CAND) and np.all(tab.pos_disc[p[58:]] == oc.G_WAVE)
    groups = np.unique(oc.selected_positions(tab, oc.sparse(oc.LARGE_QUERIES["groups"])) // (oc.CHUNK * oc.GROUP))
    assert groups.tolist() == [0, 2]
    run = oc.per_unit(oc.selected_positions(tab, oc.sparse(oc.LARGE_QUERIES["run"])), oc.CHUNK, tab.n_ord)
    assert np.all(run[2900:3001] > 0) and np.all(run[3001:3072] == 0) and run[3072] > 0 and 3072 % oc.GROUP == 0
    stride = oc.selected_positions(tab, oc.sparse(oc.LARGE_QUERIES["stride"])) // oc.CHUNK
    assert stride.tolist() == list(range(7, n_chunks, 1024)) and stride.size == 9 and np.all(cand[stride] == 1)
    assert sorted(n["bounds"]) == [524288, 4194304]
    bsel = oc.selected_positions(tab, oc.sparse(oc.LARGE_QUERIES["bounds"]))
    for target, u in n["bounds"].items():
        assert tab.uoff[u] == target and target in bsel and np.count_nonzero((bsel < target) & (bsel >= target - 512)) == 2
    with pytest.raises(AssertionError, match="8 M"):
        oc.large(520)


@pytest.mark.parametrize("name", oc.APPEND_CASES)
def test_append_cases_follow_the_model(name):
    m, first = oc.fresh_model()
    assert oc.ord_spare(m.cap_rows, m.cap_users) == 16
    for s, e, u, d, n_users, want in oc.append_case(name):
        before = m.info()
        fill, room = [len(x) for x in m.segs], np.diff(m.uoff)
        got = m.append(s, e, u, d, n_users)
        assert got == want, (name, got, want)
        after = m.info()
        if got == "kept":
            assert after["ordered_positions"] == before["ordered_positions"] and after["ordered_respreads"] == before["ordered_respreads"]
            assert after["ordered_rows"] == before["ordered_rows"] + s.size
        elif got == "respread":
            assert after["ordered_respreads"] == before["ordered_respreads"] + 1 and after["ordered_rows"] == before["ordered_rows"] + s.size
            assert after["ordered_positions"] == int(oc.seg_len(np.array([len(x) for x in m.segs]), 16).sum())
        else:
            assert after["ordered_rows"] == 0
        if name == "shift":
            assert m.shifted == (256 if got == "kept" and s[0] < oc.T0 else 0)
        if name == "fill" and got == "respread":
            assert fill[int(u[0])] == room[int(u[0])]                                 # the segment was exactly full
        if name == "fill" and got == "kept":
            assert fill[int(u[0])] + s.size == room[int(u[0])]                        # exactly the spare slots
        if name == "long-chain":
            a = oc.A_B
            k = s.size
            at = np.nonzero(u == a)[0]
            assert at.size >= 5 and {0, k - 1} <= set(at.tolist()) and all(i in at for i in (63, 64) if i < k)
            assert np.all(d[:64] == a) and np.any(np.diff(s) < 0)
            if k >= 63:
                assert [np.count_nonzero(u == x) for x in (oc.A_17, oc.A_BIG, oc.A_16, 7)] == [1, 2, 3, 4]
        if got == "dropped":
            m.scan()
            assert m.info()["ordered_builds"] == before["ordered_builds"] + 1
        for seg in m.segs:                                                            # every segment stays in (start, row) order
            assert seg == sorted(seg)
