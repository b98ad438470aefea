"""TEST INFRASTRUCTURE — designed tables for the ordered run (sph-pie_amd/csrc/pie_ordered.h and its host side in pie_scan.hip), no GPU.

test_ordered_cases_cpu.py shows with the oracle and the layout model alone that every table plants what it claims;
test_gpu_ordered_paths.py drives the tables through the C ABI and pins the model to the device.

The layout model.  run_layout restates build_ordered: segment u is cnt[u] + cnt[u] // 16 + spare positions long, spare is
ord_spare of the table's capacities (after pie_load_columns into a fresh context: cap_rows = n, cap_users = n_users; after an
append that outgrows either: grow_caps), and the row at position p is the (p - uoff[u])-th row of its user in (start, row) order.
respread_layout restates ord_respread (rows = fill + pend).  RunModel replays k_ord_append on top of them: which rows an append
places, which it leaves to a re-spread, when the run is dropped.

Construction, all tables (Design).  The layout is fixed first; then every position that holds a row gets a discipline and an
`end`, and the rows are dealt to shuffled row ids (row id order is not position order; pairs of rows of one user share a start,
so ties are broken by row).  Filler rows carry discipline FILL and end a hundred (MID) or three hundred (OLD) days before the
sparse `now`; designed rows carry a discipline of their group and, unless said otherwise, end a day after it.  Selection is
steered in two ways so that both forms reach the same positions:
  sparse   now = T_NOW: only designed rows are candidates and live (keyed form); the mask picks groups among them
  old      now = T_OLDNOW, below every `end`: every row is live (dense form, key(now) == 0); the same mask selects the same rows
  mid      now = T_MIDNOW: OLD filler is dead, MID filler live (dense form with dead slices)
Rows ending at exactly `now` (candidates, not live) and `now` + 1 (live) are the ambiguous-key candidates of both outcomes.
The rows ending at or after T_NOW stay at or below 5 % of every table (ordered_keyed_form takes the keyed form below 8 %).

What a claim is.  selected_positions / candidate_positions / live_positions evaluate a query on the POSITION arrays of the design;
answer_from_positions turns the selected positions into (counts, offsets, idx) through the layout.  The CPU test compares that
with the oracle's answer on the shuffled columns — which proves layout, shuffle and claim at once — and then checks on the
positions what the table's name promises (boundary values of uoff, per-chunk and per-tile counts, empty groups, chunk owners).

batch_ucap (pie_scan.hip: max(cap_users << bdshift, cap_rows / 16 + 4096)) is more than a sixteenth of the rows, so a union of
exactly that many rows cannot live on a table that keeps 5 % live; classify_queries keeps a batch's queries on the run below
10 % (kLiveFirstBelow), so union_cap() is a table of its own, 131 072 rows of which 9.4 % are live, used by batches only."""
import bisect
import collections
import functools

import numpy as np

DAY = 86400 * 1000
HOUR = 3600 * 1000
INT64_MIN = -(2 ** 63)
ALL = 2 ** 64 - 1
D = 64
T0 = 1700000000000
T_NOW, T_MIDNOW, T_OLDNOW = T0, T0 - 200 * DAY, T0 - 400 * DAY
LIVE_END, T_MID, T_OLD = T0 + DAY, T0 - 100 * DAY, T0 - 300 * DAY
S0 = T0 - 500 * DAY            # start of a user's first row; rank j starts at S0 + (j // 2) * 1000
FILL = 63
CHUNK, TILE, GROUP = 512, 4096, 1024          # positions per keyed unit / dense unit, units per prefix group
SHIFT_MAX, APPEND_MAX = 256, 4096             # kOrdShiftMax, kOrdAppendMax
MAX_LARGE_POSITIONS = 8 << 20

Table = collections.namedtuple("Table", "name cols U counts uoff n_ord spare row_pos pos_row pos_end pos_disc notes")


def bit(*groups):
    m = 0
    for g in groups:
        m |= 1 << g
    return m


# ------------------------------------------------------------------------------------------------ the layout model
def ord_spare(cap_rows, cap_users):
    return 16 if 16 * cap_users <= cap_rows // 4 else 4


def seg_len(cnt, spare):
    return cnt + cnt // 16 + spare


def run_layout(counts, cap_rows, cap_users):
    """-> (uoff int64[cap_users + 1], n_ord, spare) of a run built over a table with these per-user counts of selectable rows"""
    cnt = np.zeros(cap_users, np.int64)
    cnt[: len(counts)] = counts
    spare = ord_spare(cap_rows, cap_users)
    uoff = np.zeros(cap_users + 1, np.int64)
    np.cumsum(seg_len(cnt, spare), out=uoff[1:])
    return uoff, int(uoff[-1]), spare


def respread_layout(fill, pend, cap_rows, cap_users):
    """the layout after a re-spread: every segment is sized for the rows it holds plus the rows of the append still waiting"""
    return run_layout(np.asarray(fill, np.int64) + np.asarray(pend, np.int64), cap_rows, cap_users)


def grow_caps(cap_rows, cap_users, n, n_users):
    """ensure_capacity on the append path: capacities after an append to n rows / n_users users"""
    if n <= cap_rows and n_users <= cap_users:
        return cap_rows, cap_users
    rows = max(n, 2 * cap_rows) if n > cap_rows else cap_rows
    users = max(n_users, 2 * cap_users) if n_users > cap_users else cap_users
    return rows, users


def pos_cap(cap_rows, cap_users):
    return cap_rows + cap_rows // 16 + ord_spare(cap_rows, cap_users) * cap_users + 64


def rows_for_segment(length, spare):
    """the row count whose segment is exactly `length` positions, or None (cnt + cnt // 16 skips every 17th value)"""
    x = length - spare
    if x < 0:
        return None
    c = x - x // 17
    return c if c + c // 16 == x else None


def fit_boundary(counts, u, target, spare):
    """change counts[u - 1] (and counts[u - 2] by one row where needed) so that segment u starts exactly on `target`"""
    counts = np.asarray(counts, np.int64)
    for steal in range(3):
        before = int(seg_len(counts[: u - 1], spare).sum())
        c = rows_for_segment(target - before, spare)
        if c is not None and c >= 0:
            counts[u - 1] = c
            return counts
        counts[u - 2] += 1
    raise AssertionError(("no row count puts a segment start on", target))


# ------------------------------------------------------------------------------------------------ placement
class Design:
    """Positions first: .disc / .end per position (-1 / INT64_MIN on spare slots), filled with filler, then marked by the case."""

    def __init__(self, counts, seed, old_share=0.5):
        self.counts = np.asarray(counts, np.int64)
        self.U = int(self.counts.size)
        self.n = int(self.counts.sum())
        self.uoff, self.n_ord, self.spare = run_layout(self.counts, max(self.n, 1), self.U)
        self.rng = np.random.default_rng(seed)
        self.user = np.repeat(np.arange(self.U), np.diff(self.uoff))
        self.rank = np.arange(self.n_ord, dtype=np.int64) - self.uoff[self.user]
        self.is_row = self.rank < self.counts[self.user]
        self.disc = np.where(self.is_row, FILL, -1).astype(np.int32)
        self.end = np.full(self.n_ord, INT64_MIN, np.int64)
        rows = np.nonzero(self.is_row)[0]
        self.end[rows] = np.where(self.rng.random(rows.size) < old_share, T_OLD, T_MID) + self.rng.integers(0, DAY, rows.size)
        self.notes = {}

    def rows_in(self, lo, hi):
        """the positions of [lo, hi) that hold rows, ascending"""
        return lo + np.nonzero(self.is_row[lo:hi])[0]

    def pick(self, lo, hi, k, last=False):
        """k filler rows of [lo, hi), spread evenly; last: the last position of the range is one of them"""
        r = self.rows_in(lo, hi)
        r = r[self.disc[r] == FILL]
        assert r.size >= k, (lo, hi, k, r.size)
        if k == 0:
            return r[:0]
        got = r[np.unique(np.linspace(0, r.size - 1, k).astype(np.int64))] if k > 1 else r[r.size // 2: r.size // 2 + 1]
        if got.size < k:   # linspace collided: take the first k
            got = r[:k]
        if last:
            assert r[-1] == hi - 1, (hi, "is no row")
            got = np.concatenate([r[: k - 1], r[-1:]])
        return got

    def mark(self, pos, disc, end=LIVE_END):
        pos = np.asarray(pos, np.int64).reshape(-1)
        assert np.all(self.is_row[pos]) and np.all(self.disc[pos] == FILL) and np.unique(pos).size == pos.size, "not a free row"
        self.disc[pos] = disc
        self.end[pos] = end
        return pos

    def filler_end(self, lo, hi, old):
        """the filler rows of [lo, hi) all end OLD (dead under the mid query) or MID (live under it)"""
        r = self.rows_in(lo, hi)
        r = r[self.disc[r] == FILL]
        self.end[r] = (T_OLD if old else T_MID) + self.rng.integers(0, DAY, r.size)

    def table(self, name):
        rows = np.nonzero(self.is_row)[0]
        n = rows.size
        rid = self.rng.permutation(n).astype(np.int64)
        j, u = self.rank[rows], self.user[rows]
        pair = np.nonzero((j % 2 == 0) & (j + 1 < self.counts[u]))[0]       # rows i, i + 1 of one user share a start: the lower
        a, b = rid[pair], rid[pair + 1]                                      # row id comes first
        rid[pair], rid[pair + 1] = np.minimum(a, b), np.maximum(a, b)
        start, end = np.empty(n, np.int64), np.empty(n, np.int64)
        user, disc = np.empty(n, np.int32), np.empty(n, np.int32)
        start[rid], end[rid], user[rid], disc[rid] = S0 + (j // 2) * 1000, self.end[rows], u, self.disc[rows]
        row_pos = np.empty(n, np.int64)
        row_pos[rid] = rows
        pos_row = np.full(self.n_ord, -1, np.int64)
        pos_row[rows] = rid
        for arr in (start, end, user, disc, row_pos, pos_row, self.end, self.disc, self.uoff):
            arr.setflags(write=False)
        return Table(name, (start, end, user, disc), self.U, self.counts, self.uoff, self.n_ord, self.spare, row_pos, pos_row,
                     self.end, self.disc, self.notes)


def mask_bits(pos_disc, mask):
    ok = pos_disc >= 0
    sh = np.where(ok, pos_disc, 0).astype(np.uint64)
    return ok & (((np.uint64(mask) >> sh) & np.uint64(1)) == 1)


def live_positions(tab, q):
    return np.nonzero((tab.pos_disc >= 0) & (tab.pos_end > q[0]))[0]


def candidate_positions(tab, q):
    """rows whose key reaches key(now): those ending at or after `now`, given that every other row's key lies below key(now)
    (far_below asserts it with the key model)"""
    return np.nonzero((tab.pos_disc >= 0) & (tab.pos_end >= q[0]))[0]


def selected_positions(tab, q):
    return np.nonzero((tab.pos_end > q[0]) & mask_bits(tab.pos_disc, q[2]))[0]    # every cutoff of these cases is INT64_MIN


def answer_from_positions(tab, sel):
    offsets = np.searchsorted(sel, tab.uoff[: tab.U + 1]).astype(np.int64)
    return np.diff(offsets).astype(np.int32), offsets, tab.pos_row[sel].astype(np.int32)


def per_unit(pos, unit, n_ord):
    return np.bincount(pos // unit, minlength=(n_ord + unit - 1) // unit)


def sparse(mask):
    return T_NOW, INT64_MIN, mask


def old(mask):
    return T_OLDNOW, INT64_MIN, mask


def mid(mask):
    return T_MIDNOW, INT64_MIN, mask


# ------------------------------------------------------------------------------------------------ small tables
UOFF_VARIANTS = ("none", "before", "after", "both", "at")
UOFF_BOUNDS = (64, 512, 4096, "last")


def uoff_group(bi, vi):
    return 1 + bi * len(UOFF_VARIANTS) + vi


@functools.lru_cache(maxsize=None)
def uoff_edges():
    """Segment starts exactly on 64, 512, 4096 and n_ord - spare; a start with (uoff & 63) == 63; users without rows at the start
    (four in a row), in the middle (two in a row) and at the end (three in a row, the last one the boundary user of
    n_ord - spare).  Group uoff_group(b, v) selects, for boundary b, positions of the chunk AND the tile that hold uoff[b]: none of
    them (only a row of another tile), only rows before uoff[b], only rows at or after it, both, and uoff[b] itself with one row
    before it.  uoff[b] - 1 is a spare slot in every freshly built run (a segment ends in at least four), so "position
    uoff[u] - 1 selected" needs a segment that appends have filled: the `fill` append case scans that."""
    spare = 16
    c = [0, 0, 0, 0, rows_for_segment(448, spare), 0, 0, rows_for_segment(4096 - 544, spare), rows_for_segment(703, spare), 5000,
         3000, 2600, 0, 0, 0]
    d = Design(c, seed=11)
    assert d.spare == spare
    bounds = {64: 4, 512: 5, 4096: 8, "last": d.U - 1}
    far = d.rows_in(2 * TILE, 3 * TILE)                     # a tile that holds no boundary
    assert all(int(d.uoff[u]) // TILE != 2 for u in bounds.values())
    for bi, b in enumerate(UOFF_BOUNDS):
        q = int(d.uoff[bounds[b]])
        c0, t0 = q // CHUNK * CHUNK, q // TILE * TILE
        free = lambda lo, hi: [p for p in d.rows_in(lo, hi).tolist() if d.disc[p] == FILL]   # noqa: E731
        bb = free(t0, q)                                    # rows before uoff[b] in its tile (the last ones: in its chunk)
        aa = free(q + 1, min(t0 + TILE, d.n_ord))           # rows behind it in its tile (the first ones: in its chunk)
        row_at = bool(d.is_row[q])
        d.notes[b] = {"user": bounds[b], "uoff": q, "before": len(bb), "before_in_chunk": len(free(c0, q)), "after": len(aa),
                      "row_at": row_at}
        d.mark(far[bi * 3: bi * 3 + 1], uoff_group(bi, 0))
        if len(bb) >= 4:
            d.mark([bb[-1], bb[0]], uoff_group(bi, 1))
            d.mark([bb[-2]], uoff_group(bi, 3))
            d.mark([bb[-3]], uoff_group(bi, 4))
        if len(aa) >= 4:
            d.mark([aa[0], aa[-1]], uoff_group(bi, 2))
            d.mark([aa[1]], uoff_group(bi, 3))
        if row_at:
            d.mark([q], uoff_group(bi, 4))
    d.notes["bounds"] = bounds
    return d.table("uoff-edges")


def uoff_edges_queries():
    qs = {}
    for bi, b in enumerate(UOFF_BOUNDS):
        for vi, v in enumerate(UOFF_VARIANTS):
            qs[f"{b}/{v}"] = bit(uoff_group(bi, vi))
    qs["every group"] = ALL & ~bit(FILL)
    return qs


CHUNK_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 511, 512)
G_A, G_B, G_NONE = 1, 2, 5          # candidates alternate between A and B in position order; no row carries G_NONE


@functools.lru_cache(maxsize=None)
def chunk_counts():
    """Chunk 8 + 2 i holds CHUNK_COUNTS[i] candidates (the chunks between them hold none), a further chunk holds 64 whose last is
    the chunk's last position, and the table's last chunk, cut by n_ord, holds 3.  Candidates alternate between groups A and B:
    mask A | B selects all of them, A every other one, G_NONE none.  One candidate of the 65-chunk ends at exactly T_NOW (a
    candidate that is not live) and one at T_NOW + 1."""
    d = Design([30000, 0, 5000, 9000, 700], seed=12)
    chunks = {}
    plan = [(8 + 2 * i, k, False) for i, k in enumerate(CHUNK_COUNTS)] + [(40, 64, True)]
    last_chunk = (d.n_ord - 1) // CHUNK
    assert d.n_ord % CHUNK and d.rows_in(last_chunk * CHUNK, d.n_ord).size >= 3
    plan.append((last_chunk, 3, False))
    for ch, k, last in plan:
        lo, hi = ch * CHUNK, min((ch + 1) * CHUNK, d.n_ord)
        if k >= 511:
            assert d.rows_in(lo, hi).size == CHUNK
        p = np.sort(d.pick(lo, hi, k, last))
        d.mark(p[0::2], G_A)
        d.mark(p[1::2], G_B)
        chunks[ch] = k
        if k == 65:
            d.end[p[10]], d.end[p[11]] = T_NOW, T_NOW + 1
            d.notes["amb"] = (int(p[10]), int(p[11]))
    d.notes["chunks"] = chunks
    d.notes["last64"] = 40
    return d.table("chunk-counts")


G_DENSE, G_AMB = 3, 4


@functools.lru_cache(maxsize=None)
def tile_slices():
    """The dense form under the mid query (OLD filler dead, MID filler and group G_DENSE live, mask G_DENSE | G_AMB).  Tile 1: every
    position selected (4 096).  Tile 2: wave 0's quarter fully selected, wave 1's quarter OLD filler only (may == 0 in all 16
    slices), wave 2's quarter selected slices alternating with dead ones, wave 3's quarter dead but for one row ending at exactly
    T_MIDNOW (ambiguous, not live) and one at T_MIDNOW + 1 (ambiguous, live, selected) in two slices of their own.  The last tile is
    cut by n_ord inside a slice whose rows are selected."""
    c = [rows_for_segment(TILE, 16), 12000, 0, 6030, 20]
    d = Design(c, seed=13)
    assert d.uoff[1] == TILE and d.rows_in(TILE, 3 * TILE).size == 2 * TILE
    d.mark(np.arange(TILE, 2 * TILE), G_DENSE, T_MID)
    t2 = 2 * TILE
    d.mark(np.arange(t2, t2 + 1024), G_DENSE, T_MID)
    d.filler_end(t2 + 1024, t2 + 2048, old=True)
    for s in range(16):
        lo = t2 + 2048 + 64 * s
        if s % 2:
            d.filler_end(lo, lo + 64, old=True)
        else:
            d.mark(np.arange(lo, lo + 64, 3), G_DENSE, T_MID)
    d.filler_end(t2 + 3072, t2 + 4096, old=True)
    d.mark([t2 + 3072 + 64 * 5 + 7], G_AMB, T_MIDNOW)
    d.mark([t2 + 3072 + 64 * 9 + 63], G_AMB, T_MIDNOW + 1)
    last_rows = d.rows_in(d.n_ord // 64 * 64 - 64 * 2, d.n_ord)
    assert d.n_ord % 64 and d.n_ord % TILE and last_rows[-5] >= d.n_ord // 64 * 64
    # the last user's rows end 16 + cnt // 16 positions before n_ord: the slice that holds its last rows is the last with rows
    d.mark(last_rows[-5:], G_DENSE, T_MID)
    d.notes.update(full_tile=1, quarter_tile=2, amb=(t2 + 3072 + 64 * 5 + 7, t2 + 3072 + 64 * 9 + 63), last_rows=last_rows[-5:].copy())
    return d.table("tile-slices")


G_ALT = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def alternating():
    """Three queries A, B, C: group G_ALT[k] has rows only in chunks c with c % 3 == k (5 per chunk, 64 and 65 in two of them), so
    each selects in chunks the others leave empty; scanned in turn over the forms, each scan finds the unit-count buffer that the
    scan before the last one used and the last one zeroed."""
    d = Design([20000, 3000, 0, 12000, 2500], seed=14)
    n_chunks = (d.n_ord + CHUNK - 1) // CHUNK
    for ch in range(n_chunks):
        lo, hi = ch * CHUNK, min((ch + 1) * CHUNK, d.n_ord)
        k = 64 if ch == 9 else 65 if ch == 16 else 5
        if d.rows_in(lo, hi).size >= k:
            d.mark(d.pick(lo, hi, k), G_ALT[ch % 3])
    return d.table("alternating")


UNION_CHUNKS = {8: 8, 9: 9, 10: 64, 11: 1, 12: 65, 14: 512, 15: 3, 20: 9, 21: 8, 22: 0, 23: 2}   # chunk -> staged records


@functools.lru_cache(maxsize=None)
def union_chunks():
    """The batched union form: chunk c holds UNION_CHUNKS[c] rows that some query of the batch selects — 8 and 9 (kOrdChunkHeavy:
    the per-lane copy against the whole-wave copy), 64, 65, 512, heavy chunks beside light ones (8 | 9 | 64 | 1 | 65, 512 | 3,
    9 | 8 | 0 | 2).  The rows alternate between groups A and B; G_NONE is a query with no row at all."""
    d = Design([30000, 0, 5000, 9000, 700], seed=18)
    for ch, k in UNION_CHUNKS.items():
        p = np.sort(d.pick(ch * CHUNK, (ch + 1) * CHUNK, k))
        d.mark(p[0::2], G_A)
        d.mark(p[1::2], G_B)
    return d.table("union-chunks")


def union_chunks_queries(nq):
    masks = (bit(G_A, G_B), bit(G_A), bit(G_NONE), bit(G_B))
    return [(T_NOW + (i // 4), INT64_MIN, masks[i % 4]) for i in range(nq)]


def batch_ucap(cap_rows, cap_users, bdshift=4):
    return max(cap_users << bdshift, cap_rows // 16 + 4096)


G_U1, G_U2, G_U3 = 1, 2, 3


@functools.lru_cache(maxsize=None)
def union_cap():
    """131 072 rows, batch_ucap = 12 288: groups of 12 000, 288 and 1 rows; the union of the first two is exactly batch_ucap rows, with
    the third one more (n_over: the batch reruns per query and must still be exact)."""
    d = Design([60000, 0, 40000, 31072], seed=19)
    assert batch_ucap(d.n, d.U) == 12288
    free = d.rows_in(0, d.n_ord)
    d.mark(free[5: 5 + 5 * 12000: 5], G_U1)
    d.mark(free[70001: 70001 + 3 * 288: 3], G_U2)
    d.mark(free[100000: 100001], G_U3)
    return d.table("union-cap")


# ------------------------------------------------------------------------------------------------ the large table
G_WAVE, G_WAVE_CAND, G_GROUPS, G_RUN, G_STRIDE, G_BOUND = 1, 2, 4, 5, 6, 7
WAVE_PLANTS = {   # wave of the 2-byte single scan -> ((selected, unselected candidates) of its first chunk, of its second)
    10: ((40, 0), (0, 0)), 20: ((40, 0), (0, 58)), 30: ((40, 0), (30, 0)), 40: ((64, 0), (64, 0)), 50: ((70, 0), (6, 58)),
}


def keyed2_waves(n_cus):
    return 4 * 8 * n_cus


@functools.lru_cache(maxsize=None)
def large(n_cus):
    """One table sized from the CU count: n_chunks = 4 * 8 * n_cus + 300, so waves 0 .. 299 of the 2-byte single scan (W = 4 * 8 *
    n_cus waves, chunks w and w + W) own two chunks; WAVE_PLANTS puts the cross-chunk cases on five of them (in the second chunk
    of wave 50 the 58 unselected candidates come first, then the 6 selected).  Group G_GROUPS has rows in keyed groups 0 and 2
    only (group 1 = chunks 1024 .. 2047 is empty between two full ones).  Group G_RUN selects in every chunk 2900 .. 3000, in none
    of 3001 .. 3071 and in 3072 (a run of empty chunks that ends exactly on the boundary of groups 2 and 3).  Group G_STRIDE has
    one candidate in every chunk c with c % (4 * n_cus) == 7: all chunks of wave 7 of the 1-byte forms opened under PIE_ORD_GRID=1
    (eight or nine each; 64 chunks of one wave's stride would take 64 * 4 * n_cus chunks, 33 M positions on 256 CUs, so no grid
    reaches it below the 8 M-position bound).  Segments start exactly on position 524 288 (keyed groups 0 | 1) and, where the
    table is long enough, on 4 194 304 (dense groups 0 | 1); group G_BOUND selects those two positions and rows around them."""
    W = keyed2_waves(n_cus)
    n_chunks = W + 300
    n_ord_want = n_chunks * CHUNK - 200
    if n_ord_want > MAX_LARGE_POSITIONS:
        raise AssertionError(f"{n_cus} CUs: the large ordered table would hold {n_ord_want} positions, above the 8 M these tests allow")
    U, spare = max(64, n_ord_want // 2000), 16
    rng = np.random.default_rng(15)
    counts = rng.integers(1500, 2700, U).astype(np.int64)
    counts[rng.choice(U, U // 50, replace=False)] = 0
    cum = np.concatenate([[0], np.cumsum(seg_len(counts, spare))])
    bounds = {}
    for target in (GROUP * CHUNK, GROUP * TILE):
        if target + 3 * TILE > n_ord_want:
            continue
        u = int(np.searchsorted(cum, target))              # first user starting at or after the target
        counts[u - 1] = max(counts[u - 1], 200)
        counts = fit_boundary(counts, u, target, spare)
        counts[u] = max(counts[u], 100)
        cum = np.concatenate([[0], np.cumsum(seg_len(counts, spare))])
        assert cum[u] == target
        bounds[target] = u
    # the end: drop the users beyond n_ord_want and size the last one to land on it (or a position short of it)
    last = int(np.searchsorted(cum, n_ord_want, side="right")) - 1
    counts = counts[: last + 1]
    for back in range(3):
        c = rows_for_segment(n_ord_want - back - int(cum[last]), spare)
        if c is not None and c >= 0:
            counts[last] = c
            break
    d = Design(counts, seed=16, old_share=0.5)
    assert d.spare == spare and n_chunks == (d.n_ord + CHUNK - 1) // CHUNK and d.n_ord % CHUNK
    used = set()
    for w, (first, second) in WAVE_PLANTS.items():
        for ch, (n_sel, n_cand) in ((w, first), (w + W, second)):
            used.add(ch)
            p = np.sort(d.pick(ch * CHUNK, min((ch + 1) * CHUNK, d.n_ord), n_sel + n_cand))
            d.mark(p[:n_cand], G_WAVE_CAND)                # the unselected candidates first
            d.mark(p[n_cand:], G_WAVE)
    stride = 4 * n_cus
    for ch in range(7, n_chunks, stride):
        assert ch not in used
        used.add(ch)
        d.mark(d.pick(ch * CHUNK, min((ch + 1) * CHUNK, d.n_ord), 1), G_STRIDE)
    for ch in list(range(100, 1024, 7)) + [1023] + list(range(2048, 2800, 5)):
        if ch not in used:
            d.mark(d.pick(ch * CHUNK, (ch + 1) * CHUNK, 3), G_GROUPS)
    for ch in list(range(2900, 3001)) + [3072]:
        d.mark(d.pick(ch * CHUNK, (ch + 1) * CHUNK, 2), G_RUN)
    for target, u in bounds.items():
        assert d.is_row[target]
        d.mark([target, target + 1, target + 70], G_BOUND)
        r = d.rows_in(target - CHUNK, target)
        d.mark(r[d.disc[r] == FILL][-2:], G_BOUND)
    d.notes.update(n_cus=n_cus, W=W, n_chunks=n_chunks, bounds=bounds, stride=stride)
    return d.table("large")


LARGE_QUERIES = {"waves": bit(G_WAVE), "groups": bit(G_GROUPS), "run": bit(G_RUN), "stride": bit(G_STRIDE), "bounds": bit(G_BOUND),
                 "all": ALL & ~bit(FILL) & ~bit(G_WAVE_CAND)}


# ------------------------------------------------------------------------------------------------ appends
class RunModel:
    """The run of one context, replayed on the host: per user the (start, row) list of its segment in order, the layout, and the
    counters pie_table_info reports.  append() restates append_in_place / k_ord_append / ord_respread."""

    def __init__(self, cols, n_users):
        self.cols = [np.asarray(c).copy() for c in cols]
        self.n_users = n_users
        self.cap_rows, self.cap_users = max(self.cols[0].size, 1), n_users
        self.valid, self.builds, self.respreads = False, 0, 0
        self.dirty = False           # key_dirty: in-place appends and touches leave the key histogram stale; a growth refits the keys

    n = property(lambda self: int(self.cols[0].size))

    def build(self):
        s, e, u, d = self.cols
        ok = np.nonzero((e != INT64_MIN) & (d >= 0) & (d < 64))[0]
        order = ok[np.lexsort((ok, s[ok], u[ok]))]
        self.segs = [[] for _ in range(self.cap_users)]
        for r in order.tolist():
            self.segs[int(u[r])].append((int(s[r]), r))
        self.uoff, self.n_ord, self.spare = run_layout([len(x) for x in self.segs], self.cap_rows, self.cap_users)
        self.users, self.pos_cap = self.cap_users, pos_cap(self.cap_rows, self.cap_users)
        self.held = int(order.size)
        self.valid = True
        self.builds += 1

    def scan(self):
        """every scan of a context in mode 2 builds the run if there is none"""
        if not self.valid:
            self.build()

    def info(self):
        return {"ordered_positions": self.n_ord if self.valid else 0, "ordered_rows": self.held if self.valid else 0,
                "ordered_builds": self.builds, "ordered_respreads": self.respreads}

    def _pass(self, batch, todo, pend):
        """one pass of k_ord_append over the batch rows `todo` (batch indices, ascending) -> (left over, stale0, stale1)"""
        left, stale0, stale1 = [], 0, 0
        for t in todo:
            sv, u, row = batch[t]
            seg = self.segs[u]
            cap = int(self.uoff[u + 1] - self.uoff[u])
            if len(seg) >= cap:
                pend[u] += 1
                stale1 += 1
                left.append(t)
                continue
            at = bisect.bisect_right(seg, (sv, row))                 # the new row has the largest row id: behind every equal start
            if len(seg) - at > SHIFT_MAX:
                stale0 += 1
                left.append(t)
                continue
            seg.insert(at, (sv, row))
            self.shifted = max(self.shifted, len(seg) - 1 - at)
        return left, stale0, stale1

    def append(self, s, e, u, d, n_users):
        """-> "kept", "respread" or "dropped" (the run is invalid; the next scan rebuilds it)"""
        s, e, u, d = np.asarray(s, np.int64), np.asarray(e, np.int64), np.asarray(u, np.int32), np.asarray(d, np.int32)
        k, old_n = int(s.size), self.n
        assert n_users >= self.n_users, "n_users may only grow"
        in_place = old_n > 0 and old_n + k <= self.cap_rows and n_users <= self.cap_users
        self.cols = [np.concatenate([a, b]) for a, b in zip(self.cols, (s, e, u, d))]
        self.n_users = max(self.n_users, n_users)
        self.shifted = 0
        self.dirty = in_place
        if not in_place:
            self.cap_rows, self.cap_users = grow_caps(self.cap_rows, self.cap_users, old_n + k, n_users)
            self.valid = False
            return "dropped"
        # (append_in_place also asks n_users <= ord.users; the run's user capacity is the table's at its build and both only
        # change together, by the growth above, so through the ABI that test never decides)
        if not (self.valid and k <= APPEND_MAX):
            self.valid = False
            return "dropped"
        batch = [(int(s[t]), int(u[t]), old_n + t) for t in range(k)]
        pend = [0] * self.users
        # a thread places all rows of its user in batch order, whatever the chain's order
        left, stale0, stale1 = self._pass(batch, list(range(k)), pend)
        out = "kept"
        if stale0:
            self.valid = False
            return "dropped"
        if stale1:
            fill = [len(x) for x in self.segs]
            uoff, n_ord, _ = respread_layout(fill, pend, self.cap_rows, self.cap_users)
            if n_ord > self.pos_cap:
                self.valid = False
                return "dropped"
            self.uoff, self.n_ord = uoff, n_ord
            self.respreads += 1
            left, stale0, stale1 = self._pass(batch, left, [0] * self.users)
            if stale0 or stale1:
                self.valid = False
                return "dropped"
            out = "respread"
        self.held += k
        return out

    def positions(self):
        """row -> position of every row the run holds"""
        out = {}
        for u, seg in enumerate(self.segs):
            for j, (_, r) in enumerate(seg):
                out[r] = int(self.uoff[u]) + j
        return out


APPEND_U = 8          # users of the append table at its load; the first append declares 9, which doubles the user capacity to 16
A_BIG, A_0, A_15, A_16, A_17, A_B, A_C = 0, 1, 2, 3, 4, 5, 6


@functools.lru_cache(maxsize=None)
def append_table():
    """user 0: 600 rows; users 1 .. 4: 0, 15, 16 and 17 rows; users 5 .. 7: filler that makes the table 72 000 rows, so that the
    capacity after the first (growing) append holds every append of every case in place and the spare slots of users 5 and 6 (a
    sixteenth of 35 000 rows each) hold an append of kOrdAppendMax rows without a re-spread"""
    d = Design([600, 0, 15, 16, 17, 35000, 35352, 1000], seed=17)
    d.mark(d.pick(0, d.n_ord, 300), 1)
    return d.table("append")


def fresh_model():
    """the append table, loaded, scanned (build 1), grown by one append of a new user (the run is dropped: the capacities double)
    and scanned again (build 2): from here on appends are in place"""
    t = append_table()
    m = RunModel(t.cols, APPEND_U)
    m.scan()
    first = rows([T0 + HOUR], [APPEND_U], 0)
    assert m.append(*first, APPEND_U + 1) == "dropped"
    m.scan()
    assert (m.cap_rows, m.cap_users) == (2 * 72000, 2 * APPEND_U) and m.builds == 2
    return m, [first + (APPEND_U + 1, "dropped")]


def rows(starts, users, disc, ends=None):
    s = np.asarray(starts, np.int64)
    e = s + 12 * HOUR if ends is None else np.asarray(ends, np.int64)
    u = np.asarray(users, np.int32)
    d = np.full(s.size, disc, np.int32) if np.isscalar(disc) else np.asarray(disc, np.int32)
    return s, e, u, d


def start_for_shift(m, u, shift):
    """a start whose row belongs exactly `shift` rows from the end of user u's segment (behind every row with an equal start)"""
    seg = m.segs[u]
    at = len(seg) - shift
    assert at >= 1 and seg[at - 1][0] < seg[at][0], "no start sits exactly there"
    return seg[at - 1][0]


def append_case(name):
    """-> list of steps (start, end, user, disc, n_users, expected outcome) after fresh_model()'s; the expectation is what the case
    claims, the CPU test holds RunModel against it."""
    m, _ = fresh_model()
    nu = APPEND_U + 1
    steps = []

    def step(batch, want, n_users=None):
        n_users = nu if n_users is None else n_users
        steps.append(batch + (n_users, want))
        got = m.append(*batch, n_users)
        if got == "dropped":
            m.scan()
        return got

    now = T0 + 2 * HOUR
    if name == "shift":
        # user 0's rows start in pairs: the segment has an odd row on top after the first insert, which is what puts 257 within reach
        step(rows([start_for_shift(m, A_BIG, 256)], [A_BIG], 1), "kept")
        step(rows([now], [A_BIG], 1), "kept")                       # at the end: nothing shifts
        step(rows([start_for_shift(m, A_BIG, 257)], [A_BIG], 1), "dropped")
    elif name == "fill":
        for u in (A_0, A_15, A_16, A_17, APPEND_U + 3):
            room = int(m.uoff[u + 1] - m.uoff[u]) - len(m.segs[u])
            step(rows(now + np.arange(room), [u] * room, 1), "kept", n_users=max(nu, u + 1))
            nu = max(nu, u + 1)
            now += 1000
            step(rows([now], [u], 1), "respread")
            now += 1000
        step(rows([now], [2 * APPEND_U], 1), "dropped", n_users=2 * APPEND_U + 1)   # a user beyond the run's user capacity
    elif name == "batch-size":
        for k, want in ((APPEND_MAX, "kept"), (APPEND_MAX + 1, "dropped")):         # users 5 and 6 hold 2 048 more rows each in place
            st = now + np.arange(k)
            step(rows(st, A_B + np.arange(k) % 2, 1, st + 1000 * DAY), want)       # ends beyond the key range: never ambiguous
            now += 10000
    elif name == "long-chain":
        for k in (5, 63, 64, 65, 128, 129):
            a = A_B                                                    # 5 000 rows: 328 spare slots hold all of these chains
            u = np.full(k, -1, np.int64)
            mine = sorted({i for i in (0, 63, 64, k - 1) if i < k})
            mine += [i for i in (1, 2, 3, 4) if i < k and i not in mine][: max(0, 5 - len(mine))]
            u[mine] = a
            free = np.nonzero(u < 0)[0]
            other, at = [A_17, A_BIG, A_16, 7], 0                       # chains of 1, 2, 3 and 4 rows of other users
            for n_chain, ou in enumerate(other, 1):
                if at + n_chain <= free.size:
                    u[free[at: at + n_chain]] = ou
                    at += n_chain
            rest = np.nonzero(u < 0)[0]                                # the rest: half to the chain's user, half to another big one
            u[rest[0::2]], u[rest[1::2]] = A_C, a
            s = now + (np.arange(k) * 7919) % 1000                     # not in time order inside the batch
            dd = np.where(np.arange(k) < 64, a, 1)                     # the disc value of the first 64 rows is the user's id
            step(rows(s, u, dd), "kept")
            now += 5000
    elif name == "pass-2":
        room_c = int(m.uoff[A_15 + 1] - m.uoff[A_15]) - len(m.segs[A_15])
        step(rows(now + np.arange(room_c), [A_15] * room_c, 1), "kept")               # user C's segment is exactly full
        room_a = int(m.uoff[A_BIG + 1] - m.uoff[A_BIG]) - len(m.segs[A_BIG])
        assert 0 < room_a < 70                                                        # user A's chain of 70 is cut in the middle
        u = np.array(([A_BIG] * 7 + [A_B] + [A_15]) * 2 + [A_BIG] * 56 + [A_B], np.int64)
        assert np.count_nonzero(u == A_BIG) == 70
        step(rows(now + 5000 + (np.arange(u.size) * 31) % 97, u, 1), "respread")
    elif name == "mirror":
        step(rows([start_for_shift(m, A_BIG, 200)], [A_BIG], 1), "kept")
    else:
        raise KeyError(name)
    return steps


APPEND_CASES = ("shift", "fill", "batch-size", "long-chain", "pass-2", "mirror")
