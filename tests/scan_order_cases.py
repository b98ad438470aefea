"""TEST INFRASTRUCTURE — designed tables for the single scan's per-user bucket order (K2 / K3 / K4 of the general path), no GPU.

test_scan_order_cases_cpu.py shows with the oracle alone that every table plants what it claims; test_gpu_scan_order_paths.py
scans them through the C ABI.

Construction, all tables.  User u has sizes[u] designed rows, shuffled among filler rows that ended thirty days and more before
every query's `now` (no stage selects one).  Designed order is ascending row id inside the bucket.  Designed row j of user u
ends in tier(j + skip[u]), tier(x) = the first k with x < STAGE_ROWS[k], and the query of stage k has its `now` between the
ends of tiers k and k + 1: stage k selects exactly the first clip(STAGE_ROWS[k] - skip[u], 0, sizes[u]) designed rows of every
bucket (the scheme of table_model.plant_row_end).  skip is 0 except for the hot users of the `hot` tables, which a reduced
stage leaves 0 .. 16 rows.  Every query has cutoff INT64_MIN and every discipline, so `end` alone selects.

Stages: 4, 16, 17, 512, 513, 4096, 65536 and all rows.  65536 is there because the host loop that drives k_merge_pass takes its
number of passes from the LARGEST bucket (one pass up to 16 tiles of 4096 rows, two from 65537 rows on: the boundary the sizes
65536 / 65537 sit on is the real one), so only a scan whose largest bucket is exactly 65536 rows merges 16 tiles in one launch.

Start patterns, by designed row j of a bucket of n rows (PATTERNS): all equal; two values alternating, the higher first; strictly
descending; strictly ascending; organ pipe min(j, n - 1 - j); seeded random of five values.  include/pie_scan.h documents no
narrower domain for `start` than int64, so in every pattern every bucket of 17 rows or more has INT64_MAX on rows 1, 2 and n - 1
(the value the sorters pad with: a real row still sorts before the padding, its row id is below INT32_MAX) and INT64_MIN on rows
3 and n - 2 (selected, the cutoff is INT64_MIN); rows 1 .. 3 are inside every stage.  So that no bucket of two rows or more hands
the sorters an input that is already in order with all keys distinct, the ascending pattern puts INT64_MAX on row 0 of the buckets
of 2 .. 16 rows, and a random-of-five bucket of 2 .. 16 rows that came out strictly ascending is reversed."""
import collections
import functools

import numpy as np

DAY = 86400 * 1000
HOUR = 3600 * 1000
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
ALL = 2 ** 64 - 1
D = 64
ALL_ROWS = 2 ** 31 - 1
STAGE_ROWS = (4, 16, 17, 512, 513, 4096, 65536, ALL_ROWS)
STAGE = {"4": 0, "16": 1, "17": 2, "512": 3, "513": 4, "4096": 5, "65536": 6, "full": 7}
PATTERNS = ("equal", "two", "desc", "asc", "organ", "rand5")
TINY_MAX, SMALL_MAX, SEG_MAX, HOT_MAX = 16, 512, 4096, 32   # kTinyMax, kSmallMax, kSegMax, kHotMax of pie_kernels.h
STAGED_USERS = 8388609                                      # one user more than direct slots are carried for

SIZES = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025,
         2047, 2048, 2049, 4095, 4096, 4097, 8192, 8193, 65536, 65537)
SIZES_DESIGNED = 172013

Table = collections.namedtuple("Table", "name pattern cols U sizes skip designed")


def query(t0, k):
    """(now, cutoff, mask) of stage k"""
    return t0 - k * HOUR - HOUR // 2, INT64_MIN, ALL


def row_end(t0, x):
    """`end` of designed rows whose j + skip is x (an array)"""
    tier = np.searchsorted(np.asarray(STAGE_ROWS, np.int64), x, side="right")
    return t0 - tier * HOUR


def expected_counts(tab, k):
    return np.clip(STAGE_ROWS[k] - tab.skip, 0, tab.sizes).astype(np.int32)


def bucket_starts(pattern, n, rng):
    """start of designed rows 0 .. n - 1 of one bucket (see the module docstring)"""
    base = 1700000000000 - 50 * DAY
    j = np.arange(n, dtype=np.int64)
    if pattern == "equal":
        s = np.full(n, base, np.int64)
    elif pattern == "two":
        s = base + ((j + 1) % 2) * 1000
    elif pattern == "desc":
        s = base - j
    elif pattern == "asc":
        s = base + j
    elif pattern == "organ":
        s = base + np.minimum(j, n - 1 - j)
    elif pattern == "rand5":
        s = base + 977 * rng.integers(0, 5, n)
        if 2 <= n <= TINY_MAX and np.all(np.diff(s) > 0):
            s = s[::-1].copy()
    else:
        raise KeyError(pattern)
    if n > TINY_MAX:
        s[[1, 2, n - 1]] = INT64_MAX
        s[[3, n - 2]] = INT64_MIN
    elif pattern == "asc" and n >= 2:
        s[0] = INT64_MAX
    return s


def build(t0, name, pattern, sizes, skip, n_filler, seed, n_users=None, by_user=0):
    """by_user: 0 rows shuffled, 1 rows sorted by ascending user, -1 by descending user (designed order kept)."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    skip = np.asarray(skip, np.int64)
    U = int(sizes.size) if n_users is None else int(n_users)
    live = int(sizes.sum())
    n = live + n_filler
    owners = np.nonzero(sizes)[0]
    at = np.sort(rng.permutation(n)[:live])                  # the rows that hold designed rows, ascending
    owner = rng.permutation(np.repeat(owners, sizes[owners]))  # ... and whose they are
    order = np.argsort(owner, kind="stable")                 # grouped by user, ascending row id inside a user
    first = np.cumsum(sizes[owners]) - sizes[owners]
    j = np.empty(live, np.int64)
    j[order] = np.arange(live) - np.repeat(first, sizes[owners])
    st = np.empty(live, np.int64)
    for u, f in zip(owners.tolist(), first.tolist()):
        st[order[f: f + int(sizes[u])]] = bucket_starts(pattern, int(sizes[u]), rng)
    user = rng.integers(0, min(U, 1 << 20), n).astype(np.int32)
    start = (t0 - 400 * DAY + rng.integers(0, 300 * DAY, n)).astype(np.int64)
    end = (t0 - 30 * DAY - rng.integers(0, 270 * DAY, n)).astype(np.int64)
    end[rng.integers(0, n, 50)] = INT64_MIN                  # a few tombstones among the filler
    disc = rng.integers(0, D, n).astype(np.int32)
    designed = np.zeros(n, bool)
    designed[at] = True
    user[at] = owner
    start[at] = st
    end[at] = row_end(t0, j + skip[owner])
    if by_user:
        o = np.argsort(user.astype(np.int64) * by_user, kind="stable")
        start, end, user, disc, designed = start[o], end[o], user[o], disc[o], designed[o]
    full = np.zeros(U, np.int64)
    full[: sizes.size] = sizes
    sk = np.zeros(U, np.int64)
    sk[: skip.size] = skip
    return Table(name, pattern, (start, end, user, disc), U, full, sk, designed)


def sizes_layout():
    """One user per value of SIZES in that order at ids 1, 4, 7, ..: a zero-row user in front of each, a 3-row spare behind."""
    s = np.zeros(3 * len(SIZES) + 2, np.int64)
    s[1::3][: len(SIZES)] = SIZES
    s[2::3] = 3
    return s


MIDS_U = 64 * 5 + 37   # neither a multiple of 64 nor of an order block (256, 512, 1024)


def mids_layout():
    """Wave groups of 64 users: group 0 holds exactly 6 buckets of 9 .. 16 rows, group 1 exactly 7, group 2 sixty-four, groups 3
    and 4 none, and the only one of group 5 is the last user of the table."""
    rng = np.random.default_rng(31)
    s = rng.choice([0, 0, 1, 2, 3, 5, 7, 8, 8], MIDS_U)
    for g, k in ((0, 6), (1, 7)):
        lanes = np.concatenate([[0, 63], rng.choice(np.arange(1, 63), k - 2, replace=False)])
        s[64 * g + lanes] = np.concatenate([[9, 16], rng.integers(9, 17, k - 2)])
    s[128:192] = np.concatenate([[9, 16], rng.integers(9, 17, 62)])
    s[MIDS_U - 1] = 13
    return s.astype(np.int64)


HOT_U = 1000
HOT_CYCLE = (600, 777, 1024, 2048, 4096, 4097, 900, 1500)


def hot_layout(n_hot):
    """-> (sizes, skip, hot users).  n_hot users far above 1/256 of the table's designed rows (one of them the last user), every
    other bucket far below; the i-th hot user skips i % 16 tiers' worth of rows, the second one 16: the 16-row stage leaves the
    hot users 1 .. 16 rows and that one none."""
    rng = np.random.default_rng(47)
    s = rng.choice([0, 0, 0, 1, 2, 5, 9, 16, 17, 40], HOT_U).astype(np.int64)
    hot = np.concatenate([np.sort(rng.choice(HOT_U - 1, n_hot - 1, replace=False)), [HOT_U - 1]])
    s[hot] = [HOT_CYCLE[i % 8] if i < 32 else 600 for i in range(n_hot)]
    skip = np.zeros(HOT_U, np.int64)
    skip[hot] = np.arange(n_hot) % 16
    skip[hot[1]] = 16
    return s, skip, hot


@functools.lru_cache(maxsize=None)
def table(t0, name, pattern):
    """The named table under the named start pattern: built once, shared, never changed."""
    if name in ("sizes", "clustered", "clustered_desc", "staged"):
        s = sizes_layout()
        assert int(s[1::3].sum()) == SIZES_DESIGNED
        if name == "staged":   # the same users in a table too wide for direct slots, and a 17-row bucket on its last user
            s = np.concatenate([s, [17]])
            tab = build(t0, name, pattern, s[:-1], np.zeros(s.size - 1, np.int64), 800000, 5, n_users=STAGED_USERS)
            return with_last_user(t0, tab, 17, pattern)
        return build(t0, name, pattern, s, np.zeros(s.size, np.int64), 800000, 5,
                     by_user={"sizes": 0, "clustered": 1, "clustered_desc": -1}[name])
    if name == "mids":
        s = mids_layout()
        return build(t0, name, pattern, s, np.zeros(s.size, np.int64), 60000, 6)
    if name in ("hot", "hot40"):
        s, skip, _ = hot_layout(32 if name == "hot" else 40)
        return build(t0, name, pattern, s, skip, 800000, 7)
    raise KeyError(name)


def with_last_user(t0, tab, size, pattern):
    """tab with `size` designed rows of user U - 1 written over filler rows (ascending row id is the designed order)."""
    start, end, user, disc = (c.copy() for c in tab.cols)
    rng = np.random.default_rng(99)
    rows = np.sort(rng.choice(np.nonzero(~tab.designed)[0], size, replace=False))
    designed = tab.designed.copy()
    designed[rows] = True
    user[rows] = tab.U - 1
    start[rows] = bucket_starts(pattern, size, rng)
    end[rows] = row_end(t0, np.arange(size))
    sizes = tab.sizes.copy()
    sizes[tab.U - 1] = size
    return Table(tab.name, tab.pattern, (start, end, user, disc), tab.U, sizes, tab.skip, designed)


TABLES_ABOVE_16 = ("sizes", "clustered", "clustered_desc", "hot", "hot40")   # the tables the start patterns multiply


def numpy_answer(t0, tab, k):
    """(counts, offsets, idx) of stage k in plain numpy: per user, np.lexsort((row, start)) of its selected rows."""
    start, end, user, _ = tab.cols
    now, cutoff, _ = query(t0, k)
    rows = np.nonzero((end > now) & (start >= cutoff))[0]
    counts = np.bincount(user[rows], minlength=tab.U).astype(np.int32)
    offsets = np.zeros(tab.U + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    by_user = rows[np.argsort(user[rows], kind="stable")]
    idx = np.empty(rows.size, np.int32)
    for u in np.nonzero(counts)[0].tolist():
        mine = by_user[offsets[u]: offsets[u + 1]]
        idx[offsets[u]: offsets[u + 1]] = mine[np.lexsort((mine, start[mine]))]
    return counts, offsets, idx


# ------------------------------------------------------------------------------------------------ the routes, restated
class Routes:
    """What the host and K2 decide per scan, restated from pie_scan.hip (begin, finish) and k_offsets: the direct-slot capacity,
    the hot set in force, and from them the list counters a scan must report.  One per context; feed it every finished scan in
    order (scans begun and finished one at a time)."""

    def __init__(self, direct=True):
        self.direct = direct
        self.shift = self.shift_want = 4
        self.prev_m = -1
        self.hot = frozenset()     # users of the context's hot set; None: clipped at 32 of more, which 32 is not determined
        self.hot_seen = 0

    def scan(self, counts, variant):
        """-> dict of the expected stats of a scan with these per-user counts under this K1 form"""
        counts = np.asarray(counts, np.int64)
        if self.shift_want > self.shift and self.direct:
            self.shift = self.shift_want
        in_force = self.hot if (variant & 0x44) == 0x44 else frozenset()
        m = int(counts.sum())
        exp = {"direct_shift": self.shift if self.direct else 0, "max_bucket": int(counts.max()),
               "n_big": int(np.count_nonzero(counts > SEG_MAX)), "hot_in_force": None if in_force is None else len(in_force)}
        thr = self.prev_m // 256 if self.prev_m >= 65536 else 0
        cand = np.nonzero(counts > thr)[0] if thr > 0 else np.zeros(0, np.int64)
        exp["n_hot"] = min(HOT_MAX, int(cand.size))
        if in_force is not None:
            is_hot = np.zeros(counts.size, bool)
            is_hot[list(in_force)] = True
            listed = (counts > TINY_MAX) | (is_hot & (counts > 0))
            in_direct = (counts <= (1 << self.shift)) & ~is_hot if self.direct else np.zeros(counts.size, bool)
            tiles = (counts + SEG_MAX - 1) // SEG_MAX
            exp["n_over"] = int(np.count_nonzero(listed & ~in_direct))
            exp["n_small"] = int(np.count_nonzero(listed & (counts <= SMALL_MAX)))
            exp["n_segments"] = int(np.count_nonzero(listed & (counts > SMALL_MAX) & (counts <= SEG_MAX)) + tiles[counts > SEG_MAX].sum())
        # finish: what the next scan inherits
        if self.direct and exp.get("n_over", 1) > 0 and exp["max_bucket"] > (1 << self.shift):
            want = self.shift
            while want < 9 and (1 << want) < exp["max_bucket"]:
                want += 1
            self.shift_want = max(self.shift_want, want)
        if exp["n_hot"] == 0:
            self.hot, self.hot_seen = frozenset(), 0
        elif exp["n_hot"] != self.hot_seen:
            self.hot = frozenset(cand.tolist()) if cand.size <= HOT_MAX else None
            self.hot_seen = exp["n_hot"]
        self.prev_m = m
        return exp
