"""TEST INFRASTRUCTURE — a numpy model of the session table behind the C ABI, a seeded step generator over its mutators and
readers, and the runner that drives a PieScan context and the model side by side (tests/test_gpu_model.py, tools/fuzz_gpu.py).

Nothing here needs a GPU to import.  The model is the only source of expected values: scans come from
oracle_py.scan_numpy (the lexsort restatement) on the model's columns, every CHECK_C_EVERY-th one is also compared with
the C oracle, so a mistake shared by one oracle and the kernels cannot hide."""
import os

import numpy as np

INT64_MIN = -(2 ** 63)
INT64_MAX = 2 ** 63 - 1
ALL = 2 ** 64 - 1
HOUR = 3600 * 1000
DAY = 24 * HOUR
YEAR = 365 * DAY
PIE_E_STATE = -6
MAX_ROWS = 1 << 20
CHECK_C_EVERY = 7

KEY_MAX, FINE_KEY_MAX, KEY_HIST_BINS = 32767, 127, 4096

# every way a reader call can be answered; test_model_sequences_reached_every_path wants each of them seen
PATHS = ("general", "keyed_2byte", "keyed_1byte", "hot_clean", "hot_delta", "ordered_scan", "ordered_batch", "wide_pass",
         "wide_fallback")


# ------------------------------------------------------------------------------------------------ the key definition
def key_of(e, base, shift, kmax=KEY_MAX):
    """0 below `base`, else min(((e - base) >> shift) + 1, kmax).  Python ints: no overflow anywhere."""
    e = int(e)
    if e < base:
        return 0
    return min(((e - base) >> shift) + 1, kmax)


def key_params(end):
    """(key_base, key_shift, fkey_base, fkey_shift) as the table derives them at a full key build:
    base = the smallest live `end`, shift = the smallest that keeps the largest below the clamp; the fine key's base = the
    lower edge of the histogram bin (4096 bins of 8 keys) that holds the 90th percentile of the 15-bit keys of ALL rows
    (tombstones are key 0), its shift the smallest that keeps the top occupied bin's upper edge below its clamp."""
    end = np.asarray(end, np.int64)
    live = end[end != INT64_MIN]
    if live.size == 0:
        return 0, 0, 0, 0
    base, top = int(live.min()), int(live.max())
    shift = 0
    while shift < 63 and ((top - base) >> shift) >= KEY_MAX - 1:
        shift += 1
    keys = np.array([key_of(v, base, shift) for v in np.unique(end)], np.int64)
    hist = np.zeros(KEY_HIST_BINS, np.int64)
    np.add.at(hist, keys >> 3, np.unique(end, return_counts=True)[1])
    want, cum, b = int(float(end.size) * 0.9), 0, 0
    top_bin = int(np.nonzero(hist)[0].max())
    while b < KEY_HIST_BINS - 1:
        if cum + int(hist[b]) > want:
            break
        cum += int(hist[b])
        b += 1
    b = min(b, top_bin)
    fbase = base if b == 0 else base + ((8 * b - 1) << shift)
    fspan = base + ((8 * top_bin + 8) << shift) - fbase
    fshift = 0
    while fshift < 63 and (fspan >> fshift) >= FINE_KEY_MAX - 1:
        fshift += 1
    return base, shift, fbase, fshift


# ------------------------------------------------------------------------------------------------ calendar months
def add_months(ts, months, tz_offset_ms=0):
    """JS `setMonth(getMonth() + months)` on a local Date at a fixed offset, vectorised: the month moves, the day of the
    month is kept and overflows into the following month (Dec 31 + 2 -> "Feb 31" -> Mar 3), the time of day is kept."""
    local = np.asarray(ts, np.int64) + int(tz_offset_ms)
    days = np.floor_divide(local, DAY)
    tod = local - days * DAY
    date = days.astype("datetime64[D]")
    month = date.astype("datetime64[M]")
    dom = (date - month.astype("datetime64[D]")).astype(np.int64)
    moved = (month + int(months)).astype("datetime64[D]").astype(np.int64) + dom
    return moved * DAY + tod - int(tz_offset_ms)


# ------------------------------------------------------------------------------------------------ the model
def tombstone(end, sel):
    """The one rule of deleteSessionsForUser, prune and retention: the selected rows that are not tombstones yet become
    tombstones, in place -> those rows, ascending.  tests/turn_model.py deletes a user through it too."""
    rows = np.nonzero(sel & (end != INT64_MIN))[0].astype(np.int32)
    end[rows] = INT64_MIN
    return rows


class TableModel:
    """start / end / user / disc and the user and discipline counts; every table operation of include/pie_scan.h restated."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.scans = 0
        self.load(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), 1, 1)

    @property
    def n(self):
        return self.start.size

    def load(self, start, end, user, disc, U, D):
        self.start, self.end = np.array(start, np.int64), np.array(end, np.int64)
        self.user, self.disc = np.array(user, np.int32), np.array(disc, np.int32)
        self.U, self.D = int(U), int(D)

    def columns(self):
        return self.start, self.end, self.user, self.disc

    def lim(self):
        return ALL if self.D >= 64 else (1 << self.D) - 1

    # ---- mutators
    def append_rows(self, start, end, user, disc, U):
        self.start = np.concatenate([self.start, np.asarray(start, np.int64)])
        self.end = np.concatenate([self.end, np.asarray(end, np.int64)])
        self.user = np.concatenate([self.user, np.asarray(user, np.int32)])
        self.disc = np.concatenate([self.disc, np.asarray(disc, np.int32)])
        self.U = int(U)

    def set_end(self, rows, new_end):
        """The elements applied in array order: of the elements that name one row the last one gives the row its `end`
        (include/pie_scan.h).  Said outright, not left to what numpy does with a repeated fancy index: the last occurrence of
        every row is the first one in the reversed array, and only those elements are stored."""
        rows, new_end = np.asarray(rows, np.int64).reshape(-1), np.asarray(new_end, np.int64).reshape(-1)
        assert rows.size == new_end.size
        _, first_in_reversed = np.unique(rows[::-1], return_index=True)
        last = rows.size - 1 - first_in_reversed
        self.end[rows[last]] = new_end[last]

    def _tombstone(self, sel):
        return tombstone(self.end, sel)

    def delete_user(self, u):
        if not 0 <= u < self.U:
            return np.zeros(0, np.int32)
        return self._tombstone(self.user == u)

    def prune_before(self, cutoff):
        return self._tombstone(self.start < cutoff)

    def retention_purge(self, now, months, tz_offset_ms=0):
        return self._tombstone(add_months(self.start, months, tz_offset_ms) <= now)

    def shard_rows(self, rank, world):
        owner = np.array([self.oracle.shard_of(u, world) for u in range(self.U)], np.int32)
        return owner, np.nonzero(owner[self.user] == rank)[0] if self.n else np.zeros(0, np.int64)

    def shard_table(self, rank, world):
        """Rows of the users that hash to `rank` stay, in table order; those users are re-numbered densely, ascending."""
        owner, rows = self.shard_rows(rank, world)
        users = np.nonzero(owner == rank)[0]
        local = np.full(self.U, -1, np.int32)
        local[users] = np.arange(users.size, dtype=np.int32)
        self.start, self.end, self.disc = self.start[rows], self.end[rows], self.disc[rows]
        self.user = local[self.user[rows]]
        self.U = max(int(users.size), 1)
        return self.n, self.U

    # ---- readers
    def scan(self, now, cutoff, mask):
        return self.scan_many([(now, cutoff, mask)])[0]

    def scan_many(self, queries):
        """[(counts, offsets, idx)] per (now, cutoff, mask); bits of the mask at or above D are ignored.  Sparse queries
        share one pre-filter (rows with end <= the smallest of their `now`s are selected by none of them; the candidates stay
        in row order, so the restatement's tie order by row index is unchanged): the restatement then sorts only those."""
        o, lim = self.oracle, self.lim()
        out = [None] * len(queries)
        live = int(np.count_nonzero(self.end != INT64_MIN))
        sparse = []
        for qi, (now, cutoff, mask) in enumerate(queries):
            if self.n > 50000 and int(np.count_nonzero(self.end > now)) * 8 < max(live, 1):
                sparse.append(qi)
                continue
            out[qi] = o.scan_numpy(self.start, self.end, self.user, self.disc, self.U, now, cutoff, mask & lim)
        if sparse:
            cand = np.nonzero(self.end > min(queries[qi][0] for qi in sparse))[0]
            cs, ce, cu, cd = self.start[cand], self.end[cand], self.user[cand], self.disc[cand]
            for qi in sparse:
                now, cutoff, mask = queries[qi]
                c, off, idx = o.scan_numpy(cs, ce, cu, cd, self.U, now, cutoff, mask & lim)
                out[qi] = (c, off, cand[idx].astype(np.int32))
        for qi, (now, cutoff, mask) in enumerate(queries):
            self.scans += 1
            if self.scans % CHECK_C_EVERY == 0:   # the C oracle on the whole table: the two restatements must agree
                for name, a, b in zip(("counts", "offsets", "idx"), out[qi], o.scan(*self.columns(), self.U, now, cutoff, mask & lim)):
                    assert a.dtype == b.dtype and np.array_equal(a, b), ("the oracles disagree", name, queries[qi])
        return out

    def expired_queue(self, prev_now, now):
        return np.nonzero((self.end > prev_now) & (self.end <= now))[0].astype(np.int32)

    def archive_queue(self, now, window_ms):
        """Groups (users) whose earliest start over their non-tombstoned rows is at least window_ms old, in order of first
        appearance; their non-tombstoned rows in table order."""
        rows = np.nonzero(self.end != INT64_MIN)[0]
        if rows.size == 0:
            return np.zeros(0, np.int32)
        g = self.user[rows]
        earliest = np.full(self.U, INT64_MAX, np.int64)
        np.minimum.at(earliest, g, self.start[rows])
        first = np.full(self.U, INT64_MAX, np.int64)
        np.minimum.at(first, g, rows)
        qual = np.array([e != INT64_MAX and int(now) - int(e) >= int(window_ms) for e in earliest.tolist()], bool)
        keep = rows[qual[g]]
        return keep[np.lexsort((keep, first[self.user[keep]]))].astype(np.int32)


# ------------------------------------------------------------------------------------------------ hand-made edge tables
LATTICE_SHIFT = 12   # pitch 4096 ms
LATTICE_TOP = 20000  # lattice index of the largest end


def lattice_table(oracle, seed=1):
    """A few thousand rows whose `end` values all lie on base + j * 2^LATTICE_SHIFT, j in [0, LATTICE_TOP].

    The pitch follows from the key definition: key_shift is the smallest s with (span >> s) < 32766 and
    span = LATTICE_TOP << LATTICE_SHIFT, so with 16383 <= LATTICE_TOP < 32766 it is exactly LATTICE_SHIFT: the pitch equals
    the 15-bit key's bin width (the largest shift this span can produce), key(base + j * pitch) = j + 1, and EVERY lattice value
    is the lower edge of a bin.  The fine key's base is base + ((8 b - 1) << key_shift) for the histogram bin b of the 90th
    percentile: lattice index 8 b - 1.  The top of the lattice (indices LATTICE_TOP - 400 .. LATTICE_TOP, every one occupied)
    holds four fifths of the rows, so that index is an occupied value; the fine key's shift is at most key_shift (its range is a
    few dozen pitches over 126 bins), so every lattice value at or above its base is the lower edge of a fine bin too.
    -> (start, end, user, disc, U, D, occupied lattice values ascending)."""
    rng = np.random.default_rng(seed)
    U, D = 53, 32
    pitch = 1 << LATTICE_SHIFT
    base = oracle.T0_MS - LATTICE_TOP * pitch
    low = np.unique(np.concatenate([[0], rng.choice(np.arange(1, LATTICE_TOP - 3000), 150, replace=False)]))
    top = np.arange(LATTICE_TOP - 400, LATTICE_TOP + 1)
    j = np.concatenate([np.repeat(low, 4), np.repeat(top, 6)])
    j = j[rng.permutation(j.size)]
    n = j.size
    end = (base + j * pitch).astype(np.int64)
    start = (oracle.T0_MS - 70 * DAY + rng.integers(0, 69 * DAY, n)).astype(np.int64)
    user = ((np.arange(n) * 7 + j) % U).astype(np.int32)   # rows of one value get different users and disciplines
    disc = ((np.arange(n) * 5 + j // 3) % D).astype(np.int32)
    values = (base + np.concatenate([low, top]) * pitch).astype(np.int64)
    return start, end, user, disc, U, D, values


def tie_table(oracle, seed=2):
    """Per-user runs of equal starts: user 0 has 150 rows on one start (more than a wave, more than the 16-record direct
    bucket), user 1 has 70 on another and 20 on a third, the rest a few equal starts each; disciplines include 0, 63 and
    values outside [0, 64).  -> (start, end, user, disc, U, D)."""
    rng = np.random.default_rng(seed)
    U, D = 47, 64
    t0 = oracle.T0_MS
    starts = [np.full(150, t0 - 40 * DAY), np.full(70, t0 - 30 * DAY), np.full(20, t0 - 30 * DAY + 1)]
    users = [np.zeros(150), np.ones(70), np.ones(20)]
    n_rest = 2400
    pool = t0 - 50 * DAY + rng.integers(0, 60, n_rest) * (DAY // 2)      # 60 distinct starts for everybody else
    starts.append(pool)
    users.append(rng.integers(2, U, n_rest))
    start, user = np.concatenate(starts).astype(np.int64), np.concatenate(users).astype(np.int32)
    p = rng.permutation(start.size)
    start, user = start[p], user[p]
    n = start.size
    end = (t0 + rng.integers(-2 * HOUR, 10 * HOUR, n)).astype(np.int64)
    big = np.nonzero(user < 2)[0]
    end[big[::4]] = t0 + 11 * HOUR   # a quarter of the long tie runs stays live for top-of-range queries
    disc = rng.choice(np.array([0, 0, 1, 5, 31, 32, 62, 63, 63, 64, 65, 200, -1, -7], np.int32), n).astype(np.int32)
    return start, end, user, disc, U, D


# ------------------------------------------------------------------------------------------------ the user axis
# Boundaries of the library along the number of users, restated from the documented rules so that the
# CPU tests can check the tables the GPU tests rely on.
USER_TILE = 256               # users per tile of the batched union tail (and threads of its look-back)
MQ_SLOTS = 64                 # per-query totals are folded by tile & 63
BATCH_MAX_TILES = 2048        # the batched pass answers up to 2048 tiles: 524 288 users
BATCH_MAX_USERS = USER_TILE * BATCH_MAX_TILES
FUSED_SCAN_MAX_USERS = 512 * BATCH_MAX_TILES   # single scans: the fused offsets kernel, 512 users per tile, up to 2048 tiles
DIRECT_MAX_BYTES = 2 << 30    # bound of every array of bucket slots
BUCKET_REC_BYTES = 16
WIDE_MASK_BYTES = 64          # eight 64-bit mask words per bucket slot of a wide batch
UNION_SHIFT_MAX = 6           # union buckets grow from 16 over 32 to 64 slots per user

PLANT_SIZES = (1, 2, 8, 9, 16, 17, 33, 64)
PLANT_STAGE_ROWS = (16, 17, 33, 64, 65)   # rows of a planted bucket that the queries of stage k can select: min(size, this)
PLANT_GROW_USER = 263                     # tile 1: the one bucket of 65 rows (64 up to stage 3)
PLANT_OFFSETS = (0, 31, 32, 63, 64, 129, 200, 255)   # users of a full tile, by PLANT_SIZES


def batch_supported_users(n_users):
    return (n_users + USER_TILE - 1) // USER_TILE <= BATCH_MAX_TILES


def union_slots_fit(cap_users, shift):
    """the union buckets of the ordinary batch may grow to 1 << shift slots per user"""
    return (cap_users << shift) * BUCKET_REC_BYTES <= DIRECT_MAX_BYTES


def wide_union_fits(cap_users, shift):
    """a wide batch keeps its union: its slot masks, 64 B per bucket slot, stay within the same 2 GiB"""
    return (cap_users << shift) * WIDE_MASK_BYTES <= DIRECT_MAX_BYTES


def plant_places(U):
    """[(name, tile)] of the tiles that get a set of hand-made buckets, those that exist at U users: tile 0, tile 64 (congruent
    to tile 0 and to tile 256 mod 64), tiles 255, 256 and 257 (tile 257 is the first whose look-back makes a second trip), the last full tile
    and the last tile, which is partial unless U is a multiple of 256."""
    tiles, full = (U + USER_TILE - 1) // USER_TILE, U // USER_TILE
    out, seen = [], set()
    for name, t in (("tile 0", 0), ("tile 64", 64), ("tile 255", 255), ("tile 256", 256), ("tile 257", 257),
                    ("last full tile", full - 1), ("last tile", tiles - 1)):
        if 0 <= t < tiles and t not in seen:
            seen.add(t)
            out.append((name, t))
    return out


def plant_users(U):
    """{user: bucket size}.  A full tile holds all of PLANT_SIZES at PLANT_OFFSETS (64 rows on its last user); a partial last
    tile holds the largest sizes that fit, on its last users (64 rows on user U - 1); and PLANT_GROW_USER holds 65."""
    planted = {}
    for _, t in plant_places(U):
        width = min(USER_TILE, U - t * USER_TILE)
        for i, size in enumerate(sorted(PLANT_SIZES, reverse=True)):
            if width == USER_TILE:
                planted[t * USER_TILE + PLANT_OFFSETS[len(PLANT_SIZES) - 1 - i]] = size
            elif width - 1 - i >= 0:
                planted[t * USER_TILE + width - 1 - i] = size
    if U > PLANT_GROW_USER and PLANT_GROW_USER not in planted:
        planted[PLANT_GROW_USER] = 65
    return planted


def plant_row_end(t0, j):
    """`end` of row j of a planted bucket: rows 0..15 outlive every stage, row 16, rows 17..32, rows 33..63 and row 64 end one
    hour apart, so that the queries of stage k (user_axis_queries) select exactly the first PLANT_STAGE_ROWS[k] of them."""
    tier = 0 if j < 16 else 1 if j < 17 else 2 if j < 33 else 3 if j < 64 else 4
    return t0 + HOUR if tier == 0 else t0 - (tier + 1) * HOUR


def user_axis_queries(t0, k, stage):
    """k heterogeneous top-of-range queries (distinct now, cutoff and mask, as tests/test_gpu_batch.py mixes them) whose `now`
    values all lie between the ends of two tiers of the planted rows: within ten and a half minutes below
    t0 - (stage + 2) h + 30 min.  Query 0 has every discipline and a cutoff below every planted start, so the union of any
    prefix of the list holds every planted row that is live at that stage; the others select subsets of them."""
    base = t0 - (stage + 2) * HOUR + HOUR // 2
    masks = [ALL, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0x00000000FFFF0000, 0x1, 0x8000000000000001]
    return [(base - 977 * i - (i % 3) * 60000, t0 - (65 - i % 4) * DAY - 13 * i, masks[i % len(masks)]) for i in range(k)]


def plant_user_buckets(cols, U, D, t0, seed=7):
    """Copies of the columns with the buckets of plant_users(U) written into them.  Rows the planted users had are given an
    `end` thirty days back (no stage selects them); every planted user then gets `size` rows taken from the other users at
    seeded positions all over the table: starts on five values a day apart that straddle the queries' cutoffs (runs of equal
    starts, so the (start, row) order is decided by the row index), ends by plant_row_end, disciplines in steps of five.
    -> ((start, end, user, disc), {user: size})"""
    s, e, u, d = [np.array(c) for c in cols]
    planted = plant_users(U)
    is_planted = np.zeros(U, bool)
    is_planted[list(planted)] = True
    own = is_planted[u]
    e[own] = t0 - 30 * DAY
    pool = np.random.default_rng(seed).permutation(np.nonzero(~own)[0])
    starts = np.array([t0 - 64 * DAY - 12 * HOUR + k * DAY for k in range(5)], np.int64)
    at = 0
    for pi, user in enumerate(sorted(planted)):
        size = planted[user]
        rows, at = pool[at:at + size], at + size
        assert rows.size == size, "the table is too small for the planted buckets"
        j = np.arange(size)
        u[rows] = user
        s[rows] = starts[(j * 3 + j // 7 + pi) % 5]
        e[rows] = [plant_row_end(t0, int(x)) for x in j]
        d[rows] = (j * 5 + pi) % D
    return (s, e, u, d), planted


def union_sizes(cols, U, D, queries):
    """int64[U]: rows of every user that at least one query selects (plain numpy, no sort)."""
    s, e, u, d = cols
    lim = ALL if D >= 64 else (1 << D) - 1
    cand = np.nonzero(e > min(q[0] for q in queries))[0]
    cs, ce, cd = s[cand], e[cand], d[cand]
    ok = (cd >= 0) & (cd < 64)
    sh = np.where(ok, cd, 0).astype(np.uint64)
    any_q = np.zeros(cand.size, bool)
    for now, cutoff, mask in queries:
        bit = ok & (((np.uint64(mask & lim) >> sh) & np.uint64(1)) == 1)
        any_q |= (ce > now) & (cs >= cutoff) & bit
    return np.bincount(u[cand[any_q]], minlength=U).astype(np.int64)


def union_from_answers(start, user, U, answers):
    """The union of a batch from its queries' answers: per user the rows any query selects in (start, row) order, and
    ceil(Q / 64) mask words per row.  -> (uoff int64[U + 1], rows int32[Mu], masks uint64[Mu, words])"""
    words = (len(answers) + 63) // 64
    bits = np.zeros((start.size, words), np.uint64)
    for q, (_, _, idx) in enumerate(answers):
        bits[idx, q // 64] |= np.uint64(1 << (q % 64))
    rows = np.nonzero(bits.any(axis=1))[0]
    rows = rows[np.lexsort((rows, start[rows], user[rows]))]
    uoff = np.zeros(U + 1, np.int64)
    np.cumsum(np.bincount(user[rows], minlength=U), out=uoff[1:])
    return uoff, rows.astype(np.int32), bits[rows]


def union_message(U, u_pad, cap, union, n_q, wide):
    """The exchange message of a union (include/pie_scan.h): [uoff[0..U] | Mu up to word u_pad + 1 | rows[cap) | masks], the
    masks as mask_lo[cap) (| mask_hi[cap) above 32 queries) for an ordinary batch and as 2 * words int32 per row for a wide one.
    -> (int32 message, bool mask of the words the library writes: those of rows beyond Mu or cap are left alone)"""
    uoff, rows, masks = union
    mu, words = int(rows.size), masks.shape[1]
    k = min(mu, cap)
    per_row = 1 + 2 * words if wide else 3 if n_q > 32 else 2
    msg, written = np.zeros(u_pad + 2 + cap * per_row, np.int32), np.zeros(u_pad + 2 + cap * per_row, bool)
    msg[: U + 1], msg[U + 1: u_pad + 2] = uoff.astype(np.int32), mu
    written[: u_pad + 2] = True
    at = u_pad + 2
    msg[at: at + k], written[at: at + k] = rows[:k], True
    at += cap
    if wide:
        msg[at: at + k * 2 * words] = np.ascontiguousarray(masks[:k]).reshape(-1).view(np.int32)
        written[at: at + k * 2 * words] = True
    else:
        halves = np.ascontiguousarray(masks[:k, 0]).view(np.int32).reshape(k, 2)
        msg[at: at + k], written[at: at + k] = halves[:, 0], True
        if n_q > 32:
            msg[at + cap: at + cap + k], written[at + cap: at + cap + k] = halves[:, 1], True
    return msg, written


# ------------------------------------------------------------------------------------------------ the seeded chain
def same(got, want, tag):
    for name, a, b in zip(("counts", "offsets", "idx"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), (tag, name)


def check_union(tag, un, wants, wide):
    """Every query's list is a filter of the union, in order; no union row without a query, no bit beyond the batch."""
    uoff, rows, masks = un
    nq = len(wants)
    bits = masks.reshape(rows.size, (nq + 63) // 64)
    any_bit = np.zeros(rows.size, bool)
    for qi, w in enumerate(wants):
        sel = ((bits[:, qi // 64] >> np.uint64(qi % 64)) & np.uint64(1)) == 1
        any_bit |= sel
        csum = np.concatenate([[0], np.cumsum(sel)])
        assert np.array_equal(rows[sel], w[2]) and np.array_equal(csum[uoff], w[1]), (tag, "union", "wide" if wide else "", qi)
    assert np.all(any_bit), (tag, "a union row no query selected")
    if nq % 64:
        assert not np.any(bits[:, nq // 64] >> np.uint64(nq % 64)), (tag, "a query bit beyond the batch")


def ctx_with_env(pie, hot=None, async_mut=None, **env):
    """A context created under PIE_HOT_INDEX / PIE_ASYNC_MUTATIONS (where given) and any further variables passed by name; the
    environment is restored before returning."""
    want = dict(env)
    if hot is not None:
        want["PIE_HOT_INDEX"] = "1" if hot else "0"
    if async_mut is not None:
        want["PIE_ASYNC_MUTATIONS"] = "1" if async_mut else "0"
    old = {k: os.environ.get(k) for k in want}
    os.environ.update(want)
    try:
        return pie.PieScan(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def shard_owner(oracle, owner, n_users, world):
    """owner[u] = the shard user u hashes to, extended from the users `owner` already covers to n_users."""
    more = [oracle.shard_of(u, world) for u in range(owner.size, n_users)]
    return np.concatenate([owner, np.array(more, np.int32)]) if more else owner


def shard_view(m, rank, owner):
    """The shard `rank` holds of the UNSHARDED model m, as a model of its own: the rows of the users with owner[u] == rank in
    table order, those users re-numbered densely in ascending global id (a shard without a user keeps one).
    -> (model, global rows it holds ascending, global users ascending)"""
    rows = np.nonzero(owner[m.user] == rank)[0] if m.n else np.zeros(0, np.int64)
    users = np.nonzero(owner[:m.U] == rank)[0]
    local = np.full(m.U, -1, np.int32)
    local[users] = np.arange(users.size, dtype=np.int32)
    v = TableModel(m.oracle)
    v.load(m.start[rows], m.end[rows], local[m.user[rows]], m.disc[rows], max(int(users.size), 1), m.D)
    return v, rows.astype(np.int32), users.astype(np.int32)


# ------------------------------------------------------------------------------------------------ key-edge sweeps
class Edge:
    """A hand-made table in a context and in the model; sweeps of queries compared one by one."""

    def __init__(self, pie, oracle, cols, U, D, hot=1, ordered=1, async_mut=1):
        self.m = TableModel(oracle)
        self.m.load(*cols, U, D)
        self.ctx = ctx_with_env(pie, hot, async_mut)
        self.ctx.set_ordered_run(ordered)
        self.ctx.load_columns(*self.m.columns(), U)
        self.ctx.set_disciplines(ALL, D)

    def columns_match(self, tag):
        for name, got, want in zip(("start", "end", "user", "disc"), self.ctx.read_columns(), self.m.columns()):
            assert got.dtype == want.dtype and np.array_equal(got, want), (tag, "column " + name)

    def sweep(self, tag, queries, single_every=9):
        ctx, m = self.ctx, self.m
        for b in range(0, len(queries), 64):
            qs = queries[b:b + 64]
            wants = m.scan_many(qs)
            got = ctx.scan_batch(qs)
            for qi in range(len(qs)):
                same(got[qi], wants[qi], (tag, "batch at", b, "query", qs[qi]))
        for now, cutoff, mask in queries[::single_every]:
            ctx.set_disciplines(mask, m.D)
            same(ctx.scan(now, cutoff), m.scan(now, cutoff, mask), (tag, "single scan", now, cutoff, mask))
        ctx.set_disciplines(ALL, m.D)

    def set_end(self, tag, rows, ne):
        rows, ne = np.asarray(rows, np.int32), np.asarray(ne, np.int64)
        self.ctx.set_end(rows, ne)
        self.m.set_end(rows, ne)
        self.columns_match(tag)


def around(values):
    nows = sorted({int(v) + k for v in values for k in (-1, 0, 1) if INT64_MIN < int(v) + k <= INT64_MAX})
    return nows


def liveness_queries(oracle, nows):
    masks = [ALL, 0x55555555, 0xAAAAAAAA, 0x1, 0x80000001]
    cutoffs = [INT64_MIN, oracle.T0_MS - 40 * DAY]
    return [(now, cutoffs[i % 2], masks[i % 5]) for i, now in enumerate(nows)]


def chain_config(seed):
    rng = np.random.default_rng([seed, 0xC0F])
    return {
        "n": int(rng.choice([1, 65, 4099, 70001, 300007, 1 << 20])), "U": int(rng.choice([1, 3, 997, 40009])),
        "D": int(rng.choice([1, 7, 32, 64])), "flags": int(rng.integers(8)), "heavy": bool(rng.random() < 0.3),
        "hourly": bool(rng.random() < 0.3), "hot": int(rng.integers(2)), "ordered": int(rng.integers(3)),
        "lanes": int(rng.integers(1, 5)), "async": int(rng.integers(2)), "steps": int(rng.integers(30, 61)),
        "gen_seed": int(rng.integers(1, 2 ** 60)),
    }


class Chain:
    """One seeded chain: a table, a context configuration, 30 to 60 steps.  run() raises at the first difference."""

    MUTATORS = ("set_end", "set_end", "set_end", "append", "append", "delete_user", "prune", "retention", "shard", "flood")
    READERS = ("scan", "scan", "batch", "batch", "batch", "wide", "pipeline", "expired", "archive")

    def __init__(self, pie, oracle, seed, cfg=None, log=None):
        self.pie, self.oracle, self.seed = pie, oracle, seed
        self.cfg = dict(chain_config(seed), **(cfg or {}))
        self.rng = np.random.default_rng([seed, 0x57E9])
        self.rng_after = np.random.default_rng([seed, 0xAF7E])   # the batch that follows every append draws from its own stream
        self.m = TableModel(oracle)
        self.paths = {}
        self.both_valid_at_set_end = False
        self.rebuilt_after_drop = False
        self.sharded = False
        self.touched = True       # a touch or append since hot_builds last rose (nothing is built yet)
        self.builds_seen, self.dropped = 0, False
        self.log = log
        self.t0 = oracle.T0_MS

    # ---- set-up
    def make_table(self):
        c, rng, o = self.cfg, self.rng, self.oracle
        n, U, D = c["n"], c["U"], c["D"]
        s, e, u, d = [a.copy() for a in o.gen(c["gen_seed"], n, 0, n, U, D, c["flags"])]
        if c["heavy"]:
            u = np.where(rng.random(n) < 0.5, int(rng.integers(U)), u).astype(np.int32)
        if c["hourly"]:
            e, s = (e // HOUR) * HOUR, (s // HOUR) * HOUR
        self.m.load(s, e, u, d, U, D)
        self.mask = ALL if rng.random() < 0.4 else int(rng.integers(0, 2 ** 63)) | (int(rng.integers(0, 2)) << 63) | 1

    def run(self):
        self.make_table()
        c = self.cfg
        ctx = self.ctx = ctx_with_env(self.pie, c["hot"], c["async"])
        try:
            ctx.set_ordered_run(c["ordered"])
            ctx.set_batch_lanes(c["lanes"])
            ctx.load_columns(*self.m.columns(), self.m.U)
            ctx.set_disciplines(self.mask, self.m.D)
            self.check_columns("load")
            for step in range(c["steps"]):
                # the chain opens with readers (they build the ordered run and the hot index), then mixes
                kind = self.rng.choice(self.READERS) if step < 3 or self.rng.random() < 0.5 else self.rng.choice(self.MUTATORS)
                if self.log:
                    self.log("seed %d step %d %s n %d U %d" % (self.seed, step, kind, self.m.n, self.m.U))
                getattr(self, "do_" + str(kind))("seed %d step %d %s" % (self.seed, step, kind))
                self.watch_index()
        finally:
            ctx.close()
        return self

    # ---- bookkeeping
    def saw(self, path):
        assert path in PATHS, path
        self.paths[path] = self.paths.get(path, 0) + 1

    def watch_index(self):
        info = self.ctx.table_info()
        if info["hot_builds"] > self.builds_seen:
            if self.dropped:
                self.rebuilt_after_drop = True
            self.builds_seen, self.dropped, self.touched = info["hot_builds"], False, False
        elif self.builds_seen and info["hot_rows"] == 0:
            self.dropped = True
        return info

    def check_columns(self, tag):
        assert self.ctx.n == self.m.n and self.ctx.n_users == self.m.U, (tag, "shape")
        assert int(self.ctx.stats()["rows"]) == self.m.n and int(self.ctx.stats()["users"]) == self.m.U, (tag, "stats shape")
        for name, got, want in zip(("start", "end", "user", "disc"), self.ctx.read_columns(), self.m.columns()):
            assert got.dtype == want.dtype and np.array_equal(got, want), (tag, "column " + name)

    # ---- queries: sparse top-of-range, below the 90th percentile, dense, above everything; on values and next to them
    def ends_in_range(self):
        e = self.m.end
        e = e[(e != INT64_MIN) & (e < self.t0 + YEAR)]
        return e if e.size else np.array([self.t0], np.int64)

    def pick_now(self, kind):
        rng, e = self.rng, self.ends_in_range()
        if kind == "above":      # at or above every end: selects nothing
            top = int(self.m.end.max()) if self.m.n else 0
            return top if top == INT64_MAX or rng.random() < 0.5 else int(rng.integers(top, min(top + DAY, INT64_MAX)))
        if kind == "far":        # above the range the keys were fitted for (rows re-ended far ahead are still live there)
            return int(rng.choice([INT64_MAX - 1, int(e.max()), self.t0 + 10 * YEAR, self.t0 + 11 * YEAR]))
        if kind == "dense":
            return int(rng.choice([INT64_MIN, int(np.quantile(e, 0.3)), int(e.min()) - 1]))
        if kind == "below_p90":
            return int(np.quantile(e, float(rng.uniform(0.80, 0.895))))
        lo = int(np.quantile(e, 0.97))
        now = int(rng.integers(lo, int(e.max()) + 1))
        r = rng.random()
        if r < 0.3:      # exactly on a value of the column, or one below it
            v = e[e >= lo]
            now = int(v[int(rng.integers(v.size))]) - int(rng.integers(2))
        return now

    def pick_query(self, kind):
        rng, m = self.rng, self.m
        cutoff = int(rng.choice([INT64_MIN, self.t0 - 61 * DAY, int(m.start[int(rng.integers(m.n))]) if m.n else 0]))
        mask = ALL if rng.random() < 0.4 else int(rng.integers(0, 2 ** 63)) | (int(rng.integers(0, 2)) << 63)
        return self.pick_now(kind), cutoff, mask

    def query_set(self, k, dense=True):
        """k queries of all four kinds (k >= 4: at least one of each; smaller sets take them in turn)."""
        kinds = ["sparse", "below_p90", "dense", "above", "far"] if dense else ["sparse", "above", "sparse", "far"]
        qs = [self.pick_query(kinds[i] if i < len(kinds) else "sparse") for i in range(k)]
        if k < len(kinds):
            qs = [self.pick_query(kinds[int(self.rng.integers(len(kinds)))]) for _ in range(k)]
        order = self.rng.permutation(k)
        return [qs[int(i)] for i in order]

    # ---- readers
    def do_scan(self, tag):
        ctx, m = self.ctx, self.m
        for kind in ("sparse", "sparse", "sparse", "below_p90", "dense", "above"):
            now = self.pick_now(kind)
            cutoff = int(self.rng.choice([INT64_MIN, self.t0 - 61 * DAY]))
            want = m.scan(now, cutoff, self.mask)
            reps = 3 if kind == "sparse" else 1      # repeats let the adaptive forms engage
            for _ in range(reps):
                same(ctx.scan(now, cutoff), want, (tag, kind, now, cutoff))
                v = ctx.stats()["k1_variant"]
                self.saw("ordered_scan" if v & 0x2000 else "keyed_1byte" if v & 0x800 else "keyed_2byte" if v & 0x400 else "general")
            for u in {0, m.U - 1, int(self.rng.integers(m.U)), -1, m.U}:
                feed = want[2][want[1][u]:want[1][u + 1]] if 0 <= u < m.U else np.zeros(0, np.int32)
                assert np.array_equal(ctx.read_user_feed(u), feed), (tag, kind, "feed of user", u)

    def batch_path(self, hot_rows_at_begin):
        v = self.ctx.stats()["k1_variant"]
        if v == 0:
            return "general"
        if v & 0x2000:
            return "ordered_batch"
        if not v & 0x800:
            return "keyed_2byte"
        if not hot_rows_at_begin:
            return "keyed_1byte"
        return "hot_delta" if self.touched else "hot_clean"

    def check_batch_results(self, tag, qs, wants, which=None):
        ctx, m = self.ctx, self.m
        for qi in (range(len(qs)) if which is None else which):
            same(ctx.batch_read_results(qi), wants[qi], (tag, "query", qi, qs[qi]))
        for _ in range(3):
            qi, u = int(self.rng.integers(len(qs))), int(self.rng.integers(m.U))
            w = wants[qi]
            assert np.array_equal(ctx.batch_read_user_feed(qi, u), w[2][w[1][u]:w[1][u + 1]]), (tag, "feed", qi, u)

    def check_union(self, tag, un, wants, wide):
        check_union(tag, un, wants, wide)

    def one_batch(self, tag, qs):
        ctx = self.ctx
        wants = self.m.scan_many(qs)
        ctx.scan_batch_begin(qs)
        hot_rows = self.watch_index()["hot_rows"]
        ms = ctx.scan_batch_finish()
        assert list(ms) == [int(w[2].size) for w in wants], (tag, "M per query")
        self.saw(self.batch_path(hot_rows))
        un = ctx.batch_read_union()
        if un is not None:
            self.check_union(tag, un, wants, False)
        self.check_batch_results(tag, qs, wants)
        return un is not None

    def do_batch(self, tag):
        k = int(self.rng.choice([1, 3, 16, 33, 64]))
        self.one_batch((tag, k, "mixed"), self.query_set(k))
        # the same shape without the dense query: a batch that keeps its union
        self.one_batch((tag, k, "sparse"), self.query_set(k, dense=False))

    def one_wide(self, tag, qs):
        ctx = self.ctx
        wants = self.m.scan_many(qs)
        ctx.scan_wide_begin(qs)
        self.watch_index()
        ms = ctx.scan_wide_finish()
        assert ms == [int(w[2].size) for w in wants], (tag, "M per query")
        un = ctx.batch_read_union_wide()
        v = ctx.stats()["k1_variant"]
        if un is not None:
            self.saw("wide_pass")
            self.check_union(tag, un, wants, True)
        else:
            self.saw("ordered_batch" if v & 0x2000 else "wide_fallback")
        # per query: all of them on small tables, a spread of them on large ones (the union check covers every query)
        which = None if self.m.n <= 5000 else sorted({0, len(qs) - 1} | {int(i) for i in self.rng.integers(0, len(qs), 24)})
        self.check_batch_results(tag, qs, wants, which)

    def do_wide(self, tag):
        k = int(self.rng.choice([65, 200, 512]))
        self.one_wide((tag, k, "mixed"), self.query_set(k))
        self.one_wide((tag, k, "sparse"), self.query_set(k, dense=False))

    def do_pipeline(self, tag):
        """Batches begun until the lanes are full, one wide batch among them; one more begin and a mutation are refused with
        PIE_E_STATE; everything is finished in the order it was begun."""
        ctx, rng = self.ctx, self.rng
        begun = []
        wide_at = int(rng.integers(0, 3))
        while ctx.batch_room() > 0:
            assert len(begun) < 12, (tag, "more than twelve batches in flight")
            wide = len(begun) == wide_at
            qs = self.query_set(int(rng.choice([70, 130])) if wide else int(rng.choice([3, 5, 16, 40])), dense=len(begun) == 1)
            (ctx.scan_wide_begin if wide else ctx.scan_batch_begin)(qs)
            begun.append((wide, qs, self.watch_index()["hot_rows"]))
        for call in (lambda: ctx.scan_batch_begin(begun[0][1] if not begun[0][0] else begun[1][1]),
                     lambda: ctx.set_end(np.zeros(1, np.int32), np.full(1, self.t0, np.int64)),
                     lambda: ctx.append_rows(self.m.start[:1], self.m.end[:1], self.m.user[:1], self.m.disc[:1], self.m.U)):
            n_before = ctx.n
            try:
                call()
            except self.pie.PieError as exc:
                assert exc.code == PIE_E_STATE, (tag, "refused with", exc.code)
                ctx.n = n_before
            else:
                raise AssertionError((tag, "a call the header refuses while batches are in flight went through"))
        for k, (wide, qs, hot_rows) in enumerate(begun):
            wants = self.m.scan_many(qs)
            if wide:
                try:
                    ctx.scan_batch_finish()
                except self.pie.PieError as exc:   # the oldest batch is wide: nothing consumed
                    assert exc.code == PIE_E_STATE, (tag, "batch finish of a wide batch", exc.code)
                else:
                    raise AssertionError((tag, "pie_scan_batch_finish took a wide batch"))
                ms = ctx.scan_wide_finish()
                un = ctx.batch_read_union_wide()
                self.saw("wide_pass" if un is not None else "ordered_batch" if ctx.stats()["k1_variant"] & 0x2000 else "wide_fallback")
            else:
                ms = list(ctx.scan_batch_finish())
                un = ctx.batch_read_union()
                self.saw(self.batch_path(hot_rows))
            assert ms == [int(w[2].size) for w in wants], (tag, "batch", k, "M per query")
            if un is not None:
                self.check_union((tag, "batch", k), un, wants, wide)
            self.check_batch_results((tag, "batch", k), qs, wants, sorted({0, len(qs) - 1, int(rng.integers(len(qs)))}))
        assert ctx.batch_room() >= 3, (tag, "room after the burst")

    def do_expired(self, tag):
        now = self.pick_now(str(self.rng.choice(["sparse", "below_p90", "above", "dense"])))
        prev = now - int(self.rng.integers(0, 3 * DAY)) if now > INT64_MIN + 4 * DAY else INT64_MIN
        assert np.array_equal(self.ctx.expired_queue(prev, now), self.m.expired_queue(prev, now)), (tag, prev, now)

    def do_archive(self, tag):
        m = self.m
        if m.n > 300007:
            return self.do_expired(tag)
        now = int(self.rng.choice([self.t0, self.t0 - 100 * DAY, self.t0 - 119 * DAY, int(m.start[int(self.rng.integers(m.n))]) if m.n else 0, 2 ** 62, INT64_MIN + 5]))
        win = int(self.rng.choice([0, HOUR, 12 * HOUR, 30 * DAY, 2 ** 62]))
        assert np.array_equal(self.ctx.archive_queue(now, win), m.archive_queue(now, win)), (tag, now, win)

    # ---- mutators
    def mutated(self, tag, touch):
        if touch:
            self.touched = True
        self.check_columns(tag)

    def apply_set_end(self, tag, rows, ne):
        info = self.ctx.table_info()
        if info["ordered_rows"] > 0 and info["hot_rows"] > 0:
            self.both_valid_at_set_end = True
        self.ctx.set_end(rows, ne)
        self.m.set_end(rows, ne)
        self.mutated(tag, True)

    def do_set_end(self, tag):
        rng, m, t0 = self.rng, self.m, self.t0
        if m.n == 0:
            return
        e = m.end
        parts = []

        def take(pool, k, values):
            pool = np.asarray(pool)
            if pool.size:
                r = rng.choice(pool, min(k, pool.size), replace=False)
                parts.append((r, values(r.size)))

        k = int(rng.choice([1, 7, 200, 3000]))
        kinds = rng.choice(["raise", "held", "tomb", "revive", "far", "any"], 3, replace=False)
        for kind in kinds:
            if kind == "raise":      # rows far below the index's range, into it
                take(np.nonzero((e != INT64_MIN) & (e < t0 - 30 * DAY))[0], k, lambda c: t0 + rng.integers(-6 * HOUR, 12 * HOUR, c))
            elif kind == "held":     # rows it holds, up and down
                take(np.nonzero(e > t0 - 12 * HOUR)[0], k, lambda c: t0 + rng.integers(-20 * DAY, 12 * HOUR, c))
            elif kind == "tomb":
                take(np.nonzero(e != INT64_MIN)[0], max(k // 4, 1), lambda c: np.full(c, INT64_MIN))
            elif kind == "revive":
                take(np.nonzero(e == INT64_MIN)[0], k, lambda c: t0 + rng.integers(-HOUR, 6 * HOUR, c))
            elif kind == "far":      # far above the range the keys were fitted for
                take(np.arange(m.n), max(k // 8, 2), lambda c: rng.choice(np.array([t0 + 10 * YEAR, INT64_MAX, t0 + 10 * YEAR + 1], np.int64), c))
            else:
                take(np.arange(m.n), k, lambda c: rng.integers(t0 - 200 * DAY, t0 + 50 * DAY, c))
        if not parts:
            take(np.arange(m.n), k, lambda c: rng.integers(t0 - 200 * DAY, t0 + 50 * DAY, c))
        rows = np.concatenate([p[0] for p in parts]).astype(np.int32)
        ne = np.concatenate([p[1] for p in parts]).astype(np.int64)
        _, first = np.unique(rows, return_index=True)   # one value per row in a call
        first.sort()
        rows, ne = rows[first], ne[first]
        twice = rng.integers(0, rows.size, max(rows.size // 10, 1))   # the same row again, with the same value
        at = rng.permutation(rows.size + twice.size)
        rows, ne = np.concatenate([rows, rows[twice]])[at], np.concatenate([ne, ne[twice]])[at]
        self.apply_set_end(tag, rows, ne)

    def do_flood(self, tag):
        """Enough touches in one call to pass the delta's bound on the second (the index is dropped and rebuilt)."""
        m = self.m
        if m.n < 70001:
            return self.do_set_end(tag)
        rows = self.rng.choice(m.n, 40000, replace=False).astype(np.int32)
        ne = (self.t0 + self.rng.integers(-6 * HOUR, 12 * HOUR, rows.size)).astype(np.int64)
        self.apply_set_end(tag, rows, ne)

    def do_append(self, tag):
        rng, m, t0 = self.rng, self.m, self.t0
        mode = str(rng.choice(["ordered", "ordered", "late", "burst", "users"]))
        k = int(rng.choice([1, 40, 1500]))
        if mode == "burst":          # more rows than the table holds: the columns are re-allocated
            k = m.n + 1
        if m.n + k > MAX_ROWS:
            return self.do_set_end(tag)
        U = m.U + (int(rng.integers(1, 40)) if mode == "users" else 0)
        top = int(m.start.max()) if m.n else t0
        if mode == "late":
            s2 = top - rng.integers(0, 20 * HOUR, k)
        else:
            s2 = top + np.sort(rng.integers(0, 4000, k))
        s2 = s2.astype(np.int64)
        e2 = s2 + rng.integers(-2 * DAY, DAY, k)
        e2 = np.where(rng.random(k) < 0.5, t0 + rng.integers(-12 * HOUR, 12 * HOUR, k), e2).astype(np.int64)
        u2, d2 = rng.integers(0, U, k).astype(np.int32), rng.integers(0, m.D, k).astype(np.int32)
        if mode == "users":
            u2[-1] = U - 1
        self.ctx.append_rows(s2, e2, u2, d2, U)
        m.append_rows(s2, e2, u2, d2, U)
        self.mutated((tag, mode, k), True)
        # a top-of-range batch at once: an append that re-allocated has dropped the hot index and this batch rebuilds it, so
        # that the next append, which lands in place, is mirrored into a live index and read back from it by the batch after it
        main, self.rng = self.rng, self.rng_after
        try:
            self.one_batch((tag, mode, k, "batch after the append"), self.query_set(16, dense=False))
        finally:
            self.rng = main

    def listed(self, tag, got, want):
        assert got.dtype == want.dtype and np.array_equal(got, want), (tag, "rows listed")
        self.mutated(tag, False)

    def do_delete_user(self, tag):
        m = self.m
        u = int(self.rng.integers(-1, m.U + 1))
        if m.n and self.rng.random() < 0.3:
            u = int(np.bincount(m.user, minlength=m.U).argmax())
        self.listed((tag, u), self.ctx.delete_user(u), m.delete_user(u))

    def do_prune(self, tag):
        m = self.m
        cutoff = int(np.quantile(m.start, float(self.rng.uniform(0, 0.05)))) + int(self.rng.integers(2)) if m.n else 0
        self.listed((tag, cutoff), self.ctx.prune_before(cutoff), m.prune_before(cutoff))

    def do_retention(self, tag):
        m = self.m
        months, tz = int(self.rng.choice([1, 2, 3])), int(self.rng.choice([0, 0, 330 * 60000, -5 * HOUR]))
        first = int(m.start.min()) if m.n else self.t0
        now = int(add_months(np.array([first], np.int64), months, tz)[0]) + int(self.rng.integers(-DAY, 4 * DAY))
        self.listed((tag, now, months, tz), self.ctx.retention_purge(now, months, tz), m.retention_purge(now, months, tz))

    def do_shard(self, tag):
        m = self.m
        world = int(self.rng.choice([2, 3]))
        rank = int(self.rng.integers(world))
        if self.sharded or m.U < 3 or m.shard_rows(rank, world)[1].size == 0:
            return self.do_delete_user(tag)
        self.sharded = True
        got = self.ctx.shard_table(rank, world)
        assert got == m.shard_table(rank, world), (tag, "shard shape", got)
        self.ctx.set_disciplines(self.mask, m.D)
        self.mutated((tag, rank, world), True)


def run_chain(pie, oracle, seed, cfg=None, log=None):
    return Chain(pie, oracle, seed, cfg, log).run()
