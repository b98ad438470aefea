"""TEST INFRASTRUCTURE — designed tables for the archive queue (pie_archive_queue, pie_queue_pack_device, pie_comm_archive_queue),
no GPU.

test_archive_cases_cpu.py shows with the oracle alone that every table plants what it claims; test_gpu_archive_paths.py runs them
through the C ABI, comm_archive_worker.py through the communicator.

build(name, n_cus) -> (start, end, user, disc, n_users, [(now, window), ..], props).  props declares, per query and from the
construction alone (never from an oracle): `order` (the qualifying groups in the order of their first present row), `sizes`
(their present rows), `q`, `n_qual`; and the named `boundary` the table sits on.  `numpy_ok[k]` is False where the numpy twin's
INT64_MAX sentinel makes it ambiguous.  names() lists every case (they do not depend on n_cus; the tables of n_qual-grid and
many_rows do); FAMILIES groups them.

What the tables rely on (restated from pie_scan.hip / pie_kernels.h): the streaming plan at these sizes has blocks of 4 096 rows; a
select step takes 512 rows, two neighbouring rows per thread; the qualifying-groups bitmap sits in LDS up to 48 KiB (393 216
users); k_arch_heads strides past 16 x CUs x 256 selected rows, k_arch_gather past 16 x CUs qualifying groups; the merge of the
communicator runs four groups per block and strides past 2 048 blocks.

Default columns: an `old` row starts at or before T0 - W (it qualifies its group at the query (T0, W)), every other row after it;
a tombstone has end = INT64_MIN."""
import numpy as np

HOUR = 3600 * 1000
DAY = 24 * HOUR
T0 = 1700000000000
W = 12 * HOUR
LIMIT = T0 - W
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
STEP, BLOCK = 512, 4096
LDS_USERS = 393216   # 48 KiB of bitmap words

PLACEMENT_N = (1, 2, 511, 512, 513, 4095, 4096, 4097, 8193)
PLACEMENT_PATTERNS = ("none", "all", "row_0", "last_row", "last_of_every_step", "first_of_every_block_but_the_first", "pair_both",
                      "pair_even", "pair_odd", "mix", "tail_decides")
BITMAP_U = (1, 2, 3, 31, 32, 33, 64, 65)
SORT_U = (256, 257, 65536, 65537)
GROUP_SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
PACK_FAMILIES = ("group_sizes", "order", "n_qual", "tombstones")   # the families whose queues are also packed


def default_start(old):
    i = np.arange(old.size, dtype=np.int64)
    return np.where(old, LIMIT - (i % 977), LIMIT + 1 + (i % 1009))


def declare(user, present, n_users, qual):
    """(order, sizes) of one query: the groups of `qual` by their first present row, and their present rows"""
    rows = np.nonzero(present)[0]
    counts = np.bincount(user[rows], minlength=n_users)
    first = np.full(n_users, user.size, np.int64)
    np.minimum.at(first, user[rows], rows)
    qual = sorted(int(g) for g in qual)
    assert all(counts[g] > 0 for g in qual), "a designed group has no present row"
    order = sorted(qual, key=lambda g: first[g])
    return order, [int(counts[g]) for g in order]


def make(family, boundary, user, n_users, quals, start=None, old=None, tomb=None, queries=((T0, W),), numpy_ok=None, **extra):
    user = np.asarray(user, np.int32)
    n = user.size
    tomb = np.zeros(n, bool) if tomb is None else np.asarray(tomb, bool)
    start = default_start(np.asarray(old, bool)) if start is None else np.asarray(start, np.int64)
    i = np.arange(n, dtype=np.int64)
    end = np.where(tomb, INT64_MIN, T0 + DAY + i)
    disc = (i % 32).astype(np.int32)
    assert len(quals) == len(queries)
    decl = [declare(user, ~tomb, n_users, q) for q in quals]
    props = dict(family=family, boundary=boundary, order=[d[0] for d in decl], sizes=[d[1] for d in decl],
                 q=[sum(d[1]) for d in decl], n_qual=[len(d[0]) for d in decl],
                 numpy_ok=[True] * len(queries) if numpy_ok is None else list(numpy_ok), **extra)
    return start, end, user, disc, int(n_users), [(int(a), int(b)) for a, b in queries], props


# ------------------------------------------------------------------------------------------------ placement
def placement_valid(n, pattern):
    if pattern.startswith("pair"):
        return n >= 2
    if pattern == "tail_decides":
        return n % 2 == 1 and n >= 3
    if pattern == "last_of_every_step":
        return n >= STEP
    if pattern == "first_of_every_block_but_the_first":
        return n > BLOCK
    return True


def placement_hits(pattern, n):
    h = np.zeros(n, bool)
    pair = 2 * ((n // 2) // 2)   # an even row whose odd neighbour exists: the two rows of one thread
    if pattern == "all":
        h[:] = True
    elif pattern == "row_0":
        h[0] = True
    elif pattern == "last_row":
        h[n - 1] = True
    elif pattern == "last_of_every_step":
        h[STEP - 1::STEP] = True
    elif pattern == "first_of_every_block_but_the_first":
        h[BLOCK::BLOCK] = True
    elif pattern == "pair_both":
        h[[pair, pair + 1]] = True
    elif pattern == "pair_even":
        h[pair] = True
    elif pattern == "pair_odd":
        h[pair + 1] = True
    elif pattern == "mix":
        h = np.random.default_rng(n).random(n) < 0.5
    elif pattern == "tail_decides":
        h[n - 1] = True
    return h


def placement(n, pattern):
    """Group 0 owns exactly the rows of the pattern, all old; every other row belongs to the young groups 1 .. 4.  tail_decides:
    group 0 also owns rows 0 and n // 2, both young — its only old row is the last row of an odd table."""
    h = placement_hits(pattern, n)
    user = 1 + np.arange(n) % 4
    user[h] = 0
    if pattern == "tail_decides":
        user[[0, n // 2]] = 0
    return make("placement", pattern, user, 6, [{0} if h.any() else set()], old=h, hits=h)


# ------------------------------------------------------------------------------------------------ threshold
def threshold():
    """Seven groups of four rows, first appearing in descending id order; a group's third row carries its deciding start, every
    other row starts a day after T0.  Group 3 has one present row, start = INT64_MAX; group 4 is tombstoned throughout."""
    n = 28
    i = np.arange(n)
    user, rnd = 6 - i % 7, i // 7
    deciding = {0: LIMIT, 1: LIMIT + 1, 2: INT64_MIN, 3: INT64_MAX, 4: LIMIT - 5, 5: T0, 6: T0 + 1}
    start = np.full(n, T0 + DAY, np.int64)
    for g, s in deciding.items():
        start[(user == g) & (rnd == 2)] = s
    tomb = (user == 4) | ((user == 3) & (rnd != 2))
    cases = [((T0, W), {0, 2}, True),                                  # start == now - window qualifies, + 1 does not
             ((T0, W - 1), {0, 1, 2}, True),
             ((T0, 0), {0, 1, 2, 5}, True),                            # window = 0
             ((T0 + 1, 0), {0, 1, 2, 5, 6}, True),
             ((INT64_MIN + 5, 10), set(), True),                       # now - window below INT64_MIN
             ((INT64_MIN + W, W), {2}, True),                          # now - window == INT64_MIN: the group that starts there
             ((INT64_MAX - 5, -10), {0, 1, 2, 3, 5, 6}, False),        # now - window above INT64_MAX: every present group
             ((INT64_MAX, 0), {0, 1, 2, 3, 5, 6}, False),              # now - window == INT64_MAX
             ((INT64_MAX, 1), {0, 1, 2, 5, 6}, True)]
    return make("threshold", "limit", user, 7, [c[1] for c in cases], start=start, tomb=tomb, queries=[c[0] for c in cases],
                numpy_ok=[c[2] for c in cases], deciding=deciding)


# ------------------------------------------------------------------------------------------------ tombstones
def tombstones(which):
    if which == "all":
        n = 1000
        return make("tombstones", "all", np.arange(n) % 5, 5, [set()], old=np.ones(n, bool), tomb=np.ones(n, bool))
    # (group, old, tombstone): group 0's only old row is a tombstone; group 1's first row is one, its first present row (5) comes
    # after group 2's (1); group 3 is tombstoned throughout; group 4 is young
    head = [(1, 1, 1), (2, 1, 0), (0, 0, 0), (0, 1, 1), (3, 1, 1), (1, 0, 0), (1, 1, 0), (3, 1, 1), (0, 0, 0), (2, 0, 0), (4, 0, 0), (1, 0, 1)]
    rows = head + [(4, 0, 0)] * 601
    user, old, tomb = (np.array([r[k] for r in rows]) for k in range(3))
    return make("tombstones", "mixed", user, 6, [{1, 2}], old=old.astype(bool), tomb=tomb.astype(bool))


# ------------------------------------------------------------------------------------------------ order
def order(which):
    if which == "desc":
        n = 200
        return make("order", "desc", 39 - np.arange(n) % 40, 40, [set(range(40))], old=np.ones(n, bool))
    if which == "interleave":
        n = 1001
        return make("order", "interleave", np.where(np.arange(n) % 2 == 0, 3, 1), 5, [{1, 3}], old=np.ones(n, bool))
    n = 900   # late: group 2 appears first (row 0) and qualifies through row 700 alone; group 1 follows at row 1, old there
    user = np.where(np.arange(n) % 2 == 0, 2, 1)
    user[5::7] = 0
    old = np.zeros(n, bool)
    old[[1, 700]] = True
    assert user[700] == 2 and user[0] == 2 and user[1] == 1
    return make("order", "late", user, 4, [{1, 2}], old=old)


# ------------------------------------------------------------------------------------------------ bitmap words, sort bits, the LDS limit
def bitmap_words(U):
    """Every id has three rows, shuffled; ids 0, 31, 32, 63 and U - 1 (those below U) qualify, their neighbours do not."""
    user = np.random.default_rng(U).permutation(np.repeat(np.arange(U), 3))
    qual = {g for g in (0, 31, 32, 63, U - 1) if g < U}
    return make("bitmap_words", "U=%d" % U, user, U, [qual], old=np.isin(user, sorted(qual)))


def sort_bits(U):
    """Ids U - 1 and 0 interleave row by row and qualify; 1 and U - 2 are young.  For U = 2^k + 1 id U - 1 needs bit k."""
    n = 601
    user = np.where(np.arange(n) % 2 == 0, U - 1, 0)
    user[10::50] = 1
    user[11::50] = U - 2
    return make("sort_bits", "U=%d" % U, user, U, [{0, U - 1}], old=np.isin(user, (0, U - 1)))


def lds_limit(U):
    n = 5001
    cyc = [LDS_USERS - 1, 1, 0, LDS_USERS - 2] + ([LDS_USERS] if U > LDS_USERS else [])
    qual = {0, LDS_USERS - 1} | ({LDS_USERS} if U > LDS_USERS else set())
    user = np.array(cyc)[np.arange(n) % len(cyc)]
    return make("lds_limit", "U=%d" % U, user, U, [qual], old=np.isin(user, sorted(qual)), bitmap_bytes=((U + 31) // 32) * 4)


# ------------------------------------------------------------------------------------------------ group sizes, n_qual, many rows
def last_rows_of(user, groups):
    old = np.zeros(user.size, bool)
    for g in groups:
        old[np.nonzero(user == g)[0][-1]] = True
    return old


def group_sizes():
    """Group k has GROUP_SIZES[k] rows and qualifies through its LAST row; groups 8 and 9 are young; shuffled."""
    ids = np.concatenate([np.repeat(np.arange(len(GROUP_SIZES)), GROUP_SIZES), np.repeat([8, 9], 250)])
    user = np.random.default_rng(5).permutation(ids)
    qual = set(range(len(GROUP_SIZES)))
    return make("group_sizes", "sizes", user, 11, [qual], old=last_rows_of(user, qual))


N_QUAL = ("255", "256", "257", "grid", "8193")   # grid: one group more than the 16 x CUs blocks of k_arch_gather


def n_qual(G):
    """G groups of two rows: five young rows, the first rows in one shuffled order, the second rows (the old ones) in another."""
    rng = np.random.default_rng(G)
    user = np.concatenate([np.full(5, G), rng.permutation(G), np.full(4, G + 1), rng.permutation(G), np.full(3, G + 2)])
    old = np.zeros(user.size, bool)
    old[9 + G: 9 + 2 * G] = True
    return make("n_qual", "n_qual=%d" % G, user, G + 4, [set(range(G))], old=old)


def many_rows(n_cus):
    q = 16 * n_cus * 256 + 1
    user = np.concatenate([np.full(1000, 2), 1 - np.arange(q) % 2])
    return make("many_rows", "q=%d" % q, user, 3, [{0, 1}], old=user != 2)


# ------------------------------------------------------------------------------------------------ repeat
def repeat(which):
    if which == "flip":   # group 2 qualifies at T0, not 20 ms earlier, then again; group 0 always, group 1 never
        n = 300
        user = np.array([2, 0, 1])[np.arange(n) % 3]
        start = np.full(n, T0 + DAY, np.int64)
        start[150] = LIMIT - 10
        start[151] = LIMIT - DAY
        assert user[150] == 2 and user[151] == 0
        return make("repeat", "flip", user, 3, [{0, 2}, {0}, {0, 2}], start=start, queries=[(T0, W), (T0 - 20, W), (T0, W)])
    G = 3000              # shrink: 3 000 groups an hour old and group 0 twenty days old
    rng = np.random.default_rng(9)
    user = np.concatenate([1 + rng.permutation(G), [0], 1 + rng.permutation(G), [0]])
    start = np.where(user == 0, LIMIT - 20 * DAY, LIMIT - HOUR)
    every = set(range(G + 1))
    return make("repeat", "shrink", user, G + 1, [every, {0}, every, set(), {0}], start=start,
                queries=[(T0, W), (T0 - 10 * DAY, W), (T0, W), (T0 - 30 * DAY, W), (T0 - 10 * DAY, W)])


FAMILIES = ("placement", "threshold", "tombstones", "order", "bitmap_words", "sort_bits", "lds_limit", "group_sizes", "n_qual",
            "many_rows", "repeat")


def names():
    out = ["placement-%d-%s" % (n, p) for n in PLACEMENT_N for p in PLACEMENT_PATTERNS if placement_valid(n, p)]
    out += ["threshold", "tombstones-mixed", "tombstones-all", "order-desc", "order-interleave", "order-late"]
    out += ["bitmap_words-%d" % U for U in BITMAP_U] + ["sort_bits-%d" % U for U in SORT_U]
    out += ["lds_limit-%d" % U for U in (LDS_USERS, LDS_USERS + 1)] + ["group_sizes"]
    out += ["n_qual-%s" % G for G in N_QUAL] + ["many_rows", "repeat-flip", "repeat-shrink"]
    return out


def build(name, n_cus=256):
    family, _, arg = name.partition("-")
    if family == "placement":
        n, _, pattern = arg.partition("-")
        return placement(int(n), pattern)
    if family == "many_rows":
        return many_rows(n_cus)
    if family in ("threshold", "group_sizes"):
        return {"threshold": threshold, "group_sizes": group_sizes}[family]()
    if family in ("tombstones", "order", "repeat"):
        return {"tombstones": tombstones, "order": order, "repeat": repeat}[family](arg)
    if family == "n_qual":
        return n_qual(16 * n_cus + 1 if arg == "grid" else int(arg))
    return {"bitmap_words": bitmap_words, "sort_bits": sort_bits, "lds_limit": lds_limit}[family](int(arg))


def queue_groups(user, queue):
    """(order, sizes) read off a queue: its maximal runs of one group"""
    g = np.asarray(user)[np.asarray(queue, np.int64)]
    if g.size == 0:
        return [], []
    cut = np.concatenate([[0], np.nonzero(np.diff(g))[0] + 1, [g.size]])
    return [int(x) for x in g[cut[:-1]]], [int(x) for x in np.diff(cut)]


# ------------------------------------------------------------------------------------------------ sharded tables
COMM_WORLDS = (1, 2, 3, 5)
COMM_USERS = 10000
COMM_TOTALS = (0, 1, 3, 4, 5, 8193)   # around the merge's four groups per block, and past 2 048 blocks of them


def comm_names(world):
    out = ["total-%d" % G for G in COMM_TOTALS] + ["one_rank", "alternate", "sizes", "heavy"]
    return out + (["empty_rank", "idle_rank"] if world > 1 else [])


def lay(groups):
    """groups = [(id, rows, qualifies)] -> (user, old): the first rows in list order (the first-appearance order), then the other
    rows round by round; a qualifying group is old on its last row alone."""
    user = [g for g, _, _ in groups]
    for k in range(1, max(s for _, s, _ in groups)):
        user += [g for g, s, _ in groups if s > k]
    user = np.array(user, np.int32)
    return user, last_rows_of(user, [g for g, _, q in groups if q])


def build_comm(name, world, shard_of):
    """-> build()'s tuple for one sharded shape; props also holds `owner` (the rank of every user id) and, per rank, `rank_rows`,
    `rank_groups` and `rank_q` (rows held, qualifying groups, queued rows)."""
    owner = np.array([shard_of(g, world) for g in range(COMM_USERS)], np.int32)
    pool = [list(np.nonzero(owner == r)[0][::-1]) for r in range(world)]
    take = lambda r: int(pool[r].pop())
    shape, _, arg = name.partition("-")
    last = world - 1
    if shape == "total":
        G = int(arg)
        groups = [(take(r), 2, False) for r in range(world)] + [(take(k % world), 2 if G > 5 else 3, True) for k in range(G)]
    elif shape == "empty_rank":   # rank world - 1 holds no row
        groups = [(take(k % last), 3, k % 4 != 3) for k in range(8)]
    elif shape == "idle_rank":    # rank 0 holds rows and no qualifying group
        groups = [(take(0), 2, False) for _ in range(3)] + [(take(1 + k % last), 3, True) for k in range(7)]
    elif shape == "one_rank":     # every qualifying group on the last rank, young groups of every rank between them
        groups = []
        for k in range(9):
            groups += [(take(last), 2, True), (take(k % world), 2, False)]
    elif shape == "alternate":    # consecutive merged groups alternate ranks
        groups = [(take(k % world), 1 + k % 3, True) for k in range(64)]
    elif shape == "sizes":
        groups = [(take(k % world), s, True) for k, s in enumerate((63, 64, 65))] + [(take(r), 5, False) for r in range(world)]
    elif shape == "heavy":        # one group on rank 0 holds most rows, one-row groups everywhere else
        groups = [(take(0), 5000, True)]
        for k in range(20):
            groups += [(take(r), 1, True) for r in (range(1, world) if world > 1 else [0])]
    else:
        raise KeyError(name)
    user, old = lay(groups)
    qual = {g for g, _, q in groups if q}
    rank_rows = [int(np.count_nonzero(owner[user] == r)) for r in range(world)]
    rank_groups = [sum(1 for g, _, q in groups if q and owner[g] == r) for r in range(world)]
    rank_q = [sum(s for g, s, q in groups if q and owner[g] == r) for r in range(world)]
    return make("comm", name, user, COMM_USERS, [qual], old=old, owner=owner, world=world, rank_rows=rank_rows,
                rank_groups=rank_groups, rank_q=rank_q)
