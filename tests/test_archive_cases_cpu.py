"""No GPU: the designed archive tables (archive_cases.py) plant what they claim.  For every case the C oracle's queue has the
declared groups in the declared order with the declared sizes, the table sits on the boundary it is named after, and the numpy
twin agrees with the C oracle wherever its INT64_MAX sentinel leaves it unambiguous.  A table that is not what it says fails here."""
import functools

import numpy as np
import pytest

import archive_cases as AC

N_CUS = 256


@functools.lru_cache(maxsize=None)
def case(name):
    return AC.build(name, N_CUS)


def check_declared(oracle, built, twin=True):
    start, end, user, disc, U, queries, props = built
    assert start.dtype == end.dtype == np.int64 and user.dtype == disc.dtype == np.int32
    assert start.size == end.size == user.size == disc.size and 0 <= user.min() and user.max() < U
    queues = []
    for k, (now, window) in enumerate(queries):
        got = oracle.archive_queue(start, end, user, U, now, window)
        assert AC.queue_groups(user, got) == (props["order"][k], props["sizes"][k]), (k, "groups, their order, their sizes")
        assert got.size == props["q"][k] == sum(props["sizes"][k]) and len(props["order"][k]) == props["n_qual"][k], k
        assert not np.any(end[got] == AC.INT64_MIN), (k, "a tombstone is queued")
        if twin:
            same = np.array_equal(oracle.archive_queue_numpy(start, end, user, U, now, window), got)
            assert same == props["numpy_ok"][k], (k, "the numpy twin", same)
        queues.append(got)
    return queues


@pytest.mark.parametrize("name", AC.names())
def test_case_is_what_it_declares(oracle, name):
    built = case(name)
    start, end, user, disc, U, queries, props = built
    queues = check_declared(oracle, built)
    family, boundary, n = props["family"], props["boundary"], start.size
    assert family in AC.FAMILIES and name.startswith(family)
    if family == "placement":
        h = props["hits"]
        assert np.array_equal(start <= AC.LIMIT, h) and not np.any(end == AC.INT64_MIN)
        assert np.array_equal(np.sort(queues[0]), np.nonzero(user == 0)[0] if h.any() else [])
        if boundary == "tail_decides":
            mine = np.nonzero(user == 0)[0]
            assert n % 2 == 1 and mine[-1] == n - 1 and mine.size == 3 and np.array_equal(np.nonzero(h)[0], [n - 1])
        else:
            assert np.array_equal(user == 0, h), "group 0 owns exactly the pattern"
        if boundary.startswith("pair"):
            r = np.nonzero(h)[0]
            assert r.size == (2 if boundary == "pair_both" else 1) and r[0] % 2 == (1 if boundary == "pair_odd" else 0) and (r[0] | 1) < n
        if boundary == "last_row":
            assert h[n - 1] and h.sum() == 1
        if boundary == "last_of_every_step":
            assert h.sum() == n // AC.STEP and np.all(np.nonzero(h)[0] % AC.STEP == AC.STEP - 1)
        if boundary == "first_of_every_block_but_the_first":
            assert h.sum() == (n - 1) // AC.BLOCK and np.all(np.nonzero(h)[0] % AC.BLOCK == 0) and not h[0]
    elif family == "threshold":
        d = props["deciding"]
        assert d[0] == AC.T0 - AC.W and d[1] == d[0] + 1 and d[2] == AC.INT64_MIN and d[3] == AC.INT64_MAX
        assert (AC.T0, AC.W) in queries and (AC.T0, 0) in queries
        assert any(now - w < AC.INT64_MIN for now, w in queries) and any(now - w > AC.INT64_MAX for now, w in queries)
        assert np.count_nonzero((user == 3) & (end != AC.INT64_MIN)) == 1 and start[(user == 3) & (end != AC.INT64_MIN)][0] == AC.INT64_MAX
        assert props["numpy_ok"].count(False) == 2
        assert props["order"][0] == [2, 0] and 1 in props["order"][1]
    elif name == "tombstones-mixed":
        old = start <= AC.LIMIT
        dead = end == AC.INT64_MIN
        assert np.all(dead[(user == 0) & old]) and np.any((user == 0) & ~dead), "group 0: its only old row is a tombstone"
        assert dead[0] and user[0] == 1 and props["order"][0] == [2, 1], "group 1's first row is a tombstone: it comes second"
        assert np.all(dead[user == 3]) and np.any(old[user == 3])
    elif name == "tombstones-all":
        assert np.all(end == AC.INT64_MIN) and props["q"] == [0]
    elif name == "order-desc":
        assert props["order"][0] == list(range(39, -1, -1))
    elif name == "order-interleave":
        assert np.array_equal(user[queues[0]][:2], [3, 3]) and np.all(user[:-1] != user[1:]) and props["order"][0] == [3, 1]
    elif name == "order-late":
        assert user[0] == 2 and start[0] > AC.LIMIT and props["order"][0] == [2, 1]
        assert np.count_nonzero((user == 2) & (start <= AC.LIMIT)) == 1
    elif family == "bitmap_words":
        for g in props["order"][0]:
            for nb in (g - 1, g + 1):
                assert nb < 0 or nb >= U or nb in props["order"][0] or np.any(user == nb), (g, "a neighbour without rows")
        assert set(props["order"][0]) == {g for g in (0, 31, 32, 63, U - 1) if g < U}
        assert U < 3 or props["n_qual"][0] < U, "no unqualified neighbour at all"
    elif family == "sort_bits":
        assert props["order"][0] == [U - 1, 0] and {1, U - 2} <= set(user.tolist())
    elif family == "lds_limit":
        assert (props["bitmap_bytes"] == 48 * 1024) == (U == AC.LDS_USERS) and props["bitmap_bytes"] >= 48 * 1024
        assert set(props["order"][0]) == {0, AC.LDS_USERS - 1} | ({AC.LDS_USERS} if U > AC.LDS_USERS else set())
        assert {1, AC.LDS_USERS - 2} <= set(user.tolist()) and 4990 < n < 5010
    elif family == "group_sizes":
        assert sorted(props["sizes"][0]) == sorted(AC.GROUP_SIZES)
        assert all(start[np.nonzero(user == g)[0][0]] > AC.LIMIT for g in props["order"][0] if np.count_nonzero(user == g) > 1)
    elif family == "n_qual":
        assert props["n_qual"][0] == {"grid": 16 * N_CUS + 1}.get(name.split("-")[1]) or props["n_qual"][0] == int(name.split("-")[1])
        assert set(props["sizes"][0]) == {2}
        assert props["order"][0] != sorted(props["order"][0])
    elif family == "many_rows":
        assert props["q"][0] == 16 * N_CUS * 256 + 1 and props["n_qual"][0] == 2
    elif name == "repeat-flip":
        assert [sorted(o) for o in props["order"]] == [[0, 2], [0], [0, 2]]
    elif name == "repeat-shrink":
        assert props["n_qual"] == [3001, 1, 3001, 0, 1] and props["q"] == [6002, 2, 6002, 0, 2]


def test_every_family_and_value_of_the_issue_is_listed():
    names = AC.names()
    assert len(names) == len(set(names))
    assert {n.split("-")[0] for n in names} == set(AC.FAMILIES)
    for n in AC.PLACEMENT_N:
        assert "placement-%d-all" % n in names and ("placement-%d-tail_decides" % n in names) == (n % 2 == 1 and n > 1)
    assert {"n_qual-%s" % g for g in (255, 256, 257, "grid", 8193)} <= set(names)


@pytest.mark.parametrize("world", AC.COMM_WORLDS)
def test_sharded_shapes(oracle, world):
    for name in AC.comm_names(world):
        built = AC.build_comm(name, world, oracle.shard_of)
        start, end, user, disc, U, queries, props = built
        check_declared(oracle, built, twin=name != "total-8193")
        owner = props["owner"]
        assert np.array_equal(owner[:50], [oracle.shard_of(g, world) for g in range(50)])
        for r in range(world):
            mine = owner[user] == r
            assert np.count_nonzero(mine) == props["rank_rows"][r], (name, r)
            got = oracle.archive_queue(start[mine], end[mine], user[mine], U, *queries[0])
            assert got.size == props["rank_q"][r] and len(AC.queue_groups(user[mine], got)[0]) == props["rank_groups"][r], (name, r)
        ranks = [int(owner[g]) for g in props["order"][0]]
        if name.startswith("total"):
            assert props["n_qual"][0] == int(name.split("-")[1]) and ranks == [k % world for k in range(len(ranks))]
        elif name == "empty_rank":
            assert props["rank_rows"][world - 1] == 0 and min(props["rank_rows"][:-1]) > 0
        elif name == "idle_rank":
            assert props["rank_rows"][0] > 0 and props["rank_groups"][0] == 0
        elif name == "one_rank":
            assert set(ranks) == {world - 1} and min(props["rank_rows"]) > 0
        elif name == "alternate":
            assert ranks == [k % world for k in range(64)]
        elif name == "sizes":
            assert props["sizes"][0] == [63, 64, 65]
        elif name == "heavy":
            assert props["sizes"][0][0] == 5000 and set(props["sizes"][0][1:]) == {1} and props["rank_q"][0] >= 5000
