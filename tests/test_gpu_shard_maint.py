"""GPU: pie_shard_prune_before / pie_shard_retention_purge / _tz on their own.  For worlds 2 and 5 every shard's list ascends, holds
global rows, and the union of the shards' lists is the unsharded call's list; afterwards every shard's columns are the unsharded
table's rows its map names."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SEED, D, N, U = 0x5EED5EED, 32, 20003, 97
INT64_MIN = -(2 ** 63)
PIE_E_STATE, PIE_E_CAPACITY = -6, -5


@pytest.fixture(scope="module")
def columns(oracle):
    s, e, u, d = (a.copy() for a in oracle.gen(SEED, N, 0, N, U, D, 0))
    e[5::11] = INT64_MIN
    return s, e, u, d


def shards(pie, cols, world):
    out = []
    for r in range(world):
        c = pie.PieScan(0)
        c.load_columns(*cols, U)
        c.shard_table(r, world)
        out.append(c)
    return out


@pytest.mark.parametrize("world", [2, 5])
def test_union_of_the_shard_lists_is_the_unsharded_list(pie, oracle, columns, world):
    zones = json.load(open(os.path.join(GOLDEN, "addmonths_zones.json")))["zones"]
    assert "Europe/Berlin" in zones
    tz = oracle.tz_table("Europe/Berlin")
    s = np.sort(columns[0])
    t0, span = oracle.T0_MS, oracle.SPAN_MS
    plain = pie.PieScan(0)
    plain.load_columns(*columns, U)
    cs = shards(pie, columns, world)
    try:
        calls = [
            (lambda c: c.prune_before(int(s[N // 8])), lambda c: c.shard_prune_before(int(s[N // 8]))),
            (lambda c: c.retention_purge(t0 - span // 2 + 62 * 86400000, 2, 330 * 60000),
             lambda c: c.shard_retention_purge(t0 - span // 2 + 62 * 86400000, 2, 330 * 60000)),
            (lambda c: c.retention_purge(t0 - span // 2 + 80 * 86400000, 2, tz_table=tz),
             lambda c: c.shard_retention_purge(t0 - span // 2 + 80 * 86400000, 2, tz_table=tz)),
        ]
        for whole, part in calls:
            want = whole(plain)
            assert want.size > 256
            lists = [part(c) for c in cs]
            for got in lists:
                assert got.dtype == np.int32 and np.all(np.diff(got) > 0)
            assert np.array_equal(np.sort(np.concatenate(lists)), want)
            assert all(part(c).size == 0 for c in cs)   # a second identical call finds nothing
        ts, te, _, td = plain.read_columns()
        for c in cs:
            g = c.shard_maps()[0]
            ls, le, _, ld = c.read_columns()
            assert np.array_equal(ls, ts[g]) and np.array_equal(le, te[g]) and np.array_equal(ld, td[g])
    finally:
        plain.close()
        for c in cs:
            c.close()


def test_capacity_and_state(pie, oracle, columns):
    cutoff = int(np.sort(columns[0])[N // 2])
    plain = pie.PieScan(0)
    plain.load_columns(*columns, U)
    cs = shards(pie, columns, 2)
    c = cs[0]
    try:
        for fn in (lambda: plain.shard_prune_before(cutoff), lambda: plain.shard_retention_purge(cutoff, 2)):
            with pytest.raises(pie.PieError) as ei:   # not a shard
                fn()
            assert ei.value.code == PIE_E_STATE
        assert np.array_equal(plain.read_columns()[1], columns[1])
        owner = np.array([oracle.shard_of(g, 2) for g in range(U)])
        want = np.nonzero((owner[columns[2]] == 0) & (columns[0] < cutoff) & (columns[1] != INT64_MIN))[0]
        with pytest.raises(pie.PieError) as ei:
            c.shard_prune_before(cutoff, cap=want.size - 1)
        assert ei.value.code == PIE_E_CAPACITY
        g = c.shard_maps()[0]
        e = c.read_columns()[1]
        assert np.array_equal(g[(e == INT64_MIN) & (columns[1][g] != INT64_MIN)], want)   # tombstoned all the same
        # a plain append leaves rows without a global row: the shard forms refuse
        one = np.array([cutoff], np.int64)
        c.append_rows(one, one + 1, np.array([0], np.int32), np.array([0], np.int32), c.n_users)
        with pytest.raises(pie.PieError) as ei:
            c.shard_prune_before(cutoff + 2)
        assert ei.value.code == PIE_E_STATE
    finally:
        plain.close()
        for x in cs:
            x.close()
