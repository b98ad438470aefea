"""GPU: the shard form of the in-flight token lookup (pie_shard_token_lookup_begin / _finish) on `world` sharded contexts of one
GPU, each with a batch in flight, against tests/shard_token_model.py in GLOBAL ids with the per-key clock applied as
end > now[i].  Keys of other shards answer -1.  The batches are held against the oracle on the shard's own rows afterwards."""
import numpy as np
import pytest

from shard_token_model import ShardTokenModel
from table_model import same

pytestmark = pytest.mark.gpu

SEED, D = 20261, 8
MASK = (1 << D) - 1
SHAPES = {1: (4000, 40), 2: (4000, 40), 3: (4000, 40), 5: (4000, 7)}   # world 5, 7 users: a rank with no user and no row
PIE_E_STATE = -6


def random_keys(seed, n):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (n, 2), dtype=np.uint64)


@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_shard_lookup_with_a_batch_in_flight(pie, oracle, world):
    n0, u0 = SHAPES[world]
    cols = oracle.gen(SEED, n0, 0, n0, u0, D, 0)
    m = ShardTokenModel(*cols, [oracle.shard_of(u, world) for u in range(u0)], world)
    keys = random_keys(1, n0)
    m.token_set(keys)
    top = oracle.T0_MS + oracle.SPAN_MS
    rng = np.random.default_rng(2)
    qs = [(int(top - rng.integers(0, oracle.TTL_MS)), -(2 ** 63), MASK if q % 2 == 0 else int(rng.integers(1, MASK + 1))) for q in range(8)]
    ask = np.concatenate([keys[rng.integers(0, n0, 600)], random_keys(3, 100), keys[:5], keys[:5]])
    now = (top - rng.integers(0, 2 * oracle.TTL_MS, ask.shape[0])).astype(np.int64)
    now[-10:-5] = m.tm.end[:5]                # at the row's own end: not live
    now[-5:] = m.tm.end[:5] - 1               # one below: live
    ctxs = []
    try:
        for r in range(world):
            c = pie.PieScan(0)
            ctxs.append(c)
            c.set_batch_lanes(3)
            c.gen_synthetic(SEED, n0, 0, n0, u0, D, 0)
            c.shard_table(r, world)
            c.set_disciplines(MASK, D)
            c.shard_token_set(keys)
        held_by = np.zeros(ask.shape[0], int)
        for r, c in enumerate(ctxs):
            rows = m.held(r)
            if rows.size:                                # (a rank without rows has nothing to scan: its lookup runs alone)
                c.scan_batch_begin(qs)
                with pytest.raises(pie.PieError) as ei:  # the synchronous form keeps its rule
                    c.shard_token_lookup(ask, top)
                assert ei.value.code == PIE_E_STATE
            c.shard_token_lookup_begin(ask, now)
            c.shard_token_lookup_begin(ask[:3], int(now[0]))
            assert c.token_lookup_room() == 2
            got, want = c.shard_token_lookup_finish(), m.shard_lookup(r, ask, now)
            assert np.array_equal(got["row"], want["row"]), "rank %d: global row" % r
            assert np.array_equal(got["live"], want["live"]), "rank %d: live" % r
            f = want["found"]
            for col in ("user", "start", "end"):
                assert np.array_equal(got[col][f], want[col][f]), "rank %d: %s" % (r, col)
            assert np.all(got["row"][~f] == -1) and not got["live"][~f].any(), "keys of other shards answer -1"
            held_by += f
            if f[-5:].all():
                assert list(got["live"][-10:]) == [0] * 5 + [1] * 5
            short = c.shard_token_lookup_finish()
            assert np.array_equal(short["row"], want["row"][:3])
            with pytest.raises(pie.PieError) as ei:      # the plain finish of nothing
                c.token_lookup_finish()
            assert ei.value.code == PIE_E_STATE
            if rows.size:
                ms = list(c.scan_batch_finish())
                local_users = c.n_users
                users_map = c.shard_maps()[1]
                local_user = np.full(u0, -1, np.int32)
                local_user[users_map[:local_users]] = np.arange(local_users)
                tm = m.tm
                for qi, (q_now, q_cut, q_mask) in enumerate(qs):
                    w = oracle.scan(tm.start[rows], tm.end[rows], local_user[tm.user[rows]], tm.disc[rows], local_users, q_now, q_cut, q_mask)
                    assert ms[qi] == w[2].size
                    same(c.batch_read_results(qi), w, ("rank", r, "query", qi))
        assert np.all(held_by[:600] == 1) and np.all(held_by[600:700] == 0), "every present key is held by exactly one shard"
    finally:
        for c in ctxs:
            c.close()
