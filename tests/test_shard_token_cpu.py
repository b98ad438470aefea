"""CPU: the model of the sharded token column against itself (tests/shard_token_model.py).  While no compaction has dropped
rows, merging the shards' answers by largest global row is TokenModel.lookup of the unsharded table — the rule
pie_comm_token_lookup applies on the host.  No GPU, no context."""
import numpy as np
import pytest

from shard_token_model import ShardTokenModel
from token_model import END_NONE

NOW = 1700000000000
N, U = 4000, 60


def table(pie, world, seed):
    rng = np.random.default_rng(seed)
    start = (NOW - rng.integers(1, 10 ** 9, N)).astype(np.int64)
    end = (NOW + rng.integers(-5 * 10 ** 8, 5 * 10 ** 8, N)).astype(np.int64)
    end[rng.integers(0, N, 40)] = END_NONE
    user = rng.integers(0, U, N).astype(np.int32)
    owner = [pie.shard_of(u, world) for u in range(U)]
    keys = rng.integers(0, 2 ** 64, (N, 2), dtype=np.uint64)
    pool = keys[rng.integers(0, N, 30)]                    # planted duplicates: whichever users (and shards) they fall on
    keys[rng.integers(0, N, 300)] = pool[rng.integers(0, 30, 300)]
    return ShardTokenModel(start, end, user, np.zeros(N, np.int32), owner, world), keys, rng


@pytest.mark.parametrize("world", (1, 2, 3, 5))
def test_merge_is_the_unsharded_lookup(pie, world):
    m, keys, rng = table(pie, world, 100 + world)
    ask = np.concatenate([keys, rng.integers(0, 2 ** 64, (200, 2), dtype=np.uint64)])
    for covered in (0, 1, N - 137, N):
        m.token_set(keys[:covered])
        assert sum(m.covered_l(r) for r in range(world)) == covered
        for now in (NOW, END_NONE):
            got, want = m.merged_lookup(ask, now), m.tm.lookup(ask, now)
            assert np.array_equal(got["row"], want["row"]) and np.array_equal(got["live"], want["live"])
            f = want["found"]
            assert np.array_equal(got["found"], f)
            for col in ("user", "start", "end"):
                assert np.array_equal(got[col][f], want[col][f]), col
            assert np.array_equal(got["owner"][f], m.owner[want["user"][f]]) and np.all(got["owner"][~f] == -1)
    dup = m.tm.lookup(keys, NOW)["row"] != np.arange(N)
    assert dup.sum() >= 100, "the planted duplicates answer with a later row"


def test_a_shard_answers_only_for_itself(pie):
    world = 3
    m, keys, _ = table(pie, world, 7)
    m.token_set(keys)
    for r in range(world):
        got = m.shard_lookup(r, keys, NOW)
        f = got["found"]
        assert np.all(m.owner[got["user"][f]] == r)
        mine = m.owner[m.tm.user] == r
        assert np.all(f[mine]) and np.all(got["row"][mine] >= np.arange(N)[mine]), "the key of an own row finds it, or a later own row"


def test_set_end_and_compaction(pie):
    world = 2
    m, keys, rng = table(pie, world, 9)
    m.token_set(keys)
    plain = ShardTokenModel(m.tm.start, m.tm.end, m.tm.user, m.tm.disc, m.owner, world)
    plain.token_set(keys)
    ask = keys[rng.integers(0, N, 500)]
    new_end = (NOW + rng.integers(1, 10 ** 8, 500)).astype(np.int64)
    holders = sum(m.shard_lookup(r, ask, NOW)["found"].astype(int) for r in range(world))
    outs = m.shard_set_end(ask, new_end, NOW)
    # keys held by one shard only: the shards' touches together are the unsharded touch
    single = holders <= 1
    assert 0 < np.count_nonzero(~single) < 250
    want = plain.tm.token_set_end(ask[single], new_end[single], NOW)
    got = np.max(np.stack(outs), axis=0)[single]
    assert np.array_equal(got, want)
    # a compaction on rank 0 drops its dead rows only; their keys are gone from rank 0 and nothing changes on rank 1
    before = [m.shard_lookup(r, keys, NOW)["row"] for r in range(world)]
    held = m.compact(0, NOW)
    assert np.all(m.tm.end[held] > NOW)
    after = [m.shard_lookup(r, keys, NOW)["row"] for r in range(world)]
    assert np.array_equal(before[1], after[1])
    assert np.all(np.isin(after[0][after[0] >= 0], held)) and np.count_nonzero(after[0] >= 0) < np.count_nonzero(before[0] >= 0)
    assert m.covered_l(0) == held.size and m.covered_g == N
