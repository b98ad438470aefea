"""CPU: pie_shard_route, the routing pie_shard_append_rows applies on the host, against the oracle's shard rule and numpy.
No GPU, no context."""
import numpy as np
import pytest

WORLDS = (1, 2, 3, 5, 8)


def expect(oracle, users, rank, world, before, after):
    keep = np.array([1 if oracle.shard_of(int(u), world) == rank else 0 for u in users], np.uint8)
    new = np.array([u for u in range(before, after) if oracle.shard_of(u, world) == rank], np.int32)
    return keep, new


@pytest.mark.parametrize("world", WORLDS)
def test_route_matches_oracle(pie, oracle, world):
    rng = np.random.default_rng(100 + world)
    users = rng.integers(0, 500, 777).astype(np.int32)
    total_kept = 0
    seen = []
    for rank in range(world):
        keep, new = pie.shard_route(users, rank, world, 300, 500)
        want_keep, want_new = expect(oracle, users, rank, world, 300, 500)
        assert np.array_equal(keep, want_keep)
        assert np.array_equal(new, want_new) and np.all(np.diff(new) > 0)
        total_kept += int(keep.sum())
        seen.append(new)
    # every row and every new user belongs to exactly one rank
    assert total_kept == users.size
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(300, 500, dtype=np.int32))


@pytest.mark.parametrize("world", WORLDS)
def test_no_rows_and_no_new_users(pie, oracle, world):
    for rank in range(world):
        keep, new = pie.shard_route(np.empty(0, np.int32), rank, world, 40, 40)  # k = 0, users_before == users_after
        assert keep.size == 0 and new.size == 0
        keep, new = pie.shard_route(np.arange(10, dtype=np.int32), rank, world, 40, 40)
        assert new.size == 0 and np.array_equal(keep, expect(oracle, range(10), rank, world, 0, 0)[0])
        keep, new = pie.shard_route(np.empty(0, np.int32), rank, world, 50, 40)  # an empty range, not an error
        assert new.size == 0


@pytest.mark.parametrize("world", (2, 3, 5, 8))
def test_all_users_on_one_rank(pie, oracle, world):
    mine = [u for u in range(4000) if oracle.shard_of(u, world) == world - 1][:200]
    users = np.array(mine, np.int32)
    for rank in range(world):
        keep, _ = pie.shard_route(users, rank, world)
        assert int(keep.sum()) == (users.size if rank == world - 1 else 0)


@pytest.mark.parametrize("world", WORLDS)
def test_small_cap_reports_the_number(pie, oracle, world):
    _, want = expect(oracle, [], 0, world, 0, 64)
    assert want.size >= 2
    with pytest.raises(pie.PieError) as ei:
        pie.shard_route(np.empty(0, np.int32), 0, world, 0, 64, cap=want.size - 1)
    assert ei.value.code == -5 and ei.value.n_new == want.size
    _, new = pie.shard_route(np.empty(0, np.int32), 0, world, 0, 64, cap=want.size)
    assert np.array_equal(new, want)


@pytest.mark.parametrize("world", WORLDS)
def test_routing_is_not_validation(pie, oracle, world):
    users = np.array([-1, -7, 2 ** 31 - 1, 10 ** 9, 5, 99], np.int32)  # ids outside [0, users_after) are still routed by hash
    for rank in range(world):
        keep, _ = pie.shard_route(users, rank, world, 0, 6)
        assert np.array_equal(keep, expect(oracle, users, rank, world, 0, 0)[0])


def test_bad_arguments(pie):
    for rank, world in ((0, 0), (-1, 2), (2, 2)):
        with pytest.raises(pie.PieError) as ei:
            pie.shard_route(np.zeros(3, np.int32), rank, world)
        assert ei.value.code == -1
