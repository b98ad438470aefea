"""CPU: pie_delete_users_plan (what pie_delete_users uploads: the membership bitmap of the valid ids and the first-occurrence
flags) against a numpy restatement, and the inputs of tests/test_gpu_delete_users.py against the numpy table model alone: no
seeded case may pass vacuously."""
import numpy as np
import pytest

import delete_users_cases as cases
from delete_users_cases import INT32_MAX, INT32_MIN, plan_model


def id_list(k, n_users, rng):
    edge = [-1, n_users, INT32_MIN, INT32_MAX, 0, 63, 64, n_users - 1]
    if k == 0:
        return np.zeros(0, np.int32)
    if k == 1:
        return np.array([edge[int(rng.integers(0, len(edge)))]], np.int32)
    body = rng.integers(-2, n_users + 2, k // 2 - len(edge)).tolist() + edge
    ids = np.array(body + body, np.int64)          # every id repeated
    return ids[rng.permutation(ids.size)].astype(np.int32)


@pytest.mark.parametrize("n_users", (1, 63, 64, 65, 4097))
@pytest.mark.parametrize("k", (0, 1, 1000))
def test_plan_matches_numpy(pie, k, n_users):
    rng = np.random.default_rng(k * 10007 + n_users)
    for _ in range(8 if k == 1 else 1):
        ids = id_list(k, n_users, rng)
        assert ids.size == k
        bits, first = pie.delete_users_plan(ids, n_users)
        want_bits, want_first = plan_model(ids, n_users)
        assert bits.dtype == np.uint64 and bits.size == (n_users + 63) // 64
        assert np.array_equal(bits, want_bits) and np.array_equal(first, want_first)
        if n_users % 64:   # nothing at or above n_users in the last word
            assert int(bits[-1]) >> (n_users % 64) == 0
        if k == 1000:
            assert first.sum() < k // 2 + 1 and first.sum() == np.unique(ids[(ids >= 0) & (ids < n_users)]).size


def test_plan_single_edges(pie):
    for n_users in (1, 63, 64, 65, 4097):
        for u in (-1, n_users, INT32_MIN, INT32_MAX, 0, 63, 64, n_users - 1):
            bits, first = pie.delete_users_plan([u, u], n_users)
            ok = 0 <= u < n_users
            assert first.tolist() == [1 if ok else 0, 0]
            assert sum(bin(int(w)).count("1") for w in bits) == (1 if ok else 0)
            if ok:
                assert (int(bits[u // 64]) >> (u % 64)) & 1


def test_plan_without_users(pie):
    bits, first = pie.delete_users_plan([1, 2], 0)
    assert bits.size == 0 and first.tolist() == [0, 0]


def test_gpu_cases_are_not_vacuous(oracle):
    seen = 0
    for case in cases.twin_cases(oracle) + cases.user_axis_cases(oracle):
        cases.check_case(oracle, case)
        seen += 1
    for case, kind in cases.row_axis_cases(oracle):
        cases.check_case(oracle, case, kind)
        seen += 1
    assert seen == 3 + len(cases.USER_AXIS_U) + 1 + len(cases.ROW_AXIS_N) + 4
