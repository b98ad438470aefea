"""CPU: the reduction pie_set_end applies to a call that names rows more than once (pie_set_end_last_writers, host only: no
context, no GPU).  keep[i] = 1 iff element i is the last occurrence of its row, against a plain Python loop."""
import numpy as np
import pytest


def last_writers_loop(rows):
    keep, seen = [0] * len(rows), set()
    for i in range(len(rows) - 1, -1, -1):
        r = int(rows[i])
        if r not in seen:
            seen.add(r)
            keep[i] = 1
    return np.array(keep, np.uint8)


def cases():
    rng = np.random.default_rng(11)
    pool = rng.choice(3010, 40, replace=False)
    return {
        "empty": np.zeros(0, np.int32),
        "one element": np.array([7], np.int32),
        "no repeats, shuffled": rng.permutation(5000).astype(np.int32),
        "no repeats, ascending": np.arange(0, 9000, 3, dtype=np.int32),
        "all one row": np.full(1000, 5, np.int32),
        "rows descending": np.arange(4000, 0, -1, dtype=np.int32),
        "descending but for one repeat at the end": np.concatenate([np.arange(300, 0, -1), [1]]).astype(np.int32),
        "ascending but for one repeat in the middle": np.concatenate([np.arange(500), [250], np.arange(500, 900)]).astype(np.int32),
        "neighbouring pairs": np.repeat(np.arange(700, dtype=np.int32), 2),
        "16384 elements, 40 rows": rng.choice(pool, 16384).astype(np.int32),
        "16384 elements, half of them repeats": np.concatenate([rng.permutation(8192), rng.integers(0, 8192, 8192)]).astype(np.int32)[rng.permutation(16384)],
        "the ends of int32": np.array([2 ** 31 - 1, -2 ** 31, 0, -1, 2 ** 31 - 1, -1, -2 ** 31, 0, 0], np.int32),
    }


@pytest.mark.parametrize("name", list(cases()))
def test_last_writers_match_a_python_loop(pie, name):
    rows = cases()[name]
    keep = pie.set_end_last_writers(rows)
    want = last_writers_loop(rows)
    assert keep.dtype == np.uint8 and np.array_equal(keep, want), name
    assert int(keep.sum()) == np.unique(rows).size   # one element per distinct row is left


def test_argument_errors(pie):
    lib = pie.load_library()
    rows, keep = np.zeros(3, np.int32), np.zeros(3, np.uint8)
    assert lib.pie_set_end_last_writers(None, 3, keep.ctypes.data) != 0
    assert lib.pie_set_end_last_writers(rows.ctypes.data, 3, None) != 0
    assert lib.pie_set_end_last_writers(None, 0, None) == 0
