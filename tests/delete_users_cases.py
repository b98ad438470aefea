"""TEST INFRASTRUCTURE — the seeded inputs of the pie_delete_users tests and their numpy model.

Every case is (name, start, end, user, disc, U, D, ids).  The model is tests/table_model.TableModel: delete_user applied per id
in array order.  test_delete_users_cpu.py checks, on the model alone, that no case can pass vacuously (see check_case);
test_gpu_delete_users.py asserts the same before it uses a case."""
import numpy as np

from table_model import DAY, HOUR, INT64_MIN, TableModel, lattice_table, tie_table

INT32_MIN, INT32_MAX = -(2 ** 31), 2 ** 31 - 1
ROW_AXIS_N = (1, 3, 4, 5, 255, 256, 257, 1023, 1025, 65537, 300001)
USER_AXIS_U = (1, 63, 64, 65, 4097)
BIG_U, BIG_U_ROWS = 65537, 200003


def plan_model(users, n_users):
    """pie_delete_users_plan restated: (bits uint64[(n_users + 63) // 64], first uint8[k])."""
    users = np.asarray(users, np.int64).reshape(-1)
    bits = np.zeros((max(n_users, 0) + 63) // 64, np.uint64)
    first = np.zeros(users.size, np.uint8)
    seen = set()
    for i, u in enumerate(users.tolist()):
        if 0 <= u < n_users and u not in seen:
            seen.add(u)
            first[i] = 1
            bits[u // 64] |= np.uint64(1 << (u % 64))
    return bits, first


def model_of(oracle, case):
    _, s, e, u, d, U, D, _ = case
    m = TableModel(oracle)
    m.load(s, e, u, d, U, D)
    return m


def expected(m, ids):
    """K single deletes on the model, in array order -> (the single lists, their sorted union, the counts per element)."""
    singles = [m.delete_user(int(u)) for u in np.asarray(ids).tolist()]
    union = np.sort(np.concatenate(singles + [np.zeros(0, np.int32)])).astype(np.int32)
    return singles, union, np.array([x.size for x in singles], np.int32)


def check_case(oracle, case, kind="mixed"):
    """What keeps a case from passing vacuously.  mixed: the set deletes a row and holds a valid id with no live row, a repeated
    id and an invalid id (U = 1 cannot hold the first: its only valid id has to delete).  all: every live row goes.  none: no
    row goes."""
    name, s, e, u, d, U, D, ids = case
    ids = np.asarray(ids, np.int64)
    m = model_of(oracle, case)
    live_before = int(np.count_nonzero(m.end != INT64_MIN))
    _, union, per = expected(m, ids)
    valid = (ids >= 0) & (ids < U)
    _, first = plan_model(ids, U)
    if kind == "mixed":
        assert union.size > 0, (name, "deletes nothing")
        assert np.any(~valid), (name, "no invalid id")
        assert np.any(valid & (first == 0)), (name, "no repeated id")
        assert U == 1 or np.any((first == 1) & (per == 0)), (name, "no valid id without a live row")
    elif kind == "all":
        assert union.size == live_before > 0 and not np.any(m.end != INT64_MIN), name
    else:
        assert union.size == 0 and live_before > 0, name
    assert int(per.sum()) == union.size
    return union, per


# ------------------------------------------------------------------------------------------------ twin tables
def _pre_touched(end, user, dead, rng, top):
    """Some rows already tombstoned (all of user `dead`, and a few others), some touched (a later end)."""
    end = end.copy()
    end[user == dead] = INT64_MIN
    pick = rng.choice(end.size, min(60, end.size), replace=False)
    end[pick[::3]] = INT64_MIN
    end[pick[1::3]] = top + rng.integers(1, 5 * HOUR, pick[1::3].size)
    return end


def twin_cases(oracle):
    out = []
    s, e, u, d, U, D, _ = lattice_table(oracle)
    ids = [3, 20, -1, 7, 3, U, U - 1, 0, INT32_MAX, 7, INT32_MIN, 11, 52]
    out.append(("lattice", s, _pre_touched(e, u, 20, np.random.default_rng(11), int(e.max())), u, d, U, D, ids))
    s, e, u, d, U, D = tie_table(oracle)
    ids = [0, 9, 1, U + 5, 0, 46, -3, 30, 1]
    out.append(("tie", s, _pre_touched(e, u, 9, np.random.default_rng(12), int(e.max())), u, d, U, D, ids))
    n, U, D = 30011, 97, 32
    s, e, u, d = (a.copy() for a in oracle.gen(20271, n, 0, n, U, D, 0))
    ids = [96, 5, 40, -1, 5, 97, 0, 64, 63, 40, 1000]
    out.append(("seeded", s, _pre_touched(e, u, 40, np.random.default_rng(13), int(e.max())), u, d, U, D, ids))
    return out


# ------------------------------------------------------------------------------------------------ the row axis
def row_axis_table(oracle, n, U=7):
    """User 0 holds the first row, the last row and the rows on both sides of every multiple of 256 (every wave, block and load
    boundary of the passes is one); user 5's rows are tombstoned already; the rest is spread over all users."""
    rng = np.random.default_rng(1000 + n)
    user = rng.integers(0, U, n).astype(np.int32)
    r = np.arange(n)
    user[(r % 256 == 0) | (r % 256 == 255) | (r % 256 == 1) | (r == n - 1)] = 0
    start = (oracle.T0_MS - 30 * DAY + rng.integers(0, 20 * DAY, n)).astype(np.int64)
    end = (oracle.T0_MS + rng.integers(-3 * HOUR, 9 * HOUR, n)).astype(np.int64)
    end[user == 5] = INT64_MIN
    disc = rng.integers(0, 32, n).astype(np.int32)
    return start, end, user, disc, U, 32


def row_axis_cases(oracle):
    """-> [(case, kind)]"""
    out = []
    for n in ROW_AXIS_N:
        t = row_axis_table(oracle, n)
        out.append((("rows_%d" % n,) + t + ([0, 5, 3, 0, -1, 7, 3],), "mixed"))
    for n in (1025, 65537):
        t = row_axis_table(oracle, n)
        out.append((("rows_%d_all" % n,) + t + ([6, 5, 4, 3, 2, 1, 0],), "all"))
        out.append((("rows_%d_none" % n,) + t + ([-1, 7, INT32_MAX],), "none"))
    return out


# ------------------------------------------------------------------------------------------------ the user axis
def user_axis_table(oracle, U, n):
    rng = np.random.default_rng(2000 + U)
    user = rng.integers(0, U, n).astype(np.int32)
    user[:min(U, n)] = np.arange(min(U, n))   # every user has a row
    start = (oracle.T0_MS - 30 * DAY + rng.integers(0, 20 * DAY, n)).astype(np.int64)
    end = (oracle.T0_MS + rng.integers(-3 * HOUR, 9 * HOUR, n)).astype(np.int64)
    if U > 17:
        end[user == 17] = INT64_MIN
    disc = rng.integers(0, 32, n).astype(np.int32)
    return start, end, user, disc, U, 32


def user_axis_cases(oracle):
    out = []
    for U in USER_AXIS_U + (BIG_U,):
        n = BIG_U_ROWS if U == BIG_U else 4 * U + 777
        ids = [0, 31, 32, 63, 64, U - 1, 17, 0, -1, U, 65535, 65536]
        out.append(("users_%d" % U,) + user_axis_table(oracle, U, n) + (ids,))
    return out
