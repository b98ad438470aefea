"""pie_comm_delete_users in a fresh process on the one-GPU stand-in for RCCL (the set-up, the live table and its checks are those
of tests/comm_mutate_worker.py).  The model is the unsharded table: delete_user per id in array order.
usage: comm_delete_users_worker.py CASE
  worlds   worlds 1, 2, 3: one call with valid, repeated, unknown and just-appended ids; the merged ascending list, the counts and
           the owners equal the model's; columns, merged queues and gathered feeds afterwards equal the oracle's
  errors   a call refused while a pipelined step is uncollected, or by one shard, changes no shard"""
import sys

import numpy as np

from comm_mutate_worker import CASE, D, INT64_MIN, PIE_E_STATE, TOP, TTL, Live, PieError, pie


def delete_users(t, ids):
    ids = np.asarray(ids, np.int32)
    singles = []
    for x in ids.tolist():
        want = np.nonzero((t.u == x) & (t.e != INT64_MIN))[0] if 0 <= x < t.U else np.zeros(0, np.int64)
        t.e[want] = INT64_MIN
        singles.append(want)
    rows, per, owners = t.comm.delete_users(ids)
    union = np.sort(np.concatenate(singles + [np.zeros(0, np.int64)]))
    assert rows.dtype == np.int32 and np.array_equal(rows, union), (t.world, rows.size, union.size)
    assert np.array_equal(per, [w.size for w in singles]), (t.world, per)
    assert np.array_equal(owners, [pie.shard_of(x, t.world) if 0 <= x < t.U else -1 for x in ids.tolist()])
    return union.size


def case_worlds():
    checks = 0
    for world in (1, 2, 3):
        n, U = 20000, 300
        t = Live(world, n, U)
        t.append(65, 3)
        t.touch(257, 65)
        ids = [int(t.u[n // 3]), t.U - 1, t.U, -1, 7, int(t.u[n // 3]), 299, 2 ** 31 - 1, 7, 150, 151, 152]
        dead = 150
        t.comm.set_end(np.nonzero(t.u == dead)[0].astype(np.int32), np.full(int((t.u == dead).sum()), INT64_MIN, np.int64))
        t.e[t.u == dead] = INT64_MIN
        assert delete_users(t, ids) > 0
        assert delete_users(t, ids) == 0           # a second identical call finds nothing
        assert delete_users(t, []) == 0
        t.check_columns()
        checks += t.check_queues()
        checks += t.check_gather()
        t.comm.close()
    print("worlds ok: %d checks" % checks)


def case_errors():
    t = Live(3, 20000, 300)
    before = t.check_columns()
    ids = np.arange(0, 40, dtype=np.int32)

    def refused(fn):
        try:
            fn()
            raise AssertionError("the call went through")
        except PieError as e:
            assert e.code == PIE_E_STATE, e

    for r in range(3):
        t.comm.ctx(r).set_disciplines(0xFFFFFFFF, D)
    t.comm.step_reserve(1, 0, 1 << 16)
    t.comm.step_begin([(TOP - TTL // 3, TOP - 3 * TTL, 0x55555555)])
    refused(lambda: t.comm.delete_users(ids))
    t.comm.step_finish()
    refused(lambda: t.comm.delete_users(ids))
    t.comm.step_collect()
    after = t.check_columns()              # against the unchanged model
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(before, after))
    # one shard holds a row its map does not cover: every shard is asked first, so the whole call changes none
    c1 = t.comm.ctx(1)
    s = np.array([TOP], np.int64)
    c1.append_rows(s, s + TTL, np.array([0], np.int32), np.array([1], np.int32), c1.n_users)
    cols = [t.comm.ctx(r).read_columns() for r in (0, 2)]
    try:
        t.comm.delete_users(ids)
        raise AssertionError("the uncovered row went unnoticed")
    except PieError as e:
        assert e.code == PIE_E_STATE and "rank 1" in str(e), e
    for r, want in zip((0, 2), cols):
        assert all(np.array_equal(a, b) for a, b in zip(t.comm.ctx(r).read_columns(), want))
    t.comm.close()
    print("errors ok")


if __name__ == "__main__":
    {"worlds": case_worlds, "errors": case_errors}[CASE]()
    sys.stdout.flush()
