"""The cross-shard archive queue (pie_comm_archive_queue) on the designed sharded shapes of archive_cases.py, in a fresh process
whose "RCCL" is tests/stub_rccl.c (PIE_RCCL_LIB): WORLD shards of one table on GPU 0.  test_archive_cases_cpu.py shows what each
shape plants (which rank holds which groups).  Every shape checks the merged rows against the oracle's queue of the UNSHARDED
columns, the source rank and source row of every element, the copy every local rank holds, the capacity error with its total and
the repeat with room.
usage: comm_archive_worker.py WORLD"""
import ctypes as C
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
stub_dir = os.path.join(REPO, "tests", "_stub")
os.makedirs(stub_dir, exist_ok=True)
stub = os.path.join(stub_dir, "libstub_rccl.so")
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                "-L/opt/rocm/lib", "-lamdhip64"], check=True)
os.environ["PIE_RCCL_LIB"] = stub

import numpy as np
import torch  # noqa: F401  (before libpie_hip.so initialises HIP)
import oracle_py
import sph_pie_amd as pie
from sph_pie_amd.binding import _ptr

import archive_cases as AC

PIE_E_CAPACITY = -5


def raw_queue(comm, now, window, cap):
    out = np.full(max(cap, 1), -7, np.int32)
    q = C.c_size_t(12345)
    rc = comm._lib.pie_comm_archive_queue(comm._c, int(now), int(window), _ptr(out), int(cap), C.byref(q))
    return rc, q.value, out[:cap]


def shape(world, name):
    start, end, user, disc, U, queries, props = AC.build_comm(name, world, oracle_py.shard_of)
    now, window = queries[0]
    owner = props["owner"]
    want = oracle_py.archive_queue(start, end, user, U, now, window)
    local = np.zeros(user.size, np.int64)   # a global row's place among the rows of its shard
    for r in range(world):
        held = np.nonzero(owner[user] == r)[0]
        local[held] = np.arange(held.size)
    comm = pie.PieComm([0] * world)
    try:
        for r in range(world):
            comm.ctx(r).load_columns(start, end, user, disc, U)
            assert comm.ctx(r).shard_table(r, world)[0] == props["rank_rows"][r], (name, r, "rows held")
        rows, src_rank, src_row = comm.archive_queue(now, window, sources=True)
        assert rows.dtype == np.int32 and np.array_equal(rows, want), (name, "merged rows", rows.size, want.size)
        assert np.array_equal(src_rank, owner[user[want]]), (name, "source ranks")
        assert np.array_equal(src_row, local[want]), (name, "source rows")
        for at in range(world):
            assert np.array_equal(comm.queue_read(at), want), (name, "the copy of rank", at)
        if want.size:
            rc, q, out = raw_queue(comm, now, window, want.size - 1)
            assert rc == PIE_E_CAPACITY and q == want.size and np.all(out == -7), (name, "capacity", rc, q)
        rc, q, out = raw_queue(comm, now, window, want.size)
        assert rc == 0 and q == want.size and np.array_equal(out, want), (name, "the repeat with room", rc, q)
    finally:
        comm.close()


if __name__ == "__main__":
    world = int(sys.argv[1])
    names = AC.comm_names(world)
    for name in names:
        shape(world, name)
    print("world %d ok: %d shapes" % (world, len(names)))
