"""The wide pipelined exchange (pie_comm_wide_step_*) over shards of a SKEWED table, every shard's batches on the ordered run with
pie_set_wide_ordered on: a fresh process whose "RCCL" is tests/stub_rccl.c (PIE_RCCL_LIB), `world` shards on GPU 0.  Three
wide steps of 512, 300 and 65 queries: every rank reports Mu >= 0 from the first step on (there are no union slots to grow),
every global feed rebuilt from the gathered messages equals the oracle's scan of the unsharded table, and wide_step_read_feed
returns the head user's feed.
usage: comm_wide_ordered_worker.py WORLD N_ROWS N_USERS"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
stub_dir = os.path.join(REPO, "tests", "_stub")
os.makedirs(stub_dir, exist_ok=True)
stub = os.path.join(stub_dir, "libstub_rccl_wide_ord.%d.so" % os.getpid())
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                "-L/opt/rocm/lib", "-lamdhip64"], check=True, timeout=300)
os.environ["PIE_RCCL_LIB"] = stub

import numpy as np
import torch  # noqa: F401  (before libpie_hip.so initialises HIP)
import oracle_py
import sph_pie_amd as pie

T0, DAY, HOUR, SEED = 1700000000000, 86400 * 1000, 3600 * 1000, 0x5EED
ALL = 2 ** 64 - 1
MASKS = [0x5555555555555555, ALL, 0xAAAAAAAAAAAAAAAA, 0x00000000FFFF0000 | 3, 0x1]


def main():
    world, n, U = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    D = 16
    lim = (1 << D) - 1
    s, e, u, d = [c.copy() for c in oracle_py.gen(SEED + n, n, 0, n, U, D, 0)]
    head = 7 % U
    u = np.where(np.random.default_rng(SEED + n).random(n) < 0.4, head, u).astype(np.int32)
    cols = (s, e, u, d)
    comm = pie.PieComm([0] * world)
    maps = []
    for r in range(world):
        ctx = comm.ctx(r)
        ctx.load_columns(*cols, U)
        ctx.shard_table(r, world)
        ctx.set_disciplines(ALL, D)
        ctx.set_ordered_run(2)
        ctx.scan(T0 - 6 * HOUR, T0 - 61 * DAY)          # builds the shard's run: its batches now take it
        assert ctx.stats()["k1_variant"] & 0x2000
        ctx.set_wide_ordered(1)
        rows_g, users_g = ctx.shard_maps()
        maps.append((rows_g.astype(np.int64), users_g[: ctx.n_users].astype(np.int64)))
    assert sum(m[0].size for m in maps) == n
    all_q = [(T0 - 6 * HOUR - 977 * q - (q % 3) * HOUR, T0 - (61 + q % 4) * DAY - 13 * q, MASKS[q % 5]) for q in range(512)]
    all_want = [oracle_py.scan(*cols, U, now, cut, mask & lim) for now, cut, mask in all_q]
    sel = np.zeros(n, bool)
    for w in all_want:
        sel[w[2]] = True
    per_user = np.bincount(u[sel], minlength=U)
    union_rows = [int(per_user[maps[r][1]].sum()) for r in range(world)]
    assert per_user[head] > 64, "the head user's union is beyond any 64-slot bucket"
    comm.wide_step_reserve(512, 0, max(union_rows) + 16)
    checks = 0
    head_rank = [r for r in range(world) if head in maps[r][1]][0]
    head_local = int(np.flatnonzero(maps[head_rank][1] == head)[0])
    for step, nq in enumerate((512, 300, 65)):
        comm.wide_step_begin(all_q[:nq])
        ms = comm.wide_step_finish()
        assert [sum(ms[r][q] for r in range(world)) for q in range(nq)] == [int(w[2].size) for w in all_want[:nq]]
        assert comm.wide_step_collect() == step
        mu = comm.wide_step_status(step)
        assert mu.shape == (world,) and np.all(mu >= 0), (step, list(mu))
        words = (nq + 63) // 64
        for at in range(world):
            per_rank = []
            for r in range(world):
                uoff, rows, masks, mu_r = comm.wide_step_read_gathered(at, r, step)
                assert masks.shape == (rows.size, words) and mu_r == rows.size
                rows_r, users_r = maps[r]
                nu = users_r.size
                assert np.all(uoff[nu:] == mu_r)
                per_rank.append((rows_r[rows], np.repeat(users_r, np.diff(uoff[: nu + 1])), masks))
            for q in range(nq):
                wc, wo, wi = all_want[q]
                g_rows, g_users = [], []
                for rows_g, users_g, masks in per_rank:
                    bit = ((masks[:, q // 64] >> np.uint64(q % 64)) & np.uint64(1)).astype(bool)
                    g_rows.append(rows_g[bit])
                    g_users.append(users_g[bit])
                g_rows, g_users = np.concatenate(g_rows), np.concatenate(g_users)
                order = np.argsort(g_users, kind="stable")   # a user lives on one rank and its rows keep their order there
                assert np.array_equal(g_rows[order], wi), (step, at, q)
                assert np.array_equal(np.bincount(g_users, minlength=U), wc), (step, at, q)
                checks += 1
            for q in (0, 64 % nq, nq - 1):
                wc, wo, wi = all_want[q]
                got = comm.wide_step_read_feed(at, head_rank, step, q, head_local, idx_cap=n)
                assert np.array_equal(maps[head_rank][0][got], wi[wo[head]:wo[head + 1]]), (step, at, q)
                checks += 1
    comm.close()
    try:
        os.remove(stub)
    except OSError:
        pass
    print("comm wide ordered ok: world %d, %d checks" % (world, checks))


if __name__ == "__main__":
    main()
