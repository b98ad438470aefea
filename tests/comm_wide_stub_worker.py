"""The WIDE pipelined exchange of the C-ABI communicator (pie_comm_wide_step_*) with world > 1 on a one-GPU box: a fresh process
whose "RCCL" is tests/stub_rccl.c (PIE_RCCL_LIB), `world` shards of one corpus on GPU 0.  Against the oracle's scan of the
unsharded table:
  - the first steps under a 16-row reservation: PIE_E_CAPACITY at collect on every rank, and wide_step_status shows for every
    rank either its union's size or Mu = -1 (a shard whose first wide batches outgrow the 16, then 32 union slots per user) —
    which of the two is computed from the oracle's answers beforehand; then needed_cap, re-reserve, repeat;
  - 9 pipelined steps of 512 queries, 6 of 300, 4 of 65 (two steps begun ahead, the buffer sets rotate): for the last three
    steps of each run every global user's feed of every query, rebuilt from the gathered messages at every rank;
  - wide_step_read_feed for sampled (query, user); the mutual exclusion with the ordinary steps; the ordinary steps afterwards;
  - a shard that cannot begin: the wide step is refused and not counted, nothing is left in any shard, the next steps are exact.
usage: comm_wide_stub_worker.py WORLD N_ROWS N_USERS [no-union]   (no-union: this table's first steps must report Mu = -1)"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
stub_dir = os.path.join(REPO, "tests", "_stub")
os.makedirs(stub_dir, exist_ok=True)
stub = os.path.join(stub_dir, "libstub_rccl_wide.%d.so" % os.getpid())
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                "-L/opt/rocm/lib", "-lamdhip64"], check=True, timeout=300)
os.environ["PIE_RCCL_LIB"] = stub

import numpy as np
import torch  # noqa: F401  (before libpie_hip.so initialises HIP)
import oracle_py
import sph_pie_amd as pie

T0, DAY, HOUR, SEED = 1700000000000, 86400 * 1000, 3600 * 1000, 0x5EED5EED
E_CAPACITY, E_STATE = pie.binding.PIE_E_CAPACITY, -6


def expect(code, fn, *a):
    try:
        fn(*a)
    except pie.PieError as ex:
        assert ex.code == code, ex
        return
    raise AssertionError("%s did not fail with %d" % (getattr(fn, "__name__", fn), code))


def main():
    world, n, U = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    D = 32
    comm = pie.PieComm([0] * world)
    comm.gen_synthetic_sharded(SEED, n, U, D, 0)
    ctxs = [comm.ctx(r) for r in range(world)]
    maps = []
    for r in range(world):
        ctxs[r].set_disciplines(0xFFFFFFFF, D)
        rows_g, users_g = ctxs[r].shard_maps()
        maps.append((rows_g.astype(np.int64), users_g[: ctxs[r].n_users].astype(np.int64)))
    assert sum(m[0].size for m in maps) == n
    cols = oracle_py.gen(SEED, n, 0, n, U, D, 0)
    masks6 = [0x55555555, 0xAAAAAAAA, 0xFFFFFFFF, 0xFFFF0000, 0x1, 0x80000001]

    def queries_of(k):  # heterogeneous: distinct now / cutoff / mask
        return [(T0 - 6 * HOUR - 977 * q - (q % 3) * HOUR, T0 - (61 + q % 4) * DAY - 13 * q, masks6[q % 6]) for q in range(k)]

    all_q = queries_of(512)
    all_want = [oracle_py.scan(*cols, U, *q) for q in all_q]
    checks = 0
    rng = np.random.default_rng(world)

    def check_step(step, nq):
        """every global user's feed of every query from the gathered messages, at every rank"""
        nonlocal checks
        words = (nq + 63) // 64
        for at in range(world):
            got = [comm.wide_step_read_gathered(at, r, step) for r in range(world)]
            per_rank = []
            for r in range(world):
                uoff, rows, masks, mu = got[r]
                assert masks.shape == (rows.size, words) and mu == rows.size
                rows_r, users_r = maps[r]
                nu = users_r.size
                assert np.all(uoff[nu:] == mu)
                row_user_g = np.repeat(users_r, np.diff(uoff[: nu + 1]))      # global user of every union row
                per_rank.append((rows_r[rows], row_user_g, masks))
            for q in range(nq):
                wc, wo, wi = all_want[q]
                g_rows, g_users = [], []
                for rows_g, users_g, masks in per_rank:
                    bit = ((masks[:, q // 64] >> np.uint64(q % 64)) & np.uint64(1)).astype(bool)
                    g_rows.append(rows_g[bit])
                    g_users.append(users_g[bit])
                g_rows, g_users = np.concatenate(g_rows), np.concatenate(g_users)
                # a user lives on one rank and its rows keep their order there: a stable sort by user rebuilds the global lists
                order = np.argsort(g_users, kind="stable")
                assert np.array_equal(g_rows[order], wi), (step, at, q)
                assert np.array_equal(np.bincount(g_users, minlength=U), wc), (step, at, q)
                checks += 1

    def check_feeds(step, nq):
        nonlocal checks
        for _ in range(12):
            q, r = int(rng.integers(0, nq)), int(rng.integers(0, world))
            rows_r, users_r = maps[r]
            lu = int(rng.integers(0, users_r.size))
            gu = int(users_r[lu])
            wc, wo, wi = all_want[q]
            at = int(rng.integers(0, world))
            assert np.array_equal(rows_r[comm.wide_step_read_feed(at, r, step, q, lu)], wi[wo[gu]:wo[gu + 1]]), (step, q, r, lu)
            checks += 1

    def run_pipelined(nq, k, first_step):
        """begin(i+1) | finish(i) | collect(i-1): two steps begun ahead of the exchange"""
        qs_ = all_q[:nq]
        want_m = [int(w[2].size) for w in all_want[:nq]]
        comm.wide_step_begin(qs_)
        collected = []
        for i in range(k):
            if i + 1 < k:
                comm.wide_step_begin(qs_)
            ms_ = comm.wide_step_finish()
            assert [sum(ms_[r][q] for r in range(world)) for q in range(nq)] == want_m
            if i >= 1:
                collected.append(comm.wide_step_collect())
        collected.append(comm.wide_step_collect())
        assert collected == list(range(first_step, first_step + k)), collected
        for st in collected[-3:]:
            assert np.all(comm.wide_step_status(st) >= 0)
            check_step(st, nq)
        check_feeds(collected[-1], nq)
        return first_step + k

    # ---- what the oracle says about the first steps.  A shard's wide batch keeps its union only while no user's union outgrows the
    # union slots (16 per user at first, doubled after every batch that outgrew them, 64 at most): until then its Mu is -1.
    sel = np.zeros(n, bool)
    for w in all_want:
        sel[w[2]] = True
    per_user = np.bincount(cols[2][sel], minlength=U)
    union_rows = [int(per_user[maps[r][1]].sum()) for r in range(world)]
    union_max = [int(per_user[maps[r][1]].max()) for r in range(world)]
    assert max(union_max) <= 64 and min(union_rows) > 16
    slots = [16] * world
    # ---- a 16-row reservation: every step overflows at collect on every rank — a shard without a union (Mu = -1: "rerun the
    # batch") or a union above 16 rows ("re-reserve"); wide_step_status tells the two apart, exactly as the oracle predicts
    comm.wide_step_reserve(512, 0, 16)
    expect(E_STATE, comm.wide_step_status, 0)              # nothing collected yet
    step = 0
    saw_no_union = False
    while True:
        assert step < 4
        comm.wide_step_begin(all_q)
        if step == 0:
            expect(E_STATE, comm.scan_batch_gather, all_q[:7])
        ms = comm.wide_step_finish()
        assert [sum(ms[r][q] for r in range(world)) for q in range(512)] == [int(w[2].size) for w in all_want]
        expect(E_CAPACITY, comm.wide_step_collect)
        mu = comm.wide_step_status(step)
        want_mu = [union_rows[r] if union_max[r] <= slots[r] else -1 for r in range(world)]
        assert mu.shape == (world,) and list(mu) == want_mu, (step, list(mu), want_mu, union_max, slots)
        step += 1
        slots = [s_ * 2 if m_ < 0 else s_ for s_, m_ in zip(slots, want_mu)]
        if min(want_mu) >= 0:
            break
        saw_no_union = True
    assert saw_no_union == (max(union_max) > 16)
    if len(sys.argv) > 4:
        assert sys.argv[4] == "no-union" and saw_no_union, union_max
    need = comm.needed_cap()
    assert need >= max(union_rows) > 16
    comm.wide_step_reserve(512, 0, need)
    # ---- the pipelined runs
    step = run_pipelined(512, 9, step)
    step = run_pipelined(300, 6, step)
    step = run_pipelined(65, 4, step)
    # ---- a shard that cannot begin (a single scan in flight on the LAST rank's context): PIE_E_STATE, the step is not counted,
    # every context's batch room is what it was, four pipelined steps afterwards are exact and numbered without a gap.  The refusal
    # comes from the room check made before any shard begins; a shard failing after others began with steps in flight cannot be
    # staged through the public API (see comm_stub_worker.py: that branch is the same code for both kinds).
    rooms = [c.batch_room() for c in ctxs]
    assert min(rooms) > 0
    ctxs[world - 1].scan_begin(all_q[0][0], all_q[0][1])
    expect(E_STATE, comm.wide_step_begin, all_q[:65])
    ctxs[world - 1].scan_finish()
    assert [c.batch_room() for c in ctxs] == rooms
    step = run_pipelined(65, 4, step)
    # ---- mutual exclusion: no ordinary step while a wide step is uncollected, and the reverse
    qs7 = all_q[:7]
    comm.step_reserve(7, 0, need)
    comm.wide_step_begin(all_q[:65])
    expect(E_STATE, comm.step_begin, qs7)
    expect(E_STATE, comm.scan_batch_gather, qs7)
    expect(E_STATE, comm.expired_queue, T0 - DAY, T0)
    comm.wide_step_finish()
    expect(E_STATE, comm.step_begin, qs7)                   # finished, not collected
    assert comm.wide_step_collect() == step
    comm.step_begin(qs7)
    expect(E_STATE, comm.wide_step_begin, all_q[:65])
    ms7 = comm.step_finish()
    expect(E_STATE, comm.wide_step_begin, all_q[:65])
    st7 = comm.step_collect()
    # ---- the ordinary steps still pass their oracle check
    assert [sum(ms7[r][q] for r in range(world)) for q in range(7)] == [int(w[2].size) for w in all_want[:7]]
    for at in range(world):
        for r in range(world):
            uoff, rows, masks = comm.step_read_gathered(at, r, st7)
            rows_r, users_r = maps[r]
            for q in range(7):
                wc, wo, wi = all_want[q]
                sel = ((masks >> np.uint64(q)) & np.uint64(1)) == 1
                for lu in range(0, users_r.size, 7):
                    gu = int(users_r[lu])
                    a, b = int(uoff[lu]), int(uoff[lu + 1])
                    assert np.array_equal(rows_r[rows[a:b][sel[a:b]]], wi[wo[gu]:wo[gu + 1]]), (at, r, q, gu)
                checks += 1
    comm.close()
    try:
        os.remove(stub)
    except OSError:
        pass
    print("comm wide stub ok: world %d, %d checks" % (world, checks))


if __name__ == "__main__":
    main()
