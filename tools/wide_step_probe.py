#!/usr/bin/env python3
"""One pipelined 512-query WIDE step of the communicator (pie_comm_wide_step_*) against the same 512 queries as eight pipelined
64-query ordinary steps (pie_comm_step_*), and against the single-context alternative that existed before the wide step
(pie_scan_wide_begin, finish, pie_batch_pack_union_wide_device), all on one MI355X:
  rccl1   a 1-rank RCCL communicator over the shard-size table (1.25 x 10^7 rows / 12 500 users);
  stub8   8 shards of 10^8 rows / 10^5 users on GPU 0 (tests/stub_rccl.c stands in for RCCL: the "links" are copies on one
          device, so this times the host side and the shards' passes sharing one chip, not an exchange over xGMI).
bench.py's near-identical clocks (now - 977 ms q) and a heterogeneous mix, 3 batch lanes per shard, warm-up excluded, timed
regions of at least 200 steps.  Every configuration runs in a fresh child process with its own timeout; the parent writes the
record (default profiles/wide_step_probe.json).  Nobody has run the communicator across real links; these numbers do not either.

    python tools/wide_step_probe.py [--steps 200] [--modes rccl1,stub8] [--out profiles/wide_step_probe.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

T0 = 1_700_000_000_000
DAY, HOUR = 86400 * 1000, 3600 * 1000
M32 = 0xFFFFFFFF


def queries(mix, k):
    if mix == "bench":
        return [(T0 - 6 * HOUR - 977 * q, T0 - 61 * DAY, M32) for q in range(k)]
    masks = [0x55555555, 0xAAAAAAAA, M32, 0xFFFF0000, 0x1, 0x80000001]
    return [(T0 - 6 * HOUR - 977 * i - (i % 3) * HOUR, T0 - (61 + i % 4) * DAY - 13 * i, masks[i % len(masks)]) for i in range(k)]


def child(mode, steps):
    if mode == "stub8":
        stub_dir = os.path.join(REPO, "tests", "_stub")
        os.makedirs(stub_dir, exist_ok=True)
        stub = os.path.join(stub_dir, "libstub_rccl_probe.so")
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                        "-L/opt/rocm/lib", "-lamdhip64"], check=True, timeout=300)
        os.environ["PIE_RCCL_LIB"] = stub
    import torch  # noqa: F401  (before libpie_hip.so initialises HIP)
    import sph_pie_amd as pie
    pie.build_hip()
    world = 8 if mode == "stub8" else 1
    n, U = (10 ** 8, 10 ** 5) if mode == "stub8" else (12_500_000, 12_500)
    comm = pie.PieComm([0] * world)
    comm.gen_synthetic_sharded(0x5EED5EED, n, U, 32, 0)
    ctxs = [comm.ctx(r) for r in range(world)]
    for c in ctxs:
        c.set_disciplines(M32, 32)
        c.set_batch_lanes(3)

    def sync():
        for c in ctxs:
            c.synchronize()

    def wide_steps(qs, k):
        comm.wide_step_begin(qs)
        for i in range(k):
            if i + 1 < k:
                comm.wide_step_begin(qs)
            comm.wide_step_finish()
            if i >= 1:
                comm.wide_step_collect()
        comm.wide_step_collect()

    def ordinary_steps(groups, k):
        """k rounds of the eight 64-query steps, pipelined through the rounds"""
        items = [g for _ in range(k) for g in groups]
        comm.step_begin(items[0])
        for i in range(len(items)):
            if i + 1 < len(items):
                comm.step_begin(items[i + 1])
            comm.step_finish()
            if i >= 1:
                comm.step_collect()
        comm.step_collect()

    def timed(fn, k):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t) * 1e3 / k

    out = []
    reserved = 1024
    for mix in ("bench", "mixed"):
        q512 = queries(mix, 512)
        eight = [q512[64 * i: 64 * (i + 1)] for i in range(8)]
        # warm-up: the shards grow their union slots (Mu = -1 steps), then the reservation follows the gathered Mu words
        comm.wide_step_reserve(512, 0, 1024)
        need, no_union_steps = 0, 0
        for _ in range(6):
            comm.wide_step_begin(q512)
            comm.wide_step_finish()
            try:
                st = comm.wide_step_collect()
                break
            except pie.PieError as ex:
                if ex.code != pie.binding.PIE_E_CAPACITY:
                    raise
                st = None
                if all(int(v) >= 0 for v in comm.wide_step_status(comm_step_counter[0])):
                    need = comm.needed_cap()
                    comm.wide_step_reserve(512, 0, need)
                else:
                    no_union_steps += 1
            finally:
                comm_step_counter[0] += 1
        assert st is not None, "the wide step did not settle"
        mu = [int(v) for v in comm.wide_step_status(st)]
        reserved = max(reserved, need)
        comm.step_reserve(64, 0, reserved)
        wide_steps(q512, 20)
        comm_step_counter[0] += 20
        ordinary_steps(eight, 3)
        rec = {"mode": mode, "world": world, "rows_total": n, "users_total": U, "lanes": 3, "mix": mix, "steps": steps,
               "union_rows_per_rank": mu, "reserved_rows": reserved, "warmup_steps_without_union": no_union_steps}
        reps = []
        for _ in range(3):
            t_wide = timed(lambda: wide_steps(q512, steps), steps)
            comm_step_counter[0] += steps
            t_eight = timed(lambda: ordinary_steps(eight, max(steps // 8, 25)), max(steps // 8, 25))
            reps.append((t_wide, t_eight))
        reps.sort()
        rec["ms_wide_step_512"], rec["ms_eight_steps_64"] = reps[1]
        rec["wide_over_eight"] = rec["ms_wide_step_512"] / rec["ms_eight_steps_64"]
        if world == 1:
            # the single-context alternative: wide begin, finish, then the separate pack launch into device memory
            c = ctxs[0]
            words = 8
            dst = torch.empty(c.n_users + 2 + reserved * (1 + 2 * words), dtype=torch.int32, device="cuda:0")

            def single(k):
                begun = done = 0
                while done < k:
                    while begun < k and c.batch_room() > 0:
                        c.scan_wide_begin(q512)
                        begun += 1
                    c.scan_wide_finish()
                    c.batch_pack_union_wide_device(dst.data_ptr(), c.n_users, reserved)
                    done += 1

            def single_msg(k):
                begun = done = 0
                while done < k:
                    while begun < k and c.batch_room() > 0:
                        c.scan_wide_begin_union(q512, dst.data_ptr(), c.n_users, reserved)
                        begun += 1
                    c.scan_wide_finish_packed()
                    done += 1

            single(10)
            single_msg(10)
            rec["ms_single_ctx_wide_then_pack"] = sorted(timed(lambda: single(steps), steps) for _ in range(3))[1]
            rec["ms_single_ctx_wide_begin_union"] = sorted(timed(lambda: single_msg(steps), steps) for _ in range(3))[1]
        out.append(rec)
        print(json.dumps(rec), file=sys.stderr)
    comm.close()
    print(json.dumps(out))


comm_step_counter = [0]   # wide steps begun so far in this process (= the number of the next step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--modes", default="rccl1,stub8")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide_step_probe.json"))
    ap.add_argument("--child", default="")
    ap.add_argument("--timeout", type=int, default=420)
    args = ap.parse_args()
    if args.child:
        child(args.child, max(args.steps, 200))
        return
    record = {"tool": "wide_step_probe", "steps": max(args.steps, 200), "results": [], "failed": []}
    for mode in [m for m in args.modes.split(",") if m]:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--steps", str(args.steps)], cwd=REPO,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.timeout)
        if res.returncode != 0:   # reported, not retried
            record["failed"].append({"mode": mode, "returncode": res.returncode, "stderr": res.stderr[-2000:]})
            break
        record["results"].extend(json.loads(res.stdout.strip().splitlines()[-1]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps(record))
    sys.exit(1 if record["failed"] else 0)


if __name__ == "__main__":
    main()
