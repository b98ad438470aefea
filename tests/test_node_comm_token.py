"""GPU: the Node addon's token column behind the communicator (commTokenSet / commTokenAppend / commTokenLookup /
commTokenSetEnd) — a fresh node child with its own timeout runs sph-pie_amd/host/test/comm_token_test.js: world 2 on GPU 0
through PIE_RCCL_LIB (tests/stub_rccl.c), against vectors the unsharded Python model (tests/token_model.py) produced: hits, a
miss, an expired token, a tombstone and a key carried by rows of two shards."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from token_model import END_NONE, TokenModel

HOST = os.path.join(REPO, "sph-pie_amd", "host")
node = shutil.which("node")
needs_node = pytest.mark.skipif(node is None, reason="node is not installed on this machine")
SEED, N, U, D, WORLD = 0x5EED5EED, 20000, 300, 32, 2


def vectors(pie, oracle):
    tm = TokenModel(*oracle.gen(SEED, N, 0, N, U, D, 0))
    owner = np.array([pie.shard_of(u, WORLD) for u in range(U + 2)], np.int32)
    rng = np.random.default_rng(2026)
    keys = rng.integers(0, 2 ** 64, (N + 40, 2), dtype=np.uint64)
    now = int(np.median(tm.end))
    live, dead = np.nonzero(tm.end > now)[0], np.nonzero((tm.end <= now) & (tm.end != END_NONE))[0]
    # one key on a row of rank 0 and a LATER row of rank 1, and the other way round: the largest global row answers
    r0, r1 = np.nonzero(owner[tm.user] == 0)[0], np.nonzero(owner[tm.user] == 1)[0]
    dup = [(int(r0[10]), int(r1[r1 > r0[10]][5])), (int(r1[200]), int(r0[r0 > r1[200]][7]))]
    for a, b in dup:
        keys[b] = keys[a]

    def strs(a):
        return [str(int(x)) for x in a]

    def key_list(k):
        return [[str(int(x[0])), str(int(x[1]))] for x in k]

    def lookup(ask, at):
        want = tm.lookup(ask, at)
        f = want["found"]
        return {"keys": key_list(ask), "now": str(at), "row": want["row"].tolist(), "live": want["live"].tolist(),
                "user": np.where(f, want["user"], -1).tolist(), "start": strs(want["start"]), "end": strs(want["end"]),
                "owner": np.where(f, owner[want["user"]], -1).tolist()}

    miss = rng.integers(0, 2 ** 64, (3, 2), dtype=np.uint64)
    probe = np.concatenate([keys[live[:20]], keys[dead[:5]], miss, keys[[a for a, _ in dup]], keys[N - 3: N + 40]])
    out = {"world": WORLD, "seed": str(SEED), "n": N, "users": U, "disc": D}
    tm.token_set(keys[: N - 30])
    out["set_keys"] = key_list(keys[: N - 30])
    out["lookup_after_set"] = lookup(probe, now)
    assert out["lookup_after_set"]["row"][25:28] == [-1, -1, -1] and out["lookup_after_set"]["row"][28:30] == [b for _, b in dup]
    assert out["lookup_after_set"]["live"][20:25] == [0] * 5, "expired tokens are found and not live"
    # logins: 40 rows (two new users), then keys for the 30 uncovered rows and the 40 new ones
    top = oracle.T0_MS + oracle.SPAN_MS
    s = (top + 100000 + np.arange(40)).astype(np.int64)
    e = s + rng.integers(oracle.TTL_MS // 4, oracle.TTL_MS, 40)
    u = rng.integers(0, U + 2, 40).astype(np.int32)
    u[:2] = [U, U + 1]
    d = rng.integers(0, D, 40).astype(np.int32)
    tm.append_rows(s, e, u, d)
    tm.token_append(keys[N - 30:])
    out["append"] = {"start": strs(s), "end": strs(e), "user": u.tolist(), "disc": d.tolist(), "n_users": U + 2, "keys": key_list(keys[N - 30:])}
    out["lookup_after_append"] = lookup(probe, now)
    assert out["lookup_after_append"]["row"][-40:] == list(range(N, N + 40))
    # touches and deletes by token: a repeat, an expired token, a miss, a duplicate, a delete
    ask = np.concatenate([keys[live[:6]], keys[live[2:3]], keys[dead[:2]], miss[:1], keys[dup[0][0]][None], keys[N + 5: N + 7]])
    new_end = (top + rng.integers(1, oracle.TTL_MS, ask.shape[0])).astype(np.int64)
    new_end[1] = END_NONE
    rows = tm.token_set_end(ask, new_end, now)
    assert rows[6] == live[2] and list(rows[7:10]) == [-1, -1, -1]
    out["set_end"] = {"keys": key_list(ask), "new_end": strs(new_end), "now": str(now), "rows": rows.tolist()}
    out["lookup_after_set_end"] = lookup(probe, now)
    return out


@needs_node
@pytest.mark.gpu
def test_token_calls_through_the_node_host(pie, oracle, tmp_path):
    assert pie.build_napi() is not None, "node headers (node_api.h) not found"
    stub_dir = os.path.join(REPO, "tests", "_stub")
    os.makedirs(stub_dir, exist_ok=True)
    stub = os.path.join(stub_dir, "libstub_rccl_node_token.so")
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                    "-L/opt/rocm/lib", "-lamdhip64"], check=True, timeout=300)
    path = tmp_path / "comm_token_vectors.json"
    path.write_text(json.dumps(vectors(pie, oracle)))
    res = subprocess.run([node, os.path.join(HOST, "test", "comm_token_test.js")], cwd=REPO,
                         env=dict(os.environ, TZ="UTC", PIE_RCCL_LIB=stub, PIE_TOKEN_VECTORS=str(path)),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:]
    assert "host comm_token_test ok" in res.stdout
