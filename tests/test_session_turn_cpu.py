"""CPU: the host side of pie_session_turn (include/pie_scan.h), the turn that logs in.
  1. tests/session_turn_model.py, the executable form of the header's rules (a CREATE is append_rows + token_append where the op
     stands), replays the recorded reference trace G5 with the create calls inside the turns, in turns of every size: the model is
     shown to match the reference's sessionStore.js before any GPU test leans on it.
  2. pie_session_turn_plan — the row every create gets, the chains — against a Python restatement and pie_token_turn_plan, and the
     planning code through a stand-alone program under ASan + UBSan (tests/session_turn_plan_test.cpp).
  3. The entry points are declared, bound and exported alike, and refuse bad arguments."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from session_turn_model import CREATE, SessionModelStore, SessionTurnModel, replay_g5_sessions
from trace_replay import load_trace
from turn_model import DELETE, GET, TOUCH, TURN_OP, make_ops

PIE_E_INVAL = -1
ENTRY_POINTS = {"pie_session_turn_plan": 7, "pie_session_turn": 11}
NONE = -(2 ** 63)


@pytest.mark.parametrize("chunk", [None, 1, 7, 64])
def test_model_replays_g5_with_the_logins_in_the_turns(chunk):
    trace = load_trace(GOLDEN)
    kinds = [op["op"] for op in trace["ops"]]
    assert len(kinds) == 1345 and kinds.count("create") == trace["sessions"] == 659
    store = SessionModelStore(len(trace["users"]))
    checked, turns, largest, mixed = replay_g5_sessions(trace, store, chunk)
    assert checked == 1345 and store.m.start.shape[0] == 659 and store.m.covered == 659
    assert largest <= (chunk or 10 ** 9)
    if chunk == 1:
        assert mixed == 0 and turns >= 659 + 493
    else:
        assert mixed > 300, "most logins share their turn with other calls"


def test_model_rules_by_hand():
    """the CREATE line of the header's table beside the other three, on one key"""
    m = SessionTurnModel([10], [100], [3], [0])
    key, other = np.array([[7, 9]], np.uint64), np.array([[9, 7]], np.uint64)
    m.token_set(key)
    ops = np.concatenate([make_ops(other, 50, GET), make_ops(key, 50, TOUCH, 500), make_ops(key, 60, CREATE, 900), make_ops(key, 70, GET),
                          make_ops(key, 80, DELETE), make_ops(key, 90, CREATE, 90), make_ops(key, 0, GET), make_ops(other, 5, CREATE, 6),
                          make_ops(other, 5, GET)])
    user, disc = np.arange(9, dtype=np.int32) + 10, np.arange(9, dtype=np.int32) + 20
    got = m.turn(ops, user, disc)
    assert got["row"].tolist() == [-1, 0, 1, 1, 1, 2, 2, 3, 3]
    assert got["live"].tolist() == [0, 1, 1, 1, 0, 0, 1, 1, 1]
    assert got["end"].tolist() == [NONE, 500, 900, 900, NONE, 90, 90, 6, 6]
    assert got["user"].tolist()[1:] == [3, 12, 12, 12, 15, 15, 17, 17] and got["start"].tolist()[1:] == [10, 60, 60, 60, 90, 90, 5, 5]
    assert m.end.tolist() == [500, NONE, 90, 6] and m.user.tolist() == [3, 12, 15, 17] and m.disc.tolist() == [0, 22, 25, 27]
    assert m.covered == 4 and m.rows_of(np.concatenate([key, other])).tolist() == [2, 3]


def seeded_ops(seed, k, n_keys, p_create):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 2 ** 64, (max(n_keys, 1), 2), dtype=np.uint64)
    ops = make_ops(pool[rng.integers(0, max(n_keys, 1), k)], 5, GET)
    ops["kind"] = rng.choice([GET, TOUCH, DELETE, CREATE], k, p=[(1 - p_create) / 3] * 3 + [p_create])
    return ops


@pytest.mark.parametrize("k, n_keys, p_create", [(0, 1, 0.5), (1, 1, 1.0), (300, 300, 1.0), (257, 40, 0.2), (5000, 13, 0.25), (1000, 1000, 0.0)])
def test_plan_matches_its_restatement(pie, k, n_keys, p_create):
    ops = seeded_ops(17 + k, k, n_keys, p_create)
    row0 = 3000 + k
    nxt, head, new_row, n_create = pie.session_turn_plan(ops, row0)
    is_create = ops["kind"] == CREATE
    want = np.where(is_create, row0 + np.cumsum(is_create) - 1, -1).astype(np.int32)
    assert np.array_equal(new_row, want) and n_create == int(is_create.sum())
    base_next, base_head = pie.token_turn_plan(ops)              # the chains are pie_token_turn_plan's: kinds are not looked at there
    assert np.array_equal(nxt, base_next) and np.array_equal(head, base_head)


def test_plan_under_sanitizers(tmp_path):
    """the planning code is plain functions (csrc/pie_turn_plan.h): a stand-alone program runs them under ASan + UBSan and checks
    the rows the creates get and the kernel's walk against a map that applies the ops one by one"""
    assert shutil.which("g++") is not None, "g++ is needed for the stand-alone planning check"
    exe = tmp_path / "session_turn_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(REPO, "tests", "session_turn_plan_test.cpp")])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and "session turn plan ok" in res.stdout, res.stdout


def header_prototypes():
    text = open(os.path.join(REPO, "include", "pie_scan.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for name, args in re.findall(r"\bint\s+(pie_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        args = args.strip()
        protos[name] = 0 if args in ("", "void") else args.count(",") + 1
    return protos


def test_header_binding_and_addon_agree(pie):
    from sph_pie_amd import binding
    protos = header_prototypes()
    assert {n: protos.get(n) for n in ENTRY_POINTS} == ENTRY_POINTS
    sigs = {name: args for name, _, args in binding._SIGS}
    lib = pie.load_library()
    for name, n_args in ENTRY_POINTS.items():
        assert name in pie.ABI_SYMBOLS and len(sigs[name]) == n_args and getattr(lib, name) is not None, name
    assert binding.TURN_CREATE == CREATE == pie.TURN_CREATE and binding.TURN_OP == TURN_OP and binding.TURN_OP.itemsize == 40
    header = open(os.path.join(REPO, "include", "pie_scan.h")).read()
    assert re.search(r"#define\s+PIE_TURN_CREATE\s+3\b", header)
    assert callable(pie.PieScan.session_turn) and callable(pie.session_turn_plan)
    napi = open(os.path.join(REPO, "sph-pie_amd", "csrc", "pie_napi.c")).read()
    assert re.search(r"X\(int,\s*pie_session_turn,", napi) and '{"sessionTurn",' in napi


def test_argument_errors_without_a_context(pie):
    lib = pie.load_library()
    ops = make_ops(np.array([[1, 2], [1, 2], [3, 4]], np.uint64), 5, CREATE, 9)
    ops["kind"][1] = GET
    nxt, head, new_row = np.full(3, 77, np.int32), np.full(3, 77, np.uint8), np.full(3, 77, np.int32)
    n_create = C.c_size_t(55)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    plan = lambda o, k, row0, a, b, c: lib.pie_session_turn_plan(o, k, row0, a, b, c, C.byref(n_create))
    assert plan(None, 3, 0, p(nxt), p(head), p(new_row)) == PIE_E_INVAL
    assert plan(p(ops), 3, 0, None, p(head), p(new_row)) == PIE_E_INVAL
    assert plan(p(ops), 3, 0, p(nxt), None, p(new_row)) == PIE_E_INVAL
    assert plan(p(ops), 3, 0, p(nxt), p(head), None) == PIE_E_INVAL
    assert plan(p(ops), 2 ** 31, 0, p(nxt), p(head), p(new_row)) == PIE_E_INVAL
    assert plan(p(ops), 3, -1, p(nxt), p(head), p(new_row)) == PIE_E_INVAL
    assert plan(p(ops), 3, 2 ** 31 - 3, p(nxt), p(head), p(new_row)) == PIE_E_INVAL, "two creates would reach 2^31 - 1 rows"
    for field, value in (("kind", 4), ("kind", -1), ("reserved", 1)):
        bad = ops.copy()
        bad[field][2] = value
        assert plan(p(bad), 3, 0, p(nxt), p(head), p(new_row)) == PIE_E_INVAL, (field, value)
    assert nxt.tolist() == [77] * 3 and head.tolist() == [77] * 3 and new_row.tolist() == [77] * 3 and n_create.value == 55
    assert plan(None, 0, 10, None, None, None) == 0 and n_create.value == 0
    assert plan(p(ops), 3, 2 ** 31 - 4, p(nxt), p(head), p(new_row)) == 0 and new_row.tolist() == [2 ** 31 - 4, -1, 2 ** 31 - 3]
    assert plan(p(ops), 3, 10, p(nxt), p(head), p(new_row)) == 0
    assert nxt.tolist() == [1, -1, -1] and head.tolist() == [1, 0, 1] and new_row.tolist() == [10, -1, 11] and n_create.value == 2
    assert lib.pie_session_turn_plan(p(ops), 3, 10, p(nxt), p(head), p(new_row), None) == 0, "n_create_out may be NULL"
    # a NULL context is refused before anything is looked at
    user = np.zeros(3, np.int32)
    assert lib.pie_session_turn(None, p(ops), 3, p(user), p(user), 1, None, None, None, None, None) == PIE_E_INVAL
    with pytest.raises(pie.PieError):
        pie.session_turn_plan(ops, -5)
