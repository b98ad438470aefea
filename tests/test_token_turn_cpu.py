"""CPU: the host side of pie_token_turn (include/pie_scan.h).
  1. pie_token_turn_plan — the chains the device walks — against a Python restatement, and the same key sets through a stand-alone
     program under ASan + UBSan (tests/turn_plan_test.cpp).
  2. tests/turn_model.py, the executable form of the header's rules, replays the recorded reference trace G5 in turns of every
     size: the model is shown to match the reference's sessionStore.js before any GPU test leans on it.
  3. The entry points are declared, bound and exported alike, and refuse bad arguments."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from trace_replay import load_trace
from turn_model import DELETE, GET, TOUCH, TURN_OP, ModelStore, TurnModel, make_ops, replay_g5

PIE_E_INVAL = -1
ENTRY_POINTS = {"pie_token_turn_plan": 4, "pie_token_turn": 8, "pie_shard_token_turn": 8, "pie_comm_token_turn": 9}


def key_sets():
    rng = np.random.default_rng(11)
    distinct = rng.integers(0, 2 ** 64, (1000, 2), dtype=np.uint64)
    pool = rng.integers(0, 2 ** 64, (13, 2), dtype=np.uint64)
    pool[1] = pool[0][::-1]                       # the two words are not interchangeable
    pool[2] = (pool[0][0], pool[3][1])            # equal in one word only
    return {"distinct": distinct, "equal": np.tile(distinct[:1], (777, 1)), "none": distinct[:0], "one": distinct[:1],
            "repeats": pool[rng.integers(0, 13, 5000)]}


def plan_in_python(keys):
    last, nxt, head = {}, np.full(len(keys), -1, np.int32), np.zeros(len(keys), np.uint8)
    for i, k in enumerate(keys):
        k = (int(k[0]), int(k[1]))
        if k in last:
            nxt[last[k]] = i
        else:
            head[i] = 1
        last[k] = i
    return nxt, head


@pytest.mark.parametrize("name", ["distinct", "equal", "none", "one", "repeats"])
def test_plan_matches_its_restatement(pie, name):
    keys = key_sets()[name]
    ops = make_ops(keys, 5, GET)
    ops["kind"] = np.arange(len(keys)) % 3        # the plan looks at keys alone
    nxt, head = pie.token_turn_plan(ops)
    want_next, want_head = plan_in_python(keys)
    assert np.array_equal(nxt, want_next) and np.array_equal(head, want_head)
    assert int(head.sum()) == len({(int(a), int(b)) for a, b in keys})


def test_plan_under_sanitizers(tmp_path):
    """the plan is a plain function (csrc/pie_turn_plan.h): a stand-alone program runs it on the same five key sets under
    ASan + UBSan and checks it against a map"""
    assert shutil.which("g++") is not None, "g++ is needed for the stand-alone planning check"
    exe = tmp_path / "turn_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(REPO, "tests", "turn_plan_test.cpp")])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and "turn plan ok" in res.stdout, res.stdout


def test_model_rules_by_hand():
    """the table of include/pie_scan.h, one line at a time, on one row"""
    none = -(2 ** 63)
    m = TurnModel([10], [100], [3], [0])
    key = np.array([[7, 9]], np.uint64)
    m.token_set(key)
    ops = np.concatenate([make_ops(key, 50, GET), make_ops(key, 99, TOUCH, 500), make_ops(key, 100, GET), make_ops(key, 500, TOUCH, 900),
                          make_ops(key, 499, GET), make_ops(key, 10 ** 6, DELETE), make_ops(key, 0, TOUCH, 700), make_ops(key, 0, GET),
                          make_ops(key, 0, DELETE), make_ops(np.array([[9, 7]], np.uint64), 0, GET)])
    got = m.turn(ops)
    assert got["live"].tolist() == [1, 1, 1, 0, 1, 0, 0, 0, 0, 0]
    assert got["end"].tolist() == [100, 500, 500, 500, 500, none, none, none, none, none]
    assert got["row"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, -1, -1]
    assert m.end.tolist() == [none]


@pytest.mark.parametrize("chunk", [None, 1, 7, 64])
def test_model_replays_g5_in_turns(chunk):
    trace = load_trace(GOLDEN)
    kinds = [op["op"] for op in trace["ops"]]
    assert len(kinds) == 1345 and sum(k in ("get", "touch", "del") for k in kinds) == 493
    nows = [op["now"] for op in trace["ops"]]
    assert all(a <= b for a, b in zip(nows, nows[1:])), "the clocks do not decrease: the expired-lookup rule is covered"
    checked, turns, largest = replay_g5(trace, ModelStore(len(trace["users"])), chunk)
    assert checked == 1345
    assert largest <= (chunk or 10 ** 9) and (chunk != 1 or turns >= 493)
    if chunk is None:
        assert largest >= 500, "a census of every token issued is one turn"


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
    assert binding.TURN_OP == TURN_OP and binding.TURN_OP.itemsize == 40
    assert (binding.TURN_GET, binding.TURN_TOUCH, binding.TURN_DELETE) == (GET, TOUCH, DELETE)
    header = open(os.path.join(REPO, "include", "pie_scan.h")).read()
    for name, value in (("PIE_TURN_GET", GET), ("PIE_TURN_TOUCH", TOUCH), ("PIE_TURN_DELETE", DELETE)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
    for method in ("token_turn", "shard_token_turn"):
        assert callable(getattr(pie.PieScan, method))
    assert callable(pie.PieComm.token_turn)
    napi = open(os.path.join(REPO, "sph-pie_amd", "csrc", "pie_napi.c")).read()
    for name in ("pie_token_turn", "pie_comm_token_turn"):
        assert re.search(r"X\(int,\s*%s," % name, napi), name
    for export in ("tokenTurn", "commTokenTurn"):
        assert '{"%s",' % export in napi, export


def test_argument_errors_without_a_context(pie):
    lib = pie.load_library()
    ops = make_ops(np.array([[1, 2], [1, 2]], np.uint64), 5, GET)
    nxt, head = np.full(2, 77, np.int32), np.full(2, 77, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.pie_token_turn_plan(None, 2, p(nxt), p(head)) == PIE_E_INVAL
    assert lib.pie_token_turn_plan(p(ops), 2, None, p(head)) == PIE_E_INVAL
    assert lib.pie_token_turn_plan(p(ops), 2, p(nxt), None) == PIE_E_INVAL
    assert lib.pie_token_turn_plan(p(ops), 2 ** 31, p(nxt), p(head)) == PIE_E_INVAL
    assert nxt.tolist() == [77, 77] and head.tolist() == [77, 77]
    assert lib.pie_token_turn_plan(None, 0, None, None) == 0
    assert lib.pie_token_turn_plan(p(ops), 2, p(nxt), p(head)) == 0 and nxt.tolist() == [1, -1] and head.tolist() == [1, 0]
    # a NULL context or communicator is refused before anything is looked at
    assert lib.pie_token_turn(None, p(ops), 2, None, None, None, None, None) == PIE_E_INVAL
    assert lib.pie_shard_token_turn(None, p(ops), 2, None, None, None, None, None) == PIE_E_INVAL
    assert lib.pie_comm_token_turn(None, p(ops), 2, None, None, None, None, None, None) == PIE_E_INVAL
    with pytest.raises(ValueError):
        pie.turn_ops(np.zeros(3, np.int64))
