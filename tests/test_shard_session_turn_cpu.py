"""CPU: the host side of pie_shard_session_turn and pie_comm_session_turn (include/pie_scan.h), the turn that logs in on a sharded
table.
  1. pie_shard_session_turn_plan against a Python restatement for worlds 1, 2, 3, 5 and every rank, on seeded op lists: global rows
     are N_g + j, local rows count only kept creates, the chains equal pie_token_turn_plan's; its PIE_E_INVAL cases.
  2. The planning code through a stand-alone program under ASan + UBSan (tests/shard_session_turn_plan_test.cpp).
  3. The three entry points are declared, bound and exported alike, and refuse NULL contexts and NULL pointers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from session_turn_model import CREATE
from turn_model import DELETE, GET, TOUCH, TURN_OP, make_ops

PIE_E_INVAL = -1
ENTRY_POINTS = {"pie_shard_session_turn_plan": 13, "pie_shard_session_turn": 11, "pie_comm_session_turn": 12}


def seeded(seed, k, n_keys, p_create, users=997):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 2 ** 64, (max(n_keys, 1), 2), dtype=np.uint64)
    ops = make_ops(pool[rng.integers(0, max(n_keys, 1), k)], 5, GET)
    ops["kind"] = rng.choice([GET, TOUCH, DELETE, CREATE], k, p=[(1 - p_create) / 3] * 3 + [p_create])
    return ops, rng.integers(0, users, k).astype(np.int32)


@pytest.mark.parametrize("world", [1, 2, 3, 5])
@pytest.mark.parametrize("k, n_keys, p_create", [(0, 1, 0.5), (1, 1, 1.0), (300, 300, 1.0), (257, 40, 0.2), (5000, 13, 0.25), (1000, 1000, 0.0)])
def test_plan_matches_its_restatement(pie, world, k, n_keys, p_create):
    ops, user = seeded(31 + k + world, k, n_keys, p_create)
    n_g, n_l = 3000 + k, 700
    create = ops["kind"] == CREATE
    owner = np.array([pie.shard_of(int(u), world) for u in user], np.int32)
    base_next, base_head = pie.token_turn_plan(ops)
    kept_total = 0
    for rank in range(world):
        nxt, head, row_g, row_l, n_create, n_kept = pie.shard_session_turn_plan(ops, user, n_g, n_l, rank, world)
        assert np.array_equal(row_g, np.where(create, n_g + np.cumsum(create) - 1, -1)), "global rows are N_g + j, on every rank alike"
        mine = create & (owner == rank)
        assert np.array_equal(row_l, np.where(mine, n_l + np.cumsum(mine) - 1, -1)), "local rows count only kept creates"
        assert n_create == int(create.sum()) and n_kept == int(mine.sum())
        assert np.array_equal(nxt, base_next) and np.array_equal(head, base_head), "the chains are pie_token_turn_plan's"
        assert pie.PieScan.shard_session_turn_plan(ops, user, n_g, n_l, rank, world)[5] == n_kept
        kept_total += n_kept
    assert kept_total == int(create.sum()), "every create is kept by exactly one rank"


def test_plan_under_sanitizers(tmp_path):
    """the planning code is plain functions (csrc/pie_turn_plan.h): a stand-alone program runs them under ASan + UBSan"""
    assert shutil.which("g++") is not None, "g++ is needed for the stand-alone planning check"
    exe = tmp_path / "shard_session_turn_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(REPO, "tests", "shard_session_turn_plan_test.cpp")])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and "shard session turn plan ok" in res.stdout, res.stdout


def header_prototypes():
    text = open(os.path.join(REPO, "include", "pie_scan.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for name, args in re.findall(r"\bint\s+(pie_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        args = args.strip()
        protos[name] = 0 if args in ("", "void") else args.count(",") + 1
    return protos


def test_header_and_binding_agree(pie):
    from sph_pie_amd import binding
    protos = header_prototypes()
    assert {n: protos.get(n) for n in ENTRY_POINTS} == ENTRY_POINTS
    sigs = {name: args for name, _, args in binding._SIGS}
    lib = pie.load_library()
    for name, n_args in ENTRY_POINTS.items():
        assert name in pie.ABI_SYMBOLS and len(sigs[name]) == n_args and getattr(lib, name) is not None, name
    assert callable(pie.PieScan.shard_session_turn) and callable(pie.PieComm.session_turn) and callable(pie.shard_session_turn_plan)
    assert "shard_session_turn_plan" in pie.__all__ and binding.TURN_OP == TURN_OP


def test_argument_errors_without_a_context(pie):
    lib = pie.load_library()
    ops = make_ops(np.array([[1, 2], [1, 2], [3, 4]], np.uint64), 5, CREATE, 9)
    ops["kind"][1] = GET
    user = np.array([4, 4, 5], np.int32)
    world = 3
    rank = pie.shard_of(4, world)
    nxt, head, row_g, row_l = np.full(3, 77, np.int32), np.full(3, 77, np.uint8), np.full(3, 77, np.int32), np.full(3, 77, np.int32)
    n_create, n_kept = C.c_size_t(55), C.c_size_t(56)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def plan(o=p(ops), k=3, u=p(user), n_g=10, n_l=4, r=rank, w=world, a=p(nxt), b=p(head), c=p(row_g), d=p(row_l)):
        return lib.pie_shard_session_turn_plan(o, k, u, n_g, n_l, r, w, a, b, c, d, C.byref(n_create), C.byref(n_kept))

    for bad in (dict(o=None), dict(u=None), dict(a=None), dict(b=None), dict(c=None), dict(d=None), dict(k=2 ** 31), dict(n_g=-1), dict(n_l=-1),
                dict(n_l=11), dict(r=-1), dict(r=world), dict(w=0), dict(n_g=2 ** 31 - 3, n_l=0)):
        assert plan(**bad) == PIE_E_INVAL, bad
    for field, value in (("kind", 4), ("kind", -1), ("reserved", 1)):
        wrong = ops.copy()
        wrong[field][2] = value
        assert plan(o=p(wrong)) == PIE_E_INVAL, (field, value)
    assert nxt.tolist() == [77] * 3 and head.tolist() == [77] * 3 and row_g.tolist() == [77] * 3 and row_l.tolist() == [77] * 3
    assert n_create.value == 55 and n_kept.value == 56, "nothing is written on an error"
    assert plan(o=None, k=0, u=None, a=None, b=None, c=None, d=None) == 0 and n_create.value == 0 and n_kept.value == 0
    assert plan() == 0
    mine5 = pie.shard_of(5, world) == rank
    assert nxt.tolist() == [1, -1, -1] and head.tolist() == [1, 0, 1] and row_g.tolist() == [10, -1, 11]
    assert row_l.tolist() == [4, -1, 5 if mine5 else -1] and n_create.value == 2 and n_kept.value == (2 if mine5 else 1)
    assert plan(n_g=2 ** 31 - 4, n_l=0) == 0 and row_g.tolist() == [2 ** 31 - 4, -1, 2 ** 31 - 3]
    gets = make_ops(np.array([[1, 2]], np.uint64), 5, GET)
    assert plan(o=p(gets), k=1, u=None) == 0, "user_global is read at creates only"
    assert lib.pie_shard_session_turn_plan(p(ops), 3, p(user), 10, 4, rank, world, p(nxt), p(head), p(row_g), p(row_l), None, None) == 0
    # a NULL context or communicator is refused before anything is looked at
    assert lib.pie_shard_session_turn(None, p(ops), 3, p(user), p(user), 9, None, None, None, None, None) == PIE_E_INVAL
    assert lib.pie_comm_session_turn(None, p(ops), 3, p(user), p(user), 9, None, None, None, None, None, None) == PIE_E_INVAL
    with pytest.raises(pie.PieError):
        pie.shard_session_turn_plan(ops, user, 10, 4, world, world)
