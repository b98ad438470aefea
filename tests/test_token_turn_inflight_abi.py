"""CPU: the five entry points of the in-flight token turn exist in the built library, are declared in include/pie_scan.h, are
bound in binding.py with as many arguments as the header, and reach the addon as three exports; a NULL context is refused.  No
compute calls here."""
import ctypes as C
import os
import re

from conftest import REPO

ENTRY_POINTS = {"pie_token_turn_begin": 3, "pie_token_turn_finish": 8, "pie_token_turn_room": 1, "pie_shard_token_turn_begin": 3,
                "pie_shard_token_turn_finish": 8}
PIE_E_INVAL = -1


def header_prototypes():
    text = open(os.path.join(REPO, "include", "pie_scan.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for name, args in re.findall(r"\bint\s+(pie_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        args = args.strip()
        protos[name] = 0 if args in ("", "void") else args.count(",") + 1
    return protos


def test_header_declares_the_entry_points():
    protos = header_prototypes()
    assert {n: protos.get(n) for n in ENTRY_POINTS} == ENTRY_POINTS


def test_library_exports_and_binding_declares_them(pie):
    from sph_pie_amd import binding
    sigs = {name: (res, args) for name, res, args in binding._SIGS}
    lib = pie.load_library()
    for name, n_args in ENTRY_POINTS.items():
        assert name in pie.ABI_SYMBOLS and name in sigs, name
        assert len(sigs[name][1]) == n_args, name
        assert getattr(lib, name) is not None, name
    for method in ("token_turn_begin", "token_turn_finish", "token_turn_room", "shard_token_turn_begin", "shard_token_turn_finish"):
        assert callable(getattr(pie.PieScan, method)), method


def test_addon_source_exports_the_three_calls():
    src = open(os.path.join(REPO, "sph-pie_amd", "csrc", "pie_napi.c")).read()
    for js, fn, sym in (("tokenTurnBegin", "fn_token_turn_begin", "pie_token_turn_begin"),
                        ("tokenTurnFinish", "fn_token_turn_finish", "pie_token_turn_finish"),
                        ("tokenTurnRoom", "fn_token_turn_room", "pie_token_turn_room")):
        assert re.search(r'\{"%s",\s*%s\}' % (js, fn), src), js
        assert re.search(r"X\(int, %s," % sym, src), sym
    store = open(os.path.join(REPO, "sph-pie_amd", "host", "tokenSessionStore.js")).read()
    assert "turnAsync" in store and "tokenTurnBegin" in store and "tokenTurnFinish" in store


def test_null_context_is_refused(pie):
    lib = pie.load_library()
    ops = (C.c_char * 40)()
    k_out = C.c_size_t(7)
    assert lib.pie_token_turn_begin(None, ops, 1) == PIE_E_INVAL
    assert lib.pie_shard_token_turn_begin(None, ops, 1) == PIE_E_INVAL
    assert lib.pie_token_turn_finish(None, None, None, None, None, None, 0, C.byref(k_out)) == PIE_E_INVAL
    assert lib.pie_shard_token_turn_finish(None, None, None, None, None, None, 0, C.byref(k_out)) == PIE_E_INVAL
    assert lib.pie_token_turn_room(None) == PIE_E_INVAL
    assert k_out.value == 7
