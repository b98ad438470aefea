"""CPU: pie_set_turn_ordered (include/pie_scan.h) is declared, bound and exported alike, refuses a NULL context without a GPU, and
the Node addon names setTurnOrdered (and tableInfo, which the Node test reads the run's state through)."""
import ctypes as C
import os
import re

from conftest import REPO

PIE_E_INVAL = -1


def header_prototype(name):
    text = open(os.path.join(REPO, "include", "pie_scan.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    return None if m is None else [a.strip() for a in m.group(1).split(",")]


def test_library_exports_the_switch(pie):
    lib = pie.load_library()
    assert "pie_set_turn_ordered" in pie.ABI_SYMBOLS and getattr(lib, "pie_set_turn_ordered") is not None
    raw = C.CDLL(lib._name)
    assert raw.pie_set_turn_ordered is not None


def test_null_context_is_refused_without_a_gpu(pie):
    lib = pie.load_library()
    for on in (0, 1, 2, -1):
        assert lib.pie_set_turn_ordered(None, on) == PIE_E_INVAL


def test_binding_and_header_agree(pie):
    from sph_pie_amd import binding
    args = header_prototype("pie_set_turn_ordered")
    assert args == ["pie_ctx *ctx", "int on"]
    sigs = {name: (res, a) for name, res, a in binding._SIGS}
    res, a = sigs["pie_set_turn_ordered"]
    assert res is C.c_int and list(a) == [C.c_void_p, C.c_int] and sigs["pie_set_wide_ordered"] == sigs["pie_set_turn_ordered"]
    assert callable(pie.PieScan.set_turn_ordered)
    header = open(os.path.join(REPO, "include", "pie_scan.h")).read()
    assert "PIE_TURN_ORDERED=1" in header


def test_addon_and_host_name_the_switch():
    napi = open(os.path.join(REPO, "sph-pie_amd", "csrc", "pie_napi.c")).read()
    assert re.search(r"X\(int,\s*pie_set_turn_ordered,", napi) and '{"setTurnOrdered", fn_set_turn_ordered}' in napi
    assert '{"tableInfo", fn_table_info}' in napi
    store = open(os.path.join(REPO, "sph-pie_amd", "host", "tokenSessionStore.js")).read()
    assert "opts.turnOrdered" in store and "native.setTurnOrdered(ctx" in store
