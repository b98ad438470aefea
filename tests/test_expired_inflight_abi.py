"""CPU: the six entry points of the in-flight expired queue are declared in include/pie_scan.h, the binding declares each with as
many arguments as the header, the Node addon resolves and exports them, and every one refuses a NULL context with PIE_E_INVAL.
No compute calls here."""
import ctypes as C
import os
import re
import shutil
import subprocess

from conftest import REPO

ENTRY_POINTS = {"pie_expired_queue_begin": 4, "pie_expired_queue_finish": 4, "pie_expired_queue_room": 1,
                "pie_shard_expired_queue_begin": 4, "pie_shard_expired_queue_finish": 4, "pie_expired_inflight_geometry": 5}
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


def test_binding_declares_them_with_matching_argument_counts(pie):
    from sph_pie_amd import binding
    sigs = {name: (res, args) for name, res, args in binding._SIGS}
    for name, n_args in ENTRY_POINTS.items():
        assert name in pie.ABI_SYMBOLS and name in sigs, name
        assert len(sigs[name][1]) == n_args, name
    lib = pie.load_library()
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None
    for method in ("expired_queue_begin", "expired_queue_finish", "expired_queue_room", "shard_expired_queue_begin",
                   "shard_expired_queue_finish", "expired_inflight_geometry"):
        assert callable(getattr(pie.PieScan, method))
    fields = [f for f, _ in binding.PieTableInfo._fields_]
    assert fields[-2:] == ["expired_inflight_bytes", "expired_inflight_ms"], "the struct grows at its end only"


def test_addon_resolves_and_exports_them():
    text = open(os.path.join(REPO, "sph-pie_amd", "csrc", "pie_napi.c")).read()
    for name in ("pie_expired_queue_begin", "pie_expired_queue_finish", "pie_expired_queue_room"):
        assert re.search(r"X\(int,\s*%s," % name, text), name
    for export in ("expiredQueueBegin", "expiredQueueFinish", "expiredQueueRoom"):
        assert '{"%s",' % export in text, export


def test_planning_under_sanitizers(tmp_path):
    """the pass's geometry, scratch layout and buffer sizing are plain functions (csrc/pie_expq_plan.h): a stand-alone program
    replays them on host arrays under ASan + UBSan"""
    assert shutil.which("g++") is not None, "g++ is needed for the stand-alone planning check"
    exe = tmp_path / "expq_plan_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(REPO, "tests", "expq_plan_test.cpp")])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and "expq plan ok" in res.stdout, res.stdout


def test_null_context_is_refused(pie):
    lib = pie.load_library()
    q = C.c_size_t(7)
    assert lib.pie_expired_queue_room(None) == PIE_E_INVAL
    assert lib.pie_expired_queue_begin(None, 0, 1, 16) == PIE_E_INVAL
    assert lib.pie_expired_queue_finish(None, None, 0, C.byref(q)) == PIE_E_INVAL
    assert lib.pie_shard_expired_queue_begin(None, 0, 1, 16) == PIE_E_INVAL
    assert lib.pie_shard_expired_queue_finish(None, None, 0, C.byref(q)) == PIE_E_INVAL
    assert lib.pie_expired_inflight_geometry(None, 1000, None, None, None) == PIE_E_INVAL
    assert q.value == 7
