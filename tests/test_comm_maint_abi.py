"""CPU: the entries that let a sharded table age (pie_shard_prune_before, pie_shard_retention_purge / _tz, pie_comm_prune_before,
pie_comm_retention_purge / _tz, pie_comm_compact_rows, pie_comm_queue_kind) exist in the header, the binding and the library with
the header's signatures, refuse a NULL handle, and cannot be reached without a device.  No compute calls here."""
import ctypes as C
import os
import re

import pytest

from conftest import REPO

ENTRIES = ["pie_shard_prune_before", "pie_shard_retention_purge", "pie_shard_retention_purge_tz", "pie_comm_prune_before",
           "pie_comm_retention_purge", "pie_comm_retention_purge_tz", "pie_comm_compact_rows", "pie_comm_queue_kind"]
PIE_E_INVAL, PIE_E_NODEVICE = -1, -2
SCALARS = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "size_t": C.c_size_t}


def header_text():
    text = open(os.path.join(REPO, "include", "pie_scan.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_entries_in_header_binding_and_library(pie):
    declared = set(re.findall(r"\b(pie_[a-z_0-9]+)\s*\(", header_text()))
    lib = pie.load_library()
    for name in ENTRIES:
        assert name in declared, name
        assert name in pie.ABI_SYMBOLS, name
        assert getattr(lib, name) is not None, name
    for method in ("shard_prune_before", "shard_retention_purge"):
        assert callable(getattr(pie.PieScan, method)), method
    for method in ("prune_before", "retention_purge", "compact_rows", "queue_kind"):
        assert callable(getattr(pie.PieComm, method)), method
    assert lib.pie_abi_version() == 1


def test_binding_signatures_are_the_headers(pie):
    from sph_pie_amd import binding
    sigs = {s[0]: s for s in binding._SIGS}
    text = header_text()
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        _, restype, argtypes = sigs[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        for p, a in zip(params, argtypes):
            if "*" in p:
                assert a is binding._P or issubclass(a, C._Pointer), (name, p)
            else:
                assert a is SCALARS[p.split()[0]], (name, p)


def test_null_handles_are_refused(pie):
    lib = pie.load_library()
    k = C.c_size_t(7)
    off = (C.c_int64 * 1)(0)
    assert lib.pie_shard_prune_before(None, 0, None, 0, C.byref(k)) == PIE_E_INVAL
    assert lib.pie_shard_retention_purge(None, 0, 2, 0, None, 0, C.byref(k)) == PIE_E_INVAL
    assert lib.pie_shard_retention_purge_tz(None, 0, 2, None, off, 0, None, 0, C.byref(k)) == PIE_E_INVAL
    assert lib.pie_comm_prune_before(None, 0, None, 0, C.byref(k)) == PIE_E_INVAL
    assert lib.pie_comm_retention_purge(None, 0, 2, 0, None, 0, C.byref(k)) == PIE_E_INVAL
    assert lib.pie_comm_retention_purge_tz(None, 0, 2, None, off, 0, None, 0, C.byref(k)) == PIE_E_INVAL
    assert lib.pie_comm_compact_rows(None, 0, 0, C.byref(k), None) == PIE_E_INVAL
    assert lib.pie_comm_queue_kind(None) == 0
    assert k.value == 7   # nothing is written through a refused call's outputs


def test_no_device_no_handle(pie):
    """Without a device no context and no communicator exist to call these on: their creation reports PIE_E_NODEVICE."""
    lib = pie.load_library()
    if lib.pie_device_count() > 0:
        pytest.skip("a GPU is present")
    for make in (lambda: pie.PieScan(0), lambda: pie.PieComm([0])):
        with pytest.raises(pie.PieError) as ei:
            make()
        assert ei.value.code == PIE_E_NODEVICE
