"""CPU: the communicator's in-flight entries (pie_comm_token_lookup_begin / _finish / _room, pie_comm_expired_queue_begin /
_finish / _room) exist in the header, the binding and the library, and refuse a NULL communicator.  No compute calls here."""
import ctypes as C
import os
import re

from conftest import REPO

ENTRIES = ["pie_comm_token_lookup_begin", "pie_comm_token_lookup_finish", "pie_comm_token_lookup_room",
           "pie_comm_expired_queue_begin", "pie_comm_expired_queue_finish", "pie_comm_expired_queue_room"]
PIE_E_INVAL = -1


def test_entries_in_header_binding_and_library(pie):
    text = open(os.path.join(REPO, "include", "pie_scan.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pie_[a-z_0-9]+)\s*\(", text))
    lib = pie.load_library()
    for name in ENTRIES + ["pie_comm_inflight_queue_device_ptrs"]:
        assert name in declared, name
        assert name in pie.ABI_SYMBOLS, name
        assert getattr(lib, name) is not None, name
    for method in ("token_lookup_begin", "token_lookup_finish", "token_lookup_room", "expired_queue_begin", "expired_queue_finish",
                   "expired_queue_room"):
        assert callable(getattr(pie.PieComm, method)), method
    assert lib.pie_abi_version() == 1


def test_null_communicator_is_refused(pie):
    lib = pie.load_library()
    k = C.c_size_t(7)
    assert lib.pie_comm_token_lookup_begin(None, None, None, 0) == PIE_E_INVAL
    assert lib.pie_comm_token_lookup_finish(None, None, None, None, None, None, None, 0, C.byref(k)) == PIE_E_INVAL
    assert lib.pie_comm_token_lookup_room(None) == PIE_E_INVAL
    assert lib.pie_comm_expired_queue_begin(None, 0, 1, 0) == PIE_E_INVAL
    assert lib.pie_comm_expired_queue_finish(None, None, None, 0, C.byref(k)) == PIE_E_INVAL
    assert lib.pie_comm_expired_queue_room(None) == PIE_E_INVAL
    assert lib.pie_comm_inflight_queue_device_ptrs(None, None, None, None, None) == PIE_E_INVAL
