"""CPU: the five entry points of the in-flight token lookup are declared in include/pie_scan.h, and the binding declares each
with as many arguments as the header.  No compute calls here."""
import os
import re

from conftest import REPO

ENTRY_POINTS = ("pie_token_lookup_begin", "pie_token_lookup_finish", "pie_token_lookup_room", "pie_shard_token_lookup_begin",
                "pie_shard_token_lookup_finish")


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
    assert {n: protos.get(n) for n in ENTRY_POINTS} == {"pie_token_lookup_begin": 4, "pie_token_lookup_finish": 8, "pie_token_lookup_room": 1,
                                                        "pie_shard_token_lookup_begin": 4, "pie_shard_token_lookup_finish": 8}


def test_binding_declares_them_with_matching_argument_counts(pie):
    from sph_pie_amd import binding
    protos = header_prototypes()
    sigs = {name: (res, args) for name, res, args in binding._SIGS}
    for name in ENTRY_POINTS:
        assert name in pie.ABI_SYMBOLS and name in sigs, name
        assert len(sigs[name][1]) == protos[name], name
    lib = pie.load_library()
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None
    for method in ("token_lookup_begin", "token_lookup_finish", "token_lookup_room", "shard_token_lookup_begin", "shard_token_lookup_finish"):
        assert callable(getattr(pie.PieScan, method))
