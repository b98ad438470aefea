"""CPU: the compaction entry points exist in the library, the header and the binding, and tests/compact_model.py restates
pie_compact_rows correctly on a hand-worked table.  No compute calls on the device."""
import numpy as np

import compact_model as CM
from table_model import ALL, INT64_MIN

COMPACT_SYMBOLS = ("pie_compact_rows", "pie_compact_maps", "pie_compact_map_device_ptrs", "pie_compact_translate")


def test_library_exports_the_compaction_symbols(pie):
    lib = pie.load_library()
    for name in COMPACT_SYMBOLS:
        assert getattr(lib, name) is not None


def test_binding_has_the_compaction_methods(pie):
    for name in ("compact_rows", "compact_maps", "compact_translate"):
        assert callable(getattr(pie.PieScan, name, None)), name
    fields = [k for k, _ in pie.binding.PieTableInfo._fields_]
    assert "compact_bytes" in fields and "compactions" in fields
    assert fields.index("compact_bytes") > fields.index("hot_builds"), "the new fields go at the end of pie_table_info"


def test_abi_symbols_hold_the_names(pie):
    for name in COMPACT_SYMBOLS:
        assert name in pie.ABI_SYMBOLS


# The hand-worked table.  T = 1000 is dead_before.  Rows, in table order:
#   row  start  end        user  kept at dead_before = T?          kept at dead_before = INT64_MIN (tombstones only)?
#    0    50    2000        0    yes                               yes
#    1    50    INT64_MIN   1    no  (tombstone)                   no
#    2    50    1000        0    no  (end == dead_before)          yes
#    3    50    1001        0    yes (end == dead_before + 1)      yes
#    4    70    INT64_MIN   2    no  (user 2 loses all its rows)   no
#    5    70    999         2    no  (user 2 loses all its rows)   yes
#    6    50    5000        0    yes                               yes
#    7    60    3000        3    yes                               yes
#    8    60    3000        3    yes (tie with row 7 on start)     yes
#    9    60    INT64_MIN   3    no                                no
#   10    60    3000        3    yes (tie with rows 7, 8)          yes
#   11    50    INT64_MAX   1    yes                               yes
T = 1000
START = [50, 50, 50, 50, 70, 70, 50, 60, 60, 60, 60, 50]
END = [2000, INT64_MIN, 1000, 1001, INT64_MIN, 999, 5000, 3000, 3000, INT64_MIN, 3000, 2 ** 63 - 1]
USER = [0, 1, 0, 0, 2, 2, 0, 3, 3, 3, 3, 1]
DISC = [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3]


def hand_model(oracle):
    m = CM.CompactModel(oracle)
    m.load(START, END, USER, DISC, 4, 4)
    return m


def test_model_on_the_hand_worked_table(oracle):
    m = hand_model(oracle)
    before = m.scan(INT64_MIN, INT64_MIN, ALL)
    # user 0's feed before: rows 0, 2, 3, 6 (equal starts: row order); user 3's: 7, 8, 10
    assert before[2].tolist() == [0, 2, 3, 6, 11, 5, 7, 8, 10]
    new_of_old, old_of_new = m.compact_rows(T)
    assert new_of_old.tolist() == [0, -1, -1, 1, -1, -1, 2, 3, 4, -1, 5, 6]
    assert old_of_new.tolist() == [0, 3, 6, 7, 8, 10, 11]
    assert new_of_old.dtype == np.int32 and old_of_new.dtype == np.int32
    assert m.start.tolist() == [50, 50, 50, 60, 60, 60, 50]
    assert m.end.tolist() == [2000, 1001, 5000, 3000, 3000, 3000, 2 ** 63 - 1]
    assert m.user.tolist() == [0, 0, 0, 3, 3, 3, 1] and m.U == 4, "users are not renumbered; user 2 is simply empty now"
    assert m.disc.tolist() == [0, 3, 2, 3, 0, 2, 3]
    after = m.scan(INT64_MIN, INT64_MIN, ALL)
    assert after[0].tolist() == [3, 1, 0, 3]
    assert after[2].tolist() == [0, 1, 2, 6, 3, 4, 5], "the equal-start rows of users 0 and 3 keep their relative order"
    for a, b in zip(after, CM.push_result(before, new_of_old)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert CM.translate(new_of_old, [0, 1, 11, 12, -1, 2 ** 31 - 1]).tolist() == [0, -1, 6, -1, -1, -1]


def test_model_tombstones_only_and_composition(oracle):
    m = hand_model(oracle)
    n1, o1 = m.compact_rows()       # dead_before = INT64_MIN: tombstones only
    assert o1.tolist() == [0, 2, 3, 5, 6, 7, 8, 10, 11] and m.n == 9
    n2, o2 = m.compact_rows(T)      # then the expired ones: together the same as one compaction at T
    direct_new, direct_old = CM.compact_maps(np.array(END, np.int64), T)
    assert np.array_equal(o1[o2], direct_old)
    assert np.array_equal(CM.translate(n2, n1), direct_new)
    n3, o3 = m.compact_rows(T)      # nothing left to drop: identity
    assert np.array_equal(n3, np.arange(m.n)) and np.array_equal(o3, np.arange(m.n))
    n4, o4 = m.compact_rows(2 ** 63 - 1)   # nothing is greater than INT64_MAX: every row goes
    assert m.n == 0 and o4.size == 0 and np.all(n4 == -1)
