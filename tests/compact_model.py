"""TEST INFRASTRUCTURE — pie_compact_rows restated in numpy on top of tests/table_model.TableModel.

Keep is `end > dead_before`, in table order; users are not renumbered.  The maps are the two directions of the renumbering:
new_of_old[n_old] (-1 = dropped) and old_of_new[n_kept] (ascending).  push_result() carries a scan result of the old table
through new_of_old: what the compacted table must answer for the same query when no selected row was dropped."""
import numpy as np

from table_model import TableModel

INT64_MIN = -(2 ** 63)


def compact_maps(end, dead_before):
    """-> (new_of_old int32[n], old_of_new int32[k]) of keeping the rows with end > dead_before, order preserved."""
    end = np.asarray(end, np.int64)
    keep = end > np.int64(dead_before)
    old_of_new = np.nonzero(keep)[0].astype(np.int32)
    new_of_old = np.full(end.size, -1, np.int32)
    new_of_old[old_of_new] = np.arange(old_of_new.size, dtype=np.int32)
    return new_of_old, old_of_new


def translate(new_of_old, rows):
    """pie_compact_translate: old rows -> new rows; -1 for dropped rows and for indices outside [0, n_old)."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    out = np.full(rows.size, -1, np.int32)
    ok = (rows >= 0) & (rows < new_of_old.size)
    out[ok] = new_of_old[rows[ok]]
    return out


def push_result(result, new_of_old):
    """(counts, offsets, idx) of the old table -> the same feeds with the rows renumbered and the dropped rows removed
    (order inside a feed unchanged: the renumbering is monotonic, so (start asc, row asc) survives it)."""
    counts, offsets, idx = result
    new_idx = new_of_old[idx]
    keep = new_idx >= 0
    csum = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    new_off = csum[offsets]
    return np.diff(new_off).astype(np.int32), new_off, new_idx[keep].astype(np.int32)


class CompactModel(TableModel):
    """TableModel + compact_rows.  global_rows follows a sharded table's local row -> global row map through compactions."""

    def __init__(self, oracle):
        super().__init__(oracle)
        self.global_rows = None

    def shard_table(self, rank, world):
        _, rows = self.shard_rows(rank, world)
        self.global_rows = np.asarray(rows, np.int64).astype(np.int32)
        return super().shard_table(rank, world)

    def compact_rows(self, dead_before=INT64_MIN):
        new_of_old, old_of_new = compact_maps(self.end, dead_before)
        self.start, self.end = self.start[old_of_new], self.end[old_of_new]
        self.user, self.disc = self.user[old_of_new], self.disc[old_of_new]
        if self.global_rows is not None:
            self.global_rows = self.global_rows[old_of_new[old_of_new < self.global_rows.size]]
        return new_of_old, old_of_new
