"""The model the token-index tests compare the device with: a plain dict key -> largest row that carries it, beside numpy copies
of the table's columns.  It follows include/pie_scan.h (pie_token_*): the keys cover a prefix of the rows; of several rows under
one key the largest answers; a row is live iff end > now; tombstoned and expired rows stay findable; compaction keeps the rows
with end > dead_before in order and the keys of the kept covered rows."""
import numpy as np

END_NONE = -(2 ** 63)


def key_of(k):
    return (int(k[0]), int(k[1]))


class TokenModel:
    def __init__(self, start, end, user, disc):
        self.start, self.end = np.array(start, np.int64), np.array(end, np.int64)
        self.user, self.disc = np.array(user, np.int32), np.array(disc, np.int32)
        self.keys = np.zeros((0, 2), np.uint64)
        self.index = {}

    @property
    def covered(self):
        return self.keys.shape[0]

    def _reindex(self):
        self.index = {}
        for row, k in enumerate(self.keys):
            self.index[key_of(k)] = row          # ascending rows: the largest stays

    def token_set(self, keys):
        self.keys = np.array(keys, np.uint64).reshape(-1, 2)
        assert self.covered <= self.start.shape[0]
        self._reindex()

    def token_append(self, keys):
        keys = np.array(keys, np.uint64).reshape(-1, 2)
        assert self.covered + keys.shape[0] <= self.start.shape[0]
        for i, k in enumerate(keys):
            self.index[key_of(k)] = self.covered + i
        self.keys = np.concatenate([self.keys, keys])

    def append_rows(self, start, end, user, disc):
        self.start, self.end = np.concatenate([self.start, np.asarray(start, np.int64)]), np.concatenate([self.end, np.asarray(end, np.int64)])
        self.user, self.disc = np.concatenate([self.user, np.asarray(user, np.int32)]), np.concatenate([self.disc, np.asarray(disc, np.int32)])

    def rows_of(self, keys):
        return np.array([self.index.get(key_of(k), -1) for k in np.asarray(keys, np.uint64).reshape(-1, 2)], np.int32)

    def lookup(self, keys, now):
        row = self.rows_of(keys)
        found = row >= 0
        if self.end.size == 0:                       # no row yet: nothing is found, and there is no row 0 to stand in
            z = np.zeros(row.size, np.int64)
            return {"row": row, "live": z.astype(np.uint8), "user": z.astype(np.int32), "start": z, "end": z.copy(), "found": found}
        safe = np.where(found, row, 0)
        return {"row": row, "live": (found & (self.end[safe] > now)).astype(np.uint8), "user": self.user[safe], "start": self.start[safe],
                "end": self.end[safe], "found": found}

    def token_set_end(self, keys, new_end, now):
        """-> rows_out; the elements qualify against the table as it stood before the call and apply in array order."""
        got = self.lookup(keys, now)
        rows_out = np.where(got["live"] == 1, got["row"], -1).astype(np.int32)
        for r, e in zip(rows_out, np.asarray(new_end, np.int64)):
            if r >= 0:
                self.end[r] = e
        return rows_out

    def compact(self, dead_before=END_NONE):
        """-> new_of_old"""
        keep = self.end > dead_before
        new_of_old = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        self.keys = self.keys[keep[: self.covered]]
        self.start, self.end, self.user, self.disc = self.start[keep], self.end[keep], self.user[keep], self.disc[keep]
        self._reindex()
        return new_of_old


def check_layout(covered, slots, slot_row, keys, homes):
    """The invariants of the index: every covered row sits in exactly one slot, and the walk from its home to its slot (wrapping)
    meets no empty slot.  homes = token_homes(keys, log2(slots))."""
    assert slots == slot_row.shape[0] and slots & (slots - 1) == 0 and keys.shape == (covered, 2)
    held = slot_row[slot_row >= 0]
    assert np.array_equal(np.sort(held), np.arange(covered, dtype=np.int32)), "every covered row in exactly one slot, nothing else"
    slot_of = np.empty(covered, np.int64)
    slot_of[slot_row[slot_row >= 0]] = np.nonzero(slot_row >= 0)[0]
    empty = np.concatenate([[0], np.cumsum(slot_row < 0)])      # empty[s] = empty slots among [0, s)
    h, s = homes.astype(np.int64), slot_of
    straight = s >= h
    between = np.where(straight, empty[s] - empty[h], (empty[slots] - empty[h]) + empty[s])
    assert np.all(between == 0), "an empty slot between a row's home and its slot"
    return slot_of
