"""The model of the sharded token column (include/pie_scan.h, pie_shard_token_* / pie_comm_token_*): the unsharded TokenModel of
tests/token_model.py, the owning rank of every user, and per rank the global rows that rank's own compactions dropped.  Shard r
answers key q with the largest global row that carries q, belongs to a user r owns, was not dropped by r and lies below
covered_g; merging the shards' answers by largest global row gives the unsharded table's answer."""
import numpy as np

from token_model import END_NONE, TokenModel, key_of


class ShardTokenModel:
    def __init__(self, start, end, user, disc, owner, world):
        self.tm = TokenModel(start, end, user, disc)
        self.owner = np.array(owner, np.int32)            # owner[global user] = rank
        self.world = int(world)
        self.dropped = [np.zeros(self.N, bool) for _ in range(self.world)]

    @property
    def N(self):
        return self.tm.start.shape[0]

    @property
    def covered_g(self):
        return self.tm.covered

    def append_rows(self, start, end, user, disc, owner_of_new_users=()):
        self.owner = np.concatenate([self.owner, np.array(owner_of_new_users, np.int32)])
        self.tm.append_rows(start, end, user, disc)
        k = self.N - self.dropped[0].shape[0]
        self.dropped = [np.concatenate([x, np.zeros(k, bool)]) for x in self.dropped]

    def token_set(self, keys):
        self.tm.token_set(keys)

    def token_append(self, keys):
        self.tm.token_append(keys)

    def held(self, rank):
        """ascending global rows shard `rank` holds"""
        return np.nonzero((self.owner[self.tm.user] == rank) & ~self.dropped[rank])[0].astype(np.int32)

    def covered_l(self, rank):
        return int(np.count_nonzero(self.held(rank) < self.covered_g))

    def shard_keys(self, rank):
        """the keys of the shard's covered local rows, in local order"""
        rows = self.held(rank)
        return self.tm.keys[rows[rows < self.covered_g]]

    def shard_lookup(self, rank, keys, now):
        rows = self.held(rank)
        index = {}
        for g in rows[rows < self.covered_g].tolist():
            index[key_of(self.tm.keys[g])] = g            # ascending: the largest stays
        row = np.array([index.get(key_of(k), -1) for k in np.asarray(keys, np.uint64).reshape(-1, 2)], np.int32)
        return self._answer(row, now)

    def _answer(self, row, now):
        tm = self.tm
        found = row >= 0
        safe = np.where(found, row, 0)
        return {"row": row, "live": (found & (tm.end[safe] > now)).astype(np.uint8), "user": tm.user[safe], "start": tm.start[safe],
                "end": tm.end[safe], "found": found}

    def shard_set_end(self, keys, new_end, now):
        """Every shard is given the same call -> rows_global_out per rank.  A shard's elements qualify against its rows as they
        stood before the call and apply in array order; the shards' rows are disjoint."""
        outs = [np.where(got["live"] == 1, got["row"], -1).astype(np.int32)
                for got in (self.shard_lookup(r, keys, now) for r in range(self.world))]
        for rows_out in outs:
            for g, e in zip(rows_out, np.asarray(new_end, np.int64)):
                if g >= 0:
                    self.tm.end[g] = e
        return outs

    def compact(self, rank, dead_before=END_NONE):
        """pie_compact_rows on ONE shard: it drops its own rows with end <= dead_before; global ids stay.  -> rows it holds now"""
        mine = self.owner[self.tm.user] == rank
        self.dropped[rank] |= mine & (self.tm.end <= dead_before)
        return self.held(rank)

    def merged_lookup(self, keys, now):
        return merge([self.shard_lookup(r, keys, now) for r in range(self.world)])


def merge(answers):
    """Per key the answer with the largest global row (row -1, live 0, owner -1 if no shard holds it); answers[r] is rank r's."""
    k = answers[0]["row"].shape[0]
    out = {"row": np.full(k, -1, np.int32), "live": np.zeros(k, np.uint8), "user": np.full(k, -1, np.int32),
           "start": np.zeros(k, np.int64), "end": np.zeros(k, np.int64), "owner": np.full(k, -1, np.int32)}
    for r, a in enumerate(answers):
        better = a["row"] > out["row"]
        for col in ("row", "live", "user", "start", "end"):
            out[col][better] = a[col][better]
        out["owner"][better] = r
    out["found"] = out["row"] >= 0
    return out
