"""The executable form of pie_token_turn's rules (include/pie_scan.h): a whole turn — an ordered list of get / touch / delete ops,
each with its own clock — applied one op after another to the dict model of tests/token_model.py.

    GET     live = found and e > now                      end_out = e
    TOUCH   found and e > now: e := new_end, live = 1     end_out = e afterwards
    DELETE  found and e != END_NONE: e := END_NONE        end_out = e afterwards; row = -1 when nothing was written
A get or touch that finds its row expired writes nothing (expired rows stay findable and report live = 0).

Also here: the replay of tests/golden/sessionstore_g5_trace.json in turns (replay_g5), which the CPU test runs on the model alone
and the GPU tests run on the device with the model beside it."""
import hashlib

import numpy as np

from table_model import tombstone
from token_model import END_NONE, TokenModel, key_of

GET, TOUCH, DELETE = 0, 1, 2
TURN_OP = np.dtype([("tok", "<u8", (2,)), ("now", "<i8"), ("new_end", "<i8"), ("kind", "<i4"), ("reserved", "<i4")])


def make_ops(keys, now, kind, new_end=0):
    keys = np.asarray(keys, np.uint64).reshape(-1, 2)
    ops = np.zeros(keys.shape[0], TURN_OP)
    ops["tok"], ops["now"], ops["kind"], ops["new_end"] = keys, now, kind, new_end
    return ops


class TurnModel(TokenModel):
    def turn(self, ops):
        k = ops.shape[0]
        out = {"row": np.full(k, -1, np.int32), "live": np.zeros(k, np.uint8), "user": np.full(k, -1, np.int32),
               "start": np.zeros(k, np.int64), "end": np.full(k, END_NONE, np.int64), "found": np.zeros(k, bool)}
        for i, op in enumerate(ops):
            row = self.index.get(key_of(op["tok"]), -1)
            if row < 0:
                continue
            now, kind = int(op["now"]), int(op["kind"])
            e = int(self.end[row])
            out["found"][i], out["row"][i], out["user"][i], out["start"][i] = True, row, self.user[row], self.start[row]
            if kind == GET:
                out["live"][i] = e > now
            elif kind == TOUCH:
                if e > now:
                    e = int(op["new_end"])
                    out["live"][i] = 1
            elif kind == DELETE:
                if e != END_NONE:
                    e = END_NONE
                else:
                    out["row"][i] = -1
            else:
                raise AssertionError("unknown kind")
            self.end[row] = e
            out["end"][i] = e
        return out

    def delete_user(self, u):
        """-> the rows tombstoned, ascending (tests/table_model.py's rule; an id no row carries matches nothing)"""
        return tombstone(self.end, self.user == u)

    def purge(self, now):
        """purgeExpiredSessions: every row with end <= now that is not a tombstone -> tombstone; -> those rows"""
        rows = np.nonzero((self.end <= now) & (self.end != END_NONE))[0]
        self.end[rows] = END_NONE
        return rows


def same_turn(got, want, tag=""):
    """device (or any) answers == the model's: row and live and end everywhere, user and start where the key was found"""
    for col in ("row", "live", "end"):
        assert np.array_equal(got[col], want[col]), (tag, col, np.nonzero(got[col] != want[col])[0][:8])
    f = want["found"]
    for col in ("user", "start"):
        assert np.array_equal(got[col][f], want[col][f]), (tag, col)


def g5_key(tok):
    """the key of the trace's token number `tok`: the first 16 bytes of a sha256, as the host derives keys from real tokens"""
    return np.frombuffer(hashlib.sha256(b"g5-token-%d" % tok).digest()[:16], dtype="<u8").astype(np.uint64)


class ModelStore:
    """the store replay_g5 drives, on the model alone"""

    def __init__(self, n_users):
        z64, z32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
        self.m = TurnModel(z64, z64, z32, z32)
        self.U = n_users

    def create(self, start, end, user, key):
        self.m.append_rows([start], [end], [user], [0])
        self.m.token_append(key.reshape(1, 2))

    def turn(self, ops):
        return self.m.turn(ops)

    def delete_user(self, u):
        self.m.delete_user(u)

    def purge(self, now):
        self.m.purge(now)


def replay_g5(trace, store, chunk):
    """Replays the trace with every maximal run of get / touch / del calls cut into turns of at most `chunk` ops (None: the whole
    run is one turn); a census is a run of gets, one per token issued, in issue order.  Every recorded result and every census
    is compared.  -> (answers compared, turns issued, largest turn)"""
    ttl, names = trace["ttl_ms"], trace["users"]
    users = {name: i for i, name in enumerate(names)}
    issued, checked, turns, largest = 0, 0, 0, 0
    run = []

    def answers(ops_list):
        nonlocal turns, largest
        ops = np.zeros(len(ops_list), TURN_OP)
        for i, (kind, tok, now) in enumerate(ops_list):
            ops[i]["tok"], ops[i]["now"], ops[i]["kind"] = g5_key(tok), now, kind
            ops[i]["new_end"] = now + ttl if kind == TOUCH else 0
        step = len(ops_list) if chunk is None else chunk
        parts = [store.turn(ops[at:at + step]) for at in range(0, len(ops_list), step)]
        turns += len(parts)
        largest = max([largest] + [p["row"].shape[0] for p in parts])
        return {col: np.concatenate([p[col] for p in parts]) for col in ("row", "live", "user", "start", "end")}

    def flush():
        nonlocal checked
        if not run:
            return
        got = answers([(kind, op["tok"], op["now"]) for kind, op in run])
        for i, (kind, op) in enumerate(run):
            live = bool(got["live"][i])
            if kind == GET:
                res = {"userId": names[got["user"][i]], "createdAt": int(got["start"][i]), "expiresAt": int(got["end"][i])} if live else None
                assert res == op["result"], (op, res)
            elif kind == TOUCH:
                res = {"userId": names[got["user"][i]], "expiresAt": int(got["end"][i])} if live else None
                assert res == op["result"], (op, res)
            checked += 1
        run.clear()

    for op in trace["ops"]:
        kind, now = op["op"], op["now"]
        if kind in ("get", "touch", "del"):
            run.append(({"get": GET, "touch": TOUCH, "del": DELETE}[kind], op))
            continue
        flush()
        if kind == "create":
            assert now + ttl == op["expiresAt"]
            store.create(now, now + ttl, users[op["user"]], g5_key(issued))
            issued += 1
        elif kind == "delUser":
            if op["user"] in users:           # '' and unknown ids match nothing
                store.delete_user(users[op["user"]])
        elif kind == "purge":
            store.purge(now)
        elif kind == "census":
            got = answers([(GET, tok, now) for tok in range(issued)]) if issued else {"live": np.zeros(0, np.uint8)}
            assert np.nonzero(got["live"])[0].tolist() == op["live"], (now, op["live"])
        else:
            raise AssertionError("unknown op " + kind)
        checked += 1
    flush()
    return checked, turns, largest
