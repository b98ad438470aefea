"""The executable form of pie_session_turn's rules (include/pie_scan.h): a turn whose ops may log in.  GET, TOUCH and DELETE are
tests/turn_model.py's; a CREATE is, by definition, pie_append_rows of one row (start = now, end = new_end, user[i], disc[i])
followed by pie_token_append of its key, applied where the op stands in the array:

    CREATE  row = the new row   live = new_end > now   end_out = new_end   start_out = now   user_out = user[i]
From that op on the key's row is the new row (the largest row under a key answers).

Also here: the replay of tests/golden/sessionstore_g5_trace.json with the `create` calls INSIDE the turns (replay_g5_sessions):
only delUser, purge and census cut a run."""
import numpy as np

from turn_model import DELETE, GET, TOUCH, TURN_OP, TurnModel, g5_key

CREATE = 3


class SessionTurnModel(TurnModel):
    def turn(self, ops, user=None, disc=None):
        k = ops.shape[0]
        out = {"row": np.full(k, -1, np.int32), "live": np.zeros(k, np.uint8), "user": np.full(k, -1, np.int32),
               "start": np.zeros(k, np.int64), "end": np.full(k, -(2 ** 63), np.int64), "found": np.zeros(k, bool)}
        at = 0
        while at < k:                              # runs of other ops go through TurnModel.turn, one op after another
            if int(ops[at]["kind"]) != CREATE:
                to = at
                while to < k and int(ops[to]["kind"]) != CREATE:
                    to += 1
                part = TurnModel.turn(self, ops[at:to])
                for col in out:
                    out[col][at:to] = part[col]
                at = to
                continue
            op = ops[at]
            assert self.covered == self.start.shape[0], "the column is a prefix: a create needs it to cover every row"
            now, new_end = int(op["now"]), int(op["new_end"])
            self.append_rows([now], [new_end], [user[at]], [disc[at]])
            self.token_append(np.asarray(op["tok"], np.uint64).reshape(1, 2))
            out["found"][at], out["row"][at], out["live"][at] = True, self.start.shape[0] - 1, new_end > now
            out["user"][at], out["start"][at], out["end"][at] = user[at], now, new_end
            at += 1
        return out


class SessionModelStore:
    """the store replay_g5_sessions drives, on the model alone"""

    def __init__(self, n_users):
        z64, z32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
        self.m = SessionTurnModel(z64, z64, z32, z32)
        self.U = n_users

    def turn(self, ops, user, disc):
        return self.m.turn(ops, user, disc)

    def delete_user(self, u):
        self.m.delete_user(u)

    def purge(self, now):
        self.m.purge(now)


def replay_g5_sessions(trace, store, chunk):
    """tests/turn_model.py's replay_g5 with the logins in the runs: every maximal run of create / get / touch / del calls is cut
    into turns of at most `chunk` ops (None: the whole run is one turn) and goes through store.turn(ops, user, disc).  Every
    recorded result — a create's expiresAt included — and every census is compared.
    -> (answers compared, turns issued, largest turn, creates that shared a turn with another op)"""
    ttl, names = trace["ttl_ms"], trace["users"]
    users = {name: i for i, name in enumerate(names)}
    issued, checked, turns, largest, mixed = 0, 0, 0, 0, 0
    run = []

    def answers(ops_list):
        nonlocal turns, largest, mixed
        k = len(ops_list)
        ops, user, disc = np.zeros(k, TURN_OP), np.zeros(k, np.int32), np.zeros(k, np.int32)
        for i, (kind, tok, now, u) in enumerate(ops_list):
            ops[i]["tok"], ops[i]["now"], ops[i]["kind"] = g5_key(tok), now, kind
            ops[i]["new_end"] = now + ttl if kind in (TOUCH, CREATE) else 0
            user[i] = u
        step = k if chunk is None else chunk
        parts = []
        for at in range(0, k, step):
            part = ops[at:at + step]
            parts.append(store.turn(part, user[at:at + step], disc[at:at + step]))
            n_create = int(np.count_nonzero(part["kind"] == CREATE))
            mixed += n_create if part.shape[0] > 1 else 0
        turns += len(parts)
        largest = max([largest] + [p["row"].shape[0] for p in parts])
        return {col: np.concatenate([p[col] for p in parts]) for col in ("row", "live", "user", "start", "end")}

    def flush():
        nonlocal checked
        if not run:
            return
        got = answers([(kind, tok, op["now"], u) for kind, tok, op, u in run])
        for i, (kind, tok, op, u) in enumerate(run):
            live = bool(got["live"][i])
            if kind == GET:
                res = {"userId": names[got["user"][i]], "createdAt": int(got["start"][i]), "expiresAt": int(got["end"][i])} if live else None
                assert res == op["result"], (op, res)
            elif kind == TOUCH:
                res = {"userId": names[got["user"][i]], "expiresAt": int(got["end"][i])} if live else None
                assert res == op["result"], (op, res)
            elif kind == CREATE:
                assert live and int(got["end"][i]) == op["expiresAt"] and int(got["start"][i]) == op["now"] and got["user"][i] == u, (op, i)
                assert got["row"][i] == tok, "sessions get rows in issue order"
            checked += 1
        run.clear()

    for op in trace["ops"]:
        kind, now = op["op"], op["now"]
        if kind in ("get", "touch", "del"):
            run.append(({"get": GET, "touch": TOUCH, "del": DELETE}[kind], op["tok"], op, 0))
            continue
        if kind == "create":
            assert now + ttl == op["expiresAt"]
            run.append((CREATE, issued, op, users[op["user"]]))
            issued += 1
            continue
        flush()
        if kind == "delUser":
            if op["user"] in users:           # '' and unknown ids match nothing
                store.delete_user(users[op["user"]])
        elif kind == "purge":
            store.purge(now)
        elif kind == "census":
            got = answers([(GET, tok, now, 0) for tok in range(issued)]) if issued else {"live": np.zeros(0, np.uint8)}
            assert np.nonzero(got["live"])[0].tolist() == op["live"], (now, op["live"])
        else:
            raise AssertionError("unknown op " + kind)
        checked += 1
    flush()
    return checked, turns, largest, mixed
