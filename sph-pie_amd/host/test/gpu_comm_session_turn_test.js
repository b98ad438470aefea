'use strict';
// GPU check of the turn that logs in behind the communicator through the addon (commSessionTurn -> pie_comm_session_turn): a
// world-2 communicator on GPU 0 (PIE_RCCL_LIB = the one-GPU stand-in for RCCL) and a single context hold the same synthetic
// table with a key per row.  A short hand-written turn — create, get, touch, delete, get on a new token, around calls on resident
// tokens — must answer over two shards as the unsharded sessionTurn does, and leave the same table behind.
process.env.TZ = 'UTC';
const assert = require('assert');
const pieNative = require('../pieNative');

const SEED = 0x5EED5EEDn, T0 = 1700000000000, HOUR = 3600 * 1000;
const N = 1000, U = 40, D = 8, WORLD = 2;
const MASK = (1n << 64n) - 1n;
const GET = 0, TOUCH = 1, DELETE = 2, CREATE = 3;

function keyOf(r){ return [(BigInt(r + 1) * 0x9E3779B97F4A7C15n) & MASK, (BigInt(r) * 0xD1B54A32D192ED03n + 7n) & MASK]; }

function turn(calls){
  const k = calls.length;
  const t = {keys: new BigUint64Array(2 * k), nows: new BigInt64Array(k), ends: new BigInt64Array(k), kinds: new Uint8Array(k),
             users: new Int32Array(k), discs: new Int32Array(k)};
  calls.forEach((c, i) => {
    [t.keys[2 * i], t.keys[2 * i + 1]] = keyOf(c.tok);
    t.nows[i] = BigInt(c.now);
    t.ends[i] = BigInt(c.end || 0);
    t.kinds[i] = c.kind;
    t.users[i] = c.user || 0;
    t.discs[i] = c.disc || 0;
  });
  return t;
}

function main(){
  const native = pieNative.load();
  const comm = native.commCreate(new Int32Array(WORLD));
  native.commGenSyntheticSharded(comm, SEED, N, U, D, 0);
  const ctx = native.ctxCreate(0);
  native.genSynthetic(ctx, SEED, N, 0, N, U, D, 0);
  const keys = new BigUint64Array(2 * N);
  for(let r = 0; r < N; r++){ [keys[2 * r], keys[2 * r + 1]] = keyOf(r); }
  native.commTokenSet(comm, keys);
  native.tokenSet(ctx, keys);

  const now = T0 - 6 * HOUR, fresh = N + 77, other = N + 78;
  const calls = [
    {tok: 5, now, kind: GET},
    {tok: fresh, now, kind: GET},                                        // not there yet
    {tok: fresh, now, kind: CREATE, end: now + 12 * HOUR, user: 7, disc: 3},
    {tok: fresh, now: now + 1, kind: GET},
    {tok: fresh, now: now + 2, kind: TOUCH, end: now + 24 * HOUR},
    {tok: 6, now, kind: TOUCH, end: now + 24 * HOUR},
    {tok: fresh, now: now + 3, kind: DELETE},
    {tok: fresh, now: now + 4, kind: GET},
    {tok: other, now, kind: CREATE, end: now + HOUR, user: U + 1, disc: 1},   // a user the table has not seen: nUsers grows
    {tok: other, now, kind: GET},
  ];
  const t = turn(calls);
  const got = native.commSessionTurn(comm, t.keys, t.nows, t.ends, t.kinds, t.users, t.discs, U + 2);
  const want = native.sessionTurn(ctx, t.keys, t.nows, t.ends, t.kinds, t.users, t.discs, U + 2);
  assert.deepStrictEqual(Array.from(got.row), [Array.from(want.row)[0], -1, N, N, N, Array.from(want.row)[5], N, N, N + 1, N + 1]);
  for(const col of ['row', 'live', 'end']){ assert.deepStrictEqual(Array.from(got[col]), Array.from(want[col]), col); }
  calls.forEach((c, i) => {
    if(want.row[i] < 0){ assert.strictEqual(got.owner[i], -1); return; }
    assert.strictEqual(got.user[i], want.user[i], 'user of op ' + i);
    assert.strictEqual(got.start[i], want.start[i], 'start of op ' + i);
    assert.ok(got.owner[i] >= 0 && got.owner[i] < WORLD);
  });
  assert.deepStrictEqual(Array.from(got.live), [want.live[0], 0, 1, 1, 1, want.live[5], 0, 0, 1, 1]);
  assert.deepStrictEqual(native.commTableSize(comm), {rows: N + 2, users: U + 2});
  // the next call finds the new rows through every shard's index
  const ask = turn([{tok: fresh, now, kind: GET}, {tok: other, now, kind: GET}, {tok: 6, now, kind: GET}]);
  const after = native.commTokenTurn(comm, ask.keys, ask.nows, ask.ends, ask.kinds);
  const afterOne = native.tokenTurn(ctx, ask.keys, ask.nows, ask.ends, ask.kinds);
  for(const col of ['row', 'live', 'end', 'user', 'start']){ assert.deepStrictEqual(Array.from(after[col]), Array.from(afterOne[col]), col); }
  assert.deepStrictEqual(Array.from(after.row), [N, N + 1, Array.from(want.row)[5]]);
  // refusals: the lengths must agree; the other communicator turn keeps refusing the kind; a bad user changes nothing
  assert.throws(() => native.commSessionTurn(comm, t.keys, t.nows, t.ends, t.kinds, new Int32Array(1), t.discs, U + 2), TypeError);
  assert.throws(() => native.commTokenTurn(comm, t.keys, t.nows, t.ends, t.kinds), e => e.code === -1);
  assert.throws(() => native.commSessionTurn(comm, t.keys, t.nows, t.ends, t.kinds, t.users.map(() => U + 5), t.discs, U + 2), e => e.code === -1);
  assert.deepStrictEqual(native.commTableSize(comm), {rows: N + 2, users: U + 2});
  native.commDestroy(comm);
  native.ctxDestroy(ctx);
  console.log('host gpu_comm_session_turn_test ok');
}

main();
