'use strict';
// GPU check of the live sharded table through the addon: a world-3 communicator on GPU 0 (PIE_RCCL_LIB = the one-GPU stand-in
// for RCCL) and a single context hold the same synthetic table.  Logins (commAppendRows, new users among them), touches and
// deletes by global row (commSetEnd) and a user's deletion (commDeleteUser) go to the shards by GLOBAL id and to the single
// context by row; afterwards commExpiredQueue must give the single context's expired queues, element for element.
process.env.TZ = 'UTC';
const assert = require('assert');
const pieNative = require('../pieNative');

const SEED = 0x5EED5EEDn, T0 = 1700000000000, SPAN = 10368000000, TTL = 43200000, TOP = T0 + SPAN;
const END_NONE = -(2n ** 63n);
const N = 20000, U = 300, D = 32, WORLD = 3;

let state = 12345;
function rnd(n){ state = (state * 1103515245 + 12345) % 2147483648; return state % n; }

function main(){
  const native = pieNative.load();
  const comm = native.commCreate(new Int32Array(WORLD));
  native.commGenSyntheticSharded(comm, SEED, N, U, D, 0);
  const ctx = native.ctxCreate(0);
  native.genSynthetic(ctx, SEED, N, 0, N, U, D, 0);
  let rows = N, users = U, checks = 0, clock = 0;
  assert.deepStrictEqual(native.commTableSize(comm), {rows, users});

  const login = (k, newUsers) => {
    clock++;
    const nUsers = users + newUsers;
    const s = new BigInt64Array(k), e = new BigInt64Array(k), u = new Int32Array(k), d = new Int32Array(k);
    for(let i = 0; i < k; i++){
      s[i] = BigInt(TOP + clock * 100000 + i);
      e[i] = s[i] + BigInt(TTL / 4 + rnd(TTL / 2));
      u[i] = i < newUsers ? users + i : rnd(nUsers);
      d[i] = rnd(D);
    }
    assert.strictEqual(native.commAppendRows(comm, s, e, u, d, nUsers), rows);
    native.appendRows(ctx, s, e, u, d, nUsers);
    rows += k; users = nUsers;
    assert.deepStrictEqual(native.commTableSize(comm), {rows, users});
  };
  const touch = (k, recent) => {
    const r = new Int32Array(k), v = new BigInt64Array(k);
    for(let i = 0; i < k; i++){
      r[i] = i < recent ? rows - 1 - i : rnd(rows);
      v[i] = rnd(5) === 0 ? END_NONE : BigInt(TOP - TTL + rnd(2 * TTL));
    }
    r[k - 1] = r[0];   // a repeat: the last value wins on both sides
    assert.strictEqual(native.commSetEnd(comm, r, v), k);
    native.setEnd(ctx, r, v);
  };
  const remove = (user) => {
    const a = new Int32Array(rows), b = new Int32Array(rows);
    const got = native.commDeleteUser(comm, user, a);
    const want = user >= 0 && user < users ? native.deleteUser(ctx, user, b) : 0;
    assert.strictEqual(got.deleted, want);
    assert.deepStrictEqual(Array.from(a.subarray(0, want)), Array.from(b.subarray(0, want)));
    assert.strictEqual(got.owner >= 0 && got.owner < WORLD, user >= 0 && user < users);
    checks++;
  };
  const queues = () => {
    const a = new Int32Array(rows), b = new Int32Array(rows);
    let nonEmpty = 0;
    for(const [prev, now] of [[END_NONE, BigInt(TOP + 2 * TTL)], [TOP - TTL, TOP], [TOP, TOP + TTL], [TOP - 5, TOP - 5]]){
      const q = native.commExpiredQueue(comm, prev, now, a), w = native.expiredQueue(ctx, prev, now, b);
      assert.strictEqual(q, w);
      assert.deepStrictEqual(Array.from(a.subarray(0, q)), Array.from(b.subarray(0, w)));
      nonEmpty += w > 0 ? 1 : 0;
      checks++;
    }
    assert(nonEmpty >= 3, 'too few non-empty queues');
  };

  login(65, 3);
  touch(257, 65);
  login(1, 0);
  login(4096, 37);
  touch(3000, 500);
  remove(17); remove(users - 1); remove(users); remove(-1);
  queues();
  login(40000, 1);   // outgrows every shard's capacity
  touch(3000, 3000);
  queues();
  // a refused call throws with the library's code and changes nothing
  const one = new Int32Array([rows]), val = new BigInt64Array([BigInt(TOP)]);
  assert.throws(() => native.commSetEnd(comm, one, val), err => err.code === -1);
  assert.throws(() => native.commAppendRows(comm, val, val, new Int32Array([users]), new Int32Array([0]), users), err => err.code === -1);
  assert.deepStrictEqual(native.commTableSize(comm), {rows, users});
  queues();
  native.commDestroy(comm);
  native.ctxDestroy(ctx);
  console.log('host comm_mutate_test ok: ' + checks + ' checks');
}

main();
