'use strict';
// GPU check of deleteSessionsForUsers (host/sessionStore.js over native.deleteUsers): a store with a few hundred sessions over 20
// users, one call with known, unknown, falsy and repeated ids; afterwards getSession is null for every token of the named users
// and unchanged for the rest, and a second store deleted id by id (deleteSessionsForUser) agrees.  Then native.deleteUsers with
// per-user counts, and commDeleteUsers once on a two-shard communicator (PIE_RCCL_LIB = the one-GPU stand-in for RCCL).
process.env.TZ = 'UTC';
const assert = require('assert');
const {createStore} = require('../sessionStore');

const N = 400, U = 20;
const realNow = Date.now;
let fakeNow = 1760000000000;
Date.now = () => fakeNow;

function fill(store){
  const made = [];
  for(let i = 0; i < N; i++){
    fakeNow += 1000;
    const userId = 'user-' + ((i * 7) % U);
    made.push({token: store.createSession(userId).token, userId});
  }
  return made;
}

function main(){
  const a = createStore(), b = createStore();
  const ta = fill(a);
  fakeNow = 1760000000000;
  const tb = fill(b);
  const named = ['user-3', 'nobody', '', null, 'user-11', 'user-3', undefined, 0, 'user-19', 'ghost', 'user-11'];
  const gone = new Set(['user-3', 'user-11', 'user-19']);
  const before = ta.map(s => a.getSession(s.token));
  assert.ok(before.every(s => s !== null));
  const gen = a.generation();
  const k = a.deleteSessionsForUsers(named);
  assert.strictEqual(k, ta.filter(s => gone.has(s.userId)).length);
  assert.ok(k > 0 && a.generation() > gen);
  for(const id of named){ b.deleteSessionsForUser(id); }
  ta.forEach((s, i) => {
    const got = a.getSession(s.token), twin = b.getSession(tb[i].token);
    if(gone.has(s.userId)){
      assert.strictEqual(got, null, 'session ' + i + ' of ' + s.userId + ' survived');
      assert.strictEqual(twin, null);
    } else {
      assert.deepStrictEqual(got, before[i], 'session ' + i + ' changed');
      assert.notStrictEqual(twin, null);
    }
  });
  assert.strictEqual(a.size(), b.size());
  assert.strictEqual(a.deleteSessionsForUsers(named), 0);            // a second call finds nothing
  assert.strictEqual(a.deleteSessionsForUsers(['ghost', '', null]), 0);
  assert.strictEqual(a.deleteSessionsForUsers([]), 0);
  // the device agrees: a scan of everything still live returns the survivors of both stores alike
  const ra = a.scanFeeds({now: fakeNow}), rb = b.scanFeeds({now: fakeNow});
  assert.deepStrictEqual(Array.from(ra.idx).sort((x, y) => x - y), Array.from(rb.idx).sort((x, y) => x - y));
  assert.strictEqual(ra.idx.length, N - k);

  // the addon call itself, with per-user counts: a repeated id counts once, an id outside the table nothing
  const native = a.native;
  const u4 = a.userIndexOf('user-4'), u5 = a.userIndexOf('user-5');
  const list = new Int32Array(N), per = new Int32Array(5);
  const want4 = ta.filter(s => s.userId === 'user-4').length, want5 = ta.filter(s => s.userId === 'user-5').length;
  a.flush();
  const k2 = native.deleteUsers(a.ctx, Int32Array.from([u5, -1, u4, u5, 1000]), list, per);
  assert.strictEqual(k2, want4 + want5);
  assert.deepStrictEqual(Array.from(per), [want5, 0, want4, 0, 0]);
  for(let i = 1; i < k2; i++){ assert.ok(list[i] > list[i - 1]); }
  assert.throws(() => native.deleteUsers(a.ctx, Int32Array.from([a.userIndexOf('user-6')]), new Int32Array(1)), e => e.code === -5);
  assert.throws(() => native.deleteUsers(a.ctx, [1, 2], list), TypeError);
  assert.strictEqual(native.deleteUsers(a.ctx, new Int32Array(0), list), 0);
  a.close();
  b.close();

  // commDeleteUsers once, on two shards of one generated table
  const n = 20000, users = 300;
  const comm = native.commCreate(new Int32Array(2));
  native.commGenSyntheticSharded(comm, 0x5EED5EEDn, n, users, 32, 0);
  const twin = native.ctxCreate(0);
  native.genSynthetic(twin, 0x5EED5EEDn, n, 0, n, users, 32, 0);
  const ids = Int32Array.from([5, 299, -1, 5, 300, 17, 100]);
  const rowsC = new Int32Array(n), perC = new Int32Array(ids.length), owners = new Int32Array(ids.length);
  const rowsT = new Int32Array(n), perT = new Int32Array(ids.length);
  const kc = native.commDeleteUsers(comm, ids, rowsC, perC, owners);
  const kt = native.deleteUsers(twin, ids, rowsT, perT);
  assert.ok(kt > 0);
  assert.strictEqual(kc, kt);
  assert.deepStrictEqual(Array.from(rowsC.subarray(0, kc)), Array.from(rowsT.subarray(0, kt)));
  assert.deepStrictEqual(Array.from(perC), Array.from(perT));
  assert.ok(owners[2] === -1 && owners[4] === -1 && owners[0] === owners[3] && [0, 1].includes(owners[0]) && [0, 1].includes(owners[1]));
  assert.strictEqual(native.commDeleteUsers(comm, ids, rowsC), 0);
  native.commDestroy(comm);
  native.ctxDestroy(twin);
  Date.now = realNow;
  console.log('host gpu_delete_users_test ok');
}

main();
