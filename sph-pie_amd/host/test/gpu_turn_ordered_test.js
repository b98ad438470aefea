'use strict';
// GPU check of the token store's turnOrdered option (setTurnOrdered -> pie_set_turn_ordered): on a store whose table has a valid
// ordered run (mode 2, built by one scan), 50 createSession calls and one turn of mixed calls leave the run valid with every row
// — not rebuilt — and the feed of a scan on the run equals the events this file derives from the calls it made.  The same calls on
// a store without the option drop the run.
process.env.TZ = 'UTC';
const assert = require('assert');
const tokenSessionStore = require('../tokenSessionStore');

const D = 32, ALL = 0xFFFFFFFFn;
const realNow = Date.now;

function drive(turnOrdered){
  const store = tokenSessionStore.createStore(turnOrdered ? {orderedRun: 2, turnOrdered: true} : {orderedRun: 2});
  const native = store.native, ctx = store.ctx;
  assert.strictEqual(typeof native.setTurnOrdered, 'function');
  const sessions = [];                               // row -> {user, start, end}: what the calls below mean, kept by this test alone
  let clock = 1700000000000;
  Date.now = () => clock;
  const users = n => 'user-' + (n % 37);
  const made = (answers, calls) => answers.forEach((a, i) => {
    if(calls[i].op === 'create'){ sessions.push({user: calls[i].userId, start: clock, end: a.expiresAt, token: a.token}); }
  });
  const feedOf = (now, cutoff) => {
    const ids = store.userIds();
    const want = ids.map(() => []);
    sessions.forEach((s, row) => { if(s.end > now && s.start >= cutoff){ want[ids.indexOf(s.user)].push(row); } });
    const counts = new Int32Array(ids.length), offsets = new BigInt64Array(ids.length + 1), idx = new Int32Array(sessions.length);
    native.setDisciplines(ctx, ALL, D);
    const m = native.scan(ctx, now, cutoff, counts, offsets, idx);
    const got = ids.map((_, u) => Array.from(idx.subarray(Number(offsets[u]), Number(offsets[u + 1]))));
    assert.strictEqual(m, want.reduce((a, w) => a + w.length, 0));
    assert.deepStrictEqual(got, want);               // per user in (start, row) order: the rows were created in time order
  };
  try{
    // 300 sessions in one turn, then one more: the table grows to twice its rows, so the logins below find room in place
    let calls = Array.from({length: 300}, (_, i) => ({op: 'create', userId: users(i)}));
    made(store.turn(calls), calls);
    clock += 1000;
    calls = [{op: 'create', userId: users(300)}];
    made(store.turn(calls), calls);
    feedOf(clock, 0);                                // builds the run
    let info = native.tableInfo(ctx);
    assert.strictEqual(info.orderedRows, 301);
    assert.ok(Number(native.stats(ctx).k1Variant) & 0x2000, 'the scan took the ordered run');
    const builds = info.orderedBuilds;
    for(let i = 0; i < 50; i++){
      clock += 10;
      const s = store.createSession(users(7 * i));
      sessions.push({user: users(7 * i), start: clock, end: s.expiresAt, token: s.token});
    }
    clock += 1000;
    calls = [{op: 'create', userId: users(3)}, {op: 'get', token: sessions[10].token}, {op: 'touch', token: sessions[11].token},
             {op: 'del', token: sessions[12].token}, {op: 'create', userId: users(5)}, {op: 'get', token: sessions[320].token},
             {op: 'del', token: sessions[321].token}];
    const got = store.turn(calls);
    made(got, calls);
    assert.strictEqual(got[1].userId, sessions[10].user);
    sessions[11].end = got[2].expiresAt;
    sessions[12].end = sessions[321].end = -Infinity;
    info = native.tableInfo(ctx);
    assert.strictEqual(info.rows, 353);
    if(turnOrdered){
      assert.strictEqual(info.orderedRows, 353, 'the run is valid and holds every row');
      assert.strictEqual(info.orderedBuilds, builds, 'kept, not rebuilt');
    }else{
      assert.strictEqual(info.orderedRows, 0, 'without the option a login drops the run');
    }
    feedOf(clock, 0);
    feedOf(clock + store.SESSION_TTL_MS - 500, 1700000000500);   // only the sessions made or touched late are still live
    assert.ok(Number(native.stats(ctx).k1Variant) & 0x2000);
    if(turnOrdered){ assert.strictEqual(native.tableInfo(ctx).orderedBuilds, builds); }
    assert.throws(() => native.setTurnOrdered(ctx, 2));
  }finally{
    Date.now = realNow;
    store.close();
  }
}

drive(true);
drive(false);
console.log('host gpu_turn_ordered_test ok');
