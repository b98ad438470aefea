'use strict';
// GPU check of turns that log in through host/tokenSessionStore.js (turn(calls) with {op: 'create'} in the lists -> sessionTurn ->
// pie_session_turn) against the recorded reference trace tests/golden/sessionstore_g5_trace.json: every maximal run of create /
// get / touch / del calls goes to the store in turns of 7, and every answer is the reference's.  Then createSession / getSession
// as a request handler calls them.
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const tokenSessionStore = require('../tokenSessionStore');

const trace = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', '..', 'tests', 'golden', 'sessionstore_g5_trace.json'), 'utf8'));
assert.strictEqual(trace.ttl_ms, tokenSessionStore.SESSION_TTL_MS);
const realNow = Date.now;
const CHUNK = 7;

{
  const store = tokenSessionStore.createStore();
  const tokenOf = n => 'g5-token-' + n;             // the create calls carry their tokens: the replay knows them before the turn runs
  let clock = 0, checked = 0, issued = 0, mixed = 0;
  Date.now = () => clock;
  let run = [];
  const flush = () => {
    for(let at = 0; at < run.length; at += CHUNK){
      const part = run.slice(at, at + CHUNK);
      const answers = store.turn(part.map(r => r.call));
      assert.strictEqual(answers.length, part.length);
      if(part.length > 1 && part.some(r => r.op.op === 'create')){ mixed++; }
      part.forEach((r, i) => {
        if(r.op.op === 'del'){ assert.strictEqual(answers[i], undefined); }
        else if(r.op.op === 'create'){ assert.deepStrictEqual(answers[i], {token: r.call.token, expiresAt: r.op.expiresAt}); }
        else{ assert.deepStrictEqual(answers[i], r.op.result, JSON.stringify(r.op)); }
        checked++;
      });
    }
    run = [];
  };
  try{
    for(const op of trace.ops){
      clock = op.now;
      if(op.op === 'create'){
        run.push({op, call: {op: 'create', userId: op.user, now: op.now, token: tokenOf(issued++)}});
        continue;
      }
      if(op.op === 'get' || op.op === 'touch' || op.op === 'del'){
        run.push({op, call: {op: op.op, token: tokenOf(op.tok), now: op.now}});
        continue;
      }
      flush();
      if(op.op === 'delUser'){
        store.deleteSessionsForUser(op.user);
      }else if(op.op === 'purge'){
        store.purgeExpiredSessions();
      }else if(op.op === 'census'){
        const got = store.turn(Array.from({length: issued}, (_, n) => ({op: 'get', token: tokenOf(n)})));
        assert.deepStrictEqual(got.map((g, i) => (g ? i : -1)).filter(i => i >= 0), op.live, 'census at ' + op.now);
      }else{
        assert.fail('unknown op ' + op.op);
      }
      checked++;
    }
    flush();
    assert.strictEqual(checked, trace.ops.length);
    assert.strictEqual(issued, trace.sessions);
    assert.strictEqual(store.tableRows(), trace.sessions);
    assert.ok(mixed > 50, 'creates shared their turns with other calls');
    // a create and the calls on its token in one list; a create without a user is refused and changes nothing
    clock += 1000;
    const got = store.turn([{op: 'get', token: 'late'}, {op: 'create', userId: 'late-user', token: 'late'}, {op: 'get', token: 'late'},
                            {op: 'touch', token: 'late', now: clock + 5}, {op: 'del', token: 'late'}, {op: 'get', token: 'late'}]);
    assert.deepStrictEqual(got, [null, {token: 'late', expiresAt: clock + trace.ttl_ms}, {userId: 'late-user', createdAt: clock, expiresAt: clock + trace.ttl_ms},
                                 {userId: 'late-user', expiresAt: clock + 5 + trace.ttl_ms}, undefined, null]);
    assert.throws(() => store.turn([{op: 'get', token: 'late'}, {op: 'create'}]), TypeError);
    assert.strictEqual(store.tableRows(), trace.sessions + 1);
  }finally{
    Date.now = realNow;
    store.close();
  }
}

// createSession / getSession the way a request handler calls them: random tokens, the real clock; the first session of an
// empty store and the ones after it
{
  const store = tokenSessionStore.createStore();
  try{
    assert.strictEqual(store.getSession('nothing yet'), null);
    const made = [];
    for(let i = 0; i < 5; i++){
      const before = Date.now();
      const s = store.createSession('user-' + (i % 3));
      assert.ok(/^[0-9a-f]{96}$/.test(s.token) && s.expiresAt >= before + store.SESSION_TTL_MS && s.expiresAt <= Date.now() + store.SESSION_TTL_MS);
      made.push(s);
      const g = store.getSession(s.token);
      assert.deepStrictEqual(g, {userId: 'user-' + (i % 3), createdAt: s.expiresAt - store.SESSION_TTL_MS, expiresAt: s.expiresAt});
    }
    assert.strictEqual(store.tableRows(), 5);
    assert.strictEqual(new Set(made.map(s => s.token)).size, 5);
    store.deleteSession(made[1].token);
    assert.deepStrictEqual(store.turn(made.map(s => ({op: 'get', token: s.token}))).map(g => (g ? g.userId : null)),
                           ['user-0', null, 'user-2', 'user-0', 'user-1']);
  }finally{
    store.close();
  }
}
console.log('host gpu_session_turn_test ok');
