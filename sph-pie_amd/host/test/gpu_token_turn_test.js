'use strict';
// GPU check of a whole turn through the addon (tokenTurn -> pie_token_turn) against a JS restatement of the header's rules, and of
// host/tokenSessionStore.js against the recorded reference trace tests/golden/sessionstore_g5_trace.json (calls into the
// reference's sessionStore.js and its answers; the conventions of tests/trace_replay.py), once call by call and once with every
// maximal run of get / touch / del calls as one turn().
const assert = require('assert');
const crypto = require('crypto');
const fs = require('fs');
const path = require('path');
const pieNative = require('../pieNative');
const {keysOfTokens} = require('../tokenKeys');
const tokenSessionStore = require('../tokenSessionStore');

const END_NONE = -(2n ** 63n);
const NOW = 1700000000000n, HOUR = 3600000n;
const GET = 0, TOUCH = 1, DELETE = 2;

// ---- 1. tokenTurn against the rules, one op after another
{
  const native = pieNative.load();
  const ctx = native.ctxCreate(0);
  const N = 300, U = 20;
  const tokens = Array.from({length: N}, () => crypto.randomBytes(48).toString('base64'));
  const start = new BigInt64Array(N), end = new BigInt64Array(N), user = new Int32Array(N), disc = new Int32Array(N);
  const rowOf = new Map();
  for(let i = 0; i < N; i++){
    start[i] = NOW - 10n * HOUR + BigInt(i);
    end[i] = i % 3 === 0 ? NOW - BigInt(i) : NOW + HOUR + BigInt(i);   // a third expired
    if(i % 50 === 7){ end[i] = END_NONE; }                             // and a few tombstones
    user[i] = i % U; disc[i] = i % 5;
    rowOf.set(tokens[i], i);
  }
  native.loadColumns(ctx, start, end, user, disc, U);
  const empty = [new BigUint64Array(0), new BigInt64Array(0), new BigInt64Array(0), new Uint8Array(0)];
  assert.throws(() => native.tokenTurn(ctx, ...empty), e => e.code === -6);   // no column yet
  native.tokenSet(ctx, keysOfTokens(tokens));
  assert.strictEqual(native.tokenTurn(ctx, ...empty).row.length, 0);

  let seed = 12345;
  const rnd = n => { seed = (seed * 1103515245 + 12345) % 2147483648; return seed % n; };
  const misses = Array.from({length: 10}, () => crypto.randomBytes(48).toString('base64'));
  for(const k of [1, 2, 64, 257, 700]){
    const asked = [], nows = new BigInt64Array(k), newEnds = new BigInt64Array(k), kinds = new Uint8Array(k);
    for(let i = 0; i < k; i++){
      const pick = rnd(10);
      asked.push(pick < 5 ? tokens[rnd(8)] : pick < 9 ? tokens[rnd(N)] : misses[rnd(10)]);   // half on eight tokens: chains form
      nows[i] = NOW + BigInt(rnd(4 * 3600000)) - 2n * HOUR;                                  // clocks of their own, not monotone
      kinds[i] = [GET, GET, GET, TOUCH, TOUCH, DELETE][rnd(6)];
      newEnds[i] = kinds[i] === TOUCH ? nows[i] + BigInt(rnd(3 * 3600000)) - HOUR / 2n : 0n;
    }
    const got = native.tokenTurn(ctx, keysOfTokens(asked), nows, newEnds, kinds);
    assert.strictEqual(got.row.length, k);
    for(let i = 0; i < k; i++){
      const row = rowOf.has(asked[i]) ? rowOf.get(asked[i]) : -1;
      let wantRow = row, live = 0, e = row >= 0 ? end[row] : END_NONE;
      if(row >= 0){
        if(kinds[i] === GET){ live = e > nows[i] ? 1 : 0; }
        else if(kinds[i] === TOUCH){ if(e > nows[i]){ e = newEnds[i]; live = 1; } }
        else if(e !== END_NONE){ e = END_NONE; }
        else{ wantRow = -1; }
        end[row] = e;
      }
      assert.strictEqual(got.row[i], wantRow, `row of op ${i} of ${k}`);
      assert.strictEqual(got.live[i], live, `liveness of op ${i} of ${k}`);
      assert.strictEqual(got.end[i], e, `end of op ${i} of ${k}`);
      if(row >= 0){
        assert.strictEqual(got.user[i], user[row]);
        assert.strictEqual(got.start[i], start[row]);
      }
    }
    const s = new BigInt64Array(N), e2 = new BigInt64Array(N), u = new Int32Array(N), d = new Int32Array(N);
    native.readColumns(ctx, s, e2, u, d);
    assert.deepStrictEqual(Array.from(e2), Array.from(end));
  }
  // malformed turns: lengths that disagree, a kind the library does not know (nothing changes)
  const two = keysOfTokens(tokens.slice(0, 2));
  assert.throws(() => native.tokenTurn(ctx, two, new BigInt64Array(1), new BigInt64Array(2), new Uint8Array(2)), TypeError);
  assert.throws(() => native.tokenTurn(ctx, two, new BigInt64Array(2).fill(NOW - 9n * HOUR), new BigInt64Array(2).fill(NOW + 99n * HOUR), Uint8Array.of(TOUCH, 3)),
                e => e.code === -1);
  const e3 = new BigInt64Array(N);
  native.readColumns(ctx, new BigInt64Array(N), e3, new Int32Array(N), new Int32Array(N));
  assert.deepStrictEqual(Array.from(e3), Array.from(end));
  native.ctxDestroy(ctx);
}

// ---- 2. the reference trace through tokenSessionStore
const trace = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', '..', 'tests', 'golden', 'sessionstore_g5_trace.json'), 'utf8'));
assert.strictEqual(trace.ttl_ms, tokenSessionStore.SESSION_TTL_MS);
const realNow = Date.now;

function replay(asTurns){
  const store = tokenSessionStore.createStore();
  const tokens = [];
  let clock = 0, checked = 0, turns = 0;
  Date.now = () => clock;
  let run = [];
  const flush = () => {
    if(run.length === 0){ return; }
    const answers = store.turn(run.map(op => ({op: op.op, token: tokens[op.tok], now: op.now})));
    turns++;
    run.forEach((op, i) => {
      if(op.op === 'del'){ assert.strictEqual(answers[i], undefined); }
      else{ assert.deepStrictEqual(answers[i], op.result, JSON.stringify(op)); }
      checked++;
    });
    run = [];
  };
  try{
    for(const op of trace.ops){
      clock = op.now;
      if(asTurns && (op.op === 'get' || op.op === 'touch' || op.op === 'del')){
        run.push(op);
        continue;
      }
      flush();
      if(op.op === 'create'){
        const made = store.createSession(op.user);
        assert.strictEqual(made.expiresAt, op.expiresAt);
        tokens.push(made.token);
      }else if(op.op === 'get'){
        assert.deepStrictEqual(store.getSession(tokens[op.tok]), op.result, JSON.stringify(op));
      }else if(op.op === 'touch'){
        assert.deepStrictEqual(store.touchSession(tokens[op.tok]), op.result, JSON.stringify(op));
      }else if(op.op === 'del'){
        assert.strictEqual(store.deleteSession(tokens[op.tok]), undefined);
      }else if(op.op === 'delUser'){
        store.deleteSessionsForUser(op.user);
      }else if(op.op === 'purge'){
        store.purgeExpiredSessions();
      }else if(op.op === 'census'){
        // get on every token ever issued, in issue order: one turn, or one call each
        const got = asTurns ? store.turn(tokens.map(token => ({op: 'get', token}))) : tokens.map(token => store.getSession(token));
        assert.deepStrictEqual(got.map((g, i) => (g ? i : -1)).filter(i => i >= 0), op.live, 'census at ' + op.now);
      }else{
        assert.fail('unknown op ' + op.op);
      }
      checked++;
    }
    flush();
    assert.strictEqual(checked, trace.ops.length);
    assert.strictEqual(tokens.length, trace.sessions);
    // the misses of the reference: falsy tokens, unknown tokens, falsy and unknown users
    assert.strictEqual(store.getSession(''), null);
    assert.strictEqual(store.getSession(undefined), null);
    assert.strictEqual(store.touchSession('no such token'), null);
    assert.strictEqual(store.deleteSession(''), undefined);
    assert.strictEqual(store.deleteSessionsForUser(''), undefined);
    assert.strictEqual(store.deleteSessionsForUser('nobody'), undefined);
    assert.deepStrictEqual(store.turn([]), []);
    assert.throws(() => store.turn([{op: 'create', token: 'x'}]), TypeError);
    // nothing on the store grows with the sessions: its only containers are the user-id strings
    assert.strictEqual(store.tableRows(), trace.sessions);
    assert.strictEqual(store.userIds().length, new Set(trace.ops.filter(o => o.op === 'create').map(o => o.user)).size);
    for(const [name, value] of Object.entries(store)){
      const container = Array.isArray(value) || ArrayBuffer.isView(value) || value instanceof Map || value instanceof Set;
      assert.ok(!container, 'the store carries a container: ' + name);
    }
    const source = fs.readFileSync(path.join(__dirname, '..', 'tokenSessionStore.js'), 'utf8');
    const made = source.match(/new (Map|Set|Array)\b|=\s*\[\]/g) || [];
    assert.deepStrictEqual(made.sort(), ['= []', '= []', 'new Array', 'new Map'],
      'userIndex, userIds, and per-call arrays inside turn(): any other container has to be argued for here');
  }finally{
    Date.now = realNow;
    store.close();
  }
  return turns;
}
assert.strictEqual(replay(false), 0);
assert.ok(replay(true) > 50);
console.log('host gpu_token_turn_test ok');
