'use strict';
// GPU check of turns beside a batch held in flight through the addon (tokenTurnBegin / tokenTurnFinish / tokenTurnRoom ->
// pie_token_turn_begin / _finish / _room): host/tokenSessionStore.js turnAsync against the recorded reference trace
// tests/golden/sessionstore_g5_trace.json with a batch begun by scanBatchBegin open across every call, and
// createFeedService(store, {turns: true}) against the default path on a twin store.
const assert = require('assert');
const crypto = require('crypto');
const fs = require('fs');
const path = require('path');
const tokenSessionStore = require('../tokenSessionStore');
const {createStore} = require('../sessionStore');
const {createFeedService} = require('../feedService');
const {keysOfTokens} = require('../tokenKeys');

const trace = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', '..', 'tests', 'golden', 'sessionstore_g5_trace.json'), 'utf8'));
const realNow = Date.now;

// ---- 1. the reference trace: every maximal run of get / touch / del calls is one turnAsync, a batch in flight around it
async function replay(){
  const store = tokenSessionStore.createStore({orderedRun: 0});   // (a context with a valid ordered run refuses tokenTurnBegin)
  const native = store.native, ctx = store.ctx;
  const tokens = [];
  let clock = 0, checked = 0, turns = 0, open = 0;
  Date.now = () => clock;
  let run = [];
  const held = async calls => {
    if(store.tableRows() === 0){ return store.turnAsync(calls); }
    native.scanBatchBegin(ctx, BigInt64Array.of(BigInt(clock), BigInt(clock - 1000)), BigInt64Array.of(0n, 0n), BigUint64Array.of(~0n & 0xFFFFFFFFn, 1n));
    open++;
    try{
      assert.throws(() => store.turn(calls), e => e.code === -6);       // the synchronous turn keeps its rule
      assert.strictEqual(native.tokenTurnRoom(ctx), 4);
      const before = store.turnsInFlight();
      const pending = store.turnAsync(calls);                           // begun at once; the wait is on the libuv pool
      assert.strictEqual(store.turnsInFlight(), before + 1);
      assert.throws(() => native.tokenTurnRoom(ctx), e => e.code === -6);   // the handle is busy until the Promise settles
      const answers = await pending;
      assert.strictEqual(native.tokenTurnRoom(ctx), 4);
      return answers;
    }finally{
      native.scanBatchFinish(ctx);
    }
  };
  const flush = async () => {
    if(run.length === 0){ return; }
    const answers = await held(run.map(op => ({op: op.op, token: tokens[op.tok], now: op.now})));
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
      if(op.op === 'get' || op.op === 'touch' || op.op === 'del'){ run.push(op); continue; }
      await flush();
      if(op.op === 'create'){
        const made = store.createSession(op.user);
        assert.strictEqual(made.expiresAt, op.expiresAt);
        tokens.push(made.token);
      }else if(op.op === 'delUser'){
        store.deleteSessionsForUser(op.user);
      }else if(op.op === 'purge'){
        store.purgeExpiredSessions();
      }else if(op.op === 'census'){
        const calls = tokens.map(token => ({op: 'get', token}));
        const got = calls.length ? await held(calls) : [];
        assert.deepStrictEqual(got.map((g, i) => (g ? i : -1)).filter(i => i >= 0), op.live, 'census at ' + op.now);
        assert.deepStrictEqual(got, store.turn(calls), 'turnAsync equals turn');
      }else{
        assert.fail('unknown op ' + op.op);
      }
      checked++;
    }
    await flush();
    assert.strictEqual(checked, trace.ops.length);
    assert.strictEqual(tokens.length, trace.sessions);
    assert.deepStrictEqual(await store.turnAsync([]), []);
    assert.deepStrictEqual(await store.turnAsync([{op: 'get', token: ''}, {op: 'del', token: 'no such token'}]), [null, undefined]);
    assert.ok(turns > 50 && open > 50 && store.turnsInFlight() >= turns);
  }finally{
    Date.now = realNow;
    store.close();
  }
}

// ---- 2. the feed service: {turns: true} serves the same statuses and bytes as the default path, and touches the sessions it served
function twin(){
  let fakeNow = 1760000000000;
  Date.now = () => fakeNow;
  const U = 12, N = 240;
  const store = createStore({batchLanes: 3, orderedRun: 0});
  const made = [];
  for(let i = 0; i < N; i++){
    fakeNow += 1000;
    made.push(store.createSession('user-' + ((i * 5) % U)).token);
  }
  store.deleteSession(made[9]);
  store.flush();
  store.native.tokenSet(store.ctx, keysOfTokens(made));
  return {store, made, t0: fakeNow + 60000};
}

function requestsOf(t, shift){
  const N = t.made.length, t0 = t.t0 + shift, late = t0 + 2 * t.store.SESSION_TTL_MS;
  const requests = [];
  for(let i = 0; i < 60; i++){
    const kind = i % 5;
    if(kind === 3){ requests.push({token: crypto.randomBytes(48).toString('hex'), query: {now: t0, cutoff: 0}}); }              // unknown
    else if(kind === 4){ requests.push({token: t.made[(i * 7) % N], query: {now: late, cutoff: 0}}); }                          // expired at its own clock
    else{ requests.push({token: t.made[(i * 7) % N], query: {now: t0 + (i % 3) * 1000, cutoff: 0}}); }                          // valid, three clocks
  }
  requests.push({token: t.made[9], query: {now: t0, cutoff: 0}});                                                              // deleted
  requests.push({token: null, query: {now: t0, cutoff: 0}});                                                                   // no cookie
  return requests;
}

async function feedTurn(){
  const a = twin(), b = twin();
  try{
    const off = createFeedService(a.store), on = createFeedService(b.store, {turns: true});
    assert.strictEqual(off.turns(), false);
    assert.strictEqual(on.turns(), true);
    for(const shift of [0, 5000]){
      const ra = requestsOf(a, shift), rb = requestsOf(b, shift);
      const got = await on.serveTurn(rb);
      const ends = on.touchedEnds();
      // The default path's store gets the same touches by the synchronous turn, ahead of its turn: a touch applies to a live
      // session only and keeps it live, so it moves no row into or out of a feed, and the `end` a body prints is the table's
      // own when the rows are fetched (pie_batch_fetch_requests) — the touched one on both paths.
      const served = ra.map((r, i) => i).filter(i => (i < 60 ? i % 5 : 3) <= 2);
      a.store.flush();
      const res = a.store.native.tokenTurn(a.store.ctx, keysOfTokens(served.map(i => ra[i].token)), BigInt64Array.from(served, i => BigInt(ra[i].query.now)),
        BigInt64Array.from(served, i => BigInt(ra[i].query.now + a.store.SESSION_TTL_MS)), new Uint8Array(served.length).fill(1));
      assert.ok(res.live.every(x => x === 1));
      const want = await off.serveTurn(ra);
      assert.strictEqual(got.length, want.length);
      got.forEach((g, i) => {
        assert.strictEqual(g.status, want[i].status, 'status of request ' + i);
        assert.ok(Buffer.compare(g.body, want[i].body) === 0, 'body of request ' + i);
        const kind = i < 60 ? i % 5 : 3;
        assert.strictEqual(g.status, kind <= 2 ? 200 : 401, 'request ' + i);
        // the session answer: touchSession's expiresAt for a served request, nothing for a refused one
        assert.strictEqual(ends[i], g.status === 200 ? BigInt(rb[i].query.now + b.store.SESSION_TTL_MS) : 0n, 'touched end of request ' + i);
      });
      assert.ok(got.some(x => x.status === 200 && x.body.length > 20));
    }
    assert.strictEqual(on.turnsInFlight(), 2);
    assert.strictEqual(off.turnsInFlight(), 0);
  }finally{
    a.store.close();
    b.store.close();
    Date.now = realNow;
  }
}

replay().then(feedTurn).then(() => console.log('host gpu_token_turn_inflight_test ok'), err => { console.error(err); process.exit(1); });
