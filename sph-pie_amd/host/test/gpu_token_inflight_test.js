'use strict';
// GPU check of the in-flight token lookup through the addon: tokenLookupBegin / tokenLookupFinish / tokenLookupRoom against a JS Map
// keyed by token, with a batch held in flight by scanBatchBegin; then createFeedService(store, {authInFlight: true}) serving a turn
// of valid, expired and unknown cookies with the statuses and bytes of the same turn served with the option off.
process.env.TZ = 'UTC';
const assert = require('assert');
const crypto = require('crypto');
const pieNative = require('../pieNative');
const {keysOfTokens} = require('../tokenKeys');
const {createStore} = require('../sessionStore');
const {createFeedService} = require('../feedService');
const {createServer} = require('../server');

const END_NONE = -(2n ** 63n);
const NOW = 1700000000000n, HOUR = 3600000n;

async function addonCalls(){
  const native = pieNative.load();
  const ctx = native.ctxCreate(0);
  native.setBatchLanes(ctx, 3);
  const N = 300, U = 20;
  const tokens = Array.from({length: N}, () => crypto.randomBytes(48).toString('base64'));
  const start = new BigInt64Array(N), end = new BigInt64Array(N), user = new Int32Array(N), disc = new Int32Array(N);
  const sessions = new Map();
  for(let i = 0; i < N; i++){
    start[i] = NOW - 10n * HOUR + BigInt(i);
    end[i] = i % 3 === 0 ? NOW - BigInt(i) : NOW + HOUR + BigInt(i);
    user[i] = i % U; disc[i] = i % 5;
    sessions.set(tokens[i], i);
  }
  end[7] = END_NONE;                                   // a deleted session
  native.loadColumns(ctx, start, end, user, disc, U);
  native.setDisciplines(ctx, 31n, 5);
  assert.throws(() => native.tokenLookupBegin(ctx, keysOfTokens(tokens), new BigInt64Array(N).fill(NOW)), e => e.code === -6);   // no column yet
  native.tokenSet(ctx, keysOfTokens(tokens));

  const nq = 4;
  const nows = new BigInt64Array(nq).fill(NOW), cutoffs = new BigInt64Array(nq).fill(END_NONE), masks = new BigUint64Array(nq).fill(31n);
  const wantM = native.scanBatch(ctx, nows, cutoffs, masks);
  assert.strictEqual(native.scanBatchBegin(ctx, nows, cutoffs, masks), nq);
  assert.throws(() => native.tokenLookup(ctx, keysOfTokens(tokens), NOW), e => e.code === -6);   // the synchronous call keeps its rule

  const misses = Array.from({length: 40}, () => crypto.randomBytes(48).toString('base64'));
  const asked = tokens.concat(misses, [tokens[1], tokens[1], tokens[1]]);
  const clock = new BigInt64Array(asked.length).fill(NOW);
  clock[asked.length - 3] = end[1] - 1n; clock[asked.length - 2] = end[1]; clock[asked.length - 1] = end[1] + 1n;   // the key's own clock
  for(let i = 0; i < N; i += 11){ clock[i] = NOW + BigInt(i) * HOUR; }
  assert.strictEqual(native.tokenLookupRoom(ctx), 4);
  assert.strictEqual(native.tokenLookupBegin(ctx, keysOfTokens(asked), clock), asked.length);
  assert.strictEqual(native.tokenLookupBegin(ctx, keysOfTokens([tokens[5]]), BigInt64Array.of(NOW)), 1);
  assert.strictEqual(native.tokenLookupBegin(ctx, new BigUint64Array(0), new BigInt64Array(0)), 0);
  assert.strictEqual(native.tokenLookupRoom(ctx), 1);
  assert.throws(() => native.tokenLookupBegin(ctx, keysOfTokens(asked), new BigInt64Array(3)), TypeError);   // one clock per key
  const pending = native.tokenLookupFinish(ctx);
  assert.ok(pending instanceof Promise);
  assert.throws(() => native.tokenLookupRoom(ctx), e => e.code === -6);   // the handle is the worker's until the promise settles
  const got = await pending;
  assert.strictEqual(got.row.length, asked.length);
  asked.forEach((t, i) => {
    const row = sessions.has(t) ? sessions.get(t) : -1;
    assert.strictEqual(got.row[i], row, 'row of request ' + i);
    assert.strictEqual(got.live[i], row >= 0 && end[row] > clock[i] ? 1 : 0, 'liveness of request ' + i);
    if(row >= 0){
      assert.strictEqual(got.user[i], user[row]);
      assert.strictEqual(got.start[i], start[row]);
      assert.strictEqual(got.end[i], end[row]);
    }
  });
  assert.deepStrictEqual(Array.from(got.live.slice(asked.length - 3)), [1, 0, 0]);
  assert.ok(got.live.some(v => v === 1) && got.live.slice(0, N).some(v => v === 0) && got.live[7] === 0);
  const one = await native.tokenLookupFinish(ctx);
  assert.deepStrictEqual([one.row[0], one.live[0], one.user[0]], [5, 1, 5]);
  assert.strictEqual((await native.tokenLookupFinish(ctx)).row.length, 0);
  assert.strictEqual(native.tokenLookupRoom(ctx), 4);
  assert.throws(() => native.tokenLookupFinish(ctx), e => e.code === -6);
  // the batch that was in flight all along
  assert.deepStrictEqual(native.scanBatchFinish(ctx), wantM);
  assert.throws(() => native.scanBatchFinish(ctx), e => e.code === -6);
  // the drained call agrees
  const drained = native.tokenLookup(ctx, keysOfTokens(tokens), NOW);
  native.tokenLookupBegin(ctx, keysOfTokens(tokens), new BigInt64Array(N).fill(NOW));
  const again = await native.tokenLookupFinish(ctx);
  for(const col of ['row', 'live', 'user', 'start', 'end']){ assert.deepStrictEqual(Array.from(again[col]), Array.from(drained[col]), col); }
  native.ctxDestroy(ctx);
}

async function feedTurn(){
  const realNow = Date.now;
  let fakeNow = 1760000000000;
  Date.now = () => fakeNow;
  const U = 12, N = 240;
  const store = createStore({batchLanes: 3});
  const made = [];
  for(let i = 0; i < N; i++){
    fakeNow += 1000;
    made.push(store.createSession('user-' + ((i * 5) % U)).token);
  }
  store.deleteSession(made[9]);
  store.flush();
  store.native.tokenSet(store.ctx, keysOfTokens(made));
  const t0 = fakeNow + 60000;
  const late = t0 + 2 * store.SESSION_TTL_MS;          // every session has expired by then
  const requests = [];
  for(let i = 0; i < 60; i++){
    const kind = i % 5;
    if(kind === 3){ requests.push({token: crypto.randomBytes(48).toString('hex'), query: {now: t0, cutoff: 0}}); }              // unknown
    else if(kind === 4){ requests.push({token: made[(i * 7) % N], query: {now: late, cutoff: 0}}); }                             // expired at its own clock
    else{ requests.push({token: made[(i * 7) % N], query: {now: t0 + (i % 3) * 1000, cutoff: 0}}); }                             // valid, three clocks
  }
  requests.push({token: made[9], query: {now: t0, cutoff: 0}});                                                                // deleted
  requests.push({token: null, query: {now: t0, cutoff: 0}});                                                                   // no cookie
  const off = createFeedService(store), on = createFeedService(store, {authInFlight: true});
  assert.strictEqual(off.authInFlight(), false);
  assert.strictEqual(on.authInFlight(), true);
  const want = await off.serveTurn(requests);
  const got = await on.serveTurn(requests);
  assert.strictEqual(on.lookupsInFlight(), 1);
  assert.strictEqual(off.lookupsInFlight(), 0);
  assert.strictEqual(got.length, requests.length);
  requests.forEach((r, i) => {
    assert.strictEqual(got[i].status, want[i].status, 'status of request ' + i);
    assert.ok(Buffer.compare(got[i].body, want[i].body) === 0, 'body of request ' + i);
    // and both are what the store's own getSession and the per-user path give
    const kind = i < 60 ? i % 5 : 3;
    assert.strictEqual(got[i].status, kind <= 2 ? 200 : 401, 'request ' + i);
    if(got[i].status === 200){
      const session = store.getSession(r.token);
      assert.ok(session !== null);
      assert.ok(Buffer.compare(got[i].body, off.eventsJsonForUser(session.userId, r.query)) === 0, 'feed of request ' + i);
    }
  });
  assert.ok(got.some(x => x.status === 200 && x.body.length > 20));
  // the server hands the option through from the environment
  process.env.PIE_AUTH_IN_FLIGHT = '1';
  assert.strictEqual(createServer({store, findUserById: () => null}).feeds.authInFlight(), true);
  delete process.env.PIE_AUTH_IN_FLIGHT;
  assert.strictEqual(createServer({store, findUserById: () => null}).feeds.authInFlight(), false);
  store.close();
  Date.now = realNow;
}

addonCalls().then(feedTurn).then(() => console.log('host gpu_token_inflight_test ok'), err => { console.error(err); process.exit(1); });
