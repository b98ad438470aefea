'use strict';
// GPU check of the in-flight expired queue through the addon: expiredQueueBegin / expiredQueueFinish / expiredQueueRoom against
// the definition (ascending rows with prev < end <= now) with batches held in flight by scanBatchBegin; then
// createFeedService(store, {purgeInFlight: true}).purgeTick dispatching the entries of the same trace served with the option off.
process.env.TZ = 'UTC';
const assert = require('assert');
const pieNative = require('../pieNative');
const {createStore} = require('../sessionStore');
const {createFeedService} = require('../feedService');
const {createServer} = require('../server');

const END_NONE = -(2n ** 63n);
const NOW = 1700000000000n, HOUR = 3600000n;

async function addonCalls(){
  const native = pieNative.load();
  const ctx = native.ctxCreate(0);
  native.setBatchLanes(ctx, 3);
  const N = 40000, U = 20;
  const start = new BigInt64Array(N), end = new BigInt64Array(N), user = new Int32Array(N), disc = new Int32Array(N);
  for(let i = 0; i < N; i++){
    start[i] = NOW - 10n * HOUR + BigInt(i);
    end[i] = i % 7 === 0 ? NOW - BigInt(i % 5000) * 1000n : NOW + HOUR + BigInt(i);
    user[i] = i % U; disc[i] = i % 5;
  }
  end[7] = END_NONE; end[14] = NOW; end[21] = NOW - HOUR;     // a deleted session; end == now is in; end == prev is out
  const prev = NOW - HOUR;
  const want = [];
  for(let i = 0; i < N; i++){ if(end[i] > prev && end[i] <= NOW){ want.push(i); } }
  assert.ok(want.length > 1000 && want.includes(14) && !want.includes(21) && !want.includes(7));
  assert.throws(() => native.expiredQueueBegin(ctx, prev, NOW, N), e => e.code === -6);            // no table yet
  native.loadColumns(ctx, start, end, user, disc, U);
  native.setDisciplines(ctx, 31n, 5);

  const nq = 4;
  const nows = new BigInt64Array(nq).fill(NOW), cutoffs = new BigInt64Array(nq).fill(END_NONE), masks = new BigUint64Array(nq).fill(31n);
  const wantM = native.scanBatch(ctx, nows, cutoffs, masks);
  for(let b = 0; b < 3; b++){ assert.strictEqual(native.scanBatchBegin(ctx, nows, cutoffs, masks), nq); }
  assert.throws(() => native.expiredQueue(ctx, prev, NOW, new Int32Array(N)), e => e.code === -6);   // the synchronous call keeps its rule

  assert.strictEqual(native.expiredQueueRoom(ctx), 1);
  assert.throws(() => native.expiredQueueFinish(ctx), e => e.code === -6);
  assert.strictEqual(native.expiredQueueBegin(ctx, prev, NOW, N), N);
  assert.strictEqual(native.expiredQueueRoom(ctx), 0);
  assert.throws(() => native.expiredQueueBegin(ctx, prev, NOW, N), e => e.code === -6);              // one at a time
  const pending = native.expiredQueueFinish(ctx);
  assert.ok(pending instanceof Promise);
  assert.throws(() => native.expiredQueueRoom(ctx), e => e.code === -6);   // the handle is the worker's until the promise settles
  const got = await pending;
  assert.ok(got instanceof Int32Array);
  assert.deepStrictEqual(Array.from(got), want);
  assert.strictEqual(native.expiredQueueRoom(ctx), 1);
  // too little room: the rejection carries the true length
  native.expiredQueueBegin(ctx, prev, NOW, 10);
  await assert.rejects(native.expiredQueueFinish(ctx), e => e.code === -5 && e.length === want.length);
  assert.strictEqual(native.expiredQueueRoom(ctx), 1);
  // counting only, an inverted window
  native.expiredQueueBegin(ctx, prev, NOW, 0);
  assert.strictEqual((await native.expiredQueueFinish(ctx)).length, 0);
  native.expiredQueueBegin(ctx, NOW, prev, 16);
  assert.strictEqual((await native.expiredQueueFinish(ctx)).length, 0);
  // the batches that were in flight all along
  for(let b = 0; b < 3; b++){ assert.deepStrictEqual(native.scanBatchFinish(ctx), wantM); }
  assert.throws(() => native.scanBatchFinish(ctx), e => e.code === -6);
  // the drained call agrees
  const buf = new Int32Array(N);
  const k = native.expiredQueue(ctx, prev, NOW, buf);
  assert.deepStrictEqual(Array.from(buf.subarray(0, k)), want);
  native.ctxDestroy(ctx);
}

// one trace on a store: logins over ten hours, a touch and two deletes; then purge ticks at four clocks, each beside a turn's batch
async function trace(options){
  const realNow = Date.now;
  let fakeNow = 1760000000000;
  Date.now = () => fakeNow;
  try{
    const U = 12, N = 600;
    const store = createStore({batchLanes: 3});
    const made = [];
    for(let i = 0; i < N; i++){
      fakeNow += 60000;
      made.push(store.createSession('user-' + ((i * 5) % U)).token);
    }
    store.deleteSession(made[9]);
    store.deleteSession(made[300]);
    store.touchSession(made[10]);
    store.flush();
    const feeds = createFeedService(store, options);
    const sent = [], summaries = [];
    const send = async (payload, meta) => { sent.push({payload, meta}); return {success: payload.sessionRow % 50 !== 0}; };
    const first = fakeNow - N * 60000 + store.SESSION_TTL_MS;          // when the first session dies
    for(const t of [first - 1000, first + 50 * 60000, first + 50 * 60000, first + 400 * 60000, first + 550 * 60000]){
      fakeNow = Math.max(fakeNow, t);
      const queries = [{now: t, cutoff: 0}, {now: t + 1, cutoff: 0}, {now: t, cutoff: t - 3600000}];
      summaries.push(await feeds.purgeTick(t, send, queries));
    }
    summaries.push(await feeds.purgeTick(first + 800 * 60000, send));   // a tick with no turn beside it
    const out = {sent, summaries, ticksInFlight: feeds.ticksInFlight(), purgeInFlight: feeds.purgeInFlight(), store};
    return out;
  }finally{
    Date.now = realNow;
  }
}

async function purgeTicks(){
  const off = await trace(undefined), on = await trace({purgeInFlight: true});
  assert.strictEqual(off.purgeInFlight, false);
  assert.strictEqual(on.purgeInFlight, true);
  assert.strictEqual(off.ticksInFlight, 0);
  assert.strictEqual(on.ticksInFlight, 6);
  assert.deepStrictEqual(on.summaries, off.summaries);
  assert.deepStrictEqual(on.sent, off.sent);
  const totals = off.summaries.map(s => s.total);
  assert.strictEqual(totals[0], 0);
  assert.strictEqual(totals[2], 0);                                     // the same clock again: nothing new
  assert.ok(totals[1] > 0 && totals[3] > 0 && totals[4] > 0 && totals[5] > 0);
  assert.strictEqual(totals.reduce((a, b) => a + b, 0), 600 - 2);       // every session but the two deleted ones, each once
  assert.ok(off.summaries.some(s => s.failed > 0));
  const rows = off.sent.map(x => x.payload.sessionRow);
  assert.strictEqual(new Set(rows).size, rows.length);
  // the server hands the option through from the environment
  process.env.PIE_PURGE_IN_FLIGHT = '1';
  assert.strictEqual(createServer({store: on.store, findUserById: () => null}).feeds.purgeInFlight(), true);
  delete process.env.PIE_PURGE_IN_FLIGHT;
  assert.strictEqual(createServer({store: on.store, findUserById: () => null}).feeds.purgeInFlight(), false);
  off.store.close();
  on.store.close();
}

addonCalls().then(purgeTicks).then(() => console.log('host gpu_expired_inflight_test ok'), err => { console.error(err); process.exit(1); });
