'use strict';
// GPU check of the communicator's in-flight calls through the addon (commTokenLookupBegin / Finish / Room, commExpiredQueueBegin /
// Finish / Room) and of shardedQueue's in-flight tick: a world-2 communicator on GPU 0 (PIE_RCCL_LIB = the one-GPU stand-in for
// RCCL) with a pipelined step begun and unfinished.  One lookup and one queue are begun and awaited while the step stays in
// flight; after the step is finished and collected the synchronous calls (commTokenLookup, commExpiredQueue) must give the same
// answers, element for element.
process.env.TZ = 'UTC';
const assert = require('assert');
const pieNative = require('../pieNative');
const {createShardedQueue} = require('../shardedQueue');

const SEED = 0x5EED5EEDn, T0 = 1700000000000, HOUR = 3600 * 1000, DAY = 24 * HOUR, TTL = 12 * HOUR;
const N = 20000, U = 300, D = 32, WORLD = 2;
const MASK = (1n << 64n) - 1n;

function keysOf(rows){
  const k = new BigUint64Array(rows.length * 2);
  rows.forEach((r, i) => {
    k[2 * i] = (BigInt(r + 1) * 0x9E3779B97F4A7C15n) & MASK;
    k[2 * i + 1] = (BigInt(r) * 0xD1B54A32D192ED03n + 7n) & MASK;
  });
  return k;
}

async function main(){
  const native = pieNative.load();
  const comm = native.commCreate(new Int32Array(WORLD));
  native.commGenSyntheticSharded(comm, SEED, N, U, D, 0);
  for(let r = 0; r < WORLD; r++){ native.setDisciplines(native.commCtx(comm, r), 0xFFFFFFFFn, D); }
  native.commTokenSet(comm, keysOf(Array.from({length: N - 10}, (_, i) => i)));
  const source = createShardedQueue(native, comm);
  const nows = BigInt64Array.from([T0 - 6 * HOUR, T0 - 7 * HOUR, T0 - 8 * HOUR], BigInt);
  const cuts = BigInt64Array.from([T0 - 61 * DAY, T0 - 62 * DAY, T0 - 61 * DAY], BigInt);
  const masks = BigUint64Array.from([0x55555555n, 0xAAAAAAAAn, 0xFFFFFFFFn]);
  native.commStepReserve(comm, 3, N);

  // present rows, rows the column does not cover, and keys nobody carries
  const ask = keysOf([0, 1, 17, 4096, 9999, N - 11, N - 10, N - 1, N + 5, N + 6]);
  const now = BigInt(T0 - TTL / 2), prev = BigInt(T0 - TTL);
  const clocks = new BigInt64Array(ask.length / 2).fill(now);

  native.commStepBegin(comm, nows, cuts, masks);
  assert.strictEqual(native.commTokenLookupRoom(comm), 4);
  assert.strictEqual(native.commExpiredQueueRoom(comm), 1);
  assert.strictEqual(native.commTokenLookupBegin(comm, ask, clocks), ask.length / 2);
  native.commExpiredQueueBegin(comm, prev, BigInt(T0), N);
  assert.strictEqual(native.commTokenLookupRoom(comm), 3);
  assert.strictEqual(native.commExpiredQueueRoom(comm), 0);
  assert.throws(() => native.commExpiredQueueBegin(comm, prev, BigInt(T0), N), e => e.code === -6);
  assert.throws(() => native.commTokenLookup(comm, ask, now), e => e.code === -6);          // the synchronous forms keep their rule
  assert.throws(() => native.commTokenLookupBegin(comm, ask, new BigInt64Array(1)), TypeError);
  const pending = native.commTokenLookupFinish(comm);
  assert.ok(pending instanceof Promise);
  assert.throws(() => native.commTokenLookupRoom(comm), e => e.code === -6);                // busy until the promise settles
  const got = await pending;
  const queue = await native.commExpiredQueueFinish(comm);
  assert.strictEqual(native.commTokenLookupRoom(comm), 4);
  assert.strictEqual(native.commExpiredQueueRoom(comm), 1);
  assert.throws(() => native.commTokenLookupFinish(comm), e => e.code === -6);
  assert.throws(() => native.commExpiredQueueFinish(comm), e => e.code === -6);
  // too little room: the true length rides on the rejection, and the next begin is taken
  native.commExpiredQueueBegin(comm, prev, BigInt(T0), 1);
  await assert.rejects(native.commExpiredQueueFinish(comm), e => e.code === -5 && e.length === queue.rows.length);
  // the tick of a sharded source, still in flight
  const tick = await source.expiredRowsInFlight(prev, BigInt(T0));
  const cols = source.fetchRows(tick);

  native.commStepFinish(comm);
  assert.strictEqual(native.commStepCollect(comm), 0);
  const want = native.commTokenLookup(comm, ask, now);
  for(const col of ['row', 'live', 'user', 'owner']){ assert.deepStrictEqual(Array.from(got[col]), Array.from(want[col]), col); }
  for(const col of ['start', 'end']){ assert.deepStrictEqual(Array.from(got[col], String), Array.from(want[col], String), col); }
  assert.deepStrictEqual(Array.from(got.row.slice(0, 6)), [0, 1, 17, 4096, 9999, N - 11]);
  assert.ok(Array.from(got.row.slice(6)).every(r => r === -1) && Array.from(got.owner.slice(6)).every(r => r === -1));
  const rows = new Int32Array(N), rank = new Int32Array(N), local = new Int32Array(N);
  const q = native.commExpiredQueue(comm, prev, BigInt(T0), rows, rank, local);
  assert.ok(q > 1);
  assert.deepStrictEqual(Array.from(queue.rows), Array.from(rows.subarray(0, q)));
  assert.deepStrictEqual(Array.from(queue.owner), Array.from(rank.subarray(0, q)));
  assert.deepStrictEqual(Array.from(tick), Array.from(rows.subarray(0, q)));
  const drained = source.expiredRows(prev, BigInt(T0));
  const wantCols = source.fetchRows(drained);
  for(const col of ['start', 'end']){ assert.deepStrictEqual(Array.from(cols[col], String), Array.from(wantCols[col], String), col); }
  for(const col of ['user', 'disc']){ assert.deepStrictEqual(Array.from(cols[col]), Array.from(wantCols[col]), col); }
  assert.ok(Array.from(cols.end).every(e => e > prev && e <= BigInt(T0)));
  // destroyed with a lookup begun: the library lands it
  native.commTokenLookupBegin(comm, ask, clocks);
  native.commDestroy(comm);
  console.log('host comm_inflight_test ok');
}

main().catch((err) => { console.error(err); process.exit(1); });
