'use strict';
// GPU check of host/shardedQueue.js: a world-3 communicator on GPU 0 (PIE_RCCL_LIB = the one-GPU stand-in for RCCL) holds a
// synthetic table in shards; dispatchExpiredSessions / dispatchArchivedGroups drained through the sharded source must give the
// summaries and payloads, in the same order, that a single context over the same unsharded table gives.
process.env.TZ = 'UTC';
const assert = require('assert');
const pieNative = require('../pieNative');
const {createShardedQueue} = require('../shardedQueue');
const {dispatchExpiredSessions, dispatchArchivedGroups} = require('../dispatchQueue');
const dc = require('../disciplineConfig');

const SEED = 0x5EED5EEDn, T0 = 1700000000000, HOUR = 3600 * 1000, DAY = 24 * HOUR, W = 12 * HOUR;
const END_NONE = -(2n ** 63n);
const N = 120000, U = 600, D = dc.DISCIPLINES.length;

// the single-context source over the whole table, the same shape the sharded one offers
function singleSource(native){
  const ctx = native.ctxCreate(0);
  native.genSynthetic(ctx, SEED, N, 0, N, U, D, 0);
  const buf = new Int32Array(N);
  const ids = Array.from({length: U}, (_, g) => 'user-' + g);
  return {
    expiredRows: (prev, now) => buf.slice(0, native.expiredQueue(ctx, prev === null || prev === undefined ? END_NONE : prev, now, buf)),
    archivedRows: (now, windowMs) => buf.slice(0, native.archiveQueue(ctx, now, windowMs, buf)),
    fetchRows: idx => {
      const m = idx.length;
      const s = new BigInt64Array(m), e = new BigInt64Array(m), u = new Int32Array(m), d = new Int32Array(m);
      if(m > 0){ native.fetchRows(ctx, idx, m, s, e, u, d); }
      return {start: s, end: e, user: u, disc: d};
    },
    userIds: () => ids
  };
}

function recorder(){
  const sent = [];
  return {sent, send: async (payload, meta) => {
    sent.push([payload, meta]);
    return payload.sessionRow % 11 === 3 ? {success: false, error: 'refused'} : {success: true};
  }};
}

async function main(){
  const native = pieNative.load();
  const comm = native.commCreate(new Int32Array([0, 0, 0]));
  native.commGenSyntheticSharded(comm, SEED, N, U, D, 0);
  const sharded = createShardedQueue(native, comm);
  const single = singleSource(native);
  let checks = 0, nonEmpty = 0;
  const same = async (run) => {
    const a = recorder(), b = recorder();
    const sa = await run(single, a.send), sb = await run(sharded, b.send);
    assert.deepStrictEqual(sb, sa);
    assert.deepStrictEqual(b.sent, a.sent);
    if(sa.total > 0){ nonEmpty++; }
    checks++;
  };
  for(const [prev, now] of [[T0 - 6 * HOUR - 60000, T0 - 6 * HOUR], [T0 - 30 * DAY - 2 * HOUR, T0 - 30 * DAY], [null, T0 - 119 * DAY],
    [T0, T0 - DAY], [T0 - 10 * DAY, T0 - 10 * DAY]]){
    await same((src, send) => dispatchExpiredSessions(src, prev, now, send));
  }
  for(const now of [T0 - 200 * DAY, T0 - 119 * DAY - 12 * HOUR, T0 - 119 * DAY, T0 - 118 * DAY + 12 * HOUR]){
    await same((src, send) => dispatchArchivedGroups(src, now, send, W));
  }
  assert(nonEmpty >= 4, 'too few non-empty queues: ' + nonEmpty);
  // the sharded source reads the columns of any rows of its last queue, in the order asked
  const rows = sharded.expiredRows(T0 - 30 * DAY - 2 * HOUR, T0 - 30 * DAY);
  const want = single.fetchRows(single.expiredRows(T0 - 30 * DAY - 2 * HOUR, T0 - 30 * DAY));
  const rev = Int32Array.from(rows).reverse();
  const got = sharded.fetchRows(rev);
  assert.deepStrictEqual(Array.from(got.user).reverse(), Array.from(want.user));
  assert.deepStrictEqual(Array.from(got.end).reverse(), Array.from(want.end));
  checks++;
  native.commDestroy(comm);
  console.log('host comm_queue_test ok: ' + checks + ' checks, ' + nonEmpty + ' non-empty queues');
}

main().catch(err => { console.error(err); process.exit(1); });
