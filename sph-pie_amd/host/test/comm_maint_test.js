'use strict';
// GPU check of a sharded table that ages through host/shardedQueue.js (commPruneBefore, commRetentionPurge, commCompactRows): a
// world-2 communicator on GPU 0 (PIE_RCCL_LIB = the one-GPU stand-in for RCCL) holds the 1 000-row synthetic table; the lists
// must be the ones the Python side wrote (PIE_MAINT_EXPECT: {cutoff, now, months, prune, retention, kept, owner}), computed from
// the oracle's copy of the table under the zone this process runs in (TZ).
const assert = require('assert');
const fs = require('fs');
const pieNative = require('../pieNative');
const {createShardedQueue} = require('../shardedQueue');

function main(){
  const want = JSON.parse(fs.readFileSync(process.env.PIE_MAINT_EXPECT, 'utf8'));
  const native = pieNative.load();
  const comm = native.commCreate(new Int32Array(2));
  native.commGenSyntheticSharded(comm, 0x5EED5EEDn, want.rows, want.users, 32, 0);
  const q = createShardedQueue(native, comm);
  const owners = got => Array.from(got.rank);
  const ownerOf = rows => rows.map(g => want.owner[g]);

  const pruned = q.pruneBefore(want.cutoff);
  assert.deepStrictEqual(Array.from(pruned.rows), want.prune);
  assert.deepStrictEqual(owners(pruned), ownerOf(want.prune));
  // the list is the source's last queue: its rows can be fetched, and they are tombstones now
  const cols = q.fetchRows(pruned.rows);
  assert.ok(cols.end.every(e => e === -(2n ** 63n)) && cols.start.every(s => s < BigInt(want.cutoff)));
  assert.strictEqual(q.pruneBefore(want.cutoff).rows.length, 0);

  const purged = q.purgeRetention(want.now, want.months);
  assert.deepStrictEqual(Array.from(purged.rows), want.retention);
  assert.deepStrictEqual(owners(purged), ownerOf(want.retention));

  const size = native.commTableSize(comm);
  const c = q.compact(undefined, {shrink: true});
  assert.strictEqual(c.kept, want.kept);
  assert.strictEqual(c.keptLocal.reduce((a, b) => a + b, 0), want.kept);
  assert.deepStrictEqual(native.commTableSize(comm), size);
  assert.strictEqual(q.tableRows(), want.kept);
  // global rows keep their numbers: what is left expires under them
  const left = q.expiredRows(null, Number.MAX_SAFE_INTEGER);
  assert.deepStrictEqual(Array.from(left), want.left);
  const after = q.fetchRows(left);
  assert.deepStrictEqual(Array.from(after.user), want.left.map(g => want.user[g]));
  assert.strictEqual(q.compact().kept, want.kept);
  native.commDestroy(comm);
  console.log('host comm_maint_test ok');
}

main();
