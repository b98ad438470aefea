'use strict';
// GPU check of the addon's step bookkeeping with TWO communicators in one process (commStep*): the n_q of the steps begun and not
// finished is kept per communicator, so A (3 queries) and B (5 queries) finished in the other order each get their own counts,
// and destroying A with a step begun and unfinished leaves B working.  Both are one-shard communicators on GPU 0
// (PIE_RCCL_LIB = the one-GPU stand-in for RCCL) over the same corpus; the counts are those of scanBatch on a single context.
process.env.TZ = 'UTC';
const assert = require('assert');
const pieNative = require('../pieNative');

const SEED = 0x5EED5EEDn, T0 = 1700000000000, HOUR = 3600 * 1000, DAY = 24 * HOUR;
const N = 100000, U = 1000, D = 32;

function queries(k){
  const masks = [0x55555555n, 0xAAAAAAAAn, 0xFFFFFFFFn];
  const nows = new BigInt64Array(k), cutoffs = new BigInt64Array(k), ms = new BigUint64Array(k);
  for(let q = 0; q < k; q++){
    nows[q] = BigInt(T0 - 6 * HOUR - 977 * q);
    cutoffs[q] = BigInt(T0 - (61 + q % 2) * DAY);
    ms[q] = masks[q % masks.length];
  }
  return {nows, cutoffs, ms};
}

function main(){
  const native = pieNative.load();
  const q3 = queries(3), q5 = queries(5);
  const single = native.ctxCreate(0);
  native.genSynthetic(single, SEED, N, 0, N, U, D, 0);
  native.setDisciplines(single, 0xFFFFFFFFn, D);
  const want3 = native.scanBatch(single, q3.nows, q3.cutoffs, q3.ms), want5 = native.scanBatch(single, q5.nows, q5.cutoffs, q5.ms);
  assert.ok(want5.every(m => m > 0));
  const make = () => {
    const comm = native.commCreate(Int32Array.from([0]));
    native.commGenSyntheticSharded(comm, SEED, N, U, D, 0);
    native.setDisciplines(native.commCtx(comm, 0), 0xFFFFFFFFn, D);
    native.commStepReserve(comm, 5, N);
    return comm;
  };
  const A = make(), B = make();
  native.commStepBegin(A, q3.nows, q3.cutoffs, q3.ms);
  native.commStepBegin(B, q5.nows, q5.cutoffs, q5.ms);
  const mB = native.commStepFinish(B), mA = native.commStepFinish(A);
  assert.deepStrictEqual(mB, [want5]);
  assert.deepStrictEqual(mA, [want3]);
  assert.strictEqual(native.commStepCollect(B), 0);
  assert.strictEqual(native.commStepCollect(A), 0);
  // A is destroyed with a step begun and unfinished: B's bookkeeping is untouched
  native.commStepBegin(A, q3.nows, q3.cutoffs, q3.ms);
  native.commDestroy(A);
  assert.throws(() => native.commStepFinish(A), /communicator/);
  native.commStepBegin(B, q5.nows, q5.cutoffs, q5.ms);
  assert.deepStrictEqual(native.commStepFinish(B), [want5]);
  assert.strictEqual(native.commStepCollect(B), 1);
  assert.throws(() => native.commStepFinish(B), e => e.code === -6);
  native.commDestroy(B);
  native.ctxDestroy(single);
  console.log('host gpu_comm_two_test ok');
}

main();
