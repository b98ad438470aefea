'use strict';
// GPU check of the addon's wide pipelined exchange (commWideStep*): a world-2 communicator on GPU 0 (PIE_RCCL_LIB = the one-GPU
// stand-in for RCCL) runs ONE 512-query wide step over a sharded synthetic table; sampled feeds read from the gathered messages
// (commWideStepReadGathered) must equal the scanWide results of an unsharded context over the same corpus.
process.env.TZ = 'UTC';
const assert = require('assert');
const pieNative = require('../pieNative');

const SEED = 0x5EED5EEDn, T0 = 1700000000000, HOUR = 3600 * 1000, DAY = 24 * HOUR;
const N = 200000, U = 2000, D = 32, NQ = 512, WORLD = 2;

function queries(){
  const masks = [0x55555555n, 0xAAAAAAAAn, 0xFFFFFFFFn, 0xFFFF0000n, 0x1n, 0x80000001n];
  const nows = new BigInt64Array(NQ), cutoffs = new BigInt64Array(NQ), ms = new BigUint64Array(NQ);
  for(let q = 0; q < NQ; q++){
    nows[q] = BigInt(T0 - 6 * HOUR - 977 * q - (q % 3) * HOUR);
    cutoffs[q] = BigInt(T0 - (61 + q % 4) * DAY - 13 * q);
    ms[q] = masks[q % masks.length];
  }
  return {nows, cutoffs, ms};
}

function main(){
  const native = pieNative.load();
  const {nows, cutoffs, ms} = queries();
  // the unsharded table
  const single = native.ctxCreate(0);
  native.genSynthetic(single, SEED, N, 0, N, U, D, 0);
  native.setDisciplines(single, 0xFFFFFFFFn, D);
  const wantM = native.scanWide(single, nows, cutoffs, ms);
  assert.strictEqual(wantM.length, NQ);
  // the sharded one
  const comm = native.commCreate(new Int32Array(WORLD).fill(0));
  assert.strictEqual(native.commWorld(comm), WORLD);
  native.commGenSyntheticSharded(comm, SEED, N, U, D, 0);
  const rowsMap = [], usersMap = [];
  for(let r = 0; r < WORLD; r++){
    const ctx = native.commCtx(comm, r);
    native.setDisciplines(ctx, 0xFFFFFFFFn, D);
    const st = native.stats(ctx);
    const rm = new Int32Array(Number(st.rows)), um = new Int32Array(Number(st.users));
    native.shardMaps(ctx, rm, um);
    rowsMap.push(rm);
    usersMap.push(um);
  }
  // one wide step; repeated while a shard grows its union slots (Mu = -1) or the reservation is too small (code -5 either way)
  native.commWideStepReserve(comm, NQ, 1024);
  let step = -1, got = null, tries = 0;
  for(;;){
    assert.ok(++tries <= 6, 'the wide step did not settle');
    native.commWideStepBegin(comm, nows, cutoffs, ms);
    const m = native.commWideStepFinish(comm);
    for(let q = 0; q < NQ; q++){
      let sum = 0;
      for(let r = 0; r < WORLD; r++){ sum += m[r][q]; }
      assert.strictEqual(sum, wantM[q], 'M of query ' + q);
    }
    try{
      step = native.commWideStepCollect(comm);
      got = m;
      break;
    }catch(err){
      assert.strictEqual(err.code, -5, String(err));
      const mu = native.commWideStepStatus(comm, tries - 1);
      assert.strictEqual(mu.length, WORLD);
      if(Array.from(mu).every(v => v >= 0)){ native.commWideStepReserve(comm, NQ, native.commNeededCap(comm)); }
    }
  }
  assert.ok(got && step === tries - 1);
  const mu = native.commWideStepStatus(comm, step);
  const cap = native.commNeededCap(comm);
  let checks = 0;
  for(let at = 0; at < WORLD; at++){
    const msgs = [];
    for(let r = 0; r < WORLD; r++){
      const uoff = new Int32Array(U + 1), rows = new Int32Array(cap), masks = new BigUint64Array(cap * 8);
      const info = native.commWideStepReadGathered(comm, at, r, step, uoff, rows, masks);
      assert.strictEqual(info.words, 8);
      assert.strictEqual(info.mu, mu[r]);
      msgs.push({uoff, rows, masks, words: info.words});
    }
    const idx = new Int32Array(4096);
    for(let s = 0; s < 400; s++){
      const q = (s * 131 + at * 7) % NQ, g = (s * 977 + 13 * at) % U;
      let r = -1, lu = -1;
      for(let k = 0; k < WORLD && lu < 0; k++){ lu = usersMap[k].indexOf(g); r = k; }
      assert.ok(lu >= 0, 'user ' + g + ' is on no shard');
      const {uoff, rows, masks, words} = msgs[r];
      const feed = [];
      for(let i = uoff[lu]; i < uoff[lu + 1]; i++){
        if((masks[i * words + (q >> 6)] >> BigInt(q & 63)) & 1n){ feed.push(rowsMap[r][rows[i]]); }
      }
      const k = native.batchUserFeed(single, q, g, idx);
      assert.deepStrictEqual(feed, Array.from(idx.subarray(0, k)), 'feed of query ' + q + ', user ' + g);
      checks++;
    }
  }
  // a second communicator with a step of another size in flight does not disturb the first one's bookkeeping
  const other = native.commCreate(new Int32Array(WORLD).fill(0));
  native.commGenSyntheticSharded(other, SEED, 20000, 50, D, 0);
  native.commWideStepReserve(other, 65, 4096);
  native.commWideStepBegin(other, nows.subarray(0, 65), cutoffs.subarray(0, 65), ms.subarray(0, 65));
  native.commWideStepBegin(comm, nows, cutoffs, ms);
  assert.strictEqual(native.commWideStepFinish(other)[0].length, 65);
  assert.strictEqual(native.commWideStepFinish(comm)[0].length, NQ);
  assert.strictEqual(native.commWideStepCollect(comm), step + 1);
  native.commDestroy(other);
  native.commDestroy(comm);
  console.log('host gpu_comm_wide_test ok: ' + checks + ' feeds, step ' + step);
}

main();
