'use strict';
// GPU check of setWideOrdered: a 100-query wide batch on a table whose batches take the ordered run (mode 2) keeps no union
// with the switch off and keeps one with it on; its row count must equal the number the caller derived from the CPU oracle.
// usage: node gpu_wide_ordered_test.js WANT_UNION_ROWS
process.env.TZ = 'UTC';
const assert = require('assert');
const pieNative = require('../pieNative');

const SEED = 0x5EED5EEDn, T0 = 1700000000000, HOUR = 3600 * 1000, DAY = 24 * HOUR;
const N = 200000, U = 2000, D = 32, NQ = 100;

function main(){
  const wantRows = Number(process.argv[2]);
  assert.ok(Number.isInteger(wantRows) && wantRows > 0, 'usage: gpu_wide_ordered_test.js WANT_UNION_ROWS');
  const native = pieNative.load();
  assert.strictEqual(typeof native.setWideOrdered, 'function');
  const masks = [0x55555555n, 0xAAAAAAAAn, 0xFFFFFFFFn, 0xFFFF0000n, 0x1n, 0x80000001n];
  const nows = new BigInt64Array(NQ), cutoffs = new BigInt64Array(NQ), ms = new BigUint64Array(NQ);
  for(let q = 0; q < NQ; q++){
    nows[q] = BigInt(T0 - 6 * HOUR - 977 * q - (q % 3) * HOUR);
    cutoffs[q] = BigInt(T0 - (61 + q % 4) * DAY - 13 * q);
    ms[q] = masks[q % masks.length];
  }
  const ctx = native.ctxCreate(0);
  native.genSynthetic(ctx, SEED, N, 0, N, U, D, 0);
  native.setDisciplines(ctx, 0xFFFFFFFFn, D);
  native.setOrderedRun(ctx, 2);
  native.scanDevice(ctx, T0 - 6 * HOUR, T0 - 61 * DAY);   // builds the run
  const off = native.scanWide(ctx, nows, cutoffs, ms);
  assert.strictEqual(native.wideUnionRows(ctx), -1, 'switch off: no union on the run');
  assert.throws(() => native.setWideOrdered(ctx, 2));
  native.setWideOrdered(ctx, 1);
  const on = native.scanWide(ctx, nows, cutoffs, ms);
  assert.deepStrictEqual(Array.from(on), Array.from(off));
  assert.strictEqual(native.wideUnionRows(ctx), wantRows);
  assert.strictEqual(Number(native.stats(ctx).k1Variant) & 0x3000, 0x3000);
  native.ctxDestroy(ctx);
  console.log('host gpu_wide_ordered_test ok: ' + wantRows + ' union rows');
}

main();
