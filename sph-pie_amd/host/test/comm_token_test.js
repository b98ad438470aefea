'use strict';
// GPU check of the token column behind the communicator through the addon (commTokenSet / commTokenAppend / commTokenLookup /
// commTokenSetEnd): a world-2 communicator on GPU 0 (PIE_RCCL_LIB = the one-GPU stand-in for RCCL) over the synthetic table
// the vectors were made for.  The vectors (PIE_TOKEN_VECTORS, a JSON file written by tests/test_node_comm_token.py from the
// unsharded Python model) hold the keys, the calls and the expected answers, 64-bit values as decimal strings.
process.env.TZ = 'UTC';
const assert = require('assert');
const fs = require('fs');
const pieNative = require('../pieNative');

const big = (a) => BigInt64Array.from(a, BigInt);
const keysOf = (a) => BigUint64Array.from(a.flat(), BigInt);
const nums = (a) => Array.from(a, Number);
const strs = (a) => Array.from(a, String);

function main(){
  const v = JSON.parse(fs.readFileSync(process.env.PIE_TOKEN_VECTORS, 'utf8'));
  const native = pieNative.load();
  const comm = native.commCreate(new Int32Array(v.world));
  native.commGenSyntheticSharded(comm, BigInt(v.seed), v.n, v.users, v.disc, 0);
  let checks = 0;

  const lookup = (want) => {
    const got = native.commTokenLookup(comm, keysOf(want.keys), BigInt(want.now));
    assert.deepStrictEqual(nums(got.row), want.row);
    assert.deepStrictEqual(nums(got.live), want.live);
    assert.deepStrictEqual(nums(got.owner), want.owner);
    const found = want.row.map((r) => r >= 0);
    const pick = (a) => a.filter((_, i) => found[i]);
    assert.deepStrictEqual(pick(nums(got.user)), pick(want.user));
    assert.deepStrictEqual(pick(strs(got.start)), pick(want.start));
    assert.deepStrictEqual(pick(strs(got.end)), pick(want.end));
    checks++;
  };

  assert.strictEqual(native.commTokenSet(comm, keysOf(v.set_keys)), v.set_keys.length);
  lookup(v.lookup_after_set);
  const a = v.append;
  assert.strictEqual(native.commAppendRows(comm, big(a.start), big(a.end), Int32Array.from(a.user), Int32Array.from(a.disc), a.n_users), v.n);
  assert.strictEqual(native.commTokenAppend(comm, keysOf(a.keys)), a.keys.length);   // no wait in between
  lookup(v.lookup_after_append);
  const t = v.set_end;
  const rows = native.commTokenSetEnd(comm, keysOf(t.keys), big(t.new_end), BigInt(t.now));
  assert.deepStrictEqual(nums(rows), t.rows);
  checks++;
  lookup(v.lookup_after_set_end);
  // empty calls, and a refused one: keys past the table's end
  assert.strictEqual(native.commTokenLookup(comm, new BigUint64Array(0), 0n).row.length, 0);
  assert.strictEqual(native.commTokenSetEnd(comm, new BigUint64Array(0), new BigInt64Array(0), 0n).length, 0);
  assert.throws(() => native.commTokenAppend(comm, new BigUint64Array(2)), (err) => err.code === -1);
  assert.throws(() => native.commTokenLookup(comm, new BigUint64Array(3), 0n), TypeError);
  lookup(v.lookup_after_set_end);
  native.commDestroy(comm);
  console.log('host comm_token_test ok: ' + checks + ' checks');
}

main();
