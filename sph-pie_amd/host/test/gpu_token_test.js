'use strict';
// GPU check of the token index through the addon: tokenSet / tokenLookup / tokenSetEnd / tokenAppend against a JS Map keyed by
// token, the way server/sessionStore.js keys its own; and the three fixed key vectors tests/test_token_cpu.py pins for Python.
const assert = require('assert');
const crypto = require('crypto');
const pieNative = require('../pieNative');
const {keyOfToken, keysOfTokens} = require('../tokenKeys');

const END_NONE = -(2n ** 63n);
const NOW = 1700000000000n, HOUR = 3600000n;

// the vectors of tests/test_token_cpu.py (hashlib)
const VECTORS = [
  ['', 0x141cfc9842c4b0e3n, 0x24b96f99c8f4fb9an],
  ['session-token', 0x91969c4611e901c1n, 0x314305d7500b0471n],
  ['pieé-\u{1F511}', 0x86fff0f17ee33b99n, 0x5f4d0bd5c441f32fn],
];
for(const [token, k0, k1] of VECTORS){
  assert.deepStrictEqual(Array.from(keyOfToken(token)), [k0, k1]);
  assert.deepStrictEqual(Array.from(keysOfTokens(['x', token])).slice(2), [k0, k1]);
}

const native = pieNative.load();
const ctx = native.ctxCreate(0);
const N = 300, U = 20;
const tokens = Array.from({length: N}, () => crypto.randomBytes(48).toString('base64'));
const start = new BigInt64Array(N), end = new BigInt64Array(N), user = new Int32Array(N), disc = new Int32Array(N);
const sessions = new Map();   // token -> row, as the reference's Map holds the session
for(let i = 0; i < N; i++){
  start[i] = NOW - 10n * HOUR + BigInt(i);
  end[i] = i % 3 === 0 ? NOW - BigInt(i) : NOW + HOUR + BigInt(i);   // a third expired (end <= now), row 0 exactly at now
  user[i] = i % U; disc[i] = i % 5;
  sessions.set(tokens[i], i);
}
native.loadColumns(ctx, start, end, user, disc, U);
assert.throws(() => native.tokenLookup(ctx, keysOfTokens(tokens), NOW), e => e.code === -6);   // no column yet
assert.strictEqual(native.tokenSet(ctx, keysOfTokens(tokens)), N);

function check(asked, now){
  const got = native.tokenLookup(ctx, keysOfTokens(asked), now);
  assert.strictEqual(got.row.length, asked.length);
  asked.forEach((t, i) => {
    const row = sessions.has(t) ? sessions.get(t) : -1;
    assert.strictEqual(got.row[i], row, 'row of request ' + i);
    assert.strictEqual(got.live[i], row >= 0 && end[row] > now ? 1 : 0, 'liveness of request ' + i);
    if(row >= 0){
      assert.strictEqual(got.user[i], user[row]);
      assert.strictEqual(got.start[i], start[row]);
      assert.strictEqual(got.end[i], end[row]);
    }
  });
  return got;
}
// hits, misses and expired sessions in one batch
const misses = Array.from({length: 50}, () => crypto.randomBytes(48).toString('base64'));
const got = check(tokens.concat(misses), NOW);
assert.ok(got.live.some(v => v === 1) && got.live.slice(0, N).some(v => v === 0));
assert.strictEqual(native.tokenLookup(ctx, new BigUint64Array(0), NOW).row.length, 0);

// touchSession: live sessions move, expired and unknown ones do not (sessionStore.js:37-45)
{
  const asked = [tokens[1], tokens[3], misses[0], tokens[2]];
  const newEnd = BigInt64Array.from(asked, () => NOW + 12n * HOUR);
  const rows = native.tokenSetEnd(ctx, keysOfTokens(asked), newEnd, NOW);
  assert.deepStrictEqual(Array.from(rows), [1, -1, -1, 2]);
  end[1] = end[2] = NOW + 12n * HOUR;
  check(tokens, NOW);
}
// deleteSession: a tombstone, whatever the session's expiry (now = END_NONE); the row stays findable and is not live
{
  const asked = [tokens[4], tokens[6]];   // row 6 has expired
  const rows = native.tokenSetEnd(ctx, keysOfTokens(asked), new BigInt64Array(2).fill(END_NONE), END_NONE);
  assert.deepStrictEqual(Array.from(rows), [4, 6]);
  end[4] = end[6] = END_NONE;
  const after = check(tokens, NOW);
  assert.strictEqual(after.live[4], 0);
  assert.strictEqual(after.row[6], 6);
  const s = new BigInt64Array(N), e = new BigInt64Array(N), u = new Int32Array(N), d = new Int32Array(N);
  native.readColumns(ctx, s, e, u, d);
  assert.deepStrictEqual(Array.from(e), Array.from(end));
}
// createSession: appendRows + tokenAppend + lookup, nothing waited for in between
{
  const K = 40;
  const fresh = Array.from({length: K}, () => crypto.randomBytes(48).toString('base64'));
  const s = new BigInt64Array(K), e = new BigInt64Array(K), u = new Int32Array(K), d = new Int32Array(K);
  const start2 = new BigInt64Array(N + K), end2 = new BigInt64Array(N + K), user2 = new Int32Array(N + K);
  start2.set(start); end2.set(end); user2.set(user);
  for(let i = 0; i < K; i++){
    s[i] = NOW + BigInt(i); e[i] = NOW + 12n * HOUR + BigInt(i); u[i] = (7 * i) % U; d[i] = i % 5;
    start2[N + i] = s[i]; end2[N + i] = e[i]; user2[N + i] = u[i];
    sessions.set(fresh[i], N + i);
  }
  native.appendRows(ctx, s, e, u, d, U);
  assert.strictEqual(native.tokenAppend(ctx, keysOfTokens(fresh.slice(0, K - 5))), K - 5);
  const gotNew = native.tokenLookup(ctx, keysOfTokens(fresh), NOW);
  for(let i = 0; i < K; i++){
    const covered = i < K - 5;   // the last five rows have no key yet: not findable
    assert.strictEqual(gotNew.row[i], covered ? N + i : -1);
    if(covered){
      assert.strictEqual(gotNew.live[i], 1);
      assert.strictEqual(gotNew.user[i], user2[N + i]);
      assert.strictEqual(gotNew.start[i], start2[N + i]);
      assert.strictEqual(gotNew.end[i], end2[N + i]);
    }
  }
  assert.throws(() => native.tokenAppend(ctx, keysOfTokens(fresh)), e2 => e2.code === -1);   // more keys than rows behind the prefix
  assert.throws(() => native.tokenSet(ctx, new BigUint64Array(3)), TypeError);
}
native.ctxDestroy(ctx);
console.log('host gpu_token_test ok');
