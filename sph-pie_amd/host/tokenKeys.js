'use strict';
// Token keys of the device token index (pie_token_*, include/pie_scan.h): the first 16 bytes of the sha256 the reference keys
// its session Map by (server/sessionStore.js:8-10), as two little-endian 64-bit words.  The same rule as binding.token_key.
const crypto = require('crypto');

// -> BigUint64Array(2)
function keyOfToken(token){
  const digest = crypto.createHash('sha256').update(token).digest();
  return BigUint64Array.of(digest.readBigUInt64LE(0), digest.readBigUInt64LE(8));
}

// -> BigUint64Array(2 * tokens.length): the form tokenSet / tokenAppend / tokenLookup / tokenSetEnd of the addon take
function keysOfTokens(tokens){
  const keys = new BigUint64Array(2 * tokens.length);
  for(let i = 0; i < tokens.length; i++){
    const digest = crypto.createHash('sha256').update(tokens[i]).digest();
    keys[2 * i] = digest.readBigUInt64LE(0);
    keys[2 * i + 1] = digest.readBigUInt64LE(8);
  }
  return keys;
}

module.exports = {keyOfToken, keysOfTokens};
