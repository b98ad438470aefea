'use strict';
// CPU: feedService's grouping of one turn's requests over a stub store (no addon, no GPU).  With {wide: true} up to
// store.WIDE_MAX distinct groups go into ONE scanWideDevice call; without it, grouping is unchanged (store.BATCH_MAX per
// scanBatchDevice call).
const assert = require('assert');
const {createFeedService} = require('../feedService');

function stubStore(){
  const calls = [];
  return {
    calls,
    BATCH_MAX: 64,
    WIDE_MAX: 512,
    generation: () => 1,
    userIndexOf: id => (id.startsWith('user-') ? Number(id.slice(5)) : -1),
    scanBatchDevice: qs => { calls.push(['batch', qs.length]); return qs.map(() => 0); },
    scanWideDevice: qs => { calls.push(['wide', qs.length]); return qs.map(() => 0); },
    batchUserFeed: () => new Int32Array(0),
    fetchRows: idx => ({start: new BigInt64Array(idx.length), end: new BigInt64Array(idx.length), user: new Int32Array(idx.length),
      disc: new Int32Array(idx.length)}),
    batchFetch: (qis) => ({off: new BigInt64Array(qis.length + 1), idx: new Int32Array(0), start: new BigInt64Array(0),
      end: new BigInt64Array(0), disc: new Int32Array(0), total: 0}),
  };
}

function requests(nGroups, perGroup){
  const out = [];
  for(let g = 0; g < nGroups; g++){
    for(let k = 0; k < perGroup; k++){
      out.push({userId: 'user-' + ((g * 7 + k) % 50), query: {now: 1780000000000 + g * 977, cutoff: 1770000000000}});
    }
  }
  return out;
}

let checks = 0;
for(const [nGroups, perGroup] of [[1, 1], [64, 2], [65, 1], [300, 2], [512, 1], [513, 1], [1100, 1]]){
  const reqs = requests(nGroups, perGroup);
  // wide: ceil(groups / 512) scanWideDevice calls, no ordinary batch
  const sw = stubStore();
  const fw = createFeedService(sw, {wide: true});
  const bw = fw.eventsJsonForRequests(reqs);
  const wantWide = [];
  for(let at = 0; at < nGroups; at += 512){ wantWide.push(['wide', Math.min(512, nGroups - at)]); }
  assert.deepStrictEqual(sw.calls, wantWide, 'wide ' + nGroups); checks++;
  assert.strictEqual(fw.batchesRun(), wantWide.length); checks++;
  // default: unchanged, 64 groups per ordinary batch
  const sb = stubStore();
  const fb = createFeedService(sb);
  const bb = fb.eventsJsonForRequests(reqs);
  const wantBatch = [];
  for(let at = 0; at < nGroups; at += 64){ wantBatch.push(['batch', Math.min(64, nGroups - at)]); }
  assert.deepStrictEqual(sb.calls, wantBatch, 'default ' + nGroups); checks++;
  assert.strictEqual(fb.batchesRun(), wantBatch.length); checks++;
  assert.strictEqual(bw.length, reqs.length); checks++;
  bw.forEach((b, i) => { assert.ok(b.equals(bb[i]), 'body ' + i); });
  checks++;
}
console.log('wide_cpu_test ok: ' + checks + ' checks');
