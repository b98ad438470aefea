'use strict';
// GPU: one turn of 300 distinct request groups through sessionStore + feedService({wide: true}) runs in ONE device pass
// (batchesRun = 1), and every response body is byte-identical to the default service's.
const assert = require('assert');
const {createStore} = require('../sessionStore');
const {createFeedService} = require('../feedService');
const dc = require('../disciplineConfig');

let fakeNow = 0;
Date.now = () => fakeNow;

const store = createStore();
const base = 1780000000000;
for(let i = 0; i < 6000; i++){
  fakeNow = base + i * 977;
  store.createSession('user-' + (i % 53), dc.DISCIPLINES[i % dc.DISCIPLINES.length].id);
}
const t1 = base + 6000 * 977 + 5;
const requests = [];
for(let g = 0; g < 300; g++){
  const q = {now: t1 - g * 977 - (g % 3) * 3600 * 1000, cutoff: base + (g % 4) * 100000, disciplines: g % 5 === 0 ? ['drones', 'audio'] : undefined};
  requests.push({userId: 'user-' + (g % 53), query: q});
  if(g % 7 === 0){ requests.push({userId: 'user-' + ((g + 11) % 53), query: q}); }
}
requests.push({userId: 'nobody', query: {now: t1, cutoff: 0}});
fakeNow = t1;
const wide = createFeedService(store, {wide: true});
const bodies = wide.eventsJsonForRequests(requests);
assert.strictEqual(wide.batchesRun(), 1);
const plain = createFeedService(store);
const want = plain.eventsJsonForRequests(requests);
assert.strictEqual(plain.batchesRun(), 5);                     // 301 groups, 64 per ordinary batch
let nonEmpty = 0;
requests.forEach((r, i) => {
  assert.ok(bodies[i].equals(want[i]), 'request ' + i);
  if(bodies[i].length > 13){ nonEmpty++; }
});
assert.ok(nonEmpty > 100, 'most requests have events (' + nonEmpty + ')');
assert.strictEqual(bodies[bodies.length - 1].toString(), '{"events":[]}');
store.close();
console.log('gpu_wide_test ok: ' + requests.length + ' requests, ' + nonEmpty + ' with events, one wide pass');
