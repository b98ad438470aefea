'use strict';
// GPU check of store.compactDevice (pie_compact_rows behind the Node host): the same surviving sessions as the host's own
// compact() on a plain store; on a store with a synthetic base the base moves as documented, every live token still resolves and
// its feed is the one served before; createStore({deviceCompact: true}) reaches the same state through the automatic trigger.
const assert = require('assert');
const {createStore} = require('../sessionStore');
const {createFeedService} = require('../feedService');

const realNow = Date.now;
let fakeNow = 1700000000000;
Date.now = () => fakeNow;
const HOUR = 3600000;

// one history, replayed on any store: logins of 40 users over ten hours, touches, single deletes, a user delete, a purge
function history(store, autoOnly){
  const made = [];
  fakeNow = 1700000000000;
  for(let i = 0; i < 6000; i++){
    fakeNow += 6000;
    made.push({user: 'u' + (i % 40), token: store.createSession('u' + (i % 40)).token});
    if(i % 7 === 3){ store.touchSession(made[i - 2].token); }
    if(i % 3 === 0){ store.deleteSession(made[i].token); }
    if(i % 5 === 1 && i > 10){ store.deleteSession(made[i - 9].token); }
  }
  if(!autoOnly){
    store.deleteSessionsForUser('u7');
    fakeNow += 3 * HOUR;                 // the earliest untouched sessions have expired by now
    store.purgeExpiredSessions();
  }
  return made;
}
function sessionsOf(store, made){ return made.map(m => { const s = store.getSession(m.token); return s === null ? null : [s.userId, s.createdAt, s.expiresAt]; }); }
// every user's feed as columns (row numbers differ between stores that compacted differently; the rows themselves must not)
function feedsOf(store, users, query){
  store.scanDevice(query);
  return users.map(id => {
    const u = store.userIndexOf(id);
    if(u < 0){ return []; }
    const cols = store.fetchRows(store.userFeed(u));
    return Array.from(cols.start, (s, i) => [String(s), String(cols.end[i]), cols.disc[i]]);
  });
}
// every user's feed as feedService serves it: the events themselves, less what is derived from the row number (id, title and
// the show number parsed from it) — a compaction renumbers rows and nothing else
function eventsOf(feeds, users, query){
  return users.map(id => feeds.eventsForUser(id, query).map(ev => {
    assert.strictEqual(ev.id, 'session-' + ev.showNumber);
    assert.ok(ev.title.endsWith(' session #' + ev.showNumber));
    const e = Object.assign({}, ev, {name: ev.title.slice(0, ev.title.length - String(ev.showNumber).length)});
    delete e.id; delete e.title; delete e.showNumber;
    return e;
  }));
}
const users40 = Array.from({length: 40}, (_, i) => 'u' + i);

// ---- plain store: compactDevice against the host's compact() for the same history
{
  const a = createStore({compactMinRows: 1 << 30}), b = createStore({compactMinRows: 1 << 30});
  const madeA = history(a), madeB = history(b);
  const q = {now: fakeNow, cutoff: 0};
  const before = feedsOf(a, users40, q);
  a.flush(); a.compact(); a.flush();
  const res = b.compactDevice();
  assert.strictEqual(res.base, 0);
  assert.ok(res.dropped > 1000 && res.kept === b.tableRows() && b.tableRows() === a.tableRows(), 'kept ' + res.kept + ' of ' + madeB.length);
  assert.strictEqual(a.compactions(), 1);
  assert.strictEqual(b.compactions(), 1);
  assert.strictEqual(a.size(), b.size());
  assert.deepStrictEqual(sessionsOf(b, madeB), sessionsOf(a, madeA));
  assert.deepStrictEqual(sessionsOf(b, madeB).filter(s => s !== null).length, b.size());
  const fa = feedsOf(a, users40, q), fb = feedsOf(b, users40, q);
  assert.deepStrictEqual(fb, fa);
  assert.deepStrictEqual(fb, before, 'compaction changed a feed');
  // the store goes on working: new sessions land behind the kept rows, a second compaction with deadBefore drops the expired
  const t = b.createSession('u3').token;
  assert.ok(b.getSession(t) !== null);
  fakeNow += 20 * HOUR;
  const r2 = b.compactDevice({deadBefore: fakeNow, shrink: true});
  assert.strictEqual(r2.kept, 0);
  assert.strictEqual(b.size(), 0);
  assert.strictEqual(b.getSession(t), null);
  const t2 = b.createSession('u5').token;
  assert.deepStrictEqual(feedsOf(b, ['u5', 'u3'], {now: fakeNow, cutoff: 0}).map(f => f.length), [1, 0]);
  assert.ok(b.getSession(t2) !== null);
  a.close(); b.close();
}

// ---- a store with a synthetic base of 10^6 rows
{
  const BASE = 1000000, U = 5000, D = require('../disciplineConfig').DISCIPLINES.length;
  const T0 = 1700000000000;
  fakeNow = T0 - 6 * HOUR;
  const store = createStore({base: {rows: BASE, users: U, disc: D}});
  assert.throws(() => store.compact === undefined || store.deleteSessionsForUser('user-1'), /synthetic base/);
  const feeds = createFeedService(store);
  const made = [];
  for(let i = 0; i < 300; i++){ fakeNow += 1000; made.push({user: 'user-' + (i * 13 % U), token: store.createSession('user-' + (i * 13 % U)).token}); }
  for(let i = 0; i < 300; i += 4){ store.touchSession(made[i].token); }
  for(let i = 1; i < 300; i += 3){ store.deleteSession(made[i].token); made[i].deleted = true; }
  store.flush();
  // tombstone part of the base on the device (setEnd on base rows: the host holds no record of them)
  const dead = new Int32Array(BASE / 4), ends = new BigInt64Array(BASE / 4).fill(-(2n ** 63n));
  for(let i = 0; i < dead.length; i++){ dead[i] = 4 * i + 1; }
  store.native.setEnd(store.ctx, dead, ends);
  const watch = made.filter(m => !m.deleted).map(m => m.user);
  const q = {now: fakeNow, cutoff: 0};
  const before = feedsOf(store, watch, q);
  const eventsBefore = eventsOf(feeds, watch, q);
  assert.deepStrictEqual(eventsBefore.map(ev => ev.map(e => [String(e.startTs), String(e.endTs)])), before.map(f => f.map(r => [r[0], r[1]])));
  assert.ok(before.some(f => f.length > 1), 'the watched users have base rows in their feeds');
  const rowsBefore = store.tableRows();
  const res = store.compactDevice();
  assert.strictEqual(res.base, BASE - dead.length, 'base = kept rows among the old base rows');
  assert.strictEqual(store.baseRows(), res.base);
  assert.strictEqual(res.dropped, 100);
  assert.strictEqual(res.kept, rowsBefore - dead.length - 100);
  assert.strictEqual(store.tableRows(), res.kept);
  for(const m of made){ assert.strictEqual(store.getSession(m.token) === null, m.deleted === true); }
  assert.deepStrictEqual(feedsOf(store, watch, q), before, 'a live feed changed');
  // the SAME feedService object, same query: it must not answer from the scan it shared before the rows were renumbered
  const scansBefore = feeds.scansRun();
  const eventsAfter = eventsOf(feeds, watch, q);
  assert.deepStrictEqual(eventsAfter, eventsBefore, 'a feed served by feedService changed');
  assert.ok(feeds.scansRun() > scansBefore, 'feedService served a scan taken before the compaction');
  assert.ok(eventsAfter.some(ev => ev.length > 1));
  // a second create and scan; a touch of a kept session reaches its NEW row
  fakeNow += 1000;
  const t = store.createSession('user-17').token;
  store.touchSession(made[0].token);
  const f = feedsOf(store, ['user-17', made[0].user], {now: fakeNow, cutoff: 0});
  assert.ok(f[0].length >= 1 && f[1].some(r => r[1] === String(fakeNow + store.SESSION_TTL_MS)));
  assert.ok(store.getSession(t) !== null);
  // no host rows at all: base = n_kept
  const only = createStore({base: {rows: 10000, users: 10, disc: D}});
  const r3 = only.compactDevice({deadBefore: T0 - 30 * 86400000});
  assert.ok(r3.base === r3.kept && r3.kept > 0 && r3.kept < 10000 && r3.dropped === 0);
  only.close();
  store.close();
}

// ---- createStore({deviceCompact: true}): the automatic trigger runs on the device and reaches the host compaction's state
{
  const a = createStore({compactMinRows: 512}), b = createStore({compactMinRows: 512, deviceCompact: true});
  const madeA = history(a, true), madeB = history(b, true);
  // enough deletes that the dead outweigh the live, then a flush: the trigger fires
  for(let i = 0; i < 6000; i++){ if(i % 8 !== 5){ a.deleteSession(madeA[i].token); b.deleteSession(madeB[i].token); } }
  const q = {now: fakeNow, cutoff: 0};
  const fa = feedsOf(a, users40, q), fb = feedsOf(b, users40, q);
  assert.ok(a.compactions() >= 1 && b.compactions() >= 1, 'the automatic compaction ran');
  assert.strictEqual(a.tableRows(), b.tableRows());
  assert.strictEqual(a.size(), b.size());
  assert.deepStrictEqual(fb, fa);
  assert.deepStrictEqual(sessionsOf(b, madeB), sessionsOf(a, madeA));
  a.close(); b.close();
}

Date.now = realNow;
console.log('host gpu_compact_test ok');
