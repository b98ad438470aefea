'use strict';
// Session store with the reference module's interface (server/sessionStore.js:75-84: createSession, getSession, touchSession,
// deleteSession, deleteSessionsForUser, purgeExpiredSessions, SESSION_TTL_MS, SESSION_COOKIE_NAME — synchronous, never throwing
// on a miss, null for "no session") that keeps NO per-session state on the host: no token map, no row mirror.
//
// The sessions are the rows of the device table; the token -> row map is the device's token column and its index (pie_token_*,
// include/pie_scan.h).  Everything is a TURN: an ordered list of create / get / touch / del calls, each with its own clock,
// answered and applied by the device in one upload, one kernel, one download and one wait, with the results the reference gives
// when the calls are made one after another (:12-53).  A turn with a create in it goes through sessionTurn (pie_session_turn:
// the new rows, their keys and the index entries are written by the turn's own kernel), one without through tokenTurn
// (pie_token_turn).  turn(calls) is that list as the caller's event-loop turn collected it; createSession, getSession,
// touchSession and deleteSession are turns of one.  Only the first session of an empty store is made another way: the table and
// the column come with it (loadColumns + tokenSet).
// What the host keeps: the user-id strings (dense int32 <-> userId, as host/sessionStore.js keeps them) and a row count.
//
// A session found expired writes nothing (the reference drops it from its Map, :30-33); the row stays findable and answers
// "no session" at every later clock, which is the same as long as the clocks of one token do not decrease.  purgeExpiredSessions
// turns the expired rows into tombstones, as deleteSession and deleteSessionsForUser do with theirs.
const crypto = require('crypto');
const disciplineConfig = require('./disciplineConfig');
const pieNative = require('./pieNative');
const {keyOfToken} = require('./tokenKeys');

const SESSION_TTL_MS = 12 * 60 * 60 * 1000;
const SESSION_COOKIE_NAME = 'mt_session';
const END_NONE = -(2n ** 63n);          // PIE_END_NONE: tombstone, never live
const KIND = {get: 0, touch: 1, del: 2, create: 3};   // PIE_TURN_GET / _TOUCH / _DELETE / _CREATE

function createStore(options){
  const opts = options || {};
  const native = pieNative.load();                 // throws if the addon / HIP library is missing
  const ctx = native.ctxCreate(opts.device === undefined ? 0 : opts.device);   // throws without a GPU
  if(opts.orderedRun !== undefined){ native.setOrderedRun(ctx, opts.orderedRun); }
  // turnOrdered: a turn with a create in it (createSession is one) keeps a valid ordered run where an append would, instead of
  // dropping it (pie_set_turn_ordered; off by default, PIE_TURN_ORDERED=1 sets the context's own default)
  if(opts.turnOrdered !== undefined){ native.setTurnOrdered(ctx, opts.turnOrdered ? 1 : 0); }
  const userIndex = new Map();                     // userId string -> dense int32
  const userIds = [];                              // dense int32 -> userId string
  let nRows = 0;                                   // rows of the device table = sessions ever created here

  function denseUser(userId){
    let u = userIndex.get(userId);
    if(u === undefined){
      u = userIds.length;
      userIndex.set(userId, u);
      userIds.push(userId);
    }
    return u;
  }

  const discOf = disciplineId => disciplineId === undefined
    ? (disciplineConfig.DEFAULT_DISCIPLINE ? disciplineConfig.disciplineIndex(disciplineConfig.DEFAULT_DISCIPLINE.id) : 0)
    : disciplineConfig.disciplineIndex(disciplineId);

  // the first session of an empty store: the table and the column come with it
  function firstSession(call, clock){
    if(!call.userId){ throw new TypeError('turn: a create carries a userId'); }
    const token = call.token || crypto.randomBytes(48).toString('hex');
    const now = call.now === undefined ? clock : call.now;
    const expiresAt = now + SESSION_TTL_MS;
    const u = Int32Array.of(denseUser(call.userId)), d = Int32Array.of(discOf(call.disciplineId));
    native.loadColumns(ctx, BigInt64Array.of(BigInt(now)), BigInt64Array.of(BigInt(expiresAt)), u, d, userIds.length);
    native.tokenSet(ctx, keyOfToken(token));
    nRows = 1;
    return {token, expiresAt};
  }

  const createSession = (userId, disciplineId) => turn([{op: 'create', userId, disciplineId}])[0];

  // calls: [{op: 'get' | 'touch' | 'del', token, now?} | {op: 'create', userId, disciplineId?, now?, token?}] -> the reference's
  // return values in order: createSession's {token, expiresAt}, getSession's {userId, createdAt, expiresAt} or null,
  // touchSession's {userId, expiresAt} or null, undefined for del.
  // now defaults to Date.now() at the time of this call; a falsy token is answered on the host (null / no-op, :22, :48).  A
  // create's token defaults to 48 random bytes in hex (:13); the field exists so that a test can replay a recorded trace.
  function packTurn(calls){
    const results = new Array(calls.length);
    const sent = [];                               // positions of the calls that go to the device
    let creates = 0;
    for(let i = 0; i < calls.length; i++){
      if(KIND[calls[i].op] === undefined){ throw new TypeError('turn: op is create, get, touch or del'); }
      if(calls[i].op === 'create' && !calls[i].userId){ throw new TypeError('turn: a create carries a userId'); }
      results[i] = calls[i].op === 'del' ? undefined : null;
      if(calls[i].op === 'create'){ creates++; sent.push(i); }
      else if(calls[i].token && nRows > 0){ sent.push(i); }
    }
    const k = sent.length;
    const clock = Date.now();
    const keys = new BigUint64Array(2 * k), nows = new BigInt64Array(k), newEnds = new BigInt64Array(k), kinds = new Uint8Array(k);
    const users = creates ? new Int32Array(k) : null, discs = creates ? new Int32Array(k) : null;
    for(let j = 0; j < k; j++){
      const c = calls[sent[j]];
      const now = c.now === undefined ? clock : c.now;
      let token = c.token;
      if(c.op === 'create'){
        token = token || crypto.randomBytes(48).toString('hex');
        users[j] = denseUser(c.userId);
        discs[j] = discOf(c.disciplineId);
        results[sent[j]] = {token, expiresAt: now + SESSION_TTL_MS};
      }
      keys.set(keyOfToken(token), 2 * j);
      nows[j] = BigInt(now);
      kinds[j] = KIND[c.op];
      newEnds[j] = c.op === 'touch' || c.op === 'create' ? BigInt(now + SESSION_TTL_MS) : 0n;
    }
    return {results, sent, keys, nows, newEnds, kinds, users, discs, creates};
  }

  function unpackTurn(p, got){
    for(let j = 0; j < p.sent.length; j++){
      if(got.live[j] !== 1 || p.kinds[j] === KIND.create){
        continue;                                  // unknown, expired or deleted: null (undefined for del) stands; a create has its answer
      }
      const userId = userIds[got.user[j]];
      p.results[p.sent[j]] = p.kinds[j] === KIND.get ? {userId, createdAt: Number(got.start[j]), expiresAt: Number(got.end[j])}
                                                     : {userId, expiresAt: Number(got.end[j])};
    }
    return p.results;
  }

  function turn(calls){
    if(nRows === 0){                               // nothing to find yet: everything ahead of the first create answers on the host
      const first = calls.findIndex(c => c.op === 'create');
      if(first >= 0){
        const ahead = packTurn(calls.slice(0, first)).results;
        const made = firstSession(calls[first], Date.now());
        return ahead.concat([made], turn(calls.slice(first + 1)));
      }
    }
    const p = packTurn(calls);
    if(p.sent.length === 0){
      return p.results;
    }
    if(p.creates === 0){
      return unpackTurn(p, native.tokenTurn(ctx, p.keys, p.nows, p.newEnds, p.kinds));
    }
    const got = native.sessionTurn(ctx, p.keys, p.nows, p.newEnds, p.kinds, p.users, p.discs, userIds.length);
    nRows += p.creates;
    return unpackTurn(p, got);
  }

  // The same list while scans and batches are in flight on this context (pie_token_turn_begin / _finish): the turn is queued
  // behind what was begun before it and ahead of what is begun after it, and the wait runs on the libuv pool.  -> Promise of
  // what turn(calls) returns.  With no slot free (four turns begun and not finished) it is the synchronous turn, which needs
  // nothing in flight.  A list with a create in it is the synchronous turn too: logins while batches are in flight are not
  // built yet (pie_token_turn_begin takes no create op).
  let turnsInFlight = 0;
  async function turnAsync(calls){
    if(calls.some(c => c.op === 'create')){
      return turn(calls);
    }
    const p = packTurn(calls);
    if(p.sent.length === 0){
      return p.results;
    }
    if(native.tokenTurnRoom(ctx) <= 0){
      return unpackTurn(p, native.tokenTurn(ctx, p.keys, p.nows, p.newEnds, p.kinds));
    }
    native.tokenTurnBegin(ctx, p.keys, p.nows, p.newEnds, p.kinds);
    turnsInFlight++;
    return unpackTurn(p, await native.tokenTurnFinish(ctx));
  }

  const getSession = token => turn([{op: 'get', token}])[0];
  const touchSession = token => turn([{op: 'touch', token}])[0];
  const deleteSession = token => { turn([{op: 'del', token}]); };

  // full-table scan on the device (user == x, strict); the rows it tombstones are nobody's to remember here
  function deleteSessionsForUser(userId){
    if(!userId || nRows === 0){
      return;
    }
    const u = userIndex.get(userId);
    if(u === undefined){
      return;
    }
    native.deleteUser(ctx, u, new Int32Array(nRows));
  }

  // `now` is sampled once (:67); every row with end <= now that is not a tombstone becomes one
  function purgeExpiredSessions(){
    if(nRows === 0){
      return undefined;
    }
    const list = new Int32Array(nRows);
    const k = native.expiredQueue(ctx, END_NONE, Date.now(), list);
    if(k > 0){
      native.setEnd(ctx, list.subarray(0, k), new BigInt64Array(k).fill(END_NONE));
    }
    return undefined;
  }

  function close(){
    native.ctxDestroy(ctx);
  }

  return {
    createSession, getSession, touchSession, deleteSession, deleteSessionsForUser, purgeExpiredSessions, turn, turnAsync,
    turnsInFlight: () => turnsInFlight,
    SESSION_TTL_MS, SESSION_COOKIE_NAME,
    tableRows: () => nRows,
    userIds: () => userIds,
    close, native, ctx
  };
}

// module-level singleton with the reference's export names; created on first use so that requiring this file
// on a machine without a GPU fails at the first call, with the library's own error text.
let shared = null;
function store(){
  if(shared === null){
    shared = createStore();
  }
  return shared;
}

module.exports = {
  createSession: (userId, disciplineId) => store().createSession(userId, disciplineId),
  getSession: token => store().getSession(token),
  touchSession: token => store().touchSession(token),
  deleteSession: token => store().deleteSession(token),
  deleteSessionsForUser: userId => store().deleteSessionsForUser(userId),
  purgeExpiredSessions: () => store().purgeExpiredSessions(),
  turn: calls => store().turn(calls),
  turnAsync: calls => store().turnAsync(calls),
  SESSION_TTL_MS,
  SESSION_COOKIE_NAME,
  createStore,
  sharedStore: store
};
