'use strict';
// A dispatch-queue source over a SHARDED table: the shape dispatchQueue.js drains (expiredRows / archivedRows / fetchRows /
// userIds) on top of a communicator (pie_comm_*).  The queues are the whole table's — every shard computes its own, the
// communicator merges them on the devices into global rows (pie_comm_expired_queue / pie_comm_archive_queue) — and each row
// comes back with the shard that holds it and its local row there, which is how fetchRows reads it: one pie_fetch_rows per
// source shard with local rows, users mapped back to global ids through the shard's map (pie_shard_maps).  So
// dispatchQueue.dispatchExpiredSessions / dispatchArchivedGroups run unchanged over a sharded table.
//   createShardedQueue(native, comm[, {userIds, windowMs}])
//     native   the addon (pieNative.load())
//     comm     a communicator (native.commCreate) whose shards hold the table (commGenSyntheticSharded, or loaded and sharded)
//     userIds  global user id -> userId string (default: 'user-' + id, the names of a synthetic base)
// expiredRowsInFlight(prevNow, now) is the purge tick of a server that keeps pipelined steps in flight (commStepBegin ...): the
// queue is begun on every shard's side stream (pie_comm_expired_queue_begin), the wait runs on the libuv pool, and the merged
// rows come back with their owning rank; nothing is collected or drained.  The local row of each is found in the shard's row
// map as read at creation, so fetchRows and dispatchQueue.dispatchExpiredSessions work on the result as on expiredRows'.
const SESSION_TTL_MS = 12 * 60 * 60 * 1000;
const END_NONE = -(2n ** 63n);
const PIE_E_CAPACITY = -5;

function createShardedQueue(native, comm, options){
  const opts = options || {};
  const world = native.commWorld(comm);
  const shards = [];
  let totalRows = 0;
  let nUsers = 0;
  // every shard's maps as they stand (at creation, and again after a compaction: the shards' local rows move, global rows do not)
  function readMaps(){
    totalRows = 0;
    for(let r = 0; r < world; r++){
      const ctx = shards[r] ? shards[r].ctx : native.commCtx(comm, r);
      const st = native.stats(ctx);
      const rows = Number(st.rows), users = Number(st.users);
      const rowMap = new Int32Array(Math.max(rows, 1)), userMap = new Int32Array(Math.max(users, 1)).fill(-1);
      native.shardMaps(ctx, rowMap, userMap);
      for(let u = 0; u < users; u++){ nUsers = Math.max(nUsers, userMap[u] + 1); }
      shards[r] = {ctx, users: userMap, rows: rowMap.subarray(0, rows)};
      totalRows += rows;
    }
  }
  readMaps();
  let userIds = opts.userIds || null;

  // the merged queue of the last call and where each row lives
  let cap = 1024;
  let bufRows = new Int32Array(cap), bufRank = new Int32Array(cap), bufLocal = new Int32Array(cap);
  let last = null;                                  // {rows, rank, local}

  function merged(call){
    for(;;){
      try{
        const q = call(bufRows, bufRank, bufLocal);
        last = {rows: bufRows.slice(0, q), rank: bufRank.slice(0, q), local: bufLocal.slice(0, q)};
        return last.rows;
      }catch(err){
        if(err.code !== PIE_E_CAPACITY || cap >= totalRows){ throw err; }
        cap = Math.max(totalRows, 1);               // the queue outgrew the buffers: room for every row, once
        bufRows = new Int32Array(cap); bufRank = new Int32Array(cap); bufLocal = new Int32Array(cap);
      }
    }
  }

  // ascending global rows with prevNow < expiresAt <= now over every shard
  function expiredRows(prevNow, now){
    const prev = prevNow === null || prevNow === undefined ? END_NONE : prevNow;
    return merged((rows, rank, local) => native.commExpiredQueue(comm, prev, now, rows, rank, local));
  }

  let flightRoom = 1024;                            // rows the next in-flight tick makes room for

  // local row of a global row on its shard: the row maps are ascending
  function localRow(rank, g){
    const map = shards[rank].rows;
    let lo = 0, hi = map.length;
    while(lo < hi){
      const mid = (lo + hi) >> 1;
      if(map[mid] < g){ lo = mid + 1; }else{ hi = mid; }
    }
    if(lo >= map.length || map[lo] !== g){ throw new Error('row ' + g + ' is not in the map of rank ' + rank + ' (rows were added after the source was created)'); }
    return lo;
  }

  // the same queue while steps stay in flight -> Promise of the rows; one tick at a time (commExpiredQueueRoom)
  async function expiredRowsInFlight(prevNow, now){
    const prev = prevNow === null || prevNow === undefined ? END_NONE : prevNow;
    let room = Math.min(flightRoom, Math.max(totalRows, 1));
    for(;;){
      native.commExpiredQueueBegin(comm, prev, now, room);
      try{
        const got = await native.commExpiredQueueFinish(comm);
        const local = Int32Array.from(got.rows, (g, i) => localRow(got.owner[i], g));
        last = {rows: got.rows, rank: got.owner, local};
        return last.rows;
      }catch(err){
        if(err.code !== PIE_E_CAPACITY || room >= totalRows){ throw err; }
        room = Math.max(totalRows, 1);              // the queue outgrew its room: the whole table's, once
        flightRoom = Math.max(flightRoom, Number(err.length) * 2); // the next tick asks for twice what this one needed
      }
    }
  }

  // the archive queue of the whole table: users whose earliest session is at least windowMs old, in order of first appearance
  function archivedRows(now, windowMs){
    const w = windowMs === undefined ? (opts.windowMs === undefined ? SESSION_TTL_MS : opts.windowMs) : windowMs;
    return merged((rows, rank, local) => native.commArchiveQueue(comm, now, w, rows, rank, local));
  }

  // ---- a sharded table that ages (pie_comm_prune_before / pie_comm_retention_purge_tz / pie_comm_compact_rows).  The lists are the
  // rows the call tombstoned: ascending global rows with their owning rank (the host drops their token-map entries); they are
  // also the `last` queue, so fetchRows reads them.  A list is never longer than the shards' rows, which is the room offered.
  function maintained(call){
    if(cap < totalRows){
      cap = totalRows;
      bufRows = new Int32Array(cap); bufRank = new Int32Array(cap); bufLocal = new Int32Array(cap);
    }
    const n = call(bufRows, bufRank, bufLocal);
    last = {rows: bufRows.slice(0, n), rank: bufRank.slice(0, n), local: bufLocal.slice(0, n)};
    return {rows: last.rows, rank: last.rank};
  }

  // _pruneCalendarEvents (server/storage/sqlProvider.js:956-968): every row with start < cutoff
  function pruneBefore(cutoff){
    return maintained((rows, rank, local) => native.commPruneBefore(comm, cutoff, rows, rank, local));
  }

  // _purgeExpiredArchives (sqlProvider.js:863-890, 991-1009): every row with now >= addMonths(start, months) on a LOCAL date;
  // zone = {transitions, offsets} (tzTable.buildTzTable), default this process's zone
  function purgeRetention(now, months, zone){
    const tz = zone || require('./tzTable').defaultTzTable();
    const at = now === undefined || now === null ? Date.now() : now;
    return maintained((rows, rank, local) => native.commRetentionPurge(comm, at, months === undefined ? 2 : months, tz.transitions, tz.offsets,
                                                                       rows, rank, local));
  }

  // drop the dead rows on every shard (end <= deadBefore; default: tombstones only).  Global rows keep their numbers; the shards'
  // local rows move, so the maps are read again and the last queue is forgotten.  -> {kept, keptLocal}
  function compact(deadBefore, o){
    const keptLocal = new Int32Array(world);
    const kept = native.commCompactRows(comm, deadBefore === undefined || deadBefore === null ? END_NONE : deadBefore,
                                        Boolean(o && o.shrink), keptLocal);
    last = null;
    readMaps();
    return {kept, keptLocal: Array.from(keptLocal)};
  }

  // columns of global rows of the last queue (any subset, any order): {start, end, user (global id), disc}
  function fetchRows(globalRows){
    const m = globalRows.length;
    const out = {start: new BigInt64Array(m), end: new BigInt64Array(m), user: new Int32Array(m), disc: new Int32Array(m)};
    if(m === 0){ return out; }
    let rank = null, local = null;
    if(last !== null && globalRows === last.rows){
      rank = last.rank; local = last.local;
    }else{
      const at = new Map();
      if(last !== null){ last.rows.forEach((g, i) => at.set(g, i)); }
      rank = new Int32Array(m); local = new Int32Array(m);
      for(let i = 0; i < m; i++){
        const k = at.get(globalRows[i]);
        if(k === undefined){ throw new Error('row ' + globalRows[i] + ' is not in the last queue of this source'); }
        rank[i] = last.rank[k]; local[i] = last.local[k];
      }
    }
    const per = shards.map(() => []);
    for(let i = 0; i < m; i++){ per[rank[i]].push(i); }
    per.forEach((pos, r) => {
      if(pos.length === 0){ return; }
      const k = pos.length;
      const idx = Int32Array.from(pos, i => local[i]);
      const s = new BigInt64Array(k), e = new BigInt64Array(k), u = new Int32Array(k), d = new Int32Array(k);
      native.fetchRows(shards[r].ctx, idx, k, s, e, u, d);
      const users = shards[r].users;
      for(let j = 0; j < k; j++){
        const i = pos[j];
        out.start[i] = s[j]; out.end[i] = e[j]; out.disc[i] = d[j];
        out.user[i] = users[u[j]];
      }
    });
    return out;
  }

  return {
    expiredRows, expiredRowsInFlight, archivedRows, fetchRows, pruneBefore, purgeRetention, compact,
    userIds: () => {
      if(userIds === null){ userIds = Array.from({length: nUsers}, (_, g) => 'user-' + g); }
      return userIds;
    },
    world: () => world,
    tableRows: () => totalRows,
    native
  };
}

module.exports = {createShardedQueue};
