// pie_turn_plan.h — how a turn (pie_token_turn, pie_session_turn, pie_shard_session_turn; include/pie_scan.h) is cut into chains: plain
// functions, no HIP, so a host-only program can check them (tests/turn_plan_test.cpp).
//
// The ops of a turn that name one key form a CHAIN in array order; ops with different keys never interact.  next[i] = the next op
// with op i's key (or -1), head[i] = 1 iff no earlier op has it.  The device gives the head of every chain one lane, which walks
// the chain through next[].  One pass over the ops through an open-addressed table of "last op seen with this key", at most half
// full, sized by k alone (as set_end_last_writers sizes its table); `slots` is scratch the caller keeps between calls.
#ifndef PIE_TURN_PLAN_H
#define PIE_TURN_PLAN_H

#include "../../include/pie_scan.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace pie {

static_assert(sizeof(pie_turn_op) == 40, "pie_turn_op is 40 bytes without padding: the device reads the array as uploaded");

// kind in {GET, TOUCH, DELETE} and reserved == 0 for every op -> the index of the first op that fails, or k
inline size_t turn_first_bad(const pie_turn_op* ops, size_t k)
{
    for (size_t i = 0; i < k; ++i)
        if (ops[i].kind < PIE_TURN_GET || ops[i].kind > PIE_TURN_DELETE || ops[i].reserved != 0) return i;
    return k;
}

// k < 2^31 (checked by the caller).  -> false: out of memory (nothing useful in the outputs)
inline bool turn_plan(const pie_turn_op* ops, size_t k, int32_t* next, uint8_t* head, std::vector<int32_t>& slots)
{
    if (k == 0) return true;
    int bits = 4;
    while (bits < 32 && ((size_t)1 << bits) < 2 * k) ++bits;
    const size_t n_slots = (size_t)1 << bits, mask = n_slots - 1;
    try {
        slots.assign(n_slots, -1);
    } catch (...) {
        return false;
    }
    int32_t* const tab = slots.data();
    for (size_t i = 0; i < k; ++i) {
        const uint64_t k0 = ops[i].tok[0], k1 = ops[i].tok[1];
        size_t at = (size_t)(((k0 ^ ((k1 << 32) | (k1 >> 32))) * 0x9E3779B97F4A7C15ULL) >> (64 - bits));
        while (tab[at] >= 0 && (ops[tab[at]].tok[0] != k0 || ops[tab[at]].tok[1] != k1)) at = (at + 1) & mask;
        next[i] = -1;
        head[i] = tab[at] < 0 ? 1 : 0;
        if (tab[at] >= 0) next[tab[at]] = (int32_t)i; // the op that was last under this key is followed by this one
        tab[at] = (int32_t)i;
    }
    return true;
}

// ---- a turn that logs in (pie_session_turn): kind PIE_TURN_CREATE joins the three above.  The chains are the same chains (a
// create is one more op of its key's chain); what the plan adds is the row every create gets, with no device atomic: the j-th
// create of the array, counting from 0, becomes row row0 + j.

// kind in {GET, TOUCH, DELETE, CREATE} and reserved == 0 for every op -> the index of the first op that fails, or k
inline size_t session_turn_first_bad(const pie_turn_op* ops, size_t k)
{
    for (size_t i = 0; i < k; ++i)
        if (ops[i].kind < PIE_TURN_GET || ops[i].kind > PIE_TURN_CREATE || ops[i].reserved != 0) return i;
    return k;
}

inline size_t session_turn_creates(const pie_turn_op* ops, size_t k)
{
    size_t n = 0;
    for (size_t i = 0; i < k; ++i) n += ops[i].kind == PIE_TURN_CREATE ? 1 : 0;
    return n;
}

// new_row[i] = row0 + (creates before op i) for a create, -1 otherwise -> the number of creates.  The caller has checked that
// row0 + the creates stays below 2^31 - 1.
inline size_t session_turn_rows(const pie_turn_op* ops, size_t k, int64_t row0, int32_t* new_row)
{
    size_t j = 0;
    for (size_t i = 0; i < k; ++i) new_row[i] = ops[i].kind == PIE_TURN_CREATE ? (int32_t)(row0 + (int64_t)j++) : -1;
    return j;
}

// ---- the shard form (pie_shard_session_turn): every shard is given the same turn.  The j-th create of the array becomes GLOBAL
// row rows_global0 + j on every shard alike; the shard its user hashes to keeps it, as LOCAL row rows_local0 + (the creates this
// shard kept before it).  Pure arithmetic again: no shard asks another, and no device atomic.

// the owner of a user among `world` shards: the splitmix64 finaliser over the id (pie_shard_of is this function)
inline int32_t shard_of(int32_t user, int32_t world)
{
    if (world <= 1) return 0;
    uint64_t z = (uint64_t)(uint32_t)user + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (int32_t)(z % (uint64_t)world);
}

// creates of the turn whose user hashes to `rank` (user_global is read at CREATE ops only)
inline size_t shard_session_turn_kept(const pie_turn_op* ops, size_t k, const int32_t* user_global, int32_t rank, int32_t world)
{
    size_t n = 0;
    for (size_t i = 0; i < k; ++i) n += ops[i].kind == PIE_TURN_CREATE && shard_of(user_global[i], world) == rank ? 1 : 0;
    return n;
}

// users of [users_before, users_after) that hash to `rank`: the ids a call that grows the user count adds to the shard's user map
inline size_t shard_new_users(int32_t users_before, int32_t users_after, int32_t rank, int32_t world, int32_t* out = nullptr)
{
    size_t n = 0;
    for (int32_t u = users_before; u < users_after; ++u)
        if (shard_of(u, world) == rank) {
            if (out) out[n] = u;
            ++n;
        }
    return n;
}

// new_row_global[i] = rows_global0 + (creates before op i) for a create, -1 otherwise; new_row_local[i] = rows_local0 + (kept
// creates before op i) for a create this shard keeps, -1 otherwise.  Either array may be NULL.  -> the number of creates;
// *n_kept = how many of them the shard keeps.  The caller has checked that rows_global0 + the creates stays below 2^31 - 1.
inline size_t shard_session_turn_rows(const pie_turn_op* ops, size_t k, const int32_t* user_global, int64_t rows_global0, int64_t rows_local0,
                                      int32_t rank, int32_t world, int32_t* new_row_global, int32_t* new_row_local, size_t* n_kept)
{
    size_t j = 0, kept = 0;
    for (size_t i = 0; i < k; ++i) {
        const bool create = ops[i].kind == PIE_TURN_CREATE;
        const bool mine = create && shard_of(user_global[i], world) == rank;
        if (new_row_global) new_row_global[i] = create ? (int32_t)(rows_global0 + (int64_t)j) : -1;
        if (new_row_local) new_row_local[i] = mine ? (int32_t)(rows_local0 + (int64_t)kept) : -1;
        j += create ? 1 : 0;
        kept += mine ? 1 : 0;
    }
    if (n_kept) *n_kept = kept;
    return j;
}

} // namespace pie
#endif /* PIE_TURN_PLAN_H */
