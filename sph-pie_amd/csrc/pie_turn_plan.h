// pie_turn_plan.h — how a turn (pie_token_turn, pie_session_turn; include/pie_scan.h) is cut into chains: plain functions, no HIP, so a host-only
// program can check them (tests/turn_plan_test.cpp).
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

} // namespace pie
#endif /* PIE_TURN_PLAN_H */
