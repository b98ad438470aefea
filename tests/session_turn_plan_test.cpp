// Stand-alone check of the host-side planning of a turn that logs in (sph-pie_amd/csrc/pie_turn_plan.h, what
// pie_session_turn_plan and pie_session_turn run before anything is staged): the argument check with the fourth kind, the count
// of creates, the row every create gets, and the chains — unchanged by the kind — walked the way k_session_turn walks them: from
// every head through next[], with the key's current row moving to the new row at each create.  Compared with a std::map that
// applies the ops one by one.  Built with ASan + UBSan by tests/test_session_turn_cpu.py; no GPU, nothing of it is loaded into
// python.
#include "../sph-pie_amd/csrc/pie_turn_plan.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

using namespace pie;

static int fails = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            ++fails;                                                         \
        }                                                                    \
    } while (0)

static uint64_t rng_state = 0x5E5510FULL;
static uint64_t rng()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static pie_turn_op op_of(uint64_t k0, uint64_t k1, int kind)
{
    pie_turn_op o{};
    o.tok[0] = k0;
    o.tok[1] = k1;
    o.now = 1;
    o.kind = kind;
    return o;
}

// `before`: the row every key has before the turn (absent: none)
static void check(const std::vector<pie_turn_op>& ops, int64_t row0, const std::map<std::pair<uint64_t, uint64_t>, int32_t>& before,
                  std::vector<int32_t>& slots)
{
    const size_t k = ops.size();
    // exact-size heap blocks: a store past either end is ASan's to report
    std::vector<int32_t> next(k, 12345), new_row(k, 777);
    std::vector<uint8_t> head(k, 99);
    CHECK(session_turn_first_bad(ops.data(), k) == k);
    CHECK(turn_plan(ops.data(), k, next.data(), head.data(), slots));
    const size_t n_create = session_turn_rows(ops.data(), k, row0, new_row.data());
    CHECK(n_create == session_turn_creates(ops.data(), k));
    // one by one: the row each op acts on, and the rows the creates get
    std::map<std::pair<uint64_t, uint64_t>, int32_t> cur = before;
    std::vector<int32_t> want_acts(k, -1), want_new(k, -1);
    int64_t rows = row0;
    for (size_t i = 0; i < k; ++i) {
        const auto key = std::make_pair(ops[i].tok[0], ops[i].tok[1]);
        if (ops[i].kind == PIE_TURN_CREATE) cur[key] = want_new[i] = (int32_t)rows++;
        const auto it = cur.find(key);
        want_acts[i] = it == cur.end() ? -1 : it->second;
    }
    CHECK(new_row == want_new);
    CHECK((int64_t)n_create == rows - row0);
    // the kernel's walk: one probe at the head, then the row in a register
    std::vector<int32_t> acts(k, -2);
    std::vector<int> seen(k, 0);
    for (size_t t = 0; t < k; ++t) {
        if (!head[t]) continue;
        const auto it = before.find(std::make_pair(ops[t].tok[0], ops[t].tok[1]));
        int32_t row = it == before.end() ? -1 : it->second;
        long long j = (long long)t;
        for (size_t step = 0; step < k; ++step) {
            if (ops[(size_t)j].kind == PIE_TURN_CREATE) row = new_row[(size_t)j];
            acts[(size_t)j] = row;
            ++seen[(size_t)j];
            const long long nx = next[(size_t)j];
            if (nx <= j || nx >= (long long)k) break;
            j = nx;
        }
    }
    for (size_t i = 0; i < k; ++i) CHECK(seen[i] == 1);
    CHECK(acts == want_acts);
}

int main()
{
    std::vector<int32_t> slots; // kept between calls, as the library keeps it
    std::map<std::pair<uint64_t, uint64_t>, int32_t> before;
    std::vector<std::pair<uint64_t, uint64_t>> pool;
    for (int i = 0; i < 13; ++i) pool.push_back(std::make_pair(rng(), rng()));
    pool[1] = std::make_pair(pool[0].second, pool[0].first); // the two words are not interchangeable
    for (int i = 0; i < 6; ++i) before[pool[(size_t)i]] = i * 7; // half the pool has a row already
    std::vector<pie_turn_op> ops;
    check(ops, 100, before, slots); // k = 0
    ops.push_back(op_of(1, 2, PIE_TURN_CREATE)); // k = 1, a create
    check(ops, 0, before, slots);
    ops.assign(300, op_of(0, 0, PIE_TURN_CREATE)); // creates only, distinct keys
    for (size_t i = 0; i < ops.size(); ++i) ops[i].tok[0] = rng();
    check(ops, 2999, before, slots);
    ops.assign(300, op_of(5, 5, PIE_TURN_CREATE)); // creates only, ONE key: a chain of 300 creates
    check(ops, 1, before, slots);
    ops.clear();
    for (int i = 0; i < 256; ++i) ops.push_back(op_of(rng(), rng(), i % 3));
    ops.push_back(op_of(ops[3].tok[0], ops[3].tok[1], PIE_TURN_CREATE)); // 257 ops, the one create is the last op
    check(ops, 50, before, slots);
    for (size_t k : {2u, 7u, 8u, 9u, 255u, 256u, 257u, 5000u}) { // heavy repeats, every kind, sizes around the table's powers of two
        ops.clear();
        for (size_t i = 0; i < k; ++i) {
            const auto& p = pool[rng() % 13];
            ops.push_back(op_of(p.first, p.second, (int)(rng() % 4)));
        }
        check(ops, (int64_t)(rng() % 100000), before, slots);
    }
    // row numbers at the top of the range: the last row a table may hold is 2^31 - 3
    ops.assign(2, op_of(9, 9, PIE_TURN_CREATE));
    check(ops, ((int64_t)1 << 31) - 4, before, slots);
    // the argument check of the ABI: kind 3 passes here, 4 and -1 do not, reserved must be 0
    ops.assign(4, op_of(1, 2, PIE_TURN_GET));
    ops[1].kind = PIE_TURN_CREATE;
    CHECK(session_turn_first_bad(ops.data(), 4) == 4);
    CHECK(turn_first_bad(ops.data(), 4) == 1); // ... and pie_token_turn's check keeps refusing it
    ops[2].kind = 4;
    CHECK(session_turn_first_bad(ops.data(), 4) == 2);
    ops[2].kind = -1;
    CHECK(session_turn_first_bad(ops.data(), 4) == 2);
    ops[2].kind = PIE_TURN_DELETE;
    ops[3].reserved = 1;
    CHECK(session_turn_first_bad(ops.data(), 4) == 3);
    if (fails) return 1;
    std::printf("session turn plan ok\n");
    return 0;
}
