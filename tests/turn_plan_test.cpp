// Stand-alone check of a turn's host-side planning (sph-pie_amd/csrc/pie_turn_plan.h): the chains pie_token_turn's kernel walks,
// against a std::map, on five key sets — all distinct, all equal, none, one, heavy repeats — and the walk itself the way the
// kernel does it (from every head through next[], bounded by k).  Built with ASan + UBSan by tests/test_token_turn_cpu.py; no GPU,
// nothing of it is loaded into python.
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

static uint64_t rng_state = 0x5EED5EEDULL;
static uint64_t rng()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static void check(const std::vector<pie_turn_op>& ops, std::vector<int32_t>& slots)
{
    const size_t k = ops.size();
    // exact-size heap blocks: a store past either end is ASan's to report
    std::vector<int32_t> next(k, 12345);
    std::vector<uint8_t> head(k, 99);
    CHECK(turn_plan(ops.data(), k, next.data(), head.data(), slots));
    std::map<std::pair<uint64_t, uint64_t>, size_t> last;
    std::vector<int32_t> want_next(k, -1);
    std::vector<uint8_t> want_head(k, 0);
    for (size_t i = 0; i < k; ++i) {
        const auto key = std::make_pair(ops[i].tok[0], ops[i].tok[1]);
        const auto it = last.find(key);
        if (it == last.end()) want_head[i] = 1;
        else want_next[it->second] = (int32_t)i;
        last[key] = i;
    }
    CHECK(next == want_next);
    CHECK(head == want_head);
    // the kernel's walk: every op is visited exactly once, from the head of its chain, in ascending order
    std::vector<int> seen(k, 0);
    for (size_t t = 0; t < k; ++t) {
        if (!head[t]) continue;
        long long j = (long long)t;
        for (size_t step = 0; step < k; ++step) {
            CHECK(ops[(size_t)j].tok[0] == ops[t].tok[0] && ops[(size_t)j].tok[1] == ops[t].tok[1]);
            ++seen[(size_t)j];
            const long long nx = next[(size_t)j];
            if (nx <= j || nx >= (long long)k) break;
            j = nx;
        }
    }
    for (size_t i = 0; i < k; ++i) CHECK(seen[i] == 1);
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

int main()
{
    std::vector<int32_t> slots; // kept between calls, as the library keeps it
    std::vector<pie_turn_op> ops;
    for (int i = 0; i < 1000; ++i) ops.push_back(op_of(rng(), rng(), i % 3)); // all distinct
    check(ops, slots);
    ops.assign(777, op_of(rng(), rng(), PIE_TURN_TOUCH)); // all equal: one chain of 777
    check(ops, slots);
    ops.clear(); // k = 0
    check(ops, slots);
    ops.push_back(op_of(0, 0, PIE_TURN_GET)); // k = 1
    check(ops, slots);
    std::vector<std::pair<uint64_t, uint64_t>> pool;
    for (int i = 0; i < 13; ++i) pool.push_back(std::make_pair(rng(), rng()));
    pool[1] = std::make_pair(pool[0].second, pool[0].first); // the two words are not interchangeable
    pool[2] = std::make_pair(pool[0].first, pool[3].second); // equal in one word only
    ops.clear();
    for (int i = 0; i < 5000; ++i) {
        const auto& p = pool[rng() % 13];
        ops.push_back(op_of(p.first, p.second, (int)(rng() % 3)));
    }
    check(ops, slots);
    for (size_t k : {2u, 7u, 8u, 9u, 15u, 16u, 17u, 255u, 256u, 257u}) { // sizes around the table's powers of two
        ops.clear();
        for (size_t i = 0; i < k; ++i) ops.push_back(op_of(rng() % 5, 7, PIE_TURN_GET));
        check(ops, slots);
    }
    // the argument check of the ABI
    ops.assign(4, op_of(1, 2, PIE_TURN_GET));
    CHECK(turn_first_bad(ops.data(), 4) == 4);
    ops[2].kind = 3;
    CHECK(turn_first_bad(ops.data(), 4) == 2);
    ops[2].kind = -1;
    CHECK(turn_first_bad(ops.data(), 4) == 2);
    ops[2].kind = PIE_TURN_DELETE;
    ops[3].reserved = 1;
    CHECK(turn_first_bad(ops.data(), 4) == 3);
    if (fails) return 1;
    std::printf("turn plan ok\n");
    return 0;
}
