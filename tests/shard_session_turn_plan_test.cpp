// Stand-alone check of the host-side planning of a turn that logs in on a sharded table (sph-pie_amd/csrc/pie_turn_plan.h, what
// pie_shard_session_turn_plan and pie_shard_session_turn run before anything is staged): every create's GLOBAL row is
// rows_global0 + its ordinal on every shard alike; each create is kept by exactly one rank; a rank's LOCAL rows count its own
// creates only and ascend with the global ones; the new users of a call are dealt to their owners once each; the chains are
// the unsharded plan's.  Built with ASan + UBSan by tests/test_shard_session_turn_cpu.py; no GPU, nothing of it is loaded into
// python.
#include "../sph-pie_amd/csrc/pie_turn_plan.h"

#include <cstdio>
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

static uint64_t rng_state = 0x5AA4D5E5ULL;
static uint64_t rng()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static void check(const std::vector<pie_turn_op>& ops, const std::vector<int32_t>& user, int64_t rows_global0, int32_t world)
{
    const size_t k = ops.size();
    const size_t n_create = session_turn_creates(ops.data(), k);
    std::vector<int> keepers(k, 0);
    std::vector<int32_t> global_first;
    size_t kept_sum = 0;
    for (int32_t rank = 0; rank < world; ++rank) {
        // exact-size heap blocks: a store past either end is ASan's to report
        std::vector<int32_t> row_g(k, 777), row_l(k, 777);
        const int64_t rows_local0 = (int64_t)(rng() % (uint64_t)(rows_global0 + 1));
        size_t n_kept = 12345;
        CHECK(shard_session_turn_rows(ops.data(), k, user.data(), rows_global0, rows_local0, rank, world, row_g.data(), row_l.data(), &n_kept) == n_create);
        CHECK(n_kept == shard_session_turn_kept(ops.data(), k, user.data(), rank, world));
        if (rank == 0) global_first = row_g;
        CHECK(row_g == global_first); // every shard numbers the creates alike
        size_t j = 0, mine = 0;
        for (size_t i = 0; i < k; ++i) {
            const bool create = ops[i].kind == PIE_TURN_CREATE;
            CHECK(row_g[i] == (create ? (int32_t)(rows_global0 + (int64_t)j) : -1));
            const bool keep = create && shard_of(user[i], world) == rank;
            CHECK(row_l[i] == (keep ? (int32_t)(rows_local0 + (int64_t)mine) : -1));
            keepers[i] += keep ? 1 : 0;
            j += create ? 1 : 0;
            mine += keep ? 1 : 0;
        }
        CHECK(mine == n_kept);
        kept_sum += n_kept;
        // NULL outputs are allowed one by one
        CHECK(shard_session_turn_rows(ops.data(), k, user.data(), rows_global0, rows_local0, rank, world, nullptr, nullptr, nullptr) == n_create);
    }
    CHECK(kept_sum == n_create);
    for (size_t i = 0; i < k; ++i) CHECK(keepers[i] == (ops[i].kind == PIE_TURN_CREATE ? 1 : 0));
}

int main()
{
    for (int32_t world : {1, 2, 3, 5}) {
        // the owner function: in range, and 0 for a single shard
        for (int32_t u : {0, 1, 2, 1000, 0x7ffffffe}) CHECK(shard_of(u, world) >= 0 && shard_of(u, world) < world);
        CHECK(shard_of(12345, 1) == 0);
        // new users: every id of [before, after) goes to exactly one rank, ascending
        size_t total = 0;
        for (int32_t rank = 0; rank < world; ++rank) {
            const size_t n = shard_new_users(40, 140, rank, world);
            std::vector<int32_t> ids(n, -5);
            CHECK(shard_new_users(40, 140, rank, world, ids.data()) == n);
            for (size_t i = 0; i < n; ++i) CHECK(ids[i] >= 40 && ids[i] < 140 && shard_of(ids[i], world) == rank && (i == 0 || ids[i] > ids[i - 1]));
            CHECK(shard_new_users(140, 40, rank, world) == 0);
            total += n;
        }
        CHECK(total == 100);
        std::vector<pie_turn_op> ops;
        std::vector<int32_t> user;
        check(ops, user, 100, world); // k = 0
        for (size_t k : {1u, 2u, 64u, 257u, 300u, 5000u}) {
            for (int p_create : {100, 20, 0}) {
                ops.assign(k, pie_turn_op{});
                user.assign(k, 0);
                for (size_t i = 0; i < k; ++i) {
                    ops[i].tok[0] = rng() % 13;
                    ops[i].kind = (int)(rng() % 100) < p_create ? PIE_TURN_CREATE : (int)(rng() % 3);
                    user[i] = (int32_t)(rng() % 997);
                }
                check(ops, user, (int64_t)(rng() % 100000), world);
            }
        }
        ops.assign(2, pie_turn_op{}); // the last rows a table may hold
        ops[0].kind = ops[1].kind = PIE_TURN_CREATE;
        user.assign(2, 3);
        check(ops, user, ((int64_t)1 << 31) - 4, world);
    }
    if (fails) return 1;
    std::printf("shard session turn plan ok\n");
    return 0;
}
