// Stand-alone check of the in-flight expired queue's host-side planning (sph-pie_amd/csrc/pie_expq_plan.h): geometry, scratch
// layout and buffer sizing, replayed on a host array the way the kernel indexes the table.  Built with ASan + UBSan by
// tests/test_expired_inflight_abi.py; no GPU, nothing of it is loaded into python.
#include "../sph-pie_amd/csrc/pie_expq_plan.h"

#include <cstdio>
#include <cstdlib>
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

// every row belongs to exactly one unit, units ascend, each starts on a step boundary, and the grid's waves reach all of them
static void check_plan(long long n, int n_cus, int per_cu, int max_blocks, bool walk)
{
    const ExpqPlan p = expq_plan_of(n, n_cus, per_cu, max_blocks);
    CHECK(p.rows_per_wave_step == kExpqStepRows);
    CHECK(p.rows_per_unit % kExpqStepRows == 0 && p.rows_per_unit >= (long long)kExpqStepRows * kExpqMinUnitSteps);
    CHECK(p.units >= 0 && p.units <= kExpqMaxUnits);
    CHECK(p.units * p.rows_per_unit >= n && (p.units == 0 || (p.units - 1) * p.rows_per_unit < n));
    CHECK((n == 0) == (p.units == 0));
    CHECK(p.blocks >= 1 && p.blocks <= n_cus * per_cu && (max_blocks <= 0 || p.blocks <= max_blocks));
    CHECK((long long)p.blocks * kExpqWaves <= p.units + kExpqWaves - 1 || p.blocks == 1);
    if (!walk) return;
    std::vector<unsigned char> seen((size_t)n, 0);
    std::vector<int> count((size_t)p.units, -1);
    const int stride = p.blocks * kExpqWaves;
    for (int w = 0; w < stride; ++w) {
        for (long long u = w; u < p.units; u += stride) {
            const long long w0 = u * p.rows_per_unit;
            long long w1 = w0 + p.rows_per_unit;
            if (w1 > n) w1 = n;
            CHECK(w0 < w1 && w0 % 8 == 0);
            for (long long t = w0; t < w1; t += kExpqStepRows) {
                const long long t1 = t + kExpqStepRows <= w1 ? t + kExpqStepRows : w1;
                for (long long r = t; r < t1; ++r) seen[(size_t)r]++;
            }
            count[(size_t)u] = (int)(w1 - w0);
        }
    }
    long long total = 0;
    for (long long u = 0; u < p.units; ++u) {
        CHECK(count[(size_t)u] > 0);
        total += count[(size_t)u];
    }
    CHECK(total == n);
    for (long long r = 0; r < n; ++r)
        if (seen[(size_t)r] != 1) {
            CHECK(seen[(size_t)r] == 1);
            break;
        }
}

int main()
{
    const long long unit = (long long)kExpqStepRows * kExpqMinUnitSteps;
    const long long small[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, unit - 1, unit, unit + 1, 3 * unit + 777, 6 * unit + 333, 1000003};
    for (long long n : small)
        for (int per_cu : {1, 2, 16})
            for (int max_blocks : {0, 1, 3}) check_plan(n, 256, per_cu, max_blocks, true);
    check_plan(1, 1, 1, 0, true);
    const long long big[] = {100000000LL, (long long)kExpqMaxUnits * unit, (long long)kExpqMaxUnits * unit + 1, kExpqMaxRows - 1};
    for (long long n : big) check_plan(n, 256, 2, 0, false);
    CHECK(expq_plan_of(100000000LL, 256, 2).units == 6104 && expq_plan_of(100000000LL, 256, 2).blocks == 512);
    CHECK(expq_plan_of(kExpqMaxRows - 1, 256, 2).rows_per_unit == 128LL * kExpqStepRows);
    // refused inputs
    CHECK(expq_plan_of(-1, 256, 2).units == -1);
    CHECK(expq_plan_of(kExpqMaxRows, 256, 2).units == -1);
    CHECK(expq_plan_of(10, 0, 2).units == -1 && expq_plan_of(10, 256, 0).units == -1);
    // the scratch: counts, offsets (one more than the counts) and the counter do not overlap and keep their alignment
    const ExpqScratch s = expq_scratch_of();
    CHECK(s.counts == 0 && s.offsets >= (size_t)kExpqMaxUnits * 4 && s.offsets % 8 == 0);
    CHECK(s.ctl >= s.offsets + ((size_t)kExpqMaxUnits + 1) * 8 && s.ctl % 16 == 0 && s.bytes >= s.ctl + 16);
    {
        std::vector<unsigned char> mem(s.bytes, 0);
        int* counts = reinterpret_cast<int*>(mem.data() + s.counts);
        long long* off = reinterpret_cast<long long*>(mem.data() + s.offsets);
        unsigned* ctl = reinterpret_cast<unsigned*>(mem.data() + s.ctl);
        for (int u = 0; u < kExpqMaxUnits; ++u) counts[u] = 1;
        long long run = 0;
        for (int u = 0; u < kExpqMaxUnits; ++u) { off[u] = run; run += counts[u]; }
        off[kExpqMaxUnits] = run;
        ctl[0] = 7;
        CHECK(off[kExpqMaxUnits] == kExpqMaxUnits && counts[kExpqMaxUnits - 1] == 1 && ctl[0] == 7);
    }
    // the buffer never shrinks, holds what was asked, and stays within int32 rows
    CHECK(expq_buffer_rows(0, 0) == 0 && expq_buffer_rows(0, 1) == 4096 && expq_buffer_rows(4096, 4096) == 4096);
    CHECK(expq_buffer_rows(4096, 4097) == 8192 && expq_buffer_rows(8192, 5) == 8192);
    CHECK(expq_buffer_rows(4096, (size_t)kExpqMaxRows) == (size_t)kExpqMaxRows);
    for (size_t have : {(size_t)0, (size_t)4096, (size_t)1 << 20})
        for (size_t want : {(size_t)1, (size_t)4097, (size_t)100000000, (size_t)kExpqMaxRows}) {
            const size_t got = expq_buffer_rows(have, want);
            CHECK(got >= want && got >= have && got <= (size_t)kExpqMaxRows);
        }
    if (fails) return 1;
    std::printf("expq plan ok\n");
    return 0;
}
