// pie_expq_plan.h — how the in-flight expired-queue pass (pie_expired_queue_begin, pie_expq.h) cuts a table: plain functions, no
// HIP, so a host-only program can check them (tools/expq_plan_check.cpp).
//
// A UNIT is a contiguous, ascending range of rows that one wave walks alone; a wave STEP is what it reads per loop iteration
// (1024 rows: two 16-byte loads per lane of 2-byte keys, or eight of the 8-byte `end` column).  Units are a whole number of
// steps, so every unit starts 16-byte aligned in either column.  The number of units is bounded (kExpqMaxUnits), so the pass's
// scratch (one count and one offset per unit) has one size for every table and is allocated once.  The grid is a small multiple
// of the CU count; its waves take units grid-stride, so any grid covers any table.
#ifndef PIE_EXPQ_PLAN_H
#define PIE_EXPQ_PLAN_H

#include <cstddef>

namespace pie {

constexpr int kExpqStepRows = 1024;      // rows a wave reads per step
constexpr int kExpqMinUnitSteps = 16;    // a unit is at least 16 384 rows (32 KB of keys): the per-unit work amortises its count
constexpr int kExpqMaxUnits = 16384;     // what one 1024-thread block turns into offsets in a single sweep
constexpr int kExpqWaves = 4;            // waves (= units at a time) per block
constexpr int kExpqBlocksPerCu = 2;      // default grid: blocks per CU (PIE_EXPQ_BLOCKS_PER_CU overrides, 1..16)
constexpr long long kExpqMaxRows = (1LL << 31) - 1;

struct ExpqPlan {
    int rows_per_wave_step;
    long long rows_per_unit;
    long long units; // 0 for an empty table
    int blocks;
};

// n outside [0, 2^31 - 1) or n_cus / blocks_per_cu < 1: a plan with units = -1
// max_blocks > 0 caps the grid below that (PIE_EXPQ_MAX_BLOCKS: tests make waves take several units on a small table)
inline ExpqPlan expq_plan_of(long long n, int n_cus, int blocks_per_cu, int max_blocks = 0)
{
    ExpqPlan p;
    p.rows_per_wave_step = kExpqStepRows;
    p.rows_per_unit = (long long)kExpqStepRows * kExpqMinUnitSteps;
    p.units = -1;
    p.blocks = 1;
    if (n < 0 || n >= kExpqMaxRows || n_cus < 1 || blocks_per_cu < 1) return p;
    // the smallest whole number of steps per unit that keeps the units within kExpqMaxUnits
    const long long steps = (n + kExpqStepRows - 1) / kExpqStepRows;
    long long unit_steps = (steps + kExpqMaxUnits - 1) / kExpqMaxUnits;
    if (unit_steps < kExpqMinUnitSteps) unit_steps = kExpqMinUnitSteps;
    p.rows_per_unit = unit_steps * kExpqStepRows;
    p.units = (n + p.rows_per_unit - 1) / p.rows_per_unit;
    long long blocks = (p.units + kExpqWaves - 1) / kExpqWaves;
    const long long most = (long long)n_cus * blocks_per_cu;
    if (blocks > most) blocks = most;
    if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
    if (blocks < 1) blocks = 1;
    p.blocks = (int)blocks;
    return p;
}

// scratch of a pass: [counts int32 x kExpqMaxUnits | offsets int64 x (kExpqMaxUnits + 1) | done counter, padded to 16 B]
struct ExpqScratch {
    size_t counts, offsets, ctl, bytes;
};
inline ExpqScratch expq_scratch_of()
{
    ExpqScratch s;
    s.counts = 0;
    s.offsets = (size_t)kExpqMaxUnits * 4;
    s.ctl = s.offsets + ((size_t)kExpqMaxUnits + 1) * 8;
    s.ctl = (s.ctl + 15) / 16 * 16;
    s.bytes = s.ctl + 16;
    return s;
}

// rows the pass's own queue buffer holds after a begin that asks for cap_rows (never shrinks; 0 stays 0: a counting pass)
inline size_t expq_buffer_rows(size_t have_rows, size_t cap_rows)
{
    if (cap_rows <= have_rows) return have_rows;
    size_t want = have_rows ? have_rows : 4096;
    while (want < cap_rows) want *= 2;
    if (want > (size_t)kExpqMaxRows) want = (size_t)kExpqMaxRows;
    return want;
}

} // namespace pie

#endif
