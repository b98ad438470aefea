"""GPU: the edges of the key-stream walk (pie_kernels.h walk_key_stream) as the three passes that share it see them — a single
keyed scan, a 16-query batch and a 65-query wide batch, on the 1-byte and on the 2-byte key, at every chunk interleave
(PIE_RUN_SHIFT 0..3) — against the oracle on the same columns.

A chunk is one 16-byte load per lane of a wave.  The table sizes sit on its edges: the ragged tail alone, exactly one chunk, a
tail of one and of two wave-steps behind a full chunk, one wave's whole unroll, and a size at which, with the grid held to two
blocks, every wave goes twice round the outer loop, the last round is cut short by the end of the table, and a ragged tail
follows.  The live rows are the first and the last row of every chunk and of the tail plus a seeded handful: a chunk that is
skipped, read twice or read at the wrong place changes the answer of every query.  One row ends exactly on a query's `now`,
one a millisecond later (the key alone cannot tell them apart).

How the width is pinned: single scans by set_scan_form; batches read the 1-byte key whenever every query lies above its base,
which these do.  On freshly built keys a query below that base always counts as dense (the base is the 90th percentile of `end`,
so a tenth of the table lives above it) and leaves the batch, so a sparse batch is held on the 2-byte key the other way the
library offers: a context created with PIE_K1_KEYED=0x485.  PIE_HOT_INDEX=0 keeps the batched 1-byte pass on the key column."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT64_MIN = -(2 ** 63)
ALL = 2 ** 64 - 1
DAY = 86400 * 1000
HOUR = 3600 * 1000
U, D = 1009, 32
UNROLL = 8                      # the loads a wave keeps in flight in the forms used here (bit 0x80 of 0x485 / 0xC85 / 0x1485)
N_BATCH, N_WIDE = 16, 65
UNION_SLOTS = 16                # union bucket slots per user before any batch has asked for more


def kernel_constants():
    """the `constexpr int` constants of pie_kernels.h that are plain arithmetic on earlier ones"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sph-pie_amd", "csrc", "pie_kernels.h")).read()
    env = {}
    for name, expr in re.findall(r"^constexpr int (k\w+) = ([^;]+);", src, re.M):
        try:
            env[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(env)))
        except Exception:
            pass
    return env


K = kernel_constants()
CHUNK = {1: K["kFineKeyRowsPerLoad"], 2: K["kKeyRowsPerLoad"]}   # rows per chunk, by key width in bytes
WAVE, WAVES = K["kWave"], K["kK1Waves"]
BLOCKS = 2                                                       # PIE_K1_BLOCKS_FINE / _KEYED below


def sizes(width):
    c = CHUNK[width]
    return [c - 37, c, c + 1, c + WAVE + 1, UNROLL * c, 2 * (BLOCKS * WAVES * UNROLL * c) + c + 37]


def queries_for(oracle):
    """65 sparse queries, every `now` its own, spread over an hour (the live rows' ends are spread over three around it)"""
    t0 = oracle.T0_MS
    masks = [0x5555555555555555, 0xAAAAAAAAAAAAAAAA, ALL, 0x00000000FFFF0000, 0x1, 0x8000000000000001]
    return [(t0 - 2 * HOUR + q * (HOUR // N_WIDE) + q % 3, t0 - (61 + q % 4) * DAY - 13 * q, masks[q % len(masks)]) for q in range(N_WIDE)]


_tables = {}


def table(oracle, width, n):
    """-> (columns, queries, oracle answers), built once per (width, n) and shared by every interleave"""
    if (width, n) in _tables:
        return _tables[(width, n)]
    t0, c = oracle.T0_MS, CHUNK[width]
    rng = np.random.default_rng(1000 * width + n)
    qs = queries_for(oracle)
    full = n // c
    edges = [k * c for k in range(full)] + [k * c + c - 1 for k in range(full)]
    if n % c:
        edges += [full * c, n - 1]
    extra = [int(r) for r in rng.choice(n, 7, replace=False)]
    live = np.unique(np.array(edges + extra, np.int64))
    assert live.size * 10 < n, "the live share stays below the tenth at which a query goes to the general path"
    end = rng.integers(t0 - 30 * DAY, t0 - 10 * DAY, n).astype(np.int64)
    end[live] = t0 - 2 * HOUR + rng.integers(1, 3 * HOUR, live.size)
    end[extra[0]] = qs[0][0]            # ends exactly on a query's now: not live for it, and its key is that query's key
    end[extra[1]] = qs[5][0] + 1        # live by a millisecond
    start = (t0 - rng.integers(DAY, 120 * DAY, n)).astype(np.int64)
    user = rng.integers(0, U, n).astype(np.int32)
    disc = rng.integers(0, D, n).astype(np.int32)
    cols = (start, end, user, disc)
    lim = (1 << D) - 1
    want = [oracle.scan(start, end, user, disc, U, now, cutoff, mask & lim) for now, cutoff, mask in qs]
    assert sum(int(w[2].size) for w in want) > 0
    # every user's union fits the slots a fresh context gives it: no batch reruns its queries on the general path
    assert np.bincount(user[live], minlength=U).max() <= UNION_SLOTS
    _tables[(width, n)] = (cols, qs, want, int(live.size))
    return _tables[(width, n)]


def assert_same(got, want, tag):
    for name, a, b in zip(("counts", "offsets", "idx"), got, want):
        assert a.dtype == b.dtype, (tag, name)
        assert np.array_equal(a, b), (tag, name)


@pytest.mark.parametrize("run_shift", [0, 1, 2, 3])
@pytest.mark.parametrize("width", [1, 2])
def test_walk_edges(pie, oracle, monkeypatch, width, run_shift):
    monkeypatch.setenv("PIE_RUN_SHIFT", str(run_shift))            # read when the context is created
    monkeypatch.setenv("PIE_HOT_INDEX", "0")
    if width == 2:
        monkeypatch.setenv("PIE_K1_KEYED", "0x485")
    monkeypatch.setenv("PIE_K1_BLOCKS_FINE", str(BLOCKS))          # read whenever a table is loaded
    monkeypatch.setenv("PIE_K1_BLOCKS_KEYED", str(BLOCKS))
    form = 0xC85 if width == 1 else 0x485
    batch_form = 0x1485 | (0x800 if width == 1 else 0)
    with pie.PieScan(0) as ctx:
        for n in sizes(width):
            cols, qs, want, n_live = table(oracle, width, n)
            tag = "width %d, interleave %d, n %d" % (width, run_shift, n)
            blocks = min(BLOCKS, -(-n // (CHUNK[width] * UNROLL * WAVES)))
            # the rows a pass takes off the key stream: at least those live for its earliest query, at most the rows that end near it
            live_first = int((cols[1] > qs[0][0]).sum())
            ctx.load_columns(*cols, U)

            # a single keyed scan
            ctx.set_scan_form(form)
            for q in (0, 5, N_WIDE - 1):
                ctx.set_disciplines(qs[q][2], D)
                assert_same(ctx.scan(qs[q][0], qs[q][1]), want[q], tag + ", single scan of query %d" % q)
                st = ctx.stats()
                print(tag, "single", hex(st["k1_variant"]), st["k1_blocks"], st["candidates"])
                assert st["k1_variant"] == form and st["k1_blocks"] == blocks, tag
                assert int((cols[1] > qs[q][0]).sum()) <= st["candidates"] <= n_live, tag
            ctx.set_scan_form(-1)
            ctx.set_disciplines(ALL, D)

            # a 16-query batch
            got = ctx.scan_batch(qs[:N_BATCH])
            st = ctx.stats()
            print(tag, "batch", hex(st["k1_variant"]), st["k1_blocks"], st["candidates"])
            assert st["k1_variant"] == batch_form and st["k1_blocks"] == blocks, tag
            assert live_first <= st["candidates"] <= n_live, tag
            assert ctx.batch_read_union() is not None, tag + ": the batch kept its union (no query fell back)"
            for q in range(N_BATCH):
                assert_same(got[q], want[q], tag + ", batch query %d" % q)

            # a 65-query wide batch
            ctx.scan_wide_begin(qs)
            ms = ctx.scan_wide_finish()
            st = ctx.stats()
            print(tag, "wide", hex(st["k1_variant"]), st["k1_blocks"], st["candidates"])
            assert st["k1_variant"] == batch_form and st["k1_blocks"] == blocks, tag
            assert live_first <= st["candidates"] <= n_live, tag
            assert ctx.batch_read_union_wide() is not None, tag + ": the wide batch kept its union (no query fell back)"
            assert ms == [int(w[2].size) for w in want], tag
            for q in range(N_WIDE):
                assert_same(ctx.batch_read_results(q), want[q], tag + ", wide query %d" % q)
