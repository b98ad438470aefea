"""CPU: the 20-bit mask code of the batched pass (pie_batch_mask_codes, host only).  The code r | w << 7 | d << 14 of a row,
expanded through the tables the library's own builder makes for a batch, equals the row's 64-bit query mask evaluated directly —
for random queries and rows, the ends of the ranges (r, w in {0, 64}, d = 63), ties, and queries left out of the tables."""
import numpy as np
import pytest

ALL = 2 ** 64 - 1
T0 = 1700000000000


def direct_masks(queries, n_disc, start, end, disc, fallback):
    out = np.zeros(start.size, np.uint64)
    for q, (now, cutoff, mask) in enumerate(queries):
        if fallback is not None and fallback[q]:
            continue
        role = np.array([(mask >> int(x)) & 1 if x < n_disc else 0 for x in disc], bool)
        out[(end > now) & (start >= cutoff) & role] |= np.uint64(1 << q)
    return out


@pytest.mark.parametrize("nq", [1, 2, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("n_disc", [64, 32, 7])
def test_code_expands_to_the_direct_mask(pie, nq, n_disc):
    rng = np.random.default_rng(nq * 100 + n_disc)
    nows = T0 - rng.integers(0, 50, nq) * 977          # with repeats: ties between queries
    cuts = T0 - 10 ** 9 - rng.integers(0, 50, nq) * 13
    masks = [int(x) for x in rng.integers(0, 2 ** 63, nq, dtype=np.uint64) * 2 + rng.integers(0, 2, nq, dtype=np.uint64)]
    masks[0] = ALL
    queries = [(int(nows[q]), int(cuts[q]), masks[q]) for q in range(nq)]
    n = 4000
    # ends / starts on, just around and far from the queries' values
    end = np.concatenate([nows, nows + 1, nows - 1, [nows.max() + 1, nows.min(), -(2 ** 63), 2 ** 63 - 1]])[rng.integers(0, 3 * nq + 4, n)]
    start = np.concatenate([cuts, cuts + 1, cuts - 1, [cuts.min() - 1, cuts.max(), -(2 ** 63), 2 ** 63 - 1]])[rng.integers(0, 3 * nq + 4, n)]
    disc = rng.integers(0, 64, n).astype(np.int32)
    disc[:8] = [0, 31, 32, 63, 63, 63, 0, 63]
    end[:8] = [nows.max() + 1, nows.max() + 1, nows.min(), nows.min(), nows.max() + 1, nows.min() + 1, nows.max() + 1, 2 ** 63 - 1]
    start[:8] = [cuts.max(), cuts.min() - 1, cuts.max(), cuts.min() - 1, cuts.max() + 5, cuts.max(), cuts.min(), 2 ** 63 - 1]
    for fallback in (None, (rng.random(nq) < 0.3).astype(np.uint8)):
        codes, got = pie.batch_mask_codes(queries, n_disc, start, end, disc, fallback)
        assert np.array_equal(got, direct_masks(queries, n_disc, start, end, disc, fallback))
        r, w, d = codes & 127, (codes >> 7) & 127, codes >> 14
        in_tab = nq if fallback is None else int(nq - fallback.sum())
        assert np.array_equal(d, disc) and r.min() == 0 and w.min() == 0 and r.max() == in_tab and w.max() == 64 and d.max() == 63
        # r and w are what the pass computes: the queries (in the tables) with now < end, and with cutoff <= start
        # (the tables hold 64 entries, the unused ones INT64_MAX: a start of INT64_MAX ranks above those too, w = 64 whatever n_q)
        keep = np.ones(nq, bool) if fallback is None else fallback == 0
        cuts64 = np.concatenate([cuts[keep], np.full(64 - in_tab, 2 ** 63 - 1, np.int64)])
        assert np.array_equal(r, (nows[keep][None, :] < end[:, None]).sum(1)) and np.array_equal(w, (cuts64[None, :] <= start[:, None]).sum(1))
        assert w[start < 2 ** 63 - 1].max() == in_tab


def test_argument_errors(pie):
    z8, z4 = np.zeros(1, np.int64), np.zeros(1, np.int32)
    for qs, nd, dd in (([], 64, z4), ([(0, 0, 1)] * 65, 64, z4), ([(0, 0, 1)], 0, z4), ([(0, 0, 1)], 65, z4), ([(0, 0, 1)], 64, z4 + 64)):
        with pytest.raises(pie.PieError):
            pie.batch_mask_codes(qs, nd, z8, z8, dd)
