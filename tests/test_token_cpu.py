"""CPU: the host-only parts of the token index (include/pie_scan.h pie_token_*): the slot-count rule, the home-slot mix and the
token key.  No GPU, no context."""
import numpy as np
import pytest

# sha256(token)[:16] as two little-endian words, computed with hashlib; sph-pie_amd/host/test/gpu_token_test.js holds the same
TOKEN_VECTORS = [
    ("", 0x141cfc9842c4b0e3, 0x24b96f99c8f4fb9a),
    ("session-token", 0x91969c4611e901c1, 0x314305d7500b0471),
    ("pieé-\U0001F511", 0x86fff0f17ee33b99, 0x5f4d0bd5c441f32f),
]


def test_slots_for(pie):
    assert pie.token_slots_for(0) == 1024 and pie.token_slots_for(512) == 1024 and pie.token_slots_for(513) == 2048
    sweep = {0, 1, 511, 512, 513, 1023, 1024, 1025, 2 ** 31 - 2}
    for b in range(9, 31):
        sweep |= {2 ** b - 1, 2 ** b, 2 ** b + 1, 3 * 2 ** (b - 1)}
    sweep |= set(int(x) for x in np.random.default_rng(7).integers(0, 2 ** 31 - 2, 2000))
    for covered in sorted(sweep):
        if covered > 2 ** 31 - 2:
            continue
        slots = pie.token_slots_for(covered)
        assert slots & (slots - 1) == 0 and slots >= 1024 and slots >= 2 * covered
        assert slots == 1024 or slots // 2 < 2 * covered, "the smallest such power of two"


def test_homes_in_range_and_deterministic(pie):
    keys = np.random.default_rng(11).integers(0, 2 ** 64, (5000, 2), dtype=np.uint64)
    for log2_slots in (0, 1, 10, 13, 24, 32):
        homes = pie.token_homes(keys, log2_slots)
        assert homes.dtype == np.uint32 and np.all(homes.astype(np.uint64) < np.uint64(2 ** log2_slots))
        assert np.array_equal(homes, pie.token_homes(keys.copy(), log2_slots))
    assert pie.token_homes(np.zeros((0, 2), np.uint64), 10).shape == (0,)
    with pytest.raises(pie.PieError):
        pie.token_homes(keys, 33)


@pytest.mark.parametrize("word", [0, 1])
def test_homes_spread_sequential_keys(pie, word):
    # 10^6 keys that differ in their low bits only, in one word: spreading them is the mix's job.  8192 slots, mean 122.07 per
    # slot; observed largest slot 168 for keys (i, 0) and 166 for (0, i), smallest 85 and 81 (a uniform draw gives about the same).
    n, log2_slots = 10 ** 6, 13
    keys = np.zeros((n, 2), np.uint64)
    keys[:, word] = np.arange(n, dtype=np.uint64)
    counts = np.bincount(pie.token_homes(keys, log2_slots), minlength=2 ** log2_slots)
    print("slot counts: min %d max %d" % (counts.min(), counts.max()))
    assert counts.shape[0] == 2 ** log2_slots and counts.min() > 0, "every slot is some key's home"
    assert counts.max() < 3 * n / 2 ** log2_slots


def test_token_key_vectors(pie):
    for token, k0, k1 in TOKEN_VECTORS:
        for form in (token, token.encode("utf-8")):
            key = pie.token_key(form)
            assert key.dtype == np.uint64 and key.shape == (2,) and (int(key[0]), int(key[1])) == (k0, k1)
