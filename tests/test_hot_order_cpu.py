"""CPU: the sort key of the slot-ordered hot index (pie_hot_order_key, pie_hot_slot_bits) against numpy, and hist_index — the
key's low bits — as a bijection of the padded user range onto the padded histogram.  Host functions only: no context."""
import numpy as np
import pytest

USERS = [1, 31, 32, 33, 101, 1000]
BINS = [1, 64, 127]


def np_slot_bits(U):
    pad = (U + 31) // 32 * 32
    b = 0
    while (1 << b) < pad:
        b += 1
    return b


def np_slot(u, U):
    """hist_index of pie_kernels.h: user u -> (u mod 32) * T + u / 32, T = ceil(U / 32)."""
    t = (U + 31) // 32
    return (u & 31) * t + (u >> 5)


@pytest.mark.parametrize("U", USERS)
def test_slot_bits(pie, U):
    b = pie.hot_slot_bits(U)
    pad = (U + 31) // 32 * 32
    assert b == np_slot_bits(U)
    assert (1 << b) >= pad and (b == 0 or (1 << (b - 1)) < pad)


@pytest.mark.parametrize("U", USERS)
@pytest.mark.parametrize("bin_", BINS)
def test_key_matches_numpy(pie, U, bin_):
    pad = (U + 31) // 32 * 32
    users = np.arange(pad, dtype=np.int64)
    got = np.array([pie.hot_order_key(bin_, int(u), U) for u in users], dtype=np.int64)
    want = (bin_ << np_slot_bits(U)) | np_slot(users, U)
    assert np.array_equal(got, want)
    # the bin is the key's high part: every key of a bin lies below every key of the next
    assert got.max() < ((bin_ + 1) << np_slot_bits(U)) and got.min() >= (bin_ << np_slot_bits(U))
    # an id outside the padded range (a bad row: the pass counts it and selects nothing) takes slot 0, whatever it is
    for bad in (pad, pad + 7, 2 ** 31 - 1, -1, -(2 ** 31)):
        assert pie.hot_order_key(bin_, bad, U) == bin_ << np_slot_bits(U)


@pytest.mark.parametrize("U", USERS)
def test_hist_index_is_a_bijection_onto_the_padded_range(pie, U):
    pad = (U + 31) // 32 * 32
    mask = (1 << pie.hot_slot_bits(U)) - 1
    slots = np.array([pie.hot_order_key(1, u, U) & mask for u in range(pad)], dtype=np.int64)
    assert np.array_equal(np.sort(slots), np.arange(pad))
    # the users of the table proper keep distinct slots inside it
    assert np.unique(slots[:U]).size == U


def test_order_groups_neighbouring_counters(pie):
    """What the order is for: records sorted by key name ascending counter addresses, so 64 neighbours of a bin that holds
    R records over U users span about 64 U / R counters."""
    U, R = 1000, 800
    rng = np.random.default_rng(3)
    users = rng.integers(0, U, R)
    keys = np.sort(np.array([pie.hot_order_key(5, int(u), U) for u in users], dtype=np.int64))
    slots = keys & ((1 << pie.hot_slot_bits(U)) - 1)
    assert np.all(np.diff(slots) >= 0)
    span = slots[64:] - slots[:-64]
    assert np.median(span) < 2 * 64 * U / R
