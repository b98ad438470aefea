"""Host only: split_wide_message (binding.py) takes apart the wide union message
[ uoff[0..u_pad] | Mu | rows[0..cap) | masks[0..cap) as 2 * words int32 per row ] that pie_scan_wide_begin_union and
pie_batch_pack_union_wide_device write.  Messages are built in numpy; no GPU and no native library involved."""
import numpy as np
import pytest


def build_message(rng, users, u_pad, cap, words, mu, guard=7):
    """-> (msg with `guard` guard words behind it, uoff[users + 1], rows[mu], masks[mu, words]); mu = -1: the no-union header"""
    total = u_pad + 2 + cap * (1 + 2 * words)
    msg = np.full(total + guard, -77, np.int32)
    if mu < 0:
        msg[: u_pad + 2] = -1
        return msg, None, None, None
    cuts = np.sort(rng.integers(0, mu + 1, users - 1)) if users > 1 else np.zeros(0, np.int64)
    uoff = np.concatenate([[0], cuts, [mu]]).astype(np.int32)
    rows = rng.integers(0, 2 ** 31 - 1, mu).astype(np.int32)
    masks = rng.integers(0, 2 ** 64, (mu, words), dtype=np.uint64)
    if mu:
        masks[0, :] = np.uint64(2 ** 64 - 1)       # all bits, the sign bits of both int32 halves included
        masks[-1, -1] = np.uint64(1 << 63)
    k = min(mu, cap)
    msg[: users + 1] = uoff
    msg[users + 1: u_pad + 2] = mu                 # uoff[u] = Mu for u >= users, then the Mu word
    msg[u_pad + 2: u_pad + 2 + k] = rows[:k]
    base = u_pad + 2 + cap
    msg[base: base + k * 2 * words] = masks[:k].reshape(-1).view(np.int32)
    return msg, uoff, rows, masks


@pytest.mark.parametrize("words", [1, 5, 8])
@pytest.mark.parametrize("case", ["below", "equal", "above", "none"])
def test_split_wide_message_round_trip(words, case):
    from sph_pie_amd.binding import split_wide_message
    rng = np.random.default_rng(1000 * words + len(case))
    users, u_pad, cap = 37, 41, 50
    mu = {"below": 23, "equal": cap, "above": cap + 19, "none": -1}[case]
    msg, uoff, rows, masks = build_message(rng, users, u_pad, cap, words, mu)
    before = msg.copy()
    g_uoff, g_mu, g_rows, g_masks = split_wide_message(msg, u_pad, cap, words)
    assert np.array_equal(msg, before), "the message is not modified"
    assert g_mu == mu
    assert g_uoff.dtype == np.int32 and g_uoff.shape == (u_pad + 1,)
    assert g_rows.dtype == np.int32 and g_masks.dtype == np.uint64 and g_masks.ndim == 2 and g_masks.shape[1] == words
    if mu < 0:
        assert np.all(g_uoff == -1) and g_rows.size == 0 and g_masks.shape == (0, words)
        return
    k = min(mu, cap)
    assert np.array_equal(g_uoff[: users + 1], uoff) and np.all(g_uoff[users + 1:] == mu)
    assert np.array_equal(g_rows, rows[:k])                  # rows beyond cap are cut; Mu still says how many there are
    assert g_masks.shape == (k, words) and np.array_equal(g_masks, masks[:k])
    # bit q of row r, as the header states it
    for r, q in ((0, 0), (0, 64 * words - 1), (k - 1, 64 * words - 1), (k // 2, 3)):
        assert int(g_masks[r, q // 64] >> np.uint64(q % 64)) & 1 == int(masks[r, q // 64] >> np.uint64(q % 64)) & 1


def test_split_wide_message_rejects_a_short_message():
    from sph_pie_amd.binding import split_wide_message
    with pytest.raises(ValueError):
        split_wide_message(np.zeros(10 + 2 + 4 * (1 + 2 * 2) - 1, np.int32), 10, 4, 2)


def test_split_wide_message_reads_a_prefix_of_a_longer_reservation():
    """a communicator reserves for words_max; a step with fewer mask words uses a prefix of the same buffer"""
    from sph_pie_amd.binding import split_wide_message
    rng = np.random.default_rng(5)
    msg, uoff, rows, masks = build_message(rng, 9, 9, 20, 2, 11, guard=20 * 2 * 6)   # room as if reserved for 8 words
    g_uoff, g_mu, g_rows, g_masks = split_wide_message(msg, 9, 20, 2)
    assert g_mu == 11 and np.array_equal(g_rows, rows) and np.array_equal(g_masks, masks) and np.array_equal(g_uoff, uoff)
