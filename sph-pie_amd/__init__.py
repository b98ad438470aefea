"""sph-pie_amd — MI355X-native session-scan -> per-user feed path (drop-in for the path named in
BASELINE.json's north_star; nothing else of sph-pie is rebuilt here).

  csrc/      HIP kernels for gfx950 + the C ABI of include/pie_scan.h   -> libpie_hip.so
  host/      Node.js host mirror of the reference modules over a raw N-API addon
  binding.py ctypes binding of the same C ABI (used by tests, bench.py and the multi-GPU driver)
  shard.py   user-hash sharding + all-gather of per-user feeds (torch.distributed; nccl == RCCL on ROCm)
"""
from .binding import (ABI_SYMBOLS, PIE_BATCH_MAX, PIE_WIDE_MAX, PIE_END_NONE, PIE_GEN_CLUSTERED, PIE_GEN_INTERVAL, PIE_GEN_TIME_ORDERED, PieComm, PieError, PieScan,
                      batch_mask_codes, delete_users_plan, hot_order_key, hot_slot_bits, load_library, set_end_last_writers, shard_of, shard_route, split_wide_message, token_homes, token_key, token_slots_for, token_turn_plan, session_turn_plan, shard_session_turn_plan, turn_ops, tz_table, TURN_OP, TURN_GET, TURN_TOUCH, TURN_DELETE, TURN_CREATE)
from .build import UBENCH_LIB, build_all, build_hip, build_napi, build_oracle, build_ubench


def zipf_cdf(n_users, exponent=1.1):
    """uint64 thresholds floor(CDF_k * 2^64) of Zipf(exponent) over n_users ranks (for gen_synthetic_cdf)."""
    import numpy as np
    w = 1.0 / np.arange(1, n_users + 1, dtype=np.float64) ** exponent
    c = np.cumsum(w) / w.sum()
    thr = np.minimum(np.floor(c * 2.0 ** 64), 2.0 ** 64 - 2048).astype(np.uint64)
    thr[-1] = np.uint64(2 ** 64 - 1)
    return np.maximum.accumulate(thr)

__all__ = ["ABI_SYMBOLS", "PIE_BATCH_MAX", "PIE_WIDE_MAX", "PIE_END_NONE", "PIE_GEN_CLUSTERED", "PIE_GEN_INTERVAL", "PIE_GEN_TIME_ORDERED", "PieComm", "PieError", "PieScan",
           "batch_mask_codes", "delete_users_plan", "hot_order_key", "hot_slot_bits", "load_library", "set_end_last_writers", "shard_of", "shard_route", "split_wide_message", "token_homes", "token_key", "token_slots_for", "token_turn_plan", "session_turn_plan", "shard_session_turn_plan", "turn_ops", "TURN_OP", "TURN_GET", "TURN_TOUCH", "TURN_DELETE", "TURN_CREATE", "tz_table", "zipf_cdf", "build_all", "build_hip", "build_napi", "build_oracle", "build_ubench", "UBENCH_LIB"]
