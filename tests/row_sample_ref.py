"""Reference for the row sampler (include/fragnet_hip.h, fn_select_rows_u8 / fn_sample_rows_u8), numpy only and written from the rule,
not from the kernel: of the n real rows, k = int(n * keep_frac) are kept -- row i < n iff fewer than k rows j < n have
(key_j, j) < (key_i, i) lexicographically -- and rows n <= i < cap (padding) are kept.  The sampler's key of row i is word i % 4 of
Philox block offset + i // 4 (tests/philox_ref.py: the dropout stream's convention)."""
import numpy as np

from tests import philox_ref


def count(n, keep_frac):
    return int(n * keep_frac)           # the same IEEE double product the kernel forms, truncated


def select(keys, keep_frac, n=None):
    """uint8 [cap] from uint32 keys [cap]; ``n`` (default cap) is clamped to [0, cap] the way the kernel clamps a device count."""
    keys = np.asarray(keys, dtype=np.uint32)
    cap = keys.shape[0]
    n = cap if n is None else min(max(int(n), 0), cap)
    out = np.ones(cap, dtype=np.uint8)
    order = np.lexsort((np.arange(n), keys[:n]))           # by key, then by row index
    out[:n] = 0
    out[order[:count(n, keep_frac)]] = 1
    return out


def keys(cap, seed, offset, rounds=philox_ref.ROUNDS):
    blocks = (int(cap) + 3) // 4
    ctr = np.arange(blocks, dtype=np.uint64) + np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF)      # wraps modulo 2^64 like the kernel's sum
    return philox_ref.philox4x32(ctr, seed, rounds).reshape(-1)[:cap]


def sample(cap, keep_frac, seed, offset, n=None):
    return select(keys(cap, seed, offset), keep_frac, n)
