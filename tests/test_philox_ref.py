"""The dropout stream's reference (tests/philox_ref.py) against Random123's known answers, and the statistics of the SEVEN-round stream
the kernels draw their masks from (csrc/fn_internal.h): keep rates, bit frequencies, and the independence of neighbouring blocks,
words, seeds and the ranks' seeds.  Everything is deterministic (fixed seeds, 2^18 consecutive blocks = 2^20 words); every statistic
is a binomial z-score and the condition is |z| <= 6 -- a cap with a false-failure probability of about 2e-9 per check, not a tuned
tolerance.  No GPU."""
import itertools

import numpy as np
import pytest

from tests import philox_ref

BLOCKS = 1 << 18
SEEDS = [0, 1, 0x1234567, 2 ** 63 + 5]
Z_CAP = 6.0


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_known_answers():
    assert _hex(philox_ref.philox4x32(np.zeros(1, dtype=np.uint64), 0, 10)[0]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"    # Random123's kat_vectors
    assert _hex(philox_ref.philox4x32(np.zeros(1, dtype=np.uint64), 0, 7)[0]) == "5f6fb709 0d893f64 4f121f81 4f730a48"


def test_counter_and_key_words():
    """Both halves of the block index and of the seed reach the generator (Random123's other published vectors set counter words 2
    and 3, which this stream keeps at zero, so they do not apply here), and the shape follows the counters'."""
    out = philox_ref.philox4x32(np.array([2 ** 64 - 1, 2 ** 32, 1], dtype=np.uint64), 2 ** 64 - 1, 10)
    assert out.shape == (3, 4) and out.dtype == np.uint32
    assert len({_hex(r) for r in out}) == 3
    for seed_a, seed_b in ((5, 5 + 2 ** 32), (5, 6)):
        a, b = (philox_ref.philox4x32(np.arange(4, dtype=np.uint64), s, 7) for s in (seed_a, seed_b))
        assert not (a == b).all(axis=1).any()
    a = philox_ref.philox4x32(np.arange(4, dtype=np.uint64), 9, 7)
    b = philox_ref.philox4x32(np.arange(4, dtype=np.uint64) + np.uint64(2 ** 32), 9, 7)
    assert not (a == b).all(axis=1).any()
    assert philox_ref.philox4x32(np.zeros((2, 3), dtype=np.uint64), 0, 7).shape == (2, 3, 4)


def test_keep_rule_is_exact():
    top = np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint32)
    assert philox_ref.keep(top, 0.0).all()
    assert not philox_ref.keep(top, 1.0).any()
    assert list(philox_ref.keep(top, 0.5)) == [False, False, False, False, True, True, True, True]
    assert list(philox_ref.keep(top, 2.0 ** -25)) == [False, False, True, True, True, True, True, True]       # u = 0 is the only value below p
    assert list(philox_ref.keep(top, 2.0 ** -24)) == [False, False, True, True, True, True, True, True]
    assert list(philox_ref.keep(top, np.nextafter(np.float32(1), np.float32(0)))) == [False] * 6 + [True, True]   # only u = 1 - 2^-24 survives
    # float32(0.1) lies above 0.1: 0.1f * 2^24 = 1677721.625 exactly
    assert philox_ref.threshold(0.1) == 1677722
    assert philox_ref.threshold(1 / 3) == 5592406 and philox_ref.threshold(0.25) == 1 << 22


def test_mask_uses_word_e_mod_4_of_block_offset_plus_e_div_4():
    words = philox_ref.philox4x32(np.arange(7, 7 + 3, dtype=np.uint64), 11, 7).reshape(-1)
    for numel in (1, 3, 4, 5, 9, 12):
        got = philox_ref.mask(numel, 0.5, 11, 7)
        assert got.shape == (numel,) and (got == (words[:numel] >> 31).astype(bool)).all()
    # the block index is a 64-bit sum
    assert (philox_ref.mask(32, 0.25, 3, 2 ** 32 - 3)[12:] == philox_ref.mask(20, 0.25, 3, 2 ** 32)).all()


# ------------------------------------------------------------------------------------------------ the seven-round stream
_STREAMS = {}


def _words(seed):
    """uint32 [2^18, 4]: the seven-round blocks 0 .. 2^18 - 1 of ``seed`` (computed once per session)."""
    if seed not in _STREAMS:
        _STREAMS[seed] = philox_ref.philox4x32(np.arange(BLOCKS, dtype=np.uint64), seed, philox_ref.ROUNDS)
    return _STREAMS[seed]


def _z(count, n, q):
    return (float(count) - n * q) / (n * q * (1.0 - q)) ** 0.5


def _check(z, what):
    print(f"{what}: z = {z:+.2f}")
    assert abs(z) <= Z_CAP, (what, z)


def _top(seed):
    return _words(seed) >> np.uint32(31) != 0            # the keep decision at p = 0.5


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", [0.1, 0.25, 1 / 3, 0.5])
def test_keep_rate(p, seed):
    q = 1.0 - philox_ref.threshold(p) / 2.0 ** 24
    kept = philox_ref.keep(_words(seed), p)
    _check(_z(kept.sum(), kept.size, q), f"keep rate p={p:.4f} seed={seed:#x}")


@pytest.mark.parametrize("seed", SEEDS)
def test_bit_frequencies(seed):
    w = _words(seed).reshape(-1)
    for bit in range(32):
        ones = int(((w >> np.uint32(bit)) & np.uint32(1)).sum())
        _check(_z(ones, w.size, 0.5), f"bit {bit} seed={seed:#x}")


@pytest.mark.parametrize("seed", SEEDS)
def test_keep_decisions_of_neighbours_agree_half_of_the_time(seed):
    k = _top(seed)
    same = k[1:] == k[:-1]
    _check(_z(same.sum(), same.size, 0.5), f"adjacent counters seed={seed:#x}")
    for a, b in ((0, 1), (1, 2), (2, 3)):
        same = k[:, a] == k[:, b]
        _check(_z(same.sum(), same.size, 0.5), f"words {a}/{b} seed={seed:#x}")
    same = k == _top((seed + 1) & 0xFFFFFFFFFFFFFFFF)
    _check(_z(same.sum(), same.size, 0.5), f"seeds s / s + 1, s={seed:#x}")


def test_keep_decisions_of_the_ranks_seeds_agree_half_of_the_time():
    """The seeds PhiloxStream derives for ranks 0-7 from one torch.initial_seed(): every pair of ranks."""
    import torch
    from fragnet_amd import ops
    torch.manual_seed(20240229)
    seeds = [ops.PhiloxStream(rank=r).take(0)[0] for r in range(8)]
    assert len(set(seeds)) == 8 and all(0 <= s < 2 ** 64 for s in seeds)
    for (ra, sa), (rb, sb) in itertools.combinations(enumerate(seeds), 2):
        same = _top(sa) == _top(sb)
        _check(_z(same.sum(), same.size, 0.5), f"ranks {ra}/{rb}")
