"""Reference for the dropout stream (include/fragnet_hip.h, fn_dropout_act_f32): Philox-4x32 keyed by (seed, offset + element / 4),
keep iff u >= p with u = (bits >> 8) / 2^24.  numpy only -- no torch, no GPU -- and written from the Random123 definition
(Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), not from the kernels' generator:

    one round on the counter (c0, c1, c2, c3) under the key (k0, k1):
        (hi0, lo0) = 0xD2511F53 * c0,  (hi1, lo1) = 0xCD9E8D57 * c2        (32 x 32 -> 64 bit products)
        (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)
    R rounds; before rounds 2 .. R the key moves on by the Weyl constants (0x9E3779B9, 0xBB67AE85).

The stream's convention: the 64-bit block index is counter words 0 (low half) and 1 (high half), words 2 and 3 are zero; the 64-bit seed is
key words 0 (low half) and 1 (high half).  Element e of a tensor drawn at ``offset`` uses word e % 4 of block offset + e // 4."""
from fractions import Fraction

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
ROUNDS = 7                     # what the kernels run (csrc/fn_internal.h)
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(ctr, seed, rounds):
    """``ctr``: array of 64-bit block indices (any shape); ``seed``: Python int, taken modulo 2^64.  Returns uint32 [..., 4]."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c = [ctr & _LOW, ctr >> _S32, np.zeros_like(ctr), np.zeros_like(ctr)]      # 32-bit words held in uint64 lanes
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                   # < 2^64: exact
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
    return np.stack(c, axis=-1).astype(np.uint32)


def threshold(p):
    """The smallest integer k with k / 2^24 >= float32(p), on exact rationals."""
    q = Fraction(float(np.float32(p))) * (1 << 24)
    return -((-q.numerator) // q.denominator)


def keep(bits, p):
    """True where (bits >> 8) / 2^24 >= float32(p), decided on the integers."""
    return (np.asarray(bits, dtype=np.uint32) >> np.uint32(8)).astype(np.int64) >= threshold(p)


def scale(p):
    """What a kept element is multiplied by: 1 / (1 - p) in float32 (0 for p = 1: nothing is kept)."""
    p = np.float32(p)
    return np.float32(1) / (np.float32(1) - p) if p < 1 else np.float32(0)


def mask(numel, p, seed, offset, rounds=ROUNDS):
    """bool [numel]: which elements of a tensor drawn at (seed, offset) survive dropout with probability ``p``."""
    blocks = (int(numel) + 3) // 4
    ctr = (np.arange(blocks, dtype=np.uint64) + np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF))      # wraps modulo 2^64 like the kernels' sum
    return keep(philox4x32(ctr, seed, rounds).reshape(-1)[:numel], p)
