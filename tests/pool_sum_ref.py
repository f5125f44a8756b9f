"""The order of additions of the pooling kernels and of the destination-sorted edge term, restated in numpy (float32 throughout) from
csrc/shared_bodies.inc and csrc/fn_internal.h, independent of every kernel: tests/test_gpu_pool_sums.py compares bits against it,
tests/test_pool_sum_ref_host.py checks the restatement itself.  Also the inputs both use."""
import numpy as np

F32 = np.float32
D = 128
ROWS = 8                                                     # half-waves of a block (kRows)
ATOMS = (0, 1, 7, 8, 9, 16, 17, 63, 64, 65, 200)            # atoms per molecule: around one and two trips of the eight half-waves, and long
FRAGS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)                  # fragments per molecule; molecule 0 has neither atoms nor fragments


def block_rows_sum(rows):
    """block_rows_sum of shared_bodies.inc on rows [deg, ...]: partial w adds the rows w, w + 8, .. in ascending order from +0.0, then
    ((0 + p0) + p1) + .. + p7.  A row that a kernel leaves out is passed as zeros."""
    rows = np.asarray(rows, dtype=F32)
    part = np.zeros((ROWS,) + rows.shape[1:], dtype=F32)
    for i in range(rows.shape[0]):
        part[i % ROWS] = part[i % ROWS] + rows[i]
    v = np.zeros(rows.shape[1:], dtype=F32)
    for w in range(ROWS):
        v = v + part[w]
    return v


def sequential_sum(rows):
    """The plain ascending float32 sum: the order the kernels do NOT use."""
    rows = np.asarray(rows, dtype=F32)
    v = np.zeros(rows.shape[1:], dtype=F32)
    for i in range(rows.shape[0]):
        v = v + rows[i]
    return v


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding.  The product of two float32 is exact in float64; the float64 sum is rounded to odd (the
    error of the addition from TwoSum: an inexact sum with an even last bit moves to its neighbour on the side of the error), and a
    53-bit round-to-odd value rounds to 24 bits as the exact value does."""
    p = np.asarray(a, dtype=F32).astype(np.float64) * np.asarray(b, dtype=F32).astype(np.float64)
    c = np.asarray(c, dtype=F32).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def _lane_partner_sums(s):
    """head_sum<32> of fn_internal.h on the 32 lanes of a half-wave (last axis): every lane adds its partner's value, partners
    lane ^ 16, the mirror inside 16 lanes, the mirror inside 8 lanes, lane ^ 2, lane ^ 1."""
    lane = np.arange(32)
    for partner in (lane ^ 16, (lane & 16) | (15 - (lane & 15)), (lane & 24) | (7 - (lane & 7)), lane ^ 2, lane ^ 1):
        s = s + s[..., partner]
    return s


def row_dots(feat_row, A_rows):
    """<feat_row, A_rows[q]> for every q the way row_dots_sorted_body takes it: lane l holds the elements 4 l .. 4 l + 3, dot4 as the
    compiler contracts a.x b.x + a.y b.y + a.z b.z + a.w b.w (the y product, then fused multiply-adds of x, z, w: read off the kernel's
    listing), the butterfly above, the value of lane q.  The contraction is the compiler's choice, not the source's: if a compiler
    upgrade makes tests/test_gpu_pool_sums.py::test_the_sorted_edge_term fail with no change to the kernel, read the new order off
    the listing and restate it here (or fall back to the float64 bound 128 * 2^-24 * sum |a_k b_k| per entry)."""
    v = np.asarray(feat_row, dtype=F32).reshape(32, 4)
    a = np.asarray(A_rows, dtype=F32).reshape(-1, 32, 4)
    t = a[:, :, 1] * v[None, :, 1]
    for k in (0, 2, 3):
        t = fma32(v[None, :, k], a[:, :, k], t)
    s = _lane_partner_sums(t.astype(F32))
    return np.array([s[q, q] for q in range(a.shape[0])], dtype=F32)


def values(rng, shape):
    """Signed float32 with |x| in [2^-6, 2^6]: no zeros, no denormals, so 0 + x and flush modes play no part."""
    mag = np.exp2(rng.uniform(-6.0, 6.0, size=shape))
    return (mag * rng.choice((-1.0, 1.0), size=shape)).astype(F32)


def batch_inputs(seed=20):
    """The one batch of the pooling tests: ``batch`` / ``frag_batch`` keys with the molecules' rows interleaved in the tables, the
    tables, a group id per atom (molecule m's groups are 100 m + 0 .. 100 m + 4, every seventh atom from the ninth on in none: -1) and
    a bit per atom (its position among up to 64 groups, bit 63 taken in the molecules with 64 atoms and more; -1 where the group is)."""
    rng = np.random.default_rng(seed)
    B = len(ATOMS)
    batch = rng.permutation(np.repeat(np.arange(B), ATOMS)).astype(np.int64)
    frag_batch = rng.permutation(np.repeat(np.arange(B), FRAGS)).astype(np.int64)
    xa, xf = values(rng, (batch.shape[0], D)), values(rng, (frag_batch.shape[0], D))
    group = np.full(batch.shape[0], -1, dtype=np.int64)
    bit = np.full(batch.shape[0], -1, dtype=np.int8)
    for m in range(B):
        where = np.flatnonzero(batch == m)
        j = np.arange(where.shape[0])
        g = j % min(max(ATOMS[m], 1), 64)
        g[(j % 7 == 6) & (j >= 8)] = -1
        bit[where] = g
        group[where] = np.where(g >= 0, 100 * m + g % 5, -1)
    return dict(batch=batch, frag_batch=frag_batch, xa=xa, xf=xf, group=group, bit=bit)


def pooled(x, order, keep=None):
    """One pooled half: block_rows_sum over the table rows ``order`` (a segment's slice of the plan's permutation), the rows with
    ``keep[row] == False`` zeroed."""
    rows = x[order].copy()
    if keep is not None:
        rows[~keep[order]] = 0.0
    return block_rows_sum(rows)
