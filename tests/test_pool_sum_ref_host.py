"""The numpy restatement of the pooling order (tests/pool_sum_ref.py) checked on the host: it is a sum, and on the inputs of
tests/test_gpu_pool_sums.py it is not the plain ascending sum, so that test can tell the two orders apart."""
import numpy as np

from tests import pool_sum_ref as ref


def _segments():
    """(degree, rows) of every pooled half of the batch, a segment's rows in ascending table order (the plan's order is a permutation
    of it; the GPU test repeats the second check below on the plan's own order)."""
    b = ref.batch_inputs()
    for key, x in ((b["batch"], b["xa"]), (b["frag_batch"], b["xf"])):
        for m in range(len(ref.ATOMS)):
            rows = x[np.flatnonzero(key == m)]
            yield rows.shape[0], rows


def test_the_inputs_are_normal_range_and_free_of_zeros():
    b = ref.batch_inputs()
    for x in (b["xa"], b["xf"]):
        assert x.dtype == np.float32 and float(np.abs(x).min()) >= 2.0 ** -6 and float(np.abs(x).max()) <= 2.0 ** 6
    assert sorted(np.bincount(b["batch"], minlength=len(ref.ATOMS)).tolist()) == sorted(ref.ATOMS)
    assert not np.array_equal(b["batch"], np.sort(b["batch"])), "the molecules' rows are interleaved"
    assert ref.FRAGS[0] == 0 and 63 in b["bit"] and -1 in b["bit"] and -1 in b["group"]


def test_the_restatement_is_a_sum_within_the_float32_bound():
    """An addition with a zero operand is exact, so at most deg - 1 of the additions round, each by at most u = 2^-24 relative: an
    element's weight in the result is at most (1 + u)^(deg - 1), and (1 + u)^(deg - 1) - 1 <= deg u while (deg - 1)^2 u <= 2, far
    beyond these degrees.  Hence |sum - exact| <= deg 2^-24 sum |x| per column."""
    for deg, rows in _segments():
        got = ref.block_rows_sum(rows)
        assert got.dtype == np.float32 and got.shape == (ref.D,)
        want = rows.astype(np.float64).sum(axis=0)
        bound = deg * 2.0 ** -24 * np.abs(rows.astype(np.float64)).sum(axis=0)
        assert np.all(np.abs(got.astype(np.float64) - want) <= bound), deg


def test_the_restatement_is_not_the_sequential_sum():
    differing = [deg for deg, rows in _segments()
                 if deg >= 17 and not np.array_equal(ref.block_rows_sum(rows).view(np.int32), ref.sequential_sum(rows).view(np.int32))]
    assert differing, "no segment of degree >= 17 whose eight-partial sum differs from the ascending sum: the GPU test could not tell"


def test_zeroed_rows_and_trailing_axes():
    rng = np.random.default_rng(5)
    rows = ref.values(rng, (21, ref.D))
    keep = rng.random(21) < 0.5
    zeroed = rows.copy()
    zeroed[~keep] = 0.0
    assert np.array_equal(ref.pooled(rows, np.arange(21), keep), ref.block_rows_sum(zeroed))
    stacked = ref.values(rng, (4, 3, ref.D))          # [deg, segments, columns]: the segments are summed side by side
    assert np.array_equal(ref.block_rows_sum(stacked)[1], ref.block_rows_sum(stacked[:, 1]))
    assert np.array_equal(ref.block_rows_sum(rows[:0]), np.zeros(ref.D, dtype=np.float32))


def test_the_fused_multiply_add_rounds_once():
    """Against exact rational arithmetic, cancellation included."""
    from fractions import Fraction
    rng = np.random.default_rng(7)
    a, b, c = (ref.values(rng, (400,)) for _ in range(3))
    c[:200] = -(a[:200].astype(np.float64) * b[:200].astype(np.float64)).astype(np.float32)          # a b + c nearly cancels
    got = ref.fma32(a, b, c)
    for i in range(a.shape[0]):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = np.float32(float(exact))
        cands = (near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf)))
        best = min(cands, key=lambda z: (abs(Fraction(float(z)) - exact), int(np.float32(z).view(np.int32)) & 1))
        assert got[i] == best, (a[i], b[i], c[i])


def test_row_dots_is_a_dot_product_within_the_bound():
    rng = np.random.default_rng(9)
    feat, A = ref.values(rng, (ref.D,)), ref.values(rng, (8, ref.D))
    got = ref.row_dots(feat, A)
    want = A.astype(np.float64) @ feat.astype(np.float64)
    bound = 128 * 2.0 ** -24 * (np.abs(A.astype(np.float64)) * np.abs(feat.astype(np.float64))).sum(axis=1)
    assert got.dtype == np.float32 and np.all(np.abs(got - want) <= bound)
