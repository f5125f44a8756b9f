"""The metrics kernels on the GPU (csrc/metrics.hip through ops.pair_concordance / ops.regression_sums) against the numpy references
of fragnet_amd/metrics.py.

a. Pair counts: all five fields equal the O(n^2) broadcast-compare reference as INTEGERS, for every n at a tile edge (1, 2, the wave and
   workgroup sizes +-1, and 2 T + 1 for the kernel's i- and j-tile size T = ops.CONC_TILE: three tiles each way, the last with one
   row), c = 1, 12, 13 and splits = 0, 1, 3, on six label / prediction patterns.  Two calls give the same bytes.
b. Regression sums against math.fsum of the same fp32 inputs promoted to float64, relative 1e-12 at n <= 4096: an fp64 accumulation of
   n terms carries at most n 2^-53 = 4.5e-13 relative to the sum of magnitudes, and every sum here is of one sign up to noise (labels
   around 3, predictions near the labels), so the sum of magnitudes is the sum.  Bit-identical across calls and splits.
c. pred * scale + shift has the bits of numpy's float32 product-then-sum (no fma), read back through sum p of one-row inputs."""
import numpy as np
import pytest
import torch

from fragnet_amd import metrics as M
from fragnet_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = ops.CONC_TILE
SIZES = sorted({1, 2, 63, 64, 65, 255, 256, 257, 2 * T + 1})
COLS = (1, 12, 13)
SPLITS = (0, 1, 3)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)


def _binary(rng, n, c, missing=0.3):
    y = (rng.random((n, c)) < 0.4).astype(np.float32)
    y[rng.random((n, c)) < missing] = -1.0
    return y


def _scores(rng, y, levels=32):
    """class-dependent scores on a coarse grid: ties within and across the classes"""
    return (np.round((rng.standard_normal(y.shape) + np.maximum(y, 0)) * levels / 4) / levels).astype(np.float32)


def _pattern(name, n, c, seed):
    rng = np.random.default_rng(seed)
    floor = M.CLSF_LABEL_FLOOR
    if name == "binary_missing":
        y = _binary(rng, n, c)
        p = _scores(rng, y)
    elif name == "all_positive":
        y = np.ones((n, c), dtype=np.float32)
        p = _scores(rng, y)
    elif name == "all_missing":
        y = np.full((n, c), -1.0, dtype=np.float32)
        p = _scores(rng, y)
    elif name == "real_duplicates":
        y = (np.round(rng.standard_normal((n, c)) * 4) / 4).astype(np.float32)         # about 25 distinct values: many equal labels
        p = (y + np.round(rng.standard_normal((n, c)) * 8) / 8).astype(np.float32)
        floor = float("-inf")
    elif name == "pred_all_equal":
        y = _binary(rng, n, c)
        p = np.full((n, c), 0.25, dtype=np.float32)
    elif name == "special_values":
        y = _binary(rng, n, c, missing=0.2)
        y[rng.random((n, c)) < 0.05] = np.nan                                          # a NaN label is a missing label
        p = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, np.nan], dtype=np.float32), size=(n, c),
                       p=[0.2, 0.2, 0.15, 0.15, 0.12, 0.12, 0.06]).astype(np.float32)
    else:
        raise AssertionError(name)
    return p, y, floor


PATTERNS = ("binary_missing", "all_positive", "all_missing", "real_duplicates", "pred_all_equal", "special_values")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_counts_equal_the_reference_exactly(pattern):
    for n in SIZES:
        p_all, y_all, floor = _pattern(pattern, n, max(COLS), 100 + n)
        want_all = M.reference_counts(p_all, y_all, floor)               # once per n: column k of a narrower table is column k of this one
        for c in COLS:
            p, y = dev(p_all[:, :c]), dev(y_all[:, :c])
            for splits in SPLITS:
                got = ops.pair_concordance(p, y, floor, splits=splits).cpu().numpy()
                assert got.dtype == np.int64 and got.shape == (c, 5)
                assert np.array_equal(got, want_all[:c]), (pattern, n, c, splits, got.tolist(), want_all[:c].tolist())
    if pattern == "special_values":
        assert want_all[:, 1].sum() > 0                                    # the NaN predictions were seen and counted
        with pytest.raises(ValueError, match="NaN prediction"):
            M.roc_auc(got)
    if pattern == "all_missing":
        assert not want_all.any()
    if pattern == "pred_all_equal":
        assert np.array_equal(want_all[:, 2], want_all[:, 4]) and M.roc_auc(got) == 0.5


def test_counts_are_the_same_bytes_on_every_call_and_give_sklearn_auc():
    from sklearn.metrics import roc_auc_score
    n, c = 3 * T + 77, 12
    p, y, floor = _pattern("binary_missing", n, c, 5)
    pd, yd = dev(p), dev(y)
    first = ops.pair_concordance(pd, yd, floor)
    again = ops.pair_concordance(pd, yd, floor)
    forced = ops.pair_concordance(pd, yd, floor, splits=2)
    assert torch.equal(first, again) and torch.equal(first, forced)
    auc = M.concordance_per_column(first)
    for k in range(c):
        ok = y[:, k] > -0.5
        assert abs(auc[k] - roc_auc_score(y[ok, k], p[ok, k])) <= 1e-12
    # a non-contiguous view is made contiguous, not misread
    assert torch.equal(ops.pair_concordance(pd[:, 3:5], yd[:, 3:5], floor), first[3:5])
    # nothing to count: zeros, no launch
    assert not ops.pair_concordance(pd[:0], yd[:0], floor).cpu().numpy().any()
    assert not ops.regression_sums(pd[:0], yd[:0]).cpu().numpy().any()


def _regression_case(n, c, seed):
    rng = np.random.default_rng(seed)
    y = (3 + rng.standard_normal((n, c))).astype(np.float32)
    p = (y / 1.5 + 0.2 * rng.standard_normal((n, c))).astype(np.float32)
    return p, y


@pytest.mark.parametrize("c", [1, 3])
def test_regression_sums_against_fsum(c):
    ch = ops.SUMS_CHUNK
    for n in (1, 2, 63, 255, 256, 257, ch - 1, ch, ch + 1, 2 * ch + 1, 4096):
        p, y = _regression_case(n, c, 40 + n)
        for floor, scale, shift in ((float("-inf"), 1.0, 0.0), (float("-inf"), 1.5, -0.25), (3.0, 1.5, -0.25)):
            yy = y.copy()
            if n > 2:
                yy[1, 0] = np.nan                                           # never valid, whatever the floor
            want = M.reference_sums(p, yy, floor, scale, shift)
            pd, yd = dev(p), dev(yy)
            got = [ops.regression_sums(pd, yd, floor, scale, shift, splits=s).cpu().numpy() for s in (0, 0, 1, 3)]
            rel = np.abs(got[0] - want) / np.where(want != 0, np.abs(want), 1.0)
            print(f"sums n={n} c={c} floor={floor} scale={scale}: max relative error {rel.max():.3e}")
            np.testing.assert_allclose(got[0], want, rtol=1e-12, atol=0)
            assert got[0][:, 0].tolist() == want[:, 0].tolist()              # the counts of valid rows, exactly
            for g in got[1:]:
                assert g.tobytes() == got[0].tobytes(), (n, c, floor)


def test_scale_shift_is_a_float32_product_then_a_float32_sum():
    rng = np.random.default_rng(9)
    c = 64
    differs = 0
    for scale, shift in ((1.7, 0.3), (0.3, -6.11), (1e-3, 1e3), (3.1415927, 2.7182817), (123.456, -0.001)):
        p = rng.standard_normal((1, c)).astype(np.float32) * 3
        y = np.zeros((1, c), dtype=np.float32)
        got = ops.regression_sums(dev(p), dev(y), scale=scale, shift=shift).cpu().numpy()
        want = (p[0] * np.float32(scale) + np.float32(shift)).astype(np.float64)
        assert got[:, 2].tobytes() == want.tobytes(), (scale, shift)
        fused = (p[0].astype(np.float64) * np.float64(np.float32(scale)) + np.float64(np.float32(shift))).astype(np.float32)
        differs += int((fused.astype(np.float64) != want).sum())
    assert differs > 0           # the inputs tell one rounding from two: a fused multiply-add would have been caught


def test_refusals_on_the_device():
    from fragnet_amd import _lib
    p = torch.zeros(4, 2, device=DEV)
    with pytest.raises(ValueError, match=r"\[n, c\]"):
        ops.pair_concordance(p, p[:, :1])
    with pytest.raises(ValueError, match="c must be"):
        ops.pair_concordance(torch.zeros(4, 65, device=DEV), torch.zeros(4, 65, device=DEV))
    with pytest.raises(ValueError, match="splits"):
        ops.regression_sums(p, p, splits=-1)
    with pytest.raises(TypeError, match="float32"):
        ops.pair_concordance(p.double(), p.double())
    with pytest.raises(_lib.FragnetHipError):
        ops.pair_concordance(p, p.cpu())
