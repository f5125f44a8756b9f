"""Host side of the device metrics (fragnet_amd/metrics.py, ops.pair_concordance / ops.regression_sums, csrc/metrics.hip's argument
checks): the numpy reference counts against sklearn, the concordance index on a case counted by hand, the binding, the refusals.
Nothing here needs a GPU.

Tolerance of the sklearn comparison: both sides are ratios of exact integers evaluated in float64; sklearn's trapezoid sum carries at
most n roundings of 2^-53, below 5e-13 at n = 4096, so 1e-12 holds with room."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from fragnet_amd import metrics as M


def _quantised_case(n, seed, levels=16, missing=0.3):
    rng = np.random.default_rng(seed)
    label = (rng.random(n) < 0.4).astype(np.float32)
    label[rng.random(n) < missing] = -1.0
    pred = (np.floor(rng.random(n) * levels) / levels + 0.3 * np.maximum(label, 0)).astype(np.float32)
    pred = (np.round(pred * levels) / levels).astype(np.float32)          # 16-level grid: many ties within and across the classes
    return pred, label


@pytest.mark.parametrize("n", [1, 2, 63, 257, 1000, 4096])
def test_reference_roc_auc_equals_sklearn(n):
    from sklearn.metrics import roc_auc_score
    cols = [_quantised_case(n, 7 + s) for s in range(3)]
    rng = np.random.default_rng(n)
    cols.append((rng.standard_normal(n).astype(np.float32), (rng.random(n) < 0.5).astype(np.float32)))       # continuous, nothing missing
    cols.append((rng.standard_normal(n).astype(np.float32), np.ones(n, dtype=np.float32)))                   # one class only
    cols.append((rng.standard_normal(n).astype(np.float32), np.full(n, -1, dtype=np.float32)))               # nothing valid
    pred, label = np.stack([c[0] for c in cols], 1), np.stack([c[1] for c in cols], 1)
    counts = M.reference_counts(pred, label, M.CLSF_LABEL_FLOOR)
    per_col = M.concordance_per_column(counts)
    want = []
    for k in range(pred.shape[1]):
        ok = label[:, k] > -0.5
        assert counts[k, 0] == ok.sum() and counts[k, 1] == 0
        if ok.any() and len(np.unique(label[ok, k])) == 2:
            want.append(roc_auc_score(label[ok, k], pred[ok, k]))
            assert abs(per_col[k] - want[-1]) <= 1e-12, (k, per_col[k], want[-1])
            pos, neg = int((label[ok, k] == 1).sum()), int((label[ok, k] == 0).sum())
            assert counts[k, 2] == pos * neg
        else:
            assert np.isnan(per_col[k]) and counts[k, 2] == 0
    assert np.isnan(per_col[-1]) and np.isnan(per_col[-2])
    if want:
        assert abs(M.roc_auc(counts) - float(np.mean(want))) <= 1e-12
    else:
        assert math.isnan(M.roc_auc(counts))


def test_concordance_index_by_hand():
    # labels 1 < 2 = 2 < 3 < 5, one row missing (NaN label); predictions with one tie and one inversion
    label = np.array([3.0, 1.0, 2.0, np.nan, 2.0, 5.0], dtype=np.float32)
    pred = np.array([0.5, 0.1, 0.5, 9.0, 0.7, 0.6], dtype=np.float32)
    # ordered pairs (i, j), label_i > label_j, among rows 0 1 2 4 5:
    #   (0,1) 0.5>0.1 conc   (0,2) 0.5=0.5 tied   (0,4) 0.5<0.7 disc   (2,1) conc   (4,1) conc
    #   (5,0) 0.6>0.5 conc   (5,1) conc           (5,2) conc           (5,4) 0.6<0.7 disc
    counts = M.reference_counts(pred, label)
    assert counts.tolist() == [[5, 0, 9, 6, 1]]
    assert M.concordance_index(counts) == 6.5 / 9
    # a floor drops the rows below it: 2 is the floor, label 1 leaves -> pairs (0,2) (0,4) (5,0) (5,2) (5,4)
    assert M.reference_counts(pred, label, 2.0).tolist() == [[4, 0, 5, 2, 1]]
    # IEEE compares: -0 == 0 and inf == inf are ties; a NaN prediction in a valid row is counted and takes part in no pair
    label = np.array([1, 0, 1, 0, 1], dtype=np.float32)
    pred = np.array([0.0, -0.0, np.inf, np.inf, np.nan], dtype=np.float32)
    counts = M.reference_counts(pred, label)
    assert counts.tolist() == [[5, 1, 4, 1, 2]]           # (0,1) tied, (0,3) disc, (2,1) conc, (2,3) tied
    with pytest.raises(ValueError, match="column 0.*NaN"):
        M.roc_auc(counts)
    with pytest.raises(ValueError, match="column 1"):
        M.concordance_index(np.array([[3, 0, 2, 1, 0], [3, 2, 0, 0, 0]]))
    assert math.isnan(M.roc_auc(np.array([[3, 0, 0, 0, 0]])))
    assert M.roc_auc(np.array([[3, 0, 2, 1, 1], [0, 0, 0, 0, 0]])) == 0.75            # the empty column is left out of the mean


def test_regression_metrics_from_reference_sums():
    rng = np.random.default_rng(3)
    y = (3 + rng.standard_normal(500)).astype(np.float32)
    p = (y + 0.3 * rng.standard_normal(500)).astype(np.float32)
    s = M.reference_sums(p, y, scale=1.5, shift=-0.25)
    pd = (p * np.float32(1.5) + np.float32(-0.25)).astype(np.float64)
    yd = y.astype(np.float64)
    m = M.regression_metrics(s)
    assert s[0, 0] == 500
    np.testing.assert_allclose(m["mse"][0], ((yd - pd) ** 2).mean(), rtol=1e-12)
    np.testing.assert_allclose(m["rmse"][0], math.sqrt(((yd - pd) ** 2).mean()), rtol=1e-12)
    np.testing.assert_allclose(m["mae"][0], np.abs(yd - pd).mean(), rtol=1e-12)
    np.testing.assert_allclose(m["pearson"][0], np.corrcoef(yd, pd)[0, 1], rtol=1e-10)       # (the sums form cancels: var = E x^2 - (E x)^2)
    np.testing.assert_allclose(m["r2"][0], 1 - ((yd - pd) ** 2).sum() / ((yd - yd.mean()) ** 2).sum(), rtol=1e-10)
    empty = M.regression_metrics(M.reference_sums(p, np.full_like(y, np.nan)))
    assert all(np.isnan(v[0]) for v in empty.values())
    with pytest.raises(ValueError, match=r"\[c, 8\]"):
        M.regression_metrics(np.zeros((2, 5)))


def test_header_binding_and_abi():
    from fragnet_amd import _lib
    assert _lib.ABI_VERSION == 12 and _lib.load().fn_abi_version() == 12
    assert _lib.TUNE_COUNT == 35
    for name in ("fn_pair_concordance_f32", "fn_regression_sums_f32", "fn_metrics_scratch_bytes"):
        assert name in _lib.SIGNATURES and name in _lib.HEADER.functions
    assert [name for name, _ in _lib.Metrics._fields_] == ["pred", "label", "out", "scratch", "scratch_bytes", "n", "label_floor", "scale",
                                                           "shift", "c", "splits"]
    assert _lib.HEADER.functions["fn_metrics_scratch_bytes"][0] is C.c_int64
    assert (_lib.CONC_FIELDS, _lib.SUMS_FIELDS) == (len(M.CONC_FIELDS), len(M.SUMS_FIELDS)) == (5, 8)
    from fragnet_amd import ops
    assert ops.CONC_FIELDS == M.CONC_FIELDS and ops.SUMS_FIELDS == M.SUMS_FIELDS and ops.CONC_TILE == _lib.CONC_TILE


def _descriptor(_lib, **kw):
    fields = dict(pred=None, label=None, out=None, scratch=None, scratch_bytes=0, n=1000, label_floor=-0.5, scale=1.0, shift=0.0, c=12, splits=0)
    fields.update(kw)
    m = _lib.Metrics()
    for name, v in fields.items():
        setattr(m, name, v)
    return m


def test_library_refuses_bad_descriptors_before_any_launch():
    from fragnet_amd import _lib
    lib = _lib.load()
    T, CH = _lib.CONC_TILE, _lib.SUMS_CHUNK
    # concordance: one row of 5 uint64 per (column, j-slice, i-block); sums: one row of 8 doubles per (column, chunk)
    assert lib.fn_metrics_scratch_bytes(C.byref(_descriptor(_lib, n=2 * T + 1, c=3, splits=1)), 0) == 3 * 1 * 3 * 40
    assert lib.fn_metrics_scratch_bytes(C.byref(_descriptor(_lib, n=2 * T + 1, c=3, splits=3)), 0) == 3 * 3 * 3 * 40
    assert lib.fn_metrics_scratch_bytes(C.byref(_descriptor(_lib, n=2 * T + 1, c=3, splits=99)), 0) == 3 * 3 * 3 * 40     # no more slices than j-tiles
    assert lib.fn_metrics_scratch_bytes(C.byref(_descriptor(_lib, n=2 * CH + 1, c=3, splits=7)), 1) == 3 * 3 * 64           # whatever the splits
    assert lib.fn_metrics_scratch_bytes(C.byref(_descriptor(_lib, n=0)), 0) == 0
    for entry in (lib.fn_pair_concordance_f32, lib.fn_regression_sums_f32):
        assert entry(None, None) == _lib.FN_EINVAL
        for bad in (dict(n=-1), dict(n=(1 << 24) + 1), dict(c=0), dict(c=65), dict(splits=-1)):
            assert lib.fn_metrics_scratch_bytes(C.byref(_descriptor(_lib, **bad)), 0) == _lib.FN_EINVAL, bad
            assert entry(C.byref(_descriptor(_lib, **bad)), None) == _lib.FN_EINVAL, bad
        assert entry(C.byref(_descriptor(_lib)), None) == _lib.FN_EINVAL and b"null" in lib.fn_last_error()
        fake = dict(pred=1 << 20, label=1 << 21, out=1 << 22, scratch=1 << 23)                   # never dereferenced on the host
        need = lib.fn_metrics_scratch_bytes(C.byref(_descriptor(_lib)), int(entry is lib.fn_regression_sums_f32))
        assert need > 0
        assert entry(C.byref(_descriptor(_lib, **fake, scratch_bytes=need - 1)), None) == _lib.FN_EINVAL and b"scratch" in lib.fn_last_error()
        assert entry(C.byref(_descriptor(_lib, **dict(fake, scratch=None), scratch_bytes=need)), None) == _lib.FN_EINVAL
        assert entry(C.byref(_descriptor(_lib, **dict(fake, out=(1 << 22) + 4), scratch_bytes=need)), None) == _lib.FN_EINVAL
        assert b"misaligned" in lib.fn_last_error()
        assert entry(C.byref(_descriptor(_lib, **dict(fake, pred=(1 << 20) + 2), scratch_bytes=need)), None) == _lib.FN_EINVAL


def test_ops_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from fragnet_amd import _lib, ops
    p, y = torch.zeros(5, 2), torch.zeros(5, 2)
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        ops.pair_concordance(p, y, -0.5)
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        ops.regression_sums(p, y)


def test_trainers_have_the_device_methods():
    from fragnet_amd import train
    for cls in (train.TrainerFineTune, train.TrainerFineTuneCDRP, train.TrainerFineTuneDTA):
        assert callable(getattr(cls, "evaluate")) and callable(getattr(cls, "test_on_device"))
    assert train.TrainerFineTune()._eval_norm(2.0, 3.0) == (0.0, 1.0)
    assert train.TrainerFineTuneCDRP()._eval_norm(2.0, 3.0) == (0.0, 1.0)
    assert train.TrainerFineTuneDTA()._eval_norm(2.0, 3.0) == (2.0, 3.0)
