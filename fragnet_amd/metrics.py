"""Evaluation metrics from the device's raw tables (csrc/metrics.hip through ``ops.pair_concordance`` / ``ops.regression_sums``).

The kernels leave two small tables per evaluation: exact integer pair counts [c, 5] and fp64 sums [c, 8].  Everything here runs on
the host in float64 AFTER the one device-to-host copy of those tables:

  roc_auc / concordance_index   (n_conc + n_tied / 2) / n_pairs per column -- ROC-AUC is the concordance index on binary labels.  A
                                column without a pair (one class only, nothing valid) is NaN and is left out of the mean, as
                                ``TrainerFineTune.test`` leaves it out; the mean is NaN when no column remains.
  mse, rmse, mae, pearson, r2   from the sums.
  A non-zero n_nan raises, naming the column (sklearn refuses NaN input too).

``reference_counts`` / ``reference_sums`` are plain numpy statements of what the kernels compute -- an O(n^2) broadcast compare with
integer sums, and ``math.fsum`` -- for the tests and for callers without a GPU.
"""
from __future__ import annotations

import math

import numpy as np

CONC_FIELDS = ("n_valid", "n_nan", "n_pairs", "n_conc", "n_tied")
SUMS_FIELDS = ("n", "sum_y", "sum_p", "sum_y2", "sum_p2", "sum_yp", "sum_sq_err", "sum_abs_err")
CLSF_LABEL_FLOOR = -0.5       # the classification targets mark a missing label with -1 (train.compute_bce_loss: target > -0.5)


def _table(t, fields, dtype):
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    t = np.asarray(t)
    if t.ndim != 2 or t.shape[1] != len(fields):
        raise ValueError(f"expected a [c, {len(fields)}] table ({', '.join(fields)}), got shape {t.shape}")
    return t.astype(dtype)


# ------------------------------------------------------------------------------------ from the count table
def concordance_per_column(counts) -> np.ndarray:
    """float64 [c]: (n_conc + n_tied / 2) / n_pairs, NaN where a column has no pair.  Raises when a valid row's prediction was NaN."""
    t = _table(counts, CONC_FIELDS, np.int64)
    bad = np.nonzero(t[:, 1])[0]
    if bad.size:
        raise ValueError(f"column {int(bad[0])}: {int(t[bad[0], 1])} of {int(t[bad[0], 0])} valid rows have a NaN prediction")
    out = np.full(t.shape[0], np.nan)
    for k, (_, _, pairs, conc, tied) in enumerate(t.tolist()):
        if pairs:
            out[k] = (2 * conc + tied) / (2 * pairs)      # exact integers, one rounding
    return out


def _mean_defined(per_column: np.ndarray) -> float:
    ok = ~np.isnan(per_column)
    return float(per_column[ok].mean()) if ok.any() else float("nan")


def roc_auc(counts) -> float:
    """Mean ROC-AUC over the columns that have both classes (NaN when none has)."""
    return _mean_defined(concordance_per_column(counts))


def concordance_index(counts) -> float:
    """Mean concordance index over the columns with at least one pair of distinct labels: of the ordered pairs with
    label_i > label_j, the share with pred_i > pred_j, ties in the prediction counting one half."""
    return _mean_defined(concordance_per_column(counts))


# ------------------------------------------------------------------------------------ from the sums table
def regression_metrics(sums) -> dict:
    """``mse``, ``rmse``, ``mae``, ``pearson``, ``r2``: float64 [c] each, NaN where a column has no valid row (``pearson`` / ``r2``
    also where a variance is zero)."""
    t = _table(sums, SUMS_FIELDS, np.float64)
    n, sy, sp, sy2, sp2, syp, sse, sae = t.T
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = sse / n
        var_y, var_p, cov = sy2 - sy * sy / n, sp2 - sp * sp / n, syp - sy * sp / n
        pearson = np.where((var_y > 0) & (var_p > 0), cov / np.sqrt(var_y * var_p), np.nan)
        r2 = np.where(var_y > 0, 1.0 - sse / var_y, np.nan)
        return {"mse": mse, "rmse": np.sqrt(mse), "mae": sae / n, "pearson": pearson, "r2": r2}


# ------------------------------------------------------------------------------------ numpy references
def _columns(pred, label):
    pred, label = np.asarray(pred, dtype=np.float32), np.asarray(label, dtype=np.float32)
    if pred.ndim == 1:
        pred, label = pred[:, None], label[:, None]
    if pred.ndim != 2 or pred.shape != label.shape:
        raise ValueError(f"pred and label must be [n] or [n, c] of one shape, got {pred.shape} and {label.shape}")
    return pred, label


def reference_counts(pred, label, label_floor=-np.inf) -> np.ndarray:
    """int64 [c, 5], the fields in ``CONC_FIELDS`` order: what fn_pair_concordance_f32 counts, as an O(n^2) broadcast compare of the
    float32 values with integer sums."""
    pred, label = _columns(pred, label)
    out = np.zeros((pred.shape[1], len(CONC_FIELDS)), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for k in range(pred.shape[1]):
            valid = label[:, k] >= np.float32(label_floor)                  # False for a NaN label
            nan = valid & np.isnan(pred[:, k])
            p, y = pred[valid & ~nan, k], label[valid & ~nan, k]
            above = y[:, None] > y[None, :]
            out[k] = (valid.sum(), nan.sum(), above.sum(), (above & (p[:, None] > p[None, :])).sum(), (above & (p[:, None] == p[None, :])).sum())
    return out


def reference_sums(pred, label, label_floor=-np.inf, scale=1.0, shift=0.0) -> np.ndarray:
    """float64 [c, 8], the fields in ``SUMS_FIELDS`` order: ``math.fsum`` of the float32 inputs promoted to float64, with
    ``p = pred * float32(scale) + float32(shift)`` in float32."""
    pred, label = _columns(pred, label)
    out = np.zeros((pred.shape[1], len(SUMS_FIELDS)))
    with np.errstate(invalid="ignore"):
        for k in range(pred.shape[1]):
            valid = label[:, k] >= np.float32(label_floor)
            y = label[valid, k].astype(np.float64)
            p = (pred[valid, k] * np.float32(scale) + np.float32(shift)).astype(np.float64)
            d = y - p
            out[k] = [float(valid.sum())] + [math.fsum(v) for v in (y, p, y * y, p * p, y * p, d * d, np.abs(d))]
    return out
