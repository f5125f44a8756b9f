"""Float64 NumPy reference of greedy k-centre with the rules of csrc/kcenter.hip (include/fragnet_hip.h, fn_kcenter): the direct
squared L2 or the cosine distance, the strict update (the earlier centre keeps a tie), the total-order pick (largest ``mind``, then the
smallest row; a NaN never wins while a number is left; a row is picked once), ``radius`` and seeds -- and ``check_selection``, the
conditions a greedy selection computed in another precision has to meet against float64 distances of the same rows."""
import numpy as np

METRICS = {"l2": 0, "cosine": 1}


def rnorm(x):
    return 1.0 / np.maximum(np.sqrt((x * x).sum(-1)), 1e-12)


def distances(x, c, metric):
    """Distance of every row of ``x`` [n, d] to the one row ``c`` [d], float64."""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    if metric == 0:
        return ((x - c) ** 2).sum(1)
    return np.maximum(0.0, 1.0 - (x @ c) * (rnorm(x) * rnorm(c)))


def _argmax(mind, taken):
    """The pick rule: (row, its mind) of the untaken row with the largest mind, ties to the smaller row, NaN below every number;
    (-1, 0.0) when no row is left."""
    if taken.all():
        return -1, 0.0
    key = np.where(np.isnan(mind), -1.0, mind)
    key = np.where(taken, -2.0, key)
    row = int(np.argmax(key))                      # numpy's argmax returns the FIRST maximum
    return row, float(mind[row])


def kcenter(x, k, metric=0, first=0, seeds=None, init=None):
    """``(picked [s + k], radius [s + k + 1], mind [n], label [n])`` by ordinal, the ``s`` seeds first (picked -1, radius NaN).
    ``first``: the row of the first centre, or None for the arg-max (required with seeds or after ``init``, as the kernel's caller)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    seeds = np.zeros((0, x.shape[1])) if seeds is None else np.asarray(seeds, dtype=np.float64)
    s = seeds.shape[0]
    mind = np.full(n, np.inf) if init is None else np.asarray(init, dtype=np.float64).copy()
    label = np.full(n, -1, dtype=np.int64)
    picked, radius = np.full(s + k, -1, dtype=np.int64), np.full(s + k + 1, np.nan)
    taken = np.zeros(n, dtype=bool)

    def fold(c, t):
        d = distances(x, c, metric)
        lower = d < mind                           # strict; False for a NaN on either side
        mind[lower], label[lower] = d[lower], t

    for t in range(s):
        fold(seeds[t], t)
    for t in range(s, s + k):
        if t == s and first is not None and s == 0:
            row, r = int(first), float(mind[first])
        else:
            row, r = _argmax(mind, taken)
        picked[t], radius[t] = row, r
        fold(x[row], t)
        taken[row] = True
    if n > 0 and k > 0:
        radius[s + k] = _argmax(mind, taken)[1]
    return picked, radius, mind, label


def _close(got, want, tol):
    if np.isinf(want) or np.isinf(got):
        return got == want
    return abs(got - want) <= tol + tol * abs(want)


def check_selection(x64, picked, radius, label, tol, metric=0, seeds=None, init=None):
    """Greedy validity of a selection against float64 distances of ``x64``: for every pick t the float64 min-distance of ``picked[t]``
    to the earlier centres is >= the float64 maximum over all unpicked rows minus the tolerance, ``radius[t]`` is within the tolerance
    of it, the picks are distinct, and every row's labelled centre is within the tolerance of its nearest.  The tolerance of a value
    ``ref`` is ``tol + tol |ref|``.  Arrays by ordinal as ``kcenter`` returns them.  Returns the largest |radius - float64|."""
    x64 = np.asarray(x64, dtype=np.float64)
    n = x64.shape[0]
    seeds = np.zeros((0, x64.shape[1])) if seeds is None else np.asarray(seeds, dtype=np.float64)
    s = seeds.shape[0]
    picked, radius, label = np.asarray(picked), np.asarray(radius, dtype=np.float64), np.asarray(label)
    k = picked.shape[0] - s
    assert radius.shape == (s + k + 1,) and label.shape == (n,), (radius.shape, label.shape)
    assert (picked[:s] == -1).all() and np.isnan(radius[:s]).all(), "seed slots hold picked -1 and radius NaN"
    rows = picked[s:]
    assert ((rows >= 0) & (rows < n)).all() and len(set(rows.tolist())) == k, "picks must be distinct rows"
    start = np.full(n, np.inf) if init is None else np.asarray(init, dtype=np.float64)
    mind = start.copy()
    taken = np.zeros(n, dtype=bool)
    to_centre = np.empty((s + k, n))
    worst = 0.0
    for t in range(s + k):
        if t >= s:
            row = int(rows[t - s])
            own, best = mind[row], _argmax(mind, taken)[1]
            assert own >= best - (tol + tol * abs(best)) or (np.isinf(own) and np.isinf(best)), \
                f"pick {t}: row {row} at {own} but a row at {best} was left"
            assert _close(radius[t], own, tol), f"radius[{t}] = {radius[t]}, float64 {own}"
            if np.isfinite(own):
                worst = max(worst, abs(radius[t] - own))
            taken[row] = True
        to_centre[t] = distances(x64, seeds[t] if t < s else x64[row], metric)
        mind = np.where(to_centre[t] < mind, to_centre[t], mind)           # the strict update
    if n > 0 and k > 0:
        last = _argmax(mind, taken)[1]
        assert _close(radius[s + k], last, tol), f"radius[{s + k}] = {radius[s + k]}, float64 {last}"
    assert ((label >= -1) & (label < s + k)).all()
    own, has = start.copy(), label >= 0                                    # a row nothing lowered keeps label -1 and its start
    own[has] = to_centre[label[has], np.flatnonzero(has)]
    bad = ~(own <= mind + (tol + tol * np.abs(mind))) & ~(np.isinf(own) & np.isinf(mind))
    assert not bad.any(), f"rows {np.flatnonzero(bad)[:5]}: labelled centre at {own[bad][:5]}, nearest at {mind[bad][:5]}"
    return worst
